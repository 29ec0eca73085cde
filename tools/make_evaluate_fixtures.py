"""Writes tests/golden/evaluate/<case>.json: the results of the plain-Python restatement (tests/ev_oracle.py) on the hand-made
cases of tests/evcases.py -- records, total, spectrum, intervals, solid / found and the report text.  Data only.

    python tools/make_evaluate_fixtures.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import evcases  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "evaluate")
CASES = tuple(n for n in evcases.EDGE_CASES if n != "poly_a")  # (poly_a's two megabytes of reads are the filter's own workload)


def fixture(name):
    case, want = evcases.EDGE_CASES[name](), evcases.expected(name)
    return {"k": case["k"], "min_count": case["min_count"], "records": [list(r) for r in want["records"]],
            "total": list(want["total"]), "spectrum": sorted([c, a, n] for (c, a), n in want["spectrum"].items()),
            "intervals": [list(i) for i in want["intervals"]], "solid": want["solid"], "found": want["found"],
            "report": want["report"].decode()}


def main():
    os.makedirs(GOLD, exist_ok=True)
    for name in CASES:
        with open(os.path.join(GOLD, name + ".json"), "w") as h:
            json.dump(fixture(name), h, indent=1, sort_keys=True)
            h.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
