"""Record the plain-Python restatement's results for the hand-made unitig cases (muchsalsa_amd.synth.unitig_cases) under
tests/golden/unitigs/: the restatement's own output as data, so that a change to tests/ug_oracle.py cannot pass unnoticed.
Run from the repository root: python tools/make_unitig_fixtures.py"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ug_oracle  # noqa: E402
import ugcases  # noqa: E402

MIN_LENGTH = 100


def record(name, k):
    r = ug_oracle.run(k, ugcases.files(name), min_length=MIN_LENGTH)
    return {"case": name, "k": k, "min_count": 2, "trim": k, "min_length": MIN_LENGTH, "records": r["records"],
            "windows": r["windows"], "distinct": r["distinct"], "solid": r["solid"], "solid_after": r["solid_after"],
            "rounds": [list(x) for x in r["rounds"]], "cycles": r["cycles"], "alone": r["alone"], "blocked": r["blocked"],
            "unitigs": [[t[0], t[1], ug_oracle.kmer_text(t[2], k), t[3], t[4]] for t in r["unitigs"]],
            "all": r["all"].decode(), "cut": r["cut"].decode()}


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "unitigs")
    os.makedirs(out, exist_ok=True)
    for name in ugcases.HAND:
        for k in ugcases.KS_HAND:
            with open(os.path.join(out, "%s_k%d.json" % (name, k)), "w") as f:
                json.dump(record(name, k), f, indent=1)
                f.write("\n")
