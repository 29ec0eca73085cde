"""Writes tests/golden/mapper/<case>.json: the results of the mapper's plain-Python restatement (tests/map_oracle.py) on the
hand-made cases of tests/mapcases.py, as recorded data.  Run from the repository root after a deliberate change of the rules."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mapcases  # noqa: E402

KEYS = ("minimizers", "keys", "keys_dropped", "entries_dropped", "anchors", "n_groups", "groups_kept", "chains_cut",
        "below_score", "below_count", "pairs", "capped")


def record(name):
    r = mapcases.expected(name)
    out = {"made_for": mapcases.hand_cases()[name][3], "params": r["params"], "paf": r["paf"].decode(),
           "chains": [list(c) for c in r["chains"]]}
    out.update({k: r[k] for k in KEYS})
    return out


if __name__ == "__main__":
    d = os.path.join(ROOT, "tests", "golden", "mapper")
    os.makedirs(d, exist_ok=True)
    for name in mapcases.HAND:
        with open(os.path.join(d, name + ".json"), "w") as f:
            json.dump(record(name), f, indent=1, sort_keys=True)
            f.write("\n")
