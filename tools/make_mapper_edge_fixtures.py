"""Writes tests/golden/mapper/edges.json: for every case of tests/mapedgecases.py the counts that the GPU tests compare and
a SHA-256 of the PAF, as the mapper's plain-Python restatement (tests/map_oracle.py) gives them, as recorded data.  Prints the
restatement's seconds per case.  Run from the repository root after a deliberate change of the rules or of the cases."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import mapedgecases  # noqa: E402

KEYS = ("minimizers", "keys", "keys_dropped", "entries_dropped", "anchors", "n_groups", "groups_kept", "groups_small",
        "groups_large", "largest_group", "group_hist", "below_score", "below_count", "chains_cut", "pairs", "capped")
PATH = os.path.join(ROOT, "tests", "golden", "mapper", "edges.json")


def record(case):
    r = mapedgecases.expected(case[0], **case[1])
    out = {key: r[key] for key in KEYS}
    out.update(chains=len(r["chains"]), paf_bytes=len(r["paf"]), paf_sha256=hashlib.sha256(r["paf"]).hexdigest())
    return out


if __name__ == "__main__":
    out, times = {}, []
    for case in mapedgecases.CASES:
        t0 = time.perf_counter()
        mapedgecases.inputs(case[0])
        out[mapedgecases.case_id(case)] = record(case)
        times.append((time.perf_counter() - t0, mapedgecases.case_id(case)))
        print("%6.2f s  %s" % times[-1])
    print("slowest: %.2f s %s; all: %.1f s" % (max(times) + (sum(t for t, _ in times),)))
    with open(PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
