"""Record the plain-Python restatement's results for the hand-made bubble cases (muchsalsa_amd.synth.unitig_bubble_cases)
under tests/golden/unitigs_bubbles/: the restatement's own output as data -- the tip rounds, the bubble rounds, the counts and
the SHA-256 of both texts -- so that a change to tests/ug_bubble_oracle.py cannot pass unnoticed.
Run from the repository root: python tools/make_unitig_bubble_fixtures.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ugbubblecases as cases  # noqa: E402


def record(name, k):
    r = cases.expected(name, k)[0]
    return dict(cases.params(name, k), case=name, k=k, min_count=2, records=r["records"], windows=r["windows"],
                distinct=r["distinct"], solid=r["solid"], solid_after=r["solid_after"], rounds=[list(x) for x in r["rounds"]],
                bubble_rounds=[list(x) for x in r["bubble_rounds"]], bubble_phases=r["bubble_phases"], bubbles=r["bubbles"],
                bubble_branches=r["bubble_branches"], bubble_kmers=r["bubble_kmers"], unitigs=len(r["unitigs"]),
                unitigs_without=len(cases.plain(name, k)["unitigs"]), longest=r["longest"],
                all_sha256=hashlib.sha256(r["all"]).hexdigest(), cut_sha256=hashlib.sha256(r["cut"]).hexdigest())


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "unitigs_bubbles")
    os.makedirs(out, exist_ok=True)
    for name, k in cases.HAND_AT:
        with open(os.path.join(out, "%s_k%d.json" % (name, k)), "w") as f:
            json.dump(record(name, k), f, indent=1)
            f.write("\n")
