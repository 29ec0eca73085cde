"""Writes tests/golden/kmer_edges/cases.json: for every case of tests/kmeredgecases.py the counts that the GPU tests compare
and SHA-256 digests of the output texts, as the plain-Python restatements (tests/kf_oracle.py, tests/ug_oracle.py) give them,
as recorded data -- never from the device's output.  Prints the restatement's seconds per case.  Run from the repository root
after a deliberate change of the rules or of the cases."""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import kmeredgecases  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "kmer_edges", "cases.json")


def _sha(text):
    return hashlib.sha256(text).hexdigest()


def record(name):
    r = kmeredgecases.expected(name)
    stage, k = kmeredgecases.cases()[name][:2]
    if "error" in r:
        return {"stage": stage, "k": k, "error": list(r["error"])}
    if stage == "ug":
        return {"stage": stage, "k": k, "rounds": [list(x) for x in r["rounds"]], "unitigs": len(r["unitigs"]),
                "cycles": r["cycles"], "alone": r["alone"], "blocked": r["blocked"], "windows": r["windows"],
                "solid": r["solid"], "solid_after": r["solid_after"], "longest": r["longest"],
                "all": [len(r["all"]), _sha(r["all"])], "cut": [len(r["cut"]), _sha(r["cut"])]}
    return {"stage": stage, "k": k, "histogram_tail": [list(x) for x in r["histogram"][-5:]], "rows": len(r["histogram"]),
            "q1": r["q1"], "q3": r["q3"], "upper": r["upper"], "abundant": len(r["abundant"]), "windows": r["windows"],
            "distinct": r["distinct"], "pairs": r["pairs"], "dropped": sum(r["verdict"]),
            "out1": [len(r["out1"]), _sha(r["out1"])], "out2": [len(r["out2"]), _sha(r["out2"])]}


if __name__ == "__main__":
    out, times = {}, []
    for name in kmeredgecases.cases():
        t0 = time.perf_counter()
        out[name] = record(name)
        times.append((time.perf_counter() - t0, name))
    for t in sorted(times)[-5:]:
        print("%6.2f s  %s" % t)
    print("%d cases, all: %.1f s" % (len(out), sum(t for t, _ in times)))
    with open(PATH, "w") as f:
        rows = [" %s: %s" % (json.dumps(n), json.dumps(out[n], sort_keys=True)) for n in sorted(out)]  # a case per line
        f.write("{\n" + ",\n".join(rows) + "\n}\n")
