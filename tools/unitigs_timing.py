"""Timing of the short-read unitig assembly (muchsalsa_amd.unitigs) on a synthetic Illumina pair
(synth.kmer_filter_workload): the stage runs in fresh processes under `timeout` (the fastest of --repeat is reported),
device steps by events -- the count (bins, extract, sort, runs, select), the neighbour bytes, every tip round, the joins, the
pointer doubling, the order (heads, sort, coverage) and the write -- beside the wall time and the host's share.  --clean
makes the input error-free and repeat-free, so that it is one chain as long as the genome: the doubling's worst case.  The
tests' plain-Python restatement (tests/ug_oracle.py -- a restatement, NOT ABySS) is timed on a smaller shape
(--oracle-genome; 0 = not at all) as orientation, not as a claim.  --diploid takes the input from synth.diploid_workload
instead (two haplotypes with a variant every 400 bases, --coverage / 2 each, one file), --bubble N runs the stage with rule 9
(bubble popping) at N and reports its fork, walk and neighbour-byte times and its rounds, --gfa with rule 10 (the unitig
graph) and reports its links, sort and text times, --wide with the keys of three and of four words switched on (k up to 128;
above k = 64 it is needed; the read length left to itself is then at least 2 k, so that the reads hold k-mers).  Prints one JSON object; --out also writes it to a file.

    python tools/unitigs_timing.py [--genome 1000000 --coverage 40 --read-len 150 -k 31] [--clean] [--diploid] [--bubble N]
                                   [--gfa] [--wide] [--repeat 3] [--out F]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
COUNT_STEPS = ("bins", "extract", "sort", "runs", "select")
DEVICE_STEPS = COUNT_STEPS + ("adjacency", "tips", "next", "doubling", "order", "write")


def note(msg):
    sys.stderr.write("[unitigs_timing] %s\n" % msg)
    sys.stderr.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=1000000)
    ap.add_argument("--coverage", type=int, default=40)
    ap.add_argument("--read-len", type=int, default=None, help="150, or 2 k above k = 75: the reads must hold k-mers")
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--clean", action="store_true", help="no repeats, no errors, no N: one chain as long as the genome")
    ap.add_argument("--diploid", action="store_true", help="two haplotypes with a variant every 400 bases (synth.diploid_workload)")
    ap.add_argument("--bubble", type=int, default=0, help="rule 9's parameter (0: off)")
    ap.add_argument("--gfa", action="store_true", help="rule 10: the unitig graph is written as well")
    ap.add_argument("--wide", action="store_true", help="k up to 128 (msgpu_ug_set_wide)")
    ap.add_argument("--repeat", type=int, default=3, help="stage runs (fresh process each); the fastest is reported")
    ap.add_argument("--oracle-genome", type=int, default=0, help="genome of the shape the restatement is timed on")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.read_len is None:
        a.read_len = max(150, 2 * a.k)
    if a.k > 64 and not a.wide:
        ap.error("k = %d needs --wide" % a.k)
    if a.read_len <= a.k:
        ap.error("reads of %d bases hold no %d-mer" % (a.read_len, a.k))
    from muchsalsa_amd import synth
    extra = dict(families=0, copies=0, error=0.0, n_frac=0.0) if a.clean else {}
    t0 = time.perf_counter()
    if a.diploid:
        fq1, fq2 = synth.diploid_workload(a.genome, 400, a.coverage // 2, a.read_len, a.seed, 0.0 if a.clean else 0.004)[0], b""
    else:
        fq1, fq2 = synth.kmer_filter_workload(a.genome, a.coverage, a.read_len, a.seed, **extra)
    gen_s = time.perf_counter() - t0
    note("workload in %.1f s" % gen_s)
    res = {"shape": {"genome": a.genome, "coverage": a.coverage, "read_len": a.read_len, "k": a.k, "seed": a.seed,
                     "clean": a.clean, "diploid": a.diploid, "bubble": a.bubble, "wide": a.wide, "bytes": [len(fq1), len(fq2)]}, "generate_s": round(gen_s, 3), "runs": []}
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, n) for n in ("in_1.fq", "in_2.fq", "all.fa", "cut.fa")]
        for p, data in zip(paths, (fq1, fq2)):
            with open(p, "wb") as h:
                h.write(data)
        del fq1, fq2
        env = dict(os.environ, PYTHONPATH=ROOT)
        for i in range(a.repeat):
            t = time.perf_counter()
            r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, "-m", "muchsalsa_amd.unitigs", str(a.k)] +
                               paths + ["--bubble", str(a.bubble)] + (["--gfa", os.path.join(d, "graph.gfa")] if a.gfa else []) +
                               (["--wide"] if a.wide else []), cwd=ROOT, env=env, capture_output=True, text=True)
            if r.returncode != 0:
                res["error"] = {"run": i, "rc": r.returncode, "stderr": r.stderr[-2000:]}
                break
            one = json.loads(r.stdout.strip().splitlines()[-1])
            one["process_s"] = round(time.perf_counter() - t, 3)
            res["runs"].append(one)
            note("run %d: %.2f s" % (i, one["seconds"]["total"]))
    if res["runs"]:
        best = min(res["runs"], key=lambda x: x["seconds"]["total"])
        s = best["seconds"]
        dev = sum(s[x] for x in DEVICE_STEPS)
        count = sum(s[x] for x in COUNT_STEPS)
        host = s["load"] + s["copy"] + s["host"] + s["files"]  # file read + upload, copy back, headers and cut text, write
        res["best"] = {
            "seconds": s, "process_s": best["process_s"],
            "counts": {x: v for x, v in best.items() if x not in ("seconds", "process_s", "round_seconds")},
            "rounds": [{"limit": l, "removed": n, "tips_s": t, "adjacency_s": b}
                       for (l, n), (t, b) in zip(best["rounds"], best["round_seconds"])],
            "bubble_steps_s": {x: s[x] for x in ("bubble_forks", "bubble_walk", "bubble_adjacency")},
            "graph_steps_s": {x: s[x] for x in ("graph_links", "graph_sort", "graph_text") if x in s},
            "device_steps_s": round(dev, 5), "count_step_s": round(count, 5),
            "count_share_of_device_steps": round(count / dev, 4) if dev else None,
            "doubling_s_per_round": round(s["doubling"] / best["doubling_rounds"], 6) if best["doubling_rounds"] else None,
            "host_s": round(host, 4), "host_share_of_stage": round(host / s["total"], 4),
            "bases_per_s": round(sum(best["records"]) * a.read_len / s["total"]),
        }
    if a.oracle_genome and "error" not in res:
        import ug_oracle
        small = synth.kmer_filter_workload(a.oracle_genome, a.coverage, a.read_len, a.seed, **extra)
        note("restatement on %d bases ..." % (a.oracle_genome * a.coverage))
        t = time.perf_counter()
        want = ug_oracle.run(a.k, list(small))
        res["python_restatement"] = {"genome": a.oracle_genome, "bases": a.oracle_genome * a.coverage,  # tests/ug_oracle.py
                                     "seconds": round(time.perf_counter() - t, 3), "unitigs": len(want["unitigs"]),
                                     "solid_after": want["solid_after"]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as h:
            h.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["runs"] and "error" not in res else 1


if __name__ == "__main__":
    sys.exit(main())
