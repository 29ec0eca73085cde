"""Timing of the k-mer abundance filter stage (muchsalsa_amd.kmer_filter) on a synthetic Illumina pair of at least 10^9
bases (synth.kmer_filter_workload): the stage runs in fresh processes under `timeout` (the fastest of --repeat is
reported), device steps by events; then one more process runs the stage alternately with one partition and with a budget
that forces four, on the same files.  The tests' plain-Python restatement (tests/kf_oracle.py -- a restatement, NOT the
reference's tools) is timed on a smaller shape (--oracle-genome; 0 = not at all): at 10^9 bases it is not bearable.
Prints one JSON object; --out also writes it to a file.

    python tools/kmer_filter_timing.py [--genome 25000000 --coverage 40 --read-len 150 -k 31] [--repeat 3] [--out F]

Algorithmic bytes per device step (what the kernels must move at the least) and their share of the HBM peak (8 TB/s) are
derived from the stage's counts and event times."""
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
HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E
DEVICE_STEPS = ("bins", "extract", "sort", "runs", "hist", "select", "verdict", "output")


def note(msg):
    sys.stderr.write("[kmer_filter_timing] %s\n" % msg)
    sys.stderr.flush()


def alternate(k, paths, rounds):
    """child mode: the stage with one partition and with four, alternated in this process; prints one JSON line"""
    from muchsalsa_amd import kmer_filter
    out = {"one": [], "four": []}
    per_key = 20 if k <= 32 else 36
    slack = 1.03
    for _ in range(rounds):
        t = {}
        r = kmer_filter.run(k, *paths, timings=t)
        out["one"].append({"partitions": r["partitions"], "seconds": t})
        for _ in range(6):  # a budget just above a quarter of the windows; the stage says how many partitions it made
            t = {}
            r4 = kmer_filter.run(k, *paths, timings=t, budget_mb=slack * per_key * r["windows"] / 4 / (1 << 20))
            if r4["partitions"] <= 4:
                break
            slack *= 1.03
        out["four"].append({"partitions": r4["partitions"], "seconds": t})
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=25000000)
    ap.add_argument("--coverage", type=int, default=40)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("-k", type=int, default=31)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3, help="stage runs (fresh process each); the fastest is reported")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of the one / four partitions comparison (0: skip it)")
    ap.add_argument("--oracle-genome", type=int, default=1000000, help="genome of the shape the restatement is timed on")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--out")
    ap.add_argument("--alternate", nargs=5, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.alternate:
        alternate(a.k, a.alternate, a.rounds)
        return 0
    from muchsalsa_amd import synth
    t0 = time.perf_counter()
    fq1, fq2 = synth.kmer_filter_workload(a.genome, a.coverage, a.read_len, a.seed)
    gen_s = time.perf_counter() - t0
    note("workload in %.1f s" % gen_s)
    res = {"shape": {"genome": a.genome, "coverage": a.coverage, "read_len": a.read_len, "k": a.k, "seed": a.seed,
                     "bytes": [len(fq1), len(fq2)]}, "generate_s": round(gen_s, 3), "runs": []}
    with tempfile.TemporaryDirectory() as d:
        paths = [os.path.join(d, n) for n in ("in_1.fq", "in_2.fq", "report.txt", "out_1.fq", "out_2.fq")]
        for p, data in zip(paths, (fq1, fq2)):
            with open(p, "wb") as h:
                h.write(data)
        del fq1, fq2
        env = dict(os.environ, PYTHONPATH=ROOT)
        for i in range(a.repeat):
            t = time.perf_counter()
            r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, "-m", "muchsalsa_amd.kmer_filter",
                                str(a.k)] + paths, cwd=ROOT, env=env, capture_output=True, text=True)
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
            kb = 8 if a.k <= 32 else 16
            bases = sum(best["bytes_in"])  # every pass over the reads touches the whole files' sequence and index lines
            W, D, C, P = best["windows"], best["distinct"], best["candidates"], best["partitions"]
            passes = (2 * a.k + 7) // 8  # radix passes of 8 bits over bits [0, 2k)
            algo = {  # bytes the kernels must move at the least
                "bins": bases // 2,                       # the sequence lines once
                "extract": P * bases // 2 + W * kb,       # the sequence lines once per partition, every key written
                "sort": W * kb * 2 * passes,              # every key read and written per pass
                "runs": W * kb + D * (kb + 4),            # keys read, (key, count) written
                "hist": D * 4,
                "select": D * (kb + 4) + C * (kb + 4),    # runs read, candidates written (the abundant set is small beside it)
                "verdict": bases // 2,                    # the sequence lines once (plus table probes, mostly cached)
                "output": sum(best["bytes_in"]) + sum(best["bytes_out"]),
            }
            dev = sum(s[x] for x in DEVICE_STEPS)
            count = sum(s[x] for x in ("extract", "sort", "runs", "hist", "select"))
            host = s["load"] + s["copy"] + s["write"]
            res["best"] = {
                "seconds": s, "process_s": best["process_s"],
                "counts": {x: v for x, v in best.items() if x not in ("seconds", "process_s")},
                "algorithmic_bytes": algo,
                "hbm_fraction": {x: (algo[x] / (s[x] * HBM_PEAK) if s[x] > 0 else None) for x in DEVICE_STEPS},
                "device_steps_s": round(dev, 4), "count_step_s": round(count, 4),
                "sort_share_of_count_step": round(s["sort"] / count, 4) if count else None,
                "host_s": round(host, 4),  # file read + upload, copy back, write
                "host_share_of_stage": round(host / s["total"], 4),
                "bases_per_s": round(2 * best["pairs_in"] * a.read_len / s["total"]),
            }
            if a.rounds and "error" not in res:
                r = subprocess.run(["timeout", "-k", "10", str(2 * a.rounds * a.timeout), sys.executable, os.path.abspath(__file__),
                                    "-k", str(a.k), "--rounds", str(a.rounds), "--alternate"] + paths, cwd=ROOT, env=env,
                                   capture_output=True, text=True)
                if r.returncode != 0:
                    res["error"] = {"run": "alternate", "rc": r.returncode, "stderr": r.stderr[-2000:]}
                else:
                    alt = json.loads(r.stdout.strip().splitlines()[-1])
                    steps = ("bins", "extract", "sort", "runs", "hist", "select")
                    res["partitions_one_against_four"] = {
                        name: {"partitions": [x["partitions"] for x in alt[name]],
                               "count_step_s": [round(sum(x["seconds"][y] for y in steps[1:]), 4) for x in alt[name]],
                               "steps_s": [{y: round(x["seconds"][y], 4) for y in steps} for x in alt[name]]}
                        for name in ("one", "four")}
    if a.oracle_genome and "error" not in res:
        import kf_oracle
        small = synth.kmer_filter_workload(a.oracle_genome, a.coverage, a.read_len, a.seed)
        note("restatement on %d bases ..." % (a.oracle_genome * a.coverage))
        t = time.perf_counter()
        want = kf_oracle.run(a.k, small[0], small[1])
        res["python_restatement"] = {"genome": a.oracle_genome, "bases": a.oracle_genome * a.coverage,  # tests/kf_oracle.py
                                     "seconds": round(time.perf_counter() - t, 3), "upper": want["upper"],
                                     "abundant": len(want["abundant"])}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as h:
            h.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["runs"] and "error" not in res else 1


if __name__ == "__main__":
    sys.exit(main())
