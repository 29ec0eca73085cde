"""Timing of the mapper (muchsalsa_amd.mapper) on the BASELINE configs[2] shape from synth.mapper_workload (100 k reads x 10 kb,
500 k unitigs, reads at a stated error rate): seed mode, exact mode, and ava on a subset of the reads.  Every run is a fresh
process under `timeout`; the fastest of --repeat is reported with its device steps by events (sketch, sort, table, anchor
expansion, grouping sorts, DP, backtrack, pairs, distances, copy), the host's formatting, the algorithmic bytes of each step
and their share of the HBM peak, and the group-size histogram.  A mode the stage itself rejects (exit status 1 with a MapError of
code -5 or -4: rule 9's limits) is recorded with its message and the next mode starts.  Anything else -- no answer in time, a time
limit's 124 / 137, an abort, a segmentation fault, a signal, any other status -- ends the tool at once with what it has:
nothing more is started on a device that may have faulted.  The tests' plain-Python restatement
(tests/map_oracle.py -- a restatement, NOT minimap2) is timed on the tests' workloads with --oracle, as orientation and not
as a claim.  Prints one JSON object; --out also writes it to a file (profiles/map_01/).

    python tools/mapper_timing.py [--reads 100000 --read-len 10000 --unitigs 500000 --error 0.06] [--ava-reads 10000]
                                  [--repeat 3] [--oracle] [--out F]
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
HBM_PEAK = 8.0e12  # bytes per second, MI355X
STEPS = ("sketch", "sort", "table", "anchors", "group", "chain", "backtrack", "pairs", "distance", "copy")


def note(msg):
    sys.stderr.write("[mapper_timing] %s\n" % msg)
    sys.stderr.flush()


def step_bytes(r):
    """what each step must read and write at least, from the run's counts"""
    p, m, a = r["params"], r["minimizers"], r["anchors"]
    both = r["bases"][0] + (0 if p["ava"] else r["bases"][1])
    n_min = m[0] + (0 if p["ava"] else m[1])
    return {"sketch": 2 * both + 16 * n_min, "sort": 2 * 16 * m[0] * ((2 * p["k"] + 7) // 8), "table": 12 * r["keys"],
            "anchors": 2 * 16 * m[1] + 16 * a, "group": 2 * 2 * 16 * a * 8 + 16 * a, "chain": 8 * a + 16 * a,
            "backtrack": 2 * 8 * a * 8 + 25 * a, "pairs": (4 * r["bases"][1] if p["exact"] else 0) + 24 * r["pairs"],
            "distance": 28 * r["pairs"], "copy": 48 * r["chains"]}


class Stop(Exception):
    """a run ended in a way after which nothing more may start on the device"""


def stage(args, repeat, limit, env):
    """-> the fastest run's report, or {"rejected": message} when the stage refused the input; raises Stop otherwise"""
    best = None
    for i in range(repeat):
        t = time.perf_counter()
        try:
            out = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, "-m", "muchsalsa_amd.mapper"] + args, cwd=ROOT,
                                 env=env, capture_output=True, timeout=limit + 30)
        except subprocess.TimeoutExpired:
            raise Stop("no answer in %d s" % limit)
        last = out.stderr.decode(errors="replace").strip().splitlines()[-1:]
        if out.returncode == 1 and last and "MapError" in last[0] and ("(-5)" in last[0] or "(-4)" in last[0]):  # argument, memory
            return {"rejected": last[0]}
        if out.returncode != 0:
            raise Stop("exit status %d: %s" % (out.returncode, " ".join(last)))
        r = json.loads(out.stdout.decode().strip().splitlines()[-1])
        r["process_s"] = round(time.perf_counter() - t, 3)
        note("run %d: stage wall %.3f s" % (i, r["seconds"]["stage_wall"]))
        if best is None or r["seconds"]["stage_wall"] < best["seconds"]["stage_wall"]:
            best = r
    dev = sum(best["seconds"][s] for s in STEPS)
    by = step_bytes(best)
    best["steps"] = {s: {"seconds": best["seconds"][s], "share_of_device": round(best["seconds"][s] / dev, 4) if dev else 0.0,
                         "bytes": by[s],
                         "share_of_hbm_peak": round(by[s] / best["seconds"][s] / HBM_PEAK, 4) if best["seconds"][s] > 0 else None}
                     for s in STEPS}
    best["device_s"] = round(dev, 6)
    best["host_format_share_of_wall"] = round(best["seconds"]["host"] / best["seconds"]["stage_wall"], 4)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--unitigs", type=int, default=500000)
    ap.add_argument("--error", type=float, default=0.06)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--ava-reads", type=int, default=10000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--oracle", action="store_true", help="time the restatement on the tests' workloads")
    ap.add_argument("--out")
    a = ap.parse_args()
    from muchsalsa_amd import synth
    t0 = time.perf_counter()
    wl = synth.mapper_workload(a.reads, a.read_len, a.unitigs, a.seed, error=a.error)
    res = {"shape": {"reads": a.reads, "read_len": a.read_len, "unitigs": a.unitigs, "error": a.error, "seed": a.seed,
                     "bytes": [len(wl["reads"]), len(wl["unitigs"])]}, "generate_s": round(time.perf_counter() - t0, 3)}
    note("workload in %.1f s" % res["generate_s"])
    env = dict(os.environ, PYTHONPATH=ROOT)
    with tempfile.TemporaryDirectory() as d:
        reads, unitigs, sub, out = (os.path.join(d, n) for n in ("reads.fq", "unitigs.fa", "subset.fq", "out.paf"))
        with open(reads, "wb") as h:
            h.write(wl["reads"])
        with open(unitigs, "wb") as h:
            h.write(wl["unitigs"])
        with open(sub, "wb") as h:  # the first --ava-reads records
            at = 0
            for _ in range(4 * min(a.ava_reads, a.reads)):
                at = wl["reads"].index(b"\n", at) + 1
            h.write(wl["reads"][:at])
        del wl
        try:
            for name, args in (("seed_mode", [reads, unitigs, out]), ("exact_mode", [reads, unitigs, out, "--exact"]),
                               ("ava_subset", [sub, sub, out, "--ava"])):
                res[name] = stage(args, a.repeat, a.timeout, env)
        except Stop as e:
            res["stopped"] = "%s: %s" % (name, e)
            note("stopped: " + res["stopped"])
    if a.oracle and "stopped" not in res:
        import mapcases
        res["restatement_s"] = {}
        for case in mapcases.CASES[:7]:
            t = time.perf_counter()
            mapcases.expected(case[0], **case[1])
            res["restatement_s"][mapcases.case_id(case)] = round(time.perf_counter() - t, 2)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as h:
            h.write(text + "\n")
    return 1 if "stopped" in res else 0


if __name__ == "__main__":
    sys.exit(main())
