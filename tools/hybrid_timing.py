"""Times the whole pipeline two ways on one seeded workload of a size a user would run: the driver (muchsalsa_amd.hybrid: the
Illumina pair resident between the filter and the unitigs, one index of the long reads for three mappings) and the chain of
the same stages by files (eight calls, the filtered FASTQ files written and read again, three index builds).  The two
alternate, RUNS times each, every run in a fresh child process.  Prints one JSON line: per run the per-stage wall seconds
(every stage call ends in a device synchronise) and the stages' own event times, then medians and spread per stage.

    python tools/hybrid_timing.py <workdir> [--genome N=5000000] [--coverage N=40] [--long-coverage N=10] [--long-len N=10000]
            [--runs N=3] [--seed N=1]

The workload is generated once into <workdir>.  Keep what it prints under profiles/hy_01/ (DESIGN.md section 13)."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K_FILTER, K_ASSEMBLY, NAME = 21, 31, "hy"


def by_files(inputs, out):
    """the parent's offer: every hand-off a file -> {stage: {"seconds": wall, "events": the stage's own times}}"""
    from muchsalsa_amd import kmer_filter, mapper, pipeline, scrubber, unitig_filter, unitigs
    os.makedirs(os.path.join(out, "asm"), exist_ok=True)
    p = {k: os.path.join(out, k) for k in ("report.txt", "f1.fq", "f2.fq", "all.fa", "cut.fa", "u.paf", "corrected.fa", "c.paf", "ava.paf",
                                          "scrubbed.fa", "exact.paf")}
    res = {}

    def stage(key, fn, *args, **kw):
        t0, ev = time.perf_counter(), {}
        fn(*args, timings=ev, **kw)
        res[key] = {"seconds": round(time.perf_counter() - t0, 4), "events": {k: v for k, v in ev.items() if isinstance(v, float)}}

    stage("filter", kmer_filter.run, K_FILTER, inputs[0], inputs[1], p["report.txt"], p["f1.fq"], p["f2.fq"])
    stage("unitigs", unitigs.run, K_ASSEMBLY, p["f1.fq"], p["f2.fq"], p["all.fa"], p["cut.fa"], min_length=500)
    stage("map_unitigs", mapper.run, inputs[2], p["cut.fa"], p["u.paf"])
    stage("unitig_filter", unitig_filter.run, p["u.paf"], p["cut.fa"], p["report.txt"], p["corrected.fa"])
    stage("map_corrected", mapper.run, inputs[2], p["corrected.fa"], p["c.paf"])
    stage("ava", mapper.run, inputs[2], inputs[2], p["ava.paf"], ava=1)
    stage("scrubber", scrubber.run, p["c.paf"], inputs[2], p["scrubbed.fa"], p["ava.paf"])
    stage("map_exact", mapper.run, p["scrubbed.fa"], p["corrected.fa"], p["exact.paf"], exact=1)
    stage("assembly", pipeline.run, p["exact.paf"], p["corrected.fa"], p["scrubbed.fa"], os.path.join(out, "asm"))
    return res


def child(which, workdir, run):
    from muchsalsa_amd import _lib, hybrid
    _lib.PRELOAD_TORCH = False
    inputs = [os.path.join(workdir, n) for n in ("illumina_1.fq", "illumina_2.fq", "nanopore.fastq")]
    out = os.path.join(workdir, "%s_%d" % (which, run))
    t0 = time.perf_counter()
    if which == "driver":
        r = hybrid.run(K_FILTER, K_ASSEMBLY, NAME, inputs[0], inputs[1], inputs[2], out)
        stages = {k: {"seconds": v["seconds"]} for k, v in r.items() if isinstance(v, dict) and "seconds" in v}
        stages["index"]["events"] = r["index"]["seconds_of_build"]
    else:
        stages = by_files(inputs, out)
    print(json.dumps({"which": which, "run": run, "total": round(time.perf_counter() - t0, 4), "stages": stages}))


def main(argv):
    args = list(argv)
    if len(args) >= 4 and args[0] == "--child":
        child(args[1], args[2], int(args[3]))
        return 0
    opts = {"--genome": 5000000, "--coverage": 40, "--long-coverage": 10, "--long-len": 10000, "--runs": 3, "--seed": 1}
    for name in opts:
        if name in args:
            i = args.index(name)
            opts[name] = int(args[i + 1])
            del args[i:i + 2]
    if len(args) != 1:
        sys.stderr.write(__doc__.split("\n\n")[1] + "\n")
        return 2
    workdir = os.path.abspath(args[0])
    os.makedirs(workdir, exist_ok=True)
    from muchsalsa_amd import synth
    paths = [os.path.join(workdir, n) for n in ("illumina_1.fq", "illumina_2.fq", "nanopore.fastq")]
    if not all(os.path.exists(p) for p in paths):
        G, L = opts["--genome"], opts["--long-len"]
        wl = synth.hybrid_workload(G, opts["--seed"], coverage=opts["--coverage"], n_long=max(1, G * opts["--long-coverage"] // L),
                                   long_len=L, families=6, copies=25, repeat_len=1500)
        for p, key in zip(paths, ("illumina_1", "illumina_2", "reads")):
            with open(p, "wb") as h:
                h.write(wl[key])
    runs = []
    for run in range(opts["--runs"]):
        for which in ("driver", "files"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, workdir, str(run)], capture_output=True,
                               text=True, cwd=ROOT)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                return 1
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
    summary = {}
    for which in ("driver", "files"):
        mine = [r for r in runs if r["which"] == which]
        keys = ["total"] + list(mine[0]["stages"])
        value = lambda r, k: r["total"] if k == "total" else r["stages"][k]["seconds"]  # noqa: E731
        summary[which] = {k: {"median": statistics.median(value(r, k) for r in mine), "min": min(value(r, k) for r in mine),
                              "max": max(value(r, k) for r in mine)} for k in keys}
    print(json.dumps({"workload": {k[2:]: v for k, v in opts.items()}, "bytes": [os.path.getsize(p) for p in paths], "runs": runs,
                      "summary": summary}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
