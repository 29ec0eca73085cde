"""Step times of the assembly evaluation (muchsalsa_amd.evaluate) on one seeded workload, for DESIGN.md section 15.

    python tools/evaluate_timing.py [--genome 5000000] [--seed 1] [--coverage 40] [--k 21] [--contigs 50] [--repeats 3] [--out DIR]

One ``synth.hybrid_workload`` genome; the "assembly" is the genome cut into ``--contigs`` records with one substitution every
20,000 bases.  A first table and run warm every kernel up; then ``--repeats`` times: a table from the two files, the run on it
(with intervals).  The times are the stage's own: device event pairs per step (msgpu_ev_tstats / msgpu_ev_stats), host wall
where the header says so.  Writes ``steps.json`` and ``steps.md`` into ``--out``; ``--render`` writes ``steps.md`` again from
the ``steps.json`` there, and nothing runs.  Needs a GPU: there is no fallback.
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def render(out, directory):
    """steps.md from what steps.json holds -> the timed runs"""
    reads, asm = out["reads"], out["assembly"]
    timed = [r for r in out["runs"] if not r["warm_up"]]
    with open(os.path.join(directory, "steps.md"), "w") as h:
        h.write("# Assembly evaluation, step times (tools/evaluate_timing.py)\n\n")
        h.write("    python tools/evaluate_timing.py --genome %d --seed %d --coverage %d --k %d --contigs %d --repeats %d\n\n" % (
            out["genome"], out["seed"], out["coverage"], out["k"], out["contigs"], len(timed)))
        h.write("genome %d, seed %d, coverage %d, k %d, %d contigs: %d read windows, %d distinct read k-mers, %d assembly windows, "
                "%d missing, %d intervals; qv %s, completeness %s\n\n" % (out["genome"], out["seed"], out["coverage"], out["k"], out["contigs"],
                                                                       reads["windows"], reads["distinct"], asm["windows"], asm["missing"],
                                                                       asm["intervals"], asm["qv"], asm["completeness"]))
        for title, key in (("table (per build)", "table_seconds"), ("run (per assembly)", "run_seconds")):
            h.write("## %s, milliseconds, %d repeats behind one warm-up\n\n| step | %s |\n|---|%s\n" % (
                title, len(timed), " | ".join("run %d" % r["repeat"] for r in timed), "---|" * len(timed)))
            for name in timed[0][key]:
                h.write("| %s | %s |\n" % (name, " | ".join("%.3f" % (1e3 * r[key][name]) for r in timed)))
            h.write("\n")
        h.write("window kernel: %s windows per second\n" % ", ".join("%.3g" % r["windows_per_second"] for r in timed))
    return timed


def main(argv):
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=5_000_000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--coverage", type=int, default=40)
    ap.add_argument("--k", type=int, default=21)
    ap.add_argument("--contigs", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ev_01"))
    ap.add_argument("--render", action="store_true", help="write steps.md again from the steps.json in --out; nothing runs")
    a = ap.parse_args(argv)
    if a.render:
        with open(os.path.join(a.out, "steps.json")) as h:
            render(json.load(h), a.out)
        return 0
    from muchsalsa_amd import evaluate, synth
    t0 = time.perf_counter()
    w = synth.hybrid_workload(a.genome, a.seed, coverage=a.coverage, n_long=1, long_len=1000)
    g = bytearray(w["genome"])
    for p in range(10_000, len(g), 20_000):
        g[p] = b"ACGT"[(b"ACGT".index(bytes([g[p]]).upper()) + 1) & 3]
    step = (len(g) + a.contigs - 1) // a.contigs
    made = time.perf_counter() - t0
    os.makedirs(a.out, exist_ok=True)
    rows = []
    with tempfile.TemporaryDirectory() as d:
        p = [os.path.join(d, n) for n in ("1.fq", "2.fq", "assembly.fa", "report.tsv", "runs.bed")]
        for path, data in zip(p, (w["illumina_1"], w["illumina_2"],
                                  b"".join(b">contig%d\n%s\n" % (i, bytes(g[s:s + step])) for i, s in enumerate(range(0, len(g), step))))):
            with open(path, "wb") as h:
                h.write(data)
        for rep in range(a.repeats + 1):  # (the first one warms up)
            timings = {}
            with evaluate.Table(a.k, p[0], p[1]) as table:
                res = evaluate.run(a.k, None, None, p[2], p[3], table=table, bed=p[4], timings=timings)
                reads = table.stats
            asm, run_s = res["assemblies"][0], timings["assemblies"][0]
            rows.append({"repeat": rep, "warm_up": rep == 0, "table_seconds": reads["seconds"], "run_seconds": run_s,
                         "windows_per_second": asm["windows"] / run_s["window"] if run_s["window"] else None})
    out = {"genome": a.genome, "seed": a.seed, "coverage": a.coverage, "k": a.k, "contigs": a.contigs, "workload_seconds": round(made, 2),
           "reads": {key: v for key, v in reads.items() if key != "seconds"}, "assembly": asm, "runs": rows}
    with open(os.path.join(a.out, "steps.json"), "w") as h:
        json.dump(out, h, indent=1)
        h.write("\n")
    timed = render(out, a.out)
    print(json.dumps({"workload_seconds": out["workload_seconds"], "assembly": asm, "timed": timed}))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
