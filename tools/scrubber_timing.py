"""Timing of the read scrubber stage (muchsalsa_amd.scrubber) at the BASELINE configs[2] shape plus its read-to-read PAF
(synth.scrubber_workload): the stage runs in a fresh process under `timeout`, then the tests' plain-Python restatement
(tests/scrub_oracle.py -- a restatement, NOT the reference script) runs on the same host and the two outputs are compared
byte for byte.  Prints one JSON object; --out also writes it to a file.

    python tools/scrubber_timing.py [--reads 100000 --read-len 10000 --anchors 500000] [--repeat 3] [--out F]

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


def note(msg):
    sys.stderr.write("[scrubber_timing] %s\n" % msg)
    sys.stderr.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=100000)
    ap.add_argument("--read-len", type=int, default=10000)
    ap.add_argument("--anchors", type=int, default=500000)
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--subset-size", type=int, default=60000)
    ap.add_argument("--repeat", type=int, default=3, help="stage runs (fresh process each); the fastest is reported")
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from muchsalsa_amd import synth
    t0 = time.perf_counter()
    anchors, ava, fa = synth.scrubber_workload(a.reads, a.read_len, a.anchors, a.seed, n_again=3000, n_strangers=1000)
    gen_s = time.perf_counter() - t0
    note("workload in %.1f s" % gen_s)
    res = {"shape": {"reads": a.reads, "read_len": a.read_len, "anchors": a.anchors, "seed": a.seed,
                     "subset_size": a.subset_size, "anchor_paf_bytes": len(anchors), "ava_paf_bytes": len(ava),
                     "reads_bytes": len(fa)},
           "generate_s": round(gen_s, 3), "runs": []}
    with tempfile.TemporaryDirectory() as d:
        pa, pv, pr, out = (os.path.join(d, n) for n in ("anchors.paf", "ava.paf", "reads.fa", "out.fa"))
        for p, data in ((pa, anchors), (pv, ava), (pr, fa)):
            with open(p, "wb") as h:
                h.write(data)
        env = dict(os.environ, PYTHONPATH=ROOT)
        for k in range(a.repeat):
            t = time.perf_counter()
            r = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, "-m", "muchsalsa_amd.scrubber",
                                pa, pr, out, pv, "--subset-size", str(a.subset_size)], cwd=ROOT, env=env,
                               capture_output=True, text=True)
            if r.returncode != 0:
                res["error"] = {"run": k, "rc": r.returncode, "stderr": r.stderr[-2000:]}
                break
            one = json.loads(r.stdout.strip().splitlines()[-1])
            one["process_s"] = round(time.perf_counter() - t, 3)
            res["runs"].append(one)
            note("run %d: %.2f s" % (k, one["seconds"]["total"]))
        if res["runs"]:
            best = min(res["runs"], key=lambda x: x["seconds"]["total"])
            s = best["seconds"]
            pairs, edges, hits, lines = best["pairs"], best["edges"], best["hits"], best["ava_lines"]
            nodes, slots, records = best["nodes"], best["interval_slots"], best["records"]
            bases, text, walked = best["bases"], best["text_bytes"], best["subset_total"]
            algo = {  # bytes the kernels must move at the least
                # pairs written and sorted once (12 B in, 12 B out), flags + positions, directed entries written and sorted
                "graph": 4 * hits + pairs * (12 + 24 + 8) + 2 * edges * (12 + 24) + 8 * nodes,
                # the lines in (28 B), directed entries written and sorted (12 B each way), every group's lines and state once
                "fold": 28 * lines + 2 * lines * (12 + 24) + 2 * lines * (12 + 12 + 12) + 4 * walked,
                # a slot written, sorted and read (8 B each time), the states read, the ranges written
                "union": slots * (8 + 16 + 8) + 2 * lines * 12 + 8 * hits + 8 * records + 24 * nodes,
                "gather": 2 * bases,
                "format": bases + text,
                "copy": text,
            }
            res["best"] = {
                "parse_s": s["parse"], "load_reads_s": s["load"], "graph_s": s["graph"], "batching_s": s["batching"],
                "fold_s": s["fold"], "union_s": s["union"], "plan_s": s["plan"], "gather_s": s["gather"],
                "format_s": s["format"], "copy_back_s": s["copy"], "write_s": s["write"], "total_s": s["total"],
                "process_s": best["process_s"], "counts": {k: v for k, v in best.items() if k not in ("seconds", "process_s")},
                "algorithmic_bytes": algo,
                "hbm_fraction": {k: (algo[k] / (s[k] * HBM_PEAK) if s[k] > 0 else None)
                                 for k in ("graph", "fold", "union", "gather", "format")},
            }
            if not a.no_oracle:
                import scrub_oracle
                note("restatement ...")
                t = time.perf_counter()
                reads = scrub_oracle.parse_fasta(fa)
                batches, _ = scrub_oracle.scrub(anchors, ava, reads, a.subset_size)
                want = scrub_oracle.text(batches)
                res["python_restatement_s"] = round(time.perf_counter() - t, 3)  # tests/scrub_oracle.py, not the reference
                with open(out, "rb") as h:
                    res["identical_to_python_restatement"] = h.read() == want
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as h:
            h.write(json.dumps(res, indent=1) + "\n")
    return 0 if res["runs"] and "error" not in res else 1


if __name__ == "__main__":
    sys.exit(main())
