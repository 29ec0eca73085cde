"""Writes tests/golden/hybrid/expected.json: the whole pipeline (muchsalsa_amd.hybrid) on the workload of tests/hybridcases.py,
run on the CPU with the restatements the tests hold -- kf_oracle, ug_oracle, map_oracle (four times), uf_oracle, scrub_oracle
and the oracle flow of tests/test_gpu_pipeline.py -- as recorded data: per output file its byte count and SHA-256, and the
counts the workload's conditions are stated on, which this tool asserts.  Run by hand from the repository root (a few
minutes) after a deliberate change of a stage's rules or of the workload."""
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]

import hybridcases  # noqa: E402
import kf_oracle  # noqa: E402
import map_oracle  # noqa: E402
import scrub_oracle  # noqa: E402
import uf_oracle  # noqa: E402
import ug_oracle  # noqa: E402


def accepted_table(paf):
    """the PAF as muchsalsa reads it (every line but the last, paf_loader.cpp) -> (columns for synth.accepted_rows, names)"""
    lines = paf.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    cols = [ln.split(b"\t") for ln in lines[:-1]]
    ids = {}
    num = lambda j: np.array([int(c[j]) for c in cols], np.int64)  # noqa: E731
    tab = {"qname_id": np.array([ids.setdefault((0, c[0]), len(ids)) for c in cols], np.int64), "qlen": num(1), "qstart": num(2),
           "qend": num(3), "strand": np.array([c[4] == b"+" for c in cols], bool),
           "tname_id": np.array([ids.setdefault((1, c[5]), len(ids)) for c in cols], np.int64), "tlen": num(6), "tstart": num(7),
           "tend": num(8), "nmatch": num(9)}
    return tab, {v: k[1] for k, v in ids.items()}


def assembly(exact_paf, corrected, scrubbed):
    """the oracle flow of tests/test_gpu_pipeline.py on the exact PAF -> (target, query, align texts, accepted rows, contigs)"""
    import ms_oracle_ctypes as O
    from muchsalsa_amd import synth
    from test_gpu_pipeline import oracle_flow
    O.build()
    tab, name_of = accepted_table(exact_paf)
    rows, read_names, anchor_names = synth.accepted_rows(tab)
    pairs = list(zip(rows["read_id"].tolist(), rows["anchor_id"].tolist()))
    assert len(set(pairs)) == len(pairs), "a (read, unitig) pair with two accepted rows: the flow's match table keeps one"
    reads = dict(map_oracle.parse(scrubbed, False))
    unitigs = dict(map_oracle.parse(corrected, False))
    nano = {i: reads[name_of[int(n[1:])]] for i, n in enumerate(read_names)}
    illu = {i: unitigs[name_of[int(n[1:])]] for i, n in enumerate(anchor_names)}
    res = oracle_flow(O, rows, nano, illu)
    return [b"".join(r[k] for r in res) for k in ("target_fa", "query_fa", "paf")], len(rows), len(res)


def chain():
    """-> ({output name of hybrid.output_names: bytes}, counts)"""
    wl = hybridcases.workload()
    t0 = time.time()

    def lap(what):
        print("%-28s %6.1f s" % (what, time.time() - t0), flush=True)

    kf = kf_oracle.run(hybridcases.K_FILTER, wl["illumina_1"], wl["illumina_2"])
    lap("k-mer filter")
    ug = ug_oracle.run(hybridcases.K_ASSEMBLY, [kf["out1"], kf["out2"]], min_length=500)
    lap("unitigs")
    reads = map_oracle.parse(wl["reads"], map_oracle.is_fastq_name(hybridcases.READS_NAME))
    m1 = map_oracle.run(reads, map_oracle.parse(ug["cut"], False))
    lap("unitigs -> reads")
    corrected, uf = uf_oracle.run(m1["paf"], ug["cut"])
    lap("coverage filter")
    m2 = map_oracle.run(reads, map_oracle.parse(corrected, False))
    lap("corrected unitigs -> reads")
    ava = map_oracle.run(reads, None, ava=1)
    lap("reads -> reads")
    by_name = {n.decode(): s for n, s in reads}
    batches, _ = scrub_oracle.scrub(m2["paf"], ava["paf"], by_name)
    scrubbed = scrub_oracle.text(batches)
    lap("scrubber")
    m3 = map_oracle.run(map_oracle.parse(scrubbed, False), map_oracle.parse(corrected, False), exact=1)
    lap("corrected unitigs -> scrubbed")
    (target, query, align), n_rows, contigs = assembly(m3["paf"], corrected, scrubbed)
    lap("assembly")
    out = scrub_oracle.records(scrubbed)
    changed = sum(1 for n, s in reads if out.get(n + b"_0") != scrub_oracle._wrap(s) or (n + b"_1") in out)
    files = {"report": kf["report"] + uf_oracle.report_lines(uf).encode(), "unitigs": ug["all"], "unitigs_cut": ug["cut"],
             "unitigs_paf": m1["paf"], "corrected": corrected, "corrected_paf": m2["paf"], "ava_paf": ava["paf"],
             "scrubbed": scrubbed, "exact_paf": m3["paf"], "target": target, "query": query, "align": align, "assembly": target}
    counts = {"pairs": kf["pairs"], "pairs_dropped": sum(kf["verdict"]), "threshold": kf["upper"],
              "unitigs": len(ug["unitigs"]), "unitigs_500": ug["kept"],
              "unitigs_paf_rows": len(m1["chains"]), "coverage_blocks": uf["blocks"], "coverage_outliers": uf["outliers"],
              "coverage_rescued": uf["rescued"], "coverage_filter_changes": uf["outliers"] > 0,
              "corrected_paf_rows": len(m2["chains"]), "ava_rows": len(ava["chains"]),
              "long_reads": len(reads), "reads_scrubbed": changed, "scrubbed_records": len(out),
              "exact_rows": len(m3["chains"]), "exact_rows_accepted": n_rows, "contigs": contigs,
              "contig_bases": sum(len(ln) for ln in target.split(b"\n") if not ln.startswith(b">"))}
    return files, counts


if __name__ == "__main__":
    from muchsalsa_amd import hybrid
    files, counts = chain()
    names = hybrid.output_names(hybridcases.NAME, hybridcases.READS_NAME)
    e = {"shape": hybridcases.SHAPE, "k_filter": hybridcases.K_FILTER, "k_assembly": hybridcases.K_ASSEMBLY, "name": hybridcases.NAME,
         "reads_name": hybridcases.READS_NAME, "counts": counts,
         "files": {names[key]: {"bytes": len(data), "sha256": hashlib.sha256(data).hexdigest()} for key, data in sorted(files.items())}}
    print(json.dumps(counts, indent=1))
    missed = hybridcases.conditions_missed(e)
    assert not missed, missed
    os.makedirs(os.path.dirname(hybridcases.EXPECTED), exist_ok=True)
    with open(hybridcases.EXPECTED, "w") as f:
        json.dump(e, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", hybridcases.EXPECTED)
