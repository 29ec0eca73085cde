"""Workloads and hand-made cases of the mapper's tests, shared by the host and the GPU file, the restatement's result for each
(computed once per process), and the conditions the GPU tests rely on, checked on the restatement's result alone.

A case is (name of the input, parameters); an input is (targets text, its file name, queries text or None for ava, its file
name).  The workloads map unitigs (queries) onto reads (targets), as the pipeline does."""
import functools
import os

import map_oracle

MAIN = dict(n_reads=60, read_len=3000, n_unitigs=40, seed=7)
SMALL = dict(n_reads=24, read_len=1500, n_unitigs=16, seed=5, copies=4, repeat_len=300)
TINY = dict(n_reads=6, read_len=400, n_unitigs=4, seed=3, families=0)  # for k = 4
CLEAN = dict(n_reads=40, read_len=2500, n_unitigs=30, seed=9, families=0)  # no repeats: every chain is a true placement
TILED = dict(n_reads=80, read_len=4000, n_unitigs=0, seed=11, tiled=True, unitig_len=(500, 1500), error=0.04, families=0)
WORKLOADS = {"main": MAIN, "small": SMALL, "tiny": TINY, "clean": CLEAN, "tiled": TILED}
BIG = dict(n_reads=100000, read_len=10000, n_unitigs=500000, seed=1)  # the timing tool's input (tools/mapper_timing.py)


def _g(n, seed):
    from muchsalsa_amd import synth
    return synth.genome_bases(n, seed).tobytes()


def _fa(recs):
    return b"".join(b">%s\n%s\n" % (n, s) for n, s in recs)


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> (targets FASTA, queries FASTA, parameters, what the case is made for)"""
    rc = map_oracle.revcomp
    G = _g(3000, 41)
    A, B, J1, J2 = G[0:200], G[200:400], G[400:1000], G[1000:1100]
    P, S, J = G[1100:1300], G[1300:1420], G[1420:1520]
    U, V = G[1600:1700], G[1700:1800]
    unit = G[2000:2060]
    return {
        "perfect": (_fa([(b"t", G[0:400])]), _fa([(b"q", G[100:300])]), {}, "one perfect hit; links with dx < k"),
        "reverse": (_fa([(b"t", G[0:400])]), _fa([(b"q", rc(G[100:300]))]), {}, "a reverse-strand hit"),
        "two_chains": (_fa([(b"t", A + J1 + B)]), _fa([(b"q", B + J2 + A)]), {}, "two chains in one group"),
        "cut": (_fa([(b"t", P + S + J + S)]), _fa([(b"q", P + S)]), dict(min_score=40), "a chain cut at a used anchor"),
        "one_sided": (_fa([(b"t", U + b"A" * 12 + V)]), _fa([(b"q", U + b"A" * 18 + V)]), dict(w=1, exact=1),
                      "a link with lt = 0 != lq"),
        "beyond_band": (_fa([(b"t", A + B)]), _fa([(b"q", A + J1[:200] + B)]), dict(exact=1), "a segment beyond the band"),
        "n_split": (_fa([(b"t", G[0:400])]), _fa([(b"q", G[100:200] + b"N" + G[201:300])]), dict(min_score=40),
                    "an N that splits a stretch"),
        "short_stretch": (_fa([(b"t", G[0:400])]), _fa([(b"s", G[100:118]), (b"q", G[100:300])]), {},
                          "a stretch shorter than w: the record s has 4 k-mer positions"),
        "empty_queries": (_fa([(b"t", G[0:400])]), b"", {}, "an empty query file"),
        "over_max_occ": (_fa([(b"t", A + unit * 5 + B)]), _fa([(b"q", A + unit * 5 + B)]), dict(max_occ=3),
                         "a key over max_occ"),
    }


HAND = ("perfect", "reverse", "two_chains", "cut", "one_sided", "beyond_band", "n_split", "short_stretch", "empty_queries",
        "over_max_occ")


@functools.lru_cache(maxsize=None)
def workload(name, fastq=True):
    from muchsalsa_amd import synth
    return synth.mapper_workload(fastq=fastq, **WORKLOADS[name])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (targets text, targets file name, queries text or None, queries file name)"""
    if name in HAND:
        t, q = hand_cases()[name][:2]
        return t, "t.fa", q, "q.fa"
    if name.endswith("_ava"):
        return workload(name[:-4])["reads"], "reads.fq", None, "reads.fq"
    if name.endswith("_fa"):  # FASTA targets
        wl = workload(name[:-3], fastq=False)
        return wl["reads"], "reads.fa", wl["unitigs"], "unitigs.fa"
    wl = workload(name)
    return wl["reads"], "reads.fq", wl["unitigs"], "unitigs.fa"


def write_inputs(name, directory):
    """the input's files in ``directory`` -> (targets path, queries path)"""
    t, tn, q, qn = inputs(name)
    tp, qp = os.path.join(str(directory), tn), os.path.join(str(directory), qn)
    with open(tp, "wb") as f:
        f.write(t)
    if q is not None:
        with open(qp, "wb") as f:
            f.write(q)
    return tp, qp


@functools.lru_cache(maxsize=None)
def _records(name):
    t, tn, q, qn = inputs(name)
    return (map_oracle.parse(t, map_oracle.is_fastq_name(tn)),
            None if q is None else map_oracle.parse(q, map_oracle.is_fastq_name(qn)))


@functools.lru_cache(maxsize=None)
def _expected(name, params):
    t, q = _records(name)
    return map_oracle.run(t, q, **dict(params))


def expected(name, **params):
    if name in HAND:
        params = dict(hand_cases()[name][2], **params)
    if name.endswith("_ava"):
        params["ava"] = 1
    return _expected(name, tuple(sorted(params.items())))


# what the GPU file compares byte for byte: (input, parameters)
CASES = ([("main", {}), ("main", dict(exact=1)), ("main_ava", {}), ("main", dict(max_occ=12)),
          ("clean", dict(exact=1)), ("clean", dict(exact=1, band=8)), ("tiled", dict(exact=1)),
          ("tiny", dict(k=4)), ("small", dict(k=16)), ("small", dict(k=31)), ("small", dict(k=32)), ("small", dict(k=32, exact=1)),
          ("small", dict(w=1)), ("small", dict(w=64)), ("small", dict(w=64, k=32, exact=1)),
          ("small", dict(min_score=40, min_count=10)), ("small", dict(max_gap=300)), ("small", dict(bandwidth=20)),
          ("small", dict(exact=1, band=1)), ("small", dict(exact=1, band=127)), ("small_fa", {}), ("small_fa", dict(exact=1)),
          ("small_ava", dict(exact=1))] + [(name, {}) for name in HAND])


def case_id(case):
    return case[0] + "".join("-%s%d" % kv for kv in sorted(case[1].items()))


def invariants(r, targets, queries):
    """every chain's anchors rise in x and y; matches <= block; ranges inside the records; no anchor in two chains"""
    seen = set()
    for ch, anchors in zip(r["chains"], r["notes"].get("chain_anchors", [])):
        q, t, s, n, score, nm, qs, qe, ts, te, matches, block = ch
        assert n == len(anchors) >= r["params"]["min_count"] and score >= r["params"]["min_score"]
        assert all(a[0] < b[0] and a[1] < b[1] for a, b in zip(anchors, anchors[1:]))
        assert 0 <= matches <= block and nm <= block
        assert 0 <= qs < qe <= len(queries[q][1]) and 0 <= ts < te <= len(targets[t][1])
        assert block >= max(qe - qs, te - ts)  # block = k + sum max(dx, dy) over the links
        for a in anchors:
            assert (q, t, s, a) not in seen
            seen.add((q, t, s, a))
    assert len(r["chains"]) == r["paf"].count(b"\n") == len(r["notes"].get("chain_anchors", []))
    keys = [(c[0], c[1], c[2]) for c in r["chains"]]
    assert keys == sorted(keys)
