"""Read scrubber, host side (no GPU): the plain-Python restatement (tests/scrub_oracle.py) against the record sets the
reference script wrote for the small fixtures (tests/golden/scrubber, tools/make_scrubber_fixtures.py), msgpu_scrub_parse
against the restatement's reading of both PAFs, its rejections with line and file, and the batching (start choice, discovery
order, centre) of both the restatement and msgpu_scrub_plan_create on hand-made graphs."""
import hashlib
import json
import os

import numpy as np
import pytest

import scrub_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "scrubber")


@pytest.fixture(scope="module")
def sc():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import scrubber
    return scrubber


def _read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def _sorted(text):
    recs = scrub_oracle.records(text)
    return b"".join(b">" + h + b"\n" + recs[h] for h in sorted(recs)), len(recs)


@pytest.mark.parametrize("fx", ["a", "b"])
def test_oracle_gives_the_scripts_record_set(fx):
    meta = json.loads(_read(fx + ".json"))
    reads = scrub_oracle.parse_fasta(_read(fx + ".reads.fa"))
    batches, st = scrub_oracle.scrub(_read(fx + ".anchors.paf"), _read(fx + ".ava.paf"), reads, meta["subset_size"])
    got, n = _sorted(scrub_oracle.text(batches))
    assert (n, st["nodes"], st["edges"], st["batches"]) == (meta["records"], meta["nodes"], meta["edges"], meta["batches"])
    assert got == _read(fx + ".out.sorted.fa")
    assert hashlib.sha256(got).hexdigest() == meta["sha256_sorted"]


def test_fixtures_are_regenerated_by_seed():
    from muchsalsa_amd import synth
    for fx in ("a", "b"):
        meta = json.loads(_read(fx + ".json"))
        anchors, ava, fa = synth.scrubber_workload(**meta["shape"])
        assert (anchors, ava, fa) == (_read(fx + ".anchors.paf"), _read(fx + ".ava.paf"), _read(fx + ".reads.fa"))


def test_workload_has_what_the_rules_need():
    from muchsalsa_amd import synth
    anchors, ava, fa = synth.scrubber_workload(300, 4000, 900, 5)
    rows = [ln.split("\t") for ln in anchors.decode().splitlines()]
    assert any(int(r[3]) - int(r[2]) < 500 for r in rows)                      # hits the scrubber skips
    seen, repeats, came_back, prev, closed = set(), 0, 0, None, set()
    for r in rows:
        if int(r[3]) - int(r[2]) < 500:
            continue
        repeats += (r[5], r[0]) in seen
        if (r[5], r[0]) not in seen:
            if r[0] != prev:
                came_back += r[0] in closed
                closed.add(prev)
                prev = r[0]
        seen.add((r[5], r[0]))
    assert repeats > 10 and came_back > 10
    g = scrub_oracle.read_graph(anchors)
    lines = [ln.split("\t") for ln in ava.decode().splitlines()]
    assert any(t[0] not in g["node"] or t[5] not in g["node"] for t in lines) and any(t[0] == t[5] for t in lines)
    by_pair = {}
    for t in lines:
        by_pair.setdefault((t[0], t[5]), []).append(t)
    multi = [v for v in by_pair.values() if len(v) > 1]
    assert any(len(v) == 3 for v in multi) and any(len({t[4] for t in v}) == 2 for v in multi)
    gaps = set()
    for v in multi:
        v = sorted(v, key=lambda t: int(t[2]))
        gaps.update(int(b[2]) - int(a[3]) for a, b in zip(v, v[1:]))
    assert {50, 300, 499, 500, 700, 1500} <= gaps
    batches, _ = scrub_oracle.scrub(anchors, ava, scrub_oracle.parse_fasta(fa))
    assert sum(1 for h, _ in batches[0] if h.endswith(b"_1")) > 20            # reads with an uncovered middle


def _check_parse(sc, tmp_path, anchors, ava):
    pa, pv = tmp_path / "a.paf", tmp_path / "v.paf"
    pa.write_bytes(anchors)
    pv.write_bytes(ava)
    with sc.ScrubPaf(str(pa), str(pv)) as h:
        t = h.tables()
        order = h.name_order()
    g = scrub_oracle.read_graph(anchors)
    assert t["nodes"] == g["names"]
    assert t["node_length"].tolist() == g["length"]
    assert (t["node_line"] + 1).tolist() == g["line"]
    assert len(t["hit_node"]) == g["hits"] and len(t["chunk_first"]) == g["chunks"]
    # the counting lines: per node its first hit of every anchor, in line order
    per_node = [[] for _ in g["names"]]
    for v, s, e in zip(t["hit_node"].tolist(), t["hit_s"].tolist(), t["hit_e"].tolist()):
        per_node[v].append((s, e))
    assert per_node == [list(a.values()) for a in g["anchors"]]
    assert t["chunk_first"].tolist() == (np.cumsum(t["chunk_n"]) - t["chunk_n"]).tolist()
    # the chunks give the restatement's graph: every line joins its read to those already in the chunk
    adj = [[] for _ in g["names"]]
    for f, n in zip(t["chunk_first"].tolist(), t["chunk_n"].tolist()):
        nodes = t["hit_node"][f:f + n].tolist()
        assert len(set(t["hit_anchor"][f:f + n].tolist())) == 1 and len(set(nodes)) == n
        for j in range(n):
            for i in range(j):
                if nodes[j] not in adj[nodes[i]]:
                    adj[nodes[i]].append(nodes[j])
                    adj[nodes[j]].append(nodes[i])
    assert adj == g["adj"]
    want = scrub_oracle.ava_lines(ava, g["node"])
    strands = {"+": 0, "-": 1}
    for w in want:
        strands.setdefault(w[4], len(strands))
    got = list(zip(t["ava_a"].tolist(), t["ava_b"].tolist(), t["ava_sa"].tolist(), t["ava_ea"].tolist(),
                   t["ava_strand"].tolist(), t["ava_sb"].tolist(), t["ava_eb"].tolist()))
    assert got == [(a, b, s1, e1, strands[d], s2, e2) for (a, b, s1, e1, d, s2, e2) in want]
    assert order.tolist() == sorted(range(len(g["names"])), key=lambda i: g["names"][i].encode())
    return t, g


def test_parse_matches_the_restatement(sc, tmp_path):
    from muchsalsa_amd import synth
    anchors, ava, _ = synth.scrubber_workload(300, 4000, 900, 5)
    for threads in ("1", "3", "7"):
        os.environ["MSGPU_PARSE_THREADS"] = threads
        try:
            t, g = _check_parse(sc, tmp_path, anchors, ava)
        finally:
            del os.environ["MSGPU_PARSE_THREADS"]
    assert t["n_anchor_lines"] == anchors.count(b"\n") and len(t["ava_a"]) < t["n_ava_lines"]


A1 = "u1\t900\t0\t600\t+\tr1\t3000\t10\t610\t600\t600\t60\n"
A2 = "u1\t900\t0\t700\t-\tr2\t2500\t20\t720\t700\t700\t60\n"
V1 = "r1\t3000\t100\t900\t+\tr2\t2500\t0\t800\t800\t800\t60\n"


def test_parse_accepts_what_the_rules_allow(sc, tmp_path):
    # blank and one-token lines, CRLF, trailing tabs, no final newline, a short hit, an unknown strand, a negative column 6 on
    # a line that is skipped, names with spaces; read-to-read: short lines, a self hit, bad fields on lines of non-nodes
    anchors = (A1 + "\nlonely\n   \n" + A2.replace("\n", "\r\n") + "u2\t900\t0\t499\t+\tr3\t-5\t0\t499\n" +
               "u 2\t900\t5\t505\t*\tr 4\t250\t0\t500\tx\ty\t\t\n" + "u1\t900\t0\t600\t+\tr1\t1\t0\t1\n" +
               "u1\t1\t0\t500\t+\tr5\t200\t7\t8").encode()
    ava = (V1 + "one\nr1\tx\n\nr1\t3000\t0\t900\t+\tr1\t3000\t0\tbad\n" + "r1\t1\tbad\t2\t+\tghost\t1\n" +
           "ghost\t1\t0\t900\t+\tr2\n" + "r2\t1\t0\t499\t+\tr1\t1\t0\t9000\n" +
           "r 4\t1\t0\t500\tx y\tr5\t1\t3\t4\t\t\n" + "r5\t1\t10\t600\tx y\tr 4\t1\t30\t40\r\n" +
           "r2\t1\t10\t600\t\tr1\t1\t30\t40").encode()
    t, g = _check_parse(sc, tmp_path, anchors, ava)
    assert t["nodes"] == ["r1", "r2", "r 4", "r5"] and t["chunk_n"].tolist() == [2, 1, 1]
    assert t["ava_strand"].tolist() == [0, 2, 2, 3] and t["ava_line"].tolist() == [0, 8, 9, 10]


@pytest.mark.parametrize("anchors,ava,line,file", [
    ("", V1, 1, 0),                                                            # no node at all
    ("lonely\n\n", V1, 1, 0),
    ("u1\t900\t0\t499\t+\tr1\t3000\t10\t610\n", V1, 1, 0),                     # only a short hit: no node
    (A1 + "u1\t900\t0\t600\t+\tr2\t3000\t10\n", V1, 2, 0),                     # 8 fields
    (A1 + "u1\t900\n", V1, 2, 0),                                              # 2 fields
    (A1 + "u1\t900\t0\t600\t+\tr2\t3000\t10\t610\t\t\n" + "u1\t900\t0\t600\t+\tr2\t3000\t10\t\t\n", V1, 3, 0),
    (A1 + "\n" + "u1\t900\tx\t600\t+\tr2\t3000\t10\t610\n", V1, 3, 0),          # column 2
    (A1 + "u1\t900\t0\t+600\t+\tr2\t3000\t10\t610\n", V1, 2, 0),               # column 3: no sign
    (A1 + "u1\t900\t0\t400\t+\tr2\tlong\t10\t610\n", V1, 2, 0),                # column 6 is read before the span test
    (A1 + "u1\t900\t0\t600\t+\tr2\t3000\t-1\t610\n", V1, 2, 0),                # column 7: no sign
    (A1 + "u1\t900\t0\t600\t+\tr2\t3000\t10\t99999999999\n", V1, 2, 0),        # column 8: out of range
    (A1 + "\t900\t0\t600\t+\tr2\t3000\t10\t610\n", V1, 2, 0),                  # empty column 0
    (A1 + "u1\t900\t0\t600\t+\tr2\t199\t10\t610\n", V1, 2, 0),                 # the slice would end at a negative index
    (A1 + "u1\t900\t0\t600\t+\tr2\t-3000\t10\t610\n", V1, 2, 0),
    (A1 + A2, V1 + "r1\t3000\t100\t900\t+\tr2\t2500\t0\n", 2, 1),              # 8 fields, both reads are nodes
    (A1 + A2, "x\n" + V1 + "r2\t1\t1e3\t900\t+\tr1\t1\t0\t800\n", 3, 1),       # column 2
    (A1 + A2, V1 + "r2\t1\t0\t300\t+\tr1\t1\t0\t8 0\n", 2, 1),                 # column 8 is read before the span test
])
def test_parse_rejects_with_line_and_file(sc, tmp_path, anchors, ava, line, file):
    pa, pv = tmp_path / "bad.paf", tmp_path / "bad.ava.paf"
    pa.write_text(anchors)
    pv.write_text(ava)
    with pytest.raises(sc.ScrubberError) as ei:
        sc.ScrubPaf(str(pa), str(pv))
    assert (ei.value.line, ei.value.file) == (line, file)
    with pytest.raises(scrub_oracle.OracleError) as eo:
        g = scrub_oracle.read_graph(anchors.encode())
        scrub_oracle.ava_lines(ava.encode(), g["node"])
    assert (eo.value.line, eo.value.file) == (line, file)


def test_parse_missing_file(sc, tmp_path):
    pa = tmp_path / "a.paf"
    pa.write_text(A1)
    with pytest.raises(sc.ScrubberError) as ei:
        sc.ScrubPaf(str(pa), str(tmp_path / "none.paf"))
    assert ei.value.file == 1 and ei.value.line == 0


# ---- batching on hand-made graphs: both the restatement and msgpu_scrub_plan_create

def _csr(adj):
    row_off = np.zeros(len(adj) + 1, np.uint64)
    row_off[1:] = np.cumsum([len(a) for a in adj])
    return row_off, np.array([w for a in adj for w in a], np.uint32)


def _graph(n, edges):
    """adjacency lists in insertion order from an edge list"""
    adj = [[] for _ in range(n)]
    for u, v in edges:
        adj[u].append(v)
        adj[v].append(u)
    return adj


def _both(sc, names, adj, subset_size):
    want = scrub_oracle.batches(names, adj, subset_size)
    by_name = sorted(range(len(names)), key=lambda i: names[i].encode())
    got = sc.batches(by_name, *_csr(adj), subset_size=subset_size)
    assert got == [(s, list(sub), list(cen)) for s, sub, cen in want]
    return got


def test_batching_subset_fills_in_the_middle_of_a_level(sc):
    # a star: centre 0, leaves 1..6 (edges added in the order 4, 2, 6, 1, 3, 5) and a tail 6 - 7.  Names put node 0 first.
    names = ["a0", "z1", "z2", "z3", "z4", "z5", "z6", "z7"]
    adj = _graph(8, [(0, 4), (0, 2), (0, 6), (0, 1), (0, 3), (0, 5), (6, 7)])
    got = _both(sc, names, adj, 4)
    # discovery order from 0 is the insertion order of its edges: the subset fills after 4, 2, 6 -- inside level 1
    assert got[0] == (0, [0, 4, 2, 6], [2, 4])    # 0 has neighbours outside (1, 3, 5), 6 has 7; leaves 4 and 2 are inner
    # next: the smallest remaining name is a0 again; 4 and 2 are gone, so the order is 6, 1, 3 and the subset is full
    assert got[1] == (0, [0, 6, 1, 3], [1, 3])
    assert got[2] == (0, [0, 6, 5, 7], [0, 5, 6, 7])
    assert len(got) == 3


def test_batching_small_component_merges_into_the_next(sc):
    # components {0, 1} (names b, a), {2, 3, 4} path (names c, e, d), {5} (name f); subset size 4
    names = ["b", "a", "c", "e", "d", "f"]
    adj = _graph(6, [(0, 1), (2, 3), (3, 4)])
    got = _both(sc, names, adj, 4)
    # start 1 ("a"): component {1, 0} leaves the subset at 2 < 4, so the next start, 2 ("c"), joins: 2, 3 fill it; 4 is outside
    assert got[0] == (1, [1, 0, 2, 3], [0, 1, 2])    # 3 has the neighbour 4 outside the subset
    # then 4 ("d") is the smallest remaining name: 4, 3; still < 4 and 5 remains: 5 joins; all nodes are in: the batch closes
    assert got[1] == (4, [4, 3, 5], [3, 4, 5])
    assert len(got) == 2


def test_batching_start_is_the_smallest_name_as_bytes(sc):
    # Python compares str by code point = UTF-8 byte order; "r10" < "r2" < "r9" < "ra"; no edges, subset size 1: one node each
    names = ["r9", "r10", "ra", "r2", "R3", "r"]
    got = _both(sc, names, _graph(6, []), 1)
    assert [s for s, _, _ in got] == [4, 5, 1, 3, 0, 2]
    assert all(sub == [s] and cen == [s] for s, sub, cen in got)


def test_batching_depth_limit_and_exact_fill(sc):
    # a path 0 - 1 - ... - 9 searched from its end with subset size 3: each batch takes 3 nodes, the inner two leave
    names = ["n%d" % i for i in range(10)]
    adj = _graph(10, [(i, i + 1) for i in range(9)])
    got = _both(sc, names, adj, 3)
    assert got[0] == (0, [0, 1, 2], [0, 1]) and got[1] == (2, [2, 3, 4], [2, 3])
    assert [c for _, _, cen in got for c in cen] == list(range(10))
    # a subset that is full exactly when the component ends closes the batch without merging
    got = _both(sc, ["a", "b", "c", "d"], _graph(4, [(0, 1), (2, 3)]), 2)
    assert got == [(0, [0, 1], [0, 1]), (2, [2, 3], [2, 3])]


def test_batching_empty_centre_is_an_error(sc):
    # a 4-cycle with subset size 2: both subset nodes keep a neighbour outside; the script would build this batch for ever
    names = ["a", "b", "c", "d"]
    adj = _graph(4, [(0, 1), (1, 2), (2, 3), (3, 0)])
    with pytest.raises(scrub_oracle.EmptyCentre) as eo:
        scrub_oracle.batches(names, adj, 2)
    assert eo.value.start == 0
    from muchsalsa_amd import _lib
    with pytest.raises(sc.ScrubberError) as ei:
        sc.batches([0, 1, 2, 3], *_csr(adj), subset_size=2)
    assert ei.value.code == _lib.E_LAYOUT and ei.value.node == 0


def test_batching_random_graphs_agree(sc):
    rng = np.random.default_rng(3)
    done = 0
    for k in range(300):
        n = int(rng.integers(1, 40))
        m = int(rng.integers(0, 3 * n))
        edges = {tuple(sorted(e)) for e in rng.integers(0, n, (m, 2)).tolist() if e[0] != e[1]}
        edges = [list(edges)[i] for i in rng.permutation(len(edges))] if edges else []
        names = ["r%d" % v for v in rng.permutation(n * 3)[:n]]
        adj = _graph(n, edges)
        ss = int(rng.integers(1, n + 3))
        try:
            want = scrub_oracle.batches(names, adj, ss)
        except scrub_oracle.EmptyCentre as e:
            with pytest.raises(sc.ScrubberError) as ei:
                sc.batches(sorted(range(n), key=lambda i: names[i].encode()), *_csr(adj), subset_size=ss)
            assert ei.value.node == e.start
            continue
        _both(sc, names, adj, ss)
        done += len(want) > 1
    assert done > 50


def test_covered_ranges_rule():
    # sorted as pairs, merged left to right; touching ranges join (s <= ce), a gap of one position does not
    assert scrub_oracle.covered([(10, 20), (0, 5), (20, 30), (32, 40), (5, 9)]) == [(0, 9), (10, 30), (32, 40)]
    assert scrub_oracle.covered([(0, 100), (10, 20), (50, 120), (121, 130)]) == [(0, 120), (121, 130)]
