"""The edge cases of the unitig coverage filter and of the read scrubber (tests/ufedgecases.py, tests/scrubedgecases.py), host
side (no GPU): the restatements (tests/uf_oracle.py, tests/scrub_oracle.py) give every hand-derived literal, every condition
that keeps tests/test_gpu_scrub_uf_edges.py from passing on nothing holds, and the restatement of the scrubber equals the
reference script's recorded result on every case (tests/golden/scrubber/edges.json, made by tools/make_scrubber_fixtures.py
--only edges)."""
import hashlib
import json
import os

import pytest

import scrub_oracle
import scrubedgecases as S
import uf_oracle
import ufedgecases as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the lists ----------------------------------------------------------------------------------------------------------

def test_the_gpu_file_runs_these_cases_and_skips_none():
    import test_gpu_scrub_uf_edges as G
    assert G.UF_PASS1 == U.names(pass2=False) and G.UF_PASS2 == U.names(pass2=True) and G.SCRUB == S.names()
    assert sorted(G.UF_PASS1 + G.UF_PASS2) == sorted(U.cases()) and len(U.names()) == len(U.pass1_names()) + 10
    assert U.cases() is U.cases() and S.cases() is S.cases()
    for name in ("test_gpu_scrub_uf_edges.py", "ufedgecases.py", "scrubedgecases.py"):
        with open(os.path.join(ROOT, "tests", name)) as f:
            text = f.read()
        assert "xfail" not in text and "mark.skip" not in text and "pytest.skip" not in text, name


def test_every_case_is_small():
    for name, c in U.cases().items():
        assert len(c.paf) + len(c.fasta) < 1000000 and c.paf.count(b"\n") <= 4100 and c.note, name
    for name, c in S.cases().items():
        assert len(c.anchors) + len(c.ava) + len(c.reads) < 1000000 and c.note, name
    lines = [t.split(b"\t")[0] for t in S.cases()["chunk_sizes"].anchors.split(b"\n")[:-1]]
    assert max(lines.count(u) for u in set(lines)) == 257


# ---- coverage filter ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", U.names(pass2=False))
def test_filter_pass1_case(name):
    c = U.cases()[name]
    text, rep = U.expected(name)
    v = c.lit["v"]
    assert rep["q3"] == c.lit["q3"] == (1 + 0.75 * (v - 1) if v else 0.75) and U.pass1_value(c.paf) == v
    assert rep["outliers"] == 0 and text.count(b">") == rep["blocks"]
    assert U.classes(c.paf) == c.lit["klass"]
    parts = name.split("-")
    if parts[0] == "staircase":
        k = int(parts[1])
        lines = U.stairs(k, parts[-1] == "rev")
        assert v == k and [i for i, l in enumerate(lines) if l[0] == k - 1] == [0 if parts[-1] == "rev" else k - 1]
        assert U.peak_event(lines) == k - 1  # the K starts sort before every end
        if k in U.STAIRS_ONE_WAY:
            assert (k - 1) % 64 == {1089: 0, 1088: 63}[k]
        if k > U.GROUP:
            assert (k - 1) // 64 >= 16  # the depth still rises in the 17th round of 64 events
    else:
        # the padding would have counted: with its repeated read ids made unique the value is another one
        assert U.pass1_value(U.pass1(name, unique=True)[0]) != v
        assert U.classes(U.pass1(name, unique=True)[0]) == c.lit["klass"]
        blocks = c.paf.split(U.FILLER[0])
        assert blocks[-1].count(b"\n") == U.PAD[parts[1]]


def test_filter_pass1_geometries():
    """what each geometry is about, said on its lines"""
    g = U.GEOMETRY
    assert [l[:2] for l in g["touching"][1]] == [(0, 10), (10, 20), (20, 30)]
    s, e, r = zip(*g["first_line_empty"][1])
    assert r == (b"a", b"c", b"c") and (s[1], e[1]) == (30, 30) and s[0] <= s[2] < e[2] <= e[0]
    assert any(s > e for s, e, _ in g["inverted"][1]) and len(set(g["one_read"][1])) == 1
    assert all(s >= e for s, e, _ in g["all_empty"][1])
    assert all((s, e) == (0, g["from_zero_to_qlen"][0]) for s, e, _ in g["from_zero_to_qlen"][1])
    for cls in U.PAD:
        lines = U.padded("far_repeat", cls)
        assert lines[0][2] == lines[-1][2] == b"a" and len(lines) == U.PAD[cls]
    names, _, _, _, _ = uf_oracle.parse_paf(U.cases()["last_block_wins-giant"].paf)
    assert [names[0], names[5], names[6], names[-1]] == [b"T", b"f0", b"T", b"T"]


@pytest.mark.parametrize("name", U.names(pass2=True))
def test_filter_pass2_case(name):
    c = U.cases()[name]
    text, rep = U.expected(name)
    lit = c.lit
    assert (rep["q1"], rep["q3"], rep["upper"], rep["outliers"], rep["rescued"]) == (
        lit["q1"], lit["q3"], lit["upper"], lit["outliers"], lit["rescued"])
    lengths = U.record_lengths(text)
    for uid, frags in lit["frags"].items():
        assert U.fragments(text, uid) == frags and uid not in lengths
        assert [lengths[b"%s_%d" % (uid, k)] for k, _, _, _ in frags] == [
            lit["lengths"].get(b"%s_%d" % (uid, k), n) for k, n, _, _ in frags]
        assert all(n == e - s + 1 for _, n, s, e in frags)
    # every other id is written whole, under its description line
    others = [h for h in lengths if b"_" not in h]
    assert len(others) == rep["blocks"] - rep["outliers"] and all(lengths[h] == 300 for h in others)


def test_filter_pass2_conditions():
    c = U.cases()
    # the id of value 7 equals the upper bound and stays
    assert b">n7 edge case\n" in U.expected("equal_to_upper")[0] and U.OTHERS[7] == 7 == c["equal_to_upper"].lit["upper"]
    assert c["short_outlier"].lit["rescued"] == 0 and b">O" not in U.expected("short_outlier")[0]
    # pass 1 sees one line of the repeated read: with the tower's reads alone the value stays 8 (not 10)
    paf = U.FILLER[0] + U.block(b"T", 3000, U.tower(0, 500, 8, b"x") + [(1000, 2000, b"rep")] * 10)
    assert U.pass1_value(paf) == 8
    text = U.expected("two_outliers_and_one_between")[0]
    assert text.index(b">O_1") < text.index(b">n6 ") < text.index(b">P_0")
    assert U.expected("record_shorter_than_qlen")[0].endswith(b">O_1 1500 1500 2999\n")
    assert c["pile_of_endpoints"].paf.count(b"\t1000\t2000\t") == 1000
    assert U.classes(c["pile_of_endpoints"].paf)["group_blocks"] == 1
    assert c["fractional_q3"].lit["q3"] % 1 == 0.75


# ---- scrubber -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "scrubber", "edges.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name", S.names())
def test_scrubber_case(name, recorded):
    c = S.cases()[name]
    batches, st, text = S.expected(name)
    assert S.meets_literals(name, text, st) == []
    assert set(recorded["cases"]) | set(recorded["unprocessed"]) == set(S.names())
    if name in recorded["cases"]:  # the reference script's own result on these bytes
        recs = scrub_oracle.records(text)
        ref = recorded["cases"][name]
        assert (c.subset_size, len(recs)) == (ref["subset_size"], ref["records"])
        assert hashlib.sha256(b"".join(b">" + h + b"\n" + recs[h] for h in sorted(recs))).hexdigest() == ref["sha256_sorted"]
    else:
        assert recorded["unprocessed"][name]


def test_the_reference_script_processed_every_case(recorded):
    assert recorded["unprocessed"] == {}


def test_scrubber_graph_conditions():
    for name in ("no_pairs", "no_pairs_but_lines", "one_node"):
        g = S.expected(name)[1]["graph"]
        assert all(n == 1 for n in _chunk_lengths(S.cases()[name].anchors)) and not any(g["adj"])
    assert S.expected("no_pairs_but_lines")[1]["ava_lines"] == 2
    for name in ("no_ava_lines", "all_ava_lines_drop"):
        st = S.expected(name)[1]
        assert st["ava_lines"] == 0 and st["edges"] == 4
    assert S.cases()["no_ava_lines"].ava == b"" and S.cases()["all_ava_lines_drop"].ava.count(b"\n") == 4
    assert sorted(_chunk_lengths(S.cases()["chunk_sizes"].anchors)) == [2, 3, 3, 64, 65, 257]
    st = S.expected("chunk_sizes")[1]
    assert st["edges"] < S.cases()["chunk_sizes"].lit["pairs"] - 1000  # many edges are met in several chunks
    assert _chunk_lengths(S.cases()["anchor_name_returns"].anchors) == [2, 1, 2]


def _chunk_lengths(anchors):
    out, prev = [], None
    for t in anchors.split(b"\n")[:-1]:
        u = t.split(b"\t")[0]
        if u != prev:
            out.append(0)
            prev = u
        out[-1] += 1
    return out


def test_late_first_pair_depends_on_the_time_of_the_first_pair():
    c = S.cases()["late_first_pair"]
    g = S.expected("late_first_pair")[1]["graph"]
    x, y = g["node"]["X"], g["node"]["Y"]
    assert g["adj"][x] == c.extra["row_x"] and g["adj"][y] == c.extra["row_y"]
    assert _chunk_lengths(c.anchors) == [65, 2, 2, 3]
    # the pair (X, Y) is the last of the first chunk's 2080 and the first of the last chunk's
    first = [t.split(b"\t")[5] for t in c.anchors.split(b"\n")[:65]]
    assert first[63:] == [b"X", b"Y"]
    moved = scrub_oracle.read_graph(c.extra["moved"])

    def row(gr, r):
        return [gr["names"][w] for w in gr["adj"][gr["node"][r]]]

    assert sorted(row(moved, "X")) == sorted(row(g, "X")) and row(moved, "X") != row(g, "X")
    assert row(g, "X")[-3:] == ["Y", "Z1", "Z3"] and row(moved, "X")[:3] == ["Z1", "Y", "Z3"]


def test_scrubber_fold_conditions():
    lit = {n: S.cases()[n].lit["records"] for n in S.names()}
    assert lit["chain_of_130"][b"P_0"] != lit["chain_of_130_reversed"][b"P_0"]
    assert S.chain_lines(True)[0].split(b"\n")[:-1] == S.chain_lines()[0].split(b"\n")[:-1][::-1]
    rows = [t.split(b"\t") for t in S.chain_lines()[0].split(b"\n")[:-1]]
    assert len(rows) == 130 and all(t[0] == (b"P", b"Q")[i % 2] for i, t in enumerate(rows))
    # every line but the first is within 499 of the state only through the line two before it
    S0, E0 = int(rows[0][2]), int(rows[0][3])
    for i, t in enumerate(rows[1:], 1):
        s, e = int(t[2]), int(t[3])
        assert abs(S0 - e) == 300 or abs(s - E0) == 300
        assert i < 3 or min(abs(int(rows[i - 2][2]) - e), abs(s - int(rows[i - 2][3]))) == 300
        S0, E0 = min(s, S0), max(e, E0)
    c = S.cases()["lane_phases"]
    heads = {h: S.group_heads(c.anchors, c.ava, h) for h, _ in S.HUBS}
    assert [len(heads[h]) for h, _ in S.HUBS] == [64, 65, 129]
    assert {i % 64 for v in heads.values() for i in v} == set(range(64))
    assert S.expected("lane_phases")[1]["ava_lines"] == sum(1 + (i % 3 >= 1) + (i % 3 == 2) for _, n in S.HUBS
                                                            for i in range(n)) > 500


def test_three_batches_differ_from_two():
    c = S.cases()["three_batches"]
    _, st, text = S.expected("three_batches")
    assert [(a, b, d) for a, b, d in st["plan"]] == c.lit["plan"]
    assert sum(1 for _, sub, _ in st["plan"] if 1 in sub and 2 in sub) == 3
    two, st2 = scrub_oracle.scrub(c.extra["two_batch_anchors"], c.ava, S.reads_of("three_batches"), 3)
    assert sum(1 for _, sub, _ in st2["plan"] if 1 in sub and 2 in sub) == 2
    assert S.record_lengths(scrub_oracle.text(two))[b"B_0"] == c.extra["two_batch_b0"] != c.lit["records"][b"B_0"]


def test_never_together_shares_no_subset():
    c = S.cases()["never_together"]
    _, st, _ = S.expected("never_together")
    a, b = c.extra["pair"]
    assert (a, b, 2000, 3000, "+", 2000, 3000) in scrub_oracle.ava_lines(c.ava, st["graph"]["node"])
    assert not any(a in sub and b in sub for _, sub, _ in st["plan"]) and len(st["plan"]) == 2
    # at the default subset size the pair is together and both reads get the range
    one, _ = scrub_oracle.scrub(c.anchors, c.ava, S.reads_of("never_together"))
    assert S.record_lengths(scrub_oracle.text(one))[b"A_2"] == 1001
