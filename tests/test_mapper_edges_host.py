"""The mapper's edge cases (tests/mapedgecases.py), host side (no GPU): every condition that keeps tests/test_gpu_mapper_edges.py
from passing on nothing, asserted on the plain-Python restatement (tests/map_oracle.py) alone, mapcases.invariants on every
case, and the restatement against its recorded counts and PAF digests (tests/golden/mapper/edges.json, made by
tools/make_mapper_edge_fixtures.py)."""
import json
import os
import sys

import pytest

import map_oracle
import mapcases
import mapedgecases as E
import test_mapper_batches_host as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "mapper", "edges.json")) as f:
        return json.load(f)


def test_the_fixture_lists_the_cases(recorded):
    ids = [E.case_id(c) for c in E.CASES]
    assert len(set(ids)) == len(ids) and sorted(ids) == sorted(recorded)


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_restatement_against_its_recorded_results_and_invariants(case, recorded):
    import make_mapper_edge_fixtures
    assert make_mapper_edge_fixtures.record(case) == recorded[E.case_id(case)]
    r = E.expected(case[0], **case[1])
    t, q = E.records(case[0])
    assert len({n for n, _ in t}) == len(t) and len({n for n, _ in q}) == len(q)  # (the loader drops a name it has seen)
    mapcases.invariants(r, t, q)
    assert all(c[5] == 0 for c in r["chains"]) and r["keys_dropped"] == 0


def readout(name, params):
    """rules 1 to 4 by hand of the restatement's own functions -> the chain table that READOUT must give"""
    p = dict(map_oracle.PARAMS, **params)
    t, q = E.records(name)
    k = p["k"]
    index = map_oracle.build_index(t, k, p["w"], p["max_occ"])[0]
    out = []
    for (qi, ti, s), a in sorted(map_oracle.anchors(index, q, k, p["w"], 0).items()):
        qlen = len(q[qi][1])
        # rule 6 visits equal f by rising index; rule 7's ranges of a chain of one anchor
        out += [(qi, ti, s, 1, k, 0, y if s == 0 else qlen - y - k, (y if s == 0 else qlen - y - k) + k, x, x + k, k, k) for x, y in a]
    return out


@pytest.mark.parametrize("case", [c for c in E.CASES if E.is_readout(c[1])], ids=E.case_id)
def test_readout_mode_makes_every_anchor_a_chain(case):
    r = E.expected(case[0], **case[1])
    assert len(r["chains"]) == r["anchors"] > 0 and r["groups_kept"] == r["n_groups"]
    assert r["below_score"] == r["below_count"] == r["chains_cut"] == 0
    assert r["chains"] == readout(case[0], case[1])


def test_the_small_workload_in_readout_mode():
    r = E.expected("small", **E.READOUT)
    assert r["anchors"] == len(r["chains"]) == 74362 and r["n_groups"] == r["groups_kept"] == 364


def windows_with_a_hash_tie(seq, k, w):
    """the windows of rule 2 whose smallest hash occurs at two positions or more"""
    n = 0
    for st in map_oracle.positions(seq, k):
        hs = [map_oracle.kf_hash(key) for _, key, _ in st]
        for a in range(len(st) - w + 1):
            n += hs[a:a + w].count(min(hs[a:a + w])) > 1
    return n


@pytest.mark.parametrize("k,w,unit", E.TILE)
def test_the_tile_records_put_stretch_ends_at_every_phase(k, w, unit):
    name = "tile-%d-%d-%d" % (k, w, unit)
    (_, t), = E.records(name)[0]
    breaks = [i for i, b in enumerate(t) if b == ord("N")]
    assert len(t) == unit * 256 and len(breaks) == 256 and {i % 256 for i in breaks} == set(range(256))
    assert unit - 1 - k + 1 >= w  # every stretch has a window
    r = E.expected(name, **dict(E.READOUT, k=k, w=w))
    assert r["minimizers"][0] >= 256 and r["minimizers"][1] == 2 * r["minimizers"][0]
    assert r["n_groups"] >= 2 and {c[2] for c in r["chains"]} == {0, 1}
    # the sketch is that of the stretches one by one: no window crosses an N
    want = []
    for a in range(0, len(t), unit):
        want += [(a + p, key, s) for p, key, s in map_oracle.minimizers(t[a:a + unit - 1], k, w)]
    assert map_oracle.minimizers(t, k, w) == want


@pytest.mark.parametrize("k,w", E.ENDS)
def test_the_short_records_meet_their_conditions(mp, tmp_path, k, w):
    name = "ends-%d-%d" % (k, w)
    t, q = E.records(name)
    assert t == q and len(t) == E.N_ENDS
    lens = [len(s) for _, s in t]
    assert min(lens) >= max(1, k - 2) and max(lens) < k + w + 6
    assert {k - 1, k, k + w - 2, k + w - 1} <= set(lens)
    n_min = [len(map_oracle.minimizers(s, k, w)) for _, s in t]
    print(name, "records without a minimizer:", n_min.count(0), "with one:", n_min.count(1))
    assert n_min.count(0) >= 50 and n_min.count(1) >= 50
    assert all((n == 0) == (ln < k + w - 1) for n, ln in zip(n_min, lens))
    assert record_start_residues(name, tmp_path) >= 128


def record_start_residues(name, directory, store=None):
    """how many residues modulo 256 the records' offsets in the loader's buffer take (the host's parse, or the parse into a
    device store)"""
    from muchsalsa_amd import _lib, sequences
    tp, _ = E.write_inputs(name, directory)
    f = sequences.SeqFile(tp) if store is None else store.parse_upload(sequences.NANOPORE, tp)
    try:
        return len({int(_lib.lib().msgpu_seq_offset(f._h, i)) % 256 for i in range(len(f))})
    finally:
        f.close()


@pytest.mark.parametrize("w", E.TIES_W)
@pytest.mark.parametrize("k", E.TIES_K)
def test_the_runs_make_hash_ties_and_ties_in_the_chains(k, w):
    name = "ties-%d-%d" % (k, w)
    (_, t), = E.records(name)[0]
    (_, q), (_, qr) = E.records(name)[1]
    assert qr == map_oracle.revcomp(q)
    n = E.ties_run_length(k)
    assert n >= 60 and n // 2 > k
    for run in (b"A" * n, b"T" * n, (b"AC" * n)[:n], (b"ACG" * n)[:n], (b"ACGT" * n)[:n]):
        assert run in t and run[:n // 2] in q
    sketch = map_oracle.minimizers(t, k, w)
    assert sum(1 for _, key, _ in sketch if key == 0) >= 2 and map_oracle.kf_hash(0) == 0  # poly-A and poly-T: the smallest hash
    if w > 1:
        assert windows_with_a_hash_tie(t, k, w) >= 10 and windows_with_a_hash_tie(q, k, w) >= 10
    if k % 2 == 0:
        p = E.palindrome(k)
        assert p == map_oracle.revcomp(p) and len(p) == k
        for seq in (t, q, qr):
            at = seq.find(p)
            hit = [m for m in map_oracle.minimizers(seq, k, w) if m[0] == at]
            assert at >= 0 and len(hit) == 1 and hit[0][2] == 0
    r = E.expected(name, **dict(E.TIES_PARAMS[1], k=k, w=w))
    print(name, r["notes"].get("pred_ties"), r["notes"].get("start_ties"), r["chains_cut"], r["largest_group"])
    assert r["notes"]["pred_ties"] >= 1000 and r["notes"]["start_ties"] >= 100 and r["chains_cut"] >= 10
    assert r["largest_group"] > 64 and r["keys_dropped"] == 0 and {c[2] for c in r["chains"]} == {0, 1}
    assert E.expected(name, **dict(E.TIES_PARAMS[0], k=k, w=w))["keys_dropped"] == 0


def test_the_letters_fold_and_break():
    (_, t), = E.records("letters")[0]
    (_, q), _ = E.records("letters")[1]
    assert any(97 <= b <= 122 for b in t) and any(97 <= b <= 122 for b in q)
    iupac = set(b"RYKMSWBDHV")
    assert len({b & 0xdf for b in t} & iupac) >= 8 and len({b & 0xdf for b in q} & iupac) >= 8 and b"N" not in t + q
    r = E.expected("letters", **dict(E.READOUT, w=1))
    covered = set()
    for c in r["chains"]:
        if c[0] == 0 and c[2] == 0:
            covered.update(range(c[8], c[9]))
    lower_t = {i for i, b in enumerate(t) if 97 <= b <= 122 and (b & 0xdf) in b"ACGT"}
    other_t = {i for i, b in enumerate(t) if (b & 0xdf) not in b"ACGT"}
    assert len(lower_t & covered) >= 60 and not other_t & covered  # lower case matches upper case; no k-mer over another letter
    up = map_oracle.run([(b"t", t.upper())], [(b"q", q.upper())], **dict(E.READOUT, w=1))
    assert [c for c in r["chains"] if c[0] == 0] == up["chains"]
    clean = len(map_oracle.minimizers(bytes(b if (b & 0xdf) in b"ACGT" else 65 for b in t), 15, 1))
    assert len(map_oracle.minimizers(t, 15, 1)) <= clean - 14 * len(other_t) // 2
    assert {c[2] for c in E.expected("letters", w=1, min_score=40)["chains"]} == {0, 1}


@pytest.mark.parametrize("m", E.WINDOW_M)
@pytest.mark.parametrize("z", E.WINDOW_Z)
def test_the_window_is_64_predecessors(z, m):
    r = E.expected("window-%d-%d" % (z, m), **E.WINDOW_PARAMS)
    a = sorted(E.window_anchors(z, m))
    assert r["groups"] == [(0, 0, 0, z + m + 2, 1 if m <= 63 else 0, 0)] and r["n_groups"] == 1 and r["anchors"] == z + m + 2
    if m <= 63:
        assert r["chains"] == [(0, 0, 0, 2, 30, 0, a[z][1], a[-1][1] + 15, a[z][0], a[-1][0] + 15, 30, a[-1][0] - a[z][0] + 15 + 3)]
        assert r["notes"]["chain_anchors"] == [[a[z], a[-1]]]
    else:
        assert r["chains"] == []
    assert r["below_score"] == z + m + (0 if m <= 63 else 2)


def test_the_extreme_parameters():
    for m in (63, 64):
        r = E.expected("window-37-%d" % m, **dict(E.WINDOW_PARAMS, max_gap=2 ** 31 - 1, bandwidth=2 ** 31 - 1))
        assert r["groups"][0][3] == 37 + m + 2 and len(r["chains"]) == (m <= 63)
        prm = dict(E.WINDOW_PARAMS, k=32, bandwidth=100000, min_score=0)
        r = E.expected("window-37-%d-32" % m, **prm)
        a = sorted(E.window_anchors(37, m, 32))
        assert r["groups"] == [(0, 0, 0, 37 + m + 2, int(m <= 63), 0)]
        # offers below zero: the last B against C, dd = OFF or more
        dx, dy = a[-1][0] - a[-2][0], a[-1][1] - a[-2][1]
        dd = abs(dx - dy)
        assert dx > 0 and dy > 0 and dd <= 100000 and 32 + min(dx, dy, 32) - ((dd * 32) // 100 + ((dd.bit_length() - 1) >> 1)) < 0
        if m <= 63:
            assert r["chains"][0][3:5] == (2, 64) and r["notes"]["chain_anchors"] == [[a[37], a[-1]]]


@pytest.mark.parametrize("i,p,q", E.TIE_SHAPES)
def test_a_tie_goes_to_the_later_predecessor(i, p, q):
    r = E.expected("tie-%d-%d-%d" % (i, p, q), **E.TIE_PARAMS)
    a = E.tie_anchors(i, p, q)
    assert a == sorted(a) and r["groups"] == [(0, 0, 0, i + 1, 1, 0)] and r["n_groups"] == 1
    assert i - 64 <= p < q < i and r["notes"]["pred_ties"] == 1
    f, pred = map_oracle.chain_dp(a, 15, 100000, 10)
    assert f == [15] * i + [29] and pred == [-1] * i + [q]
    assert r["notes"]["chain_anchors"] == [[a[q], a[i]]] and r["chains"][0][8] == a[q][0] != a[p][0]
    assert r["groups_small"] == (i + 1 <= 16)


def test_the_size_classes(mp):
    fw, rv = E.expected("sizes", **E.SIZES_PARAMS), E.expected("sizes-rc", **E.SIZES_PARAMS)
    assert sorted(E.SIZES) == sorted([1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193] + [16] * 5)
    for r, s in ((fw, 0), (rv, 1)):
        assert r["groups"] == [(i, 0, s, n, 1, 0) for i, n in enumerate(E.SIZES)]
        assert (r["groups_small"], r["groups_large"], len(r["chains"])) == (10, 14, 24)
        assert [c[3] for c in r["chains"]] == list(E.SIZES) and all(c[4] == 15 + c[3] - 1 for c in r["chains"])
    # rule 9's cut at the smallest budget: the batches, and how many groups of at most 16 anchors each one holds
    a, b = edge_record_counts("sizes", E.SIZES_PARAMS)
    assert a == E.SIZES
    one = edge_budgets("sizes", E.SIZES_PARAMS)[0]
    cut = host.greedy_cut(a, b, host.batch_bytes(0), one)
    small = [sum(1 for n in a[first:first + cnt] if n <= 16) for first, cnt, _, _ in cut]
    print(cut, small)
    assert len(cut) == 9 and small.count(1) == 7 and small.count(0) == 1 and small[-1] == 3  # rows of k_mp_chain16 without a group


def edge_record_counts(name, params):
    """test_mapper_batches_host.record_counts for an input of mapedgecases"""
    p = dict(map_oracle.PARAMS, **params)
    t, q = E.records(name)
    index = map_oracle.build_index(t, p["k"], p["w"], p["max_occ"])[0]
    a = [0] * len(q)
    for (qi, _, _), g in map_oracle.anchors(index, q, p["k"], p["w"], 0).items():
        a[qi] += len(g)
    return tuple(a), tuple(len(s) for _, s in q)


def edge_budgets(name, params):
    """test_mapper_batches_host.budgets for an input of mapedgecases: every record fits; one batch; half-way"""
    a, b = edge_record_counts(name, params)
    nbytes = host.batch_bytes(params.get("exact", 0))
    one, whole = nbytes(max(a, default=0), max(b, default=0)), nbytes(sum(a), sum(b))
    return one, whole, (one + whole) // 2
