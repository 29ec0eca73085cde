"""The 16-byte scaffold rows of by_anchor and the rank the candidate kernels hand to the chain kernels (which read both rows of
an EdgeMatch from by_read: v2's at read_off[v2] + rank), at the smallest shapes where either can go wrong.  Hand-built row
tables against the C oracle, all four tables bit for bit, on the bin path and on the atomic path (MSGPU_NO_BIN=1) of the index
build: ranks that run against the lane order or are no run at all, ranks among the rows that survive the duplicate rule, ranks
that do not fit a byte, every chain kernel body, scaffolds that end on and cross a 128-byte line at the table's end, and the
same kernels through the shard and window entries.  Each workload asserts that it holds what it claims to test."""
import numpy as np
import pytest

import extremecases as X
from helpers import assert_tables_equal
from muchsalsa_amd.synth import ROW_DTYPE

pytestmark = pytest.mark.gpu

PATHS = [None, "MSGPU_NO_BIN"]
CHAIN_ENVS = [None, "MSGPU_NO_SUBWAVE", "MSGPU_CHAIN_SERIAL", "MSGPU_NO_FASTPATH"]
LEN = 4_000_000  # every read's length
SIZES = (1, 2, 8, 9, 16, 17, 32, 33, 64, 65)


# ---- builders -------------------------------------------------------------------------------------------------------------------
def table(scaffolds):
    """A row table from its scaffolds in file order.  A scaffold is the list of its rows in line order, a row
    (read label, n_lo, plus[, i_lo, i_hi]).  Anchors are numbered by position, reads by first appearance, lines count up: the
    Registry's ids, grouped by anchor with ascending lines as the PAF loader leaves them."""
    ids, out, line = {}, [], 0
    for a, sc in enumerate(scaffolds):
        for ent in sc:
            label, n_lo, plus = ent[:3]
            i_lo, i_hi = ent[3:5] if len(ent) > 3 else (0, 599)
            r = ids.setdefault(label, len(ids))
            out.append(X.row(a, r, LEN, i_lo, i_hi, n_lo, n_lo + (i_hi - i_lo), 500 + (7 * line) % 100, line, plus))
            line += 1
    return X.check_int32(np.array(out, dtype=ROW_DTYPE))


def pair_edge(sc, e, n, minus=False, swap=None, gap=None, base=0):
    """scaffolds of one edge between reads (e, "a") and (e, "b") over n anchors, "a" ascending.  minus: "b" on the reverse strand
    and descending, so its ranks fall along the edge.  swap = k: the places of "b"'s rows k and k + 1 exchanged (one inversion).
    gap = k: a row of "b" on an anchor of its own between its rows k and k + 1 (the ranks are no run)."""
    pos = [1000 * (n - 1 - j) if minus else 1000 * j for j in range(n)]
    if swap is not None:
        pos[swap], pos[swap + 1] = pos[swap + 1], pos[swap]
    for j in range(n):
        sc.append([((e, "a"), base + 1000 * j, True), ((e, "b"), base + 200 + pos[j], not minus)])
    if gap is not None:
        sc.append([((e, "b"), base + 200 + (pos[gap] + pos[gap + 1]) // 2, not minus)])


def rank_order_rows():
    """per size class of the chain kernels: ranks falling, falling with one inversion and one gap, and an edge whose v2 shares
    only its first and its last row with v1"""
    sc, e = [], 0
    for n in (66, 6, 12, 48, 24):  # (in this order the bin path's buckets of sixteen reads hold alike numbers of rows)
        pair_edge(sc, e, n, minus=True)
        pair_edge(sc, e + 1, n, minus=True, swap=n // 2, gap=2)
        pair_edge(sc, e + 2, n, minus=False, swap=1, gap=n - 2)
        e += 3
    for m in (2, 10, 40):  # v2 of m rows: rank 0 and rank m - 1 are shared, the rows between them are v2's alone
        sc.append([((e, "a"), 0, True), ((e, "b"), 100, True)])
        for k in range(1, m - 1):
            sc.append([((e, "b"), 100 + 1000 * k, True)])
        sc.append([((e, "a"), 1000 * m, True), ((e, "b"), 100 + 1000 * (m - 1), True)])
        e += 1
    return table(sc)


def duplicate_rows(on):
    """reads a, b, c over 10 anchors; read `on` ("a" = v1 of two edges, "b" = v2 of a-b) has a second row on anchor 3, on a later
    line (it loses) and in front of all its other rows: every live row's rank among all rows is one above its rank among the
    survivors.  c shares anchors 5..9, so b owns an edge too."""
    sc = []
    for j in range(10):
        s = [("a", 5000 + 1000 * j, True), ("b", 5300 + 1000 * j, True)]
        if j >= 5:
            s.append(("c", 5100 + 1000 * j, j % 2 == 0))
        if j == 3:
            s.append((on, 10, True))
        sc.append(s)
    return table(sc)


def long_read_rows(n_long):
    """a read L of n_long rows between partners with lower ids (L is their v2, its ranks cross 255 / 256) and partners with
    higher ids (L owns those edges); preamble scaffolds of one row fix the id order"""
    shares = {  # partner -> (L's anchors it shares, reverse strand)
        "S0": (range(250, 263), False), "S1": (range(n_long - 100, n_long - 29), True), "S2": ((0, 255, 256), False),
        "T0": (range(0, 5), False), "T1": (range(254, 259), True), "T2": (range(n_long - 300, n_long), False)}
    sc = [[(s, 0, True)] for s in ("S0", "S1", "S2")]
    span = 1000 * n_long
    for j in range(n_long):
        ent = {p: (p, 1000 + (span - 1000 * j if rev else 1000 * j), not rev) for p, (js, rev) in shares.items() if j in js}
        sc.append([ent[p] for p in ("S0", "S1", "S2") if p in ent] + [("L", 1000 * j, True)] +
                  [ent[p] for p in ("T0", "T1", "T2") if p in ent])
    return table(sc)


# (eight edges = sixteen reads = one bucket of the bin path: the order keeps the buckets' row counts alike)
BODY_ORDER = (65, 1, 64, 2, 33, 8, 32, 9, 17, 16, 65, 1, 64, 2, 33, 8, 32, 9, 17, 16)


def bodies_rows(big):
    """edges of every size in SIZES twice (forward with an inversion, reverse with a gap), and with `big` one of 300"""
    sc = []
    for e, n in enumerate(BODY_ORDER):
        first = e < len(BODY_ORDER) // 2
        pair_edge(sc, e, n, minus=not first, swap=(n // 2 - 1) if first and n >= 3 else None,
                  gap=(n // 3) if not first and n >= 2 else None)
    if big:
        pair_edge(sc, len(BODY_ORDER), 300, minus=True, swap=255, gap=100)
    return table(sc)


def ends_rows(last):
    """nine reads; scaffolds of 1, 2, 8 and 9 rows (nine 16-byte rows cross a 128-byte line), then the job's last anchor with
    `last` rows: the reads with the highest ids, so the table's last 16 bytes are the row of the highest read id"""
    sc = [[(r, 1000 * k, True) for r in range(s)] for k, s in enumerate((1, 2, 8, 9))]
    sc.append([(r, 9000, True) for r in range(9 - last, 9)])
    return table(sc)


def no_candidate_rows():
    """visits without a candidate (two rows of one anchor whose unitig intervals do not overlap) and scaffolds of one row"""
    return table([[("a", 0, True)], [("a", 1000, True, 0, 299), ("b", 1000, True, 300, 599)], [("b", 3000, True)], [("c", 0, True)]])


# ---- what a table holds ---------------------------------------------------------------------------------------------------------
def live_ranks(rows):
    """{(read, anchor): (rank among the surviving rows of the read, rank among all its rows)} in the order of by_read:
    (n_lo, n_hi, anchor); of a duplicate (read, anchor) pair the lowest line survives"""
    out = {}
    for r in np.unique(rows["read_id"]):
        mine = rows[rows["read_id"] == r]
        mine = mine[np.lexsort((mine["line"], mine["anchor_id"], mine["n_hi"], mine["n_lo"]))]
        best = {}
        for m in mine:
            best[int(m["anchor_id"])] = min(best.get(int(m["anchor_id"]), 2 ** 32), int(m["line"]))
        live = 0
        for k, m in enumerate(mine):
            if int(m["line"]) == best[int(m["anchor_id"])]:
                out[(int(r), int(m["anchor_id"]))] = (live, k)
                live += 1
    return out


def v2_ranks(rows, want):
    """per edge of the oracle's tables: the ranks in v2 of its EdgeMatches, in the edge's (= v1's) order"""
    rk = live_ranks(rows)
    out = []
    for e in want["edges"]:
        ems = want["ems"][int(e["em_off"]):int(e["em_off"]) + int(e["em_cnt"])]
        out.append([rk[(int(e["v2"]), int(m["anchor_id"]))][0] for m in ems])
    return out


def _run(rows):
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables(), int(ctx.counts().index_path)


def _check(oracle, monkeypatch, rows, want, what, path_env, bin_expected=False, generic=False):
    """run on one index path and compare; which path the build took is part of the claim"""
    from muchsalsa_amd import _lib
    if path_env:
        monkeypatch.setenv(path_env, "1")
    got, path = _run(rows)
    print(what, "rows", len(rows), "edges", len(want["edges"]), "ems", len(want["ems"]), "index_path", path)
    if path_env:
        assert (path & 3) != _lib.INDEX_BIN, (what, path)
    elif bin_expected:
        assert path == _lib.INDEX_BIN, (what, path)
    if generic:
        assert path & _lib.INDEX_GENERIC and (path & 3) != _lib.INDEX_BIN, (what, path)
    assert_tables_equal(got, want, "%s/%s" % (what, path_env))


@pytest.fixture(scope="module")
def wants(oracle):
    """the oracle's tables of a workload, computed once"""
    cache = {}

    def get(key, rows):
        if key not in cache:
            cache[key] = oracle.overlap(rows)
        return cache[key]
    return get


# ---- rank order against lane order ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_env", PATHS)
def test_rank_order_against_lane_order(oracle, wants, monkeypatch, path_env):
    rows = rank_order_rows()
    want = wants("rank_order", rows)
    ranks = v2_ranks(rows, want)
    n = [len(r) for r in ranks]
    falling = [r for r in ranks if len(r) > 1 and all(a == b + 1 for a, b in zip(r, r[1:]))]
    assert {len(r) for r in falling} == {6, 12, 24, 48, 66}  # one unbroken run against the lane order per class
    broken = [r for r in ranks if len(r) > 2 and sum(a < b for a, b in zip(r, r[1:])) == 1 and
              any(abs(a - b) > 1 for a, b in zip(r, r[1:])) and r[0] > r[-1]]
    assert {len(r) for r in broken} == {6, 12, 24, 48, 66}   # falling, one inversion, one gap
    rising = [r for r in ranks if len(r) > 2 and sum(a > b for a, b in zip(r, r[1:])) == 1 and r[0] < r[-1] and
              any(b - a > 1 for a, b in zip(r, r[1:]))]
    assert {len(r) for r in rising} == {6, 12, 24, 48, 66}   # rising, one inversion, one gap
    assert sorted(r for r in ranks if len(r) == 2 and r[0] == 0)[-3:] == [[0, 1], [0, 9], [0, 39]]  # first and last row only
    assert max(n) > 64 and min(n) == 2
    _check(oracle, monkeypatch, rows, want, "rank order", path_env, bin_expected=True)


# ---- rank among live rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_env", PATHS)
@pytest.mark.parametrize("on", ["b", "a"])
def test_rank_among_live_rows(oracle, wants, monkeypatch, path_env, on):
    rows = duplicate_rows(on)
    want = wants("dup_" + on, rows)
    rid = {"a": 0, "b": 1}[on]
    rk = {k: v for k, v in live_ranks(rows).items() if k[0] == rid}
    assert len(rk) == 10 and all(allr == live + 1 for live, allr in rk.values())  # the loser sorts in front of every live row
    assert int((rows["read_id"] == rid).sum()) == 11
    edges = {(int(e["v1"]), int(e["v2"])): int(e["em_cnt"]) for e in want["edges"]}
    assert edges == {(0, 1): 10, (0, 2): 5, (1, 2): 5}
    _check(oracle, monkeypatch, rows, want, "duplicate on " + on, path_env, generic=True)


# ---- ranks above 255 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_env", PATHS)
@pytest.mark.parametrize("n_long", [300, 1100])
def test_ranks_above_255(oracle, wants, monkeypatch, path_env, n_long):
    """L as v2 (ranks on both sides of 255 / 256 in one edge) and as owner: 300 rows take the largest LDS class of k_candidates,
    1100 rows k_candidates_big (more than 1024 rows); an edge of more than 64 and one of more than 256 EdgeMatches"""
    from muchsalsa_amd import _lib
    rows = long_read_rows(n_long)
    want = wants("long_%d" % n_long, rows)
    L = 3
    assert int((rows["read_id"] == L).sum()) == n_long
    as_v2 = [r for e, r in zip(want["edges"], v2_ranks(rows, want)) if int(e["v2"]) == L]
    as_v1 = [int(e["em_cnt"]) for e in want["edges"] if int(e["v1"]) == L]
    assert sorted(len(r) for r in as_v2) == [3, 13, 71] and sorted(as_v1) == [5, 5, 300]
    assert all(min(r) <= 255 < max(r) for r in as_v2 if len(r) != 71) and max(max(r) for r in as_v2) == n_long - 30
    assert any(r[0] > r[-1] for r in as_v2)  # (the reverse partner: ranks fall)
    if path_env:
        monkeypatch.setenv(path_env, "1")
    got, path = _run(rows)
    print("long read", n_long, "rows", len(rows), "index_path", path)
    assert (path & 3) != _lib.INDEX_BIN, path  # a read of more than 256 rows is the atomic path's, whoever asks
    assert_tables_equal(got, want, "long read %d/%s" % (n_long, path_env))


# ---- every kernel body -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_env", PATHS)
@pytest.mark.parametrize("env", CHAIN_ENVS)
def test_every_kernel_body(oracle, wants, monkeypatch, path_env, env):
    """one job with edges of 1, 2, 8, 9, 16, 17, 32, 33, 64, 65 and 300 EdgeMatches; the same without the edge of 300 (whose reads
    are beyond the bin path) so that the bin path's tables meet every body too"""
    if env:
        monkeypatch.setenv(env, "1")
    for big in (True, False):
        rows = bodies_rows(big)
        want = wants("bodies_%d" % big, rows)
        n = sorted(int(e["em_cnt"]) for e in want["edges"])
        assert n == sorted(BODY_ORDER + ((300,) if big else ())) and set(SIZES) <= set(n)
        ranks = v2_ranks(rows, want)
        assert any(r[0] > r[-1] for r in ranks if len(r) == 300) == big
        for size in SIZES[1:]:
            mine = [r for r in ranks if len(r) == size]
            assert any(r[0] > r[-1] for r in mine) and any(r[0] < r[-1] for r in mine), size
        _check(oracle, monkeypatch, rows, want, "bodies big=%d/%s" % (big, env), path_env, bin_expected=not big)


# ---- table ends --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path_env", PATHS)
@pytest.mark.parametrize("last", [1, 2, 8, 9])
def test_table_ends(oracle, wants, monkeypatch, path_env, last):
    rows = ends_rows(last)
    want = wants("ends_%d" % last, rows)
    sizes = np.bincount(rows["anchor_id"])
    assert list(sizes) == [1, 2, 8, 9, last] and len(rows) == 20 + last
    tail = rows[rows["anchor_id"] == 4]
    assert int(tail["read_id"].max()) == int(rows["read_id"].max()) == 8   # the highest read id in the table's last row
    assert len(want["edges"]) == 36                                        # every pair of the nine reads
    _check(oracle, monkeypatch, rows, want, "ends %d" % last, path_env, bin_expected=True)


@pytest.mark.parametrize("path_env", PATHS)
def test_one_row_and_no_candidate(oracle, wants, monkeypatch, path_env):
    one = table([[("a", 0, True)]])
    want = wants("one", one)
    assert len(one) == 1 and all(len(want[k]) == 0 for k in ("edges", "ems", "orders", "ids"))
    _check(oracle, monkeypatch, one, want, "one row", path_env)
    none = no_candidate_rows()
    want = wants("none", none)
    assert int(np.bincount(none["anchor_id"]).max()) == 2 and len(want["edges"]) == 0 and len(want["ems"]) == 0
    _check(oracle, monkeypatch, none, want, "no candidate", path_env)


# ---- the same kernels through the other entries ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def synth_job(oracle):
    from muchsalsa_amd import synth
    rows = synth.synth_rows(2000, 5000, 10000, 7)
    return rows, oracle.overlap(rows)


@pytest.mark.parametrize("path_env", PATHS)
def test_shards(synth_job, monkeypatch, path_env):
    """the union over set_shard(r, 3): every shard's tables are the oracle's cut to the edges it owns"""
    from muchsalsa_amd import distributed as D, overlap
    rows, want = synth_job
    if path_env:
        monkeypatch.setenv(path_env, "1")
    n_edges = 0
    for r in range(3):
        with overlap.OverlapContext(0) as ctx:
            ctx.set_shard(r, 3)
            ctx.load_rows(rows)
            ctx.calculate_edges()
            ctx.chaining_and_overlaps()
            t = ctx.tables()
        assert_tables_equal(t, D.shard_view_host(want, r, 3), "shard %d/3/%s" % (r, path_env))
        n_edges += len(t["edges"])
    assert n_edges == len(want["edges"])


@pytest.mark.parametrize("path_env", PATHS)
def test_windows(synth_job, monkeypatch, path_env):
    """overlap_batched with 3 windows: plain, resident, and resident without the EdgeMatch table"""
    from muchsalsa_amd import overlap
    rows, want = synth_job
    if path_env:
        monkeypatch.setenv(path_env, "1")
    with overlap.OverlapContext(0) as ctx:
        got, _ = ctx.overlap_batched(rows, 3)
        assert_tables_equal(got, want, "3 windows/%s" % path_env)
        got, _ = ctx.overlap_batched(rows, 3, resident=True)
        assert_tables_equal(got, want, "3 windows, resident/%s" % path_env)
        assert_tables_equal(ctx.tables(), want, "3 windows, resident: the context's tables/%s" % path_env)
        got, info = ctx.overlap_batched(rows, 3, resident=True, edgematches=False)
        assert got["ems"] is None and info["n_ems"] == len(want["ems"])
        for k in ("edges", "orders", "ids"):
            assert got[k].tobytes() == want[k].tobytes(), (k, path_env)
        idx = np.arange(0, len(want["edges"]), 37, dtype="<u4")
        off, ems = ctx.get_edgematches(idx)
        w = np.concatenate([want["ems"][int(e["em_off"]):int(e["em_off"]) + int(e["em_cnt"])] for e in want["edges"][idx]])
        assert list(np.diff(off)) == [int(c) for c in want["edges"]["em_cnt"][idx]] and ems.tobytes() == w.tobytes()
