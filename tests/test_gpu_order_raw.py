"""Orders as RAW records.  The chain kernels of edges of at most 64 EdgeMatches (k_chain, k_chain_sub_all and their
per-class and WIDE forms) leave an order as the four overhangs of its path -- L1 / L2 stored by the lane of the path's first
anchor, R1 / R2 by the lane of its last -- with the score as a double; k_compact runs getOverlap's four cases (ol.cpp:53-101),
start / end / base and the truncation of the score on them (order_finish, one function for both, msgpu_order_finish on the
host).  k_chain_big still writes finished records, so one k_compact chunk can hold both kinds.  What can go wrong: a case of
(L1 ? L2, R1 ? R2) finished differently, the v2 side taken from the wrong end on a reverse path (main.cpp:73-76), the lanes f
and l mixed up or equal, the second order of an edge (ids_off > 0), minus before plus, a finished record taken for a raw one,
the bases of a window added to the wrong quarter.  Every GPU case compares all four tables with the C oracle bit for bit, and
asserts on the oracle's tables that the input holds what it claims."""
import itertools
import math
import struct

import numpy as np
import pytest

from helpers import assert_tables_equal
from test_golden_hand import case_single_anchor, case_two_anchor_chain, order_from_overhangs, pad, row
from test_gpu_chain_classes import _rows, _run
from muchsalsa_amd.synth import ROW_DTYPE

gpu = pytest.mark.gpu

WIDTHS = (2, 8, 9, 16, 17, 32, 33, 64)
SIGNS = (-1, 0, 1)
START_V1, CONTAINED, DIR, PRIMARY = 1, 2, 4, 8


def probe(s_l, s_r, plus):
    """Reads 0 and 1 share anchors 0 and 1, 700 apart on both (a gap of 102 on each read: compatible, one path [0, 1]); every
    anchor interval is whole on both reads, so the corrections are 0 and the overhangs are integers:
        L1 = 1500, R1 = 7000 - 2799 = 4201 on read 0;  L2 = L1 + 100 s_l, R2 = R1 + 100 s_r on read 1
    with the length of read 1 chosen for it.  plus: read 1 on the same strand (L2 = the first anchor's n_lo, R2 = len2 - the
    last anchor's n_hi); else on the other one, its anchors in descending order (main.cpp:73-76: L2 = len2 - the FIRST
    anchor's n_hi, R2 = the LAST anchor's n_lo).  Returns rows, (L1, R1, L2, R2)."""
    L1, R1 = 1500, 7000 - 2799
    L2, R2 = L1 + 100 * s_l, R1 + 100 * s_r
    len2 = L2 + 1299 + R2
    r0 = [row(0, 0, 7000, 0, 599, 1500, 2099, 580, 0, True), row(1, 0, 7000, 0, 599, 2200, 2799, 560, 2, True)]
    if plus:
        r1 = [row(0, 1, len2, 0, 599, L2, L2 + 599, 570, 1, True), row(1, 1, len2, 0, 599, L2 + 700, L2 + 1299, 550, 3, True)]
    else:
        r1 = [row(0, 1, len2, 0, 599, R2 + 700, R2 + 1299, 570, 1, False), row(1, 1, len2, 0, 599, R2, R2 + 599, 550, 3, False)]
    rows = np.array([r0[0], r1[0], r0[1], r1[1]], dtype=ROW_DTYPE)
    return rows, (float(L1), float(R1), float(L2), float(R2))


def relabel(rows, read0, anchor0, line0):
    out = rows.copy()
    out["read_id"] += read0
    out["anchor_id"] += anchor0
    out["line"] += line0
    return out


def stack(tables):
    """row tables, each on reads 0 and 1, as ONE table: table k on reads 2 k and 2 k + 1, anchors and lines behind the ones
    before it -> (rows, [(first read, first anchor)])"""
    out, where, anchor, line = [], [], 0, 0
    for k, t in enumerate(tables):
        out.append(relabel(t, 2 * k, anchor, line))
        where.append((2 * k, anchor))
        anchor += int(t["anchor_id"].max()) + 1
        line += int(t["line"].max()) + 1
    return np.concatenate(out), where


def sign_table():
    """the nine sign combinations x both strands x every width class (144 edges of one probe path each), and behind them one
    edge of 70 EdgeMatches for k_chain_big: all in one chunk of k_compact"""
    tables, want = [], []
    for n, plus, (s_l, s_r) in itertools.product(WIDTHS, (True, False), itertools.product(SIGNS, SIGNS)):
        rows, lr = probe(s_l, s_r, plus)
        tables.append(pad(rows, n - 2))
        want.append((n, plus, lr))
    tables.append(_rows([(70, "mixed")], 7))
    rows, where = stack(tables)
    return rows, where, want


def orders_of(t, e):
    o0, n = int(t["edges"]["order_off"][e]), int(t["edges"]["order_cnt"][e])
    return t["orders"][o0:o0 + n]


def ids_of(t, o):
    return [int(x) for x in t["ids"][int(o["ids_off"]): int(o["ids_off"]) + int(o["ids_cnt"])]]


@pytest.fixture(scope="module")
def signs(oracle):
    rows, where, want = sign_table()
    t = oracle.overlap(rows)
    # the oracle's tables hold what the input claims
    edges = t["edges"]
    assert len(edges) == len(want) + 1
    by_v1 = {int(v): i for i, v in enumerate(edges["v1"])}
    seen = set()
    for (read0, anchor0), (n, plus, (L1, R1, L2, R2)) in zip(where, want):
        e = by_v1[read0]
        assert int(edges["em_cnt"][e]) == n
        os_ = orders_of(t, e)
        assert len(os_) == 1  # the probe path alone: the fillers are not primary (main.cpp:355-366)
        o = os_[0]
        assert ids_of(t, o) == [anchor0, anchor0 + 1] and bool(int(o["flags"]) & DIR) == plus
        start_v1, contained, left, right = order_from_overhangs(L1, R1, L2, R2)
        assert (bool(int(o["flags"]) & START_V1), bool(int(o["flags"]) & CONTAINED)) == (start_v1, contained)
        assert (float(o["left_offset"]), float(o["right_offset"])) == (left, right)
        assert (int(o["start"]), int(o["end"]), int(o["base"])) == ((read0, read0 + 1, read0) if start_v1 else (read0 + 1, read0, read0))
        seen.add((n, plus, (L1 > L2) - (L1 < L2), (R1 > R2) - (R1 < R2)))
    assert len(seen) == len(WIDTHS) * 2 * 9
    big = by_v1[where[-1][0]]
    assert int(edges["em_cnt"][big]) == 70 and int(edges["order_cnt"][big]) >= 1
    return rows, t


def surround(rows, n_front, n_mid, plus):
    """rows of probe() plus fillers that lie IN FRONT of the probe's first anchor on read 0 (n_front of them, at 100..699) and
    BETWEEN its two anchors (n_mid, at 1800..2399), so that in the edge's EdgeMatches (v1's order = the lanes) the path's first
    anchor is lane n_front and its last one lane n_front + n_mid + 1.  As in test_golden_hand.pad the fillers are not primary
    and their EdgeMatches have the direction the probe's have not (read 1 on the other strand for a forward probe, on the same
    one for a reverse probe), so none is ever compared with a probe EdgeMatch; all lie at 6000..6599 on read 1."""
    out = [tuple(r) for r in rows]
    line, anchor = int(rows["line"].max()) + 1, int(rows["anchor_id"].max()) + 1
    for k in range(n_front + n_mid):
        lo = 100 if k < n_front else 1800
        out.append(row(anchor, 0, 7000, 0, 599, lo, lo + 599, 450, line, True))
        out.append(row(anchor, 1, 7000, 0, 599, 6000, 6599, 440, line + 1, not plus))
        anchor, line = anchor + 1, line + 2
    return np.array(out, dtype=ROW_DTYPE)


INNER = ((8, 3, 3), (16, 5, 9), (32, 11, 19), (64, 29, 33), (64, 61, 1))  # (EdgeMatches, fillers in front, fillers between)


@pytest.fixture(scope="module")
def inner(oracle):
    """the nine combinations x both strands again, with the path's ends on lanes other than 0 and 1: (f, l) = (3, 7), (5, 15),
    (11, 31), (29, 63) and (61, 63), every other lane a filler"""
    tables, want = [], []
    for (n, n_front, n_mid), plus, (s_l, s_r) in itertools.product(INNER, (True, False), itertools.product(SIGNS, SIGNS)):
        rows, lr = probe(s_l, s_r, plus)
        assert n == 2 + n_front + n_mid
        tables.append(surround(rows, n_front, n_mid, plus))
        want.append((n, n_front, n_mid, plus, lr))
    rows, where = stack(tables)
    t = oracle.overlap(rows)
    edges = t["edges"]
    by_v1 = {int(v): i for i, v in enumerate(edges["v1"])}
    assert len(edges) == len(want)
    for (read0, anchor0), (n, n_front, n_mid, plus, (L1, R1, L2, R2)) in zip(where, want):
        e = by_v1[read0]
        assert int(edges["em_cnt"][e]) == n
        em0 = int(edges["em_off"][e])
        lanes = [int(x) for x in t["ems"]["anchor_id"][em0:em0 + n]]
        assert (lanes.index(anchor0), lanes.index(anchor0 + 1)) == (n_front, n_front + n_mid + 1)  # f and l
        os_ = orders_of(t, e)
        assert len(os_) == 1 and ids_of(t, os_[0]) == [anchor0, anchor0 + 1] and bool(int(os_[0]["flags"]) & DIR) == plus
        start_v1, contained, left, right = order_from_overhangs(L1, R1, L2, R2)
        assert (bool(int(os_[0]["flags"]) & START_V1), bool(int(os_[0]["flags"]) & CONTAINED)) == (start_v1, contained)
        assert (float(os_[0]["left_offset"]), float(os_[0]["right_offset"])) == (left, right)
    assert {(w[3], w[1]) for w in want} >= {(True, 3), (True, 61), (False, 61)}
    return rows, t


@gpu
@pytest.mark.parametrize("env", [None, "MSGPU_NO_SUBWAVE"])
def test_path_ends_on_inner_lanes(inner, monkeypatch, env):
    """the lanes f and l that store quarters 1 and 3 are neither lane 0 nor lane 1, and not neighbours: fillers in front of the
    path's first anchor and between its two"""
    if env:
        monkeypatch.setenv(env, "1")
    rows, want = inner
    assert_tables_equal(_run(rows), want, "inner/%s" % env)


@gpu
@pytest.mark.parametrize("env", [None, "MSGPU_CHAIN_SERIAL", "MSGPU_NO_SUBWAVE", "MSGPU_CAND_WIDE"])
def test_sign_combinations(signs, monkeypatch, env):
    """(L1 ? L2, R1 ? R2) in all nine combinations, forward and reverse, in edges of 2, 8, 9, 16, 17, 32, 33 and 64 EdgeMatches
    (test_golden_hand.pad), beside an edge of 70 whose records k_chain_big writes finished -- under the default dispatch, a
    launch per class, the mode without size classes and the WIDE form of the kernels"""
    if env:
        monkeypatch.setenv(env, "1")
    rows, want = signs
    assert_tables_equal(_run(rows), want, "signs/%s" % env)


def both_directions():
    """reads 0 and 1 share anchor 0 on the same strand and anchor 1 on opposite strands, neither primary (scores below 500): a
    path of one anchor in each direction, and with no primary path and no longer one both are kept (main.cpp:355-387), so
    the edge is a shadow with two orders"""
    return np.array([row(0, 0, 9000, 0, 599, 1000, 1599, 450, 0, True), row(0, 1, 9000, 0, 599, 3000, 3599, 440, 1, True),
                     row(1, 0, 9000, 0, 599, 4000, 4599, 430, 2, True), row(1, 1, 9000, 0, 599, 5000, 5599, 420, 3, False)],
                    dtype=ROW_DTYPE)


def several_table():
    """edge 0: two kept paths of one anchor each (chain3000 of test_golden_hand: f == l, the second order's ids_off is 1);
    edge 1: the same in a 33-wide edge (k_chain); edge 2: a path in each direction; edge 3: one EdgeMatch; edge 4: both
    directions in a 17-wide edge"""
    two = case_two_anchor_chain(3000)
    return stack([two, pad(two, 31), both_directions(), case_single_anchor(True), pad(both_directions(), 15)])


@pytest.fixture(scope="module")
def several(oracle):
    rows, where = several_table()
    t = oracle.overlap(rows)
    edges = t["edges"]
    assert [int(x) for x in edges["em_cnt"]] == [2, 33, 2, 1, 17] and [int(x) for x in edges["v1"]] == [0, 2, 4, 6, 8]
    for e in (0, 1):  # two kept paths of one direction; the second one's ids lie behind the first one's
        os_ = orders_of(t, e)
        a0 = where[e][1]
        assert [ids_of(t, o) for o in os_[:2]] == [[a0], [a0 + 1]]
        assert int(os_[1]["ids_off"]) - int(os_[0]["ids_off"]) == 1 and int(edges["shadow"][e]) == 1
    assert len(orders_of(t, 0)) == 2
    for e in (2, 4):  # minus before plus (main.cpp:341-353), though the plus anchor comes first in the edge
        os_ = orders_of(t, e)
        a0 = where[e][1]
        fl = [int(o["flags"]) & DIR for o in os_]
        assert fl == sorted(fl) and set(fl) == {0, DIR}
        assert [a0 + 1] in [ids_of(t, o) for o in os_ if not int(o["flags"]) & DIR]
        assert [ids_of(t, o) for o in os_ if int(o["flags"]) & DIR] == [[a0]]  # the last order: its ids behind all the others'
        assert int(os_[-1]["ids_off"]) - int(os_[0]["ids_off"]) == len(os_) - 1
    assert [ids_of(t, o) for o in orders_of(t, 2)] == [[where[2][1] + 1], [where[2][1]]]
    assert len(orders_of(t, 4)) > 2  # (the fillers of the 17-wide edge are minus paths of their own)
    assert len(orders_of(t, 3)) == 1 and int(orders_of(t, 3)[0]["ids_cnt"]) == 1
    return rows, t


def test_inputs_hold_what_they_claim(signs, several, inner):
    """no GPU: the assertions of the three fixtures on the oracle's tables"""
    assert len(signs[1]["edges"]) == 145 and len(several[1]["edges"]) == 5 and len(inner[1]["edges"]) == 90


@gpu
@pytest.mark.parametrize("env", [None, "MSGPU_NO_SUBWAVE"])
def test_several_kept_paths(several, monkeypatch, env):
    """two orders of one edge (edge-relative ids_off above zero), both directions in one edge (minus first), paths of one
    anchor (the lanes f and l are one lane, which stores both quarters) and an edge of one EdgeMatch -- in the sub-wavefront
    bodies and k_chain, and all of them in k_chain's body (the mode without size classes)"""
    if env:
        monkeypatch.setenv(env, "1")
    rows, want = several
    assert_tables_equal(_run(rows), want, "several/%s" % env)


def degenerate_rows():
    """the probe with an empty interval on read 1's first row: (a) i_hi = i_lo - 1, (b) n_hi = n_lo - 1, (c) both"""
    out = []
    for i_empty, n_empty in ((True, False), (False, True), (True, True)):
        rows, _ = probe(0, 0, True)
        if i_empty:
            rows["i_hi"][1] = rows["i_lo"][1] - 1
        if n_empty:
            rows["n_hi"][1] = rows["n_lo"][1] - 1
        out.append(rows)
    return out


def test_no_row_makes_a_nan_overhang(oracle):
    """`have` is false only for a NaN among the four overhangs, and a NaN needs 0 / 0: rRatio = (i_hi - i_lo + 1) / (n_hi - n_lo
    + 1) with both intervals empty, or a numerator over rRatio = 0.  A row with i_hi = i_lo - 1 never gets that far: the test
    of an EdgeMatch, MatchMap.cpp:192 (`ov_lo <= ov_hi && ov_hi - ov_lo > th_overlap`, in the oracle and in k_candidates),
    refuses every pair it is part of, since ov = [max i_lo, min i_hi] is then empty -- so rRatio's numerator is at least
    th_overlap + 2 wherever overhangs are computed.  n_hi = n_lo - 1 alone gives rRatio = inf and corrections x / inf = 0: finite
    overhangs.  So no row table holds an edge with em_cnt > 0 and order_cnt == 0; have == false is covered through the host
    entry (test_order_finish_on_the_host)."""
    a, b, c = (oracle.overlap(r) for r in degenerate_rows())
    for t in (a, c):  # the row with the empty anchor interval makes no EdgeMatch: anchor 1 alone is left
        assert [int(x) for x in t["edges"]["em_cnt"]] == [1] and [int(x) for x in t["ems"]["anchor_id"]] == [1]
    assert [int(x) for x in b["edges"]["em_cnt"]] == [2]
    for t in (a, b, c):
        assert (t["edges"]["order_cnt"] > 0).all()
        assert np.isfinite(t["orders"]["left_offset"]).all() and np.isfinite(t["orders"]["right_offset"]).all()


@gpu
def test_degenerate_rows_on_the_gpu(oracle):
    """the same three tables through the kernels (the division by an empty nanopore interval included)"""
    for k, rows in enumerate(degenerate_rows()):
        assert_tables_equal(_run(rows), oracle.overlap(rows), "degenerate %d" % k)


@gpu
def test_three_resident_windows(signs):
    """overlap_batched with three resident windows against the single pass: the windows' edge, order and id bases are added
    in k_compact, to the quarters of the FINISHED record"""
    from muchsalsa_amd import overlap
    rows, want = signs
    with overlap.OverlapContext(0, overlap.default_params()) as ctx:
        got, _ = ctx.overlap_batched(rows, 3, resident=True)
        got = {k: got[k] for k in ("edges", "ems", "orders", "ids")}
    assert_tables_equal(got, want, "three windows")


# ---- the shared function, without a GPU --------------------------------------------------------------------------------------

def finish_py(raw_flags, score, L1, L2, R1, R2, v1, v2):
    """ol.cpp:53-101 restated: the four cases in the reference's order; then the order's fields"""
    case = order_from_overhangs(L1, R1, L2, R2)
    if case is None:
        return None
    start_v1, contained, left, right = case
    fl = (START_V1 if start_v1 else 0) | (CONTAINED if contained else 0) | (raw_flags & (DIR | PRIMARY))
    return fl, left, right, int(score), (v1 if start_v1 else v2), (v2 if start_v1 else v1), v1


def finish_c(raw_flags, score, L1, L2, R1, R2, v1, v2):
    from muchsalsa_amd import _lib
    o = np.zeros(1, dtype=_lib.ORDER_DTYPE)
    o["edge_idx"], o["ids_off"], o["ids_cnt"] = 77, 88, 99
    have = _lib.lib().msgpu_order_finish(raw_flags, score, L1, L2, R1, R2, v1, v2, o.ctypes.data)
    assert (int(o["edge_idx"][0]), int(o["ids_off"][0]), int(o["ids_cnt"][0])) == (77, 88, 99)  # left alone
    if not have:
        return None
    r = o[0]
    return (int(r["flags"]), float(r["left_offset"]), float(r["right_offset"]), int(r["score"]), int(r["start"]), int(r["end"]),
            int(r["base"]))


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def same(a, b):
    if a is None or b is None:
        return a is b
    return a[0] == b[0] and bits(a[1]) == bits(b[1]) and bits(a[2]) == bits(b[2]) and a[3:] == b[3:]


def test_order_finish_on_the_host():
    """msgpu_order_finish (order_finish compiled for the host) against the restatement: the nine sign combinations with DIR and
    PRIMARY in every setting and the RAW marker dropped, +-inf on either side, a NaN in each of the four places (have == false:
    the one way an order is not emitted), and scores at 2^53 and above, where a double no longer holds every integer"""
    inf, nan = math.inf, math.nan
    n = 0
    for (s_l, s_r), raw in itertools.product(itertools.product(SIGNS, SIGNS), (0, DIR, PRIMARY, DIR | PRIMARY)):
        args = (1500.25, 1500.25 + 100 * s_l, 4201.5, 4201.5 + 100 * s_r, 5, 9)
        got = finish_c(raw | (1 << 31), 925.75, *args)
        assert got is not None and same(got, finish_py(raw, 925.75, *args)) and got[0] & ~15 == 0
        n += 1
    assert n == 36
    values = (-inf, -1.0, 0.0, -0.0, 1.0, inf)
    for L1, L2, R1, R2 in itertools.product(values, repeat=4):
        # (inf against the same inf: case 1, an offset inf - inf = NaN -- and still an order)
        got, want = finish_c(DIR, 7.0, L1, L2, R1, R2, 3, 4), finish_py(DIR, 7.0, L1, L2, R1, R2, 3, 4)
        assert want is not None and got is not None
        assert got[0] == want[0] and got[3:] == want[3:]
        for g, w in ((got[1], want[1]), (got[2], want[2])):
            assert (math.isnan(g) and math.isnan(w)) or bits(g) == bits(w)
    for place in range(4):
        v = [10.0, 20.0, 30.0, 40.0]
        v[place] = nan
        assert finish_c(DIR | PRIMARY, 7.0, *v, 3, 4) is None and finish_py(DIR | PRIMARY, 7.0, *v, 3, 4) is None
    assert finish_c(0, 7.0, nan, nan, nan, nan, 3, 4) is None
    for score in (0.0, 0.999, 2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 62 + 1024, 2.0 ** 63, 2.0 ** 63 + 2048, 2.0 ** 64 - 2048):
        got = finish_c(PRIMARY, score, 1.0, 2.0, 3.0, 4.0, 3, 4)
        assert got[3] == int(score) and same(got, finish_py(PRIMARY, score, 1.0, 2.0, 3.0, 4.0, 3, 4))
