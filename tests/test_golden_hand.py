"""Hand-derived known-answer vectors for the overlap path.

Expected values are worked out from the reference text (file:line in the comments) with explicit arithmetic here,
independently of either restatement's code.  They check the CPU oracle on CPU; test_gpu_parity.py re-uses CASES to
check the HIP path against the same expectations on the GPU.
"""
import numpy as np
import pytest

from muchsalsa_amd.synth import ROW_DTYPE


def row(anchor, read, read_len, i_lo, i_hi, n_lo, n_hi, score, line, plus):
    prim = (i_hi - i_lo + 1) >= 500 and score >= 500  # BlastFileReader.cpp:121-122
    return (anchor, read, read_len, i_lo, i_hi, n_lo, n_hi, score, line, (1 if plus else 0) | (2 if prim else 0))


def case_single_anchor(plus1=True, i1=(100, 699)):
    """Two reads sharing one anchor."""
    rows = np.array([row(0, 0, 5000, 0, 599, 1000, 1599, 550, 0, True),
                     row(0, 1, 5000, i1[0], i1[1], 200, 799, 560, 1, plus1)], dtype=ROW_DTYPE)
    return rows


def expected_single_anchor(plus1):
    # MatchMap.cpp:188-202: outer = line 1 (read 1), inner = line 0 (read 0)
    ov = (max(100, 0), min(699, 599))
    assert ov == (100, 599) and ov[1] - ov[0] > 100
    cl, ol, il = float(ov[1] - ov[0] + 1), float(699 - 100 + 1), float(599 - 0 + 1)
    score = 560.0 * cl / ol + 550.0 * cl / il
    # getOverhangs (ol.cpp:31-50); rRatio = 600/600 on both reads
    rr = 600.0 / 600.0
    ncl1, ncr1 = (100 - 0) / rr, (599 - 599) / rr          # read 0 is '+'
    L1, R1 = 1000.0 + ncl1, float(5000 - 1599) + ncr1
    ncl2, ncr2 = (100 - 100) / rr, (699 - 599) / rr
    if not plus1:                                           # swap_if(!vertexMatch->direction), ol.cpp:42
        ncl2, ncr2 = ncr2, ncl2
    l2, r2 = 200.0 + ncl2, float(5000 - 799) + ncr2
    if plus1:
        L2, R2 = l2, r2
    else:                                                   # ol.cpp:73-76: second read's sides swap
        L2, R2 = r2, l2
    return dict(score=score, direction=plus1, L1=L1, R1=R1, L2=L2, R2=R2)


def order_from_overhangs(L1, R1, L2, R2):
    """The four cases of ol.cpp:79-97 -> (start_is_v1, contained, left, right)."""
    if L1 <= L2 and R1 <= R2:
        return True, True, L2 - L1, R2 - R1
    if L1 >= L2 and R1 >= R2:
        return False, True, L1 - L2, R1 - R2
    if L1 > L2 and R1 < R2:
        return True, False, L1 - L2, R2 - R1
    if L1 < L2 and R1 > R2:
        return False, False, L2 - L1, R1 - R2
    return None


def check_single_anchor(t, plus1):
    exp = expected_single_anchor(plus1)
    assert len(t["edges"]) == 1 and len(t["ems"]) == 1 and len(t["orders"]) == 1 and list(t["ids"]) == [0]
    e, em, o = t["edges"][0], t["ems"][0], t["orders"][0]
    # v1 = read with the lower first line (MatchMap.cpp:204-213)
    assert (e["v1"], e["v2"], e["em_cnt"], e["order_cnt"]) == (0, 1, 1, 1)
    assert (em["ov_lo"], em["ov_hi"], em["anchor_id"], em["line"]) == (100, 599, 0, 1)
    assert em["flags"] == (1 if plus1 else 0) | 2
    assert float(em["score"]) == exp["score"]
    # single anchor: hasPrimary = EdgeMatch.isPrimary (mpp.cpp:217-220); anchored at both read ends (both reads have
    # only this anchor) -> stays primary (:272-296) -> edge is not a shadow (main.cpp:393-394)
    assert e["shadow"] == 0
    start_v1, contained, left, right = order_from_overhangs(exp["L1"], exp["R1"], exp["L2"], exp["R2"])
    fl = int(o["flags"])
    assert bool(fl & 1) == start_v1 and bool(fl & 2) == contained and bool(fl & 4) == plus1 and bool(fl & 8)
    assert float(o["left_offset"]) == left and float(o["right_offset"]) == right
    assert int(o["score"]) == int(exp["score"])  # truncation to std::size_t (mpp.cpp:34,221)
    assert (o["start"], o["end"], o["base"]) == ((0, 1, 0) if start_v1 else (1, 0, 0))
    assert (o["ids_off"], o["ids_cnt"]) == (0, 1)


def test_expected_numbers_by_hand():
    # the worked example in numbers: score = 560*500/600 + 550*500/600, overhangs 1100/3401 vs 200/4301
    exp = expected_single_anchor(True)
    assert abs(exp["score"] - 925.0) < 1e-9
    assert (exp["L1"], exp["R1"], exp["L2"], exp["R2"]) == (1100.0, 3401.0, 200.0, 4301.0)
    assert order_from_overhangs(1100.0, 3401.0, 200.0, 4301.0) == (True, False, 900.0, 900.0)
    expm = expected_single_anchor(False)
    assert (expm["L2"], expm["R2"]) == (4201.0, 300.0)  # read 1 flipped: (len-n_hi)+0 = 4201 on the left, 200+100 right
    assert order_from_overhangs(1100.0, 3401.0, 4201.0, 300.0) == (False, False, 3101.0, 3101.0)


@pytest.mark.parametrize("plus1", [True, False])
def test_single_anchor_oracle(oracle, plus1):
    check_single_anchor(oracle.overlap(case_single_anchor(plus1)), plus1)


def case_overlap_threshold(delta):
    """ov.hi - ov.lo == delta: an EdgeMatch exists iff delta > 100 (strict, MatchMap.cpp:192)."""
    return np.array([row(0, 0, 5000, 0, 599, 1000, 1599, 550, 0, True),
                     row(0, 1, 5000, 599 - delta, 1200, 200, 801 + delta, 560, 1, True)], dtype=ROW_DTYPE)


@pytest.mark.parametrize("delta,edges", [(99, 0), (100, 0), (101, 1), (400, 1)])
def test_overlap_threshold_oracle(oracle, delta, edges):
    t = oracle.overlap(case_overlap_threshold(delta))
    assert len(t["edges"]) == edges and len(t["ems"]) == edges


def case_two_anchor_chain(gap2):
    """Two reads, two shared anchors 2000 bp apart on read 0 and `gap2` apart on read 1 (all '+', rRatio 1)."""
    return np.array([
        row(0, 0, 9000, 0, 599, 1000, 1599, 580, 0, True),
        row(0, 1, 9000, 0, 599, 3000, 3599, 570, 1, True),
        row(1, 0, 9000, 0, 599, 3600, 4199, 560, 2, True),
        row(1, 1, 9000, 0, 599, 3600 + gap2, 4199 + gap2, 550, 3, True),
    ], dtype=ROW_DTYPE)


@pytest.mark.parametrize("gap2,chained", [(2000, True), (2300, True), (2301, True), (2353, True), (2354, False), (3000, False)])
def test_two_anchor_chain_oracle(oracle, gap2, chained):
    """checkCompatibility (mpp.cpp:133-139): orientation 1 on both reads, diff1 = 3600-1599+1 = 2002,
    diff2 = 2002 + (gap2 - 2000).  Compatible iff |d1-d2| <= 300 or |d1-d2|*100/max <= 15:
    301*100/2303 = 13.07 and 353*100/2355 = 14.99 still chain, 354*100/2356 = 15.03 does not."""
    d1, d2 = 3600.0 - 1599.0 + 1, (3600.0 + gap2) - 3599.0 + 1
    df = max(d1, d2) - min(d1, d2)
    assert chained == (df <= 300.0 or df * 100 / max(d1, d2) <= 15)
    t = oracle.overlap(case_two_anchor_chain(gap2))
    assert len(t["edges"]) == 1 and len(t["ems"]) == 2
    s0, s1 = 570.0 * 600.0 / 600.0 + 580.0 * 600.0 / 600.0, 550.0 + 560.0
    assert [float(x) for x in t["ems"]["score"]] == [s0, s1]
    if chained:
        # one path [u0, u1], score truncated; len 2 -> not "> 2", primary through EdgeMatch.isPrimary
        assert len(t["orders"]) == 1 and list(t["ids"]) == [0, 1] and int(t["orders"][0]["score"]) == int(s0 + s1)
        assert t["edges"][0]["shadow"] == 0
    else:
        # two disjoint single-anchor paths: best = u0 (1150 > 1110), alternative u1 (1110 > 0.75*1150);
        # combined size 2 -> shadow (main.cpp:389-391)
        assert len(t["orders"]) == 2 and list(t["ids"]) == [0, 1]
        assert [int(s) for s in t["orders"]["score"]] == [int(s0), int(s1)]
        assert t["edges"][0]["shadow"] == 1


CASES = {
    "single_plus": case_single_anchor(True), "single_minus": case_single_anchor(False),
    "thr100": case_overlap_threshold(100), "thr101": case_overlap_threshold(101),
    "chain2000": case_two_anchor_chain(2000), "chain2300": case_two_anchor_chain(2300),
    "chain2301": case_two_anchor_chain(2301), "chain2353": case_two_anchor_chain(2353),
    "chain2354": case_two_anchor_chain(2354), "chain3000": case_two_anchor_chain(3000),
}


# ----------------------------------------------------------------------------------------------------------------------
# Non-default msgpu_params: the parameter-dependent rules of checkCompatibility (mpp.cpp:133-139: wiggle room and the
# ratio rule) and of the alternatives of getMaxPairwisePaths (mpp.cpp:223-249: alt_frac) at their boundaries.
# ----------------------------------------------------------------------------------------------------------------------
def case_two_anchors(n0, n1, scores=(580, 570, 560, 550)):
    """case_two_anchor_chain with the second anchor placed freely: anchor 0 at 1000..1599 on read 0 and 3000..3599 on
    read 1, anchor 1 at n0..n0+599 on read 0 and n1..n1+599 on read 1 (all '+', full anchor overlaps, rRatio 1: the
    corrected ranges are the raw ones and the EdgeMatch scores are the row-score sums, exactly)."""
    return np.array([
        row(0, 0, 9000, 0, 599, 1000, 1599, scores[0], 0, True),
        row(0, 1, 9000, 0, 599, 3000, 3599, scores[1], 1, True),
        row(1, 0, 9000, 0, 599, n0, n0 + 599, scores[2], 2, True),
        row(1, 1, 9000, 0, 599, n1, n1 + 599, scores[3], 3, True),
    ], dtype=ROW_DTYPE)


def case_gaps(d1, d2, scores=(580, 570, 560, 550)):
    """Orientation +1 on both reads with diff1 = d1 and diff2 = d2 (diff = c2.lo - c1.hi + 1, mpp.cpp:115-120)."""
    return case_two_anchors(1598 + d1, 3598 + d2, scores)


def case_mixed(d1, d2):
    """Orientation +2 on read 0 (anchor 1 overlaps anchor 0 by d1 = c1.hi - c2.lo + 1 bases, mpp.cpp:106-110; the raw
    ranges are in the same order, so nanoCheck does not abort) and +1 on read 1 with a gap diff2 = d2: a mixed pair,
    compatible iff d1 + d2 <= wiggle (mpp.cpp:137-138); the ratio rule does not apply."""
    return case_two_anchors(1600 - d1, 3598 + d2)


def pad(rows, n_fill):
    """rows plus n_fill filler anchors shared by reads 0 and 1 with the OPPOSITE strand on read 1: their EdgeMatches are
    reverse, so no filler is ever compared with a probe EdgeMatch (pairs of unlike direction are not compared,
    main.cpp:335-347), and all of them sit on the same ranges of both reads, so no two fillers are compatible
    (orientation 0 on both reads).  They are not primary (score < 500), so the primary filter of main.cpp:355-366 never
    drops a probe path for them.  They fill the edge into a width class of the chain kernels and leave the probe's
    chaining verdict as derived by hand."""
    out = [tuple(r) for r in rows]
    line = int(rows["line"].max()) + 1
    for k in range(n_fill):
        a = int(rows["anchor_id"].max()) + 1 + k
        out.append(row(a, 0, 9000, 0, 599, 6000, 6599, 450, line, True))
        out.append(row(a, 1, 9000, 0, 599, 6000, 6599, 440, line + 1, False))
        line += 2
    return np.array(out, dtype=ROW_DTYPE)


# EdgeMatches per edge in each width class of the chain kernels: <= 8, 9-16, 17-32, 33-64 (sub-wavefront and wavefront
# bodies), 65-256 (k_chain_big, LDS) and > 256 (k_chain_big, global memory)
PAD_FILL = {"w8": 4, "w16": 12, "w32": 28, "w64": 60, "w256": 200, "wbig": 300}


def chained(t):
    """Is there an order whose path holds both probe anchors (0 and 1)?  -- the chaining verdict, read off the ids."""
    o = t["orders"]
    return any({0, 1} <= set(int(x) for x in t["ids"][int(q["ids_off"]): int(q["ids_off"]) + int(q["ids_cnt"])]) for q in o)


def single_paths(t):
    """The set of one-anchor paths among the orders (anchor ids)."""
    return {int(t["ids"][int(q["ids_off"])]) for q in t["orders"] if int(q["ids_cnt"]) == 1}


def params(oracle, **kw):
    p = oracle.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# (name, rows, msgpu_params fields, expected chaining verdict of the probe)
PARAM_CASES = []
for _w in (0, 1, 7, 299, 301, 1000):
    # ratio 0: only diff == 0 passes the ratio rule, so the wiggle rule alone decides; d1 = 2002
    PARAM_CASES.append(("wiggle%d_eq" % _w, case_gaps(2002, 2002 + _w), dict(wiggle_room=_w, ratio_pct=0.0), True))
    PARAM_CASES.append(("wiggle%d_over" % _w, case_gaps(2002, 2003 + _w), dict(wiggle_room=_w, ratio_pct=0.0), False))
PARAM_CASES += [
    # 500 * 100 / 2000 == 25.0 exactly in fp64: <= 25 chains; 501 * 100 / 2000 = 25.05 does not (wiggle 0 rules itself out)
    ("ratio25_eq", case_gaps(2000, 1500), dict(wiggle_room=0, ratio_pct=25.0), True),
    ("ratio25_over", case_gaps(2000, 1499), dict(wiggle_room=0, ratio_pct=25.0), False),
    ("ratio25_eq_swapped", case_gaps(1500, 2000), dict(wiggle_room=0, ratio_pct=25.0), True),
    # the ratio rule beyond wiggle 300: 375 * 100 / 5000 == 7.5 exactly; and at ratio 0 a diff of 301 (13 %) no longer chains
    ("w300_ratio7.5_eq", case_gaps(5000, 4625), dict(wiggle_room=300, ratio_pct=7.5), True),
    ("w300_ratio7.5_over", case_gaps(5000, 4624), dict(wiggle_room=300, ratio_pct=7.5), False),
    ("w300_ratio0_eq", case_gaps(2002, 2302), dict(wiggle_room=300, ratio_pct=0.0), True),
    ("w300_ratio0_over", case_gaps(2002, 2303), dict(wiggle_room=300, ratio_pct=0.0), False),
    # mixed pair: d1 + d2 == wiggle chains, one more does not -- at any ratio (100 % would pass every same-orientation pair)
    ("mixed300_eq", case_mixed(100, 200), dict(wiggle_room=300, ratio_pct=100.0), True),
    ("mixed300_over", case_mixed(100, 201), dict(wiggle_room=300, ratio_pct=100.0), False),
    ("mixed50_eq", case_mixed(20, 30), dict(wiggle_room=50, ratio_pct=100.0), True),
    ("mixed50_over", case_mixed(21, 30), dict(wiggle_room=50, ratio_pct=100.0), False),
]

# alternatives (mpp.cpp:223-249): two incompatible single-anchor paths (diff 2002 against 5000: 59.96 % apart) with
# EdgeMatch scores `best` and `alt`; the second one is an alternative iff alt > alt_frac * best (strictly)
ALT_CASES = [  # (name, best, alt, alt_frac, taken)
    ("alt075_eq", 2400, 1800, 0.75, False), ("alt075_over", 2400, 1801, 0.75, True),
    ("alt050_eq", 2400, 1200, 0.5, False), ("alt050_over", 2400, 1201, 0.5, True),
    ("alt000", 2400, 1000, 0.0, True), ("alt100", 2400, 2399, 1.0, False),
]


def case_alt(best, alt):
    return case_gaps(2002, 5000, (best // 2, best - best // 2, alt // 2, alt - alt // 2))


def test_param_cases_arithmetic():
    """The boundaries above in the reference's own fp64 arithmetic (mpp.cpp:133-139, :223)."""
    assert 500.0 * 100 / 2000.0 == 25.0 and 501.0 * 100 / 2000.0 > 25.0
    assert 375.0 * 100 / 5000.0 == 7.5 and 376.0 * 100 / 5000.0 > 7.5 and 301.0 * 100 / 2303.0 <= 15
    assert 2400.0 * 0.75 == 1800.0 and 2400.0 * 0.5 == 1200.0
    assert 2998.0 * 100 / 5000.0 > 15.0


@pytest.mark.parametrize("fill", [0] + sorted(PAD_FILL.values()))
@pytest.mark.parametrize("name,rows,kw,want", PARAM_CASES, ids=[c[0] for c in PARAM_CASES])
def test_param_cases_oracle(oracle, name, rows, kw, want, fill):
    t = oracle.overlap(pad(rows, fill), params(oracle, **kw))
    assert len(t["edges"]) == 1 and int(t["edges"]["em_cnt"][0]) == 2 + fill
    assert chained(t) == want
    if fill == 0 and want:
        assert list(t["ids"]) == [0, 1] and len(t["orders"]) == 1
    if fill == 0 and not want:  # two single-anchor paths, both kept (1110 > 0.75 * 1150)
        assert len(t["orders"]) == 2 and single_paths(t) == {0, 1} and t["edges"]["shadow"][0] == 1


@pytest.mark.parametrize("fill", [0] + sorted(PAD_FILL.values()))
@pytest.mark.parametrize("name,best,alt,frac,taken", ALT_CASES, ids=[c[0] for c in ALT_CASES])
def test_alt_cases_oracle(oracle, name, best, alt, frac, taken, fill):
    t = oracle.overlap(pad(case_alt(best, alt), fill), params(oracle, alt_frac=frac))
    assert [float(s) for s in t["ems"]["score"][:2]] == [float(best), float(alt)]
    assert not chained(t)
    assert (1 in single_paths(t)) == taken and 0 in single_paths(t)
