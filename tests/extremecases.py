"""Row tables at the corners of the chain kernels: ill-formed nanopore ranges, fp64 ties in the chaining DP, zero scores,
exact alternative-path thresholds and coordinates, lengths and scores near the integer limits.

Every table takes the Registry ids in first-line order (reads and anchors are numbered as their first rows appear), as
test_gpu_chain_classes._edge does.  Edge e lies between reads 2e and 2e + 1.  Every builder asserts that none of the
reference's own int32 expressions (i_hi - i_lo + 1, n_hi - n_lo + 1, len - n_hi, ov_hi - ov_lo) overflows: that would
be undefined behaviour, with no answer to match.

The families of the chain kernels' corners:
  (a) rows_of(ill_formed_specs()): "point" (n_hi = n_lo - 1), "reversed" (n_hi < n_lo - 1) and "beyond"
                         (n_hi >= read_len or n_lo < 0) ranges, one bad element among clean ones or every element bad,
                         one strand or both, at every width-class bound; bug_a_rows: the mixed pair whose signed diff
                         sum chains it; subwave_mix_rows: wavefronts of k_chain_sub whose groups are well formed and ill
                         formed in turn
  (b) shortcut_tie_rows: one-strand edges the all-pairs-compatible shortcut accepts, holding an fp64 tie of the DP
  (c) ties_rows:         equal EdgeMatch scores with twin predecessors, all-zero scores, an alternative path whose
                         population equals max * alt_frac exactly
  (d) magnitude_rows:    shortcut bounds av / bv just inside and outside +-1e9, coordinates near +-2^30, read length
                         2^31 - 1, scores 2^30 - 1 .. 2^32 - 1
"""
import math

import numpy as np

from muchsalsa_amd.synth import ROW_DTYPE

BOUNDS = (2, 8, 9, 16, 17, 32, 33, 64, 65, 256, 257)
KINDS = ("point", "reversed", "beyond")
I32 = 2 ** 31 - 1
STEP = 800  # anchor spacing on both reads
# the shortcut's guards (k_chain / k_chain_sub): |av|, |bv| below AV_LIMIT and every EdgeMatch score above SCORE_FLOOR
AV_LIMIT = 1.0e9
SCORE_FLOOR = 1.0e-6


def row(anchor, read, read_len, i_lo, i_hi, n_lo, n_hi, score, line, plus):
    prim = (i_hi - i_lo + 1) >= 500 and score >= 500  # BlastFileReader.cpp:121-122
    return (anchor, read, read_len, i_lo, i_hi, n_lo, n_hi, score, line, (1 if plus else 0) | (2 if prim else 0))


def _fits(x):
    return -2 ** 31 <= x <= I32


def check_int32(rows):
    """none of the reference's int32 expressions overflows on this table"""
    by_anchor = {}
    for r in rows:
        i_lo, i_hi, n_lo, n_hi, ln = (int(r[k]) for k in ("i_lo", "i_hi", "n_lo", "n_hi", "read_len"))
        assert _fits(i_hi - i_lo + 1) and _fits(n_hi - n_lo + 1) and _fits(ln - n_hi), tuple(r)
        lo, hi = by_anchor.get(int(r["anchor_id"]), (i_lo, i_hi))
        by_anchor[int(r["anchor_id"])] = (min(lo, i_lo), max(hi, i_hi))
    for lo, hi in by_anchor.values():  # ov_hi - ov_lo over any two rows of one anchor lies within these bounds
        assert _fits(hi - lo) and _fits(lo - hi)
    return rows


def join(parts):
    """row tables of disjoint read / anchor / line spaces, one after the other (ids stay in first-line order)"""
    out, r0, a0, l0 = [], 0, 0, 0
    for p in parts:
        p = p.copy()
        p["read_id"] += r0
        p["anchor_id"] += a0
        p["line"] += l0
        r0, a0, l0 = int(p["read_id"].max()) + 1, int(p["anchor_id"].max()) + 1, int(p["line"].max()) + 1
        out.append(p)
    return check_int32(np.concatenate(out))


# ---- (a) ill-formed edges -------------------------------------------------------------------------------------------
def _spoil(r, kind, L, rng):
    """r = [n_lo, n_hi] of one row, made ill formed in place"""
    if kind == "point":
        r[1] = r[0] - 1
    elif kind == "reversed":  # short and long reversals: a short one nested in a neighbour gives a negative diff
        w = int(rng.choice([2, 5, 40, 300, 599]))
        r[0], r[1] = r[0] + w, r[0]
    else:  # beyond: past the read's end, or in front of its start (negative overhangs and order offsets)
        if rng.random() < 0.5:
            r[1] = L + int(rng.integers(0, 400))
        else:
            r[0] = -int(rng.integers(1, 700))


def _edge(out, n, read0, anchor0, line0, rng, strands="one", kind=None, spread="one"):
    """rows of one edge: reads read0 and read0 + 1 share n anchors (one EdgeMatch each).  strands "both": about a third of
    the anchors on the other strand of the second read.  kind (see KINDS) spoils the nanopore range of one row of one
    element (spread "one") or of every element (spread "all")"""
    L = 2000 + STEP * n
    bad = set(range(n)) if spread == "all" else {int(rng.integers(0, n))}
    line = line0
    for j in range(n):
        p0 = 500 + STEP * j
        p1 = 700 + STEP * j + int(rng.integers(-60, 61))
        u = rng.random()
        if u < 0.2:
            p1 += int(rng.integers(-1500, 1501))  # far off the chain: incompatible with most
        elif u < 0.35 and j > 0:
            p1 = 700 + STEP * (j - 1)  # on its neighbour's range: contained, orientation 0
        p1 = min(max(p1, 0), L - 600)
        plus = not (strands == "both" and rng.random() < 0.35)
        if not plus:
            p1 = L - 600 - p1
        i_lo = int(rng.integers(0, 40))
        r0, r1 = [p0, p0 + 599], [p1, p1 + 599 - i_lo]
        if kind is not None and j in bad:
            _spoil(r0 if rng.random() < 0.5 else r1, kind, L, rng)
        s0, s1 = int(rng.integers(440, 620)), int(rng.integers(440, 620))
        out.append(row(anchor0 + j, read0, L, 0, 599, r0[0], r0[1], s0, line, True))
        out.append(row(anchor0 + j, read0 + 1, L, i_lo, 599, r1[0], r1[1], s1, line + 1, plus))
        line += 2
    return line


def rows_of(specs, seed):
    """one row table: an edge per spec (n, strands, kind, spread), each on a pair of reads of its own"""
    rng = np.random.default_rng(seed)
    out, anchor, line = [], 0, 0
    for e, (n, strands, kind, spread) in enumerate(specs):
        line = _edge(out, n, 2 * e, anchor, line, rng, strands, kind, spread)
        anchor += n
    return check_int32(np.array(out, dtype=ROW_DTYPE))


def ill_formed_specs(sizes=BOUNDS):
    return [(n, strands, kind, spread) for n in sizes for kind in KINDS for spread in ("one", "all")
            for strands in ("one", "both")]


def bug_a_rows():
    """The mixed pair of k_chain's former |d1 + d2| test.  Both anchors cover their whole unitig range on both rows, so
    the corrected ranges equal the raw ones (every correction is 0 / rRatio).  Vertex 1 (read 0): K = [7, 1000],
    L = [10, 5] (a reversed row); vertex 2 (read 1): K = [3000, 3599], L = [3500, 4099]."""
    return np.array([row(0, 0, 9000, 0, 599, 7, 1000, 550, 0, True),
                     row(0, 1, 9000, 0, 599, 3000, 3599, 560, 1, True),
                     row(1, 0, 9000, 0, 599, 10, 5, 540, 2, True),
                     row(1, 1, 9000, 0, 599, 3500, 4099, 530, 3, True)], dtype=ROW_DTYPE)


def bug_a_verdict(wiggle):
    """checkCompatibility(K, L) by hand (mpp.cpp:67-91, 133-139): vertex 1 -- the ranges do not overlap (7 <= 5 fails)
    and K starts first, orientation +1, diff 10 - 1000 + 1 = -989; the raw ranges do not overlap either: no abort.
    Vertex 2 -- they overlap in order, orientation +2, diff 3599 - 3500 + 1 = 100; raw order agrees.  Orientations +1
    and +2: the mixed rule, diff1 + diff2 <= wiggle."""
    d1, d2 = 10.0 - 1000.0 + 1, 3599.0 - 3500.0 + 1
    assert (d1, d2, d1 + d2) == (-989.0, 100.0, -889.0)
    return d1 + d2 <= float(wiggle)


def subwave_mix_rows(seed):
    """edges of k_chain_sub's classes (2..32) where well-formed and ill-formed edges of one size alternate, so that the
    groups of one wavefront differ in it"""
    specs = []
    for n in (2, 3, 5, 8, 9, 12, 16, 17, 24, 32):
        for r in range(8):
            specs.append((n, ("one", "both")[r // 2 % 2], None if r % 2 == 0 else KINDS[r // 2 % 3], "one"))
    return rows_of(specs, seed)


# ---- per-EdgeMatch arithmetic of the reference, for the workloads' coverage claims ------------------------------------
def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def elements(rows, tables):
    """per edge of an overlap result (canonical order): its EdgeMatches in v1's order as dicts with the corrected and raw
    nanopore ranges on both vertices (mpp.cpp:48-65), the direction and the score"""
    first = {}
    for r in sorted(rows, key=lambda r: int(r["line"])):
        first.setdefault((int(r["read_id"]), int(r["anchor_id"])), r)
    out = []
    for e in tables["edges"]:
        ems = tables["ems"][int(e["em_off"]):int(e["em_off"]) + int(e["em_cnt"])]
        els = []
        for m in ems:
            d = dict(dir=bool(int(m["flags"]) & 1), score=float(m["score"]), anchor=int(m["anchor_id"]))
            for v, s in ((int(e["v1"]), "1"), (int(e["v2"]), "2")):
                r = first[(v, int(m["anchor_id"]))]
                rr = _div(float(int(r["i_hi"]) - int(r["i_lo"]) + 1), float(int(r["n_hi"]) - int(r["n_lo"]) + 1))
                ncl = _div(float(int(m["ov_lo"]) - int(r["i_lo"])), rr)
                ncr = _div(float(int(r["i_hi"]) - int(m["ov_hi"])), rr)
                if not int(r["flags"]) & 1:
                    ncl, ncr = ncr, ncl
                d["clo" + s], d["chi" + s] = float(int(r["n_lo"])) + ncl, float(int(r["n_hi"])) - ncr
                d["rlo" + s], d["rhi" + s] = int(r["n_lo"]), int(r["n_hi"])
            els.append(d)
        out.append(els)
    return out


def _nano(c1, c2, r1, r2):
    """nanoCheck (mpp.cpp:67-109) -> (orientation, diff, abort)"""
    o, d = 0, 0.0
    if c1[0] <= c2[1] and c2[0] <= c1[1]:
        if c1[0] < c2[0] and c1[1] < c2[1]:
            o, d = 2, c1[1] - c2[0] + 1
        if c1[0] > c2[0] and c1[1] > c2[1]:
            o, d = -2, c2[1] - c1[0] + 1
    elif c1[0] < c2[0]:
        o, d = 1, c2[0] - c1[1] + 1
    else:
        o, d = -1, c1[0] - c2[1] + 1
    uco = 0
    if r1[0] <= r2[1] and r2[0] <= r1[1]:
        if r1[0] < r2[0] and r1[1] < r2[1]:
            uco = 2
        if r1[0] > r2[0] and r1[1] > r2[1]:
            uco = -2
        if (o < 0 and uco >= 0) or (o > 0 and uco <= 0):
            return o, d, True
    return o, d, False


def pair_terms(K, L):
    """(orientation1, diff1, orientation2 after the flip of mpp.cpp:131, diff2, abort) of checkCompatibility(K, L)"""
    o1, d1, a1 = _nano((K["clo1"], K["chi1"]), (L["clo1"], L["chi1"]), (K["rlo1"], K["rhi1"]), (L["rlo1"], L["rhi1"]))
    o2, d2, a2 = _nano((K["clo2"], K["chi2"]), (L["clo2"], L["chi2"]), (K["rlo2"], K["rhi2"]), (L["rlo2"], L["rhi2"]))
    return o1, d1, (o2 if K["dir"] else -o2), d2, a1 or a2


def ill_formed(el):
    return el["clo1"] > el["chi1"] or el["clo2"] > el["chi2"]


def width_class(n):
    return next(i for i, b in enumerate((8, 16, 32, 64, 256)) if n <= b) if n <= 256 else 5


def coverage_a(rows, tables, wiggle, max_n=64):
    """(edges with an ill-formed corrected range per width class, mixed pairs of edges of <= max_n EdgeMatches that are
    not aborted and have diff1 + diff2 < -wiggle: the reference chains them, |d1 + d2| <= wiggle would not)"""
    per_class, neg_mixed = [0] * 6, 0
    for els in elements(rows, tables):
        if not any(ill_formed(x) for x in els):
            continue
        per_class[width_class(len(els))] += 1
        if len(els) > max_n:
            continue
        for k in range(len(els)):
            for l in range(k + 1, len(els)):
                if els[k]["dir"] != els[l]["dir"]:
                    continue
                o1, d1, o2, d2, ab = pair_terms(els[k], els[l])
                if not ab and o1 != o2 and o1 * o2 > 0 and d1 + d2 < -float(wiggle):
                    neg_mixed += 1
    return per_class, neg_mixed


# ---- (b) shortcut ties ----------------------------------------------------------------------------------------------
BIG = 2 ** 32 - 1  # row score of the large anchors: EdgeMatch score 2^33 - 2
TINY_SPAN = 70_000_000  # unitig bases of the tiny anchor's row of score 1


def _tie_edge(out, n, t, read0, anchor0, line0, tiny):
    """a one-strand edge of n anchors, all on the chain (every pair compatible).  Anchor t is the tiny one (tiny=True):
    on read0 a row of score 1 over TINY_SPAN unitig bases, on read0 + 1 a row of score 0 that overlaps it by 102 bases,
    so its EdgeMatch score is 103 / 7e7 ~ 1.47e-6.  Its nanopore ranges keep both reads' corrected and raw ranges
    strictly increasing and its shortcut terms av, bv next to everybody's -200."""
    L = 2000 + STEP * n
    line = line0
    for j in range(n):
        p = 500 + STEP * j
        if tiny and j == t:
            out.append(row(anchor0 + j, read0, L, 0, TINY_SPAN - 1, p, p + 599, 1, line, True))
            out.append(row(anchor0 + j, read0 + 1, L, 0, 102, p + 200, p + 200, 0, line + 1, True))
        else:
            out.append(row(anchor0 + j, read0, L, 0, 599, p, p + 599, BIG, line, True))
            out.append(row(anchor0 + j, read0 + 1, L, 0, 599, p + 200, p + 799, BIG, line + 1, True))
        line += 2
    return line


def shortcut_predicate(els, wiggle):
    """the all-pairs-compatible shortcut of k_chain / k_chain_sub, as the kernels state it: one direction, n >= 2,
    corrected and raw ranges strictly monotone along v1's order (increasing on v1; on v2 increasing for a forward edge,
    decreasing for a reverse one), |av|, |bv| < 1e9, every EdgeMatch score > 1e-6, and the integer bound
    max ceil(a) - min floor(b) <= min(wiggle, 2^40) - 3 (and with a, b swapped)"""
    if len(els) < 2 or len({x["dir"] for x in els}) != 1:
        return False
    plus = els[0]["dir"]
    for P, X in zip(els, els[1:]):
        ok = P["clo1"] < X["clo1"] and P["chi1"] < X["chi1"] and P["rlo1"] < X["rlo1"] and P["rhi1"] < X["rhi1"]
        if plus:
            ok &= P["clo2"] < X["clo2"] and P["chi2"] < X["chi2"] and P["rlo2"] < X["rlo2"] and P["rhi2"] < X["rhi2"]
        else:
            ok &= P["clo2"] > X["clo2"] and P["chi2"] > X["chi2"] and P["rlo2"] > X["rlo2"] and P["rhi2"] > X["rhi2"]
        if not ok:
            return False
    av = [x["clo1"] - x["clo2"] if plus else x["clo1"] + x["chi2"] for x in els]
    bv = [x["chi1"] - x["chi2"] if plus else x["chi1"] + x["clo2"] for x in els]
    if not all(-AV_LIMIT < v < AV_LIMIT for v in av + bv) or not all(x["score"] > SCORE_FLOOR for x in els):
        return False
    margin = min(int(wiggle), 2 ** 40) - 3
    return (max(math.ceil(v) for v in av) - min(math.floor(v) for v in bv) <= margin and
            max(math.ceil(v) for v in bv) - min(math.floor(v) for v in av) <= margin)


def all_compatible_dp(scores):
    """the DP of mpp.cpp:185-199 with every pair compatible: (populations, predecessor of each l or -1)"""
    pop, pred = list(scores), [-1] * len(scores)
    for k in range(len(scores)):
        for l in range(k + 1, len(scores)):
            s = pop[k] + scores[l]
            if s > pop[l]:
                pop[l], pred[l] = s, k
    return pop, pred


def has_tie(scores):
    """the DP leaves the left-to-right chain somewhere: an fp64 sum absorbed a score, the strict > kept the first k"""
    _, pred = all_compatible_dp(scores)
    return any(p != l - 1 for l, p in enumerate(pred) if l > 0)


def shortcut_tie_specs(sizes=tuple(range(3, 65)) + (65, 80, 130)):
    """(n, t): the tiny anchor at t behind at least three large ones, with at least one large anchor after it"""
    return [(n, t) for n in sizes for t in sorted({3, n // 2, n - 2}) if 3 <= t <= n - 2]


TIE_SCORES = (float(BIG) * 600.0 / 600.0 + float(BIG) * 600.0 / 600.0,  # MatchMap.cpp:196-202: outer + inner
              0.0 * 103.0 / 103.0 + 1.0 * 103.0 / float(TINY_SPAN))


def shortcut_tie_rows(specs):
    """per spec whose scores tie (has_tie) a tie edge and its control twin (the tiny anchor made large), the twin right
    behind it"""
    big, tiny = TIE_SCORES
    out, anchor, line, read = [], 0, 0, 0
    for n, t in specs:
        if not has_tie([tiny if j == t else big for j in range(n)]):
            continue
        for tiny in (True, False):
            line = _tie_edge(out, n, t, read, anchor, line, tiny)
            anchor += n
            read += 2
    return check_int32(np.array(out, dtype=ROW_DTYPE))


# ---- (c) ties and zeros ---------------------------------------------------------------------------------------------
def _twin_edge(out, n, read0, anchor0, line0, score, plus, rng):
    """n anchors of one EdgeMatch score: a chain on both reads, with every third anchor followed by a twin on the same
    nanopore ranges of both reads (the two are incompatible: orientation 0; each is compatible with the same others, so
    their populations are equal and the next anchor of the chain takes the first of them), and a few anchors far off
    the chain (incompatible).  Every row covers its whole unitig range: the score is s0 + s1 exactly."""
    L = 3000 + STEP * n
    line, j, pos = line0, 0, 0
    while j < n:
        reps = 2 if (pos % 3 == 1 and j + 1 < n) else 1
        p0 = 500 + STEP * pos
        p1 = 700 + STEP * pos
        if rng.random() < 0.15:
            p1 += 1500 + int(rng.integers(0, 400))
        p1 = min(p1, L - 600)
        q1 = p1 if plus else L - 600 - p1
        for _ in range(reps):
            out.append(row(anchor0 + j, read0, L, 0, 599, p0, p0 + 599, score[0], line, True))
            out.append(row(anchor0 + j, read0 + 1, L, 0, 599, q1, q1 + 599, score[1], line + 1, plus))
            line += 2
            j += 1
        pos += 1
    return line


def _alt_edge(out, m, q, read0, anchor0, line0, plus):
    """a main chain of m anchors and a side chain of q anchors 8000 bases off it on the second read (incompatible with
    the main chain, also by the ratio rule while no gap is much above 45 kb), every EdgeMatch score 1000: populations
    1000 m and 1000 q; with alt_frac = q / m the side chain's population
    equals the threshold max * alt_frac exactly (mpp.cpp:223-249 wants more)"""
    L = 4000 + STEP * (m + q) + 9000
    line = line0
    for j in range(m + q):
        p0 = 500 + STEP * j
        p1 = 700 + STEP * j if j < m else 700 + STEP * j + 8000
        q1 = p1 if plus else L - 600 - p1
        out.append(row(anchor0 + j, read0, L, 0, 599, p0, p0 + 599, 500, line, True))
        out.append(row(anchor0 + j, read0 + 1, L, 0, 599, q1, q1 + 599, 500, line + 1, plus))
        line += 2
    return line


def ties_rows(seed, sizes=BOUNDS):
    """per width-class bound and direction: an equal-score edge with twins, the same edge with every row of score 0;
    then main / side chains (m, q) = (4, 3), (8, 6), (2, 1) for alt_frac 0.75 and 0.5 in both directions"""
    rng = np.random.default_rng(seed)
    out, anchor, line, read = [], 0, 0, 0
    for n in sizes:
        for plus in (True, False):
            for score in ((560, 540), (0, 0)):
                line = _twin_edge(out, n, read, anchor, line, score, plus, rng)
                anchor, read = anchor + n, read + 2
    for m, q in ALT_CHAINS:
        for plus in (True, False):
            line = _alt_edge(out, m, q, read, anchor, line, plus)
            anchor, read = anchor + m + q, read + 2
    return check_int32(np.array(out, dtype=ROW_DTYPE))


ALT_CHAINS = ((4, 3), (8, 6), (2, 1), (20, 15), (48, 36))  # side / main = 0.75 or 0.5


def dp_populations(rows, tables, wiggle=300, ratio_pct=15.0):
    """per edge and direction the populations of the DP (mpp.cpp:181-199) through the Python restatement's
    checkCompatibility: [(edge index, direction, populations, tied)] where tied says that some l had two compatible
    predecessors with the same candidate score"""
    import ms_oracle_py as P
    mm = P.MatchMap()
    for r in sorted(({k: int(r[k]) for k in ROW_DTYPE.names} for r in rows), key=lambda r: r["line"]):
        mm.add_row(r)
    mm.calculate_edges()
    out = []
    for ei, e in enumerate(tables["edges"]):
        key = (int(e["v1"]), int(e["v2"]))
        edge, ems = mm.edges[key], mm.edge_matches[key]
        for direction in (False, True):
            ids = [i for i, m in ems.items() if m.direction == direction]
            if not ids:
                continue
            vs = sorted((mm.vertex_matches[key[0]][i].nano, i) for i in ids)
            pop = [ems[i].score for _, i in vs]
            tied = False
            for l in range(1, len(vs)):
                own = ems[vs[l][1]].score
                cands = [pop[k] + own for k in range(l) if P.check_compatibility(mm, edge, vs[k][1], vs[l][1], wiggle,
                                                                                   ratio_pct)]
                tied |= bool(cands) and max(cands) > own and cands.count(max(cands)) > 1
                for c in cands:
                    if c > pop[l]:
                        pop[l] = c
            out.append((ei, direction, pop, tied))
    return out


# ---- (d) magnitudes -------------------------------------------------------------------------------------------------
SCORES_D = (2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1, 2 ** 32 - 1)


def _shifted_edge(out, n, read0, anchor0, line0, base1, base2, len1, len2, plus, scores, rng):
    """a one-strand chain of n anchors on nanopore positions base1 + 800 j (read0) and base2 + 800 j (forward) or
    base2 - 800 j (reverse) on read0 + 1; whole unitig ranges, so av and bv are the same for every anchor"""
    line = line0
    for j in range(n):
        p0 = base1 + STEP * j
        p1 = base2 + STEP * j if plus else base2 - STEP * j
        s0, s1 = (int(rng.choice(scores)), int(rng.choice(scores)))
        out.append(row(anchor0 + j, read0, len1, 0, 599, p0, p0 + 599, s0, line, True))
        out.append(row(anchor0 + j, read0 + 1, len2, 0, 599, p1, p1 + 599, s1, line + 1, plus))
        line += 2
    return line


def magnitude_specs():
    """(n, base1, base2, len1, len2, plus): every anchor has av = bv = base1 - base2 on a forward edge and
    base1 + base2 + 599 on a reverse one"""
    specs = []
    for n in (2, 9, 33, 65):
        for off in (-50, 50):  # |av| just inside / just outside 1e9
            specs.append((n, 500_000_000, -500_000_000 + off, I32, 1_600_000_000, True))   # av = 1e9 - off
            specs.append((n, -500_000_000 + off, 500_000_000, 1_600_000_000, I32, True))    # av = -1e9 + off
            specs.append((n, 500_000_000, 500_000_000 - 599 - off, I32, I32, False))          # av = 1e9 - off
        specs.append((n, 2 ** 30 - 800 * n - 700, -2 ** 30, I32, 2 ** 30 - 1, True))       # coordinates near +-2^30
        specs.append((n, 2 ** 30 - 800 * n - 700, 2 ** 30 - 700, I32, I32, False))
        specs.append((n, 1000, 1200, I32, I32, True))                                     # read length 2^31 - 1
    return specs


def magnitude_rows(seed, specs=None, scores=SCORES_D):
    rng = np.random.default_rng(seed)
    out, anchor, line = [], 0, 0
    for e, (n, b1, b2, l1, l2, plus) in enumerate(specs or magnitude_specs()):
        line = _shifted_edge(out, n, 2 * e, anchor, line, b1, b2, l1, l2, plus, scores, rng)
        anchor += n
    return check_int32(np.array(out, dtype=ROW_DTYPE))


# ---- the loader's view: PAF text ------------------------------------------------------------------------------------
def paf_text(rows):
    """PAF lines of a row table (query = unitig "u<anchor>", target = read "r<read>"; columns 7 and 8 are n_lo and
    n_hi + 1 as given) plus the sentinel line the reference never parses.  Only rows the loader keeps belong here
    (score and query span >= 400)."""
    lines = []
    for r in sorted(rows, key=lambda r: int(r["line"])):
        i_lo, i_hi = int(r["i_lo"]), int(r["i_hi"])
        lines.append("u%d\t%d\t%d\t%d\t%s\tr%d\t%d\t%d\t%d\t%d\t%d\t60" % (
            int(r["anchor_id"]), i_hi + 1, i_lo, i_hi + 1, "+" if int(r["flags"]) & 1 else "-", int(r["read_id"]),
            int(r["read_len"]), int(r["n_lo"]), int(r["n_hi"]) + 1, int(r["score"]), i_hi + 1 - i_lo))
    lines.append("u0\t1\t0\t1\t+\tr0\t1\t0\t1\t0\t1\t0")
    return "\n".join(lines) + "\n"


def loader_rows(seed):
    """the part of (a) and (d) that a PAF file reaches: columns 7 and 8 equal (point), reversed or negative, scores up
    to 2^31 - 1 (the loader's int) -- every row with a query span and a score of at least 400"""
    a = rows_of([(n, s, k, sp) for n in (2, 9, 17, 33, 65) for k in KINDS for sp in ("one", "all")
                 for s in ("one", "both")], seed)
    d = magnitude_rows(seed + 1, scores=(400, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1))
    return join([a, bug_a_rows(), d])
