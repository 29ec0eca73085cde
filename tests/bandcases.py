"""Row tables for the banded pair sweep of the chain kernels ("the band"), and the rule itself in
plain Python over ms_oracle_py.check_compatibility.

The band: sweep and DP run over the pairs (k, l) with l - B <= k < l only; with pmax[j] = max(pop[0..j]) row l > B is
accepted when pmax[l - B - 1] + s[l] < pop[l] (strictly, a NaN rejects); an edge with a rejected row is done again with
the full sweep.  Rows are ALL EdgeMatches of an edge in v1's order (the kernels' lanes): pairs of different directions are
incompatible, the prefix maximum runs over both directions.

Every table takes the Registry ids in first-line order; edge e lies between reads 2e and 2e + 1; every row covers its
whole unitig range, so an EdgeMatch score is the sum of its two row scores and the corrected ranges are the raw ones
(except the absorbed family's tiny anchor, built as extremecases._tie_edge builds it).

  gap_rows:      a chain, then G rows off it (8000 bases further on the second read, or on its other strand: "both"),
                 then the chain goes on: the rows behind the gap need a predecessor outside the band.  G = B + 1, and
                 B at n = B + 2 (one chain row on either side: the last row's band is exactly the gap).
  tie_rows:      two chains X and Y of m >= B rows each, one after the other in v1's order, of equal scores and mutually
                 incompatible; then a row FAR behind both, compatible with every row of either (with Y's by the ratio rule):
                 the last row of Y (in the band) and the last row of X (outside it) give the same sum bit for bit, every
                 score in the band is the true one, and the reference keeps the smaller k -- only the strict < rejects.
  flat_rows:     chains along which pop does not grow: every score 0; one tiny score among 2^33 - 2 (absorbed by the sum).
                 One row off the chain keeps the all-pairs-compatible shortcut away.
"""
import numpy as np

from muchsalsa_amd.synth import ROW_DTYPE

STEP = 800
OFF = 8000  # off the chain on the second read: incompatible by wiggle room, and by the ratio rule below 45 kb gaps
BIG = 2 ** 32 - 1
TINY_SPAN = 70_000_000
FAR = 60_000  # a gap of more than 8000 * 100 / 15 bases: the ratio rule accepts an 8000-base difference


def row(anchor, read, read_len, i_lo, i_hi, n_lo, n_hi, score, line, plus):
    prim = (i_hi - i_lo + 1) >= 500 and score >= 500  # BlastFileReader.cpp:121-122
    return (anchor, read, read_len, i_lo, i_hi, n_lo, n_hi, score, line, (1 if plus else 0) | (2 if prim else 0))


class _Table:
    def __init__(self):
        self.out, self.anchor, self.line, self.read = [], 0, 0, 0

    def edge(self, places, scores=None):
        """places: per anchor (position on read0, position on read1, plus) -- one EdgeMatch each, 600 bases wide"""
        n = len(places)
        L = 4000 + STEP * n + 2 * OFF + FAR
        for j, (p0, p1, plus) in enumerate(places):
            s0, s1 = scores[j] if scores else (560, 540)
            q1 = p1 if plus else L - 600 - p1
            self.out.append(row(self.anchor + j, self.read, L, 0, 599, p0, p0 + 599, s0, self.line, True))
            self.out.append(row(self.anchor + j, self.read + 1, L, 0, 599, q1, q1 + 599, s1, self.line + 1, plus))
            self.line += 2
        self.anchor += n
        self.read += 2

    def rows(self):
        return np.array(self.out, dtype=ROW_DTYPE)


def gap_sizes(B):
    return sorted({B + 2, 32, 33, 48, 64})


def gap_len(n, B):
    return min(B + 1, n - 2)


def gap_rows(B, sizes=None):
    """per size an edge of one direction and one of both; -> (rows, [n per edge])"""
    t, ns = _Table(), []
    for n in sizes or gap_sizes(B):
        assert n >= B + 2
        G = gap_len(n, B)
        a = max(1, (n - G) // 2)
        for both in (False, True):
            places = []
            for j in range(n):
                gap = a <= j < a + G
                if gap and both:
                    places.append((500 + STEP * j, 700 + STEP * j, False))  # a chain of its own on the other strand
                else:
                    places.append((500 + STEP * j, 700 + STEP * j + (OFF if gap else 0), True))
            t.edge(places)
            ns.append(n)
    return t.rows(), ns


def tie_sizes(B):
    return sorted({2 * B + 1, max(33, 2 * B + 1), 48, 64})


def tie_rows(B, sizes=None):
    """-> (rows, [n per edge], [(edge, lane of the out-of-band twin, lane of the in-band twin, lane of the tied row)])"""
    t, ns, where = _Table(), [], []
    for e, n in enumerate(sizes or tie_sizes(B)):
        m = (n - 1) // 2
        assert m >= B and n <= 64
        places = []
        for j in range(n):
            if j < m:  # X
                places.append((500 + STEP * j, 700 + STEP * j, True))
            elif j < 2 * m:  # Y: off X by wiggle room and by the ratio rule (gaps below 53 kb)
                places.append((500 + STEP * j, 700 + STEP * j + OFF, True))
            else:  # the tied row (and one behind it for an even n): FAR behind both, compatible with X by wiggle room, with Y by ratio
                places.append((500 + STEP * j + FAR, 700 + STEP * j + FAR, True))
        t.edge(places)
        ns.append(n)
        where.append((e, m - 1, 2 * m - 1, 2 * m))
    return t.rows(), ns, where


def flat_sizes(B):
    return sorted({B + 2, 32, 33, 64})


def flat_rows(B, sizes=None):
    """per size: a zero-score chain, and a chain of large scores with one tiny anchor behind at least three large ones
    (extremecases._tie_edge's recipe); each with one anchor off the chain.  -> (rows, [n per edge])"""
    t, ns = _Table(), []
    for n in sizes or flat_sizes(B):
        off_at = n // 3
        places = [(500 + STEP * j, 700 + STEP * j + (OFF if j == off_at else 0), True) for j in range(n)]
        t.edge(places, [(0, 0)] * n)
        ns.append(n)
        # the absorbed score: anchor n - 3 tiny
        L = 4000 + STEP * n + 2 * OFF
        tiny = n - 3
        for j in range(n):
            p = 500 + STEP * j
            q = p + 200 + (OFF if j == off_at else 0)
            if j == tiny:
                t.out.append(row(t.anchor + j, t.read, L, 0, TINY_SPAN - 1, p, p + 599, 1, t.line, True))
                t.out.append(row(t.anchor + j, t.read + 1, L, 0, 102, q, q, 0, t.line + 1, True))
            else:
                t.out.append(row(t.anchor + j, t.read, L, 0, 599, p, p + 599, BIG, t.line, True))
                t.out.append(row(t.anchor + j, t.read + 1, L, 0, 599, q, q + 599, BIG, t.line + 1, True))
            t.line += 2
        t.anchor += n
        t.read += 2
        ns.append(n)
    return t.rows(), ns


# ---- the rule -------------------------------------------------------------------------------------------------------
def match_map(rows):
    import ms_oracle_py as P
    mm = P.MatchMap()
    for r in sorted(({k: int(r[k]) for k in ROW_DTYPE.names} for r in rows), key=lambda r: r["line"]):
        mm.add_row(r)
    mm.calculate_edges()
    return mm


def edge_lanes(mm, key):
    """the EdgeMatches of an edge as the chain kernels' lanes hold them: v1's order (nanopore range, then id), both
    directions together.  -> (ids, scores, directions)"""
    ems = mm.edge_matches[key]
    vs = sorted((mm.vertex_matches[key[0]][i].nano, i) for i in ems)
    ids = [i for _, i in vs]
    return ids, [ems[i].score for i in ids], [ems[i].direction for i in ids]


def compat_matrix(mm, key, ids, dirs, wiggle=300, ratio_pct=15):
    import ms_oracle_py as P
    n, edge = len(ids), mm.edges[key]
    C = [[False] * n for _ in range(n)]
    for l in range(n):
        for k in range(l):
            C[k][l] = dirs[k] == dirs[l] and P.check_compatibility(mm, edge, ids[k], ids[l], wiggle, ratio_pct)
    return C


def dp(C, s, B=None):
    """the chaining DP of mpp.cpp:181-199 in increasing k with a strict >, over the band (B) or over every pair (None)
    -> (pop, pred, every row accepted by the rule)"""
    n = len(s)
    pop, pred, ok, pm = list(s), [-1] * n, True, []
    for l in range(n):
        lo = 0 if B is None else max(0, l - B)
        for k in range(lo, l):
            if C[k][l] and pop[k] + s[l] > pop[l]:
                pop[l], pred[l] = pop[k] + s[l], k
        if B is not None and lo > 0 and not (pm[lo - 1] + s[l] < pop[l]):
            ok = False
        pm.append(pop[l] if l == 0 else max(pm[-1], pop[l]))
    return pop, pred, ok
