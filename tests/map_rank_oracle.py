"""Rule 12 of the mapper (include/msgpu.h, "unitig-to-read mapping"), restated in plain Python on a chain table: primaries,
secondaries, parents, sub, n_secondary and the integer mapping quality, the counts of msgpu_map_rstats, and the ranked PAF made
from an unranked one.  Integers only.  A chain is the tuple of msgpu_map_chain: (query, target, strand, n_anchors, score, nm,
q_start, q_end, t_start, t_end, matches, block)."""

LDS = 512  # MSGPU_MAP_RANK_LDS: the primaries of a list segment that stay in LDS
WAVE = 64  # the largest segment of the wavefront class
STATS = ("n_segments", "n_primaries", "n_secondaries", "n_mapq0", "largest_segment", "n_segments_single", "n_segments_wave",
         "n_segments_list", "n_segments_spilled")

Q, ANCHORS, SCORE, QS, QE = 0, 3, 4, 6, 7


class RankError(ValueError):
    """a table that rule 12 rejects; ``chain`` is the first bad chain"""

    def __init__(self, chain, what):
        super().__init__("chain %d: %s" % (chain, what))
        self.chain = chain


def check(chains):
    for i, c in enumerate(chains):
        if c[QS] > c[QE]:
            raise RankError(i, "q_start > q_end")
        if i and c[Q] < chains[i - 1][Q]:
            raise RankError(i, "query record")


def segments(chains):
    """[(first, end)] of the maximal runs of one query record"""
    out, first = [], 0
    for i in range(1, len(chains) + 1):
        if i == len(chains) or chains[i][Q] != chains[first][Q]:
            if i > first:
                out.append((first, i))
            first = i
    return out


def masks(c, p):
    """12.2: does primary p make c secondary"""
    ov = max(0, min(c[QE], p[QE]) - max(c[QS], p[QS]))
    return 2 * ov > min(c[QE] - c[QS], p[QE] - p[QS])


def mapq(s1, sub, n_anchors):
    if s1 <= 0:
        return 0
    return max(0, min(60, (60 * (s1 - sub) * min(n_anchors, 10)) // (10 * s1)))  # (s1 >= sub: the quotient is not negative)


def rank(chains, base=0):
    """-> per chain (parent, sub, n_secondary, mapq); ``base`` is added to every parent"""
    check(chains)
    parent = list(range(len(chains)))
    for first, end in segments(chains):
        primaries = []
        for i in sorted(range(first, end), key=lambda j: (-chains[j][SCORE], j)):  # 12.1
            parent[i] = next((p for p in primaries if masks(chains[i], chains[p])), i)
            if parent[i] == i:
                primaries.append(i)
    rows = [None if p == i else (base + p, 0, 0, 0) for i, p in enumerate(parent)]  # 12.3: zeros for a secondary
    kids = {}
    for i, p in enumerate(parent):
        if p != i:
            kids.setdefault(p, []).append(chains[i][SCORE])
    for i, c in enumerate(chains):
        if rows[i] is None:
            s = kids.get(i, [])
            sub = max(s) if s else 0
            rows[i] = (base + i, sub, sum(1 for x in s if 10 * x >= 9 * c[SCORE]), mapq(c[SCORE], sub, c[ANCHORS]))
    return rows


def stats(chains, rows, base=0):
    seg = segments(chains)
    sizes = [e - f for f, e in seg]
    prim = [r[0] == base + i for i, r in enumerate(rows)]
    return {"n_segments": len(seg), "n_primaries": sum(prim), "n_secondaries": len(rows) - sum(prim),
            "n_mapq0": sum(1 for r in rows if r[3] == 0), "largest_segment": max(sizes, default=0),
            "n_segments_single": sum(1 for n in sizes if n == 1), "n_segments_wave": sum(1 for n in sizes if 2 <= n <= WAVE),
            "n_segments_list": sum(1 for n in sizes if n > WAVE),
            "n_segments_spilled": sum(1 for f, e in seg if e - f > WAVE and sum(prim[f:e]) > LDS)}


def invariants(chains, rows):
    """a parent is a primary of the same query; sub <= score(parent); secondaries carry zeros"""
    for i, (p, sub, n_sec, q) in enumerate(rows):
        assert 0 <= p < len(chains) and rows[p][0] == p and chains[p][Q] == chains[i][Q]
        assert 0 <= q <= 60
        if p != i:
            assert (sub, n_sec, q) == (0, 0, 0)
            assert chains[i][SCORE] <= rows[p][1] <= chains[p][SCORE]
            assert (chains[i][SCORE], -i) < (chains[p][SCORE], -p)  # the parent was visited first
        else:
            assert sub <= chains[i][SCORE] or n_sec == 0 and sub == 0
            if chains[i][SCORE] <= 0:
                assert q == 0


def ranked_paf(paf, rows, base=0):
    """12.5 on the lines of an unranked PAF: column 12 and the tags tp and s2"""
    lines = paf.split(b"\n")
    assert lines.pop() == b"" and len(lines) == len(rows)
    out = []
    for i, (line, r) in enumerate(zip(lines, rows)):
        f = line.split(b"\t")
        assert f[11] == b"255" and f[12].startswith(b"cm:i:") and f[13].startswith(b"s1:i:")
        f[11] = b"%d" % r[3]
        f[12:14] = [b"tp:A:P" if r[0] == base + i else b"tp:A:S", f[12], f[13], b"s2:i:%d" % r[1]]
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)
