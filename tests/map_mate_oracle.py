"""Rule 13 of the mapper (include/msgpu.h, "unitig-to-read mapping"), restated in plain Python on a chain table: the concordant
combinations of a pair's chains, the selected one, n_best, the rows, the counts of msgpu_map_mstats, the PAF with the rule's tags
made from one without, rule 9's cut by pairs, and the invariants of a table of rows.  Integers only.  A chain is the tuple of
msgpu_map_chain: (query, target, strand, n_anchors, score, nm, q_start, q_end, t_start, t_end, matches, block)."""

NONE = 0xFFFFFFFF
EMPTY = (NONE, 0, 0, 0)
ANCHOR_BYTES, FIXED_BYTES = 60, 12 * 256  # MSGPU_MAP_MATES_ANCHOR_BYTES, MSGPU_MAP_MATES_FIXED_BYTES
STATS = ("n_pairs", "n_proper", "n_ambiguous", "n_discordant", "n_single", "n_unmapped", "n_pairs_settled", "n_pairs_lanes16",
         "n_pairs_lanes64", "n_pairs_list", "largest_pair", "tlen_sum", "tlen_min", "tlen_max")

Q, TARGET, STRAND, SCORE, TS, TE = 0, 1, 2, 4, 8, 9


class MateError(ValueError):
    """a table that rule 13 rejects; ``chain`` is the smallest bad chain, ``word`` the first violated condition"""

    def __init__(self, chain, word):
        super().__init__("chain %d: %s" % (chain, word))
        self.chain, self.word = chain, word


def check(chains):
    for i, c in enumerate(chains):
        if i and c[Q] < chains[i - 1][Q]:
            raise MateError(i, "order")
        if c[STRAND] > 1:
            raise MateError(i, "strand")
        if c[TS] > c[TE]:
            raise MateError(i, "range")


def segments(chains):
    """[(first, middle, end)] of the maximal runs of one pair (query >> 1): mate 1's chains are [first, middle)"""
    out, first = [], 0
    for i in range(1, len(chains) + 1):
        if i == len(chains) or chains[i][Q] >> 1 != chains[first][Q] >> 1:
            if i > first:
                out.append((first, first + sum(1 for c in chains[first:i] if not c[Q] & 1), i))
            first = i
    return out


def concordant(a, b, max_insert):
    """13.1 -> tl, or None"""
    if a[TARGET] != b[TARGET] or a[STRAND] == b[STRAND]:
        return None
    f, r = (b, a) if a[STRAND] else (a, b)
    if f[TS] > r[TS] or f[TE] > r[TE]:
        return None
    tl = r[TE] - f[TS]
    return tl if tl <= max_insert else None


def combinations(chains, seg, max_insert):
    """the concordant combinations of a segment as (-sum, tl, a, b): the smallest is 13.2's selection"""
    first, middle, end = seg
    out = []
    for a in range(first, middle):
        for b in range(middle, end):
            tl = concordant(chains[a], chains[b], max_insert)
            if tl is not None:
                out.append((-(chains[a][SCORE] + chains[b][SCORE]), tl, a, b))
    return out


def mates(chains, max_insert=1000, base=0, n_records=None):
    """-> (per chain (mate, tlen, cls, n_best), the counts); ``base`` is added to every mate.  n_records: the query records of
    the run (the pairs without a chain are unmapped); None: a table, which knows the pairs with a chain only"""
    check(chains)
    assert 1 <= max_insert < 1 << 31
    rows = [EMPTY] * len(chains)
    segs = segments(chains)
    st = dict.fromkeys(STATS, 0)
    tls = []
    for seg in segs:
        first, middle, end = seg
        n1, n2 = middle - first, end - middle
        st["largest_pair"] = max(st["largest_pair"], end - first)
        if not n1 or not n2:
            st["n_single"] += 1
            st["n_pairs_settled"] += 1
            continue
        st["n_pairs_settled" if n1 == n2 == 1 else "n_pairs_lanes16" if end - first <= 16 else "n_pairs_lanes64" if end - first <= 64
           else "n_pairs_list"] += 1
        combos = combinations(chains, seg, max_insert)
        if not combos:
            st["n_discordant"] += 1
            continue
        top, tl, a, b = min(combos)
        n_best = min(sum(1 for c in combos if c[0] == top), NONE)
        rows[a] = (base + b, tl, 1, n_best)
        rows[b] = (base + a, tl, 1, n_best)
        st["n_proper"] += 1
        st["n_ambiguous"] += n_best > 1
        tls.append(tl)
    st["n_pairs"] = len(segs) if n_records is None else n_records // 2
    st["n_unmapped"] = st["n_pairs"] - len(segs)
    st["tlen_sum"], st["tlen_min"], st["tlen_max"] = sum(tls), min(tls, default=0), max(tls, default=0)
    return rows, st


def invariants(chains, rows, max_insert=1000, base=0):
    """selected chains come in twos that name each other, lie in one pair and are concordant, and no concordant combination
    of the pair beats them in 13.2's order; every other row is the empty one"""
    assert len(rows) == len(chains)
    for seg in segments(chains):
        first, middle, end = seg
        sel = [i for i in range(first, end) if rows[i][2] == 1]
        for i in range(first, end):
            if rows[i][2] != 1:
                assert rows[i] == EMPTY, (i, rows[i])
        if not sel:
            if (middle - first) * (end - middle) <= 1 << 17:
                assert not combinations(chains, seg, max_insert), seg
            continue
        assert len(sel) == 2 and first <= sel[0] < middle <= sel[1] < end, (seg, sel)
        a, b = sel
        assert rows[a][0] == base + b and rows[b][0] == base + a and rows[a][1:] == rows[b][1:]
        assert chains[a][Q] ^ 1 == chains[b][Q]
        tl = concordant(chains[a], chains[b], max_insert)
        assert tl is not None and tl == rows[a][1] and rows[a][3] >= 1
        if (middle - first) * (end - middle) <= 1 << 17:
            combos = combinations(chains, seg, max_insert)
            mine = (-(chains[a][SCORE] + chains[b][SCORE]), tl, a, b)
            assert min(combos) == mine, (seg, min(combos), mine)
            assert rows[a][3] == sum(1 for c in combos if c[0] == mine[0])


def mated_paf(paf, rows):
    """13.5 on the lines of a PAF without the rule's tags: pr (and mi, tl, nb) behind s1:i, or behind s2:i where it follows"""
    lines = paf.split(b"\n")
    assert lines.pop() == b"" and len(lines) == len(rows)
    out = []
    for line, (mate, tl, cls, n_best) in zip(lines, rows):
        f = line.split(b"\t")
        at = next(i for i, x in enumerate(f) if x.startswith(b"s1:i:")) + 1
        if at < len(f) and f[at].startswith(b"s2:i:"):
            at += 1
        f[at:at] = [b"pr:A:P", b"mi:i:%d" % mate, b"tl:i:%d" % tl, b"nb:i:%d" % n_best] if cls else [b"pr:A:U"]
        out.append(b"\t".join(f) + b"\n")
    return b"".join(out)


def cut(batch_bytes, anchors, bases, budget):
    """rule 9's greedy cut with the pair as its unit (13.7).  anchors, bases: per query record (an even number of them);
    batch_bytes(a, b): the bound of a batch.  -> [(first_query, n_queries, n_anchors, n_query_bases, bytes_bound)]; MemoryError
    names the pair that exceeds the budget on its own"""
    assert len(anchors) == len(bases) and len(anchors) % 2 == 0
    out, first, n = [], 0, len(anchors)
    while first < n:
        a = b = 0
        end = first
        while end < n:
            a2, b2 = a + anchors[end] + anchors[end + 1], b + bases[end] + bases[end + 1]
            if not (a2 < 1 << 31 and batch_bytes(a2, b2) <= budget):
                break
            a, b, end = a2, b2, end + 2
        if end == first:
            raise MemoryError("pair %d" % (first // 2))
        out.append((first, end - first, a, b, batch_bytes(a, b)))
        first = end
    return out
