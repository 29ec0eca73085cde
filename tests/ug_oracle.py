"""The short-read unitig assembly restated in plain Python, from the rules in include/msgpu.h ("short-read unitig
assembly") -- not from the kernels.  A k-mer is a Python integer (A=0, C=1, G=2, T=3, first base most significant), the
solid set a dict canonical k-mer -> count, the graph is never stored: succ() and pred() ask the dict.  Only the exact
counting of the windows is borrowed, from kf_oracle (rules 1 and 2 of the k-mer filter hold here word for word).

    rule 1  input        parse_files, count_files
    rule 2  solid set    run: count >= min_count
    rule 3  graph        succ, pred
    rule 4  tips         tip_round, tip_rounds
    rule 5  unitigs      joined_next, unitigs
    rule 6  output       texts
"""
import kf_oracle
from kf_oracle import FastqError, kmer_text  # noqa: F401  (re-exported for the tests)

_RC_BYTE = bytes((((b & 3) << 6) | (((b >> 2) & 3) << 4) | (((b >> 4) & 3) << 2) | ((b >> 6) & 3)) ^ 0xff for b in range(256))


def rc(x, k):
    """reverse complement of a k-mer: four bases per byte are mirrored and complemented by the table, the byte order by
    reading the 16 bytes the other way round"""
    return int.from_bytes(x.to_bytes(16, "little").translate(_RC_BYTE), "big") >> (128 - 2 * k)


def canon(x, k):
    return min(x, rc(x, k))


def parse_files(datas):
    """rule 1: every file by the k-mer filter's FASTQ rules, file 0 first; the files are not pairs"""
    return [kf_oracle.parse_fastq(d, f) for f, d in enumerate(datas)]


def count_files(records, k):
    """-> (dict canonical k-mer -> count over all files, windows)"""
    return kf_oracle.count(records[0], records[1] if len(records) > 1 else [], k)


class Graph:
    """rule 3 over a solid set ``S`` (anything with ``in``)"""

    def __init__(self, S, k):
        self.S, self.k = S, k
        self.mask, self.top = (1 << (2 * k)) - 1, 2 * (k - 1)

    def succ(self, s):
        base = (s << 2) & self.mask
        return [base | c for c in range(4) if canon(base | c, self.k) in self.S]

    def pred(self, s):
        base = s >> 2
        return [base | (c << self.top) for c in range(4) if canon(base | (c << self.top), self.k) in self.S]

    def nodes(self):
        """every oriented node once: a self-complementary k-mer is one node"""
        for x in self.S:
            yield x
            y = rc(x, self.k)
            if y != x:
                yield y


def tip_round(S, k, limit):
    """rule 4, one round on the snapshot ``S`` -> the set of canonical k-mers that leave"""
    g = Graph(S, k)
    gone = set()
    for s in g.nodes():
        if g.pred(s):
            continue
        path = [s]
        while True:
            nxt = g.succ(path[-1])
            if len(nxt) != 1:
                break  # not a tip
            if len(g.pred(nxt[0])) >= 2:
                gone.update(canon(x, k) for x in path)  # a tip
                break
            if len(path) == limit:
                break  # not a tip
            path.append(nxt[0])
    return gone


def tip_limits(trim):
    out, l = [], 1
    while l < trim:
        out.append(l)
        l *= 2
    return out + ([trim] if trim > 0 else [])


def tip_rounds(S, k, trim):
    """rule 4 -> (the solid set after trimming, [(limit, k-mers removed)])"""
    S = dict(S)
    rounds = []
    limits = tip_limits(trim)
    i = 0
    while i < len(limits):
        gone = tip_round(S, k, limits[i])
        for x in gone:
            del S[x]
        rounds.append((limits[i], len(gone)))
        if i + 1 < len(limits) or not gone:
            i += 1  # the last limit repeats until a round removes nothing
    return S, rounds


def joined_next(g, s):
    """rule 5: the node s is joined to, or None.  ``blocked`` pairs (a single successor with a single predecessor, kept
    apart by the self-complement rules) come back as (None, True)."""
    k = g.k
    nxt = g.succ(s)
    if len(nxt) != 1:
        return None, False
    t = nxt[0]
    if g.pred(t) != [s]:
        return None, False
    if s == rc(s, k) or t == rc(t, k) or canon(s, k) == canon(t, k):
        return None, True
    return t, False


def unitigs(S, k):
    """rule 5 -> ([(first k-mer, [oriented nodes], cyclic)], blocked pairs), unsorted"""
    g = Graph(S, k)
    nxt, has_prev, blocked = {}, set(), 0
    for s in g.nodes():
        t, b = joined_next(g, s)
        blocked += b
        if t is not None:
            nxt[s] = t
            has_prev.add(t)
    out, seen = [], set()
    for h in g.nodes():  # linear chains, from their heads
        if h in has_prev:
            continue
        chain = [h]
        while chain[-1] in nxt:
            chain.append(nxt[chain[-1]])
        seen.update(chain)
        mirror_first = rc(chain[-1], k)
        if len(chain) == 1 and mirror_first == h:
            out.append((h, chain, False))  # a self-complementary k-mer alone: it exists once
        elif h < mirror_first:
            out.append((h, chain, False))
    for s in g.nodes():  # what is left lies on cycles
        if s in seen:
            continue
        cyc = [s]
        while nxt[cyc[-1]] != s:
            cyc.append(nxt[cyc[-1]])
        mir = [rc(x, k) for x in reversed(cyc)]
        seen.update(cyc)
        seen.update(mir)
        use = cyc if min(cyc) < min(mir) else mir
        at = use.index(min(use))
        out.append((use[at], use[at:] + use[:at], True))
    return out, blocked


def texts(units, S, k, min_length):
    """rule 6 -> (table [(length, coverage, first k-mer, offset of the sequence in the all text, cyclic)], all text, cut
    text), the unitigs in output order"""
    table, all_text, cut_text = [], [], []
    at = 0
    for i, (first, chain, cyclic) in enumerate(sorted(units, key=lambda u: u[0])):
        seq = kmer_text(first, k) + "".join("ACGT"[x & 3] for x in chain[1:])
        cov = sum(S[canon(x, k)] for x in chain)
        head = ">%d %d %d\n" % (i, len(seq), cov)
        rec = (head + seq + "\n").encode()
        table.append((len(seq), cov, first, at + len(head), int(cyclic)))
        at += len(rec)
        all_text.append(rec)
        if len(seq) >= min_length:
            cut_text.append(rec)
    return table, b"".join(all_text), b"".join(cut_text)


def run(k, datas, min_count=2, trim=None, min_length=500):
    """The whole stage on one or two files (bytes) -> dict.  Beside what the stage reports: ``chains`` (per unitig in
    output order, its oriented nodes), ``blocked`` (adjacent pairs kept apart by the self-complement rules), ``alone``
    (self-complementary k-mers that are a unitig of their own) and ``other_bytes`` (sequence bytes outside ACGTacgt)."""
    if not 2 <= k <= 64 or min_count < 1:
        raise ValueError("k / min_count")
    trim = k if trim is None else trim
    records = parse_files(datas)
    counts, windows = count_files(records, k)
    solid = {x: c for x, c in counts.items() if c >= min_count}
    S, rounds = tip_rounds(solid, k, trim)
    units, blocked = unitigs(S, k)
    table, all_text, cut_text = texts(units, S, k, min_length)
    chains = [u[1] for u in sorted(units, key=lambda u: u[0])]
    other = sum(1 for rs in records for r in rs for b in r[1] if b not in b"ACGTacgt")
    return {"k": k, "records": [len(r) for r in records], "windows": windows, "distinct": len(counts), "solid": len(solid),
            "solid_after": len(S), "rounds": rounds, "unitigs": table, "kept": sum(1 for t in table if t[0] >= min_length),
            "cycles": sum(t[4] for t in table), "longest": max([len(c) for c in chains], default=0), "all": all_text,
            "cut": cut_text, "chains": chains, "blocked": blocked, "counts": S,
            "alone": sum(1 for c in chains if len(c) == 1 and c[0] == rc(c[0], k)), "other_bytes": other}
