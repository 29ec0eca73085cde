"""Synthetic unitig-anchor -> long-read PAF generator (SURVEY.md section 8(d) workload shape).

Portable and deterministic: every random draw comes from a counter-based splitmix64 stream, so the same
(seed, shape) gives the same table with any numpy version and in any other language.

Genome of length G = reads * read_len / coverage; reads start ~U[0, G-L], strand ~Bernoulli(1/2), length exactly L,
named r<i>; anchors are independent unitigs, length ~U{500..1500}, start ~U[0, G-len], named u<i>; one PAF row per
(anchor, read) whose genomic intersection is >= 420 bp: query coords = intersection in the anchor frame, target
coords = intersection on the read's own strand, each end jittered by U{-15..15} and clamped to [0, L],
nmatch = floor(span * U(0.86, 0.97)); rows grouped by anchor then read; one trailing sentinel line (the reference
never parses the last line of the file, BlastFileReader.cpp:76).

`paf_table` returns PAF-level columns; `accepted_rows` applies the reference's A1 rules (filter + Registry ids,
BlastFileReader.cpp:101-126) and returns the msgpu_row table that msgpu_parse_paf would produce from the text.
"""
import numpy as np

ROW_DTYPE = np.dtype([("anchor_id", "<u4"), ("read_id", "<u4"), ("read_len", "<i4"), ("i_lo", "<i4"),
                      ("i_hi", "<i4"), ("n_lo", "<i4"), ("n_hi", "<i4"), ("score", "<u4"), ("line", "<u4"),
                      ("flags", "<u4")])

_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def splitmix64(seed, stream, n):
    """n outputs of splitmix64 started at state seed ^ (stream * 0xD1342543DE82EF95), as uint64."""
    with np.errstate(over="ignore"):
        s0 = np.uint64(seed) ^ (np.uint64(stream) * np.uint64(0xD1342543DE82EF95))
        z = s0 + (np.arange(1, n + 1, dtype=np.uint64) * _GAMMA)
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def _randint(seed, stream, n, lo, hi):
    """integers in [lo, hi] (element-wise bounds allowed)"""
    u = splitmix64(seed, stream, n)
    span = (np.asarray(hi, dtype=np.int64) - np.asarray(lo, dtype=np.int64) + 1).astype(np.uint64)
    return np.asarray(lo, dtype=np.int64) + (u % span).astype(np.int64)


def _uniform(seed, stream, n, lo, hi):
    u = (splitmix64(seed, stream, n) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    return lo + (hi - lo) * u


def read_lengths(n_reads, read_len, seed, read_len_min=None):
    """per-read lengths: exactly read_len (the BASELINE shape), or ~U{read_len_min..read_len} (reads of mixed length, so
    that short reads lie inside long ones: contained EdgeOrders, the input of findContractionEdges)"""
    if read_len_min is None or read_len_min >= read_len:
        return np.full(n_reads, read_len, dtype=np.int64)
    return _randint(seed, 9, n_reads, read_len_min, read_len)


def read_layout(n_reads, read_len, seed, coverage=10, read_len_min=None):
    """(genome length, read starts, read strands) -- the same draws paf_table() makes."""
    G = max(int(n_reads) * int(read_len) // int(coverage), read_len + 1500)
    r_start = _randint(seed, 3, n_reads, 0, G - read_lengths(n_reads, read_len, seed, read_len_min))
    r_fwd = (splitmix64(seed, 4, n_reads) & np.uint64(1)).astype(bool)
    return G, r_start, r_fwd


def anchor_layout(n_reads, read_len, n_anchors, seed, coverage=10, tiled=False):
    """(anchor starts, anchor lengths) on the genome -- the same draws paf_table() makes.  tiled: the anchors are
    consecutive, NON-overlapping stretches of length ~U{500..1500} separated by gaps ~U{0..300} that cover the genome end to
    end -- what the unitigs of one genome are (n_anchors is ignored; about G / 1150 of them)."""
    G = max(int(n_reads) * int(read_len) // int(coverage), read_len + 1500)
    if tiled:
        n_max = G // 500 + 2
        a_len = _randint(seed, 1, n_max, 500, 1500)
        gap = _randint(seed, 10, n_max, 0, 300)
        a_start = np.cumsum(a_len + gap) - a_len - gap + _randint(seed, 11, 1, 0, 199)[0]
        keep = a_start + a_len <= G
        return a_start[keep], a_len[keep]
    a_len = _randint(seed, 1, n_anchors, 500, 1500)
    a_start = _randint(seed, 2, n_anchors, 0, G - a_len)
    return a_start, a_len


def genome_bases(G, seed):
    """Uniform ACGT genome of length G as a uint8 array (32 bases per splitmix64 draw)."""
    u = splitmix64(seed, 8, (G + 31) // 32)
    shifts = (np.arange(32, dtype=np.uint64) * np.uint64(2))[None, :]
    codes = ((u[:, None] >> shifts) & np.uint64(3)).astype(np.uint8).reshape(-1)[:G]
    return np.frombuffer(b"ACGT", dtype=np.uint8)[codes]


def paf_table(n_reads, read_len, n_anchors, seed, coverage=10, min_intersection=420, jitter=15, tiled=False,
              read_len_min=None):
    """PAF-level columns of the synthetic alignment set (before the reference's filter).  tiled / read_len_min: see
    anchor_layout / read_lengths (defaults = the BASELINE shape: independent random anchors, reads of exactly read_len)."""
    G, r_start, r_fwd = read_layout(n_reads, read_len, seed, coverage, read_len_min)
    a_start, a_len = anchor_layout(n_reads, read_len, n_anchors, seed, coverage, tiled)
    n_anchors = len(a_start)
    read_len = read_lengths(n_reads, read_len, seed, read_len_min)  # per read from here on

    order = np.argsort(a_start, kind="stable")
    starts = a_start[order]
    lo = np.searchsorted(starts, r_start - 1500, side="left")
    hi = np.searchsorted(starts, r_start + read_len, side="right")
    cnt = hi - lo
    tot = int(cnt.sum())
    rid = np.repeat(np.arange(n_reads, dtype=np.int64), cnt)
    first = np.repeat(np.cumsum(cnt) - cnt, cnt)
    k = np.arange(tot, dtype=np.int64) - first + np.repeat(lo, cnt)
    aid = order[k]
    g_lo = np.maximum(a_start[aid], r_start[rid])
    g_hi = np.minimum(a_start[aid] + a_len[aid], r_start[rid] + read_len[rid])
    keep = (g_hi - g_lo) >= min_intersection
    aid, rid, g_lo, g_hi = aid[keep], rid[keep], g_lo[keep], g_hi[keep]
    # rows grouped by anchor id, then read id
    o = np.lexsort((rid, aid))
    aid, rid, g_lo, g_hi = aid[o], rid[o], g_lo[o], g_hi[o]
    n = len(aid)
    q_lo = g_lo - a_start[aid]
    q_hi = g_hi - a_start[aid]
    fwd = r_fwd[rid]
    t_lo = np.where(fwd, g_lo - r_start[rid], r_start[rid] + read_len[rid] - g_hi)
    t_hi = np.where(fwd, g_hi - r_start[rid], r_start[rid] + read_len[rid] - g_lo)
    t_lo = np.maximum(0, t_lo + _randint(seed, 5, n, -jitter, jitter))
    t_hi = np.minimum(read_len[rid], t_hi + _randint(seed, 6, n, -jitter, jitter))
    nmatch = np.floor((q_hi - q_lo) * _uniform(seed, 7, n, 0.86, 0.97)).astype(np.int64)
    return {"qname_id": aid, "qlen": a_len[aid], "qstart": q_lo, "qend": q_hi, "strand": fwd, "tname_id": rid,
            "tlen": read_len[rid], "tstart": t_lo, "tend": t_hi, "nmatch": nmatch,
            "genome": G}


def accepted_rows(tab, min_matches=400, th_length=500, th_matches=500):
    """The reference's A1 rules applied to paf_table() columns -> msgpu_row table (line order)."""
    span = tab["qend"] - tab["qstart"]
    ok = (tab["nmatch"] >= min_matches) & (span >= min_matches)
    line = np.nonzero(ok)[0]

    def registry(names):  # dense ids in first-seen order (Registry.cpp:36-45)
        uniq, first_idx, inv = np.unique(names, return_index=True, return_inverse=True)
        rank = np.empty(len(uniq), dtype=np.int64)
        rank[np.argsort(first_idx, kind="stable")] = np.arange(len(uniq))
        return rank[inv], uniq[np.argsort(first_idx, kind="stable")]

    read_id, read_names = registry(tab["tname_id"][ok])
    anchor_id, anchor_names = registry(tab["qname_id"][ok])
    rows = np.zeros(len(line), dtype=ROW_DTYPE)
    rows["anchor_id"] = anchor_id
    rows["read_id"] = read_id
    rows["read_len"] = tab["tlen"][ok]
    rows["i_lo"] = tab["qstart"][ok]
    rows["i_hi"] = tab["qend"][ok] - 1
    rows["n_lo"] = tab["tstart"][ok]
    rows["n_hi"] = tab["tend"][ok] - 1
    rows["score"] = tab["nmatch"][ok]
    rows["line"] = line
    prim = (span[ok] >= th_length) & (tab["nmatch"][ok] >= th_matches)
    rows["flags"] = tab["strand"][ok].astype(np.uint32) | (prim.astype(np.uint32) << 1)
    return rows, ["r%d" % i for i in read_names], ["u%d" % i for i in anchor_names]


def paf_lines(tab):
    """PAF text lines (12 columns) + the trailing sentinel line the reference never parses."""
    out = []
    for i in range(len(tab["qname_id"])):
        out.append("u%d\t%d\t%d\t%d\t%s\tr%d\t%d\t%d\t%d\t%d\t%d\t60" % (
            tab["qname_id"][i], tab["qlen"][i], tab["qstart"][i], tab["qend"][i], "+" if tab["strand"][i] else "-",
            tab["tname_id"][i], tab["tlen"][i], tab["tstart"][i], tab["tend"][i], tab["nmatch"][i],
            tab["qend"][i] - tab["qstart"][i]))
    out.append("u0\t1\t0\t1\t+\tr0\t1\t0\t1\t0\t1\t0")
    return out


def synth_rows(n_reads, read_len, n_anchors, seed, coverage=10, **shape):
    """Convenience: accepted msgpu_row table of a synthetic workload."""
    rows, _, _ = accepted_rows(paf_table(n_reads, read_len, n_anchors, seed, coverage, **shape))
    return rows


ORD_DIR = 4  # msgpu_order.flags: EdgeOrder::direction


def directed_step(tables, edge_idx, a, b, dir_a):
    """EdgeOrders + EdgeMatches of the directed edge a -> b as getDirectedGraph fills it (dg.cpp:70-102): an order of
    the undirected edge goes onto (start, end), swapped when exactly one of {!order.direction and base == b, !dir_a}."""
    e = tables["edges"][edge_idx]
    orders = []
    for o in tables["orders"][int(e["order_off"]): int(e["order_off"]) + int(e["order_cnt"])]:
        flip = (not (int(o["flags"]) & ORD_DIR) and int(o["base"]) == b) != (not dir_a)
        start, end = (int(o["end"]), int(o["start"])) if flip else (int(o["start"]), int(o["end"]))
        if (start, end) != (a, b):
            continue
        ids = tables["ids"][int(o["ids_off"]): int(o["ids_off"]) + int(o["ids_cnt"])]
        orders.append({"ids": [int(x) for x in ids], "score": int(o["score"]), "base": int(o["base"])})
    ems = tables["ems"][int(e["em_off"]): int(e["em_off"]) + int(e["em_cnt"])]
    return {"orders": orders, "em": {int(m["anchor_id"]): (int(m["ov_lo"]), int(m["ov_hi"])) for m in ems}}


def chain_paths(tables, read_start, read_fwd, read_len, window_end, max_reads=12, max_paths=1 << 30):
    """Disjoint greedy left-to-right chains of reads starting before `window_end` on the synthetic genome.

    Stands in for the phases between the overlap path and assemblePath (graph clean-up, getDirectedGraph,
    linearizeGraph): consecutive reads share an overlap-graph edge with at least one
    EdgeOrder pointing along the chain; read direction = its strand.  read_start / read_fwd are indexed by read id.
    -> [(path, steps)] in the form muchsalsa_amd.assembly.Assembly.add_path takes."""
    edges = tables["edges"]
    inside = (read_start[edges["v1"]] < window_end) & (read_start[edges["v2"]] < window_end)
    adj = {}
    for i in np.nonzero(inside)[0]:
        a, b = int(edges["v1"][i]), int(edges["v2"][i])
        adj.setdefault(a, []).append((b, int(i)))
        adj.setdefault(b, []).append((a, int(i)))
    reads = [int(r) for r in np.argsort(read_start, kind="stable") if read_start[r] < window_end]
    used, out, frontier = set(), [], -1
    for s in reads:
        if s in used or read_start[s] <= frontier or len(out) >= max_paths:
            continue
        path, steps, cur = [s], [], s
        used.add(s)
        while len(path) < max_reads:
            best = None
            for nb, ei in adj.get(cur, []):
                if nb in used or read_start[nb] <= read_start[cur]:
                    continue
                if best is not None and read_start[nb] <= read_start[best[0]]:
                    continue
                st = directed_step(tables, ei, cur, nb, bool(read_fwd[cur]))
                if st["orders"]:
                    best = (nb, st)
            if best is None:
                break
            path.append(best[0])
            steps.append(best[1])
            used.add(best[0])
            cur = best[0]
        if len(path) >= 2:
            out.append(([{"id": r, "dir": bool(read_fwd[r]), "len": int(read_len)} for r in path], steps))
            frontier = int(read_start[path[-1]])
    return out


# the configurations BASELINE.json names
CONFIGS = {
    "cfg2": dict(n_reads=10_000, read_len=5_000, n_anchors=50_000, seed=42),
    "cfg3": dict(n_reads=100_000, read_len=10_000, n_anchors=500_000, seed=43),
}
# the same sizes on the shape the graph stage and assemblePath exist for: unitigs that TILE the genome (no two anchors
# overlap) and reads of mixed length (short ones contained in long ones).  Not BASELINE configurations.
TILED = {
    "cfg2": dict(n_reads=10_000, read_len=5_000, n_anchors=0, seed=42, tiled=True, read_len_min=1_250),
    "cfg3": dict(n_reads=100_000, read_len=10_000, n_anchors=0, seed=43, tiled=True, read_len_min=2_500),
}


def unitig_filter_workload(n_reads, read_len, n_anchors, seed, coverage=10, n_repeats=12, repeat_hits=(200, 3000),
                           n_long=2, long_len=120000, long_hits=12000, n_dup=2000, n_again=300):
    """Input of the unitig coverage filter (muchsalsa_amd.unitig_filter): (PAF text, unitig FASTA text), both bytes.

    Built on paf_table / genome_bases: the anchors are the unitigs (u<i>, their bases cut from the genome) and every
    paf_table row is a PAF line (qlen = the unitig's length).  On top of that shape:
      * n_repeats repeat unitigs (x<j>, 2-6 kb) that map at many genome positions: ~U{repeat_hits} lines each, all
        inside the first half of the unitig -- outliers whose second half is a fragment; the largest blocks are giant;
      * n_long long unitigs (l<j>, long_len bases) with long_hits lines each, piled up in a few windows: outliers with
        many fragments;
      * n_dup lines that repeat a read of their block with other coordinates (pass 1 counts a read once per block);
      * n_again blocks of earlier unitigs that come back at the end of the file (the id's last block decides its value).
    Deterministic in (seed, shape)."""
    tab = paf_table(n_reads, read_len, n_anchors, seed, coverage)
    a_start, a_len = anchor_layout(n_reads, read_len, n_anchors, seed, coverage)
    genome = genome_bases(tab["genome"], seed)
    G = int(tab["genome"])
    names, qlen, qs, qe, reads = [], [], [], [], []  # one entry per block: arrays of its lines

    aid, rid = tab["qname_id"], tab["tname_id"]
    cut = np.flatnonzero(np.diff(aid)) + 1
    starts = np.concatenate(([0], cut))
    ends = np.concatenate((cut, [len(aid)]))
    dup_blocks = set(_randint(seed, 40, n_dup, 0, max(len(starts) - 1, 0)).tolist()) if len(starts) else set()
    for bi, (b0, b1) in enumerate(zip(starts.tolist(), ends.tolist())):
        u = int(aid[b0])
        s, e, r = tab["qstart"][b0:b1], tab["qend"][b0:b1], rid[b0:b1]
        if bi in dup_blocks:
            k = int(_randint(seed + b0, 41, 1, 0, b1 - b0 - 1)[0])
            ns = int(_randint(seed + b0, 42, 1, 0, max(int(a_len[u]) - 1, 0))[0])
            ne = int(_randint(seed + b0, 43, 1, ns, int(a_len[u]))[0])
            s, e, r = np.append(s, ns), np.append(e, ne), np.append(r, r[k])
        names.append("u%d" % u)
        qlen.append(int(a_len[u]))
        qs.append(s)
        qe.append(e)
        reads.append(r)
    n_normal = len(names)
    seqs = {"u%d" % i: genome[a_start[i]:a_start[i] + a_len[i]].tobytes() for i in range(len(a_start))}

    def piled(name, L, n, stream, lo, hi, lens):
        s = _randint(seed, stream, n, lo, hi)
        e = np.minimum(s + _randint(seed, stream + 1, n, lens[0], lens[1]), L)
        r = _randint(seed, stream + 2, n, 0, n_reads - 1)
        r[1::17] = r[0::17][: len(r[1::17])]  # reads that hit the same unitig twice
        names.append(name)
        qlen.append(L)
        qs.append(s)
        qe.append(e)
        reads.append(r)

    r_len = _randint(seed, 44, n_repeats, 2000, 6000)
    r_hits = _randint(seed, 45, n_repeats, repeat_hits[0], repeat_hits[1])
    r_pos = _randint(seed, 46, n_repeats, 0, G - 6000)
    for j in range(n_repeats):
        L = int(r_len[j])
        seqs["x%d" % j] = genome[r_pos[j]:r_pos[j] + L].tobytes()
        piled("x%d" % j, L, int(r_hits[j]), 100 + 3 * j, 0, L // 2 - 400, (100, 400))
    l_pos = _randint(seed, 47, n_long, 0, max(G - long_len, 0))
    for j in range(n_long):
        L = long_len
        seqs["l%d" % j] = (genome[l_pos[j]:l_pos[j] + L].tobytes() * (L // max(G, 1) + 1))[:L]
        # windows of 4 kb every 10 kb: the 6 kb between two windows are fragments
        w = _randint(seed, 200 + 3 * j, long_hits, 0, L // 10000 - 1) * 10000
        s = w + _randint(seed, 201 + 3 * j, long_hits, 0, 3000)
        e = np.minimum(s + _randint(seed, 202 + 3 * j, long_hits, 100, 1000), L)
        names.append("l%d" % j)
        qlen.append(L)
        qs.append(s)
        qe.append(e)
        reads.append(_randint(seed, 48 + j, long_hits, 0, n_reads - 1))
    for k in _randint(seed, 49, min(n_again, n_normal), 0, max(n_normal - 1, 0)).tolist():
        m = max(1, len(qs[k]) // 2)
        names.append(names[k])
        qlen.append(qlen[k])
        qs.append(qs[k][:m])
        qe.append(qe[k][:m])
        reads.append(reads[k][:m])

    out = []
    for name, L, s, e, r in zip(names, qlen, qs, qe, reads):
        n = len(s)
        nm = np.maximum(np.asarray(e) - np.asarray(s), 0)
        cols = [np.full(n, name, dtype=object), np.full(n, L), s, e, np.full(n, "+", dtype=object),
                np.char.add("r", np.asarray(r).astype(str)), np.full(n, read_len), np.zeros(n, np.int64), nm, nm, nm,
                np.full(n, 60)]
        out.append("\n".join("\t".join(map(str, row)) for row in zip(*cols)))
    paf = ("\n".join(out) + "\n").encode()
    fasta = b"".join(b">%s synthetic len=%d\n%s\n" % (k.encode(), len(v), v) for k, v in seqs.items())
    return paf, fasta


def scrubber_workload(n_reads, read_len, n_anchors, seed, coverage=10, read_len_min=None, hole_every=7, dup_frac=0.05,
                      n_again=200, n_strangers=50, fastq=False):
    """Input of the read scrubber (muchsalsa_amd.scrubber): (anchor PAF, read-to-read PAF, reads file), all bytes.

    Built on paf_table / genome_bases: every paf_table row is an anchor line (its hits of 420..499 positions are the ones
    the scrubber skips), the reads are r<i> = their stretch of the genome (FASTA, or FASTQ with fastq=True).  On top:
      * a fraction dup_frac of the anchor lines is followed by a second hit of the same (read, anchor) with other read
        coordinates, and every second line of n_again anchors comes back at the end of the file (a later chunk of an
        anchor seen before);
      * the read-to-read PAF has one pair per two reads that overlap by >= 800 positions, in either column order; a pair of
        > 1300 positions is split, half of the time, into two lines (of > 3000 positions sometimes into three) whose gaps
        are drawn from {50, 300, 499, 500, 700, 1500} (the second read's coordinates are shifted by a few positions, so the
        two sides see different gaps), and a later line of a pair flips the strand one time in five; the lines are
        shuffled;
      * every hole_every-th read has an uncovered middle: its anchor hits and read-to-read lines that touch the middle fifth
        are left out, so it is written as several records;
      * n_strangers read-to-read lines name a read that no anchor line names, one line maps a read to itself, and reads
        without an anchor hit of >= 500 positions are no nodes although lines name them.
    Deterministic in (seed, shape)."""
    tab = paf_table(n_reads, read_len, n_anchors, seed, coverage, read_len_min=read_len_min)
    G, r_start, r_fwd = read_layout(n_reads, read_len, seed, coverage, read_len_min)
    L = read_lengths(n_reads, read_len, seed, read_len_min)
    genome = genome_bases(G, seed)
    hole = (np.arange(n_reads) % max(int(hole_every), 1)) == (max(int(hole_every), 1) - 1) if hole_every else \
        np.zeros(n_reads, bool)
    h_lo, h_hi = (L * 2) // 5, (L * 3) // 5

    # ---- anchor PAF
    aid, rid = tab["qname_id"], tab["tname_id"]
    keep = (~(hole[rid] & (tab["tstart"] < h_hi[rid]) & (tab["tend"] > h_lo[rid]))).tolist()
    n = len(aid)
    dup = (splitmix64(seed, 60, n) % np.uint64(1000)) < np.uint64(int(dup_frac * 1000))
    rows = []
    strand = np.where(tab["strand"], "+", "-")
    cols = [tab[k].tolist() for k in ("qlen", "qstart", "qend", "tlen", "tstart", "tend", "nmatch")]
    for i, a_, r_, st_, d_, (ql, qs, qe, tl, ts, te, nm) in zip(range(n), aid.tolist(), rid.tolist(), strand.tolist(),
                                                               dup.tolist(), zip(*cols)):
        if not keep[i]:
            continue
        rows.append((a_, "u%d\t%d\t%d\t%d\t%s\tr%d\t%d\t%d\t%d\t%d\t%d\t60" % (a_, ql, qs, qe, st_, r_, tl, ts, te, nm,
                                                                                  qe - qs)))
        if d_:
            rows.append((a_, "u%d\t%d\t0\t%d\t-\tr%d\t%d\t5\t700\t600\t600\t60" % (a_, ql, ql, r_, tl)))
    again = set(_randint(seed, 61, n_again, 0, max(int(aid.max()) if n else 0, 0)).tolist()) if n else set()
    head, tail, seen_of = [], [], {}
    for a, text in rows:
        k = seen_of.get(a, 0)
        seen_of[a] = k + 1
        (tail if (a in again and k % 2 == 1) else head).append((a, text))
    tail.sort(key=lambda x: x[0])
    anchor_paf = ("\n".join(t for _, t in head + tail) + "\n").encode()

    # ---- read-to-read PAF: reads sorted by start, read x against the later reads that begin >= 800 before its end
    order = np.argsort(r_start, kind="stable")
    s_sorted = r_start[order]
    e_sorted = s_sorted + L[order]
    hi = np.searchsorted(s_sorted, e_sorted - 800, side="left")
    cnt = np.maximum(hi - np.arange(n_reads) - 1, 0)
    x = np.repeat(np.arange(n_reads), cnt)
    y = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + x + 1
    i, j = order[x], order[y]
    lo, hi = r_start[j], np.minimum(r_start[i] + L[i], r_start[j] + L[j])
    ok = (hi - lo) >= 800
    i, j, lo, hi = i[ok], j[ok], lo[ok], hi[ok]
    m = len(i)
    u = splitmix64(seed, 62, m)
    swap = (u & np.uint64(1)).astype(bool)
    a, b = np.where(swap, j, i), np.where(swap, i, j)
    pieces = np.ones(m, np.int64)
    ov = hi - lo
    pieces[(ov > 1300) & (((u >> np.uint64(1)) % np.uint64(100)) < np.uint64(50))] = 2
    pieces[(ov > 3000) & (((u >> np.uint64(1)) % np.uint64(100)) < np.uint64(15))] = 3
    gaps = np.array([50, 300, 499, 500, 700, 1500])
    g1 = gaps[(splitmix64(seed, 63, m) % np.uint64(6)).astype(np.int64)]
    g2 = gaps[(splitmix64(seed, 64, m) % np.uint64(6)).astype(np.int64)]
    shift = _randint(seed, 65, m, -3, 3)
    flip = splitmix64(seed, 66, m)
    base_strand = r_fwd[a] == r_fwd[b]
    out = []
    lo_l, hi_l, pc_l, u_l, g1_l, g2_l = lo.tolist(), hi.tolist(), pieces.tolist(), u.tolist(), g1.tolist(), g2.tolist()
    a_l, b_l, sh_l, fl_l, bs_l = a.tolist(), b.tolist(), shift.tolist(), flip.tolist(), base_strand.tolist()
    rs_l, L_l, hole_l, hlo_l, hhi_l = r_start.tolist(), L.tolist(), hole.tolist(), h_lo.tolist(), h_hi.tolist()
    for k in range(m):
        p, q = lo_l[k], hi_l[k]
        if pc_l[k] == 1:
            cuts = [(p, q)]
        elif pc_l[k] == 2:
            mid = p + 550 + (u_l[k] >> 8) % (q - p - 1100)
            cuts = [(p, mid), (min(mid + g1_l[k], q - 520), q)]
        else:  # every cut stays inside the overlap: 600 + w + 1500 + 600 + w <= q - p - 100
            w = (q - p - 2800) // 2
            m1 = p + 600 + (u_l[k] >> 8) % w
            z1 = m1 + g1_l[k]
            m2 = z1 + 600 + (u_l[k] >> 24) % w
            cuts = [(p, m1), (z1, m2), (min(m2 + g2_l[k], q - 520), q)]
        ra, rb = a_l[k], b_l[k]
        sa, sb, La, Lb = rs_l[ra], rs_l[rb], L_l[ra], L_l[rb]
        for c, (l0, h0) in enumerate(cuts):
            if h0 - l0 < 1:
                continue
            plus = bs_l[k] ^ (c > 0 and (fl_l[k] >> (8 * c)) % 5 == 0)
            a0, a1 = l0 - sa, h0 - sa
            b0, b1 = max(l0 - sb + sh_l[k] * c, 0), min(h0 - sb + sh_l[k] * c, Lb)
            if (hole_l[ra] and a0 < hhi_l[ra] and a1 > hlo_l[ra]) or (hole_l[rb] and b0 < hhi_l[rb] and b1 > hlo_l[rb]):
                continue
            out.append("r%d\t%d\t%d\t%d\t%s\tr%d\t%d\t%d\t%d\t%d\t%d\t60" % (ra, La, a0, a1, "+" if plus else "-", rb, Lb, b0,
                                                                              b1, h0 - l0, h0 - l0))
    for k, r in enumerate(_randint(seed, 67, n_strangers, 0, n_reads - 1).tolist()):
        out.append("r%d\t%d\t0\t900\t+\tstranger%d\t4000\t10\t910\t900\t900\t60" % (r, int(L[r]), k) if k % 2 else
                   "stranger%d\t4000\t10\t910\t-\tr%d\t%d\t0\t900\t900\t900\t60" % (k, r, int(L[r])))
    out.append("r0\t%d\t0\t900\t+\tr0\t%d\t0\t900\t900\t900\t60" % (int(L[0]), int(L[0])))
    perm = np.argsort(splitmix64(seed, 68, len(out)), kind="stable")
    ava_paf = ("\n".join(out[k] for k in perm.tolist()) + "\n").encode()

    # ---- the reads
    recs = []
    for r in range(n_reads):
        seq = genome[r_start[r]:r_start[r] + L[r]].tobytes()
        recs.append(b"@r%d\n%s\n+\n%s\n" % (r, seq, b"I" * len(seq)) if fastq else b">r%d\n%s\n" % (r, seq))
    return anchor_paf, ava_paf, b"".join(recs)


def kmer_filter_workload(genome, coverage, read_len, seed, families=6, copies=25, repeat_len=1500, error=0.005,
                         n_frac=0.0005, lower_frac=0.001, insert=None):
    """Input of the k-mer abundance filter (muchsalsa_amd.kmer_filter): (FASTQ file 1, FASTQ file 2), bytes.

    A uniform genome of ``genome`` bases (genome_bases) in which ``families`` repeat units of ``repeat_len`` bases are each
    written ``copies`` times (identical copies, one per slot of an even grid, at a drawn offset inside the slot): their k-mers
    are what the filter finds abundant.  genome * coverage / (2 * read_len) fragments of ``insert`` (default 2.5 read
    lengths) bases at uniform starts; mate 1 is the fragment's first read_len bases, mate 2 the reverse complement of its
    last; every second fragment comes from the other strand (the mates swap roles).  On the reads: a fraction ``error`` of
    the bases is replaced by another base, ``n_frac`` become 'N', ``lower_frac`` lower case.  Record i of both files is
    named p<i, zero padded>/1 and /2; the quality line is all 'I', and starts with '@' in every 97th record.
    Deterministic in (seed, shape)."""
    G, L = int(genome), int(read_len)
    insert = int(insert) if insert else (5 * L) // 2
    g = _planted_genome(G, seed, families, copies, repeat_len, 70, at_least=insert)
    return _illumina_pairs(g, coverage, L, seed, error, n_frac, lower_frac, insert)


def _planted_genome(G, seed, families, copies, repeat_len, stream, at_least=0):
    """genome_bases(G, seed) with ``families`` repeat units of ``repeat_len`` bases each written ``copies`` times: identical
    copies, one per slot of an even grid (which slot: drawn from ``stream``), at an offset inside the slot drawn from
    ``stream`` + 1"""
    g = genome_bases(G, seed).copy()
    slots = int(families) * int(copies)
    if slots:
        slot = G // slots
        if slot < repeat_len or G < at_least:
            raise ValueError("genome too short for the repeats")
        units = genome_bases(int(families) * int(repeat_len), seed + 1).reshape(int(families), int(repeat_len))
        where = np.argsort(splitmix64(seed, stream, slots), kind="stable")  # which slot a (family, copy) lands in
        jitter = _randint(seed, stream + 1, slots, 0, slot - int(repeat_len))
        for i in range(slots):
            at = int(where[i]) * slot + int(jitter[i])
            g[at:at + int(repeat_len)] = units[i // int(copies)]
    return g


def _illumina_pairs(g, coverage, L, seed, error, n_frac, lower_frac, insert):
    """the read pairs of kmer_filter_workload from the genome ``g`` -> (FASTQ file 1, FASTQ file 2)"""
    G = len(g)
    n = max(G * int(coverage) // (2 * L), 1)
    start = _randint(seed, 72, n, 0, G - insert)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    col = np.arange(L, dtype=np.int64)[None, :]
    left = g[start[:, None] + col]
    right = comp[g[(start + insert - 1)[:, None] - col]]
    other = (np.arange(n) & 1).astype(bool)[:, None]
    mates = [np.where(other, right, left), np.where(other, left, right)]
    nb = n * L
    alt = {65: b"CGT", 67: b"GTA", 71: b"TAC", 84: b"ACG"}
    sub = np.zeros((256, 3), np.uint8)
    for b, t in alt.items():
        sub[b] = list(t)
    out = []
    for m, reads in enumerate(mates):
        flat = np.ascontiguousarray(reads).reshape(-1)
        pos = _randint(seed, 73 + 10 * m, int(nb * error), 0, nb - 1)
        flat[pos] = sub[flat[pos], (splitmix64(seed, 74 + 10 * m, len(pos)) % np.uint64(3)).astype(np.int64)]
        flat[_randint(seed, 75 + 10 * m, int(nb * n_frac), 0, nb - 1)] = ord("N")
        pos = _randint(seed, 76 + 10 * m, int(nb * lower_frac), 0, nb - 1)
        flat[pos] |= 0x20
        width = len(str(n - 1))
        head = 2 + width + 3  # "@p", digits, "/1\n"
        rec = np.empty((n, head + L + 3 + L + 1), np.uint8)
        rec[:, 0], rec[:, 1] = ord("@"), ord("p")
        idx = np.arange(n, dtype=np.int64)
        for d in range(width):
            rec[:, 2 + d] = 48 + (idx // 10 ** (width - 1 - d)) % 10
        rec[:, 2 + width:head] = np.frombuffer(b"/%d\n" % (m + 1), np.uint8)
        rec[:, head:head + L] = flat.reshape(n, L)
        rec[:, head + L:head + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, head + L + 3:head + 2 * L + 3] = ord("I")
        rec[::97, head + L + 3] = ord("@")
        rec[:, -1] = 10
        out.append(rec.tobytes())
    return out[0], out[1]


def _revcomp(seq):
    return seq[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def unitig_cases():
    """Hand-made inputs of the short-read unitig assembly (muchsalsa_amd.unitigs): name -> (FASTQ file 1, FASTQ file 2 or
    None, what the case is made of).  Every read is written twice, so its k-mers are solid at min_count = 2.

    rings    two circular sequences of 300 bases, 100-base reads tiled around each at a step of 10: two cyclic unitigs
             (300 k-mers, 300 + k - 1 bases each).  The smallest oriented k-mer of the first ring lies on the strand the
             reads were written from, that of the second on the other one.
    selfcomp a linear sequence of 240 bases with x + rc(x) (16 bases each) in its middle: a self-complementary 32-mer.
    hairpin  one read x + rc(x) of 2 x 100 bases: the read is its own reverse complement."""
    def fq(name, reads):
        return b"".join(b"@%s%d\n%s\n+\n%s\n" % (name, i, r, b"I" * len(r)) for i, r in enumerate(reads))

    rings = [genome_bases(300, 101).tobytes(), genome_bases(300, 102).tobytes()]
    ring_reads = [[(r + r)[at:at + 100] for at in range(0, 300, 10) for _ in (0, 1)] for r in rings]
    left, x, right = genome_bases(112, 201).tobytes(), genome_bases(16, 202).tobytes(), genome_bases(112, 203).tobytes()
    selfcomp = left + x + _revcomp(x) + right
    h = genome_bases(100, 301).tobytes()
    hairpin = h + _revcomp(h)
    return {"rings": (fq(b"a", ring_reads[0]), fq(b"b", ring_reads[1]), {"rings": rings}),
            "selfcomp": (fq(b"s", [selfcomp, selfcomp]), None, {"sequence": selfcomp, "self_complementary": x + _revcomp(x)}),
            "hairpin": (fq(b"h", [hairpin, hairpin]), None, {"sequence": hairpin})}


def _other_base(b, step):
    """the base ``step`` (1..3) places behind ``b`` in ACGT"""
    return b"ACGT"[(b"ACGT".index(b) + step) % 4]


def diploid_workload(genome=6000, every=400, coverage=15, read_len=100, seed=7, error=0.0):
    """Input of the unitig assembly with bubble popping (rule 9): (one FASTQ file, None, what it is made of).

    Haplotype 1 is genome_bases(genome, seed).  Haplotype 2 is haplotype 1 with a variant every ``every`` bases (the first at
    every / 2): by a draw a substitution, or an insertion or a deletion of 1-3 bases, about half each.  From each haplotype
    ``coverage`` * its length / read_len reads of read_len bases at uniform starts, every read reverse-complemented with
    probability 1/2; a fraction ``error`` of the bases of the reads is replaced by another base.  Deterministic in
    (seed, shape)."""
    G, L = int(genome), int(read_len)
    a = genome_bases(G, seed)
    sites = np.arange(every // 2, G - every // 2 + 1, every, dtype=np.int64)
    kind = splitmix64(seed, 90, len(sites)) % np.uint64(4)        # 0, 1: substitution, 2: insertion, 3: deletion
    size = (splitmix64(seed, 91, len(sites)) % np.uint64(3)).astype(np.int64) + 1
    ins = genome_bases(3 * len(sites), seed + 2)
    parts, at, variants = [], 0, []
    for i, p in enumerate(int(x) for x in sites):
        parts.append(a[at:p])
        if kind[i] < 2:
            parts.append(np.array([_other_base(int(a[p]), int(size[i]))], np.uint8))
            at = p + 1
            variants.append((p, "snp", 1))
        elif kind[i] == 2:
            parts.append(ins[3 * i:3 * i + int(size[i])])
            at = p
            variants.append((p, "ins", int(size[i])))
        else:
            at = p + int(size[i])
            variants.append((p, "del", int(size[i])))
    parts.append(a[at:])
    b = np.concatenate(parts)
    comp = np.zeros(256, np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    col = np.arange(L, dtype=np.int64)[None, :]
    reads = []
    for h, hap in enumerate((a, b)):
        n = max(len(hap) * int(coverage) // L, 1)
        start = _randint(seed, 92 + h, n, 0, len(hap) - L)
        r = hap[start[:, None] + col]
        flip = (splitmix64(seed, 94 + h, n) & np.uint64(1)).astype(bool)[:, None]
        reads.append(np.where(flip, comp[r[:, ::-1]], r))
    flat = np.ascontiguousarray(np.concatenate(reads)).reshape(-1)
    n, nb = len(flat) // L, len(flat)
    sub = np.zeros((256, 3), np.uint8)
    for base, t in {65: b"CGT", 67: b"GTA", 71: b"TAC", 84: b"ACG"}.items():
        sub[base] = list(t)
    pos = _randint(seed, 96, int(nb * error), 0, nb - 1)
    flat[pos] = sub[flat[pos], (splitmix64(seed, 97, len(pos)) % np.uint64(3)).astype(np.int64)]
    width = len(str(n - 1))
    head = 2 + width + 1  # "@d", digits, "\n"
    rec = np.empty((n, head + L + 3 + L + 1), np.uint8)
    rec[:, 0], rec[:, 1] = ord("@"), ord("d")
    idx = np.arange(n, dtype=np.int64)
    for d in range(width):
        rec[:, 2 + d] = 48 + (idx // 10 ** (width - 1 - d)) % 10
    rec[:, head - 1] = 10
    rec[:, head:head + L] = flat.reshape(n, L)
    rec[:, head + L:head + L + 3] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, head + L + 3:head + 2 * L + 3] = ord("I")
    rec[:, -1] = 10
    return rec.tobytes(), None, {"haplotypes": (a.tobytes(), b.tobytes()), "variants": variants}


def _tile(seq, L, step=10):
    """the reads of L bases at every ``step``-th position of seq, and the one that ends with it"""
    starts = list(range(0, len(seq) - L + 1, step))
    if starts[-1] != len(seq) - L:
        starts.append(len(seq) - L)
    return [seq[s:s + L] for s in starts]


def _snp(seq, at, step=1):
    return seq[:at] + bytes([_other_base(seq[at], step)]) + seq[at + 1:]


def _bubble_case(haps, extra, L, **meta):
    """-> (FASTQ file, None, meta and ``haplotypes``): every haplotype (sequence, multiplicity) tiled into reads of L bases,
    each read written ``multiplicity`` times, then the reads of ``extra``"""
    reads = [r for seq, m in haps for r in _tile(seq, L) for _ in range(m)] + list(extra)
    fq = b"".join(b"@b%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    return fq, None, dict({"haplotypes": haps}, **meta)


def unitig_bubble_cases(k=21):
    """Hand-made inputs of rule 9 (bubble popping) of the unitig assembly: name -> (FASTQ file, None, what the case is made
    of: ``haplotypes`` [(sequence, multiplicity)], ``bubble`` and ``trim`` to run it with).  A is a random sequence of 400
    bases; every haplotype is tiled into 80-base reads at a step of 10, each read written ``multiplicity`` times.  p = 200.

    edge        A x 3, A with one substitution at p x 2: one bubble of two branches of k k-mers
    indel_long  A x 3, A without its bases p, p + 1 x 2: the longer branch is the majority
    indel_short A x 2, the deletion x 2 and the deletion's read over the site once more: the shorter branch has the greater
                mean and the smaller sum.  Above k = 21 its haplotypes are tiled into reads of k + 100 bases: the one extra
                read adds 1 to each of the shorter branch's k - 1 k-mers, so its sum stays below that of the longer branch's
                k + 1 only where a k-mer is counted more than (k - 1) / 2 times, and 80-base reads count a 33-mer 10 times
    tie         A x 2, the substitution x 2: equal counts, the smaller base wins
    three_way   three bases at p, x 3, x 2, x 1: one bubble of three branches
    nested      A x 3, B = A with substitutions at p and p + 12 x 2, B with a further one at p + 6 x 1: a bubble inside a
                branch of a bubble
    overlapped  A x 3, B = A with a substitution at p x 2, B with a further one at p + 5 x 1: the branches merge at
                different nodes
    palindrome  P + A + rc(P) x 3 beside P + C + rc(P) x 2 for 150 bases P: fork and merge are one k-mer
    alternate   A x 3, A with a substitution at k + 9 x 2, and 100 random bases followed by A[k + 16 : k + 76] x 2: a junction
                just behind the bubble, so the start of A is a tip once the bubble is gone; trim = bubble = 3 k"""
    snp = _snp

    def case(haps, extra=(), L=80, **kw):
        return _bubble_case(haps, extra, L, **dict({"bubble": 3 * k, "trim": k}, **kw))

    A, p = genome_bases(400, 401).tobytes(), 200
    dele = A[:p] + A[p + 2:]
    B = snp(snp(A, p), p + 12)
    P = genome_bases(150, 402).tobytes()
    R = genome_bases(100, 403).tobytes()
    return {"edge": case([(A, 3), (snp(A, p), 2)]),
            "indel_long": case([(A, 3), (dele, 2)]),
            "indel_short": case([(A, 2), (dele, 2)], extra=[dele[p - 40:p + 40]], L=80 if k <= 21 else k + 100),
            "tie": case([(A, 2), (snp(A, p), 2)]),
            "three_way": case([(A, 3), (snp(A, p, 1), 2), (snp(A, p, 2), 1)]),
            "nested": case([(A, 3), (B, 2), (snp(B, p + 6), 1)]),
            "overlapped": case([(A, 3), (snp(A, p), 2), (snp(snp(A, p), p + 5), 1)]),
            "palindrome": case([(P + b"A" + _revcomp(P), 3), (P + b"C" + _revcomp(P), 2)]),
            "alternate": case([(A, 3), (snp(A, k + 9), 2), (R + A[k + 16:k + 76], 2)], bubble=3 * k, trim=3 * k)}


def _pick(n, seed, ok):
    """the first of genome_bases(n, seed), genome_bases(n, seed + 1000), ... that ``ok`` accepts"""
    while True:
        s = genome_bases(n, seed).tobytes()
        if ok(s):
            return s
        seed += 1000


def _plain_kmers(seq, k):
    """every k-mer of seq occurs once on its two strands together (a self-complementary one counts as one)"""
    mers = [seq[i:i + k] for i in range(len(seq) - k + 1)]
    both = set(mers) | {_revcomp(m) for m in mers}
    return len(both) == 2 * len(mers) - sum(1 for m in mers if m == _revcomp(m))


def unitig_bubble_edge_cases(k, read_len=None):
    """Edge inputs of rule 9 aimed at the bubble kernels: name -> (FASTQ file, None, what the case is made of), laid out as
    unitig_bubble_cases lays its cases out -- haplotypes tiled into reads of ``read_len`` bases (default 80 up to k = 33, 140
    above: an 80-base read holds 17 windows of k = 64, and a haplotype written once is not solid) at a step of 10.  A is a
    random sequence of 400 bases, p = 200, u = A[p - k : p] the fork and t = A[p + 1 : p + 1 + k] the merge of a substitution
    at p.  Strings compare as the 2k-bit keys do (A < C < G < T), so which side judges a bubble (u < rc(t)) and on which strand
    a fork is stored (u < rc(u)) is decided here: where a case needs one of the two, A is the first of a sequence of seeds
    that has it.  ``fork`` and ``merge`` in what a case is made of are these strings.

    four_way      the four bases at p, x 4, x 3, x 2, x 2: one bubble of four branches, every lane of the quad walks
    two_pairs     A x 3, A with the second base at p x 2, C = A with the third base at p and a substitution at p + 5 x 3,
                  D = C with the fourth base at p x 2, and u < rc(t) for both merges: one quad judges two bubbles
    homopolymer   left + 'A' (k - 1) + right x 3, left + 'A' (k - 2) + right x 2: branches of 2 and of 1 k-mers
    blocked_lane  three bases at p, x 3, x 2, x 1, and a path x 2 that joins the second k-mer of the x 2 branch: that lane's
                  walk ends at a merge of its own, the other two lanes are a bubble.  (The first k-mers of a fork's branches
                  share their first k - 1 bases and so their predecessors: one of them alone cannot be joined)
    blocked_fork  the same with the path joining the first k-mers: every branch starts at a merge, no lane walks
    second_phase  A x 3, the substitution x 2, and Dg = R + A[p - 5 : p - 5 + read_len] x 2 beside Dg with a substitution at
                  k + 4 x 2, R random of 2k + 10 bases; trim = bubble = 3k.  Dg's bubble pops in the first phase, R is then a
                  tip, and without R the junction inside A's branch is gone: A's bubble pops in the second phase
    limit_split   A x 3, A without its bases p, p + 1 x 2 (indel_long): branches of k + 1 and k - 1 k-mers
    near_tie_a/b  A x 2, the deletion x 2, and reads of k bases, one k-mer each, from the middle of either branch, as many as
                  bring sum_a len_b - sum_b len_a into (0, min len) -- the longer branch a wins by less than one branch
                  length -- or into (-min len, 0)
    tie_fwd/rev   A x 2, the substitution x 2, the judging fork on its canonical strand / on the other one
    two_loops     L + U + X1 + U + X2 + U + R x 2 with U of k and X1, X2 of 10 bases: two branches that leave U and come back
                  to it, fork and merge are one oriented node
    even k only, x of k / 2 bases:
    selfcomp_fork   L + x + rc(x) + c + R for two bases c, x 3 and x 2, and u = x + rc(x) < rc(t)
    selfcomp_merge  L + c + x + rc(x) + R likewise, and u < t = x + rc(x)
    hairpin_even    P + AT + rc(P) x 3 beside P + CG + rc(P) x 2: a self-complementary k-mer in the middle of either branch"""
    L = int(read_len) if read_len else (80 if k <= 33 else 140)
    snp, rc, p = _snp, _revcomp, 200

    def case(haps, extra=(), **kw):
        return _bubble_case(haps, extra, L, **dict({"bubble": 3 * k, "trim": k}, **kw))

    def fork(A):
        return A[p - k:p]

    def merge(A):
        return A[p + 1:p + 1 + k]

    def judged_from_u(A):
        return _plain_kmers(A, k) and fork(A) < rc(merge(A))

    out = {}
    A = _pick(400, 501, judged_from_u)
    out["four_way"] = case([(A, 4), (snp(A, p, 1), 3), (snp(A, p, 2), 2), (snp(A, p, 3), 2)], fork=fork(A), merge=merge(A))

    A = _pick(400, 502, lambda s: judged_from_u(s) and fork(s) < rc(merge(snp(s, p + 5))))
    C = snp(snp(A, p, 2), p + 5)
    out["two_pairs"] = case([(A, 3), (snp(A, p, 1), 2), (C, 3), (snp(C, p, 1), 2)], fork=fork(A), merge=merge(A), merge2=merge(C))

    left = _pick(200, 503, lambda s: s[-1:] != b"A" and _plain_kmers(s, k))
    right = _pick(200, 504, lambda s: s[:1] != b"A" and _plain_kmers(s, k))
    out["homopolymer"] = case([(left + b"A" * (k - 1) + right, 3), (left + b"A" * (k - 2) + right, 2)],
                              short=left[-1:] + b"A" * (k - 2) + right[:1])

    A = _pick(400, 505, judged_from_u)
    B, R = snp(A, p, 1), genome_bases(2 * k + 10, 506).tobytes()
    three = [(A, 3), (B, 2), (snp(A, p, 2), 1)]
    join2 = R + bytes([_other_base(A[p - k + 1], 1)]) + B[p - k + 2:p - k + 2 + L]
    join1 = R + bytes([_other_base(A[p - k], 1)]) + B[p - k + 1:p - k + 1 + L]
    out["blocked_lane"] = case(three + [(join2, 2)], fork=fork(A), merge=merge(A), blocked=B[p - k + 1:p + 1])
    out["blocked_fork"] = case(three + [(join1, 2)], fork=fork(A), merge=merge(A))

    A = _pick(400, 507, lambda s: _plain_kmers(s, k))
    Dg = genome_bases(2 * k + 10, 508).tobytes() + A[p - 5:p - 5 + L]
    out["second_phase"] = case([(A, 3), (snp(A, p), 2), (Dg, 2), (snp(Dg, k + 4), 2)], bubble=3 * k, trim=3 * k)

    A = _pick(400, 509, lambda s: _plain_kmers(s, k))
    dele = A[:p] + A[p + 2:]
    out["limit_split"] = case([(A, 3), (dele, 2)])

    # the near ties: the branches are the k-mers of one haplotype alone; every k-mer of the tiled reads is counted here
    A = _pick(400, 510, lambda s: _plain_kmers(s, k))
    dele = A[:p] + A[p + 2:]
    mers = lambda s: [s[i:i + k] for i in range(len(s) - k + 1)]
    a = [m for m in mers(A) if m not in set(mers(dele))]
    b = [m for m in mers(dele) if m not in set(mers(A))]
    count = {}
    for seq, m in ((A, 2), (dele, 2)):
        for r in _tile(seq, L):
            for w in mers(r):
                count[w] = count.get(w, 0) + m
    d0 = sum(count[m] for m in a) * len(b) - sum(count[m] for m in b) * len(a)
    for name, sign in (("near_tie_a", 1), ("near_tie_b", -1)):
        x, y = next((x, n - x) for n in range(2000) for x in range(n + 1)
                    if 0 < sign * (d0 + x * len(b) - (n - x) * len(a)) < min(len(a), len(b)))
        out[name] = case([(A, 2), (dele, 2)], extra=[a[len(a) // 2]] * x + [b[len(b) // 2]] * y, extra_a=x, extra_b=y)

    def judging(A):
        return min(fork(A), rc(merge(A)))

    A = _pick(400, 511, lambda s: _plain_kmers(s, k) and judging(s) < rc(judging(s)))
    out["tie_fwd"] = case([(A, 2), (snp(A, p), 2)], fork=fork(A), merge=merge(A))
    A = _pick(400, 512, lambda s: _plain_kmers(s, k) and judging(s) > rc(judging(s)))
    out["tie_rev"] = case([(A, 2), (snp(A, p), 2)], fork=fork(A), merge=merge(A))

    Lf, Rr, U = genome_bases(150, 513).tobytes(), genome_bases(150, 514).tobytes(), genome_bases(k, 515).tobytes()
    X1, X2 = genome_bases(10, 516).tobytes(), genome_bases(10, 517).tobytes()
    X1 = bytes([_other_base(Rr[0], 1)]) + X1[1:-1] + bytes([_other_base(Lf[-1], 1)])
    X2 = bytes([_other_base(Rr[0], 2)]) + X2[1:-1] + bytes([_other_base(Lf[-1], 2)])
    out["two_loops"] = case([(Lf + U + X1 + U + X2 + U + Rr, 2)], fork=U)

    if k % 2 == 0:
        comp = lambda c: rc(bytes([c]))[0]
        Lf, Rr = genome_bases(150, 521).tobytes(), genome_bases(150, 522).tobytes()
        x = _pick(k // 2, 523, lambda s: s + rc(s) < rc(Rr[:k]))
        cs = [c for c in b"ACGT" if c != comp(Lf[-1])][:2]
        out["selfcomp_fork"] = case([(Lf + x + rc(x) + bytes([c]) + Rr, m) for c, m in zip(cs, (3, 2))], fork=x + rc(x), merge=Rr[:k])
        x = _pick(k // 2, 524, lambda s: Lf[-k:] < s + rc(s))
        cs = [c for c in b"ACGT" if c != comp(Rr[0])][:2]
        out["selfcomp_merge"] = case([(Lf + bytes([c]) + x + rc(x) + Rr, m) for c, m in zip(cs, (3, 2))], fork=Lf[-k:], merge=x + rc(x))
        P = genome_bases(150, 525).tobytes()
        out["hairpin_even"] = case([(P + b"AT" + rc(P), 3), (P + b"CG" + rc(P), 2)], fork=P[-k:])
    return out


def unitig_bubble_cap_cases(k=21, d=5):
    """Two inputs at the cap of rule 9's parameter (MSGPU_UG_BUBBLE_MAX = 4096): A of 4500 random bases x 3 beside A with a
    substitution every ``d`` bases from position 200 on x 2, tiled into 80-base reads.  With m sites the two branches have
    (m - 1) d + k k-mers each: 4096 in ``cap_4096``; ``cap_4097`` has one more site, one base behind the last."""
    m = (4096 - k) // d + 1
    assert (m - 1) * d + k == 4096
    A = _pick(4500, 531, lambda s: _plain_kmers(s, k))
    B = A
    for i in range(m):
        B = _snp(B, 200 + i * d)
    meta = dict(bubble=4096, trim=k)
    return {"cap_4096": _bubble_case([(A, 3), (B, 2)], (), 80, branch=4096, **meta),
            "cap_4097": _bubble_case([(A, 3), (_snp(B, 200 + (m - 1) * d + 1), 2)], (), 80, branch=4097, **meta)}


def unitig_tangle(k, genome, seed):
    """A tangled input of rule 9: (FASTQ file, None, what it is made of).  A random genome of ``genome`` bases and three
    copies of it edited at two positions in 5k -- half substitutions, a quarter insertions of a base, a quarter deletions of
    one; each whole sequence is one read, written one to three times.  At k = 8 .. 12 the k-mers repeat by chance: hundreds of
    forks, bubbles inside and beside each other, branches from one k-mer on.  To be run at min_count = 1."""
    g = genome_bases(genome, seed)
    seqs = [g.tobytes()]
    for j in range(3):
        hit = (splitmix64(seed, 100 + j, genome) % np.uint64(5 * k)) < np.uint64(2)
        kind = splitmix64(seed, 110 + j, genome) % np.uint64(4)  # 0, 1: substitution, 2: insertion, 3: deletion
        draw = splitmix64(seed, 120 + j, genome)
        parts = []
        for i in range(genome):
            b = int(g[i])
            if not hit[i]:
                parts.append(b)
            elif kind[i] < 2:
                parts.append(_other_base(b, int(draw[i] % np.uint64(3)) + 1))
            elif kind[i] == 2:
                parts += [b"ACGT"[int(draw[i] % np.uint64(4))], b]
        seqs.append(bytes(parts))
    times = [int(x) + 1 for x in splitmix64(seed, 130, 4) % np.uint64(3)]
    reads = [s for s, m in zip(seqs, times) for _ in range(m)]
    fq = b"".join(b"@t%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)) for i, r in enumerate(reads))
    return fq, None, {"sequences": list(zip(seqs, times)), "bubble": 3 * k, "trim": k, "min_count": 1}


def mapper_workload(n_reads, read_len, n_unitigs, seed, coverage=10, error=0.06, families=2, copies=6, repeat_len=600,
                    n_frac=0.0005, lower_frac=0.001, tiled=False, unitig_len=(500, 3000), fastq=True):
    """Input of the mapper (muchsalsa_amd.mapper): a dict with ``reads`` (FASTQ bytes, or FASTA with fastq=False),
    ``unitigs`` (FASTA bytes), ``genome`` (bytes) and the layout (``read_start``, ``read_fwd``, ``unitig_start``,
    ``unitig_fwd``, ``unitig_len``).

    A uniform genome of n_reads * read_len / coverage bases (at least read_len + 3500) in which ``families`` repeat units of
    ``repeat_len`` bases are each written ``copies`` times, as kmer_filter_workload does it.  Read r<i> is read_len genome
    bases from a uniform start, every other one (a drawn bit) reverse-complemented, then edited: a fraction ``error`` of its
    bases, split evenly, is replaced by another base, followed by an inserted drawn base, or deleted; after that ``n_frac``
    of the bases become 'N' and ``lower_frac`` lower case.  Unitig u<i> is an error-free stretch of
    U{unitig_len[0]..unitig_len[1]} bases at a uniform start, or with ``tiled`` the consecutive stretches that cover the
    genome end to end (n_unitigs is ignored); every other one (a drawn bit) is written reverse-complemented.
    Deterministic in (seed, shape)."""
    L = int(read_len)
    G = max(int(n_reads) * L // int(coverage), L + unitig_len[1] + 500)
    g = _planted_genome(G, seed, families, copies, repeat_len, 80)
    recs, r_start, r_fwd = _long_reads(g, n_reads, L, seed, error, n_frac, lower_frac, fastq)
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    if tiled:
        n_max = G // unitig_len[0] + 2
        u_len = _randint(seed, 84, n_max, unitig_len[0], unitig_len[1])
        u_start = np.cumsum(u_len) - u_len
        keep = u_start < G
        u_start, u_len = u_start[keep], np.minimum(u_len[keep], G - u_start[keep])
    else:
        u_len = _randint(seed, 84, n_unitigs, unitig_len[0], unitig_len[1])
        u_start = _randint(seed, 85, n_unitigs, 0, G - u_len)
    u_fwd = (splitmix64(seed, 86, len(u_len)) & np.uint64(1)).astype(bool)
    unitigs = []
    for i in range(len(u_len)):
        seq = g[u_start[i]:u_start[i] + u_len[i]]
        unitigs.append(b">u%d\n%s\n" % (i, (seq if u_fwd[i] else comp[seq[::-1]]).tobytes()))
    return {"reads": b"".join(recs), "unitigs": b"".join(unitigs), "genome": g.tobytes(), "read_start": r_start, "read_fwd": r_fwd,
            "unitig_start": u_start, "unitig_fwd": u_fwd, "unitig_len": u_len}


def _long_reads(g, n_reads, L, seed, error, n_frac, lower_frac, fastq):
    """the reads of mapper_workload from the genome ``g`` -> (records, start of every read, its strand)"""
    G = len(g)
    comp = np.arange(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    sub = np.zeros((256, 3), np.uint8)
    for b, t in {65: b"CGT", 67: b"GTA", 71: b"TAC", 84: b"ACG"}.items():
        sub[b] = list(t)
    r_start = _randint(seed, 82, n_reads, 0, G - L)
    r_fwd = (splitmix64(seed, 83, n_reads) & np.uint64(1)).astype(bool)
    recs = []
    col = np.arange(L, dtype=np.int64)[None, :]
    step = max(1, (1 << 22) // L)
    for lo in range(0, int(n_reads), step):
        hi = min(lo + step, int(n_reads))
        n = hi - lo
        fw = g[r_start[lo:hi, None] + col]
        rv = comp[g[(r_start[lo:hi] + L - 1)[:, None] - col]]
        flat = np.ascontiguousarray(np.where(r_fwd[lo:hi, None], fw, rv)).reshape(-1)
        u = _uniform(seed, 1000 + 4 * (lo // step), n * L, 0.0, 1.0)
        draw = (splitmix64(seed, 1001 + 4 * (lo // step), n * L) % np.uint64(12)).astype(np.int64)
        is_sub, is_ins, is_del = u < error / 3, (u >= error / 3) & (u < 2 * error / 3), (u >= 2 * error / 3) & (u < error)
        flat = np.where(is_sub, sub[flat, draw % 3], flat)
        count = 1 + is_ins.astype(np.int64) - is_del.astype(np.int64)
        out = np.repeat(flat, count)
        first = np.cumsum(count) - count
        out[first[is_ins] + 1] = np.frombuffer(b"ACGT", np.uint8)[draw[is_ins] // 3]
        lens = count.reshape(n, L).sum(axis=1)
        nb = len(out)
        out[_randint(seed, 1002 + 4 * (lo // step), int(nb * n_frac), 0, nb - 1)] = ord("N")
        out[_randint(seed, 1003 + 4 * (lo // step), int(nb * lower_frac), 0, nb - 1)] |= 0x20
        ends = np.cumsum(lens)
        for i in range(n):
            seq = out[ends[i] - lens[i]:ends[i]].tobytes()
            recs.append(b"@r%d\n%s\n+\n%s\n" % (lo + i, seq, b"I" * len(seq)) if fastq else b">r%d\n%s\n" % (lo + i, seq))
    return recs, r_start, r_fwd


def hybrid_workload(genome, seed, coverage=40, read_len=100, n_long=50, long_len=3000, families=2, copies=6, repeat_len=400,
                    error=0.005, long_error=0.06, n_frac=0.0005, lower_frac=0.001, fastq=True):
    """Input of the whole pipeline (muchsalsa_amd.hybrid): a dict with ``illumina_1`` / ``illumina_2`` (FASTQ bytes), ``reads``
    (the long reads: FASTQ bytes, or FASTA with fastq=False) and ``genome`` (bytes), all from ONE genome.

    The genome has ``genome`` bases with planted repeats, made as kmer_filter_workload makes them (``families`` units of
    ``repeat_len`` bases, ``copies`` each).  The Illumina pairs are drawn from it as kmer_filter_workload draws them
    (``coverage``, ``read_len``, ``error``); the ``n_long`` long reads of ``long_len`` genome bases as mapper_workload draws
    and edits them (``long_error``).  Deterministic in (seed, shape).

    The planted repeats carry the k-mer filter's abundant k-mers: the filter drops the pairs that touch them, so the unitigs
    end at the repeats and none lies inside one.  An outlier of the unitig coverage filter is then no repeat but the unitig
    on which the drawn long reads happen to pile up; whether there is one depends on the seed and on ``n_long``."""
    G, L = int(genome), int(read_len)
    insert = (5 * L) // 2
    g = _planted_genome(G, seed, families, copies, repeat_len, 70, at_least=insert)
    one, two = _illumina_pairs(g, coverage, L, seed, error, n_frac, lower_frac, insert)
    recs, r_start, r_fwd = _long_reads(g, n_long, int(long_len), seed + 2, long_error, n_frac, lower_frac, fastq)  # (streams of their own)
    return {"illumina_1": one, "illumina_2": two, "reads": b"".join(recs), "genome": g.tobytes(), "read_start": r_start,
            "read_fwd": r_fwd}


def mates_workload(genome=4000, seed=1, coverage=8, read_len=100, insert=300, repeat_len=250, copies=2, error=0.0, n_frac=0.0,
                   lower_frac=0.0):
    """Input of the mapper's rule 13 (mates): a dict with ``genome`` (bytes: one record's bases), ``illumina_1`` / ``illumina_2``
    (FASTQ bytes) and ``repeats`` (the start of every copy of the repeat).  The genome has ``genome`` bases and one repeat unit
    of ``repeat_len`` bases written ``copies`` times, as kmer_filter_workload plants it; the pairs are drawn from it as
    kmer_filter_workload draws them, fragments of ``insert`` bases.  A read that falls inside a copy maps equally well onto
    every copy; its mate in the unique flank says which.  Deterministic in (seed, shape)."""
    G, L = int(genome), int(read_len)
    g = _planted_genome(G, seed, 1, copies, repeat_len, 70, at_least=int(insert))
    unit = genome_bases(int(repeat_len), seed + 1).tobytes()
    text = g.tobytes()
    starts, at = [], text.find(unit)
    while at >= 0:
        starts.append(at)
        at = text.find(unit, at + 1)
    one, two = _illumina_pairs(g, coverage, L, seed, error, n_frac, lower_frac, int(insert))
    return {"genome": text, "illumina_1": one, "illumina_2": two, "repeats": starts}
