"""Edge inputs of the read scrubber (msgpu_scrub.hip), built against the way its kernels are written and shared by
tests/test_scrub_uf_edges_host.py, tests/test_gpu_scrub_uf_edges.py and tools/make_scrubber_fixtures.py --only edges:
``cases()`` maps a name to Case(anchors, ava, reads, subset_size, note, lit, extra), ``expected(name)`` is the plain-Python
restatement's result (scrub_oracle.scrub, once per process).  ``note`` names the kernel line the case aims at; ``lit`` holds
the hand-derived figures: ``records`` (record name -> bases, of every record of the output unless ``partial``), ``edges``,
``pairs``, ``chunks``, ``batches``; ``extra`` holds what the host test needs to show that the case is not vacuous.  Every
input is built deterministically; the only random draws are the bases (numpy.random.default_rng(seed)).

A record of the covered range (cs, ce) on a read of PAF length L holds the bases [max(cs, 200), min(ce, L - 200)], so the
state (S, E) of a pair is read off the record's length.

Graph:   no_pairs, no_pairs_but_lines, no_ava_lines, all_ava_lines_drop, one_node, chunk_sizes, late_first_pair,
         anchor_name_returns
Fold:    near_499_500, strand, chain_of_130, chain_of_130_reversed, lane_phases, three_batches, never_together
Union and output: touching, contained_and_identical, 300_merge_into_one, 300_stay_apart, inside_the_trim, length_200,
         record_shorter_than_paf, wrap
"""
import collections
import functools

import numpy as np

import scrub_oracle

Case = collections.namedtuple("Case", "anchors ava reads subset_size note lit extra")


def bases(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def line(a, b, s, e, strand="+", alen=4000, blen=4000, sb=None, eb=None):
    sb, eb = (s if sb is None else sb), (e if eb is None else eb)
    return b"%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t60\n" % (a, alen, s, e, strand.encode(), b, blen, sb, eb, e - s, e - s)


def hit(u, r, s, e, blen=4000):
    """an anchor line: anchor u on read r, the anchor range (s, e)"""
    return line(u, r, 0, 600, alen=900, blen=blen, sb=s, eb=e)


def fasta(names, n=4000, seed=0):
    return b"".join(b">%s\n%s\n" % (r, bases(n, seed + i)) for i, r in enumerate(names))


def span(cs, ce, length=4000):
    """bases of the record of the covered range (cs, ce)"""
    return max(min(ce, length - 200) - max(cs, 200) + 1, 0)


def _case(c, name, anchors, ava, reads, note, lit, subset_size=scrub_oracle.SUBSET_SIZE, **extra):
    c[name] = Case(anchors, ava, reads, subset_size, note, lit, extra)


# ---- graph --------------------------------------------------------------------------------------------------------------

DROPPED = (line(b"A", b"A", 1000, 2000) + line(b"A", b"stranger", 1000, 2000) + line(b"A", b"B", 1000, 1499) + b"token\n")


def chunk_sizes_anchors():
    """chunks of 2, 3, 64, 65 and 257 lines over a pool of 300 reads, every chunk a stride through the pool"""
    out = []
    for k, (n, first, step) in enumerate(((2, 0, 7), (3, 7, 7), (64, 0, 7), (65, 14, 11), (257, 3, 1), (3, 0, 7))):
        out.append(b"".join(hit(b"u%d" % k, b"r%d" % ((first + i * step) % 300), 300, 700, 1000) for i in range(n)))
    return out


def late_first_pair_chunks():
    """c1: 63 reads, then X, Y (the edge X-Y is the LAST pair of the chunk); X-Z1 and Y-Z2; c3: X, Y first"""
    c1 = b"".join(hit(b"c1", b"r%02d" % i, 300, 900) for i in range(63)) + hit(b"c1", b"X", 300, 900) + hit(b"c1", b"Y", 300, 900)
    mid = hit(b"m1", b"X", 1000, 1600) + hit(b"m1", b"Z1", 300, 900) + hit(b"m2", b"Y", 1000, 1600) + hit(b"m2", b"Z2", 300, 900)
    c3 = hit(b"c3", b"X", 2000, 2600) + hit(b"c3", b"Y", 2000, 2600) + hit(b"c3", b"Z3", 300, 900)
    return c1, mid, c3


def _graph_cases(c):
    four = [b"A", b"B", b"C", b"D"]
    alone = b"".join(hit(b"u%d" % i, r, 300, 900) for i, r in enumerate(four))
    lit = dict(edges=0, pairs=0, chunks=4, batches=1, records={r + b"_0": 601 for r in four})
    _case(c, "no_pairs", alone, b"", fasta(four), "P == 0: the graph block is skipped, row_off stays zero, adj is empty", lit)
    _case(c, "no_pairs_but_lines", alone, line(b"A", b"C", 1000, 2000) + line(b"D", b"A", 2500, 3100, sb=2500, eb=3200),
          fasta(four),
          "P == 0 with entries to fold: the components merge into one subset",
          dict(lit, records={b"A_0": 601, b"A_1": 1001, b"A_2": 701, b"B_0": 601, b"C_0": 601, b"C_1": 1001, b"D_0": 601,
                             b"D_1": 601}))
    edged = (hit(b"u1", b"A", 300, 900) + hit(b"u1", b"B", 300, 900) + hit(b"u1", b"C", 300, 900) + hit(b"u2", b"C", 1000, 1600) +
             hit(b"u2", b"D", 300, 900))
    lit = dict(edges=4, pairs=4, chunks=2, batches=1, ava_lines=0,
               records={b"A_0": 601, b"B_0": 601, b"C_0": 601, b"C_1": 601, b"D_0": 601})
    _case(c, "no_ava_lines", edged, b"", fasta(four), "A == 0: d_ek stays null, ent_off is memset, every slot an anchor range",
          lit)
    _case(c, "all_ava_lines_drop", edged, DROPPED, fasta(four),
          "rule 3 on the host: the same name twice, an unknown read, col3 - col2 = 499, one token", lit)
    _case(c, "one_node", hit(b"u1", b"A", 300, 900), b"", fasta([b"A"]), "N == 1: grids of one thread, one batch of one",
          dict(edges=0, pairs=0, chunks=1, batches=1, records={b"A_0": 601}))
    pool = [b"r%d" % i for i in range(300)]
    _case(c, "chunk_sizes", b"".join(chunk_sizes_anchors()),
          line(b"r0", b"r7", 100, 700, blen=1000, alen=1000) + line(b"r3", b"r4", 250, 800, "-", blen=1000, alen=1000),
          fasta(pool, 1000, 50),
          "k_scrub_pairs' (j, i) from the square root at chunks of 2, 3, 64, 65 and 257 lines; k_scrub_first over repeated edges",
          dict(pairs=1 + 3 + 2016 + 2080 + 32896 + 3, chunks=6, partial=True,
               records={b"r0_0": 501, b"r7_0": 501, b"r3_0": 551, b"r4_0": 551, b"r259_0": 401}))
    c1, mid, c3 = late_first_pair_chunks()
    reads = [b"r%02d" % i for i in range(63)] + [b"X", b"Y", b"Z1", b"Z2", b"Z3"]
    _case(c, "late_first_pair", c1 + mid + c3, line(b"X", b"Y", 1000, 2000), fasta(reads, 4000, 70),
          "the stable sort of (edge, ord): the edge X-Y keeps time pair_off[1] - 1, not the time of its pair in the last chunk",
          dict(pairs=2080 + 1 + 1 + 3, edges=2080 + 1 + 1 + 2, chunks=4, partial=True, records={}),
          moved=mid + c3 + c1, row_x=list(range(63)) + [64, 65, 67], row_y=list(range(64)) + [66, 67])
    _case(c, "anchor_name_returns",
          hit(b"u1", b"A", 300, 900) + hit(b"u1", b"B", 300, 900) + hit(b"u2", b"C", 300, 900) + hit(b"u1", b"D", 300, 900) +
          hit(b"u1", b"E", 300, 900), line(b"A", b"B", 1000, 2000), fasta([b"A", b"B", b"C", b"D", b"E"]),
          "a chunk is a RUN of one column 0: u1 after u2 starts a new chunk, A and D get no edge",
          dict(pairs=2, edges=2, chunks=3, batches=1,
               records={b"A_0": 601, b"A_1": 1001, b"B_0": 601, b"B_1": 1001, b"C_0": 601, b"D_0": 601, b"E_0": 601}))


# ---- fold ---------------------------------------------------------------------------------------------------------------

def chain_lines(reverse=False):
    """130 lines of the pair (P, Q), the column order alternating: line 0 in the middle, the odd lines each 300 beyond the
    right end, the even lines each 300 before the left end"""
    out, lo, hi = [], 60000, 60600
    for i in range(130):
        if i == 0:
            s, e = lo, hi
        elif i % 2:
            s, e = hi + 300, hi + 900
            hi = e
        else:
            s, e = lo - 900, lo - 300
            lo = s
        out.append(line(b"P", b"Q", s, e, alen=120000, blen=120000) if i % 2 == 0 else line(b"Q", b"P", s, e, alen=120000,
                                                                                           blen=120000))
    return b"".join(out[::-1] if reverse else out), (lo, hi)


HUBS = ((b"h64", 64), (b"h65", 65), (b"h129", 129))


def lane_phase_files():
    """three hubs with 64, 65 and 129 partners, each hub and its partners one chunk; partner i has 1 + i % 3 lines with the
    hub: a first line, a second that joins it, a third on the other strand"""
    anchors, ava, names, want = [], [], [], {}
    for h, n in HUBS:
        ps = [b"%s_p%03d" % (h, i) for i in range(n)]
        names += [h] + ps
        anchors.append(b"".join(hit(b"u_" + h, r, 2700, 2790, 3000) for r in [h] + ps))
        for i, p in enumerate(ps):
            s = 300 + 20 * (i % 7)
            a, b = (h, p) if i % 2 else (p, h)
            ava.append((0, line(a, b, s, s + 600, "+-"[i % 2], 3000, 3000)))
            if i % 3 >= 1:
                ava.append((1, line(b, a, s + 700, s + 1300, "+-"[i % 2], 3000, 3000)))
            if i % 3 == 2:
                ava.append((2, line(a, b, s + 1400, s + 2000, "+-"[(i + 1) % 2], 3000, 3000)))
            want[p + b"_0"] = 601 if i % 3 == 0 else 1301
            want[p + b"_1"] = 91
        want[h + b"_0"] = (300 + 120 + 1300) - 300 + 1  # the union of its groups: [300, 1720]
        want[h + b"_1"] = 91
    # every first line, then every second, then every third: no group's lines are neighbours in the file
    ava = [l for rank in range(3) for r, l in ava if r == rank]
    return b"".join(anchors), b"".join(ava), names, want


def group_heads(anchors, ava, hub):
    """the places, among the hub's entries sorted by partner, where a group starts"""
    g = scrub_oracle.read_graph(anchors)
    x = g["node"][hub.decode()]
    partners = sorted([b for a, b, *_ in scrub_oracle.ava_lines(ava, g["node"]) if a == x] +
                      [a for a, b, *_ in scrub_oracle.ava_lines(ava, g["node"]) if b == x])
    return [i for i, p in enumerate(partners) if i == 0 or partners[i - 1] != p]


def three_batch_anchors(with_f=True):
    out = (hit(b"u1", b"A", 300, 900, 5000) + hit(b"u1", b"B", 300, 900, 5000) + hit(b"u1", b"C", 3500, 3900, 5000) +
           hit(b"u2", b"B", 400, 800, 5000) + hit(b"u2", b"D", 300, 900, 5000) + hit(b"u3", b"C", 3400, 3950, 5000) +
           hit(b"u3", b"E", 300, 900, 5000))
    return out + (hit(b"u4", b"B", 500, 700, 5000) + hit(b"u4", b"F", 300, 900, 5000) if with_f else b"")


def _fold_cases(c):
    # four pairs, state (2000, 3000), then a second line at 499 / 500 from either end
    eight = [b"%s%d" % (x, i) for i in range(4) for x in (b"P", b"Q")]
    anchors = b"".join(hit(b"u0", r, 8200, 8700, 9000) for r in eight)
    second = ((1001, 1501), (1000, 1500), (3499, 4000), (3500, 4000))
    ava = b"".join(line(b"P%d" % i, b"Q%d" % i, 2000, 3000, alen=9000, blen=9000) for i in range(4))
    ava += b"".join(line(b"Q%d" % i, b"P%d" % i, s, e, alen=9000, blen=9000) for i, (s, e) in enumerate(second))
    want = {}
    for i, n in enumerate((2000, 1001, 2001, 1001)):  # (1001, 3000), (2000, 3000), (2000, 4000), (2000, 3000)
        for x in (b"P", b"Q"):
            want[b"%s%d_0" % (x, i)] = n
            want[b"%s%d_1" % (x, i)] = 501
    _case(c, "near_499_500", anchors, ava, fasta(eight, 9000, 10), "abs(S - e) < SC_NEAR and abs(s - E) < SC_NEAR at 499 and 500",
          dict(pairs=28, edges=28, chunks=1, batches=1, records=want))

    six = [b"P1", b"Q1", b"P2", b"Q2", b"P3", b"Q3"]
    anchors = b"".join(hit(b"u0", r, 8200, 8700, 9000) for r in six)

    def l9(a, b, s, e, d):
        return line(a, b, s, e, d, 9000, 9000)

    # the states end at (2000, 3900), (2000, 3000) and (2000, 3700)
    ava = (l9(b"P1", b"Q1", 2000, 3000, "-") + l9(b"P1", b"Q1", 1600, 2300, "+") + l9(b"Q1", b"P1", 3200, 3900, "-") +
           l9(b"P2", b"Q2", 2000, 3000, "+") + l9(b"P2", b"Q2", 3100, 3700, "-") + l9(b"P2", b"Q2", 3800, 4400, "-") +
           l9(b"P3", b"Q3", 2000, 3000, "*") + l9(b"P3", b"Q3", 1600, 2300, "+") + l9(b"Q3", b"P3", 3100, 3700, "*"))
    want = {}
    for i, n in ((1, 1901), (2, 1001), (3, 1701)):
        for x in (b"P", b"Q"):
            want[b"%s%d_0" % (x, i)] = n
            want[b"%s%d_1" % (x, i)] = 501
    _case(c, "strand", anchors, ava, fasta(six, 9000, 20),
          "d == D: the first line fixes D for good; a near line of another strand is ignored; '*' is a strand like any other",
          dict(pairs=15, edges=15, chunks=1, batches=1, records=want))

    anchors = hit(b"u0", b"P", 60100, 60500, 120000) + hit(b"u0", b"Q", 60100, 60500, 120000)
    reads = fasta([b"P", b"Q"], 120000, 30)
    ava, (lo, hi) = chain_lines()
    assert (lo, hi) == (2400, 119100)
    _case(c, "chain_of_130", anchors, ava, reads,
          "the walk for (j = i; keys[j] == k) carries (S, E) from line to line in FILE order (the stable sort of the entries)",
          dict(pairs=1, edges=1, chunks=1, batches=1, records={b"P_0": 116701, b"Q_0": 116701}))
    # reversed, the left-hand lines are met while the state is still on the right: only line 0, met last, joins on the left
    _case(c, "chain_of_130_reversed", anchors, chain_lines(True)[0], reads, "the same lines in reverse file order",
          dict(pairs=1, edges=1, chunks=1, batches=1, records={b"P_0": 59101, b"Q_0": 59101}))

    anchors, ava, names, want = lane_phase_files()
    _case(c, "lane_phases", anchors, ava, fasta(names, 3000, 40),
          "i = e0 + lane, i += 64 with keys[i - 1] == k: group heads on every lane, groups that straddle a stride",
          dict(pairs=65 * 64 // 2 + 66 * 65 // 2 + 130 * 129 // 2, chunks=3, batches=1, records=want))

    # test_gpu_scrubber.test_fold_changes_in_a_later_batch with a third batch: B keeps the neighbour F through batch 2
    ava = (line(b"B", b"C", 0, 1000, alen=5000, blen=5000) + line(b"C", b"B", 3300, 3900, alen=5000, blen=5000) +
           line(b"C", b"B", 2000, 3000, alen=5000, blen=5000) + line(b"B", b"C", 1200, 1900, alen=5000, blen=5000))
    six = [b"A", b"B", b"C", b"D", b"E", b"F"]
    _case(c, "three_batches", three_batch_anchors(), ava, fasta(six, 5000, 60),
          "st_s / st_e / st_d persist from batch to batch: walk 1 ends at (0, 1900), walk 2 at (0, 3000), walk 3 at (0, 3900)",
          dict(batches=4, chunks=4, records={b"A_0": 601, b"B_0": 3701, b"C_0": 3751, b"D_0": 601, b"E_0": 601, b"F_0": 601},
               plan=[(0, [0, 1, 2], [0]), (1, [1, 2, 3], [3]), (1, [1, 2, 5], [1, 5]), (2, [2, 4], [2, 4])]),
          subset_size=3, two_batch_anchors=three_batch_anchors(False), two_batch_b0=2801)

    anchors = hit(b"u1", b"A", 300, 900) + hit(b"u1", b"B", 300, 900) + hit(b"u2", b"C", 300, 900) + hit(b"u2", b"D", 300, 900)
    ava = line(b"A", b"C", 2000, 3000) + line(b"A", b"B", 1200, 1800) + line(b"C", b"D", 1200, 1800)
    _case(c, "never_together", anchors, ava, fasta([b"A", b"B", b"C", b"D"], 4000, 80),
          "a group whose partner is never stamped keeps st_d == SC_NONE: a sentinel slot, between live ones before the sort",
          dict(batches=2, chunks=2, edges=2, ava_lines=3,
               records={b"A_0": 601, b"A_1": 601, b"B_0": 601, b"B_1": 601, b"C_0": 601, b"C_1": 601, b"D_0": 601, b"D_1": 601}),
          subset_size=2, pair=(0, 2))


# ---- union and output ---------------------------------------------------------------------------------------------------

def ranges_case(ranges, blen=4000):
    """one read A with these anchor ranges, every one from an anchor of its own"""
    return b"".join(hit(b"u%d" % i, b"A", s, e, blen) for i, (s, e) in enumerate(ranges))


def _union_cases(c):
    one = dict(edges=0, pairs=0, batches=1)
    _case(c, "touching", ranges_case([(300, 900), (900, 1500), (1501, 1600)]), b"", fasta([b"A"], 4000, 90),
          "s <= ce in k_scrub_merge: s == ce joins, s == ce + 1 does not", dict(one, records={b"A_0": 1201, b"A_1": 100}))
    anchors = (hit(b"u0", b"A", 1000, 3000) + hit(b"u0", b"B", 1000, 3000) + hit(b"u1", b"A", 1500, 2000) +
               hit(b"u2", b"A", 1000, 3000) + hit(b"u3", b"A", 3200, 3600))
    _case(c, "contained_and_identical", anchors, line(b"A", b"B", 1000, 3000), fasta([b"A", b"B"], 4000, 91),
          "ce = max(e, ce) keeps the outer end; equal keys of an entry and of an anchor range",
          dict(edges=1, pairs=1, batches=1, records={b"A_0": 2001, b"A_1": 401, b"B_0": 2001}))
    scrambled = [(i * 7) % 300 for i in range(300)]
    _case(c, "300_merge_into_one", ranges_case([(300 + 10 * i, 310 + 10 * i) for i in scrambled]), b"", fasta([b"A"], 4000, 92),
          "300 slots of one node through the segmented sort, each touching the next", dict(one, records={b"A_0": 3001}))
    _case(c, "300_stay_apart", ranges_case([(300 + 10 * i, 309 + 10 * i) for i in scrambled]), b"", fasta([b"A"], 4000, 93),
          "s == ce + 1, 299 times: rec_off and the emit pass of k_scrub_merge",
          dict(one, records={b"A_%d" % i: 10 for i in range(300)}))
    _case(c, "inside_the_trim", ranges_case([(0, 150), (3900, 3999)]), b"", fasta([b"A"], 4000, 94),
          "lo = max(cs, 200) beyond hi, and hi = min(ce, length - 200) before lo: header lines alone",
          dict(one, records={b"A_0": 0, b"A_1": 0}))
    _case(c, "length_200", ranges_case([(0, 150)], 200), b"", fasta([b"A"], 200, 95), "length - SC_TRIM == 0",
          dict(one, records={b"A_0": 0}))
    _case(c, "record_shorter_than_paf", ranges_case([(2500, 3500), (3600, 3750)]), b"", fasta([b"A"], 3000, 96),
          "e = min(hi + 1, L), b = min(lo, L): a range across the record's end and one beyond it",
          dict(one, records={b"A_0": 500, b"A_1": 0}))
    _case(c, "wrap", ranges_case([(300, 358), (400, 459), (500, 560), (600, 719)]), b"", fasta([b"A"], 4000, 97),
          "hi + 1: the inclusive end; msgpu_fasta_format at 59, 60, 61 and 120 bases",
          dict(one, records={b"A_0": 59, b"A_1": 60, b"A_2": 61, b"A_3": 120}))


# ---- the cases ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    c = collections.OrderedDict()
    _graph_cases(c)
    _fold_cases(c)
    _union_cases(c)
    return c


def names():
    return list(cases())


def reads_of(name):
    return scrub_oracle.parse_fasta(cases()[name].reads)


@functools.lru_cache(maxsize=None)
def expected(name):
    """(batches, stats, text) of the restatement"""
    c = cases()[name]
    batches, st = scrub_oracle.scrub(c.anchors, c.ava, reads_of(name), c.subset_size)
    return batches, st, scrub_oracle.text(batches)


def record_lengths(text):
    return {h: len(body.replace(b"\n", b"")) for h, body in scrub_oracle.records(text).items()}


def meets_literals(name, text, counts):
    """the literals of a case that an output text and the counts (edges, pairs, chunks, batches, ava_lines where known) miss"""
    lit, bad = cases()[name].lit, []
    got = record_lengths(text)
    for h, n in lit["records"].items():
        if got.get(h) != n:
            bad.append("%s: %r bases, not %d" % (h.decode(), got.get(h), n))
    if not lit.get("partial") and set(got) != set(lit["records"]):
        bad.append("records %r" % sorted(set(got) ^ set(lit["records"])))
    for k in ("edges", "pairs", "chunks", "batches", "ava_lines"):
        if k in lit and k in counts and counts[k] != lit[k]:
            bad.append("%s: %d, not %d" % (k, counts[k], lit[k]))
    return bad
