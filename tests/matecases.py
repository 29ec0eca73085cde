"""Hand-made chain tables for rule 13 (the mapper's mates), shared by the host and the GPU file, with what each is made for.  A
chain is the tuple of msgpu_map_chain; only query, target, strand, score, t_start and t_end matter to the rule, the other fields
are filled so that a table could be a mapper's.  Pair p is the query records 2p and 2p + 1."""
import functools
import random

import map_mate_oracle as mo

# (n1, n2) by the kernel that takes the pair
SETTLED = ((1, 0), (0, 1), (1, 1))
LANES16 = ((1, 2), (2, 1), (8, 8), (1, 15), (15, 1))
LANES64 = ((16, 1), (1, 16), (32, 32), (63, 1), (1, 63))
LIST = ((64, 1), (1, 64), (65, 65), (130, 3), (3, 130))


def ch(q, score, ts, te, strand=0, target=0, anchors=5):
    return (q, target, strand, anchors, score, 0, 0, te - ts, ts, te, te - ts, te - ts)


def fr(p, score1, f, score2, r, target=0, flip=False):
    """pair p with one chain each: mate 1 forward on f = (ts, te), mate 2 reverse on r; flip: mate 1 is the reverse one"""
    if flip:
        return [ch(2 * p, score1, r[0], r[1], 1, target), ch(2 * p + 1, score2, f[0], f[1], 0, target)]
    return [ch(2 * p, score1, f[0], f[1], 0, target), ch(2 * p + 1, score2, r[0], r[1], 1, target)]


def random_pair(rng, p, n1, n2, span=1500):
    """n1 + n2 chains of pair p on two targets and both strands, 100 bases each, with score ties: about one combination in
    eight is concordant at max_insert = 1000"""
    out = []
    for mate, n in ((0, n1), (1, n2)):
        for _ in range(n):
            a = rng.randrange(0, span)
            out.append(ch(2 * p + mate, rng.choice((40, 60, 60, 80, 100, 100)), a, a + 100, rng.randrange(2), rng.randrange(2)))
    return out


def planted(p, n1, n2, a, b, decoy_score=200):
    """n1 + n2 chains of pair p of which exactly (a, b) is concordant: every other chain lies on a target of its own kind (mate
    1's decoys on target 1, mate 2's on target 2) with a better score than the planted two"""
    out = [ch(2 * p, decoy_score, 10 * i, 10 * i + 100, 0, 1) for i in range(n1)]
    out += [ch(2 * p + 1, decoy_score, 10 * i, 10 * i + 100, 1, 2) for i in range(n2)]
    out[a] = ch(2 * p, 50, 1000, 1100, 0, 0)
    out[n1 + b] = ch(2 * p + 1, 50, 1300, 1400, 1, 0)
    return out


def with_decoy(pair):
    """a (1, 1) pair as a (1, 2) pair: a second chain of mate 2 on a target nobody else uses, so that k_mt_lanes<16> decides
    what k_mt_classify decided"""
    q = pair[1][0]
    return [pair[0], pair[1], ch(q, 500, 0, 100, 1, 77)]


def renumber(pair, p):
    return [(2 * p + (c[0] & 1),) + c[1:] for c in pair]


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (chains, max_insert, what the table is made for)"""
    rng = random.Random(13)
    t = {}
    everything = []
    for p, (n1, n2) in enumerate(SETTLED + LANES16 + LANES64 + LIST):
        everything += random_pair(rng, p, n1, n2)
    everything += fr(len(SETTLED + LANES16 + LANES64 + LIST), 100, (0, 100), 100, (200, 300))
    everything += fr(len(SETTLED + LANES16 + LANES64 + LIST) + 1, 100, (500, 600), 100, (200, 300))
    t["classes"] = (everything, 1000, "every (n1, n2) of every kernel class in one table, a concordant and a discordant (1, 1) behind them")
    for n1, n2 in SETTLED + LANES16 + LANES64 + LIST:
        t["alone_%d_%d" % (n1, n2)] = (random_pair(rng, 3, n1, n2), 1000, "pair (%d, %d) as the only pair of its table" % (n1, n2))
    t["alone_1_1_concordant"] = (fr(0, 70, (10, 110), 60, (300, 400)), 1000, "one chain each, concordant: settled by the classifier")
    t["alone_1_1_discordant"] = (fr(0, 70, (10, 110), 60, (300, 400), target=0)[:1] + [ch(1, 60, 300, 400, 1, 1)], 1000,
                                 "one chain each on two targets: settled by the classifier, discordant")
    sizes16 = ((1, 2), (8, 8), (15, 1), (2, 3), (7, 9))
    for count in (1, 4, 5):
        chains = []
        for p in range(count):
            chains += random_pair(rng, p, *sizes16[p], span=600)
        t["lanes16_x%d" % count] = (chains, 1000, "%d pairs of the 16-lane class with different sizes: %s" % (
            count, {1: "one group of a wavefront, three idle", 4: "a full wavefront", 5: "a second wavefront with one group"}[count]))
    t["last_lane_16"] = (planted(0, 2, 2, 0, 0) + planted(1, 3, 3, 1, 2) + planted(2, 4, 4, 3, 3) + planted(3, 15, 1, 14, 0) +
                         planted(4, 1, 15, 0, 14), 1000,
                         "the only concordant combination sits in the last mate-1 lane of the wavefront's last group of 16, and in the last "
                         "mate-2 chain of a group")
    t["last_lane_64"] = (planted(0, 63, 1, 62, 0) + planted(1, 1, 63, 0, 62) + planted(2, 32, 32, 31, 31), 1000,
                         "the only concordant combination sits in the last mate-1 lane of a wavefront, and in its last mate-2 chain")
    t["last_of_last_tile"] = (planted(0, 130, 300, 129, 299) + planted(1, 65, 257, 64, 256), 1000,
                              "the only concordant combination is the last mate-1 chain of the last register tile against the last "
                              "mate-2 chain of the last LDS tile (a tile of 44, and a tile of one chain)")
    gaps = renumber(fr(0, 100, (0, 100), 90, (250, 350)), 3) + renumber(random_pair(rng, 0, 3, 4, span=600), 10)
    gaps += [ch(40, 100, 0, 100)] + renumber(fr(0, 100, (0, 100), 90, (250, 350), flip=True), 2000000000)
    gaps += renumber(fr(0, 80, (5, 105), 70, (400, 500)), 2147483647)
    t["pair_ids"] = (gaps, 1000, "pair numbers with gaps, the first pair not 0, the largest pair number, and a proper pair as the "
                                 "table's last two chains")
    # ---- 13.1, clause by clause; every pair also behind a decoy, so that both the classifier and k_mt_lanes<16> meet it
    edges = [fr(0, 100, (0, 100), 100, (200, 300)),                       # concordant
             fr(0, 100, (0, 100), 100, (200, 300))[:1] + [ch(1, 100, 200, 300, 1, 1)],  # another target
             [ch(0, 100, 0, 100, 0), ch(1, 100, 200, 300, 0)],           # equal strands, both forward
             [ch(0, 100, 0, 100, 1), ch(1, 100, 200, 300, 1)],           # equal strands, both reverse
             fr(0, 100, (0, 100), 100, (900, 1000)),                      # tl == max_insert
             fr(0, 100, (0, 100), 100, (901, 1001)),                      # tl == max_insert + 1
             fr(0, 100, (50, 150), 100, (50, 160)),                       # f.t_start == r.t_start
             fr(0, 100, (50, 150), 100, (60, 150)),                       # f.t_end == r.t_end
             fr(0, 100, (50, 150), 100, (50, 150)),                       # both equal
             fr(0, 100, (200, 300), 100, (0, 100)),                       # outward-facing: f.t_start > r.t_start
             fr(0, 100, (0, 400), 100, (100, 300)),                       # containment: f.t_end > r.t_end
             fr(0, 100, (0, 100), 100, (200, 300), flip=True),            # mate 1 on strand 1, mate 2 on strand 0
             fr(0, 100, (200, 300), 100, (0, 100), flip=True)]            # the same, outward-facing
    chains = []
    for p, pair in enumerate(edges):
        chains += renumber(pair, 2 * p) + renumber(with_decoy(pair), 2 * p + 1)
    t["edges"] = (chains, 1000, "13.1 clause by clause: each pair once for the classifier and once, behind a decoy chain, for k_mt_lanes<16>")
    tiny = [fr(0, 100, (7, 7), 100, (7, 8)), fr(0, 100, (7, 7), 100, (7, 9)), fr(0, 100, (7, 7), 100, (7, 7))]
    chains = []
    for p, pair in enumerate(tiny):
        chains += renumber(pair, 2 * p) + renumber(with_decoy(pair), 2 * p + 1)
    t["max_insert_1"] = (chains, 1, "max_insert = 1: templates of 1, 2 and 0 bases")
    big = 1 << 31
    wide = [fr(0, 100, (1, 101), 100, (big - 100, big)),                # tl = 2^31 - 1
            fr(0, 100, (0, 100), 100, (big - 100, big)),                # tl = 2^31
            fr(0, 100, (big - 5, big - 1), 100, (big, 2 * big - 1)),    # t_end = 2^32 - 1, tl = 2^31 + 4
            fr(0, 100, (big + 5, big + 9), 100, (big + 7, 2 * big - 1))]  # tl = 2^31 - 6 beyond 2^31
    chains = []
    for p, pair in enumerate(wide):
        chains += renumber(pair, 2 * p) + renumber(with_decoy(pair), 2 * p + 1)
    t["max_insert_max"] = (chains, big - 1, "max_insert = 2^31 - 1 with t_end around 2^31 and 2^32: the difference needs all 32 bits")
    # ---- 13.2
    t["sum_then_tl"] = ([ch(0, 100, 0, 100), ch(0, 100, 50, 150), ch(0, 90, 60, 160), ch(1, 100, 300, 400, 1), ch(1, 100, 280, 380, 1),
                         ch(1, 500, 0, 100, 1, 3)], 1000,
                        "four combinations of the greatest sum: the smallest tl wins, whatever the indices; a better chain elsewhere is no help")
    t["tl_then_a_then_b"] = ([ch(0, 100, 50, 150), ch(0, 100, 50, 140), ch(0, 100, 50, 150), ch(1, 100, 300, 400, 1), ch(1, 100, 290, 400, 1),
                              ch(1, 100, 300, 400, 1),
                              ch(2, 100, 60, 150), ch(2, 100, 50, 150), ch(3, 100, 310, 400, 1), ch(3, 100, 300, 400, 1), ch(3, 100, 310, 400, 1)],
                             1000, "equal sums and equal tl: the smaller a, then the smaller b; in the second pair two mate-1 chains "
                                   "differ in tl, which decides in front of the indices")
    t["negative"] = ([ch(0, -5, 0, 100), ch(0, -7, 0, 100), ch(1, -3, 200, 300, 1), ch(1, 2, 200, 300, 1, 1),
                      ch(2, -1, 0, 100), ch(2, 0, 0, 100), ch(3, -1, 200, 300, 1), ch(3, 0, 200, 300, 1)], 1000,
                     "negative scores and zero: -8 beats -10; 0 + 0 beats the rest")
    hi, lo = 2147483647, -2147483648
    t["extremes"] = ([ch(0, hi, 0, 100), ch(0, hi - 1, 0, 90), ch(1, hi, 200, 300, 1), ch(1, hi - 1, 200, 290, 1),
                      ch(2, lo, 0, 100), ch(2, lo, 0, 90), ch(3, lo, 200, 300, 1), ch(3, lo + 1, 200, 300, 1),
                      ch(4, hi, 0, 100), ch(4, lo, 0, 100), ch(5, lo, 200, 300, 1), ch(5, hi, 200, 310, 1)], 1000,
                     "both scores 2^31 - 1 and both -2^31: the sum needs 33 bits; 2^31 - 1 with -2^31 twice beside the greatest sum")
    nb = []
    for p, n2 in enumerate((1, 2, 64, 65)):
        nb += [ch(2 * p, 100, 0, 100)] + [ch(2 * p + 1, 100, 200, 300, 1)] * n2 + [ch(2 * p + 1, 99, 200, 300, 1)]
    t["n_best"] = (nb, 1000, "n_best of 1, 2, 64 and 65, a combination of a smaller sum beside each")
    t["n_best_across_tl"] = ([ch(0, 100, 0, 100), ch(0, 100, 20, 100), ch(1, 100, 200, 300, 1), ch(1, 100, 200, 350, 1), ch(1, 99, 110, 120, 1)],
                             1000, "four combinations of the greatest sum with four different tl count alike; a closer one of a smaller sum does not")
    t["n_best_90000"] = ([ch(0, 100, 0, 100)] * 300 + [ch(1, 100, 200, 300, 1)] * 300, 1000,
                         "a pair of (300, 300) identical chains: n_best = 90,000 through the 64-bit counter and the clamp's comparison")
    t["empty"] = ([], 1000, "the empty table")
    rng = random.Random(257)
    full = []
    for p, (n1, n2) in enumerate(((1, 0), (1, 1), (30, 34), (100, 89))):
        full += random_pair(rng, p, n1, n2)
    t["chains_256"] = (full, 1000, "256 chains: k_stage_seg_starts' thread n, which writes the closing entry, is alone in a second workgroup")
    t["chains_257"] = (full + [ch(9, 100, 0, 100)], 1000, "the same and a single chain more, of mate 2")
    return t


NAMES = tuple(tables())


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (rows, counts) of the restatement"""
    chains, max_insert, _ = tables()[name]
    return mo.mates(list(chains), max_insert)


def bad_tables():
    """name -> (chains, the smallest bad chain, the word of the message)"""
    good = list(tables()["classes"][0])
    down = list(good)
    down[70] = ch(1, 100, 0, 10)  # (behind a later pair)
    down[200] = ch(0, 100, 0, 10)
    strand = list(good)
    strand[131] = strand[131][:2] + (2,) + strand[131][3:]
    strand[300] = strand[300][:2] + (4000000000,) + strand[300][3:]
    rng_ = list(good)
    rng_[90] = rng_[90][:8] + (500, 499) + rng_[90][10:]
    two = list(good)
    two[150] = two[150][:8] + (9, 1) + two[150][10:]
    two[40] = two[40][:2] + (2,) + two[40][3:]
    both = list(good)  # one chain that breaks strand and range: strand is the first of the two
    both[60] = both[60][:2] + (3,) + both[60][3:8] + (9, 1) + both[60][10:]
    first = [ch(0, 100, 0, 100)[:8] + (10, 9) + ch(0, 100, 0, 100)[10:]] + good
    return {"query_decreases": (down, 70, "order"), "strand_2": (strand, 131, "strand"), "t_start_beyond_t_end": (rng_, 90, "range"),
            "two_bad_chains": (two, 40, "strand"), "two_words_one_chain": (both, 60, "strand"), "first_chain": (first, 0, "range")}
