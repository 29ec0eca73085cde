"""Hand-made chain tables for rule 12 (the mapper's primaries, secondaries and mapping quality), shared by the host and the GPU
file, with what each is made for.  A chain is the tuple of msgpu_map_chain; only query, n_anchors, score, q_start and q_end
matter to the rule, the other fields are filled so that a table could be a mapper's."""
import functools
import random

import map_rank_oracle as ro

LDS = ro.LDS


def ch(q, score, qs, qe, anchors=12, target=0, strand=0):
    return (q, target, strand, anchors, score, 0, qs, qe, qs, qe, qe - qs, qe - qs)


def random_segment(rng, q, n, span=6000):
    """n chains of one query with overlapping ranges, score ties and 3..15 anchors"""
    out = []
    for _ in range(n):
        a = rng.randrange(0, span - 900)
        out.append(ch(q, rng.choice((60, 100, 100, 150, 200, 200, 333, 500)) + rng.randrange(3), a, a + rng.randrange(50, 900),
                      anchors=rng.randrange(3, 16), target=rng.randrange(4), strand=rng.randrange(2)))
    return out


def disjoint(q, n, score=lambda i: 100 + i % 7):
    """n chains whose ranges do not meet: every one is primary"""
    return [ch(q, score(i), 10 * i, 10 * i + 9) for i in range(n)]


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (chains, what the table is made for)"""
    rng = random.Random(12)
    t = {}
    sizes = []
    for q, n in enumerate((1, 2, 63, 64, 65, 128, 129)):
        sizes += random_segment(rng, q, n)
    t["sizes"] = (sizes, "segments of 1, 2, 63, 64, 65, 128 and 129 chains: every class and both sides of the wavefront's 64")
    for n in (1, 2, 63, 64, 65, 128, 129):
        t["alone_%d" % n] = (random_segment(rng, 3, n), "one segment of %d chains: the first and the last of its table" % n)
    t["lds_exact"] = (disjoint(0, LDS), "exactly MSGPU_MAP_RANK_LDS primaries: the list stays in LDS")
    # one primary more, and secondaries of the first, of the last LDS entry and of the entry in the arena, visited last
    more = disjoint(0, LDS + 1, score=lambda i: 1000 - i)  # (visited in table order: entry e is chain e)
    more += [ch(0, 50, 0, 9), ch(0, 49, 10 * (LDS - 1), 10 * (LDS - 1) + 9), ch(0, 48, 10 * LDS, 10 * LDS + 9), ch(0, 47, 10 * LDS + 2, 10 * LDS + 8)]
    t["lds_plus_one"] = (more, "MSGPU_MAP_RANK_LDS + 1 primaries: one entry in the arena, read back by two secondaries")
    t["lds_far"] = (disjoint(0, LDS + 70, score=lambda i: 1000 + i % 7) + random_segment(rng, 0, 80, span=10 * (LDS + 70)) +
                    random_segment(rng, 1, 70),
                    "more than a ballot of entries in the arena, overlapping chains behind them, and a list segment that stays in LDS")
    t["half"] = ([ch(0, 200, 0, 100), ch(0, 100, 50, 150), ch(1, 200, 0, 100), ch(1, 100, 49, 149), ch(2, 200, 0, 100), ch(2, 100, 50, 120),
                  ch(3, 200, 0, 100), ch(3, 100, 65, 135), ch(4, 200, 0, 100), ch(4, 100, 64, 134)],
                 "2 * ov == min(len) stays primary, one base more is secondary; the shorter of the two lengths decides")
    t["nested"] = ([ch(0, 300, 0, 1000), ch(0, 200, 100, 200), ch(0, 100, 120, 130), ch(0, 250, 900, 2000), ch(0, 50, 0, 2000),
                    ch(1, 100, 100, 200), ch(1, 300, 0, 1000), ch(1, 50, 0, 0), ch(1, 40, 5, 5)],
                   "ranges inside one another, an outer chain visited last, and empty ranges (never masked: 0 > 0 is false)")
    t["ties"] = ([ch(0, 100, 0, 100), ch(0, 100, 10, 110), ch(0, 100, 200, 300), ch(0, 100, 190, 290), ch(0, 100, 20, 120)],
                 "equal scores: the smaller index is visited first and becomes the primary")
    t["first_overlap"] = ([ch(0, 100, 0, 100), ch(0, 90, 40, 140), ch(0, 300, 60, 160), ch(0, 80, 45, 125),
                           ch(1, 80, 45, 125), ch(1, 300, 60, 160), ch(1, 100, 0, 38)],
                          "a secondary that meets two primaries: the parent is the first in visiting order (the best score), not the "
                          "first in table order")
    t["ratio"] = ([ch(0, 100, 0, 100), ch(0, 90, 0, 100), ch(0, 89, 0, 100), ch(0, 100, 0, 100), ch(1, 7, 0, 50), ch(1, 6, 0, 50),
                   ch(1, 7, 0, 50)], "10 * s == 9 * s1 exactly counts, one less does not; 10 * 6 < 9 * 7")
    t["low_scores"] = ([ch(0, 0, 0, 100), ch(0, -5, 0, 100), ch(1, -3, 0, 100), ch(1, -3, 50, 150), ch(1, -2147483648, 0, 100),
                        ch(2, 2147483647, 0, 100), ch(2, -2147483648, 0, 100), ch(3, 5, 0, 10), ch(3, -7, 0, 10)],
                       "scores 0 and negative give mapq 0; the extremes of 32 bits; a negative sub")
    t["anchors"] = ([ch(0, 100, 0, 100, anchors=9), ch(0, 50, 0, 100), ch(1, 100, 0, 100, anchors=10), ch(1, 50, 0, 100),
                     ch(2, 100, 0, 100, anchors=11), ch(2, 50, 0, 100), ch(3, 100, 0, 100, anchors=1), ch(4, 100, 0, 100, anchors=9),
                     ch(5, 101, 0, 7, anchors=3), ch(5, 1, 0, 7)], "n_anchors 9, 10 and 11 around the formula's min(n_anchors, 10)")
    singles = []
    for q in range(64):
        singles += random_segment(rng, q, 1)
    t["singles_then_list"] = (singles + random_segment(rng, 64, 65), "64 one-chain segments followed by one of 65")
    t["wide"] = ([ch(0, 10, 0, 4294967295), ch(0, 9, 2147483648, 4294967295), ch(0, 8, 0, 2147483647), ch(0, 7, 0, 2147483648)],
                 "ranges up to 2^32 - 1: 2 * ov needs 33 bits")
    t["sparse_queries"] = ([ch(5, 100, 0, 10), ch(5, 90, 0, 10), ch(4000000000, 100, 0, 10), ch(4294967295, 100, 0, 10),
                            ch(4294967295, 100, 5, 15)], "query records that are not consecutive numbers")
    t["empty"] = ([], "the empty table")
    # (a generator of their own: the tables above stay what they were)
    rng = random.Random(256)
    full = []
    for q, n in enumerate((1, 2, 64, 189)):
        full += random_segment(rng, q, n)
    t["chains_256"] = (full, "256 chains in segments of 1, 2, 64 and 189: k_stage_seg_starts' thread n, which writes the closing "
                             "entry of the segment starts, is alone in a second workgroup")
    t["chains_257"] = (full + random_segment(rng, 4, 1), "the same and one more segment of 1 chain: the last chain and the closing "
                                                         "entry come from the second workgroup")
    return t


NAMES = tuple(tables())


@functools.lru_cache(maxsize=None)
def expected(name):
    """-> (rows, stats) of the restatement"""
    chains = tables()[name][0]
    rows = ro.rank(chains)
    return rows, ro.stats(chains, rows)


def bad_tables():
    """name -> (chains, the first bad chain, a word of the message)"""
    good = tables()["sizes"][0]
    down = list(good)
    down[70] = ch(1, 100, 0, 10)  # (behind query 3)
    down[200] = ch(0, 100, 0, 10)
    rev = list(good)
    rev[131] = rev[131][:6] + (500, 499) + rev[131][8:]
    rev[300] = rev[300][:6] + (9, 1) + rev[300][8:]
    first = [ch(0, 100, 0, 1)[:6] + (10, 9) + ch(0, 100, 0, 1)[8:]] + list(good)
    return {"query_decreases": (down, 70, "query"), "q_start_beyond_q_end": (rev, 131, "q_start"),
            "first_chain": (first, 0, "q_start")}
