"""Edge inputs of the unitig coverage filter (msgpu_filter.hip), built against the way its kernels are written and shared by
tests/test_scrub_uf_edges_host.py and tests/test_gpu_scrub_uf_edges.py: ``cases()`` maps a name to Case(paf, fasta, note,
lit), ``expected(name)`` is the per-base restatement's result (uf_oracle.run, once per process).  ``note`` names the kernel
line the case aims at, ``lit`` holds the hand-derived figures.  Every input is built deterministically; the only random
draws are the bases (numpy.random.default_rng(seed)).

Pass 1.  A block's value v shows only in the report, so every pass-1 case has two ids: the filler f0 of value 1 and the
block under test.  Then Q3 = 1 + 0.75 (v - 1) for v >= 1 and 0.75 for v = 0, and nothing is an outlier.  A geometry is a few
counting lines; the width classes (k_uf_wave <= 64 lines, k_uf_group <= 1024, the sort-and-sweep route above) get the same
geometry padded to 64, 65, 1024 and 1025 lines with lines that must not count: repeats of a read id the block has seen, over
an interval that would raise the maximum, and empty intervals of fresh read ids.  ``pass1(name, unique=True)`` is the same
block with the repeats renamed to fresh read ids: its value must differ, or the padding proves nothing.

    touching            [0,10) [10,20) [20,30) of three reads: v = 1 (s < ej, ends before starts at one position)
    stairs5             five nested lines: v = 5
    first_line_empty    c's first line [30,30), its second [5,15) over a's [0,20): v = 1
    inverted            a line with qs > qe across the peak of two: v = 2
    one_read            five lines of one read over one interval: v = 1
    all_empty           empty and inverted lines only: v = 0 (neutral events only on the sweep route)
    from_zero_to_qlen   three lines [0, qlen): v = 3 (real starts at 0 among the neutral pairs)
    far_repeat          the repeated read id on the first and on the last line of the block
    last_block_wins     the id's first block has v = 5, f0 lies between, its last block v = 1: the id's value is 1
    staircase-K[-rev]   K reads, line i = [i, 2K - i), unpadded, in file order and reversed: v = K.  K = 64 (the maximum on
                        lane 63 / lane 0), 1024 (LDS line 1023 / 0), 1100 and 4000 (many 64-event rounds while the depth
                        rises), 1089 (the peak start is a round's first event), 1088 (a round's last)

Pass 2 and the outlier decision: eight ids of 2,2,2,3,3,3,4,7 lines over one interval and an outlier of >= 8 give Q1 = 2,
Q3 = 4, upper = 7.0 whatever the outlier's value, so the id of value 7 stays and the threshold of the runs is 4.

    equal_to_upper  run_499_500  run_at_both_ends  ends_at_qlen  short_outlier  pile_of_endpoints
    repeats_count_in_pass_2  two_outliers_and_one_between  record_shorter_than_qlen  fractional_q3
"""
import collections
import functools

import numpy as np

import uf_oracle

Case = collections.namedtuple("Case", "paf fasta note lit")

WAVE, GROUP = 64, 1024  # UF_WAVE, UF_GROUP of msgpu_filter.hip
PAD = collections.OrderedDict((("wave", 64), ("group65", 65), ("group1024", 1024), ("giant", 1025)))
STAIRS = (64, 1024, 1100, 4000)
STAIRS_ONE_WAY = (1089, 1088)  # 64 * 17 + 1 (= 32 * 34 + 1) and 64 * 17


def bases(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def line(u, qlen, s, e, r):
    w = max(e - s, 0)
    return b"%s\t%d\t%d\t%d\t+\t%s\t5000\t0\t%d\t%d\t%d\t60\n" % (u, qlen, s, e, r, w, w, w)


def block(u, qlen, lines):
    return b"".join(line(u, qlen, s, e, r) for s, e, r in lines)


def record(u, n, seed, desc=b"edge case"):
    return b">%s %s\n%s\n" % (u, desc, bases(n, seed))


FILLER = (line(b"f0", 300, 0, 100, b"a"), b">f0 filler\n" + bases(300, 11) + b"\n")  # test_gpu_unitig_filter._fillers(1, 11)


def q3_of(v):
    return 1 + 0.75 * (v - 1) if v >= 1 else 0.75


def classes(paf):
    """the width-class counters the stage must report for this PAF"""
    names = uf_oracle.parse_paf(paf)[0]
    b0, b1 = uf_oracle._blocks(names)
    n = b1 - b0
    return {"wave_blocks": int((n <= WAVE).sum()), "group_blocks": int(((n > WAVE) & (n <= GROUP)).sum()),
            "giant_blocks": int((n > GROUP).sum())}


# ---- pass 1 -------------------------------------------------------------------------------------------------------------

# name -> (qlen, lines, v, the read id the padding repeats, the interval it repeats it over, lines after the padding, note)
GEOMETRY = collections.OrderedDict((
    ("touching", (100, [(0, 10, b"a"), (10, 20, b"b"), (20, 30, b"c")], 1, b"a", (0, 100), [],
                  "s < ej in k_uf_wave / k_uf_group; ends before starts in uf_put_events")),
    ("stairs5", (100, [(i, 10 - i, b"s%d" % i) for i in range(5)], 5, b"s0", (0, 100), [],
                 "the all-pairs depth and the sweep agree on a nested pile")),
    ("first_line_empty", (100, [(0, 20, b"a"), (30, 30, b"c"), (5, 15, b"c")], 1, b"a", (0, 100), [],
                          "the first line of a read id counts even when it is empty: kept = have && s < e BEFORE the "
                          "de-duplication; lr[j] == lr[i] alone; first && s < e")),
    ("inverted", (100, [(0, 20, b"a"), (10, 20, b"d"), (12, 3, b"b")], 2, b"a", (0, 100), [],
                  "s < e is false for qs > qe: no events, no depth")),
    ("one_read", (100, [(0, 20, b"a")] * 5, 1, b"a", (0, 100), [], "later lines of a read id add nothing")),
    ("all_empty", (100, [(30, 30, b"a"), (40, 10, b"b"), (0, 0, b"c")], 0, b"a", (0, 100), [],
                   "m = kept ? depth : 0 with no kept line; neutral pairs only in k_uf_sweep_max")),
    ("from_zero_to_qlen", (100, [(0, 100, b"a"), (0, 100, b"b"), (0, 100, b"c")], 3, b"a", (0, 100), [],
                           "real starts at position 0 carry the key of the neutral starts")),
    ("far_repeat", (100, [(0, 20, b"a"), (10, 30, b"b")], 2, b"b", (0, 100), [(0, 100, b"a")],
                    "j < lane over all 64 lanes; the LDS loop to i - 1; the (read, line) sort over the whole segment")),
))


def _padding(n, seen, cover, unique):
    out = []
    for i in range(n):
        if i % 2 == 0:
            out.append((cover[0], cover[1], b"pad%d" % i if unique else seen))
        else:
            out.append((7 + i % 11, 7 + i % 11, b"e%d" % i))
    return out


def padded(geom, cls, unique=False):
    """the lines of a geometry's block in a width class"""
    qlen, lines, v, seen, cover, tail, _ = GEOMETRY[geom]
    tail = [(s, e, b"tail" if unique else r) for s, e, r in tail]
    return lines + _padding(PAD[cls] - len(lines) - len(tail), seen, cover, unique) + tail


def stairs(k, rev=False):
    lines = [(i, 2 * k - i, b"s%d" % i) for i in range(k)]
    return lines[::-1] if rev else lines


def pass1(name, unique=False):
    """-> (paf, fasta, v, note) of a pass-1 case"""
    parts = name.split("-")
    if parts[0] == "staircase":
        k, rev = int(parts[1]), parts[-1] == "rev"
        qlen, v = 2 * k, k
        blk = block(b"T", qlen, stairs(k, rev))
        note = "the maximum on the %s line of %d; k_uf_sweep_max's carry over %d rounds" % (
            "first" if rev else "last", k, (2 * k + 63) // 64)
        return FILLER[0] + blk, FILLER[1] + record(b"T", qlen, k), v, note
    geom, cls = parts
    if geom == "last_block_wins":
        first = block(b"T", 100, stairs(5))
        last = [(0, 20, b"a")] + _padding(PAD[cls] - 1, b"a", (0, 100), unique)
        return (first + FILLER[0] + block(b"T", 100, last), FILLER[1] + record(b"T", 100, 5), 1,
                "k_uf_id_values reads val[last_block[u]]")
    qlen, _, v, _, _, _, note = GEOMETRY[geom]
    return FILLER[0] + block(b"T", qlen, padded(geom, cls, unique)), FILLER[1] + record(b"T", qlen, len(geom)), v, note


def pass1_names():
    out = ["%s-%s" % (g, c) for g in list(GEOMETRY) + ["last_block_wins"] for c in PAD]
    out += ["staircase-%d%s" % (k, r) for k in STAIRS for r in ("", "-rev")]
    return out + ["staircase-%d" % k for k in STAIRS_ONE_WAY]


def pass1_value(paf):
    """v of the block T from the restatement's Q3 (two ids, the other of value 1)"""
    q3 = uf_oracle.run(paf, FILLER[1] + b">T\nA\n")[1]["q3"]
    return 0 if q3 == 0.75 else round((q3 - 1) / 0.75) + 1


def peak_event(lines):
    """the place, among the sorted endpoint keys of the counting lines, of the start that first reaches the maximum"""
    seen, ev = set(), []
    for s, e, r in lines:
        if r not in seen and s < e:
            ev += [(s << 1) | 1, e << 1]
        else:
            ev += [1, 0]
        seen.add(r)
    ev.sort()
    depth = np.cumsum([1 if k & 1 else -1 for k in ev])
    return int(np.argmax(depth))


# ---- pass 2 -------------------------------------------------------------------------------------------------------------

def pile(name, v):
    """an id of value v: v reads over [0, 100) of 300 positions"""
    return block(name, 300, [(0, 100, b"r%d" % i) for i in range(v)]), record(name, 300, 100 + v)


def tower(s, e, n, tag):
    return [(s, e, b"%s%d" % (tag, i)) for i in range(n)]


OTHERS = (2, 2, 2, 3, 3, 3, 4, 7)
UPPER_OUTLIER = [(1000, 1500 + k, b"o%d" % k) for k in range(8)]  # 8 deep on [1000, 1500), 4 deep at 1503


def _pass2(outliers, others=OTHERS, between=None):
    """the other ids (n0, n1, ...) in order, then the outlier blocks (name, qlen, lines, record length); `between`: the index
    of the other id that is written between the first two outlier blocks instead"""
    paf, fa = [], []
    ids = [pile(b"n%d" % i, v) for i, v in enumerate(others)]
    for i, (p, f) in enumerate(ids):
        if i != between:
            paf.append(p)
            fa.append(f)
    for k, (name, qlen, lines, n_bases) in enumerate(outliers):
        paf.append(block(name, qlen, lines))
        fa.append(record(name, n_bases, 7 * qlen + k) if n_bases else b">%s no bases\n" % name)
        if k == 0 and between is not None:
            paf.append(ids[between][0])
            fa.append(ids[between][1])
    return b"".join(paf), b"".join(fa)


def _lit(frags, q1=2.0, q3=4.0, upper=7.0, rescued=None, lengths=None, blocks=None):
    return dict(q1=q1, q3=q3, upper=upper, outliers=len(frags), frags=frags,
                rescued=sum(1 for f in frags.values() if f) if rescued is None else rescued, lengths=lengths or {},
                blocks=blocks)


def _pass2_cases():
    c = collections.OrderedDict()

    def add(name, files, note, lit):
        c[name] = Case(files[0], files[1], note, lit)

    add("equal_to_upper", _pass2([(b"O", 3000, UPPER_OUTLIER, 3000)]),
        "idval > S.upper with idval == upper (the id n7 of value 7 is written whole); depth <= t at depth == t",
        _lit({b"O": [(0, 1000, 0, 999), (1, 1497, 1503, 2999)]}))
    add("run_499_500", _pass2([(b"O", 4000, tower(0, 1000, 8, b"x") + tower(1499, 2000, 8, b"y") + tower(2500, 4000, 8, b"z"),
                                4000)]),
        "a - run >= UF_RUN at 499 and at 500", _lit({b"O": [(0, 500, 2000, 2499)]}))
    add("run_at_both_ends", _pass2([(b"O", 3000, tower(500, 2500, 8, b"x"), 3000)]),
        "a run from position 0; the closing run qlen - run >= UF_RUN at exactly 500",
        _lit({b"O": [(0, 500, 0, 499), (1, 500, 2500, 2999)]}))
    add("ends_at_qlen", _pass2([(b"O", 3000, tower(1000, 3000, 8, b"x"), 3000)]),
        "qlen > cur is false: no closing segment, no fragment at the end", _lit({b"O": [(0, 1000, 0, 999)]}))
    add("short_outlier", _pass2([(b"O", 499, tower(0, 100, 8, b"x"), 499)]),
        "qlen < UF_RUN: count 0, the id leaves the output and is not rescued", _lit({b"O": []}))
    add("pile_of_endpoints", _pass2([(b"O", 3000, tower(1000, 2000, 1000, b"x"), 3000)]),
        "the inner loop of k_uf_runs over 1000 events at one position, twice",
        _lit({b"O": [(0, 1000, 0, 999), (1, 1000, 2000, 2999)]}))
    add("repeats_count_in_pass_2", _pass2([(b"O", 3000, tower(0, 500, 8, b"x") + [(1000, 2000, b"rep")] * 10, 3000)]),
        "k_uf_all_events takes every line (s < e alone): 10 deep where pass 1 saw 1",
        _lit({b"O": [(0, 500, 500, 999), (1, 1000, 2000, 2999)]}))
    add("two_outliers_and_one_between",
        _pass2([(b"O", 3000, UPPER_OUTLIER, 3000), (b"P", 3000, tower(500, 2500, 8, b"x"), 3000)],
               others=(2, 2, 2, 3, 3, 4, 4), between=6),
        "frag_off[g] of the second outlier block; the host's o / outl[o] == b walk with a normal block between",
        _lit({b"O": [(0, 1000, 0, 999), (1, 1497, 1503, 2999)], b"P": [(0, 500, 0, 499), (1, 500, 2500, 2999)]}))
    add("record_shorter_than_qlen", _pass2([(b"O", 3000, tower(1000, 1500, 8, b"x"), 600)]),
        "the output plan's min(stop, L) and min(start, e): a fragment cut by the record's end and one beyond it",
        _lit({b"O": [(0, 1000, 0, 999), (1, 1500, 1500, 2999)]}, lengths={b"O_0": 600, b"O_1": 0}))
    # ten ids 2,2,2,3,3,3,4,5,5,9: Q1 = 2 + 0.25 = 2.25, Q3 = 5 - 0.25 = 4.75, upper = 4.75 + 1.5 * 2.5 = 8.5; floor(Q3) = 4
    add("fractional_q3",
        _pass2([(b"O", 4000, tower(0, 100, 9, b"x") + tower(600, 700, 4, b"y") + tower(1500, 1600, 5, b"z"), 4000)],
               others=(2, 2, 2, 3, 3, 3, 4, 5, 5)),
        "t = floor(q3): a stretch 4 deep stays inside a fragment, one 5 deep cuts",
        _lit({b"O": [(0, 1400, 100, 1499), (1, 2400, 1600, 3999)]}, q1=2.25, q3=4.75, upper=8.5))
    return c


# ---- the cases ----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cases():
    c = collections.OrderedDict()
    for name in pass1_names():
        paf, fa, v, note = pass1(name)
        c[name] = Case(paf, fa, note, dict(v=v, q3=q3_of(v), klass=_klass(name)))
    c.update(_pass2_cases())
    return c


def _klass(name):
    """hand-derived: the filler is one wave block; last_block_wins has a first block of five lines too"""
    parts = name.split("-")
    n = int(parts[1]) if parts[0] == "staircase" else PAD[parts[1]]
    k = {"wave_blocks": 1 + (parts[0] == "last_block_wins"), "group_blocks": 0, "giant_blocks": 0}
    k["wave_blocks" if n <= 64 else "group_blocks" if n <= 1024 else "giant_blocks"] += 1
    return k


def names(pass2=None):
    return [n for n, c in cases().items() if pass2 is None or ("frags" in c.lit) == pass2]


@functools.lru_cache(maxsize=None)
def expected(name):
    c = cases()[name]
    return uf_oracle.run(c.paf, c.fasta)


def fragments(text, uid):
    """[(index, length, start, end)] of the fragment headers of ``uid`` in an output text, in file order"""
    out = []
    for h in text.split(b"\n"):
        if h.startswith(b">" + uid + b"_"):
            t = h[len(uid) + 2:].split()
            out.append(tuple(int(x) for x in t))
    return out


def record_lengths(text):
    """header's first word -> bases"""
    out = collections.OrderedDict()
    for rec in text.split(b">")[1:]:
        h, _, body = rec.partition(b"\n")
        out[h.split()[0]] = len(body.replace(b"\n", b""))
    return out
