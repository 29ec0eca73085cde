"""Edge inputs of the k-mer abundance filter (msgpu_kmer.hip) and of the short-read unitig assembly (msgpu_unitig.hip), built
against the way their kernels are written, shared by tests/test_kmer_edges_host.py and tests/test_gpu_kmer_edges.py:
``cases()`` maps a name to (stage, k, files, params), ``expected(name)`` is the plain-Python restatement's result
(kf_oracle.run / ug_oracle.run, once per process), ``meets_conditions(name, result)`` the list of the conditions the case was
built for and misses, ``family_conditions()`` the same for the conditions that hold over a family of cases.  Every input is a
function of fixed seeds.

Unitig graph (min_count = 1, min_length = 0):

    ladder-K-T    a trunk with one dead-end branch of j k-mers per j in {1, 2, 3}, the tip limits, every limit + 1 and
                  trim - 1: tips of exactly limit, limit + 1, trim and trim + 1 k-mers.  The rounds equal the plan.
    snapshot-K    two dead ends of 3 k-mers that meet with nothing upstream: one round removes both (the snapshot rule).
    cascade-K     a branch of 6 onto the 7th k-mer of a branch of 12: the rounds end (6, 12), (6, 6), (6, 0).
    three_in-K    three branches of 3 onto one trunk k-mer (in-degree 4): one round removes 9.
    rings-K       12 cycles of 2 ... 1000 k-mers beside a linear chain of 5000, some written from the mirror strand.
    hairpin-K, selfcomp-K   synth.unitig_cases' constructions at other k (128-bit keys among them).
    dense-K-D-T   random reads over D percent of the canonical k-mers at k = 2 ... 6: over the family every in-degree and
                  out-degree 0 ... 4 occurs at every k >= 3, all 5 x 5 x 2 = 50 combinations of (in-degree, out-degree,
                  strand) -- there are no more than these 50 to ask for -- and all 256 values of the neighbour byte
                  (in-set, out-set) that k_ug_adj builds.

Count and records (both stages where the stage allows it):

    tile-F        FASTQ files whose '\\n' fall on chosen bytes around the 16-byte and 4096-byte tiles of k_kf_lines, of
                  sizes 4095, 4096, 4097, 8192 and 4112, with and without the final newline; one line of 10,000 bases;
                  tile-bad-*: a format error on the line that starts at byte 4096.
    wave-N, wave-short, wave-long   record counts around the wavefront and the workgroup; a block of 128 reads shorter than
                  k; one read of 5000 bases among 63 of exactly k.
    hist_rows     counts 1023 ... 1025 and 10000 ... 10002 (k_kf_hist's LDS rows and the clamp at 10001).
    upper5, upper5-32, upper5-33    upper == 5 with keys of count 4 and 5; 32 and 33 abundant keys (the table's load).
    on_threshold  a key of count upper and one of count upper - 1.
    high-K        keys whose top bits are all set.
    parts-*       a budget under which the count cuts fewer than 2000 windows into 1024 partitions or more.
"""
import functools

import numpy as np

import kf_oracle
import ug_oracle

MASK64 = (1 << 64) - 1
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(s):
    return s[::-1].translate(_COMP)


@functools.lru_cache(maxsize=None)
def rnd(n, seed):
    """n uniform bases, a function of the seed"""
    from muchsalsa_amd import synth
    return synth.genome_bases(n, seed).tobytes()


def draws(n, seed, lo, hi):
    """n integers in [lo, hi], a function of the seed"""
    from muchsalsa_amd import synth
    return (lo + (synth.splitmix64(seed, 77, n) % np.uint64(hi - lo + 1)).astype(np.int64)).tolist()


def fq(reads, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, r, b"I" * len(r)) for i, r in enumerate(reads))


def other_base(b, pick=0):
    """a base that is not ``b`` (one byte as an int)"""
    return [c for c in b"ACGT" if c != b][pick]


# ---- unitig graph ------------------------------------------------------------------------------------------------------

LADDER = ((15, 15), (31, 31), (32, 7), (33, 33), (64, 64), (21, 1))
SNAPSHOT_K = (21, 33)
CASCADE_K = (15, 63)
THREE_IN_K = (15, 64)
RINGS_K = (15, 32, 33, 63, 64)
RING_L = (2, 3, 5, 63, 64, 65, 127, 128, 129, 255, 257, 1000)
# chosen so that the conditions hold (a ring of 2 must not be AA, AT, CG, ...)
RING_SEED = {15: 1510, 32: 3200, 33: 3301, 63: 6301, 64: 6402}
HAIRPIN_K = (33, 63, 64)
SELFCOMP_K = (4, 32, 64)
DENSE_K = (2, 3, 4, 5, 6)
DENSE_D = (10, 30, 60, 100)


def branch(target, at, j, k, seed, pick=0):
    """a read whose first j k-mers run into the k-mer of ``target`` at ``at``"""
    return rnd(j - 1, seed) + bytes([other_base(target[at - 1], pick)]) + target[at:at + k - 1 + 4]


def ladder_lengths(trim):
    limits = ug_oracle.tip_limits(trim)
    return sorted(j for j in {1, 2, 3} | set(limits) | {l + 1 for l in limits} | {trim - 1} if j >= 1)


def ladder_plan(trim):
    """the rounds a ladder must give: the round at limit l removes the branches of (previous limit, l] k-mers"""
    js, plan, prev = ladder_lengths(trim), [], 0
    for l in ug_oracle.tip_limits(trim):
        plan.append((l, sum(j for j in js if prev < j <= l)))
        prev = l
    return plan + ([(trim, 0)] if plan[-1][1] else [])


def ladder_reads(k, trim):
    js = ladder_lengths(trim)
    step = trim + k + 40
    trunk = rnd(step * (len(js) + 1) + k, 1000 * k + trim)
    reads = [trunk]
    for i, j in enumerate(js):
        b = branch(trunk, step * (i + 1), j, k, 1000 * k + 10 * trim + 100 + i)
        reads.append(revcomp(b) if i & 1 else b)
    return reads


def snapshot_reads(k):
    down = rnd(k + 80, 50 * k)
    a, b = rnd(3, 50 * k + 1), rnd(2, 50 * k + 2)
    return [a + down, b + bytes([other_base(a[-1])]) + down[:k + 5]], down


def cascade_reads(k):
    trunk = rnd(4 * k + 200, 60 * k)
    b1 = branch(trunk, 2 * k + 100, 12, k, 60 * k + 1)
    b2 = branch(b1, 6, 6, k, 60 * k + 2)
    return [trunk, b1, revcomp(b2)]


def three_in_reads(k):
    trunk = rnd(4 * k + 200, 70 * k)
    return [trunk] + [branch(trunk, 2 * k + 100, 3, k, 70 * k + 1 + p, p) for p in range(3)]


def ring_circles(k):
    """the 12 circular sequences as they are written (every third one from the mirror strand)"""
    out = []
    for i, n in enumerate(RING_L):
        c = rnd(n, RING_SEED[k] + i)
        out.append(revcomp(c) if i % 3 == 1 else c)
    return out


def ring_reads(k):
    reads = [(c * (2 + (k + len(c)) // len(c)))[:2 * len(c) + k - 1] for c in ring_circles(k)]
    return reads + [rnd(5000 + k - 1, RING_SEED[k] + 50)]


def hairpin_reads(k):
    h = rnd(100, 80 * k)
    return [h + revcomp(h)]


def selfcomp_reads(k):
    """left + x + rc(x) + right; the base behind the self-complementary k-mer is the complement of the one in front of it, so
    that the k-mer has one successor (its predecessor's mirror is that same node) and the join is the self-complement
    rule's to refuse"""
    left, x, right = rnd(112, 90 * k + 1), rnd(k // 2, 90 * k + 2), rnd(111, 90 * k + 3)
    right = revcomp(left[-1:]) + right
    return [left + x + revcomp(x) + right], x + revcomp(x)


def dense_reads(k, percent):
    """reads of k ... k + 3 bases until about ``percent`` of the canonical k-mers are present (100: every one of them)"""
    whole = 4 ** k // 2
    if percent >= 100:
        return [rnd(12 * 4 ** k + 40, 7 * k)]
    want = int(-np.log(1 - percent / 100.0) * whole) + 1
    lens = draws(want, 11 * k + percent, k, k + 3)
    big = rnd(sum(lens), 13 * k + percent)
    reads, at, windows = [], 0, 0
    for n in lens:
        reads.append(big[at:at + n])
        at += n
        windows += n - k + 1
        if windows >= want:
            break
    return reads


# ---- count and records -------------------------------------------------------------------------------------------------

K_TILE = 11
K_WAVE = (21, 33)
POOL = 240  # bases of the little genome the filler reads are cut from


def pool_read(i, n=25, seed=31):
    """read i of n bases from a genome of POOL bases, every third one from the mirror strand; every fifth read starts at
    base 0, so that the k-mers there are abundant"""
    g = rnd(POOL, seed)
    at = 0 if i % 5 == 4 else (i * 37) % (POOL - n)
    return revcomp(g[at:at + n]) if i % 3 == 2 else g[at:at + n]


def tile_file(size, final_newline, marks, long_line=0):
    """A FASTQ file of exactly ``size`` bytes.  ``marks``: [(byte, empty)] -- the '\\n' of a record's first line falls on
    ``byte``, by padding that line; the record's sequence and quality are empty with ``empty``.  ``long_line``: the record at
    the last mark has a sequence of that many bases."""
    out, pos, i = [], 0, 0

    def head(n):
        base = b"@t%d" % i
        assert n >= len(base), (size, marks, n)
        return base + b"x" * (n - len(base))

    def record(h, seq):
        nonlocal pos, i
        rec = head(h) + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n"
        out.append(rec)
        pos += len(rec)
        i += 1

    for n, (m, empty) in enumerate(marks):
        while m - pos >= 5 + 55 + 8:
            record(5, pool_read(i))
        last = n == len(marks) - 1
        record(m - pos, b"" if empty else rnd(long_line, 99) if long_line and last else pool_read(i))
    total = size + (0 if final_newline else 1)
    while total - pos >= 5 + 55 + 12:
        record(5, pool_read(i))
    left = total - pos
    s = min(25, (left - 10) // 2)
    record(left - 2 * s - 5, pool_read(i)[:s])
    data = b"".join(out)
    data = data if final_newline else data[:-1]
    assert len(data) == size
    return data


EMPTY = True
TILE_FILES = {  # name: (size, final newline, marks, long line)
    "4095n": (4095, True, [(15, EMPTY)], 0),
    "4095o": (4095, False, [(16, EMPTY)], 0),
    "4096n": (4096, True, [(17, EMPTY)], 0),  # the last '\n' on byte 4095
    "4096o": (4096, False, [(15, EMPTY)], 0),
    "4097n": (4097, True, [(16, EMPTY)], 0),  # the last '\n' on byte 4096
    "4097o": (4097, False, [(14, EMPTY)], 0),  # '\n' on 14 and 15, and on 17 and 18
    "8192n": (8192, True, [(15, EMPTY), (4095, EMPTY)], 0),  # the last '\n' on byte 8191
    "8192o": (8192, False, [(17, EMPTY), (4097, EMPTY)], 0),
    "4112n": (4112, True, [(16, EMPTY), (4094, EMPTY)], 0),
    "4112o": (4112, False, [(15, EMPTY), (4096, EMPTY)], 0),
    "long": (28688, True, [(16, EMPTY), (4096, False), (8192, False)], 10000),  # the line of 10,000 bases starts at byte 8193
}
NEWLINE_BYTES = (15, 16, 17, 4095, 4096, 4097, 8191, 8192)


def mate_file(data):
    """a plain second file with as many records as ``data``: the same reads from the other strand"""
    recs = kf_oracle.parse_fastq(data)
    return fq([revcomp(r[1]) if set(r[1]) <= set(b"ACGT") else r[1] for r in recs], b"m")


def tile_bad_at():
    """a first line without '@' that starts at byte 4096"""
    return tile_file(4096, True, [(16, EMPTY)]) + b"t99\nACGTACGTACGTA\n+\nIIIIIIIIIIIII\n" + fq([pool_read(3)], b"z")


def tile_bad_quality():
    """a quality line one byte short that starts at byte 4096"""
    seq = pool_read(5)
    pre = b"@q\n" + seq + b"\n+\n"
    return tile_file(4096 - len(pre), True, [(17, EMPTY)]) + pre + b"I" * (len(seq) - 1) + b"\n" + fq([pool_read(4)], b"z")


def wave_reads(n, k, seed):
    """n reads whose lengths run through k - 1, k, k + 1, 40, 0 and 2 k bases"""
    pattern = (k - 1, k, k + 1, 40, 0, k, 2 * k, k + 1)
    return [pool_read(i + seed, 2 * k + 40, 41)[:pattern[i % len(pattern)]] for i in range(n)]


def wave_short_reads(k, seed):
    """64 long reads, 128 reads shorter than k, 64 long reads"""
    short = [pool_read(i + seed, 70, 43)[:i % k] for i in range(128)]
    return [pool_read(i + seed, 70, 43) for i in range(64)] + short + [pool_read(i + seed + 64, 70, 43) for i in range(64)]


def wave_long_reads(k, seed):
    """63 reads of exactly k bases (8 distinct ones) and one of 5000 bases, the 18th"""
    reads = [pool_read((i * i) % 8 + seed, k, 47) for i in range(63)]
    return reads[:17] + [rnd(5000, 48 + seed)] + reads[17:]


def distinct_kmers(n, k, seed):
    """n k-mers (bytes) with n distinct canonical forms"""
    out, seen = [], set()
    big = rnd(4 * n * k + 4 * k, seed)
    for at in range(0, len(big) - k, k):
        x = big[at:at + k]
        c = min(x, revcomp(x))
        if c not in seen:
            seen.add(c)
            out.append(x)
            if len(out) == n:
                return out
    raise AssertionError("not enough distinct k-mers")


def two_files(reads):
    """exact-k reads -> two files of equal record counts with one-line headers"""
    if len(reads) & 1:
        raise AssertionError("an odd number of reads")
    def text(rs):
        return b"".join(b"@\n%s\n+\n%s\n" % (r, b"I" * len(r)) for r in rs)
    return text(reads[:len(reads) // 2]), text(reads[len(reads) // 2:])


HIST_COUNTS = (1023, 1024, 1025, 10000, 10001, 10002)


def hist_rows_files():
    k = 11
    keys = distinct_kmers(len(HIST_COUNTS) + 100, k, 501)
    reads = []
    for i, x in enumerate(keys[len(HIST_COUNTS):]):  # the background: counts 2 ... 6
        reads += [x if j & 1 else revcomp(x) for j in range(2 + i % 5)]
    for x, c in zip(keys, HIST_COUNTS):
        reads += [x if j % 3 else revcomp(x) for j in range(c)]
    order = np.argsort(np.asarray(draws(len(reads), 502, 0, 1 << 40)), kind="stable").tolist()
    reads = [reads[i] for i in order]
    return two_files(reads + ([] if len(reads) % 2 == 0 else [keys[len(HIST_COUNTS)]]))  # (the background key goes 2 -> 3)


def upper5_files(n2, n3, n4, n5, seed):
    """exact-k reads: n2 keys of count 2, n3 of count 3, n4 of count 4, n5 of count 5 and singletons to fill up; every read of
    a count-5 key lies in a pair of its own, mates 1 and 2 alternating"""
    k = 11
    keys = distinct_kmers(n2 + n3 + n4 + n5 + 2, k, seed)
    rest = []
    for i, x in enumerate(keys[:n2 + n3 + n4]):
        rest += [x if j & 1 else revcomp(x) for j in range(2 if i < n2 else 3 if i < n2 + n3 else 4)]
    hot = [x if j & 1 else revcomp(x) for x in keys[n2 + n3 + n4:n2 + n3 + n4 + n5] for j in range(5)]
    if (len(rest) + len(hot)) & 1:
        rest.append(keys[-1])  # a singleton: row 1 is no part of the total
    pairs = (len(rest) + len(hot)) // 2
    assert len(hot) <= pairs
    one, two, at = [], [], 0
    for p in range(pairs):
        if p < len(hot):  # a hot read as mate 1 (even p) or mate 2 (odd p), a cold read as the other mate
            a, b = (hot[p], rest[at]) if p % 2 == 0 else (rest[at], hot[p])
            at += 1
        else:
            a, b = rest[at], rest[at + 1]
            at += 2
        one.append(a)
        two.append(b)
    assert at == len(rest)
    return two_files(one + two)


def on_threshold_files():
    """reads of 30 bases over a genome of 1500, every third one from its first 90 bases"""
    g = rnd(1500, 61)
    at = [(i * 7) % 60 if i % 3 == 0 else (i * 53) % 1470 for i in range(150)]
    reads = [revcomp(g[a:a + 30]) if i & 1 else g[a:a + 30] for i, a in enumerate(at)]
    return fq(reads[:75], b"a"), fq(reads[75:], b"b")


def high_reads(k):
    """T^(k/2) A^(k/2) (self-complementary at even k), poly-A, poly-C, reads T...A of exactly k bases (both strands start
    with T: so does the canonical key) in 2 ... 4 copies, the first in 9, and two ordinary reads"""
    half = (k + 1) // 2
    reads = [b"T" * half + b"A" * (k - half)] * 9 + [b"A" * (k + 9), b"C" * (k + 5), b"T" * (k + 1)]
    for i in range(20):
        x = b"T" + rnd(k - 2, 700 + 20 * k + i) + b"A"
        reads += [x if j & 1 else revcomp(x) for j in range(2 + i % 3 if i else 9)]
    return reads + [rnd(2 * k, 800 + k), rnd(2 * k, 801 + k)]


def parts_reads():
    """ten stretches of 70 bases read at depths 1, 1, 1, 1, 2, 2, 2, 3, 3, 3 and an eleventh at depth 6: fewer than 2000
    windows at k >= 21, most keys once or twice, one read's keys abundant"""
    g = rnd(770, 901)
    reads = []
    for i, depth in enumerate((1, 1, 1, 1, 2, 2, 2, 3, 3, 3, 6)):
        reads += [g[70 * i:70 * i + 70] if j & 1 else revcomp(g[70 * i:70 * i + 70]) for j in range(depth)]
    return [reads[(7 * i) % len(reads)] for i in range(len(reads))]


# ---- the partitions, restated (msgpu_kmer_shared.h: kf_mix, kf_bin, kf_first_bin, kf_pick_partitions) -------------------

BINS = 4096


def kf_bin(key):
    """the hash bin of a canonical key (a Python integer of up to 128 bits)"""
    x = (key & MASK64) ^ (((key >> 64) * 0x9e3779b97f4a7c15) & MASK64)
    x ^= x >> 30
    x = (x * 0xbf58476d1ce4e5b9) & MASK64
    x ^= x >> 27
    x = (x * 0x94d049bb133111eb) & MASK64
    x ^= x >> 31
    return x >> 52


def per_key(k):
    return 2 * (8 if k <= 32 else 16) + 4


def bin_prefix(datas, k):
    """windows per hash bin over all files -> their prefix sums"""
    bins = np.zeros(BINS, np.int64)
    for d in datas:
        for r in kf_oracle.parse_fastq(d):
            for key in kf_oracle.canonical_kmers(r[1], k):
                bins[kf_bin(key)] += 1
    return np.concatenate(([0], np.cumsum(bins)))


def pick_partitions(pre, k, budget):
    """-> (the number of partitions the stage chooses under ``budget`` bytes (0: no cut fits), the largest one's windows)"""
    for q in range(1, BINS + 1):
        first = (np.arange(q + 1, dtype=np.int64) * BINS + q - 1) // q
        m = int(np.diff(pre[first]).max())
        if m * per_key(k) <= budget:
            return q, m
    return 0, 0


@functools.lru_cache(maxsize=None)
def parts_budgets(stage, k):
    """-> (a budget in bytes that gives 1024 partitions or more, that number, a budget below the finest cut)"""
    pre = bin_prefix(_parts_files(), k)
    finest = int(np.diff(pre).max())
    best = None
    for m in range(finest, finest + 64):
        q, _ = pick_partitions(pre, k, m * per_key(k))
        if q < 1024:
            break
        best = (m * per_key(k), q)  # the largest such budget: the fewest partitions that are still 1024 or more
    if best is None:
        raise AssertionError("no budget gives 1024 partitions or more")
    return best[0], best[1], finest * per_key(k) - 1


def _parts_files():
    reads = parts_reads()
    return (fq(reads[::2], b"p"), fq(reads[1::2] + ([b"ACGT"] if len(reads) & 1 else []), b"q"))


# ---- the cases ---------------------------------------------------------------------------------------------------------

UG = dict(min_count=1, min_length=0)
K_PARTS = {"kf": 21, "ug": 40}


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (stage, k, files, params).  ``params`` goes to the restatement and to the stage as it is, but for
    ``budget_bytes`` (the stage's budget; the restatement knows none) and ``error`` (the case is a format error)."""
    c = {}
    for k, trim in LADDER:
        c["ladder-%d-%d" % (k, trim)] = ("ug", k, [fq(ladder_reads(k, trim))], dict(UG, trim=trim))
    for k in SNAPSHOT_K:
        c["snapshot-%d" % k] = ("ug", k, [fq(snapshot_reads(k)[0])], dict(UG))
    for k in CASCADE_K:
        c["cascade-%d" % k] = ("ug", k, [fq(cascade_reads(k))], dict(UG, trim=6))
    for k in THREE_IN_K:
        r = three_in_reads(k)
        c["three_in-%d" % k] = ("ug", k, [fq(r[:2]), fq(r[2:])], dict(UG))
    for k in RINGS_K:
        r = ring_reads(k)
        c["rings-%d" % k] = ("ug", k, [fq(r[:7]), fq(r[7:])], dict(UG, trim=0))
    for k in HAIRPIN_K:
        c["hairpin-%d" % k] = ("ug", k, [fq(hairpin_reads(k))], dict(UG))
    for k in SELFCOMP_K:
        c["selfcomp-%d" % k] = ("ug", k, [fq(selfcomp_reads(k)[0])], dict(UG))
    for k in DENSE_K:
        for d in DENSE_D:
            for trim in (0, k):
                c["dense-%d-%d-%d" % (k, d, trim)] = ("ug", k, [fq(dense_reads(k, d))], dict(UG, trim=trim))
    for name, (size, final, marks, long_line) in TILE_FILES.items():
        a = tile_file(size, final, marks, long_line)
        b = mate_file(a)
        c["tile-%s-kf" % name] = ("kf", K_TILE, [a, b], {})
        c["tile-%s-ug" % name] = ("ug", K_TILE, [b[:-1], a], dict(UG))
    good = tile_file(4096, True, [(15, EMPTY)])
    c["tile-bad-at-kf"] = ("kf", K_TILE, [tile_bad_at(), tile_bad_quality()], {"error": True})  # file 0 is judged first
    c["tile-bad-quality-kf"] = ("kf", K_TILE, [good, tile_bad_quality()], {"error": True})
    c["tile-bad-at-ug"] = ("ug", K_TILE, [good, tile_bad_at()], {"error": True})
    c["tile-bad-quality-ug"] = ("ug", K_TILE, [tile_bad_quality()], {"error": True})
    for n in (63, 64, 65, 255, 256, 257):
        k = K_WAVE[n & 1]
        a, b = fq(wave_reads(n, k, 0), b"a"), fq(wave_reads(n, k, 5), b"b")
        c["wave-%d-kf" % n] = ("kf", k, [a, b], {})
        c["wave-%d-ug" % n] = ("ug", k, [a, b], dict(UG))
    k = K_WAVE[0]
    a64, one = fq(wave_reads(64, k, 0), b"a"), fq([pool_read(9, 40, 41)], b"b")
    c["wave-64+1-ug"] = ("ug", k, [a64, one], dict(UG))
    c["wave-1+64-ug"] = ("ug", k, [one, a64], dict(UG))
    c["wave-0+65-ug"] = ("ug", k, [b"", fq(wave_reads(65, k, 0), b"a")], dict(UG))
    for k in K_WAVE:
        a, b = fq(wave_short_reads(k, 0), b"a"), fq(wave_short_reads(k, 7), b"b")
        c["wave-short-%d-kf" % k] = ("kf", k, [a, b], {})
        c["wave-short-%d-ug" % k] = ("ug", k, [a, b], dict(UG))
        a, b = fq(wave_long_reads(k, 0), b"a"), fq(wave_long_reads(k, 3)[::-1], b"b")
        c["wave-long-%d-kf" % k] = ("kf", k, [a, b], {})
        c["wave-long-%d-ug" % k] = ("ug", k, [a, b], dict(UG))
    c["hist_rows"] = ("kf", 11, list(hist_rows_files()), {})
    c["upper5"] = ("kf", 11, list(upper5_files(50, 50, 3, 3, 601)), {})
    c["upper5-32"] = ("kf", 11, list(upper5_files(80, 80, 3, 32, 602)), {})
    c["upper5-33"] = ("kf", 11, list(upper5_files(80, 80, 3, 33, 603)), {})
    c["on_threshold"] = ("kf", 9, list(on_threshold_files()), {})
    for k in (32, 33, 64):
        r = high_reads(k)
        r += [r[0]] * (len(r) & 1)
        c["high-%d-kf" % k] = ("kf", k, [fq(r[::2], b"a"), fq(r[1::2], b"b")], {})
        c["high-%d-ug" % k] = ("ug", k, [fq(r, b"a")], dict(UG))
    for stage in ("kf", "ug"):
        k = K_PARTS[stage]
        c["parts-%s" % stage] = (stage, k, list(_parts_files()), dict(UG if stage == "ug" else {}, budget_bytes=True))
    return c


def names(stage=None, errors=False):
    return [n for n, v in cases().items() if stage in (None, v[0]) and bool(v[3].get("error")) == errors]


def oracle_params(params):
    return {key: v for key, v in params.items() if key not in ("budget_bytes", "error")}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement's result; for a format error {"error": (file, line)}"""
    stage, k, files, params = cases()[name]
    try:
        if stage == "kf":
            return kf_oracle.run(k, files[0], files[1])
        return ug_oracle.run(k, files, **oracle_params(params))
    except kf_oracle.FastqError as e:
        return {"error": (e.file, e.line)}


# ---- the conditions ----------------------------------------------------------------------------------------------------

def newline_bytes(data):
    at = np.flatnonzero(np.frombuffer(data, np.uint8) == 10)
    return set(at.tolist())


def mirror_cycles(r, rings):
    import ugcases
    return ugcases.mirror_cycles(r, rings)


def degrees(name):
    """[(in-degree, out-degree, strand, neighbour byte)] of every oriented node of a case's solid set"""
    _, k, files, params = cases()[name]
    counts, _ = ug_oracle.count_files(ug_oracle.parse_files(files), k)
    g = ug_oracle.Graph(counts, k)
    out = []
    for s in g.nodes():
        succ, pred = g.succ(s), g.pred(s)
        byte = sum(1 << (t & 3) for t in succ) | sum(16 << (t >> g.top) for t in pred)
        out.append((len(pred), len(succ), int(s != ug_oracle.canon(s, k)), byte if s == ug_oracle.canon(s, k) else -1))
    return out


def largest_key(name):
    stage, k, files, _ = cases()[name]
    recs = [kf_oracle.parse_fastq(d) for d in files]
    return max(key for rs in recs for r in rs for key in kf_oracle.canonical_kmers(r[1], k))


def _ug_conditions(name, r, missed):
    family, k = name.split("-")[0], r["k"]
    rounds = [tuple(x) for x in r["rounds"]]
    removed = [x for x in rounds if x[1]]
    lengths = sorted(t[0] - k + 1 for t in r["unitigs"])
    if family == "ladder":
        trim = cases()[name][3]["trim"]
        if rounds != ladder_plan(trim):
            missed.append("rounds %r are not the plan %r" % (rounds, ladder_plan(trim)))
        if trim + 1 not in lengths:
            missed.append("the branch of trim + 1 k-mers is gone")
    elif family == "snapshot":
        down = snapshot_reads(k)[1]
        if [x[1] for x in removed] != [6]:
            missed.append("not one round that removes 6: %r" % rounds)
        if r["all"].split(b"\n")[1:2] not in ([down], [revcomp(down)]) or len(r["unitigs"]) != 1:
            missed.append("the unitig left is not the sequence below the junction")
    elif family == "cascade":
        if rounds[-3:] != [(6, 12), (6, 6), (6, 0)] or len(removed) != 2:
            missed.append("the rounds %r do not end (6, 12), (6, 6), (6, 0)" % rounds)
    elif family == "three_in":
        if [x[1] for x in removed] != [9]:
            missed.append("not one round that removes 9: %r" % rounds)
    elif family == "rings":
        cyc = sorted(t[0] - k + 1 for t in r["unitigs"] if t[4])
        lin = [t[0] - k + 1 for t in r["unitigs"] if not t[4]]
        if r["cycles"] != 12 or cyc != sorted(RING_L):
            missed.append("the cyclic unitigs have %r k-mers" % cyc)
        if lin != [5000]:
            missed.append("the linear unitigs have %r k-mers" % lin)
        if mirror_cycles(r, ring_circles(k)) in (0, 12):
            missed.append("every cycle is emitted from the same strand relative to its reads")
    elif family == "hairpin":
        if k % 2 and r["blocked"] < 1:
            missed.append("no pair of adjacent nodes kept apart by the hairpin rule")
        if k % 2 == 0 and r["alone"] < 1:
            missed.append("no self-complementary solid k-mer standing alone")
    elif family == "selfcomp":
        if r["alone"] < 1:
            missed.append("no self-complementary solid k-mer standing alone")
        if k >= 32 and r["blocked"] < 2:  # (at k = 4 the graph around it is dense)
            missed.append("no join refused because a node is its own reverse complement")
    elif family == "dense":
        if r["solid"] > 3000:
            missed.append("%d solid k-mers" % r["solid"])
    elif family == "wave":
        _wave_conditions(name, missed)
    elif family == "high":
        if largest_key(name) < 3 * 4 ** (k - 1):
            missed.append("no canonical key with the top base T")
        if k % 2 == 0 and r["alone"] < 1:
            missed.append("T^(k/2) A^(k/2) is not a unitig of its own")
    elif family == "parts":
        _parts_conditions(name, r["windows"], missed)


def _wave_conditions(name, missed):
    stage, k, files, _ = cases()[name]
    lens = [len(r[1]) for d in files for r in kf_oracle.parse_fastq(d)]
    waves = [lens[i:i + 64] for i in range(0, len(lens), 64)]
    kind = name.split("-")[1]
    if kind == "short":
        if not any(len(w) == 64 and max(w) < k for w in waves) or not any(min(w) >= k for w in waves):
            missed.append("no wavefront of reads shorter than k between long ones")
    elif kind == "long":
        if not any(sorted(w) == [k] * 63 + [5000] for w in waves):
            missed.append("no wavefront of 63 reads of k bases and one of 5000")
    else:
        if not any({k - 1, k, k + 1} <= set(w) for w in waves):
            missed.append("no wavefront with reads of k - 1, k and k + 1 bases")
        want = {"64+1": [64, 1], "1+64": [1, 64], "0+65": [0, 65]}.get(kind)
        got = [len(kf_oracle.parse_fastq(d)) for d in files]
        if got != (want or [int(kind)] * 2):
            missed.append("record counts %r" % got)
        if kind == "0+65" and files[0] != b"":
            missed.append("the first file is not empty")


def _parts_conditions(name, windows, missed):
    stage, k, _, _ = cases()[name]
    budget, parts, below = parts_budgets(stage, k)
    if windows >= 2000:
        missed.append("%d windows" % windows)
    if parts < 1024:
        missed.append("%d partitions" % parts)
    pre = bin_prefix(cases()[name][2], k)
    if int(pre[-1]) != windows:
        missed.append("the bins hold %d windows of %d" % (pre[-1], windows))
    first = (np.arange(parts + 1, dtype=np.int64) * BINS + parts - 1) // parts
    if np.count_nonzero(np.diff(pre[first])) * 2 >= parts:
        missed.append("most partitions are not empty")
    if pick_partitions(pre, k, below)[0] != 0 or pick_partitions(pre, k, below + 1)[0] == 0:
        missed.append("the budget below the finest cut is not just below it")


def _kf_conditions(name, r, missed):
    family = name.split("-")[0]
    rows = [tuple(x) for x in r["histogram"]]
    row = dict(rows)
    if family == "hist_rows":
        if rows[-5:] != [(1023, 1), (1024, 1), (1025, 1), (10000, 1), (10001, 2)]:
            missed.append("the histogram ends %r" % rows[-5:])
        if sorted(c for _, c in r["abundant"] if c >= 1023) != sorted(HIST_COUNTS):
            missed.append("the large counts are not 1023 ... 10002")
        if set(a for a, _ in rows[:-5]) != {2, 3, 4, 5, 6}:
            missed.append("the background's rows are %r" % rows[:-5])
    elif family == "upper5":
        n5 = {"upper5": 3, "upper5-32": 32, "upper5-33": 33}[name]
        if (r["q1"], r["q3"], r["upper"]) != (2, 3, 5):
            missed.append("q1, q3, upper = %r" % ((r["q1"], r["q3"], r["upper"]),))
        if row.get(4) != 3 or row.get(5) != n5 or max(row) != 5:
            missed.append("rows %r" % rows)
        if len(r["abundant"]) != n5 or r["verdict"] != [1] * (5 * n5) + [0] * (r["pairs"] - 5 * n5):  # the first pairs carry them
            missed.append("%d abundant keys, %d pairs dropped" % (len(r["abundant"]), sum(r["verdict"])))
        if not (any(a and not b for a, b in zip(r["verdict1"], r["verdict2"]))
                and any(b and not a for a, b in zip(r["verdict1"], r["verdict2"]))):
            missed.append("the pairs are not dropped by either mate alone")
    elif family == "on_threshold":
        if not (row.get(r["upper"]) and row.get(r["upper"] - 1)):
            missed.append("no key of count upper and one of count upper - 1: upper %d, rows %r" % (r["upper"], rows))
        if not 0 < sum(r["verdict"]) < r["pairs"]:
            missed.append("%d of %d pairs dropped" % (sum(r["verdict"]), r["pairs"]))
    elif family == "wave":
        _wave_conditions(name, missed)
    elif family == "high":
        k = cases()[name][1]
        if largest_key(name) < 3 * 4 ** (k - 1):
            missed.append("no canonical key with the top base T")
        if not any(x >= 3 * 4 ** (k - 1) for x, _ in r["abundant"]) or not any(x < 4 ** (k - 1) for x, _ in r["abundant"]):
            missed.append("the abundant set has no key with the top base T, or none with the top base A")
    elif family == "parts":
        _parts_conditions(name, r["windows"], missed)
    if family in ("tile", "high", "parts", "on_threshold") and not 0 < sum(r["verdict"]) < r["pairs"]:
        missed.append("%d of %d pairs dropped" % (sum(r["verdict"]), r["pairs"]))


def meets_conditions(name, r):
    """-> the list of the conditions that the case ``name`` was built for and its result ``r`` misses"""
    stage, k, files, params = cases()[name]
    missed = []
    if params.get("error"):
        if "error" not in r:
            missed.append("no format error")
        return missed
    if "error" in r:
        return ["a format error at %r" % (r["error"],)]
    if name.startswith("tile-"):
        tile = name.split("-")[1]
        data = files[0] if stage == "kf" else files[1]
        size, final, marks, long_line = TILE_FILES[tile]
        if len(data) != size or data.endswith(b"\n") != final:
            missed.append("%d bytes, final newline %r" % (len(data), data.endswith(b"\n")))
        if not {m for m, _ in marks} <= newline_bytes(data):
            missed.append("no newline on the marks")
        recs = kf_oracle.parse_fastq(data)
        if long_line and max(len(x[1]) for x in recs) != long_line:
            missed.append("no line of %d bases" % long_line)
        if not any(len(x[1]) == 0 for x in recs):
            missed.append("no record with an empty sequence")
    (_kf_conditions if stage == "kf" else _ug_conditions)(name, r, missed)
    return missed


def family_conditions():
    """the conditions that hold over a family of cases -> the list of those missed"""
    missed = []
    seen = set()
    for tile in TILE_FILES:
        seen |= newline_bytes(cases()["tile-%s-kf" % tile][2][0])
    for b in NEWLINE_BYTES:
        if b not in seen:
            missed.append("no tile file with a newline on byte %d" % b)
    sizes = {TILE_FILES[t][0] for t in TILE_FILES}
    if not {4095, 4096, 4097, 8192} <= sizes or not any(s % 16 == 0 and s % 4096 for s in sizes):
        missed.append("tile file sizes %r" % sorted(sizes))
    for bad, start in (("tile-bad-at-kf", b"t99\n"), ("tile-bad-quality-kf", None)):
        data = cases()[bad][2][0 if start else 1]
        line = expected(bad)["error"][1]
        at = [0] + [x + 1 for x in sorted(newline_bytes(data))]
        if at[line - 1] != 4096:
            missed.append("%s: the offending line starts at byte %d" % (bad, at[line - 1]))
    combos, bytes_seen = set(), set()
    for k in DENSE_K:
        ins, outs = set(), set()
        for d in DENSE_D:
            for i, o, strand, byte in degrees("dense-%d-%d-0" % (k, d)):
                ins.add(i)
                outs.add(o)
                combos.add((i, o, strand))
                if byte >= 0:
                    bytes_seen.add(byte)
        if k >= 3 and (ins != set(range(5)) or outs != set(range(5))):
            missed.append("dense, k = %d: in-degrees %r, out-degrees %r" % (k, sorted(ins), sorted(outs)))
    if len(combos) != 50:
        missed.append("dense: %d of the 50 (in-degree, out-degree, strand) combinations" % len(combos))
    if len(bytes_seen) != 256:
        missed.append("dense: %d distinct neighbour bytes" % len(bytes_seen))
    return missed
