"""Inputs of the unitig assembly above k = 64 (keys of three and of four 64-bit words), shared by the host and the GPU file:
``cases()`` maps a name to (k, files, params), ``expected(name)`` is the restatement's result (tests/ug_wide_oracle.py, once per
process).  The builders are the existing ones wherever they take k (tests/kmeredgecases.py: ladders, hairpin, selfcomp,
three_in); ``rings`` and the bubble cases are copies of synth.unitig_cases / synth.unitig_bubble_cases with reads long enough
to hold k-mers, because those builders fix the read length at 100 and 80 bases.  Every input is a function of fixed seeds.

    rings-K      two circular sequences of 300 bases, reads of k + 100 bases tiled around each at a step of 10, each twice: two
                 cyclic unitigs, whose min-reduction compares 2k-bit strings across the words
    selfcomp-K   kmeredgecases.selfcomp_reads (even k): a self-complementary k-mer; hairpin-K  kmeredgecases.hairpin_reads
    ladder-K-K   kmeredgecases.ladder_reads(k, k): tips of every limit and limit + 1 -- rule 4's walk, rule 5's joins
    words-K      two solid k-mers that differ only in their first base and two that differ only in their last, each the
                 first k-mer of an emitted unitig: rule 6's order rests on the top word alone, and on the lowest alone
    small-K      the shape of ugcases.SMALL (30 kb with repeats) at a read length of 250
    edge-K, tie-K, indel_short-K (and -flip)   synth.unitig_bubble_cases' three constructions, bubble = 3 k
    three_in-K   kmeredgecases.three_in_reads with trim = 0: forks that stay, for rule 10
"""
import functools

import kmeredgecases as E
import ug_wide_oracle
import ugbubblecases

KS = (65, 96, 97, 128)  # the first and the last k of three words, and of four
KS_EDGE = (65, 97)      # where the two top bits stand alone in a new word
HAND = ("rings", "selfcomp", "hairpin")
BUBBLES = ("edge", "tie", "indel_short")
SMALL = dict(genome=30000, coverage=30, read_len=250, seed=3, families=3, copies=8, repeat_len=400)
KS_SMALL = (90, 128)
MIN_LENGTH = 100  # of the hand-made cases


def ring_reads(k):
    rings = [E.rnd(300, 101), E.rnd(300, 102)]
    return [[(r * 3)[at:at + k + 100] for at in range(0, 300, 10) for _ in (0, 1)] for r in rings], rings


def words_reads(k):
    """-> (reads, (X1, X2, Y1, Y2) as base strings).  X = c + B for c in A, C: B ends in A, so rc(X) starts with T and X is the
    emitted orientation; the two reads go on with different bases, so X1 and X2 each have both continuations as successors and
    are unitigs of one k-mer.  Y = B' + c: B' starts with A and each read ends in A, so the mirror chain's first k-mer starts
    with T; every k-mer of the two reads holds the differing base or lies in the reads' own random tails."""
    B = E.rnd(k - 2, 7000 + k) + b"A"
    t1, t2 = b"G" + E.rnd(k + 8, 7100 + k), b"T" + E.rnd(k + 8, 7200 + k)
    B2 = b"A" + E.rnd(k - 2, 7300 + k)
    u1, u2 = E.rnd(k + 8, 7400 + k) + b"A", E.rnd(k + 8, 7500 + k) + b"A"
    reads = [b"A" + B + t1, b"C" + B + t2, B2 + b"A" + u1, B2 + b"C" + u2]
    return reads, (b"A" + B, b"C" + B, B2 + b"A", B2 + b"C")


def kmer_of(text):
    x = 0
    for b in text:
        x = (x << 2) | b"ACGT".index(b)
    return x


def _tile(seq, L, step=10):
    starts = list(range(0, len(seq) - L + 1, step))
    if starts[-1] != len(seq) - L:
        starts.append(len(seq) - L)
    return [seq[s:s + L] for s in starts]


def _snp(seq, at):
    return seq[:at] + bytes([b"ACGT"[(b"ACGT".index(seq[at]) + 1) % 4]]) + seq[at + 1:]


def bubble_reads(name, k):
    """synth.unitig_bubble_cases' edge, tie and indel_short with every haplotype tiled into reads of k + 100 bases, and
    indel_short's one extra read cut k + 19 bases to either side of the site, so that it holds every k-mer over the site; its
    haplotypes are written six times each, because the shorter branch's sum stays below the longer's only where a k-mer is
    counted more than (k - 1) / 2 times (synth.unitig_bubble_cases says why), and a read of k + 100 bases at a step of 10
    counts a k-mer ten times"""
    A, p, L = E.rnd(400, 401), 200, k + 100
    dele = A[:p] + A[p + 2:]
    haps, extra = {"edge": ([(A, 3), (_snp(A, p), 2)], []), "tie": ([(A, 2), (_snp(A, p), 2)], []),
                   "indel_short": ([(A, 6), (dele, 6)], [dele[p - k - 19:p + k + 19]])}[name]
    return [r for seq, m in haps for r in _tile(seq, L) for _ in range(m)] + extra


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (k, files, params); ``params`` goes to the restatement and to the stage as it is"""
    c = {}
    for k in KS:
        twice = lambda reads: [r for r in reads for _ in (0, 1)]  # noqa: E731  (solid at min_count = 2)
        rr = ring_reads(k)[0]
        c["rings-%d" % k] = (k, [E.fq(rr[0], b"a"), E.fq(rr[1], b"b")], dict(min_length=MIN_LENGTH))
        if k % 2 == 0:
            # (trim = 32: the two arms hold fewer than k k-mers, and at trim = k they would go as tips)
            c["selfcomp-%d" % k] = (k, [E.fq(twice(E.selfcomp_reads(k)[0]), b"s")], dict(min_length=MIN_LENGTH, trim=32))
        c["hairpin-%d" % k] = (k, [E.fq(twice(E.hairpin_reads(k)), b"h")], dict(min_length=MIN_LENGTH))
        c["ladder-%d-%d" % (k, k)] = (k, [E.fq(E.ladder_reads(k, k))], dict(E.UG, trim=k))
    for k in KS_EDGE:
        c["words-%d" % k] = (k, [E.fq(words_reads(k)[0])], dict(E.UG, trim=0))
        for name in BUBBLES:
            data = E.fq(bubble_reads(name, k), b"b")
            p = dict(bubble=3 * k, trim=k, min_length=MIN_LENGTH)
            c["%s-%d" % (name, k)] = (k, [data], p)
            c["%s-%d-flip" % (name, k)] = (k, [ugbubblecases.flipped(data)], p)
            c["%s_plain-%d" % (name, k)] = (k, [data], dict(p, bubble=0))  # (the counts before popping)
            c["%s_plain-%d-flip" % (name, k)] = (k, [ugbubblecases.flipped(data)], dict(p, bubble=0))
        r = E.three_in_reads(k)
        c["three_in-%d" % k] = (k, [E.fq(r[:2]), E.fq(r[2:])], dict(E.UG, trim=0, graph=True))
        c["hairpin_gfa-%d" % k] = (k, c["hairpin-%d" % k][1], dict(min_length=MIN_LENGTH, graph=True))
    for k in KS_SMALL:
        from muchsalsa_amd import synth
        c["small-%d" % k] = (k, list(synth.kmer_filter_workload(**SMALL)), {})
    return c


def names(family=None):
    return [n for n in cases() if family is None or n.split("-")[0] in family]


@functools.lru_cache(maxsize=None)
def expected(name, found=False):
    """the restatement on the case -> its result (with ``found``: (result, the bubbles judged per bubble round))"""
    k, files, params = cases()[name]
    seen = [] if found else None
    r = ug_wide_oracle.run(k, files, found=seen, **params)
    return (r, seen) if found else r


def bubble_conditions(full):
    """what the bubble case was built for, on the restatement alone -> (its result, the list of the conditions missed)"""
    name, k = full.split("-")[0], cases()[full][0]
    want, found = expected(full, found=True)
    missed = []
    judged = [b for b in found[0] if b[3] is not None]
    if len(judged) != 1 or want["bubbles"] != 1 or want["bubble_kmers"] < k - 1 or len(want["unitigs"]) != 1:
        return want, ["not one bubble popped into one unitig: %r" % (want["bubble_rounds"],)]
    (u, t, brs, win), = judged
    counts = expected(full.replace(name, name + "_plain", 1))["counts"]
    stats = [(sum(counts[min(x, ug_wide_oracle.rc(x, k))] for x in path), len(path)) for _, path in brs]
    if name == "edge" and [n for _, n in stats] != [k, k]:
        missed.append("branches of %r k-mers" % ([n for _, n in stats],))
    if name == "tie" and (stats[0][0] * stats[1][1] != stats[1][0] * stats[0][1] or win != 0 or brs[0][0] > brs[1][0]):
        missed.append("no tie decided by the base")
    if name == "indel_short":
        shorter = min(range(2), key=lambda i: stats[i][1])
        if stats[0][1] == stats[1][1] or win != shorter or stats[shorter][0] >= stats[1 - shorter][0]:
            missed.append("the shorter branch does not win by the mean against the sum: %r, winner %d" % (stats, win))
    return want, missed
