"""Named cases of the assembly evaluation and the conditions they are built to meet, checked on the oracle alone
(tests/test_evaluate_host.py); the GPU tests (tests/test_gpu_evaluate.py) run the same cases on the stage.

A case is a dict: k, min_count, reads (one or two FASTQ texts), assembly (a FASTA text).  The tile cases rest on the layout
of a small file in the sequence store: the records' bases lie back to back, so a record's first base lies at the sum of
the lengths before it (``offsets``; the host test checks it against the loader)."""
import functools
import random

import ev_oracle
import kf_oracle

TILE = 256  # positions of the store per workgroup of the window kernel
KS_WIDTH = (1, 2, 31, 32, 33, 64)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def rand_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


def revcomp(s):
    return s.translate(_COMP)[::-1]


def fastq(seqs, tag=b"r"):
    return b"".join(b"@%s%d\n%s\n+\n%s\n" % (tag, i, s, b"I" * len(s)) for i, s in enumerate(seqs))


def fasta(recs):
    return b"".join(b">%s\n%s\n" % (n.encode(), s) if s else b">%s\n" % n.encode() for n, s in recs)


def tiling(g, length=100, step=25):
    """reads that hold every window of g of up to length - step + 1 bases"""
    at = list(range(0, max(len(g) - length, 0) + 1, step))
    if at[-1] + length < len(g):
        at.append(len(g) - length)
    return [g[p:p + length] for p in at]


def mutate(s, *positions):
    """another base at each of the positions"""
    s = bytearray(s)
    for p in positions:
        s[p] = b"ACGT"[(b"ACGT".index(bytes([s[p]]).upper()) + 1) & 3]
    return bytes(s)


def offsets(recs):
    out, at = [], 0
    for _, s in recs:
        out.append(at)
        at += len(s)
    return out


def _case(k, reads, recs, min_count=2):
    return {"k": k, "min_count": min_count, "reads": list(reads), "records": recs, "assembly": fasta(recs)}


@functools.lru_cache(maxsize=None)
def workload(k):
    """a few hundred pairs over five contigs; the "assembly" is the genome with planted substitutions, an insertion and a
    deletion in the first contig, the second contig written twice, the third three times, the fourth five times, the fifth
    left out"""
    rng = random.Random(20261020)
    g = [rand_seq(rng, n) for n in (900, 300, 260, 250, 300)]
    r1, r2 = [], []
    for _ in range(320):
        c = rng.choice(g)
        p, q = rng.randrange(len(c) - 100 + 1), rng.randrange(len(c) - 100 + 1)
        a, b = c[p:p + 100], revcomp(c[q:q + 100])
        if rng.random() < 0.5:
            a, b = b, a
        r1.append(a)
        r2.append(b)
    r1[7] = r1[7][:40] + b"N" + r1[7][41:]
    r2[9] = r2[9].lower()
    edited = mutate(g[0], 100, 333, 334, 700)
    edited = edited[:500] + b"G" + edited[500:600] + edited[601:]  # an insertion at 500, a deletion at 600
    recs = [("c0", edited), ("c1a", g[1]), ("c1b", g[1]), ("c2a", g[2]), ("c2b", revcomp(g[2])), ("c2c", g[2])]
    recs += [("c3%s" % x, g[3]) for x in "abcde"]
    return _case(k, (fastq(r1), fastq(r2, b"s")), recs)


def _tile_records(k, rng):
    """consecutive slices of one genome, so that a window that crossed two records would be a window of the reads"""
    lengths = [255, 257, 256, 511, 513, k - 1, k, k + 1, 0] + [1] * 300 + [700, 3 * k, 3 * k]
    g = rand_seq(rng, sum(lengths) + 200)
    recs, at = [], 0
    for i, n in enumerate(lengths):
        recs.append(("t%d" % i, g[at:at + n]))
        at += n
    return g, recs


@functools.lru_cache(maxsize=None)
def tiles(k=11):
    """record lengths k - 1, k, k + 1, 255, 256, 257, 511, 513; an empty record; 300 records of one base; one record over
    three tiles; a record that starts on the last byte of a tile; N and lower case at tile offsets 0, 255 and 256; a missing
    window at the last base of a record and at the first base of the next"""
    rng = random.Random(11)
    g, recs = _tile_records(k, rng)
    off = offsets(recs)
    assert off[1] == TILE - 1 and off[2] == 2 * TILE and off[3] == 3 * TILE
    store = bytearray(b"".join(s for _, s in recs))
    for p in (2 * TILE, 4 * TILE - 1, 5 * TILE):  # tile offsets 0, 255, 256
        store[p] = ord("N")
    for p in (3 * TILE - 1, 3 * TILE, 4 * TILE, 5 * TILE - 1):
        store[p] = ord(bytes([store[p]]).lower())
    big = len(recs) - 3  # the record over three tiles: substitutions inside it, one run across a tile boundary
    edge = (off[big] // TILE + 1) * TILE
    for p in (edge + 3, off[big] + 650):
        store[p] = mutate(bytes(store), p)[p]
    last, nxt = len(recs) - 2, len(recs) - 1  # the last base of one record and the first base of the next
    store[off[nxt] - 1] = mutate(bytes(store), off[nxt] - 1)[off[nxt] - 1]
    store[off[nxt]] = mutate(bytes(store), off[nxt])[off[nxt]]
    recs = [(n, bytes(store[o:o + len(s)])) for (n, s), o in zip(recs, off)]
    assert len(recs[last][1]) == 3 * k
    return _case(k, (fastq(tiling(g)),), recs)


@functools.lru_cache(maxsize=None)
def intervals(k=11):
    """a run at a record's first window and one at its last; two runs with one present window between them; a run across
    a tile boundary"""
    rng = random.Random(7)
    g = rand_seq(rng, 1000)
    recs = [("first_last", mutate(g[:200], 0, 199)), ("two_runs", mutate(g[200:400], 50, 50 + k + 1)),
            ("boundary", mutate(g[400:1000], 2 * TILE + 3 - 400))]
    return _case(k, (fastq(tiling(g)),), recs)


def runs_k1():
    """k = 1: every position is a window, so missing windows at the end of one record and at the start of the next touch
    in the store; they are two intervals"""
    return _case(1, (fastq([b"AATTA", b"TTTA"]),), [("a", b"AAC"), ("b", b"CAA"), ("c", b"GGG"), ("d", b"G")], min_count=1)


@functools.lru_cache(maxsize=None)
def extreme(name):
    rng = random.Random(sum(map(ord, name)))
    g, h = rand_seq(rng, 1500), rand_seq(rng, 1500)
    slices = [("s%d" % i, g[p:p + 300]) for i, p in enumerate(range(0, 1500, 300))]
    if name == "nothing_missing":
        return _case(15, (fastq(tiling(g)),), slices)
    if name == "all_missing":
        return _case(15, (fastq(tiling(h)), fastq(tiling(h)[:3], b"s")), slices)
    if name == "no_assembly_window":
        return _case(31, (fastq(tiling(g)),), [("a", g[:30]), ("e", b""), ("b", g[30:31]), ("n", g[100:120] + b"N" + g[121:140])])
    if name == "no_read_window":
        return _case(31, (fastq([g[p:p + 20] for p in range(0, 400, 20)]), fastq([b"", g[:30]], b"s")), slices[:2])
    if name == "palindrome":  # ACGT is its own reverse complement; once in the reads, once in the assembly
        return _case(4, (fastq([b"AACGTT"]),), [("p", b"GACGTC")], min_count=1)
    if name == "copies":  # copy numbers 1..6 at k = 21: class 4 takes 4 and up
        seg = [g[200 * i:200 * i + 60] for i in range(6)]
        recs = [("u%d_%d" % (i + 1, j), seg[i]) for i in range(6) for j in range(i + 1)]
        return _case(21, (fastq(tiling(g)), fastq(tiling(g), b"s")), recs)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def poly_a():
    """the filter's poly_a reads: one k-mer above 10000 (row 10001), present in the assembly"""
    import kfcases
    a, b = kfcases.workload("poly_a")
    first = kf_oracle.lines_of(a)[1]
    return _case(31, (a, b), [("pa", b"A" * 40 + first[:50]), ("other", first[50:] + b"ACGTTGCAAC")])


EXTREMES = ("nothing_missing", "all_missing", "no_assembly_window", "no_read_window", "palindrome", "copies")


def tiny():
    """small enough to verify by hand: reads ACGTA, assembly ACGTT, k = 3"""
    return _case(3, (fastq([b"ACGTA"]),), [("c", b"ACGTT")], min_count=1)


EDGE_CASES = {"tiles": tiles, "intervals": intervals, "runs_k1": runs_k1, "tiny": tiny, "poly_a": poly_a}
EDGE_CASES.update({name: functools.partial(extreme, name) for name in EXTREMES})


@functools.lru_cache(maxsize=None)
def expected(name, k=None):
    """the oracle's result of a named case (the workload at k, or an edge case)"""
    case = workload(k) if name == "workload" else EDGE_CASES[name]()
    return ev_oracle.run(case["k"], case["reads"], case["assembly"], min_count=case["min_count"])


def meets_conditions(want):
    """what a workload must show (an empty list: everything)"""
    bad = []
    if not want["total"][2] > 0:
        bad.append("missing > 0")
    for c in range(ev_oracle.CLASSES):
        if not any(cc == c for cc, _ in want["spectrum"]):
            bad.append("copy class %d is empty" % c)
    if not want["intervals"]:
        bad.append("an interval")
    if not want["solid"] > want["found"] > 0:
        bad.append("solid > found > 0")
    return bad
