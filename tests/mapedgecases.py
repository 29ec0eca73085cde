"""Inputs of the mapper's tests that aim at how its kernels are built (muchsalsa_amd/csrc/msgpu_map.hip), shared by
tests/test_mapper_edges_host.py, tests/test_gpu_mapper_edges.py and tools/make_mapper_edge_fixtures.py: builders, parameters,
the restatement's result for every case (tests/map_oracle.py, computed once per process) and the conditions every input must
meet, checked on the restatement alone.  The interface is that of tests/mapcases.py: a case is (name of the input,
parameters); an input is (targets text, its file name, queries text, its file name), always two FASTA files.

The inputs:
  tile-K-W-UNIT       k_mp_sketch's tiles of 256 positions: one record of UNIT * 256 bases with an N at the end of every UNIT
                      bases (UNIT odd, so stretch ends and starts fall on every residue modulo 256), against itself and its
                      reverse complement
  ends-K-W            700 records of max(1, K - 2) .. K + W + 5 bases, one text cut into pieces, against themselves
  ties-K-W            hash ties of rule 2: unique pieces between runs of A, T, AC, ACG, ACGT and of a random unit of W - 1, W
                      and W + 1 bases (and, at even K, a k-mer that is its own reverse complement), against the unique pieces
                      with the first half of every run, forward and reverse-complemented
  letters             lower-case runs and IUPAC letters inside matching pieces
  window-Z-M[-K]      k_mp_chain's 64 predecessors: one group of Z + M + 2 anchors in which only A (index Z) and C (the last)
                      can link, with M anchors between them
  tie-I-P-Q           rule 5's tie: C at index I of its group with two predecessors at indices P < Q that offer the same
                      value and cannot link to each other; every other anchor links to nothing
  sizes, sizes-rc     k_mp_classify's classes and k_mp_chain16's rows: 24 query records whose groups have SIZES anchors
  small               mapcases' small workload (for the anchor read-out)
READOUT (max_gap = 0, min_count = 1, min_score = 0) allows no link and keeps every group, so every anchor is a chain of its
own and the chain table reads rules 1 to 4 out position by position.

Bases come from numpy.random.default_rng(seed) over ACGT.  A piece of the target that is copied into a query gets, in the
query, a base in front of it and one behind it that differ from the target's neighbours (``_embed``), so that no piece grows.

The restatement's seconds on the project's CPU host (tools/make_mapper_edge_fixtures.py prints them): the slowest cases are
the small workload in read-out mode and ties-4-1 with chaining, 1.7 s each; all 81 cases together take 22 s, and
tests/test_mapper_edges_host.py as a whole 26 s."""
import functools
import os

import numpy as np

import map_oracle
import mapcases

READOUT = dict(max_gap=0, min_count=1, min_score=0)
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
rc = map_oracle.revcomp


def bases(rng, n):
    return ACGT[rng.integers(0, 4, size=int(n))].tobytes()


def _fa(recs):
    return b"".join(b">%s\n%s\n" % (n, s) for n, s in recs)


def _other(*forbidden):
    return next(b for b in b"ACGT" if b not in forbidden)


def _embed(rng, target, qlen, pieces):
    """a query of ``qlen`` random bases with target[x:x + n] at y for every (x, y, n) of ``pieces``; the query's bases next to a
    piece differ from the target's bases next to it"""
    q = bytearray(bases(rng, qlen))
    taken = bytearray(qlen)
    for x, y, n in pieces:
        assert 0 <= x and x + n <= len(target) and 0 <= y and y + n <= qlen and not any(taken[y:y + n]), (x, y, n)
        q[y:y + n] = target[x:x + n]
        taken[y:y + n] = b"\x01" * n
    forbid = {}
    for x, y, n in pieces:
        for qp, tp in ((y - 1, x - 1), (y + n, x + n)):
            if 0 <= qp < qlen and 0 <= tp < len(target):
                assert not taken[qp], "two pieces touch in the query"
                forbid.setdefault(qp, []).append(target[tp])
    for qp, f in forbid.items():
        q[qp] = _other(*f)
    return bytes(q)


# ---- rule 2: the sketch ---------------------------------------------------------------------------------------------

TILE = [(15, 5, 37), (16, 2, 37), (15, 64, 101), (32, 64, 101), (15, 1, 37)]
ENDS = [(15, 5), (4, 1), (32, 64), (15, 1)]
TIES_K, TIES_W = (4, 15, 32), (1, 2, 5, 64)
TIES_PARAMS = (dict(READOUT, max_occ=1000), dict(max_occ=1000, min_count=2, min_score=0))
N_ENDS = 700


def tile_input(k, w, unit):
    rng = np.random.default_rng(1000 + 100 * k + w)
    s = bytearray(bases(rng, unit * 256))
    assert unit % 2 == 1
    for i in range(unit - 1, len(s), unit):
        s[i] = ord("N")
    s = bytes(s)
    return _fa([(b"t", s)]), _fa([(b"q", s), (b"qr", rc(s))])


def ends_lengths(k, w):
    rng = np.random.default_rng(2000 + 100 * k + w)
    return [int(x) for x in rng.integers(max(1, k - 2), k + w + 6, size=N_ENDS)]


def ends_input(k, w):
    lens = ends_lengths(k, w)
    text = bases(np.random.default_rng(2500 + 100 * k + w), sum(lens))
    recs, at = [], 0
    for i, n in enumerate(lens):
        recs.append((b"e%d" % i, text[at:at + n]))
        at += n
    return _fa(recs), _fa(recs)


@functools.lru_cache(maxsize=None)
def palindrome(k):
    """an even k's k-mer that is its own reverse complement, S + revcomp(S), with the smallest hash of 4096 draws (of all 16 at
    k = 4), so that it is the minimizer of the windows around it"""
    rng = np.random.default_rng(3000 + k)
    best = None
    for _ in range(4096):
        s = bases(rng, k // 2)
        p = s + rc(s)
        key = 0
        for b in p:
            key = (key << 2) | map_oracle.CODE[b]
        h = map_oracle.kf_hash(key)
        if best is None or h < best[0]:
            best = (h, p)
    return best[1]


def ties_run_length(k):
    """about 60 bases; at k = 32 long enough for the query's half of a run to hold whole k-mers"""
    return max(60, 2 * (k + 8))


def ties_runs(k, w, rng):
    n = ties_run_length(k)
    runs = [b"A" * n, b"T" * n, (b"AC" * n)[:n], (b"ACG" * n)[:n], (b"ACGT" * n)[:n]]
    for u in (w - 1, w, w + 1):
        if u >= 1:  # the same k-mer again u positions on: its first half holds a pair of them
            unit = bases(rng, u)
            m = max(n, 2 * (2 * u + k))
            runs.append((unit * (m // u + 1))[:m])
    if k % 2 == 0:
        runs.append(palindrome(k))
    return runs


def ties_input(k, w):
    rng = np.random.default_rng(4000 + 100 * k + w)
    runs = ties_runs(k, w, rng)
    t, q = [], []
    for r in runs:
        u = bases(rng, 100)
        t += [u, r]
        q += [u, r if k % 2 == 0 and r == palindrome(k) else r[:len(r) // 2]]
    u = bases(rng, 100)
    t, q = b"".join(t + [u]), b"".join(q + [u])
    return _fa([(b"t", t)]), _fa([(b"q", q), (b"qr", rc(q))])


def letters_input():
    rng = np.random.default_rng(5000)
    g = bytearray(bases(rng, 1200))
    t = bytearray(g)
    q = bytearray(g[100:1100])
    t[200:260] = bytes(t[200:260]).lower()      # a lower-case run in the target only
    q[300:420] = bytes(q[300:420]).lower()      # one in the query only (target 400 .. 520)
    t[600:640] = bytes(t[600:640]).lower()      # one in both
    q[500:540] = bytes(q[500:540]).lower()
    for i, c in zip(range(700, 1000, 23), b"RYKMSWBDHVrykm"):
        t[i] = c                                 # IUPAC letters in the target
    for i, c in zip(range(650, 950, 29), b"yRkMsWbDhV"):
        q[i] = c                                 # and others in the query
    q[40] = ord("U")
    t[1150] = ord("-")
    q = bytes(q)
    return _fa([(b"t", bytes(t))]), _fa([(b"q", q), (b"qr", rc(q))])


# ---- rules 5 and 6: the chain kernels -------------------------------------------------------------------------------

WINDOW_Z, WINDOW_M = (0, 1, 37, 63, 64), (62, 63, 64, 65)
WINDOW_PARAMS = dict(w=1, bandwidth=10, max_gap=100000, min_count=2, min_score=30)
TIE_PARAMS = dict(w=1, bandwidth=10, max_gap=100000, min_count=2, min_score=0)
TIE_I = (64, 65, 100, 127, 128)
TIE_SHAPES = [(i, p, q) for i in TIE_I for p, q in ((i - 64, i - 1), (i - 64, i - 63), (i - 2, i - 1))] + [
    (9, 0, 8), (9, 0, 1), (9, 7, 8)]
# (in this order rule 9's greedy cut at the smallest budget leaves most batches with one group of at most 16 anchors)
SIZES = (193, 1, 192, 2, 191, 3, 129, 128, 15, 127, 16, 33, 66, 65, 16, 32, 64, 63, 16, 31, 17, 16, 16, 16)
SIZES_PARAMS = dict(w=1, min_count=1, min_score=0)
C0, OFF = 10000, 5000  # the diagonal of the anchors that link, and how far above or below it the others lie


def group_input(seed, anchors, k):
    """one target and one query whose only shared k-mers are one per (x, y) of ``anchors``: random bases now and then share a
    k-mer by chance, so the seed moves on until rules 1 to 4 (at w = 1) give these anchors and no others"""
    step = k + 1
    xs, ys = sorted(x for x, _ in anchors), sorted(y for _, y in anchors)
    assert all(b - a >= step for a, b in zip(xs, xs[1:])) and all(b - a >= step for a, b in zip(ys, ys[1:]))
    assert xs[0] >= 1 and ys[0] >= 1
    for attempt in range(16):
        rng = np.random.default_rng(seed + 100000 * attempt)
        t = bases(rng, xs[-1] + step)
        q = _embed(rng, t, ys[-1] + step, [(x, y, k) for x, y in anchors])
        index = map_oracle.build_index([(b"t", t)], k, 1, 1)[0]
        if map_oracle.anchors(index, [(b"q", q)], k, 1, 0) == {(0, 0, 0): sorted(anchors)}:
            return _fa([(b"t", t)]), _fa([(b"q", q)])
    raise AssertionError("no seed gives the anchors alone")


def _above(x, i, step):
    """the i-th anchor of a run whose y falls by ``step`` as x rises by it, all at least OFF above the diagonal C0"""
    return (x, x + C0 + OFF + 2 * step * (200 - i))


def _below(x, i, step):
    return (x, x + C0 - OFF - 2 * step * i)


def window_anchors(z, m, k=15):
    """sorted by x: z anchors D (above), A, m anchors B (below), C; A and C within 3 of the diagonal C0"""
    step = k + 1
    x = [step * (j + 1) for j in range(z + m + 2)]
    out = [_above(x[i], i, step) for i in range(z)]
    out.append((x[z], x[z] + C0))
    out += [_below(x[z + 1 + i], i, step) for i in range(m)]
    out.append((x[z + m + 1], x[z + m + 1] + C0 + 3))
    return out


def tie_anchors(i, p, q, k=15):
    """sorted by x: C at index i; P at index p offers it dd = 6 from above the diagonal, Q at index q dd = 6 from below, so both
    offer f + k - pen(6) and P -> Q has dd = 12 > bandwidth; the others lie OFF away (above in front of P, below behind it).
    The anchors are k + 13 apart in x, so that P and Q are more than k apart in y even when q = p + 1"""
    step = k + 13
    x = [step * (j + 1) for j in range(i + 1)]
    out = []
    for j in range(i):
        if j == p:
            out.append((x[j], x[j] + C0 + 6))
        elif j == q:
            out.append((x[j], x[j] + C0 - 6))
        elif j < p:
            out.append(_above(x[j], j, step))
        else:
            out.append(_below(x[j], j, step))
    out.append((x[i], x[i] + C0))
    return out


def sizes_input(reverse):
    rng = np.random.default_rng(7000)
    k = 15
    gaps = [bases(rng, 7) for _ in range(len(SIZES) + 1)]
    pieces = [bases(rng, n + k - 1) for n in SIZES]
    t, at = gaps[0], []
    for p, g in zip(pieces, gaps[1:]):
        at.append(len(t))
        t += p + g
    qs = []
    for i, (x, p) in enumerate(zip(at, pieces)):
        q = _embed(rng, t, len(p) + 40, [(x, 20, len(p))])
        qs.append((b"s%d" % i, rc(q) if reverse else q))
    return _fa([(b"t", t)]), _fa(qs)


# ---- the cases ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (targets text, targets file name, queries text, queries file name)"""
    if name == "small":
        return mapcases.inputs("small")
    kind, *a = name.split("-")
    a = [int(x) for x in a if x != "rc"]
    if kind == "tile":
        t, q = tile_input(*a)
    elif kind == "ends":
        t, q = ends_input(*a)
    elif kind == "ties":
        t, q = ties_input(*a)
    elif kind == "letters":
        t, q = letters_input()
    elif kind == "window":
        k = a[2] if len(a) > 2 else 15
        t, q = group_input(8000 + 100 * a[0] + a[1] + k, window_anchors(a[0], a[1], k), k)
    elif kind == "tie":
        t, q = group_input(9000 + 1000 * a[0] + 10 * a[1] + a[2], tie_anchors(*a), 15)
    elif kind == "sizes":
        t, q = sizes_input(name.endswith("-rc"))
    else:
        raise KeyError(name)
    return t, "t.fa", q, "q.fa"


def write_inputs(name, directory):
    """the input's files in ``directory`` -> (targets path, queries path)"""
    t, tn, q, qn = inputs(name)
    tp, qp = os.path.join(str(directory), tn), os.path.join(str(directory), qn)
    for path, text in ((tp, t), (qp, q)):
        with open(path, "wb") as f:
            f.write(text)
    return tp, qp


@functools.lru_cache(maxsize=None)
def records(name):
    t, tn, q, qn = inputs(name)
    return map_oracle.parse(t, map_oracle.is_fastq_name(tn)), map_oracle.parse(q, map_oracle.is_fastq_name(qn))


@functools.lru_cache(maxsize=None)
def _expected(name, params):
    t, q = records(name)
    return map_oracle.run(t, q, **dict(params))


def expected(name, **params):
    return _expected(name, tuple(sorted(params.items())))


SKETCH = ([("small", dict(READOUT))] +
          [("tile-%d-%d-%d" % p, dict(READOUT, k=p[0], w=p[1])) for p in TILE] +
          [("ends-%d-%d" % p, dict(READOUT, k=p[0], w=p[1])) for p in ENDS] +
          [("ties-%d-%d" % (k, w), dict(prm, k=k, w=w)) for k in TIES_K for w in TIES_W for prm in TIES_PARAMS] +
          [("letters", dict(READOUT)), ("letters", dict(READOUT, w=1)), ("letters", dict(w=1, min_score=40))])
WINDOW = [("window-%d-%d" % (z, m), dict(WINDOW_PARAMS)) for z in WINDOW_Z for m in WINDOW_M]
EXTREME = ([("window-37-%d" % m, dict(WINDOW_PARAMS, max_gap=2 ** 31 - 1, bandwidth=2 ** 31 - 1)) for m in (63, 64)] +
           [("window-37-%d-32" % m, dict(WINDOW_PARAMS, k=32, bandwidth=100000, min_score=0)) for m in (63, 64)])
TIE = [("tie-%d-%d-%d" % s, dict(TIE_PARAMS)) for s in TIE_SHAPES]
CLASSES = [("sizes", dict(SIZES_PARAMS)), ("sizes-rc", dict(SIZES_PARAMS))]
CASES = SKETCH + WINDOW + EXTREME + TIE + CLASSES


def case_id(case):
    return case[0] + "".join("-%s%d" % kv for kv in sorted(case[1].items()))


def is_readout(params):
    return all(params.get(key) == v for key, v in READOUT.items())
