"""Inputs of the edit-script and cigar-mode tests, shared by the host and the GPU files: the pair lists of msgpu_edit_script
(every one is a function of fixed seeds), the mapper cases of cigar mode, and the restatement's result for each (computed once
per process, on top of the exact-mode result that tests/mapcases.py caches)."""
import functools
import os

import numpy as np

import map_cigar_oracle
import map_oracle
import mapcases

ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def mutate(rng, s, n_edits):
    """(tests/test_gpu_edit_distance.py's, copied)"""
    s = bytearray(s)
    for _ in range(n_edits):
        op = int(rng.integers(0, 3))
        pos = int(rng.integers(0, len(s) + 1))
        if op == 0 and len(s):  # substitution
            pos = min(pos, len(s) - 1)
            s[pos] = b"ACGT"[(b"ACGT".index(s[pos]) + 1 + int(rng.integers(0, 3))) % 4] if s[pos] in b"ACGT" else 65
        elif op == 1:  # insertion
            s.insert(pos, b"ACGT"[int(rng.integers(0, 4))])
        elif len(s):  # deletion
            del s[min(pos, len(s) - 1)]
    return bytes(s)


RANDOM_BANDS = (127, 64, 8, 1, 0)


@functools.lru_cache(maxsize=None)
def random_pairs(band):
    """the first generator of tests/test_gpu_edit_distance.py"""
    rng = np.random.default_rng(100 + band)
    pairs = []
    for _ in range(150):
        n = int(rng.integers(0, 1800))
        a = bytes(rng.choice(ALPHA, n))
        pairs.append((a, mutate(rng, a, int(rng.integers(0, 2 * band + 12)))))
    pairs += [(b"", b""), (b"A", b""), (b"", b"ACGT"), (b"ACGT", b"ACGT"), (b"ACGT", b"TGCA"), (b"A" * 300, b"A" * 290)]
    pairs += [(bytes(rng.choice(ALPHA, 700)), bytes(rng.choice(ALPHA, 650))) for _ in range(5)]
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def slide_pairs():
    """its third: single edits around multiples of 8, 16 and 512 and at the first and last byte, sequences that end inside a
    step, near-identical pairs of 40 kb, and last a pair that ends with the device buffers (band 64)"""
    rng = np.random.default_rng(5)
    base = bytes(rng.choice(ALPHA, 2100))
    pairs = []
    for pos in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 511, 512, 513, 519, 520, 527, 528, 529, 1023, 1024, 1031, 1040, 2098, 2099):
        sub = bytearray(base)
        sub[pos] = b"ACGT"[(b"ACGT".index(sub[pos]) + 1) % 4]
        pairs.append((base, bytes(sub)))
        pairs.append((base, base[:pos] + base[pos + 1:]))
        pairs.append((base[:pos] + b"G" + base[pos:], base))
    for n in (1, 7, 8, 9, 15, 16, 17, 31, 511, 512, 513, 527, 528, 1031):
        pairs.append((base[:n], base[:n]))
        pairs.append((base[:n], base[:n] + b"A"))
        pairs.append((base[:n] + b"C", base[:n] + b"T"))
    long_a = bytes(rng.choice(ALPHA, 40000))
    pairs += [(long_a, mutate(rng, long_a, k)) for k in (0, 1, 5, 30)]
    pairs.append((base, base))
    return tuple(pairs)


@functools.lru_cache(maxsize=None)
def long_pairs():
    """its second: pairs of 30 kb and 9 kb with 50 to 90 edits (band 127)"""
    rng = np.random.default_rng(7)
    a = bytes(rng.choice(ALPHA, 30000))
    b = mutate(rng, a, 60)
    c = mutate(rng, b, 50)
    short = bytes(rng.choice(ALPHA, 9000))
    short2 = mutate(rng, short, 90)
    return ((a, b), (b, a), (a, a), (b, c), (short, short2), (short2, short))


@functools.lru_cache(maxsize=None)
def sweep_pairs():
    """200-base pairs with d = 0..129 spread substitutions, and the same with d deletions (band 127): the distances cross the
    boundary between the two classes of the kernel, the band and band + 1"""
    rng = np.random.default_rng(17)
    pairs = []
    for d in range(130):
        a = bytes(rng.choice(ALPHA, 200))
        where = [(2 * i + 1) * 200 // (2 * d) for i in range(d)] if d else []
        sub = bytearray(a)
        for p in where:
            sub[p] = b"ACGT"[(b"ACGT".index(sub[p]) + 1) % 4]
        pairs.append((a, bytes(sub)))
        pairs.append((a, bytes(x for i, x in enumerate(a) if i not in set(where))))
    return tuple(pairs)


TIE_BAND = 64


@functools.lru_cache(maxsize=None)
def tie_pairs():
    """600 two-letter pairs over homopolymer, dinucleotide and trinucleotide runs: inputs on which candidates of two kinds
    reach equally far, so the order X, D, I of rule 10 decides"""
    import random
    r = random.Random(3)
    out = []
    for t in range(600):
        unit = [b"A", b"AC", b"AAC", b"ACC"][t % 4]
        a = bytearray((unit * 60)[:r.randrange(10, 60)])
        for _ in range(r.randrange(0, 3)):
            a[r.randrange(len(a))] = r.choice(b"AC")
        b = bytearray(a)
        for _ in range(r.randrange(1, 9)):
            op, pos = r.randrange(3), r.randrange(len(b) + 1)
            if op == 0 and b:
                b[min(pos, len(b) - 1)] = r.choice(b"AC")
            elif op == 1:
                b.insert(pos, r.choice(b"AC"))
            elif b:
                del b[min(pos, len(b) - 1)]
        out.append((bytes(a), bytes(b)))
    return tuple(out)


EDGE_BAND = 8
EDGE_PAIRS = ((b"", b""), (b"A", b""), (b"", b"ACGT"), (b"A", b"CCA"), (b"CCA", b"A"), (b"A" * 30, b"A" * 25), (b"ACGT", b"TGCA"),
              (b"", b"A" * EDGE_BAND), (b"A" * EDGE_BAND, b""), (b"", b"A" * (EDGE_BAND + 1)), (b"A" * (EDGE_BAND + 1), b""))


@functools.lru_cache(maxsize=None)
def slab_pairs():
    """300-base pairs with 32..91 spread substitutions (the class whose tables share the slab: 60 pairs of differing d), three
    times over, and a few of the other classes between them (band 127)"""
    rng = np.random.default_rng(23)
    pairs = []
    for rep in range(3):
        for d in range(32, 92):
            a = bytes(rng.choice(ALPHA, 300))
            sub = bytearray(a)
            for i in range(d):
                p = (2 * i + 1) * 300 // (2 * d)
                sub[p] = b"ACGT"[(b"ACGT".index(sub[p]) + 1) % 4]
            pairs.append((a, bytes(sub)))
            if d % 10 == 0:
                pairs += [(a, a), (a, mutate(rng, a, 5)), (a, a[:100])]
    return tuple(pairs)


def pair_lists():
    """name -> (pairs, band): every list the GPU file gives msgpu_edit_script"""
    out = {"random-%d" % band: (random_pairs(band), band) for band in RANDOM_BANDS}
    out.update({"slides": (slide_pairs(), 64), "long": (long_pairs(), 127), "sweep": (sweep_pairs(), 127),
                "ties": (tie_pairs(), TIE_BAND), "edges": (EDGE_PAIRS, EDGE_BAND), "slab": (slab_pairs(), 127)})
    return out


@functools.lru_cache(maxsize=None)
def expected_scripts(name):
    """-> (dist, off, words) of the restatement for a pair list"""
    pairs, band = pair_lists()[name]
    dist, off, words = [], [0], []
    for a, b in pairs:
        d, w = map_cigar_oracle.script(a, b, band)
        dist.append(d)
        words += w or []
        off.append(len(words))
    return dist, off, words


# ---- the mapper in cigar mode

@functools.lru_cache(maxsize=None)
def slab_link_case():
    """two records whose single link spans 560 bases with 40 evenly spaced substitutions: no 15-mer of the stretch survives, so
    it is one segment of 40 edits, more than the LDS class takes"""
    G = mapcases._g(3000, 43)
    left, mid, right = G[0:220], bytearray(G[220:780]), G[780:1000]
    changed = bytearray(mid)
    for p in range(7, 560, 14):
        changed[p] = b"ACGT"[(b"ACGT".index(changed[p]) + 1) % 4]
    return mapcases._fa([(b"t", left + bytes(mid) + right)]), mapcases._fa([(b"q", left + bytes(changed) + right)])


HAND = ("perfect", "reverse", "one_sided", "beyond_band", "two_chains", "cut", "empty_queries")
CASES = ([("clean", {}), ("clean", dict(band=8)), ("tiled", {}), ("small", dict(k=32)), ("small", dict(k=15, w=1)), ("main", {}),
          ("main_ava", {})] + [(name, {}) for name in HAND] + [("slab_link", {})])


def write_inputs(name, directory):
    if name != "slab_link":
        return mapcases.write_inputs(name, directory)
    t, q = slab_link_case()
    tp, qp = os.path.join(str(directory), "t.fa"), os.path.join(str(directory), "q.fa")
    for path, text in ((tp, t), (qp, q)):
        with open(path, "wb") as f:
            f.write(text)
    return tp, qp


def records(name):
    if name != "slab_link":
        return mapcases._records(name)
    t, q = slab_link_case()
    return map_oracle.parse(t, False), map_oracle.parse(q, False)


@functools.lru_cache(maxsize=None)
def _expected(name, params):
    params = dict(params)
    t, q = records(name)
    if name == "slab_link":
        return map_cigar_oracle.cigar_run(t, q, **params)
    exact = mapcases.expected(name, **dict(params, exact=1))  # (shared with the exact-mode tests of the process)
    return map_cigar_oracle.cigar_run(t, q, exact_result=exact, **exact["params"])


def expected(name, **params):
    """the restatement's cigar-mode result for an input of mapcases (or slab_link)"""
    return _expected(name, tuple(sorted(params.items())))


def params_of(name, **params):
    """the keywords of mapper.run for a case (the hand cases carry parameters of their own)"""
    if name in mapcases.HAND:
        params = dict(mapcases.hand_cases()[name][2], **params)
    if name.endswith("_ava"):
        params["ava"] = 1
    return dict(params, exact=1)
