"""Inputs of the end-extension tests (rule 11), shared by the host and the GPU files: the flank pairs of msgpu_extend_ends
(every one is a function of fixed seeds), the mapper cases, and the restatement's result for each, computed once per process
(tests/map_extend_oracle.py on top of the cigar-mode results that tests/cigarcases.py caches)."""
import functools
import os

import numpy as np

import cigarcases
import map_extend_oracle as xo
import map_oracle
import mapcases

ALPHA = cigarcases.ALPHA
BANDS = (8, 31, 32, 64, 127)  # both table classes and both sides of ES_LDS_MAXD = 31
IDENTICAL = (0, 1, 7, 8, 9, 15, 16, 17, 511, 512, 513, 1030)  # match_run8's widths; the wide slide's 512 once and twice


def _sub(s, pos):
    s = bytearray(s)
    s[pos] = b"ACGT"[(b"ACGT".index(s[pos]) + 1) % 4]
    return bytes(s)


@functools.lru_cache(maxsize=None)
def hand_pairs(band):
    """the hand-made flank pairs (A, B) for a band, in the flank's own order; the first and the last have odd lengths, so that
    in a buffer that holds the pairs one behind the other no later offset is a multiple of 8 by design"""
    rng = np.random.default_rng(1100 + band)
    g = bytes(rng.choice(ALPHA, 3000))
    h = bytes(rng.choice(ALPHA, 2000))
    pairs = [(g[:13], g[:11])]
    pairs += [(g[:n], g[:n]) for n in IDENTICAL]
    pairs += [(g[:100], g[:60]), (g[:60], g[:100]), (g[:9], g[:300]), (g[:300], g[:9]), (b"", g[:50]), (g[:50], b""), (b"", b"")]
    base = g[:200]
    for pos in (0, 100, 199):  # one edit of each kind at byte 0, in the middle and as the last byte
        pairs.append((base, _sub(base, pos)))
        pairs.append((base, base[:pos] + base[pos + 1:]))
        pairs.append((base, base[:pos] + b"G" + base[pos:]))
        pairs.append((base[:pos] + base[pos + 1:], base))
    if band >= 70:  # an indel of `gap` bases and 700 matching bytes behind it: end cells either side of the lane 63 / 64 seam
        for gap in (63, 64, 65, 70):
            pairs.append((g[:40] + h[:gap] + g[40:740], g[:740]))
            pairs.append((g[:740], g[:40] + h[:gap] + g[40:740]))
    for edits in (band, band + 1):  # an end cell in row `band` exactly, and one that would need row band + 1
        a = g[:20 * edits + 20]
        b = a
        for i in range(edits):
            b = _sub(b, 10 + 20 * i)
        pairs.append((a, b))
    pairs.append((g[:300], h[:300]))  # two random flanks: every row runs, the extension is a few bytes at most
    pairs.append((g[300:450] + g[1000:1150], g[300:450] + h[1000:1150]))  # 150 good bytes, then random ones
    pairs.append((g[5:26], g[5:24]))
    return tuple(pairs)


RANDOM = ((1500, 16, 91), (500, 40, 92))  # (pairs, band, seed): 2,000 pairs at 0-20 % edits, either table class


@functools.lru_cache(maxsize=None)
def random_pairs(which):
    count, band, seed = RANDOM[which]
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(count):
        n = int(rng.integers(0, 260))
        a = bytes(rng.choice(ALPHA, n))
        b = cigarcases.mutate(rng, a, int(n * rng.uniform(0, 0.2)))
        cut = int(rng.integers(0, 4))
        if cut == 1:
            b = b[:int(rng.integers(0, len(b) + 1))]
        elif cut == 2:
            a = a[:int(rng.integers(0, len(a) + 1))]
        pairs.append((a, b))
    return tuple(pairs), band


@functools.lru_cache(maxsize=None)
def expected_pairs(key):
    """-> (ends, off, words) of the restatement for hand_pairs(band) (key = a band) or random_pairs(i) (key = ("random", i))"""
    pairs, band = (hand_pairs(key), key) if not isinstance(key, tuple) else random_pairs(key[1])
    ends, off, words = [], [0], []
    for a, b in pairs:
        end, w = xo.reach(a, b, band)
        xo.check_extension(a, b, end, w)
        ends.append(end)
        words += w
        off.append(len(words))
    return ends, off, words


def layout(pairs, reverse):
    """the two buffers that hold the flanks one behind the other without padding, and the descriptors: forward as they are;
    reversed as the bytes lie in a sequence (byte i of a flank at off - 1 - i), the offsets naming the byte behind the flank.
    The first flank starts at byte 0 of its buffer and the last one ends at the buffer's last byte either way."""
    a = b"".join(p[0][::-1] if reverse else p[0] for p in pairs)
    b = b"".join(p[1][::-1] if reverse else p[1] for p in pairs)
    desc, ao, bo = [], 0, 0
    for x, y in pairs:
        desc.append((ao + len(x), bo + len(y), len(x), len(y)) if reverse else (ao, bo, len(x), len(y)))
        ao += len(x)
        bo += len(y)
    return a, b, desc


# ---- the mapper with extend > 0

@functools.lru_cache(maxsize=None)
def ends_case():
    """chains at the ends of their sequences: queries that hang over the target's first and last byte (the extension must stop
    at target byte 0 / at the last byte), queries contained in the target whose flanks carry one edit of each kind near either
    end, and the reverse complement of each"""
    G = mapcases._g(4000, 47)
    t = G[100:1300]
    left, right = G[0:500], G[900:1400]  # overhang 100 at either end
    inner = G[300:1000]
    noisy = _sub(inner[:10] + inner[11:], 24)  # a deletion 10 bases from the start, a substitution behind it
    noisy = _sub(noisy[:-12] + b"T" + noisy[-12:], len(noisy) - 30)  # an insertion 12 bases from the end, a substitution before it
    qs = [(b"left", left), (b"right", right), (b"inner", inner), (b"noisy", noisy), (b"left_noisy", _sub(_sub(left, 80), 130))]
    qs += [(n + b"_rc", map_oracle.revcomp(s)) for n, s in list(qs)]
    return mapcases._fa([(b"t", t), (b"u", G[2000:2400])]), mapcases._fa(qs)


LARGEST = 65535  # MSGPU_MAP_EXTEND_MAX: longer than any record of the tests
CASES = ([("clean", {}, e) for e in (1, 16, 300, LARGEST)] + [("ends", {}, e) for e in (16, 300)] +
         [("perfect", {}, 300), ("reverse", {}, 300), ("two_chains", {}, 300)])


def write_inputs(name, directory):
    if name != "ends":
        return cigarcases.write_inputs(name, directory)
    t, q = ends_case()
    tp, qp = os.path.join(str(directory), "t.fa"), os.path.join(str(directory), "q.fa")
    for path, text in ((tp, t), (qp, q)):
        with open(path, "wb") as f:
            f.write(text)
    return tp, qp


def records(name):
    if name != "ends":
        return cigarcases.records(name)
    t, q = ends_case()
    return map_oracle.parse(t, False), map_oracle.parse(q, False)


@functools.lru_cache(maxsize=None)
def _cigar(name, params):
    if name != "ends":
        return cigarcases.expected(name, **dict(params))
    import map_cigar_oracle
    t, q = records(name)
    return map_cigar_oracle.cigar_run(t, q, **dict(dict(params), exact=1))


@functools.lru_cache(maxsize=None)
def _expected(name, params, extend):
    t, q = records(name)
    return xo.extend_run(t, q, extend, cigar_result=_cigar(name, params))


def expected(name, extend, **params):
    """the restatement's result for an input of cigarcases (or ``ends``) with extend"""
    return _expected(name, tuple(sorted(params.items())), extend)


def params_of(name, **params):
    return dict(params, exact=1) if name == "ends" else cigarcases.params_of(name, **params)
