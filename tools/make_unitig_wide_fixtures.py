"""Record, under tests/golden/unitigs_wide/, the restatement's results above k = 64 (tests/ug_wide_oracle.py) for the hand-made
cases of tests/ugwidecases.py (rings, selfcomp, hairpin at k = 65, 96, 97, 128), as tools/make_unitig_fixtures.py does below it,
and ``key_vectors.txt``: what the operations of the multi-word key (csrc/msgpu_kmer_wide.h) must give, worked out on Python
integers, for tests/cpp/test_kmer_wide.cpp.  Run from the repository root: python tools/make_unitig_wide_fixtures.py

key_vectors.txt is lines of ``name value ...``; a number is hexadecimal, up to 64 digits (256 bits).  Per k a block:

    k K
    mask M
    ops X c succ pred down rc text Y lt eq
                              succ = ((X << 2) | c) & mask, pred = (X >> 2) | (c << top), down = X >> top, rc = the reverse
                              complement, text = X as bases; Y is another number, lt = X < Y, eq = X == Y
    roll SEQUENCE n           then n lines ``key K``: the canonical k-mer of every window of the sequence, in order
"""
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import kf_oracle  # noqa: E402
import ug_wide_oracle  # noqa: E402
import ugwidecases  # noqa: E402

KS_KEY = (65, 66, 95, 96, 97, 127, 128)


def record(name):
    k, files, params = ugwidecases.cases()[name]
    r = ugwidecases.expected(name)
    return {"case": name, "k": k, "min_count": 2, "trim": params.get("trim", k), "min_length": params["min_length"],
            "records": r["records"], "windows": r["windows"], "distinct": r["distinct"], "solid": r["solid"],
            "solid_after": r["solid_after"], "rounds": [list(x) for x in r["rounds"]], "cycles": r["cycles"], "alone": r["alone"],
            "blocked": r["blocked"], "unitigs": [[t[0], t[1], kf_oracle.kmer_text(t[2], k), t[3], t[4]] for t in r["unitigs"]],
            "all": r["all"].decode(), "cut": r["cut"].decode()}


def key_values(k, rnd):
    """2k-bit numbers aimed at the word boundaries: all ones, the top bit, and to either side of every boundary a single bit
    and a run of ones; then random ones"""
    bits = 2 * k
    full = (1 << bits) - 1
    out = [full, 1 << (bits - 1), 1]
    for edge in (64, 128, 192):
        if edge < bits:
            out += [1 << (edge - 1), 1 << edge, (1 << edge) - 1, full ^ ((1 << edge) - 1)]
    return out + [rnd.getrandbits(bits) for _ in range(4)]


def key_vectors():
    rnd = random.Random(20251)
    h = lambda x: "%x" % x  # noqa: E731
    lines = []
    for k in KS_KEY:
        mask, top = (1 << (2 * k)) - 1, 2 * (k - 1)
        lines += ["k %d" % k, "mask %s" % h(mask)]
        vals = key_values(k, rnd)
        for i, x in enumerate(vals):
            # the other number: the next value, the same, or this one with one bit flipped in the lowest, a middle or the top word
            y = (vals[(i + 1) % len(vals)], x, x ^ 1, x ^ (1 << 64), x ^ (1 << (2 * k - 1)), x ^ (1 << 127))[i % 6] & mask
            c = i & 3
            lines.append("ops %s %d %s %s %s %s %s %s %d %d" % (
                h(x), c, h(((x << 2) | c) & mask), h((x >> 2) | (c << top)), h(x >> top), h(ug_wide_oracle.rc_by_rule(x, k)),
                kf_oracle.kmer_text(x, k), h(y), x < y, x == y))
        seq = "".join(rnd.choice("ACGT") for _ in range(2 * k + 13))
        seq = seq[:k + 5] + "N" + seq[k + 6:k + 30].lower() + seq[k + 30:]  # a window broken by an N, lower case behind it
        keys = kf_oracle.canonical_kmers(seq.encode(), k)
        lines.append("roll %s %d" % (seq, len(keys)))
        lines += ["key %s" % h(x) for x in keys]
    return "\n".join(lines) + "\n"


def compact(d):
    """a JSON object with one key per line"""
    return "{\n" + ",\n".join(" %s: %s" % (json.dumps(k), json.dumps(v)) for k, v in d.items()) + "\n}\n"


if __name__ == "__main__":
    out = os.path.join(ROOT, "tests", "golden", "unitigs_wide")
    os.makedirs(out, exist_ok=True)
    for name in ugwidecases.names(ugwidecases.HAND):
        with open(os.path.join(out, name.replace("-", "_k") + ".json"), "w") as f:
            f.write(compact(record(name)))
    with open(os.path.join(out, "key_vectors.txt"), "w") as f:
        f.write(key_vectors())
