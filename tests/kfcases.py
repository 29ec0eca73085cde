"""Workloads of the k-mer abundance filter tests, shared by the host and the GPU file, and the restatement's result for
each (computed once per process)."""
import functools

import kf_oracle

SMALL = dict(genome=30000, coverage=30, read_len=100, seed=3, families=3, copies=8, repeat_len=400)
TINY = dict(genome=2000, coverage=6, read_len=50, seed=9, families=0, copies=0)  # k = 1 without a degenerate histogram
BIG = dict(genome=1000000, coverage=40, read_len=150, seed=5)  # 6 families x 25 copies x 1.5 kb, 0.5 % errors
KS_SMALL = (15, 21, 31, 32, 33, 50, 63, 64)  # and k = 1 on TINY
KS_BIG = (31, 50)


@functools.lru_cache(maxsize=None)
def workload(name):
    from muchsalsa_amd import synth
    if name == "poly_a":  # SMALL and 100 pairs of poly-A / poly-T: one k-mer with a count above 10000
        a, b = workload("small")
        extra = [b"".join(b"@a%d/%d\n%s\n+\n%s\n" % (i, m, base * 100, b"I" * 100) for i in range(100))
                 for m, base in ((1, b"A"), (2, b"T"))]
        return a + extra[0], b + extra[1]
    shape = {"small": SMALL, "tiny": TINY, "big": BIG}[name]
    return synth.kmer_filter_workload(**shape)


@functools.lru_cache(maxsize=None)
def expected(name, k):
    a, b = workload(name)
    return kf_oracle.run(k, a, b)


def meets_conditions(r):
    """what the GPU tests rely on, on the restatement's result alone -> list of the conditions missed"""
    missed = []
    share = sum(r["verdict"]) / max(r["pairs"], 1)
    if r["upper"] < 5:
        missed.append("upper %d < 5" % r["upper"])
    if not 0.05 <= share <= 0.60:
        missed.append("dropped share %.3f outside [0.05, 0.60]" % share)
    if not any(x and not y for x, y in zip(r["verdict1"], r["verdict2"])):
        missed.append("no pair dropped by mate 1 alone")
    if not any(y and not x for x, y in zip(r["verdict1"], r["verdict2"])):
        missed.append("no pair dropped by mate 2 alone")
    if not r["other_bytes"]:
        missed.append("no window broken by a non-ACGT byte")
    return missed
