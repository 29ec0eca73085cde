"""Workloads of the bubble popping tests (rule 9 of the short-read unitig assembly), shared by the host and the GPU file: the
diploid workload and the hand-made cases (muchsalsa_amd.synth), the restatement's result for each (tests/ug_bubble_oracle.py,
computed once per process), and the conditions the tests rely on, checked on the restatement's result alone."""
import functools

import ug_bubble_oracle as bo
import ug_oracle

DIPLOID = ("diploid", "diploid_err")  # sequencing error 0 and 0.004 per base
KS_DIPLOID = (15, 31, 32, 33, 64)
KS_CONDITIONS = (15, 31, 32, 33)  # at k = 64 a 100-base read holds 37 k-mers: too few of them are solid for the conditions
HAND = ("edge", "indel_long", "indel_short", "tie", "three_way", "nested", "overlapped", "palindrome", "alternate")
K_HAND = 21
HAND_33 = HAND  # every hand-made case runs at k = 33 (the first 128-bit keys) and at k = 32 (the key mask is all ones) as well
KS_HAND = (K_HAND, 33, 32)
HAND_AT = [(n, k) for k in KS_HAND for n in HAND]
# every condition of meets_conditions holds at the three k.  indel_short needs reads of k + 100 bases above k = 21 for "the
# sum and the mean disagree" (synth.unitig_bubble_cases says why); every haplotype written once is solid in 80-base reads
MIN_LENGTH = 100  # of the hand-made cases


@functools.lru_cache(maxsize=None)
def _hand(k):
    from muchsalsa_amd import synth
    return synth.unitig_bubble_cases(k)


@functools.lru_cache(maxsize=None)
def workload(name, k=K_HAND):
    """-> (the FASTQ file, what the case is made of); the hand-made cases are laid out for their k"""
    from muchsalsa_amd import synth
    if name in DIPLOID:
        w = synth.diploid_workload(error=0.004 if name == "diploid_err" else 0.0)
    else:
        w = _hand(k)[name]
    return w[0], w[2]


def params(name, k):
    """-> dict(bubble, trim, min_length) the case is run with at k"""
    if name in DIPLOID:
        return dict(bubble=3 * k, trim=k, min_length=500)
    meta = workload(name, k)[1]
    return dict(bubble=meta["bubble"], trim=meta["trim"], min_length=MIN_LENGTH)


def flipped(data):
    """the FASTQ file with every read reverse-complemented"""
    comp = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
    lines = data.split(b"\n")
    for i in range(1, len(lines), 4):
        lines[i] = lines[i][::-1].translate(comp)
    return b"\n".join(lines)


@functools.lru_cache(maxsize=None)
def expected(name, k, bubble=None, flip=False):
    """the restatement on the workload, at the case's own parameters (``bubble`` overrides the case's) -> (result, the
    bubbles found per bubble round)"""
    p = params(name, k)
    if bubble is not None:
        p["bubble"] = bubble
    data = workload(name, k)[0]
    found = []
    r = bo.run(k, [flipped(data) if flip else data], found=found, **p)
    return r, found


def plain(name, k):
    """the restatement with rule 9 off"""
    return expected(name, k, bubble=0)[0]


def meets_conditions(name, k):
    """-> list of the conditions missed (the issue's), for the workload ``name`` at k"""
    missed = []
    (on, found), off = expected(name, k), plain(name, k)
    br, n_on, n_off = on["bubble_rounds"], len(on["unitigs"]), len(off["unitigs"])
    judged = [[b for b in rnd if b[3] is not None] for rnd in found]
    if name in DIPLOID:
        if br[0][2] < 10:
            missed.append("%d bubbles in the first bubble round" % br[0][2])
        if not any(len({len(p) for _, p in b[2]}) > 1 for b in judged[0]):
            missed.append("no bubble whose branches differ in length")
        if 4 * n_on > n_off:
            missed.append("%d unitigs with popping, %d without" % (n_on, n_off))
        if on["longest"] < 5 * off["longest"]:
            missed.append("longest %d with popping, %d without" % (on["longest"], off["longest"]))
    elif name == "edge":
        low = expected(name, k, bubble=k - 1)[0]
        if (br[0][2:], n_off, n_on) != ((1, 1, k), 4, 1):
            missed.append("bubble = 3k: %r, %d -> %d unitigs" % (br, n_off, n_on))
        at_k = expected(name, k, bubble=k)[0]
        if at_k["all"] != on["all"] or at_k["bubble_rounds"][0][2:] != (1, 1, k):
            missed.append("bubble = k does not pop it")
        if low["all"] != off["all"] or low["bubble_kmers"] or low["rounds"] != off["rounds"]:
            missed.append("bubble = k - 1 changes something")
    elif name in ("indel_long", "indel_short"):
        (u, t, brs, win), = judged[0]
        counts = expected(name, k, bubble=0)[0]["counts"]
        stats = [(sum(counts[ug_oracle.canon(x, k)] for x in p), len(p)) for _, p in brs]
        longer = max(range(2), key=lambda i: stats[i][1])
        by_sum = max(range(2), key=lambda i: stats[i][0])
        if stats[0][1] == stats[1][1]:
            missed.append("the branches have one length")
        if (win == longer) != (name == "indel_long"):
            missed.append("the %s branch wins" % ("shorter" if name == "indel_long" else "longer"))
        if name == "indel_short" and by_sum == win:
            missed.append("the sum and the mean agree")
        if n_on != 1:
            missed.append("%d unitigs" % n_on)
    elif name == "tie":
        (u, t, brs, win), = judged[0]
        counts = plain(name, k)["counts"]
        a, b = [(sum(counts[ug_oracle.canon(x, k)] for x in p), len(p)) for _, p in brs]
        if a[0] * b[1] != b[0] * a[1] or win != 0 or brs[0][0] > brs[1][0]:
            missed.append("no tie decided by the base")
    elif name == "three_way":
        if br[0][2:4] != (1, 2) or len(br) != 2:
            missed.append("not one bubble with two branches removed in one round: %r" % (br,))
    elif name == "nested":
        if not any(r[4] for r in br[1:]):
            missed.append("no bubble round after the first removes anything")
        if [r[4] for r in br] != [k, k + 12, 0]:
            missed.append("rounds remove %r" % [r[4] for r in br])
    elif name == "overlapped":
        if on["bubble_kmers"] or n_on != n_off or on["all"] != off["all"]:
            missed.append("something is popped")
        if br[0][1] < 2:
            missed.append("no forks")
    elif name == "palindrome":
        same = [b for rnd in found for b in rnd if b[3] is None]
        if not same or not all(len(b[2]) >= 2 and ug_oracle.canon(b[0], k) == ug_oracle.canon(b[1], k) for b in same):
            missed.append("no bubble whose fork and merge are one k-mer")
        if on["bubble_kmers"] or on["all"] != off["all"]:
            missed.append("something is popped")
    elif name == "alternate":
        first_phase_end = next(i for i, r in enumerate(br) if not r[4])
        after = br[first_phase_end][0]
        if not any(rem for _, rem in on["rounds"][after:]):
            missed.append("no tip round after the first bubble phase removes anything")
        if on["bubble_phases"] != 2 or br[-1][4] or br[-1][0] <= after:
            missed.append("no final bubble phase that removes nothing")
    return missed
