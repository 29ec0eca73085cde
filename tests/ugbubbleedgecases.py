"""Edge inputs of the bubble popping tests (rule 9 of the short-read unitig assembly) aimed at k_ug_forks, k_ug_bubbles and the
phase loop, shared by the host file, the GPU file and the poisoned-arena file: the cases of
muchsalsa_amd.synth.unitig_bubble_edge_cases at every key width, the two inputs at the cap of the parameter, the tangled
workloads, the restatement's result for each (tests/ug_bubble_oracle.py, computed once per process), and the conditions the tests
rely on, checked on the restatement's result and its list of the bubbles found alone -- never on the GPU."""
import functools

import ug_bubble_oracle as bo
import ug_oracle
from ugbubblecases import flipped

KS = (15, 31, 32, 33, 63, 64)  # below, at and above one 64-bit word; at k = 32 the key mask is all ones; the last two words' ends
KS_EVEN = (16, 32, 64)         # a self-complementary k-mer exists for even k only
HAND = ("four_way", "two_pairs", "homopolymer", "blocked_lane", "blocked_fork", "second_phase", "limit_split", "near_tie_a",
        "near_tie_b", "tie_fwd", "tie_rev", "two_loops")
EVEN = ("selfcomp_fork", "selfcomp_merge", "hairpin_even")
CAP, K_CAP = ("cap_4096", "cap_4097"), 21
# name -> (k, genome, seed): at k = 9, 11, 12 the first two seeds from 1 on that meet tangle_conditions on the restatement.
# At k = 8 no seed from 1 to 2500 does: 1000 bases in four edited copies hold about 2200 distinct 8-mers, so each of the six
# other neighbours of a node is there by chance with probability 4400 / 4^8, four nodes in ten have one, and a simple branch of
# eight k-mers is rare; the restatement finds 0 to 9 bubbles.  The conditions on the bubbles and the rounds are therefore
# asserted at TANGLE_KS_CONDITIONS only.  The two seeds at k = 8 are the one with the most bubbles among those with three
# rounds (788: 9 bubbles) and the first with a branch of one k-mer and four bubbles (124); what is asserted of them is more than
# 256 forks, a bubble, and a second round
TANGLES = {"tangle-8-124": (8, 1000, 124), "tangle-8-788": (8, 1000, 788), "tangle-9-2": (9, 1500, 2), "tangle-9-3": (9, 1500, 3),
           "tangle-11-1": (11, 2000, 1), "tangle-11-2": (11, 2000, 2), "tangle-12-3": (12, 2000, 3), "tangle-12-4": (12, 2000, 4)}
TANGLE_KS_CONDITIONS = (9, 11, 12)
MIN_LENGTH = 100  # of the hand-made cases; the tangles are run at 0

HAND_AT = [(n, k) for k in KS for n in HAND] + [(n, k) for k in KS_EVEN for n in EVEN]
CAP_AT = [(n, K_CAP) for n in CAP]
TANGLE_AT = [(n, v[0]) for n, v in TANGLES.items()]
CASES = HAND_AT + CAP_AT + TANGLE_AT


def read_len(k):
    return 80 if k <= 33 else 140


@functools.lru_cache(maxsize=None)
def _hand(k):
    from muchsalsa_amd import synth
    return synth.unitig_bubble_edge_cases(k, read_len(k))


@functools.lru_cache(maxsize=None)
def _cap():
    from muchsalsa_amd import synth
    return synth.unitig_bubble_cap_cases(K_CAP)


@functools.lru_cache(maxsize=None)
def workload(name, k):
    """-> (the FASTQ file, what the case is made of)"""
    from muchsalsa_amd import synth
    if name in TANGLES:
        assert TANGLES[name][0] == k
        w = synth.unitig_tangle(*TANGLES[name])
    else:
        w = _cap()[name] if name in CAP else _hand(k)[name]
    return w[0], w[2]


def params(name, k):
    """-> dict(bubble, trim, min_length, min_count) the case is run with at k"""
    meta = workload(name, k)[1]
    return dict(bubble=meta["bubble"], trim=meta["trim"], min_length=0 if name in TANGLES else MIN_LENGTH,
                min_count=meta.get("min_count", 2))


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


def enc(seq):
    """a k-mer's string as the restatement's integer"""
    x = 0
    for b in seq:
        x = 4 * x + b"ACGT".index(b)
    return x


def branch_stats(name, k, brs):
    """-> [(sum of counts, length)] of the branches of a bubble found in the first round"""
    counts = plain(name, k)["counts"]
    return [(sum(counts[ug_oracle.canon(x, k)] for x in p), len(p)) for _, p in brs]


def limits(name, k):
    """limit_split: the values of ``bubble`` at its edge and whether each pops -- the longer branch's length pops, the
    shorter's and the longer's - 1 do not"""
    (_, _, brs, _), = [b for b in expected(name, k)[1][0] if b[3] is not None]
    short, long_ = sorted(len(p) for _, p in brs)
    return [(long_, True), (short, False), (long_ - 1, False)]


def runs(name, k):
    """the values of ``bubble`` a case is run at, one after the other on one context, and whether each pops (None: the case
    has one run, at its own parameter)"""
    if name == "limit_split":
        lim = limits(name, k)
        return [lim[0], lim[1], (3 * k, True), lim[2]]
    if name == "cap_4096":
        return [(4096, True), (4095, False), (4096, True)]
    if name == "cap_4097":
        return [(4096, False)]
    return [(params(name, k)["bubble"], None)]


def unpopped(name, k, r):
    """the result r is that of the run with rule 9 off"""
    off = plain(name, k)
    return not r["bubble_kmers"] and r["all"] == off["all"] and r["cut"] == off["cut"] and r["unitigs"] == off["unitigs"]


def tangle_conditions(r, k):
    """the conditions every tangled input meets -> list of those missed"""
    br, missed = r["bubble_rounds"], []
    if r["bubbles"] < (10 if k in TANGLE_KS_CONDITIONS else 1):
        missed.append("%d bubbles" % r["bubbles"])
    if len(br) < (3 if k in TANGLE_KS_CONDITIONS else 2):
        missed.append("%d bubble rounds" % len(br))
    if br[0][1] <= 256:
        missed.append("%d forks in the first round" % br[0][1])
    return missed


def meets_conditions(name, k):
    """-> list of the conditions missed (the issue's), for the workload ``name`` at k"""
    missed = []
    (on, found), meta = expected(name, k), workload(name, k)[1]
    br = on["bubble_rounds"]
    judged = [[b for b in rnd if b[3] is not None] for rnd in found]
    same = [b for rnd in found for b in rnd if b[3] is None]
    canon, rc = ug_oracle.canon, ug_oracle.rc
    if name in TANGLES:
        return tangle_conditions(on, k)
    if name == "four_way":
        if br[0][2:] != (1, 3, 3 * k) or len(br) != 2 or [len(b[2]) for b in judged[0]] != [4]:
            missed.append("not one bubble of four branches, three removed in one round: %r" % (br,))
    elif name == "two_pairs":
        if br[0][2:] != (2, 2, 2 * k) or {b[0] for b in judged[0]} != {enc(meta["fork"])}:
            missed.append("the first round does not judge two bubbles at one fork: %r" % (br,))
        elif {b[1] for b in judged[0]} != {enc(meta["merge"]), enc(meta["merge2"])}:
            missed.append("the merges are not the two of the construction")
        if len(br) != 3 or br[1][2:] != (1, 1, k + 5):
            missed.append("the second round does not pop the bubble of k + 5 between the winners: %r" % (br,))
    elif name == "homopolymer":
        if br[0][2:] != (1, 1, 1) or sorted(len(p) for b in judged[0] for _, p in b[2]) != [1, 2] or on["bubble_kmers"] != 1:
            missed.append("not one bubble of branches of 2 and 1 k-mers with one k-mer removed: %r" % (br,))
    elif name == "blocked_lane":
        if br[0][2:] != (1, 1, k) or len(br) != 2 or on["bubble_kmers"] != k:
            missed.append("not 1 bubble with 1 branch removed: %r" % (br,))
        elif [(b[0], b[1], len(b[2])) for b in judged[0]] != [(enc(meta["fork"]), enc(meta["merge"]), 2)]:
            missed.append("the bubble is not judged from the fork of three successors")
        if canon(enc(meta["blocked"]), k) not in on["counts"]:
            missed.append("the blocked branch is gone")
    elif name == "blocked_fork":
        if any(found) or not unpopped(name, k, on) or br[0][1] < 3:
            missed.append("a bubble is found, or fewer than three forks: %r" % (br,))
    elif name == "second_phase":
        z = next(i for i, r in enumerate(br) if not r[4])
        if on["bubble_phases"] != 2 or z + 1 >= len(br):
            missed.append("%d bubble phases" % on["bubble_phases"])
        elif not sum(r[4] for r in br[:z]) or not sum(r[4] for r in br[z + 1:]):
            missed.append("a phase removes nothing: %r" % (br,))
        elif not sum(n for _, n in on["rounds"][br[z][0]:br[z + 1][0]]):
            missed.append("no tip round between the phases removes anything")
    elif name == "limit_split":
        (long_, _), (short, _), (below, _) = limits(name, k)
        at = expected(name, k, bubble=long_)[0]
        if short == long_:
            missed.append("the branches have one length")
        if not at["bubble_kmers"] or at["all"] != on["all"]:
            missed.append("bubble = %d does not pop it" % long_)
        for b in (short, below):
            if not unpopped(name, k, expected(name, k, bubble=b)[0]):
                missed.append("bubble = %d changes something" % b)
    elif name in ("near_tie_a", "near_tie_b"):
        (u, t, brs, win), = judged[0]
        (sa, la), (sb, lb) = branch_stats(name, k, brs)
        if la == lb or not 0 < abs(sa * lb - sb * la) < min(la, lb):
            missed.append("products %d and %d, lengths %d and %d" % (sa * lb, sb * la, la, lb))
        if (len(brs[win][1]) == max(la, lb)) != (name == "near_tie_a"):
            missed.append("the %s branch wins" % ("shorter" if name == "near_tie_a" else "longer"))
    elif name in ("tie_fwd", "tie_rev"):
        (u, t, brs, win), = judged[0]
        (sa, la), (sb, lb) = branch_stats(name, k, brs)
        if sa * lb != sb * la or win != 0 or brs[0][0] > brs[1][0]:
            missed.append("no tie decided by the base")
        if (u == canon(u, k)) != (name == "tie_fwd"):
            missed.append("the judging fork lies on the %s strand" % ("other" if name == "tie_fwd" else "canonical"))
    elif name == "two_loops":
        if not any(b[0] == b[1] == enc(meta["fork"]) and len(b[2]) == 2 for b in same):
            missed.append("no bubble whose fork and merge are one oriented node")
        if not unpopped(name, k, on):
            missed.append("something is popped")
    elif name == "selfcomp_fork":
        if [(b[0], b[1]) for b in judged[0]] != [(enc(meta["fork"]), enc(meta["merge"]))] or rc(enc(meta["fork"]), k) != enc(meta["fork"]):
            missed.append("no bubble judged from a fork that is its own reverse complement")
        if br[0][1:] != (2, 1, 1, k):
            missed.append("the forks are not the self-complementary one, once, and the merge's mirror: %r" % (br,))
    elif name == "selfcomp_merge":
        if [(b[0], b[1]) for b in judged[0]] != [(enc(meta["fork"]), enc(meta["merge"]))] or rc(enc(meta["merge"]), k) != enc(meta["merge"]):
            missed.append("no bubble judged whose merge is its own reverse complement")
        if br[0][2:] != (1, 1, k):
            missed.append("not popped: %r" % (br,))
    elif name == "hairpin_even":
        if not any(canon(b[0], k) == canon(b[1], k) and len(b[2]) == 2 and all(any(x == rc(x, k) for x in p) for _, p in b[2])
                   for b in same):
            missed.append("no bubble of one k-mer as fork and merge with a self-complementary k-mer inside each branch")
        if not unpopped(name, k, on):
            missed.append("something is popped")
    elif name == "cap_4096":
        if br[0][2:] != (1, 1, 4096) or [len(p) for _, p in judged[0][0][2]] != [4096, 4096]:
            missed.append("bubble = 4096 does not pop two branches of 4096: %r" % (br,))
        if not unpopped(name, k, expected(name, k, bubble=4095)[0]):
            missed.append("bubble = 4095 changes something")
    elif name == "cap_4097":
        if not unpopped(name, k, on):
            missed.append("bubble = 4096 changes something")
        beyond = []  # the round itself, past the parameter's cap: the branches are there, and one k-mer too long
        bo.bubble_round(plain(name, k)["counts"], k, 4097, beyond)
        if [[len(p) for _, p in b[2]] for b in beyond if b[3] is not None] != [[4097, 4097]]:
            missed.append("no two branches of 4097")
    return missed
