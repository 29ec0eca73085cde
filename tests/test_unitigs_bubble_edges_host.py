"""The edge inputs of bubble popping (rule 9), host side (no GPU): every case of tests/ugbubbleedgecases.py meets the conditions
the GPU tests rely on, judged on the plain-Python restatement (tests/ug_bubble_oracle.py) alone; the restatement's own
assertions (no k-mer in two branches, no winner removed) hold on every one of them, the tangled inputs included; an input with
every read reverse-complemented gives the same result; and three verdicts are derived here by hand, from the strings the cases
are made of, without the restatement's comparison."""
import pytest

import ug_oracle
import ugbubbleedgecases as cases
from test_unitigs_bubbles_host import _invariants

P = 200  # the site of the hand-made cases
COMP = bytes.maketrans(b"ACGT", b"TGCA")


def _rc(seq):
    return seq[::-1].translate(COMP)


def _left(name, k):
    """the canonical k-mers that rule 9 removed, and those that are left"""
    on, off = cases.expected(name, k)[0], cases.plain(name, k)
    tips = sum(n for _, n in on["rounds"]) - sum(n for _, n in off["rounds"])
    assert tips == 0 and len(off["counts"]) - len(on["counts"]) == on["bubble_kmers"]
    return set(off["counts"]) - set(on["counts"]), set(on["counts"])


def _over_site(seq, k, at=P):
    """the canonical k-mers of seq that hold its base ``at``"""
    return {ug_oracle.canon(cases.enc(seq[i:i + k]), k) for i in range(at - k + 1, at + 1)}


@pytest.mark.parametrize("name,k", cases.CASES)
def test_cases_meet_their_conditions(name, k):
    """(the restatement's assertions are part of every run: an AssertionError here is rule 9's claim failing)"""
    assert cases.meets_conditions(name, k) == []


def test_the_tangles_meet_the_conditions_over_the_set():
    first_forks, lengths, widths = [], [], []
    for name, k in cases.TANGLE_AT:
        r, found = cases.expected(name, k)
        first_forks.append(r["bubble_rounds"][0][1])
        judged = [b for rnd in found for b in rnd if b[3] is not None]
        lengths += [len(p) for b in judged for _, p in b[2]]
        widths += [len(b[2]) for b in judged]
    assert any(f % 64 for f in first_forks), first_forks
    assert min(lengths) <= 2 and max(widths) >= 3
    print("forks in the first round %r, branches of %d to %d k-mers, %d bubbles of three or four branches" % (
        first_forks, min(lengths), max(lengths), sum(1 for w in widths if w >= 3)))


@pytest.mark.parametrize("name,k", cases.CASES)
def test_strand_symmetry(name, k):
    a, b = cases.expected(name, k)[0], cases.expected(name, k, flip=True)[0]
    assert a["all"] == b["all"] and a["cut"] == b["cut"]
    assert (a["rounds"], a["bubble_rounds"], a["unitigs"], a["bubble_phases"]) == (
        b["rounds"], b["bubble_rounds"], b["unitigs"], b["bubble_phases"])


@pytest.mark.parametrize("name,k", cases.CASES)
def test_restatement_invariants(name, k):
    _invariants(cases.expected(name, k)[0], cases.params(name, k)["min_length"])


def test_the_generators_are_deterministic():
    from muchsalsa_amd import synth
    assert synth.unitig_bubble_edge_cases(32, 80) == synth.unitig_bubble_edge_cases(32, 80)
    assert set(synth.unitig_bubble_edge_cases(33)) == set(cases.HAND)
    assert set(synth.unitig_bubble_edge_cases(16)) == set(cases.HAND + cases.EVEN)
    assert synth.unitig_tangle(8, 1000, 1) == synth.unitig_tangle(8, 1000, 1) != synth.unitig_tangle(8, 1000, 2)
    assert [k for _, k in cases.TANGLE_AT] == [8, 8, 9, 9, 11, 11, 12, 12] and set(cases.TANGLE_KS_CONDITIONS) == {9, 11, 12}


# ---- three verdicts by hand

@pytest.mark.parametrize("k", cases.KS)
def test_homopolymer_removes_the_one_kmer_over_the_shorter_run(k):
    """left + A (k - 1) + right x 3 beside left + A (k - 2) + right x 2: the only k-mer that the second sequence has alone
    is its last base of left, the k - 2 A and the first base of right; the first has two alone, each counted more often"""
    (long_, _), (short, _) = cases.workload("homopolymer", k)[1]["haplotypes"]
    own = short[199:199 + k]
    assert own[1:-1] == b"A" * (k - 2) and own[:1] != b"A" and own[-1:] != b"A"
    assert own not in long_ and _rc(own) not in long_
    gone, left = _left("homopolymer", k)
    assert gone == {ug_oracle.canon(cases.enc(own), k)}
    assert {ug_oracle.canon(cases.enc(long_[i:i + k]), k) for i in (199, 200)} <= left


@pytest.mark.parametrize("k", cases.KS)
def test_four_way_keeps_the_base_written_four_times(k):
    haps = cases.workload("four_way", k)[1]["haplotypes"]
    assert [m for _, m in haps] == [4, 3, 2, 2] and len({h[P] for h, _ in haps}) == 4
    gone, left = _left("four_way", k)
    assert _over_site(haps[0][0], k) <= left
    assert gone == set().union(*(_over_site(h, k) for h, _ in haps[1:])) and len(gone) == 3 * k


@pytest.mark.parametrize("k", cases.KS)
@pytest.mark.parametrize("name", ["tie_fwd", "tie_rev"])
def test_a_tie_keeps_the_smaller_base_on_the_judging_side(name, k):
    """both branches are counted alike.  The fork in front of the site is u, the merge behind it t; the side whose fork is
    the smaller string judges.  From u the branches are entered by the two bases at the site; from rc(t) by their
    complements, so there the greater base of the two stays"""
    (a, ma), (b, mb) = cases.workload(name, k)[1]["haplotypes"]
    assert ma == mb and a[:P] == b[:P] and a[P + 1:] == b[P + 1:] and a[P] != b[P]
    u, t = a[P - k:P], a[P + 1:P + 1 + k]
    if u < _rc(t):
        keep, drop = (a, b) if a[P] < b[P] else (b, a)
        judging = u
    else:
        keep, drop = (a, b) if a[P] > b[P] else (b, a)
        judging = _rc(t)
    assert (judging < _rc(judging)) == (name == "tie_fwd")  # the strand the stage stores the judging fork on
    gone, left = _left(name, k)
    assert gone == _over_site(drop, k) and _over_site(keep, k) <= left
