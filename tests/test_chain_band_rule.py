"""The band rule of the chain kernels stated in plain Python (bandcases.dp) over
ms_oracle_py.check_compatibility, no GPU: wherever the rule accepts an edge, the banded DP's scores and predecessors are
the full DP's; on cfg3-shaped synthetic rows the rule accepts at least 0.98 of the edges of either class above B + 1 rows
at the band width the library ships; and the adversarial families (bandcases) hold what they claim -- every gap, tie and
zero-score edge is rejected, and on the tie edges only the strict < does it."""
import pytest

import bandcases as K
from muchsalsa_amd import synth


def shipped_band():
    from muchsalsa_amd import _lib
    return int(_lib.lib().msgpu_chain_band_width())


def _edges(rows):
    mm = K.match_map(rows)
    for key in sorted(mm.edge_matches):
        ids, s, dirs = K.edge_lanes(mm, key)
        yield key, ids, s, dirs, mm


def _check(rows, B, min_rows=0):
    """-> [(n, accepted)] per edge of more than max(B + 1, min_rows - 1) rows; asserts the banded DP where the rule accepts"""
    out = []
    for key, ids, s, dirs, mm in _edges(rows):
        n = len(ids)
        if n <= B + 1 or n < min_rows:
            continue
        C = K.compat_matrix(mm, key, ids, dirs)
        pop_f, pred_f, _ = K.dp(C, s)
        pop_b, pred_b, ok = K.dp(C, s, B)
        if ok:
            assert [x.hex() for x in map(float, pop_b)] == [x.hex() for x in map(float, pop_f)], (key, B)
            assert pred_b == pred_f, (key, B)
        out.append((n, ok, pred_b == pred_f))
    return out


@pytest.mark.parametrize("B", [8, 12, 16])
def test_rule_is_exact_on_synthetic_rows(B):
    rows = synth.synth_rows(300, 10_000, 1500, 7)
    res = _check(rows, B, min_rows=17)
    assert len(res) > 1500


def test_accepted_share_at_the_shipped_band():
    B = shipped_band()
    rows = synth.synth_rows(300, 10_000, 1500, 7)
    res = _check(rows, B, min_rows=17)
    for lo, hi in ((17, 32), (33, 64)):
        cls = [ok for n, ok, _ in res if max(lo, B + 2) <= n <= hi]
        if not cls:
            continue
        share = sum(cls) / len(cls)
        print("class %d..%d: %d edges above B + 1 = %d rows, accepted share %.4f" % (lo, hi, len(cls), B + 1, share))
        assert len(cls) > 500
        assert share >= 0.98, (lo, hi, share)


@pytest.mark.parametrize("B", [8, 12, 16])
def test_adversarial_families(B):
    rows, ns = K.gap_rows(B)
    res = _check(rows, B)
    assert len(res) == len(ns) and not any(ok for _, ok, _ in res), "every gap edge is rejected"
    assert not any(same for _, _, same in res), "the band alone gives every gap edge a wrong predecessor"
    rows, ns, where = K.tie_rows(B)
    res = _check(rows, B)
    assert len(res) == len(ns) and not any(ok for _, ok, _ in res), "every tie edge is rejected"
    edges = list(_edges(rows))
    for (e, k_out, k_in, l), (key, ids, s, dirs, mm) in zip(where, edges):
        C = K.compat_matrix(mm, key, ids, dirs)
        pop, pred, _ = K.dp(C, s)
        pop_b, pred_b, _ = K.dp(C, s, B)
        assert C[k_out][l] and C[k_in][l] and pop[k_out] == pop[k_in] and k_out < l - B <= k_in
        assert pred[l] == k_out and pred_b[l] == k_in and pop_b == pop, "equal sums: only the predecessor differs"
        # with <= in place of < the rule would accept this edge: the tie is what rejects it
        pm = max(pop_b[: l - B])
        assert pm + s[l] == pop_b[l]
    rows, ns = K.flat_rows(B)
    res = _check(rows, B)
    assert len(res) == len(ns)
    assert not any(ok for (n, ok, _), i in zip(res, range(len(res))) if i % 2 == 0), "zero scores: pop never grows, never accepted"
