"""The banded pair sweep of the chain kernels against the C oracle, every table bit for bit, under
the default dispatch, with the band off (MSGPU_NO_BAND), with every fast path off (MSGPU_NO_FASTPATH), a launch per width
class (MSGPU_CHAIN_SERIAL) and one edge per wavefront (MSGPU_NO_SUBWAVE), on the families of tests/bandcases.py -- rows that
need a predecessor outside the band, fp64 ties between a predecessor inside and one outside, chains along which the score
does not grow -- and on cfg3-shaped synthetic rows.  Each workload asserts through the band counters
(OverlapContext.chain_band_counts) that it holds what it claims: the adversarial edges of a banded class all fell back, the
synthetic sample on at most 2 % of its banded edges, and no edge took the band where a switch forbids it."""
import numpy as np
import pytest

import bandcases as K
from helpers import assert_tables_equal

pytestmark = pytest.mark.gpu

ENVS = [None, "MSGPU_NO_BAND", "MSGPU_NO_FASTPATH", "MSGPU_CHAIN_SERIAL", "MSGPU_NO_SUBWAVE"]
# the classes whose kernel has the band: k_chain -- the edges of 33..64 EdgeMatches, and every edge of at most 64 with one edge
# per wavefront (MSGPU_NO_SUBWAVE); an edge is banded when it has more than B + 1 rows (and the shortcut did not take it)
K_CHAIN_MIN = 33


def _run(rows, monkeypatch, env):
    from muchsalsa_amd import overlap
    if env:
        monkeypatch.setenv(env, "1")
    with overlap.OverlapContext(0) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables(), ctx.counts(), ctx.chain_band_counts(), ctx.chain_band_width()


def _banded_class(n, B, env):
    if env in ("MSGPU_NO_BAND", "MSGPU_NO_FASTPATH"):
        return False
    return B + 1 < n <= 64 and (n >= K_CHAIN_MIN or env == "MSGPU_NO_SUBWAVE")


def _band():
    from muchsalsa_amd import _lib
    return int(_lib.lib().msgpu_chain_band_width())


@pytest.mark.parametrize("env", ENVS, ids=lambda e: e or "default")
@pytest.mark.parametrize("family", ["gap", "tie", "flat"])
def test_adversarial(oracle, monkeypatch, family, env):
    B = _band()
    rows, ns = {"gap": K.gap_rows, "tie": lambda b: K.tie_rows(b)[:2], "flat": K.flat_rows}[family](B)
    want = oracle.overlap(rows)
    assert [int(c) for c in want["edges"]["em_cnt"]] == ns, "an EdgeMatch per anchor, an edge per pair of reads"
    got, counts, (n_band, n_fb), width = _run(rows, monkeypatch, env)
    assert width == B
    assert_tables_equal(got, want, "%s, %s" % (family, env or "default"))
    assert counts.n_edges_fastpath == 0, "no edge of these families is all-pairs-compatible"
    expect = sum(1 for n in ns if _banded_class(n, B, env))
    print("%s %s: B = %d, %d edges, %d banded, %d fell back" % (family, env or "default", B, len(ns), n_band, n_fb))
    assert n_band == expect
    if family in ("gap", "tie"):
        assert n_fb == n_band, "every gap / tie edge of a banded class is done again with the full sweep"
        if env in (None, "MSGPU_CHAIN_SERIAL", "MSGPU_NO_SUBWAVE"):
            assert n_band > 0
    else:
        # zero scores never pass the strict <; the absorbed score is rejected at the rows behind the tiny anchor when it
        # lies outside their band -- at least the zero-score half falls back
        assert n_band // 2 <= n_fb <= n_band


@pytest.mark.parametrize("env", ENVS, ids=lambda e: e or "default")
def test_synthetic_sample(oracle, monkeypatch, env):
    from muchsalsa_amd import synth
    B = _band()
    rows = synth.synth_rows(300, 10_000, 1500, 7)
    want = oracle.overlap(rows)
    got, counts, (n_band, n_fb), _ = _run(rows, monkeypatch, env)
    assert_tables_equal(got, want, "synthetic, %s" % (env or "default"))
    cnt = want["edges"]["em_cnt"]
    cls = int(np.count_nonzero([_banded_class(int(n), B, env) for n in cnt]))
    print("synthetic %s: B = %d, %d edges of a banded class, %d shortcut, %d banded, %d fell back" % (
        env or "default", B, cls, counts.n_edges_fastpath, n_band, n_fb))
    if env in ("MSGPU_NO_BAND", "MSGPU_NO_FASTPATH"):
        assert (n_band, n_fb) == (0, 0)
    else:
        assert 0 < n_band <= cls and n_band >= cls - counts.n_edges_fastpath
        assert n_fb <= 0.02 * n_band, "the fallback pays both sweeps: at most 2 % of the banded edges"
