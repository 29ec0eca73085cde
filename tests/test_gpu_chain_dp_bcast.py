"""The chaining DP of k_chain with population[k] broadcast through the LDS crossbar ("The DP's
broadcast"), and the one-instruction minimum of nano_check<WF = true>, against the C oracle: all four tables bit for bit.

The DP takes its steps eight at a time (the source lane of a step is an address register plus an immediate), reloads the
reversed compatibility word at step 32 and stops inside a group of eight wherever n - 1 is no multiple of 8.  So: n = 1 (no
step), 2 (one step), B + 1 and B + 2 (the band's threshold) with one edge per wavefront (MSGPU_NO_SUBWAVE sends them to
k_chain); n = 33, 34 (the first step with k >= 32, and the reload), 63, 64 (the last lane) in the default dispatch; band
fallbacks (the second pass starts from the EdgeMatch scores, not from the first pass's populations); ties and zero scores
(cand == pop takes no update); a chain in which every row takes its predecessor l - 1 (the score a step writes is the one
the next step reads); twelve edges of different n in one launch.  With the band off and with every fast path off as well.

For the minimum: edges whose anchors are nested in their neighbour or start where it starts on one read, against ordered
anchors on the other (orientation 0 on one vertex: neither pos nor neg, the lanes where min and select may differ)."""
import numpy as np
import pytest

import bandcases as K
import extremecases as X
from helpers import assert_tables_equal
from test_gpu_chain_classes import _check, _rows
from muchsalsa_amd.synth import ROW_DTYPE

pytestmark = pytest.mark.gpu

KINDS = ("clean", "mixed", "both")
ENVS = [None, "MSGPU_NO_BAND", "MSGPU_NO_FASTPATH"]


def _band():
    from muchsalsa_amd import _lib
    return int(_lib.lib().msgpu_chain_band_width())


def _setenv(monkeypatch, *envs):
    for e in envs:
        if e:
            monkeypatch.setenv(e, "1")


def _run_counts(rows):
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables(), ctx.counts(), ctx.chain_band_counts()


@pytest.mark.parametrize("env", ENVS, ids=lambda e: e or "default")
@pytest.mark.parametrize("kind", KINDS)
def test_one_edge_per_wavefront(oracle, monkeypatch, env, kind):
    """n = 1, 2, B + 1, B + 2 in k_chain: no step, one step, the last edge without the band and the first with it"""
    B = _band()
    _setenv(monkeypatch, "MSGPU_NO_SUBWAVE", env)
    specs = [(n, kind) for n in (1, 2, B + 1, B + 2) for _ in range(3)]
    _check(oracle, _rows(specs, 31), [n for n, _ in specs], "subwave off, %s/%s" % (kind, env))


@pytest.mark.parametrize("env", ENVS, ids=lambda e: e or "default")
@pytest.mark.parametrize("kind", KINDS)
def test_default_dispatch(oracle, monkeypatch, env, kind):
    """n = 33, 34 (step 32 and the reload of the reversed word), 63, 64 (the last lane as a source and as a row)"""
    _setenv(monkeypatch, env)
    specs = [(n, kind) for n in (33, 34, 63, 64) for _ in range(3)]
    want = _check(oracle, _rows(specs, 37), [n for n, _ in specs], "%s/%s" % (kind, env))
    if kind != "both":  # (two strands share the anchors between them)
        assert (want["orders"]["ids_cnt"] > 32).any(), "some path has more than 32 anchors: it crosses step 32"


@pytest.mark.parametrize("family", ["gap", "tie"])
def test_fallback_starts_afresh(oracle, family):
    """gap and tie edges at n = 40 and 64: every edge takes the band, is rejected and done again with the full table -- from the
    EdgeMatch scores, whatever the first pass left in the lanes"""
    B = _band()
    rows, ns = {"gap": K.gap_rows, "tie": lambda b, s: K.tie_rows(b, s)[:2]}[family](B, [40, 64])
    want = oracle.overlap(rows)
    assert [int(c) for c in want["edges"]["em_cnt"]] == ns
    got, counts, (n_band, n_fb) = _run_counts(rows)
    assert_tables_equal(got, want, family)
    assert counts.n_edges_fastpath == 0
    assert n_band == len(ns) and n_fb == n_band, "every edge fell back"


@pytest.fixture(scope="module")
def ties(oracle):
    """the reference's tables of the tie workload, computed once: (rows, tables)"""
    rows = X.ties_rows(5, (2, 9, 33, 40, 64))
    want = oracle.overlap(rows)
    pops = X.dp_populations(rows, want)
    assert any(t for _, _, _, t in pops), "some row has two predecessors with the same candidate score"
    assert any(all(p == 0.0 for p in pop) for _, _, pop, _ in pops), "some edge has zero scores only"
    return rows, want


@pytest.mark.parametrize("env", [None, "MSGPU_NO_SUBWAVE", "MSGPU_NO_BAND", "MSGPU_NO_FASTPATH"], ids=lambda e: e or "default")
def test_ties_and_zero_scores(ties, monkeypatch, env):
    """equal scores with twin predecessors and all-zero scores: cand == pop is no update, the first k keeps the row"""
    _setenv(monkeypatch, env)
    rows, want = ties
    got, _, _ = _run_counts(rows)
    assert_tables_equal(got, want, "ties/%s" % env)


@pytest.mark.parametrize("env", [None, "MSGPU_NO_FASTPATH", "MSGPU_NO_SUBWAVE"], ids=lambda e: e or "default")
def test_every_row_takes_its_neighbour(oracle, monkeypatch, env):
    """a chain with every pair compatible and every score positive: row l takes l - 1 in step l - 1, the step after the one
    that wrote population[l - 1] -- the path of the last row holds every anchor"""
    _setenv(monkeypatch, env)
    sizes = [64, 47, 33, 9]
    want = _check(oracle, _rows([(n, "clean") for n in sizes], 41), sizes, "neighbour/%s" % env)
    assert sorted(int(c) for c in want["orders"]["ids_cnt"]) == sorted(sizes)


@pytest.mark.parametrize("env", ENVS, ids=lambda e: e or "default")
def test_twelve_edges_one_launch(oracle, monkeypatch, env):
    """twelve edges of different n in one launch of k_chain: every remainder of n - 1 by eight, both sides of step 32"""
    _setenv(monkeypatch, "MSGPU_NO_SUBWAVE", env)
    sizes = [1, 2, 3, 5, 9, 14, 17, 31, 36, 40, 57, 64]
    specs = [(n, KINDS[i % 3]) for i, n in enumerate(sizes)]
    _check(oracle, _rows(specs, 43), sizes, "twelve/%s" % env)


def _nested_rows(n, nested_on):
    """one edge of n anchors: an ordered chain on one read; on the other (`nested_on`: 0 or 1) every fourth anchor lies
    inside its predecessor's range and every fourth starts where its predecessor starts and ends behind it"""
    L = 4000 + 800 * n
    out = []
    prev = None
    for j in range(n):
        a = [500 + 800 * j, 500 + 800 * j + 599]
        b = [700 + 800 * j, 700 + 800 * j + 599]
        if prev is not None and j % 4 == 1:
            b = [prev[0] + 100, prev[1] - 150]  # nested
        elif prev is not None and j % 4 == 3:
            b = [prev[0], prev[1] + 200]  # equal start
        prev = b
        r0, r1 = (b, a) if nested_on == 0 else (a, b)
        out.append(K.row(j, 0, L, 0, 599, r0[0], r0[1], 560, 2 * j, True))
        out.append(K.row(j, 1, L, 0, 599, r1[0], r1[1], 540, 2 * j + 1, True))
    return np.array(out, dtype=ROW_DTYPE)


@pytest.mark.parametrize("env", [None, "MSGPU_NO_SUBWAVE"], ids=lambda e: e or "default")
@pytest.mark.parametrize("nested_on", [0, 1])
@pytest.mark.parametrize("n", [5, 20, 40])
def test_nested_and_equal_start(oracle, monkeypatch, n, nested_on, env):
    _setenv(monkeypatch, env)
    rows = _nested_rows(n, nested_on)
    want = oracle.overlap(rows)
    assert [int(c) for c in want["edges"]["em_cnt"]] == [n]
    got, counts, _ = _run_counts(rows)
    assert_tables_equal(got, want, "nested on read %d, n = %d, %s" % (nested_on, n, env))
    assert counts.n_edges_fastpath == 0, "a nested anchor keeps the shortcut away: the pair sweep decides"
    # the nested anchors are off the chain of their neighbours: no path holds every anchor
    assert int(want["orders"]["ids_cnt"].max()) < n
