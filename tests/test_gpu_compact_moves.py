"""k_compact's moves -- the orders by slot of the chunk, the ids as one flat range, the edge record finished by the edge's own
thread -- and the chain kernels' hand-over of their counts in the edge record, at the smallest shapes where either can go wrong.
Hand-built row tables (compactcases.py) against the C oracle, all four tables bit for bit.  What each workload holds (chunks,
orders per edge, id runs and where they lie) is asserted without a GPU in test_compact_workloads.py."""
import pytest

import compactcases as CC
from helpers import assert_tables_equal

pytestmark = pytest.mark.gpu

CHAIN_ENVS = [None, "MSGPU_NO_SUBWAVE", "MSGPU_CHAIN_SERIAL", "MSGPU_NO_FASTPATH"]


@pytest.fixture(scope="module")
def jobs(oracle):
    """rows and the oracle's tables of a workload, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            rows = CC.WORKLOADS[name]()
            cache[name] = (rows, oracle.overlap(rows))
        return cache[name]
    return get


def _tables(ctx, rows):
    ctx.load_rows(rows)
    ctx.calculate_edges()
    ctx.chaining_and_overlaps()
    return ctx.tables()


def _run(rows):
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0) as ctx:
        return _tables(ctx, rows)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_edge_counts(jobs, n):
    """one chunk short of, exactly and just beyond 1024 edges; 2049: a chunk with two chunks before it.  A full chunk holds 1229
    orders: a second round of the order move"""
    rows, want = jobs("count_%d" % n)
    assert_tables_equal(_run(rows), want, "%d edges" % n)


@pytest.mark.parametrize("env", CHAIN_ENVS)
@pytest.mark.parametrize("name", ["runs", "mix"])
def test_runs_and_order_mix(jobs, monkeypatch, name, env):
    """runs: id runs of 1, 2, 63, 64, 65 and 70 (k_chain_big), runs across dword 64, across the copy's stride of 1024 and across
    its round of 8192.  mix: edges of one and of two orders in turn and in a row, two orders by both directions and by a kept
    alternative.  Each through every chain epilogue: the sub-wavefront kernels, k_chain alone, the classes one after the other,
    no shortcut"""
    if env:
        monkeypatch.setenv(env, "1")
    rows, want = jobs(name)
    assert_tables_equal(_run(rows), want, "%s/%s" % (name, env))


@pytest.mark.parametrize("name", ["count_2049", "mix"])
def test_shard_bases(jobs, name):
    """set_shard(1, 2): the second shard's tables are the oracle's cut to the edges it owns"""
    from muchsalsa_amd import distributed as D, overlap
    rows, want = jobs(name)
    with overlap.OverlapContext(0) as ctx:
        ctx.set_shard(1, 2)
        got = _tables(ctx, rows)
    assert_tables_equal(got, D.shard_view_host(want, 1, 2), "%s, shard 1 of 2" % name)


@pytest.mark.parametrize("name,n_batches", [("count_2049", 2), ("runs", 3), ("mix", 2)])
def test_window_bases(jobs, name, n_batches):
    """overlap_batched, resident: every window behind the first has non-zero bases in all four tables (out_em_base among them)"""
    from muchsalsa_amd import overlap
    rows, want = jobs(name)
    with overlap.OverlapContext(0) as ctx:
        got, _ = ctx.overlap_batched(rows, n_batches, resident=True)
        assert_tables_equal(got, want, "%s, %d windows" % (name, n_batches))
        assert_tables_equal(ctx.tables(), want, "%s, %d windows: the context's tables" % (name, n_batches))


def test_relaunch_and_direct_launch(jobs):
    """one context: a job of one edge; then 2049 edges, whose orders and ids do not fit what the first left -- the first launch of
    k_compact writes nothing (the edge records keep the chain kernels' counts) and the second moves; then the same job again and
    a smaller one, which fit: the first launch moves"""
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0) as ctx:
        for name in ("count_1", "count_2049", "count_2049", "mix", "runs", "count_1025"):
            rows, want = jobs(name)
            assert_tables_equal(_tables(ctx, rows), want, "one context: " + name)
        assert ctx.counts().n_lost_publications == 0


def test_sync_readback(jobs, monkeypatch):
    monkeypatch.setenv("MSGPU_SYNC_READBACK", "1")
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0) as ctx:
        for name in ("mix", "count_1025", "count_1025"):
            rows, want = jobs(name)
            assert_tables_equal(_tables(ctx, rows), want, "copy read-back: " + name)
