"""The overlap context gives back what it took: a context created, used on every path that allocates, and closed leaves no
device memory behind, and closing one that runs on a caller's stream leaves that stream usable."""
import numpy as np
import pytest

from helpers import assert_tables_equal

pytestmark = pytest.mark.gpu

SHAPE = (300, 3000, 900, 1)  # about 3 k edges: the smallest shape the suite runs on every path


@pytest.fixture(scope="module")
def job(oracle):
    from muchsalsa_amd import synth
    rows = synth.synth_rows(*SHAPE)
    shuffled = rows.copy()
    np.random.default_rng(5).shuffle(shuffled)
    want = oracle.overlap(rows)
    return rows, shuffled, want, oracle.find_contraction_edges(want, len(want["read_len"]))


def _three_calls(ctx, rows):
    ctx.load_rows(rows)
    ctx.calculate_edges()
    ctx.chaining_and_overlaps()


def _cycle(monkeypatch, job):
    """contexts created, used and closed in each of three ways, and one closed unused"""
    from muchsalsa_amd import overlap
    rows, shuffled, want, want_co = job
    for name in ("MSGPU_NO_BIN", "MSGPU_SYNC_READBACK"):
        monkeypatch.delenv(name, raising=False)
    overlap.OverlapContext(0).close()  # some handles were never made, the ring of chain-kernel events is empty
    with overlap.OverlapContext(0) as ctx:
        _three_calls(ctx, rows)
        assert_tables_equal(ctx.tables(), want, "three calls")
        last = len(want["edges"]) - 1
        off, ems = ctx.get_edgematches([0, last])
        e = want["edges"]
        assert ems.tobytes() == (want["ems"][: int(e["em_cnt"][0])].tobytes() +
                                 want["ems"][int(e["em_off"][last]): int(e["em_off"][last]) + int(e["em_cnt"][last])].tobytes())
        assert np.array_equal(ctx.find_contraction_edges(), want_co)
        lean, _ = ctx.overlap_batched(rows, 3, resident=True, edgematches=False)  # the wire form, its blocks, the unpacker
        assert lean["ems"] is None
        assert_tables_equal(dict(lean, ems=ctx.tables()["ems"]), want, "resident dispatcher")
        got, _ = ctx.overlap_batched(rows, 3)  # the two table sets swapped an odd number of times: closed with them swapped
        assert_tables_equal(got, want, "three windows")
        assert ctx.counts().n_lost_publications == 0
    monkeypatch.setenv("MSGPU_NO_BIN", "1")  # the atomic path, generic scaffolds: a second read-back in the index build
    with overlap.OverlapContext(0) as ctx:
        _three_calls(ctx, shuffled)
        assert_tables_equal(ctx.tables(), want, "atomic path, shuffled")
        assert ctx.counts().n_lost_publications == 0
    monkeypatch.delenv("MSGPU_NO_BIN")
    monkeypatch.setenv("MSGPU_SYNC_READBACK", "1")
    with overlap.OverlapContext(0) as ctx:
        _three_calls(ctx, rows)
        assert_tables_equal(ctx.tables(), want, "copy read-back")
    monkeypatch.delenv("MSGPU_SYNC_READBACK")


def test_no_device_memory_is_lost(job, monkeypatch):
    import torch
    _cycle(monkeypatch, job)  # warm-up: the runtime's pools, the kernels' code objects
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(2):
        _cycle(monkeypatch, job)
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print("free device memory: %d bytes before the first create, %d after the last destroy" % (before, after))
    assert after >= before


def test_destroy_leaves_the_callers_stream_alone(job):
    import torch
    from muchsalsa_amd import overlap
    rows, _, want, _ = job
    stream = torch.cuda.Stream(0)
    ctx = overlap.OverlapContext(0)
    ctx.set_stream(stream.cuda_stream)
    assert ctx.stream() == stream.cuda_stream
    _three_calls(ctx, rows)
    assert_tables_equal(ctx.tables(), want, "on the caller's stream")
    assert ctx.counts().n_lost_publications == 0
    ctx.close()  # with the caller's stream still set
    with torch.cuda.stream(stream):
        total = (torch.arange(1000, device="cuda:0", dtype=torch.int64) * 2).sum()
    stream.synchronize()
    assert int(total) == 999000
