"""The overlap context's edge inputs once more, on device memory that is poisoned and fenced: MSGPU_POISON is set for every
test of this file, so every buffer of the context (DevBuf, csrc/msgpu_devbuf.h; the table of them is in csrc/msgpu_api.hip)
is allocated at exactly the size that was asked for, filled with 0xA5 instead of whatever hipMalloc returns -- zero pages in a
fresh process, an earlier job's own plausible values after it -- and lies between guards that every entry compares before it
returns MSGPU_OK; and every job starts on fresh blocks, because a job start gives back whatever does not carry state.  The
inputs, the comparisons and the expected values are those of the clean files: this file imports them and runs their checks
(RUN), under the names "test_<file>__<check>" and with the clean file's own parameter lists, so every table is compared with
the oracle bit for bit (helpers.assert_tables_equal) and a case added to a clean file is run here too.  What is left out, and
why, is in LEFT_OUT.  A difference under poison is a kernel that read something before anything wrote it; an error that begins
with "arena guard:" is a write outside a table, named by buffer, size and side.  That the poison and the guards work is shown
by tests/cpp/test_devbuf.hip (tests/test_gpu_devbuf.py), that the switch reaches every buffer of the context by the two tests
at the end of this file -- not by damaging a context.  Every test runs under its own time limit: a watchdog ends the process
when a call does not come back.  No test provokes a device fault."""
import ctypes as C
import faulthandler
import os

import pytest

import test_gpu_batched as batched
import test_gpu_chain_band as chain_band
import test_gpu_chain_classes as chain_classes
import test_gpu_chain_directions as chain_directions
import test_gpu_chain_extremes as chain_extremes
import test_gpu_compact_moves as compact_moves
import test_gpu_params as params
import test_gpu_parity as parity
import test_gpu_scaffold_rows as scaffold_rows
import test_packed_rows as packed_rows
from helpers import assert_tables_equal
from test_gpu_poisoned_arena import LIMIT  # seconds per test: the sister file's
# the module-scoped inputs and expected tables of the clean files (made once per file, on the CPU or on clean memory)
from test_gpu_chain_extremes import ill_formed, ill_formed_want, ties_b, ties_c  # noqa: F401
from test_gpu_compact_moves import jobs  # noqa: F401
from test_gpu_scaffold_rows import synth_job, wants  # noqa: F401

pytestmark = pytest.mark.gpu

ALL = None  # every test of the file
# the checks that run poisoned: (file, its name here, the checks)
RUN = (
    (parity, "parity", (
        "test_synthetic_matches_oracle", "test_dense_inputs_take_the_big_paths", "test_every_sort_path_of_the_index",
        "test_bin_path_ranks_reads_with_equal_nanopore_ranges", "test_scaffold_lengths_around_the_pass1_context",
        "test_mixed_direction_edges", "test_reads_with_many_partners", "test_shortcut_and_full_sweep_agree",
        "test_index_bin_path_and_atomic_path_agree", "test_a_context_reused_for_growing_and_failing_jobs_stays_on_the_bin_path",
        "test_sub_wavefront_and_whole_wavefront_chaining_agree", "test_one_context_many_jobs_of_changing_size",
        "test_both_read_back_modes_on_one_context", "test_empty_and_tiny", "test_hand_derived_cases",
        "test_duplicates_and_row_order_do_not_matter", "test_golden_fixtures", "test_shards_union_equals_single_gpu",
        "test_wire_form_merge_equals_whole_record_merge", "test_one_context_goes_from_shard_to_shard_and_back", "test_declared_id_space", "test_find_contraction_edges_matches_oracle",
        "test_find_contraction_edges_state_and_empty", "test_find_contraction_edges_on_random_graphs")),
    (chain_classes, "chain_classes", ALL),
    (chain_extremes, "chain_extremes", ALL),
    (chain_band, "chain_band", ALL),
    (chain_directions, "chain_directions", ALL),
    (scaffold_rows, "scaffold_rows", ALL),
    (compact_moves, "compact_moves", ALL),
    (params, "params", ("test_hand_cases_at_params",)),
    (batched, "batched", ("test_any_batch_count_gives_the_single_pass_tables", "test_batched_edge_cases",
                          "test_resident_run_leaves_the_job_tables_in_hbm", "test_lean_windows_leave_in_wire_form_or_as_records")),
    (packed_rows, "packed_rows", ("test_load_rows_packed_gives_the_same_tables",)),
)
# what is left out: (what, why)
LEFT_OUT = (
    ("test_gpu_fullsize.py, test_gpu_batched.py::*_cfg2_full_size*, test_gpu_parity.py::test_property_checks_at_full_size, "
     "test_gpu_parity.py::test_index_bin_path_takes_several_passes_beyond_131072_reads",
     "configuration size: seconds of filling and of oracle, and no edge that the small inputs lack"),
    ("test_gpu_parity.py::test_bench_*, test_group_*, test_pipelined_exchange_*, test_stream_contract_caller_buffers, test_api_state_and_id_checks",
     "the benchmark, the group over RCCL and the stream contract: processes, collectives and stream order, not tables"),
    ("test_gpu_parity.py::test_group_deadline_on_a_stalled_stream",
     "a verifying entry synchronises the context's streams, and a wait that gives up is what that test is about"),
    ("test_gpu_params.py but its hand cases", "workloads at parameter sets: the chain stage's arithmetic, not its memory"),
)

for _mod, _short, _names in RUN:
    for _name in (_names if _names is not ALL else [n for n, f in sorted(vars(_mod).items())
                                                     if n.startswith("test_") and getattr(f, "__module__", None) == _mod.__name__]):
        # the clean file's function itself, with its parameter lists: collected here too, under this file's autouse fixtures
        globals()["test_%s__%s" % (_short, _name[len("test_"):])] = getattr(_mod, _name)


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("MSGPU_POISON", "1")  # (DevBuf asks per allocation, the context per entry)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import _lib
    return _lib


@pytest.fixture(autouse=True)
def time_limit(lib):  # (after lib: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def test_nothing_that_should_run_is_missing():
    """every check of RUN is a test of this file, and a clean file's test is here under a name of its own"""
    mine = {n for n in globals() if n.startswith("test_")}
    for mod, short, names in RUN:
        for name in names or ():
            assert "test_%s__%s" % (short, name[len("test_"):]) in mine, name
    assert len(mine) >= 60  # (functions: their parameter lists come on top)


# ---- the switch reaches the context, and moves nothing

# the buffers that carry something across the start of a job: the second copy of the `carries` column of the buffer table in
# csrc/msgpu_api.hip (MSGPU_CTX_BUFS) -- a change to one must be made to the other
CARRIES = {
    "bin_cursor",  # the bin path's bucket cursors and row base, zero at rest: k_index_sort_bin and k_index_epilogue leave them so
    "pair_tab",    # the chain kernels' constant pair tables, filled when the buffer is allocated
}
SAME_COUNTS = ("index_path", "n_lost_publications", "n_edges", "n_ems", "n_orders", "n_ids")


def _report(lib, ctx):
    """msgpu_debug_buffers: {name: (bytes, guarded, carries, generation)}"""
    need = C.c_size_t()
    assert lib.lib().msgpu_debug_buffers(ctx._h, None, 0, C.byref(need)) == lib.OK
    text = C.create_string_buffer(need.value)
    assert lib.lib().msgpu_debug_buffers(ctx._h, text, need.value, None) == lib.OK
    lines = [ln.split() for ln in text.value.decode().splitlines()]
    assert len(lines) >= 60 and all(len(ln) == 5 for ln in lines), lines
    rep = {ln[0]: tuple(int(x) for x in ln[1:]) for ln in lines}
    assert len(rep) == len(lines)  # every buffer has a name of its own
    return rep


def _job(lib, ctx, rows):
    """load, candidates, chains through the C ABI: every return code and error text, the tables, the counts"""
    L = lib.lib()
    for call in (lambda: L.msgpu_load_rows(ctx._h, rows.ctypes.data, len(rows)), lambda: L.msgpu_calculate_edges(ctx._h),
                 lambda: L.msgpu_chaining_and_overlaps(ctx._h)):
        rc = call()
        assert (rc, L.msgpu_last_error(ctx._h)) == (lib.OK, b"")
    tables = ctx.tables()
    assert L.msgpu_last_error(ctx._h) == b""
    counts = ctx.counts()
    return tables, {f: int(getattr(counts, f)) for f in SAME_COUNTS}


def test_the_switch_reaches_the_context_and_moves_no_table(oracle, lib, monkeypatch):
    """one small job on a context with the switch and on another one without it, in this process: the oracle's tables twice, the
    same counts, MSGPU_OK with no error text (the guards were compared); the poisoned context's report shows every buffer
    that holds a block as guarded, the plain one's none, and the buffers that carry state are the ones written down here"""
    from muchsalsa_amd import overlap, synth
    rows = synth.synth_rows(300, 3000, 900, 1)
    want = oracle.overlap(rows)
    assert os.environ.get("MSGPU_POISON") == "1"
    with overlap.OverlapContext(0) as ctx:
        poisoned, poisoned_counts = _job(lib, ctx, rows)
        rep = _report(lib, ctx)
    with monkeypatch.context() as clean:
        clean.delenv("MSGPU_POISON")
        with overlap.OverlapContext(0) as ctx:
            plain, plain_counts = _job(lib, ctx, rows)
            plain_rep = _report(lib, ctx)
    assert_tables_equal(poisoned, want, "poisoned")
    assert_tables_equal(plain, want, "plain")
    assert_tables_equal(poisoned, plain, "poisoned against plain")
    assert poisoned_counts == plain_counts and poisoned_counts["n_lost_publications"] == 0
    assert poisoned_counts["index_path"] == lib.INDEX_BIN and len(want["edges"]) == poisoned_counts["n_edges"] > 0
    held = {n for n, (nbytes, _, _, _) in rep.items() if nbytes}
    assert len(held) >= 40 and held == {n for n, (nbytes, _, _, _) in plain_rep.items() if nbytes}
    assert all(rep[n][1] == 1 and rep[n][3] >= 1 for n in held), {n: rep[n] for n in held if rep[n][1] != 1}
    assert not any(g for _, g, _, _ in plain_rep.values())
    assert all(rep[n][0] <= plain_rep[n][0] for n in held)  # exact against need + need / 8 + 256
    assert {n for n, v in rep.items() if v[2]} == CARRIES == {n for n, v in plain_rep.items() if v[2]}
    assert CARRIES <= held


def test_a_second_job_starts_on_fresh_blocks(oracle, lib):
    """two jobs on one poisoned context, the second one smaller: every buffer that carries nothing and that the second job uses
    was allocated again for it, and none is larger than what the second job asks for by itself -- what a fresh context that
    runs the second job alone allocates; the tables are the oracle's"""
    from muchsalsa_amd import overlap, synth
    large, small = synth.synth_rows(600, 4000, 1500, 13), synth.synth_rows(300, 3000, 900, 1)
    assert len(small) < len(large)
    with overlap.OverlapContext(0) as ctx:
        first, _ = _job(lib, ctx, large)
        after_first = _report(lib, ctx)
        second, _ = _job(lib, ctx, small)
        after_second = _report(lib, ctx)
    with overlap.OverlapContext(0) as ctx:
        alone, _ = _job(lib, ctx, small)
        own = _report(lib, ctx)
    assert_tables_equal(first, oracle.overlap(large), "the larger job")
    want = oracle.overlap(small)
    assert_tables_equal(second, want, "the smaller job behind the larger one")
    assert_tables_equal(alone, want, "the smaller job alone")
    used = {n for n, v in own.items() if v[0]}
    assert len(used) >= 40
    for name in sorted(used - CARRIES):
        assert after_second[name][3] > after_first[name][3], (name, after_first[name], after_second[name])
        assert after_second[name][1] == 1 and after_second[name][0] == own[name][0], (name, after_second[name], own[name])
    for name, (nbytes, _, carries, _) in after_second.items():  # what the second job does not use is gone, or carries
        assert name in used or carries or nbytes == 0, (name, nbytes)
    assert any(after_second[n][0] < after_first[n][0] for n in used - CARRIES)


def test_scratch_entries_leave_the_standing_job_usable(oracle, lib):
    """msgpu_get_edgematches and msgpu_merge_gathered give back the buffers that are scratch of one call; the job that stands
    must not notice: on ONE poisoned context shard 0 of 2, then EdgeMatches of three edges (a scan of its own, a few bytes of
    scratch), a merge of the shard's own tables on the context's stream, and shard 1 of 2 and shard 0 again on the index that
    stands -- the candidate stage of a shard scans the visit counts itself, in the scratch the index build sized"""
    import numpy as np
    import torch
    from muchsalsa_amd import distributed as D, overlap, synth
    from muchsalsa_amd._lib import EDGE_DTYPE, ORDER_DTYPE
    rows = synth.synth_rows(300, 3000, 900, 1)
    full = oracle.overlap(rows)
    dev = torch.device("cuda", 0)

    def shard(ctx, r):
        ctx.set_shard(r, 2)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        t = ctx.tables()
        assert_tables_equal(t, D.shard_view_host(full, r, 2), "shard %d of 2" % r)
        return t

    with overlap.OverlapContext(0) as ctx:
        ctx.set_shard(0, 2)
        ctx.load_rows(rows)
        t = shard(ctx, 0)
        before = _report(lib, ctx)
        e = t["edges"]
        assert len(e) > 3
        pick = [0, len(e) // 2, len(e) - 1]
        _, ems = ctx.get_edgematches(pick)
        assert ems.tobytes() == b"".join(t["ems"][int(e["em_off"][i]): int(e["em_off"][i]) + int(e["em_cnt"][i])].tobytes() for i in pick)
        counts = np.array([[len(t["edges"]), len(t["orders"]), len(t["ids"])]], dtype=np.int64)
        offs, slab_bytes = D.slab_layout(counts.max(axis=0))
        gathered = np.zeros(slab_bytes, dtype=np.uint8)
        for name, off in zip(("edges", "orders", "ids"), offs):
            b = t[name].view(np.uint8)
            gathered[off: off + len(b)] = b
        d_g = torch.from_numpy(gathered).to(dev)
        d_e = torch.zeros(len(t["edges"]) * EDGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_o = torch.zeros(max(len(t["orders"]), 1) * ORDER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        d_i = torch.zeros(max(len(t["ids"]), 1) * 4, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()  # (STREAM CONTRACT rule 3, the host-wait way)
        ctx.merge_gathered(d_g.data_ptr(), counts, slab_bytes, offs, d_e.data_ptr(), d_o.data_ptr(), d_i.data_ptr())
        ctx.synchronize()
        assert d_o.cpu().numpy()[: len(t["orders"]) * ORDER_DTYPE.itemsize].tobytes() == t["orders"].tobytes()
        after = _report(lib, ctx)
        for name in ("scan_tmp", "read_off", "vis16", "edges"):  # the job's buffers stand: the same blocks
            assert after[name] == before[name] and before[name][0] > 0, (name, before[name], after[name])
        shard(ctx, 1)
        _, ems = ctx.get_edgematches([0])
        shard(ctx, 0)
        assert int(ctx.counts().n_lost_publications) == 0
