"""GPU parity: libmsgpu (through the C-ABI) against the CPU oracle on identical rows.  Bit-exact."""
import numpy as np
import pytest

from helpers import assert_tables_equal

pytestmark = pytest.mark.gpu


def _gpu_tables(rows, **kw):
    from muchsalsa_amd import overlap
    return overlap.build_overlaps(rows, **kw)


@pytest.mark.parametrize("shape", [(300, 3000, 900, 1), (2000, 5000, 10000, 7), (1500, 10000, 8000, 11)])
def test_synthetic_matches_oracle(oracle, shape):
    from muchsalsa_amd import synth
    rows = synth.synth_rows(*shape)
    want = oracle.overlap(rows)
    got = _gpu_tables(rows)
    assert_tables_equal(got, want, "synth%r" % (shape,))


@pytest.mark.parametrize("shape,coverage,what", [
    ((120, 20000, 2400, 5), 10, "reads with ~190 rows (global-memory sort path), candidate class 1, edges > 64"),
    ((400, 4000, 120, 6), 200, "200x coverage: candidate lists beyond LDS (k_candidates_big), many edges > 64"),
])
def test_dense_inputs_take_the_big_paths(oracle, shape, coverage, what):
    from muchsalsa_amd import synth
    rows, _, _ = synth.accepted_rows(synth.paf_table(*shape, coverage=coverage))
    want = oracle.overlap(rows)
    assert want["edges"]["em_cnt"].max() > 64, what
    got = _gpu_tables(rows)
    assert_tables_equal(got, want, what)


@pytest.mark.parametrize("n_anchors,lo,hi", [(1200, 65, 128), (2400, 129, 256), (4800, 257, 2000)])
def test_every_sort_path_of_the_index(oracle, n_anchors, lo, hi):
    """k_sort_read ranks a read's rows in registers up to 256 rows (1, 2 or 4 rows per lane) and in global memory
    beyond; a duplicated (read, anchor) pair sends a register-sized read down the global path too.  Each size class,
    as grouped input (scaffold table = input order) and shuffled with duplicates (generic index build)."""
    from muchsalsa_amd import synth
    rows, _, _ = synth.accepted_rows(synth.paf_table(120, 20000, n_anchors, 5, coverage=10))
    per_read = np.bincount(rows["read_id"])
    assert ((per_read >= lo) & (per_read <= hi)).sum() > 20, per_read
    want = oracle.overlap(rows)
    assert_tables_equal(_gpu_tables(rows), want, "grouped input")
    rng = np.random.default_rng(n_anchors)
    dup = rows[rng.choice(len(rows), 60, replace=False)].copy()
    dup["line"] = rows["line"].max() + 1 + np.arange(len(dup))
    dup["n_hi"] += 3
    allrows = np.concatenate([rows, dup])
    rng.shuffle(allrows)
    assert_tables_equal(_gpu_tables(allrows), want, "shuffled with duplicates")


def test_bin_path_ranks_reads_with_equal_nanopore_ranges(oracle):
    """Regression shape for round 4's 02:15 abort (profiles/r5_01/README.md): dense reads of 50..130 rows ON THE BIN PATH -- the
    wavefront-wide bitonic ranking of k_index_sort_bin (one row per lane) and the two-rows-per-lane broadcast ranking -- with
    rows of one read that share their nanopore range, so that the anchor id decides (mpp.cpp:164-172) and the sort network's
    equal-neighbour test must send the read to the broadcast loop.  The dense shape of test_dense_inputs_take_the_big_paths
    itself (200x coverage) leaves the bin path at pass 1 (scaffolds of 400 rows): its index path is asserted here too."""
    from muchsalsa_amd import _lib, overlap, synth

    def run(rows):
        with overlap.OverlapContext(0) as ctx:
            ctx.load_rows(rows)
            ctx.calculate_edges()
            ctx.chaining_and_overlaps()
            return ctx.tables(), int(ctx.counts().index_path)

    rows = synth.accepted_rows(synth.paf_table(400, 4000, 400, 6, coverage=60))[0].copy()  # reads of 52..78 rows
    per_read = np.bincount(rows["read_id"])
    assert per_read.max() > 64 and (per_read <= 64).sum() > 50 and np.bincount(rows["anchor_id"]).max() < 128, (per_read.min(), per_read.max())
    # ties: in every third read, the second row (in file order) takes the first row's nanopore range
    order = np.argsort(rows["read_id"], kind="stable")
    starts = np.concatenate([[0], np.cumsum(per_read)[:-1]])
    n_ties = 0
    for r in range(0, len(per_read), 3):
        if per_read[r] >= 2:
            a, b = order[starts[r]], order[starts[r] + 1]
            rows["n_lo"][b], rows["n_hi"][b] = rows["n_lo"][a], rows["n_hi"][a]
            n_ties += 1
    assert n_ties > 100
    want = oracle.overlap(rows)
    got, path = run(rows)
    assert path == _lib.INDEX_BIN, path
    assert_tables_equal(got, want, "bin path, equal nanopore ranges inside a read")
    dense = synth.accepted_rows(synth.paf_table(400, 4000, 120, 6, coverage=200))[0]
    got, path = run(dense)
    assert (path & 3) != _lib.INDEX_BIN, path  # scaffolds beyond pass 1's context: the atomic path
    assert_tables_equal(got, oracle.overlap(dense), "dense shape of the round-4 abort")


@pytest.mark.parametrize("coverage,n_anchors", [(40, 400), (85, 60), (95, 60), (300, 40)])
def test_scaffold_lengths_around_the_pass1_context(oracle, coverage, n_anchors):
    """Scaffolds are kept in read-id order.  With the input grouped by anchor, k_index_pass1 places every row inside its
    scaffold from an LDS tile holding 128 rows of context on either side; a scaffold that does not fit raises IXF_BIGSCAF
    and the generic scaffold build (rank by read id) runs.  Scaffolds of tens of rows (the tile path, straddling
    workgroup boundaries), just under and around the limit, and of 500 rows (generic), grouped and shuffled."""
    from muchsalsa_amd import synth
    rows, _, _ = synth.accepted_rows(synth.paf_table(500, 4000, n_anchors, 77, coverage=coverage))
    longest = int(np.bincount(rows["anchor_id"]).max())
    assert longest > (30 if coverage == 40 else 100), longest
    want = oracle.overlap(rows)
    assert_tables_equal(_gpu_tables(rows), want, "grouped, longest scaffold %d" % longest)
    sh = rows.copy()
    np.random.default_rng(coverage).shuffle(sh)
    assert_tables_equal(_gpu_tables(sh), want, "shuffled, longest scaffold %d" % longest)


@pytest.mark.parametrize("dense", [False, True])
def test_mixed_direction_edges(oracle, dense):
    """Rows of one read with both strands give edges whose EdgeMatches differ in direction: the pair sweep then skips
    pairs of unlike direction, both path lists fill, and the filters of main.cpp:355-387 work on their union.  (The
    generators give every read one strand, so no other test has such an edge.)"""
    from muchsalsa_amd import synth
    ROW_DIR, ROW_PRIMARY = 1, 2  # MSGPU_ROW_DIR, MSGPU_ROW_PRIMARY (include/msgpu.h)
    if dense:
        rows, _, _ = synth.accepted_rows(synth.paf_table(120, 20000, 1200, 5, coverage=10))
    else:
        rows = synth.synth_rows(600, 4000, 1500, 13)
    rows = rows.copy()
    rng = np.random.default_rng(17 + dense)
    flip = rng.random(len(rows)) < 0.3
    rows["flags"] = np.where(flip, rows["flags"] ^ ROW_DIR, rows["flags"])
    rows["flags"] = np.where(rng.random(len(rows)) < 0.2, rows["flags"] ^ ROW_PRIMARY, rows["flags"])
    want = oracle.overlap(rows)
    e, em = want["edges"], want["ems"]
    plus = np.bincount(np.repeat(np.arange(len(e)), e["em_cnt"]), weights=em["flags"] & 1, minlength=len(e))
    n_mixed = int(((plus > 0) & (plus < e["em_cnt"])).sum())
    assert n_mixed > 200, n_mixed
    assert_tables_equal(_gpu_tables(rows), want, "mixed directions (%d edges)" % n_mixed)


@pytest.mark.parametrize("n_anchors,coverage", [(100, 40), (200, 60)])
def test_reads_with_many_partners(oracle, n_anchors, coverage):
    """k_candidates orders a group's candidates by popcounts in one bitmap per group (64 / 128 groups fit in LDS,
    depending on the class); a read with more partner reads than that takes the staged comparison ranking instead.
    High coverage with few anchors per read gives such reads inside the LDS classes."""
    from muchsalsa_amd import synth
    rows, _, _ = synth.accepted_rows(synth.paf_table(600, 3000, n_anchors, 31, coverage=coverage))
    want = oracle.overlap(rows)
    partners = np.bincount(want["edges"]["v1"], minlength=int(rows["read_id"].max()) + 1)
    visits = np.bincount(rows["read_id"], weights=np.bincount(rows["anchor_id"])[rows["anchor_id"]])
    small = ((partners > 64) & (visits <= 512)).sum()
    mid = ((partners > 128) & (visits > 512) & (visits <= 1024)).sum()
    assert small + mid > 0, (int(partners.max()), int(visits.max()))
    assert_tables_equal(_gpu_tables(rows), want, "many partners")


def test_shortcut_and_full_sweep_agree(oracle, monkeypatch):
    """k_chain's all-pairs-compatible shortcut must change nothing: same tables with it disabled, and equal to the
    oracle's; and it must actually be taken on clean synthetic overlaps."""
    from muchsalsa_amd import overlap, synth
    rows = synth.synth_rows(2000, 5000, 10000, 7)
    want = oracle.overlap(rows)
    with overlap.OverlapContext(0) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        fast = ctx.tables()
        c = ctx.counts()
    assert 0 < c.n_edges_fastpath <= c.n_edges
    monkeypatch.setenv("MSGPU_NO_FASTPATH", "1")
    with overlap.OverlapContext(0) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        slow = ctx.tables()
        assert ctx.counts().n_edges_fastpath == 0
    assert_tables_equal(fast, want, "shortcut")
    assert_tables_equal(slow, want, "full sweep")


def test_index_bin_path_and_atomic_path_agree(oracle, monkeypatch):
    """The index build has two ways to the same tables: the bin path (rows binned by coarse read-id bucket, no global atomic per
    row: what a table from msgpu_parse_paf takes) and the atomic path of rounds 1-3 (every input).  A loader-shaped table takes
    the bin path; MSGPU_NO_BIN=1 forces the atomic one; shuffled rows, a duplicate (read, anchor) pair, a read of more than 256
    rows and a scaffold longer than pass 1's context fall back by themselves.  All equal the oracle -- and each other, down to
    the per-read Vertex facts."""
    from muchsalsa_amd import _lib, overlap, synth

    def run(rows):
        with overlap.OverlapContext(0) as ctx:
            ctx.load_rows(rows)
            ctx.calculate_edges()
            ctx.chaining_and_overlaps()
            return ctx.tables(), ctx.reads(), int(ctx.counts().index_path)

    # (the last two: reads of 65..128 and 129..256 rows -- two and four rows per lane in the ranking; the very last one's buckets
    # need more than 64 KB of LDS in k_index_sort_bin)
    shapes = [(1000, 5000, 4000, 13), (37, 3000, 150, 4), (3000, 2500, 9000, 5), (400, 30000, 3000, 6), (400, 30000, 4400, 6)]
    for shape in shapes:
        rows = synth.synth_rows(*shape)
        want = oracle.overlap(rows)
        t_bin, reads_bin, path = run(rows)
        assert path == _lib.INDEX_BIN, (shape, path)
        assert_tables_equal(t_bin, want, "bin path %r" % (shape,))
        monkeypatch.setenv("MSGPU_NO_BIN", "1")
        t_at, reads_at, path = run(rows)
        monkeypatch.delenv("MSGPU_NO_BIN")
        # (a read of more than 128 rows does not fit the atomic path's fixed bucket: count, scan, scatter)
        assert path in (_lib.INDEX_ATOMIC, _lib.INDEX_TWO_PASS), (shape, path)
        assert_tables_equal(t_at, want, "atomic path %r" % (shape,))
        assert all(np.array_equal(a, b) for a, b in zip(reads_bin, reads_at))
    rows = synth.synth_rows(1000, 5000, 4000, 13)
    want = oracle.overlap(rows)
    rng = np.random.default_rng(3)
    shuffled = rows.copy()
    rng.shuffle(shuffled)
    t, _, path = run(shuffled)                       # not grouped by anchor: generic scaffolds on the atomic path
    assert path == (_lib.INDEX_ATOMIC | _lib.INDEX_GENERIC), path
    assert_tables_equal(t, want, "shuffled")
    dup = rows[100:101].copy()                       # a second row of one (read, anchor) pair, on a later line: it loses
    dup["line"] = rows["line"].max() + 5
    dup["n_lo"] += 3
    k = int(np.searchsorted(rows["anchor_id"], dup["anchor_id"][0], side="right"))
    with_dup = np.concatenate([rows[:k], dup, rows[k:]])
    with_dup["line"][k + 1:] += 0                    # (lines stay ascending inside every anchor: the duplicate has the largest)
    t, _, path = run(with_dup)
    assert path & _lib.INDEX_GENERIC and (path & 3) == _lib.INDEX_ATOMIC, path
    assert_tables_equal(t, want, "duplicate pair")
    # a read of more than 256 rows (long read, dense anchors): beyond what a wavefront ranks in registers
    long_rows = synth.accepted_rows(synth.paf_table(60, 60000, 9000, 5, coverage=10))[0]
    assert np.bincount(long_rows["read_id"]).max() > 256
    t, _, path = run(long_rows)
    assert (path & 3) != _lib.INDEX_BIN, path
    assert_tables_equal(t, oracle.overlap(long_rows), "long reads")


def test_a_context_reused_for_growing_and_failing_jobs_stays_on_the_bin_path(oracle):
    """The bin path's bucket cursors and the scalar block are zero AT REST (no init launch, no memset per build: round 5): whoever
    consumes a counter last leaves it zero.  The corner cases of that bookkeeping on ONE context: a job with more buckets than any
    before it but inside the buffer's slack (words no init launch has reached; tests/test_gpu_poisoned_overlap.py runs this check
    under MSGPU_POISON, where the buffer has no slack and the larger job gets a block of 0xA5), a job the bin path refuses (duplicates: flags raised, cursors left behind), the same sizes again
    afterwards, and back-to-back loads without the later stages -- every loader-shaped job must take the bin path and give the
    oracle's tables."""
    from muchsalsa_amd import _lib, overlap, synth

    def tables_of(ctx, rows):
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables(), int(ctx.counts().index_path)

    small = synth.synth_rows(3000, 2500, 9000, 5)
    larger = synth.synth_rows(3900, 2500, 11000, 6)  # 244 buckets instead of 188: inside the cursor buffer's slack
    with overlap.OverlapContext(0) as ctx:
        for name, rows in (("small", small), ("larger", larger), ("small again", small)):
            got, path = tables_of(ctx, rows)
            assert path == _lib.INDEX_BIN, (name, path)
            assert_tables_equal(got, oracle.overlap(rows), name)
        dup = larger[100:101].copy()  # a second row of one (read, anchor) pair on a later line: the bin path raises its flag and stops
        dup["line"] = larger["line"].max() + 5
        k = int(np.searchsorted(larger["anchor_id"], dup["anchor_id"][0], side="right"))
        with_dup = np.concatenate([larger[:k], dup, larger[k:]])
        got, path = tables_of(ctx, with_dup)
        assert (path & 3) != _lib.INDEX_BIN, path
        assert_tables_equal(got, oracle.overlap(larger), "duplicate pair")
        for name, rows in (("larger after the refused job", larger), ("small after it", small)):
            got, path = tables_of(ctx, rows)
            assert path == _lib.INDEX_BIN, (name, path)
            assert_tables_equal(got, oracle.overlap(rows), name)
        ctx.load_rows(small)   # loads without the later stages: the list cursors of the first are still standing
        ctx.load_rows(larger)
        got, path = tables_of(ctx, small)
        assert path == _lib.INDEX_BIN and ctx.counts().n_lost_publications == 0
        assert_tables_equal(got, oracle.overlap(small), "after two bare loads")
        ctx.calculate_edges()  # the candidate stage twice on one index: its sums start over
        ctx.chaining_and_overlaps()
        assert_tables_equal(ctx.tables(), oracle.overlap(small), "second candidate stage on the same index")


def test_index_bin_path_takes_several_passes_beyond_131072_reads(oracle):
    """k_index_bin bins 8192 buckets of 16 read ids per pass: 139,978 reads take two passes over the row table (the second one's
    buckets start behind the first one's rows in by_read).  Every table equal to the oracle's; the Vertex facts too."""
    from muchsalsa_amd import _lib, overlap, synth
    rows = synth.synth_rows(140000, 1500, 120000, 17)
    assert int(rows["read_id"].max()) + 1 > 131072
    want = oracle.overlap(rows)
    with overlap.OverlapContext(0) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        assert int(ctx.counts().index_path) == _lib.INDEX_BIN
        assert_tables_equal(ctx.tables(), want, "two passes")
        rl, fl = ctx.reads()
        assert np.array_equal(rl, want["read_len"]) and np.array_equal(fl, want["read_first_line"])


def test_sub_wavefront_and_whole_wavefront_chaining_agree(oracle, monkeypatch):
    """Edges of <= 32 EdgeMatches share a wavefront (the 8-, 16- and 32-wide bodies of k_chain_sub_all: one launch), longer
    ones take one each (k_chain): MSGPU_CHAIN_SERIAL=1 gives every width a launch of its own (k_chain_sub<8|16|32>, one
    after the other), MSGPU_NO_SUBWAVE=1 sends every edge through k_chain.  All three must give the oracle's tables; the
    workload has edges in all four width classes."""
    from muchsalsa_amd import overlap, synth
    rows, _, _ = synth.accepted_rows(synth.paf_table(400, 8000, 3200, 23, coverage=8))
    want = oracle.overlap(rows)
    n = want["edges"]["em_cnt"]
    assert (n <= 8).sum() > 100 and ((n > 8) & (n <= 16)).sum() > 100 and ((n > 16) & (n <= 32)).sum() > 100 \
        and ((n > 32) & (n <= 64)).sum() > 100, np.bincount(np.minimum(n, 65) // 9)
    assert_tables_equal(_gpu_tables(rows), want, "width classes")
    monkeypatch.setenv("MSGPU_CHAIN_SERIAL", "1")
    assert_tables_equal(_gpu_tables(rows), want, "a launch per width")
    monkeypatch.delenv("MSGPU_CHAIN_SERIAL")
    monkeypatch.setenv("MSGPU_NO_SUBWAVE", "1")
    assert_tables_equal(_gpu_tables(rows), want, "one edge per wavefront")


def test_one_context_many_jobs_of_changing_size(oracle):
    """A context keeps its tables between calls and launches edge emission, size sort and compaction into them before it
    knows the new sizes (the kernels and the host compare the same counts with the same capacities).  Jobs that grow, shrink
    and grow again on ONE context -- every launch-again and every first-try path -- each equal the oracle; with the stage
    markers off the tables are the same and only the chain-kernel time is reported."""
    from muchsalsa_amd import overlap, synth
    shapes = [(300, 3000, 900, 1), (2000, 5000, 10000, 7), (300, 3000, 900, 2), (1500, 10000, 8000, 11), (2000, 5000, 10000, 8),
              (40, 3000, 200, 3), (120, 20000, 2400, 5)]
    with overlap.OverlapContext(0) as ctx:
        for k, shape in enumerate(shapes):
            rows = synth.synth_rows(*shape) if k != len(shapes) - 1 else synth.accepted_rows(synth.paf_table(*shape, coverage=10))[0]
            want = oracle.overlap(rows)
            ctx.set_stage_events(k % 2 == 0)
            for rep in range(2):  # the second pass over the same job finds every table large enough
                ctx.load_rows(rows)
                ctx.calculate_edges()
                ctx.chaining_and_overlaps()
                assert_tables_equal(ctx.tables(), want, "job %d %r pass %d" % (k, shape, rep))
            tm = ctx.timings()
            assert tm.chain_kernel_launches == 2 and tm.chain_kernel_ms > 0
            assert (tm.index_ms > 0 and tm.candidates_ms > 0 and tm.chain_ms > 0) == (k % 2 == 0)
            assert ctx.timings().chain_kernel_launches == 0  # the window of chain-kernel events starts afresh


@pytest.mark.parametrize("mode", ["mapped", "copy"])
def test_both_read_back_modes_on_one_context(oracle, monkeypatch, mode):
    """The table sizes reach the host one of two ways, fixed when the context is created: the stage-closing kernels publish the
    scalar block into mapped memory (default), or, with MSGPU_SYNC_READBACK set, a copy follows them.  In each mode: jobs that
    grow, shrink and grow again on ONE context (k_emit_edges and k_compact launched again behind a reallocation, and not), a
    dispatcher run of several windows, and bin-path and atomic-path index builds (grouped and shuffled rows) -- every table
    equal to the oracle's, no publication lost."""
    from muchsalsa_amd import _lib, overlap, synth
    if mode == "copy":
        monkeypatch.setenv("MSGPU_SYNC_READBACK", "1")
    else:
        monkeypatch.delenv("MSGPU_SYNC_READBACK", raising=False)

    def tables_of(ctx, rows):
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables(), int(ctx.counts().index_path)

    # edges, orders and ids: 3.1 k / 3.8 k / 20 k, 9.8 k / 11 k / 94 k, 2.8 k / 3.5 k / 18 k, 20 k / 22 k / 208 k
    shapes = [(300, 3000, 900, 1), (1000, 5000, 4000, 13), (300, 3000, 900, 2), (2000, 5000, 10000, 7)]
    with overlap.OverlapContext(0) as ctx:
        for shape in shapes:
            rows = synth.synth_rows(*shape)
            got, path = tables_of(ctx, rows)
            assert path == _lib.INDEX_BIN, (mode, shape, path)
            assert_tables_equal(got, oracle.overlap(rows), "%s read-back, job %r" % (mode, shape))
        rows = synth.synth_rows(*shapes[1])
        got, _ = ctx.overlap_batched(rows, 4)
        assert_tables_equal(got, oracle.overlap(rows), "%s read-back, four windows" % mode)
        assert ctx.counts().n_lost_publications == 0
    monkeypatch.setenv("MSGPU_NO_BIN", "1")
    rows = synth.synth_rows(*shapes[1])
    shuffled = rows.copy()
    np.random.default_rng(5).shuffle(shuffled)
    want = oracle.overlap(rows)
    with overlap.OverlapContext(0) as ctx:
        got, path = tables_of(ctx, rows)
        assert path in (_lib.INDEX_ATOMIC, _lib.INDEX_TWO_PASS), (mode, path)
        assert_tables_equal(got, want, "%s read-back, atomic path" % mode)
        got, path = tables_of(ctx, shuffled)  # generic scaffolds: a second read-back in the index build
        assert path == (_lib.INDEX_ATOMIC | _lib.INDEX_GENERIC), (mode, path)
        assert_tables_equal(got, want, "%s read-back, atomic path, shuffled" % mode)
        assert ctx.counts().n_lost_publications == 0


def test_empty_and_tiny(oracle):
    from muchsalsa_amd import synth
    rows = synth.synth_rows(300, 3000, 900, 1)
    for n in (0, 1, 2, 5):
        sub = rows[:n].copy()
        # keep Registry-dense ids
        _, sub["read_id"] = np.unique(sub["read_id"], return_inverse=True)
        _, sub["anchor_id"] = np.unique(sub["anchor_id"], return_inverse=True)
        assert_tables_equal(_gpu_tables(sub), oracle.overlap(sub), "n=%d" % n)


def test_hand_derived_cases(oracle):
    """The known-answer vectors of test_golden_hand.py through the HIP path."""
    import test_golden_hand as H
    for name, rows in H.CASES.items():
        got = _gpu_tables(rows)
        assert_tables_equal(got, oracle.overlap(rows), name)
    H.check_single_anchor(_gpu_tables(H.CASES["single_plus"]), True)
    H.check_single_anchor(_gpu_tables(H.CASES["single_minus"]), False)


def test_duplicates_and_row_order_do_not_matter(oracle):
    """addVertexMatch keeps the lowest line of a (read, anchor) pair (MatchMap.cpp:64-80); row order is free."""
    from muchsalsa_amd import synth
    rows = synth.synth_rows(300, 4000, 1000, 9)
    rng = np.random.default_rng(5)
    dup = rows[rng.choice(len(rows), 200, replace=False)].copy()
    dup["line"] = rows["line"].max() + 1 + np.arange(len(dup))
    dup["n_lo"] += 7
    allrows = np.concatenate([rows, dup])
    rng.shuffle(allrows)
    want = oracle.overlap(rows)
    assert_tables_equal(_gpu_tables(allrows), want, "dups")


def test_golden_fixtures():
    """Committed golden tables (tests/golden/, made by tools/make_golden.py from the oracle)."""
    import glob
    import os
    files = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.npz")))
    assert files
    for f in files:
        z = np.load(f)
        got = _gpu_tables(z["rows"])
        assert_tables_equal(got, {k: z[k] for k in ("edges", "ems", "orders", "ids")}, os.path.basename(f))


@pytest.mark.parametrize("world", [2, 3, 8])
def test_shards_union_equals_single_gpu(oracle, world):
    """Any GPU count gives the same edge list: run every shard (on this one GPU), check each against the cut of the
    oracle's tables it must equal, merge on the device like the N-GPU path does, and compare with the 1-GPU result."""
    import torch
    from muchsalsa_amd import distributed as D, overlap, synth
    from muchsalsa_amd._lib import EDGE_DTYPE, ORDER_DTYPE
    rows = synth.synth_rows(1000, 5000, 4000, 13)
    full = oracle.overlap(rows)
    shards = []
    for r in range(world):
        t = _gpu_tables(rows, shard=r, n_shards=world)
        assert_tables_equal(t, D.shard_view_host(full, r, world), "shard %d/%d" % (r, world))
        shards.append(t)
    counts = np.array([[len(t["edges"]), len(t["orders"]), len(t["ids"])] for t in shards], dtype=np.int64)
    offs, slab_bytes = D.slab_layout(counts.max(axis=0))
    gathered = np.zeros(world * slab_bytes, dtype=np.uint8)
    for r, t in enumerate(shards):
        for name, off in zip(("edges", "orders", "ids"), offs):
            b = t[name].view(np.uint8)
            gathered[r * slab_bytes + off: r * slab_bytes + off + len(b)] = b
    dev = torch.device("cuda", 0)
    d_g = torch.from_numpy(gathered).to(dev)
    tot = counts.sum(axis=0)
    d_e = torch.empty(max(int(tot[0]), 1) * EDGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_o = torch.empty(max(int(tot[1]), 1) * ORDER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_i = torch.empty(max(int(tot[2]), 1) * 4, dtype=torch.uint8, device=dev)
    with overlap.OverlapContext(0) as ctx:
        ctx.merge_gathered(d_g.data_ptr(), counts, slab_bytes, offs, d_e.data_ptr(), d_o.data_ptr(), d_i.data_ptr())
        ctx.synchronize()
    merged = {"edges": d_e.cpu().numpy()[: int(tot[0]) * 32].view(EDGE_DTYPE),
              "orders": d_o.cpu().numpy()[: int(tot[1]) * 64].view(ORDER_DTYPE),
              "ids": d_i.cpu().numpy()[: int(tot[2]) * 4].view("<u4")}
    host = D.merge_tables_host(shards)
    for k in merged:
        assert merged[k].tobytes() == host[k].tobytes(), k
    canon = D.canonicalize(merged)
    want = {k: full[k].copy() for k in ("edges", "orders", "ids")}
    want["edges"]["em_off"] = 0
    canon["edges"]["em_off"] = 0
    canon["ems"] = want["ems"] = np.zeros(0, dtype=full["ems"].dtype)
    assert_tables_equal(canon, want, "merged world=%d" % world)


def test_one_context_goes_from_shard_to_shard_and_back(oracle):
    """The index build classifies the owner reads of the context's shard (the prologue); a later msgpu_calculate_edges for
    another shard writes its own read lists over them.  Back on the first shard the prologue's lists no longer stand: the
    candidate stage must classify again (it once ran the other shard's lists and returned the other shard's tables)."""
    from muchsalsa_amd import distributed as D, overlap, synth
    rows = synth.synth_rows(300, 3000, 900, 1)
    full = oracle.overlap(rows)
    with overlap.OverlapContext(0) as ctx:
        ctx.set_shard(0, 2)
        ctx.load_rows(rows)
        for r in (0, 1, 0, 0, 1):
            ctx.set_shard(r, 2)
            ctx.calculate_edges()
            ctx.chaining_and_overlaps()
            assert_tables_equal(ctx.tables(), D.shard_view_host(full, r, 2), "shard %d of 2" % r)


@pytest.mark.parametrize("world", [1, 3, 8])
def test_wire_form_merge_equals_whole_record_merge(oracle, world):
    """The exchange's wire form (msgpu_pack_wire / msgpu_merge_wire): every shard's tables packed on the GPU equal the host
    statement of the form byte for byte, and the merge of the wire slabs -- with id bases -- is the merge of the whole-record
    slabs, byte for byte (so everything proven for msgpu_merge_gathered holds for it)."""
    import torch
    from muchsalsa_amd import distributed as D, overlap, synth
    from muchsalsa_amd._lib import EDGE_DTYPE, ORDER_DTYPE
    dev = torch.device("cuda", 0)
    shapes = [(1000, 5000, 4000, 13), (120, 20000, 2400, 5)] if world == 1 else [(1000, 5000, 4000, 13)]
    for shape in shapes:
        rows = synth.synth_rows(*shape) if shape[0] == 1000 else synth.accepted_rows(synth.paf_table(*shape, coverage=10))[0]
        full = oracle.overlap(rows)
        shards, blocks = [], []
        for r in range(world):
            with overlap.OverlapContext(0) as ctx:
                ctx.set_shard(r, world)
                ctx.load_rows(rows)
                ctx.calculate_edges()
                ctx.chaining_and_overlaps()
                t = ctx.tables()
                assert_tables_equal(t, D.shard_view_host(full, r, world), "shard %d/%d" % (r, world))
                cnt = (len(t["edges"]), len(t["orders"]), len(t["ids"]))
                per_form = {}
                for ib in (4, 3):  # 4-byte and 3-byte anchor ids
                    nb = D.block_bytes(cnt, wire=ib)
                    assert nb[0] == ctx._L.msgpu_wire_edges_bytes(cnt[0]) and nb[1] == ctx._L.msgpu_wire_orders_bytes(cnt[1])
                    assert nb[2] == ctx._L.msgpu_wire_ids_bytes(cnt[2], ib)
                    d = [torch.full((n + 8,), 0xAB, dtype=torch.uint8, device=dev) for n in nb]
                    # The fills run on torch's stream, the pack kernel on the context's own (non-blocking) stream: without
                    # an order between them the two write the blocks concurrently (round 3's red run: the head of a block
                    # still 0xAB, its tail packed).  include/msgpu.h, STREAM CONTRACT rule 3 -- here: the event way.
                    ts = torch.cuda.current_stream().cuda_stream
                    ctx.stream_wait(ts)
                    ctx.pack_wire(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), id_bytes=ib)
                    ctx.stream_release(ts)
                    got = [x.cpu().numpy() for x in d]
                    want = D.pack_wire_host(t, ib)
                    for name, g, w_, n in zip(("edges", "orders", "ids"), got, want, nb):
                        # (the last word of a 3-byte id block may end in padding the kernel writes as zeros, like the host)
                        assert g[:n].tobytes() == w_.tobytes(), (name, r, ib)
                        assert (g[n:] == 0xAB).all(), (name, r, ib)  # nothing written behind a block
                    back = D.unpack_wire_host(*want, cnt, ib)
                    for k in ("edges", "orders", "ids"):
                        assert back[k].tobytes() == t[k].tobytes(), (k, r, ib)
                    per_form[ib] = want
            shards.append(t)
            blocks.append(per_form)
        counts = np.array([[len(t["edges"]), len(t["orders"]), len(t["ids"])] for t in shards], dtype=np.int64)
        id_base = np.array([[r * 1000, r * 70000] for r in range(world)], dtype="<u4")
        tot = counts.sum(axis=0)
        results = []
        with overlap.OverlapContext(0) as ctx:
            for wire in (False, 4, 3):
                offs, slab_bytes = D.slab_layout(counts.max(axis=0), wire=wire)
                gathered = np.full(world * slab_bytes, 0xCD, dtype=np.uint8)
                for r, t in enumerate(shards):
                    parts = blocks[r][wire] if wire else [t[name].view(np.uint8) for name in ("edges", "orders", "ids")]
                    for b, off in zip(parts, offs):
                        gathered[r * slab_bytes + off: r * slab_bytes + off + len(b)] = b
                d_g = torch.from_numpy(gathered).to(dev)
                d_e = torch.zeros(max(int(tot[0]), 1) * EDGE_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                d_o = torch.zeros(max(int(tot[1]), 1) * ORDER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                d_i = torch.zeros(max(int(tot[2]), 1) * 4, dtype=torch.uint8, device=dev)
                torch.cuda.synchronize()  # STREAM CONTRACT rule 3, the host-wait way: the zero fills are done before the merge is queued
                if wire:
                    ctx.merge_wire(d_g.data_ptr(), counts, slab_bytes, offs, d_e.data_ptr(), d_o.data_ptr(), d_i.data_ptr(),
                                   id_base=id_base, id_bytes=wire)
                else:
                    ctx.merge_gathered(d_g.data_ptr(), counts, slab_bytes, offs, d_e.data_ptr(), d_o.data_ptr(),
                                       d_i.data_ptr(), id_base=id_base)
                ctx.synchronize()
                results.append([x.cpu().numpy().tobytes() for x in (d_e, d_o, d_i)])
        assert int(tot[0]) > 0 and int(tot[1]) > 0
        for form in (1, 2):
            for name, a, b in zip(("edges", "orders", "ids"), results[0], results[form]):
                assert a == b, (name, world, form)


@pytest.mark.parametrize("way", ["set_stream", "events", "events_default_stream", "host_wait"])
def test_stream_contract_caller_buffers(oracle, way):
    """include/msgpu.h, STREAM CONTRACT rule 3: device buffers of the caller are touched in the order of the context's
    stream only.  The caller fills its blocks on ITS stream (torch's), behind 256 MB of other work so that the fill is still
    queued when the library call is made -- the situation in which round 3's wire-form test turned red -- and orders the
    library against it in each of the three documented ways; afterwards it reads the blocks on its own stream again.  Also
    the empty table: its closing CSR entries are on the wire (zeros), nothing else is written."""
    import torch
    from muchsalsa_amd import distributed as D, overlap, synth
    from muchsalsa_amd._lib import EDGE_DTYPE, ORDER_DTYPE
    dev = torch.device("cuda", 0)
    rows = synth.synth_rows(1000, 5000, 4000, 13)
    full = oracle.overlap(rows)
    cnt = (len(full["edges"]), len(full["orders"]), len(full["ids"]))
    want = D.pack_wire_host(full, 3)
    nb = D.block_bytes(cnt, wire=3)
    offs, slab_bytes = D.slab_layout(cnt, wire=3)
    ballast = torch.empty(256 << 20, dtype=torch.uint8, device=dev)
    # the caller's stream: a stream of its own, or (events_default_stream) the legacy default stream, which a non-blocking
    # stream does not synchronise with either (its handle is NULL: msgpu_set_stream cannot name it, the event calls can)
    caller = torch.cuda.Stream(device=dev) if way != "events_default_stream" else torch.cuda.default_stream(dev)
    if way == "events_default_stream":
        way = "events"
    torch.cuda.synchronize()
    with overlap.OverlapContext(0) as ctx, torch.cuda.stream(caller):
        ts = torch.cuda.current_stream().cuda_stream
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        own = ctx.stream()
        assert own and own != ts and (ts != 0) == (caller != torch.cuda.default_stream(dev))
        if way == "set_stream":
            ctx.set_stream(ts)
            assert ctx.stream() == ts
        for it in range(8):
            slab = torch.empty(slab_bytes + 8, dtype=torch.uint8, device=dev)
            out = [torch.empty(max(n, 1) * sz + 8, dtype=torch.uint8, device=dev)
                   for n, sz in zip(cnt, (EDGE_DTYPE.itemsize, ORDER_DTYPE.itemsize, 4))]
            for k in range(4):
                ballast.fill_(k)          # work in front of the fills on the caller's stream
            slab.fill_(0xAB)
            for o in out:
                o.fill_(0xCD)
            if way == "events":
                ctx.stream_wait(ts)
            elif way == "host_wait":
                torch.cuda.synchronize()
            ctx.pack_wire(slab.data_ptr() + offs[0], slab.data_ptr() + offs[1], slab.data_ptr() + offs[2], id_bytes=3)
            ctx.merge_wire(slab.data_ptr(), np.array([cnt], dtype=np.int64), slab_bytes, offs, out[0].data_ptr(),
                           out[1].data_ptr(), out[2].data_ptr(), id_bytes=3)
            if way == "events":
                ctx.stream_release(ts)
            elif way == "host_wait":
                ctx.synchronize()
            got = slab.cpu().numpy()      # on the caller's stream again
            for name, off, w_, n in zip(("edges", "orders", "ids"), offs, want, nb):
                assert got[off: off + n].tobytes() == w_.tobytes(), (way, it, name)
            for name, o, n, sz in zip(("edges", "orders", "ids"), out, cnt, (EDGE_DTYPE.itemsize, ORDER_DTYPE.itemsize, 4)):
                g = o.cpu().numpy()
                assert g[: n * sz].tobytes() == full[name].tobytes(), (way, it, name)
                assert (g[n * sz:] == 0xCD).all(), (way, it, name)
        if way == "set_stream":
            ctx.set_stream(None)
            assert ctx.stream() == own
        # an empty job: 8 + 4 bytes of closing CSR entries, as the host statement has them
        ctx.load_rows(rows[:0])
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        empty = {k: full[k][:0] for k in ("edges", "orders", "ids")}
        d = [torch.full((16,), 0xAB, dtype=torch.uint8, device=dev) for _ in range(3)]
        torch.cuda.synchronize()
        ctx.pack_wire(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), id_bytes=3)
        ctx.synchronize()
        for g, w_ in zip(d, D.pack_wire_host(empty, 3)):
            g = g.cpu().numpy()
            assert g[: len(w_)].tobytes() == w_.tobytes() and (g[len(w_):] == 0xAB).all()


def test_api_state_and_id_checks():
    from muchsalsa_amd import _lib, overlap, synth
    rows = synth.synth_rows(100, 3000, 300, 2)
    with overlap.OverlapContext(0) as ctx:
        with pytest.raises(overlap.MsgpuError) as e:
            ctx.calculate_edges()
        assert e.value.code == _lib.E_STATE
        bad = rows.copy()
        bad["read_id"] = bad["read_id"].max() - bad["read_id"]  # reversed ids: not first-line order
        with pytest.raises(overlap.MsgpuError) as e:
            ctx.load_rows(bad)
        assert e.value.code == _lib.E_IDS
        ctx.load_rows(rows)
        with pytest.raises(overlap.MsgpuError) as e:
            ctx.chaining_and_overlaps()
        assert e.value.code == _lib.E_STATE
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        c = ctx.counts()
        assert c.n_rows_in == len(rows) and c.n_edges > 0 and c.n_orders > 0
        # the context is reusable: a second run gives the same tables
        a = ctx.tables()
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        b = ctx.tables()
        for k in a:
            assert a[k].tobytes() == b[k].tobytes()


def test_declared_id_space(oracle):
    """msgpu_set_id_space: the loader's Registry sizes replace the index build's own pass over the table; wrong
    declarations are refused, a too-large anchor space (anchors without rows) is legal."""
    from muchsalsa_amd import _lib, overlap, synth
    rows = synth.synth_rows(300, 3000, 900, 1)
    want = oracle.overlap(rows)
    V, A = int(rows["read_id"].max()) + 1, int(rows["anchor_id"].max()) + 1

    def run(ctx):
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables()

    with overlap.OverlapContext(0) as ctx:
        ctx.set_id_space(V, A)
        assert_tables_equal(run(ctx), want, "declared")
        ctx.set_id_space(V, A + 5)
        assert_tables_equal(run(ctx), want, "anchor ids without rows")
        for v, a in ((V - 1, A), (V, A - 1), (V + 1, A)):
            ctx.set_id_space(v, a)
            with pytest.raises(overlap.MsgpuError) as e:
                ctx.load_rows(rows)
            assert e.value.code == _lib.E_IDS, (v, a)
        with pytest.raises(overlap.MsgpuError) as e:
            ctx.set_id_space(V, 0)
        assert e.value.code == _lib.E_ARG
        ctx.set_id_space(0, 0)
        assert_tables_equal(run(ctx), want, "discovery again")


def test_property_checks_at_full_size():
    """cfg2-size run checked through size-independent properties (no oracle): table cross references are dense and
    consistent, every order's ids are a subset of its edge's EdgeMatch anchors in vStart order, shards partition."""
    from muchsalsa_amd import synth
    rows = synth.synth_rows(**synth.CONFIGS["cfg2"])
    t = _gpu_tables(rows)
    e, em, o, ids = t["edges"], t["ems"], t["orders"], t["ids"]
    assert np.all(e["v1"] < e["v2"])
    key = e["v1"].astype(np.uint64) << np.uint64(32) | e["v2"].astype(np.uint64)
    assert np.all(key[1:] > key[:-1])  # sorted, unique edges
    assert np.array_equal(e["em_off"], np.concatenate([[0], np.cumsum(e["em_cnt"])[:-1]]))
    assert np.array_equal(e["order_off"], np.concatenate([[0], np.cumsum(e["order_cnt"])[:-1]]))
    assert e["em_cnt"].sum() == len(em) and e["order_cnt"].sum() == len(o) and o["ids_cnt"].sum() == len(ids)
    assert np.array_equal(em["edge_idx"], np.repeat(np.arange(len(e)), e["em_cnt"]))
    assert np.array_equal(o["edge_idx"], np.repeat(np.arange(len(e)), e["order_cnt"]))
    assert np.all(o["base"] == e["v1"][o["edge_idx"]])
    assert np.all(np.where(o["flags"] & 1, o["start"], o["end"]) == e["v1"][o["edge_idx"]])
    assert np.all(em["ov_hi"] - em["ov_lo"] > 100) and np.all(em["score"] > 0)
    assert np.all(o["left_offset"] >= 0) and np.all(o["right_offset"] >= 0)
    assert np.all(e["order_cnt"] >= 1)
    # an edge with more than one order is a shadow (main.cpp:389-391)
    assert np.all(e["shadow"][e["order_cnt"] > 1] == 1)
    # ids of an order: anchors of the edge with the order's direction, ascending vStart position
    rng = np.random.default_rng(0)
    for q in rng.choice(len(o), 2000, replace=False):
        ed = e[o[q]["edge_idx"]]
        anchors = em["anchor_id"][int(ed["em_off"]): int(ed["em_off"]) + int(ed["em_cnt"])]
        flags = em["flags"][int(ed["em_off"]): int(ed["em_off"]) + int(ed["em_cnt"])]
        mine = ids[int(o[q]["ids_off"]): int(o[q]["ids_off"]) + int(o[q]["ids_cnt"])]
        pos = [int(np.nonzero(anchors == a)[0][0]) for a in mine]
        assert pos == sorted(pos) and len(set(pos)) == len(pos)
        assert np.all((flags[pos] & 1) == ((int(o[q]["flags"]) >> 2) & 1))


def test_bench_distributed_path_smoke():
    """bench.py's N>1 step (msgpu_pack_wire -> all-gather over RCCL -> msgpu_merge_wire; with --exchange-format whole:
    copy_tables_device -> all-gather -> msgpu_merge_gathered) at world size 1."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "tiny", "--steps", "2",
                          "--warmup", "1", "--cpu-sample-reads", "0", "--force-dist", "--full"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and line["config"]["edges"] > 0
    assert 0 < line["roofline"]["frac"] < 1
    assert line["config"]["merged_edge_list_consistent"] is True   # all-gather + merge reproduced our own tables
    assert line["consensus"]["verified_against_genome"] is True
    assert line["rccl_ranks"] == 1 and line["rank_ms_per_step"]["min"] > 0
    assert line["exchange"]["collectives_per_step"] < 1.5  # the slab all-gather alone once the capacity is agreed
    # the default N > 1 line: STRONG scaling (BASELINE.json configs[3]: the one job sharded by v1 % N) is `value`; the weak
    # figure (N partitions, the exchange one step behind the compute on its own stream) and the rank-sharded host-to-host
    # figure stand beside it
    assert line["scaling"] == "strong" and line["exchange"]["regrows"] == 0 and "strong" not in line
    wk = line["weak"]
    assert wk["scaling"] == "weak" and wk["exchange"]["regrows"] == 0 and wk["exchange"]["collectives_per_step"] < 1.5
    assert wk["exchange"]["format"].startswith("wire") and wk["exchange"]["slab_bytes"] < 0.7 * wk["exchange"]["whole_record_slab_bytes"]
    assert wk["merged_edge_list_consistent"] is True and wk["value"] > 0
    assert wk["edges"] == line["config"]["edges"]  # (world 1: one partition = the job)
    assert line["host_to_host_sharded"]["edges"] == line["config"]["edges"] and line["host_to_host_sharded"]["ms"] > 0
    # ... and, once the ranks have left their process group, msgpu_group_overlap over the node's devices in a child process
    assert "error" not in line["group_on_node"] and line["group_on_node"]["members"] == 1 and line["group_on_node"]["transport"] == "rccl"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", "tiny", "--steps", "2",
                          "--warmup", "1", "--kernels-only", "--force-dist", "--scaling", "strong", "--exchange-format", "whole"],
                         env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["scaling"] == "strong" and line["config"]["merged_edge_list_consistent"] is True and "strong" not in line


def test_bench_two_and_three_ranks_rehearsal():
    """The N > 1 control flow of bench.py with REAL ranks: RCCL refuses two ranks on one device, so this runs them over gloo
    with every rank on GPU 0 (a rehearsal, labelled so in the line; nothing of it is a measurement) -- weak scaling with the
    communication thread (partitions, id bases in the merge), the strong leg (shards by v1 % N) and the rank-sharded
    host-to-host leg (1/N of the rows per rank + all-gather of the row table) all complete and agree on the edge counts."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    single = None
    for n in (2, 3):
        out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", str(n), "--backend", "gloo",
                              "--single-device", "--workload", "tiny", "--steps", "2", "--warmup", "1", "--kernels-only"],
                             env=env, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, out.stderr[-2000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["n_gpus"] == n and line["scaling"] == "strong" and "rehearsal" in line and line["rccl_ranks"] is None
        assert line["config"]["merged_edge_list_consistent"] is True and line["exchange"]["regrows"] == 0
        assert len(line["rank_ms_per_step"]["per_rank"]) == n
        wk, h = line["weak"], line["host_to_host_sharded"]
        assert wk["merged_edge_list_consistent"] is True and wk["exchange"]["regrows"] == 0
        assert line["config"]["edges"] == h["edges"] > 0
        single = single or line["config"]["edges"]
        assert line["config"]["edges"] == single   # the ONE job has the same edges however many ranks share it
        assert wk["edges"] > (n - 1) * single      # n partitions of that shape


def test_bench_group_on_node_child_process():
    """What `bench.py --gpus N` attaches to its line as "group_on_node": msgpu_group_overlap over the node's devices in a child
    process of rank 0 (tools/group_rehearsal.py --devices ... --json), verified against the host merge of the shard tables on
    every repetition.  One device here; a failure comes back as {"error": ...}, never as an exception."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    got = bench.group_on_node(1, "tiny")
    assert "error" not in got, got
    assert got["members"] == 1 and got["transport"] == "rccl" and got["edges"] > 0 and got["wall_ms"] >= got["compute_ms"] > 0
    assert got["verified"].startswith("merged edge / order / id tables ==")
    bad = bench.group_on_node(1, "no such workload", timeout_s=120)
    assert "error" in bad


def test_bench_starts_its_own_ranks():
    """`python bench.py --gpus N` without a launcher must start the rank processes itself (before touching the GPU) and
    relay rank 0's line: exercised with one rank (--self-launch), which is all a one-GPU box can run."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--self-launch", "--workload",
                          "tiny", "--steps", "2", "--warmup", "1", "--kernels-only"], env=env, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["n_gpus"] == 1 and line["rccl_ranks"] == 1 and line["value"] > 0
    assert line["config"]["merged_edge_list_consistent"] is True


def test_bench_plain_run_and_dumped_outputs(oracle, tmp_path):
    """A plain `bench.py` run (no --full) is the timed steps alone: the line holds the headline figures and none of --full's.
    --dump-outputs writes the tables of the last timed step, and they are the oracle's tables for the same rows."""
    import json
    import os
    import subprocess
    import sys
    from muchsalsa_amd import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", "tiny", "--steps", "3",
                          "--warmup", "1", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == line["unit"] == "overlap-pairs/s" and line["higher_is_better"] is True and line["dtype"] == "int32+f64"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert abs(line["value"] - line["config"]["edges"] / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert not set(line) & {"stage_ms", "roofline", "roofline_stages", "host_to_host", "group", "consensus", "graph_stage",
                            "assemble_path", "tiled_unitigs", "e2e", "cpu_baseline"}
    w = bench.WORKLOADS["tiny"]
    rows, _, _ = synth.accepted_rows(synth.paf_table(w["n_reads"], w["read_len"], w["n_anchors"], w["seed"]))
    want = oracle.overlap(rows)
    assert line["config"]["edges"] == len(want["edges"])
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
    for name in ("edges", "ems", "orders", "ids"):
        t = want[name]
        assert np.load(d / (name + "_count.npy")).tolist() == [len(t)]
        part = t[np.load(d / (name + "_row.npy")).astype(np.int64)]
        if t.dtype.names is None:
            assert np.array_equal(np.load(d / (name + ".npy")), part.astype(np.float64)), name
            continue
        for f in t.dtype.names:
            if f != "pad":
                got = np.load(d / ("%s_%s.npy" % (name, f)))
                assert got.dtype == np.float64 and np.array_equal(got, part[f].astype(np.float64)), (name, f)


def test_group_of_one_over_rccl_equals_single_context(oracle):
    """msgpu_group (one process, the node's GPUs, ONE grouped RCCL all-gather): with one member the whole path -- shard 0 of 1,
    wire-form pack, ncclAllGather through librccl, msgpu_merge_wire, copy-out -- must give the single-context tables bit for bit,
    EdgeMatches on demand from the member's context, and findContractionEdges on the merged list in HBM == the oracle's.  (The
    protocol at world 2 / 3 runs under gloo on the CPU: tests/test_distributed_gloo.py; two members on real GPUs need a
    multi-GPU box.)  A second job on the same group re-uses its communicator and its buffers."""
    from muchsalsa_amd import overlap, synth
    from graphcases import varlen_rows
    with overlap.OverlapGroup([0]) as grp:
        for k, rows in enumerate((synth.synth_rows(1000, 5000, 4000, 13), varlen_rows(400, 2500, 250_000, 2),
                                  synth.synth_rows(300, 3000, 900, 1))):
            want = oracle.overlap(rows)
            t, info = grp.overlap(rows)
            assert info["n_members"] == 1 and info["id_bytes"] == 3 and info["n_ems"] == len(want["ems"]) and not info["rows_sliced"]
            got = dict(t, ems=want["ems"])  # (EdgeMatch tables are not gathered: checked through the member below)
            assert_tables_equal(got, want, "group of one, job %d" % k)
            rl, fl = want["read_len"], want["read_first_line"]
            assert np.array_equal(t["read_len"], rl) and np.array_equal(t["read_first_line"], fl)
            pick = np.array([0, len(want["edges"]) // 2, len(want["edges"]) - 1], dtype="<u4")
            off, ems = grp.member_edgematches(0, pick)
            e = want["edges"]
            assert ems.tobytes() == b"".join(want["ems"][int(e["em_off"][i]): int(e["em_off"][i]) + int(e["em_cnt"][i])].tobytes()
                                             for i in pick)
            co = grp.find_contraction_edges(len(t["edges"]), len(t["orders"]), len(rl))
            assert np.array_equal(co, oracle.find_contraction_edges(want, len(rl)))
            assert info["exchange_ms"] > 0 and info["wall_ms"] >= info["compute_ms"] > 0
    with pytest.raises(overlap.MsgpuError):
        overlap.OverlapGroup([0, 0])  # one member per device
    with pytest.raises(overlap.MsgpuError):
        overlap.OverlapGroup([99])


@pytest.mark.parametrize("members,row_mode", [(2, "sliced"), (3, "sliced"), (8, "sliced"), (3, "replicate")])
def test_group_of_several_members_rehearsed_on_one_gpu(oracle, monkeypatch, members, row_mode):
    """msgpu_group with n > 1 on a box with ONE GPU: MSGPU_GROUP_TRANSPORT=copy carries the all-gather by device-to-device copies
    instead of RCCL and lets the members share the device -- a member thread per shard, v1 % n sharding, the slab layout sized
    by the largest member, msgpu_pack_wire, msgpu_merge_wire with the counts of all members: everything of the n > 1 path but the
    ncclAllGather call itself.  The merged list == the host statement of the merge over the oracle's shard cuts, and, sorted back
    into (v1, v2) order, the single-GPU tables; EdgeMatches from the owning member.  The rows reach the members as a 1/n-th each
    over the link + an all-gather among them (the default with n > 1; 41,322 rows: a ragged last slice with 8 members) or whole to every
    member (MSGPU_GROUP_ROWS=replicate); the merged tables leave as n slices, one per member."""
    from muchsalsa_amd import distributed as D, overlap, synth
    monkeypatch.setenv("MSGPU_GROUP_TRANSPORT", "copy")
    if row_mode == "replicate":
        monkeypatch.setenv("MSGPU_GROUP_ROWS", "replicate")
    rows = synth.synth_rows(1000, 5000, 4000, 13)
    full = oracle.overlap(rows)
    shards = [D.shard_view_host(full, r, members) for r in range(members)]
    host = D.merge_tables_host(shards)
    with overlap.OverlapGroup([0] * members) as grp:
        for rep in range(2):  # (the second call re-uses every buffer)
            t, info = grp.overlap(rows)
            assert info["n_members"] == members and info["n_ems"] == len(full["ems"])
            assert info["rows_sliced"] == (row_mode == "sliced")
            for k in ("edges", "orders", "ids"):
                got = t[k].copy()
                want = host[k].copy()
                assert got.tobytes() == want.tobytes(), (k, rep)
            canon = D.canonicalize({k: t[k] for k in ("edges", "orders", "ids")})
            want = {k: full[k].copy() for k in ("edges", "orders", "ids")}
            want["edges"]["em_off"] = 0
            canon["edges"]["em_off"] = 0
            canon["ems"] = want["ems"] = np.zeros(0, dtype=full["ems"].dtype)
            assert_tables_equal(canon, want, "group of %d" % members)
        # the EdgeMatches of a merged edge live with its owner, at the em_off the merged record carries
        e = t["edges"]
        bounds = np.concatenate([[0], np.cumsum([len(s_["edges"]) for s_ in shards])])
        for m in range(members):
            if bounds[m + 1] > bounds[m]:
                local = np.array([0, bounds[m + 1] - bounds[m] - 1], dtype="<u4")
                off, ems = grp.member_edgematches(m, local)
                rec = e[bounds[m] + local]
                exp = b"".join(shards[m]["ems"][int(o): int(o) + int(c)].tobytes() for o, c in zip(rec["em_off"], rec["em_cnt"]))
                assert ems.tobytes() == exp
    monkeypatch.delenv("MSGPU_GROUP_TRANSPORT")
    with pytest.raises(overlap.MsgpuError):
        overlap.OverlapGroup([0, 0])  # without the rehearsal transport: one member per device


@pytest.mark.parametrize("stall_at", [0, 1])
def test_group_deadline_on_a_stalled_stream(oracle, monkeypatch, stall_at):
    """msgpu_group_set_timeout: a member's stream that stops draining (the test hook queues a sleeping host function on the last
    member's stream -- in front of the row exchange, stall_at 0, or in front of the slab exchange, stall_at 1: what a collective
    that never completes looks like to everything behind it) must end the call with MSGPU_E_TIMEOUT instead of holding the
    caller; the group is usable again once the stream has moved on, with the same tables as before.  Rehearsal transport, two
    members on the one GPU.  The reference's error model: one catch at src/main.cpp:313-315."""
    import time
    from muchsalsa_amd import _lib, overlap, synth
    monkeypatch.setenv("MSGPU_GROUP_TRANSPORT", "copy")
    # page-locked rows, as msgpu_parse_paf hands them over: a copy out of pageable memory is staged by the calling thread
    # and would itself wait behind the stalled stream
    rows = overlap.PinnedRows(synth.synth_rows(1000, 5000, 4000, 13))
    with overlap.OverlapGroup([0, 0]) as grp:
        good, _ = grp.overlap(rows)  # (buffers, first-call allocations)
        grp.set_timeout(250)
        monkeypatch.setenv("MSGPU_GROUP_TEST_STALL_MS", "1500")
        monkeypatch.setenv("MSGPU_GROUP_TEST_STALL_AT", str(stall_at))
        t0 = time.perf_counter()
        with pytest.raises(overlap.MsgpuError) as info:
            grp.overlap(rows)
        dt = time.perf_counter() - t0
        assert info.value.code == _lib.E_TIMEOUT, str(info.value)
        assert "NOT drained" in str(info.value)  # (the stall outlasts deadline + grace: the text says what is still queued)
        assert dt < 1.2, dt                       # 250 ms + 250 ms of grace, not the 1.5 s of the stall
        monkeypatch.delenv("MSGPU_GROUP_TEST_STALL_MS")
        # while the stall lasts the next call gives up as well (its first act is to drain what the last one left) ...
        with pytest.raises(overlap.MsgpuError) as info2:
            grp.overlap(rows)
        assert info2.value.code == _lib.E_TIMEOUT
        # ... and once the stream has moved on the group works again, without a timeout in its way
        time.sleep(1.6)
        grp.set_timeout(0)
        again, _ = grp.overlap(rows)
        for k in ("edges", "orders", "ids"):
            assert again[k].tobytes() == good[k].tobytes(), k
    rows.close()


def test_pipelined_exchange_threaded_regrow_world1():
    """The exchange as a GPU run drives it (RCCL at world 1, communication thread + stream): a rank outgrows the slab
    capacity in two consecutive batches; merged tables == own tables in every batch, and every batch goes out with the slab
    size the unthreaded protocol gives (capacity adopted at a fixed point: tests/scripts/exchange_world1.py)."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29541")
    for wire in ("3", "4"):
        out = subprocess.run([sys.executable, os.path.join(here, "scripts", "exchange_world1.py"), wire], capture_output=True,
                             text=True, timeout=600, env=env)
        assert out.returncode == 0, out.stderr[-3000:]
        line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["ok"] and line["regrows"] == 2


def test_find_contraction_edges_matches_oracle(oracle):
    """findContractionEdges + sanityCheck (main.cpp:416-463, sc.cpp:29-90) on resident tables: reads of mixed length
    give contained orders; the order tables are also run with every contained order promoted to primary (more
    candidates, all four containment cases of sanityCheck) -- through the device-pointer form of the entry point."""
    import torch
    from graphcases import varlen_rows
    from muchsalsa_amd.overlap import OverlapContext
    n_hit = n_cand = 0
    for seed in (1, 2, 3):
        rows = varlen_rows(400, 2500, 250_000, seed)
        ctx = OverlapContext(device=0)
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        t = ctx.tables()
        n_reads = ctx.counts().n_reads
        want = oracle.find_contraction_edges(t, n_reads)
        got = ctx.find_contraction_edges()
        assert np.array_equal(got, want)
        # promoted variant on caller-owned device tables
        t2 = {"edges": t["edges"].copy(), "orders": t["orders"].copy()}
        t2["orders"]["flags"] |= np.where(t2["orders"]["flags"] & 2, 8, 0).astype(np.uint32)
        if seed == 3:  # and with some edges un-shadowed / shadowed
            t2["edges"]["shadow"] ^= (np.arange(len(t2["edges"])) % 3 == 0).astype(np.uint8)
        want2 = oracle.find_contraction_edges(t2, n_reads)
        d_e = torch.from_numpy(t2["edges"].view(np.uint8).copy()).cuda()
        d_o = torch.from_numpy(t2["orders"].view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        got2 = ctx.find_contraction_edges(d_e.data_ptr(), len(t2["edges"]), d_o.data_ptr(), len(t2["orders"]), n_reads)
        assert np.array_equal(got2, want2)
        n_hit += int((want2 >= 0).sum())
        n_cand += int(((t2["orders"]["flags"] & 10) == 10).sum())
        ctx.close()
    assert n_cand > 1000 and 50 < n_hit < n_cand  # both outcomes are well represented


def test_find_contraction_edges_state_and_empty():
    from muchsalsa_amd.overlap import MsgpuError, OverlapContext
    from muchsalsa_amd import _lib
    ctx = OverlapContext(device=0)
    with pytest.raises(MsgpuError) as e:
        ctx.find_contraction_edges()
    assert e.value.code == _lib.E_STATE
    ctx.close()


def test_find_contraction_edges_on_random_graphs(oracle):
    """sanityCheck's four containment cases and both outcomes on tables no overlap run would produce (random pairs,
    random strand / containment / start side, 1-3 orders per edge), through the device-pointer form."""
    import torch
    from test_graph_stage import random_tables
    from muchsalsa_amd.overlap import OverlapContext
    rng = np.random.default_rng(77)
    ctx = OverlapContext(device=0)
    hits = cands = 0
    for trial in range(60):
        n_reads = int(rng.integers(5, 200))
        n_edges = int(rng.integers(n_reads // 2, min(n_reads * 4, n_reads * (n_reads - 1) // 2) + 1))
        t = random_tables(rng, n_reads, n_edges)
        t["orders"]["flags"] |= np.where(rng.integers(0, 2, len(t["orders"])) == 0, 2, 0).astype(np.uint32)  # more contained
        want = oracle.find_contraction_edges(t, n_reads)
        d_e = torch.from_numpy(t["edges"].view(np.uint8).copy()).cuda()
        d_o = torch.from_numpy(t["orders"].view(np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        got = ctx.find_contraction_edges(d_e.data_ptr(), len(t["edges"]), d_o.data_ptr(), len(t["orders"]), n_reads)
        assert np.array_equal(got, want), trial
        hits += int((want >= 0).sum())
        cands += int(((t["orders"]["flags"] & 10) == 10).sum())
    ctx.close()
    assert cands > 2000 and 20 < hits < cands
