"""Every stage's edge inputs once more, on device memory that is poisoned and fenced: MSGPU_POISON is set for every test of
this file, so each block of the stages' arena (DevArena, csrc/msgpu_stage.h) comes filled with 0xA5 instead of whatever
hipMalloc returns -- zero pages in a fresh process, an earlier run's own values after it -- and lies between guards that the
stage checks before it returns MSGPU_OK.  The inputs, the comparisons and the expected values are those of the clean files:
this file imports their case modules and calls their checks, so every table and every output byte is compared with the
plain-Python restatements without any tolerance, and a case added to an edge module is run here too.  The only inputs left out
are the workload-sized ones (WORKLOADS).  A difference under poison is a block that a kernel reads before anything wrote it; a
stage error that begins with "arena guard:" is a write outside a block.  That the poison and the guards work is shown by
tests/cpp/test_arena.hip (tests/test_gpu_arena.py), not by damaging a stage.  No test provokes a device fault.  Every test runs
under its own time limit: a watchdog ends the process when a stage call does not come back."""
import ctypes as C
import faulthandler
import os

import pytest

import cigarcases
import extendcases
import kmeredgecases
import mapcases
import mapedgecases
import pledgecases
import plcases
import rankcases
import scrubedgecases
import test_gpu_edit_script as edit_script_tests
import test_gpu_kmer_edges as kmer_edges
import test_gpu_map_extend as extend_tests
import test_gpu_map_rank as rank_tests
import test_gpu_mapper as mapper_tests
import test_gpu_mapper_cigar as cigar_tests
import test_gpu_mapper_edges as mapper_edges
import test_gpu_pair as pair_tests
import test_gpu_polish_edges as polish_edges
import test_gpu_polish_rank as polish_rank
import test_gpu_scrub_uf_edges as scrub_uf_edges
import test_gpu_unitigs_bubble_edges as bubble_edge_tests
import test_gpu_unitigs_bubbles as bubble_tests
import test_mapper_batches_host as batches_host
import ufedgecases
import ugbubblecases
import ugbubbleedgecases

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
# the inputs that are left out: workloads, whose size adds seconds and no edge (tests/test_gpu_fullsize.py is not run here either)
WORKLOADS = ("main", "main_ava", "tiled", "clean")


def _small(cases):
    return [c for c in cases if c[0] not in WORKLOADS]


@pytest.fixture(autouse=True)
def poison(monkeypatch):
    monkeypatch.setenv("MSGPU_POISON", "1")  # (the arena asks per call)


@pytest.fixture(scope="module")
def mods():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import _lib, kmer_filter, mapper, polish, scrubber, unitig_filter, unitigs
    return {"lib": _lib, "kf": kmer_filter, "ug": unitigs, "uf": unitig_filter, "sc": scrubber, "mp": mapper, "pl": polish}


@pytest.fixture(autouse=True)
def time_limit(mods):  # (after mods: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def mp(mods):
    return mods["mp"]


@pytest.fixture(scope="module")
def pl(mods):
    return mods["pl"]


# ---- the k-mer filter and the unitig assembly

@pytest.mark.parametrize("name", [n for n in kmeredgecases.names() if not n.startswith("parts-")])
def test_kmer_edges(mods, tmp_path, name):
    """both stages, 64-bit and 128-bit keys (k <= 32 and k > 32 are different instantiations)"""
    kmer_edges.test_against_the_restatement(mods, tmp_path, name)


@pytest.mark.parametrize("name", kmeredgecases.names(errors=True))
def test_kmer_format_errors(mods, tmp_path, name):
    kmer_edges.test_a_format_error_on_the_line_at_byte_4096(mods, tmp_path, name)


@pytest.mark.parametrize("stage", ["kf", "ug"])
def test_kmer_partitions(mods, tmp_path, stage):
    """the budgeted case: a thousand partitions, each on blocks that the one before it gave back"""
    kmer_edges.test_a_thousand_partitions_do_not_change_the_result(mods, tmp_path, stage)


@pytest.mark.parametrize("name,k", bubble_tests.HAND_AT)
def test_unitig_bubbles(mods, tmp_path, name, k):
    bubble_tests.test_hand_made_cases(mods["ug"], tmp_path, name, k)


@pytest.mark.parametrize("name,k", ugbubbleedgecases.HAND_AT + [ugbubbleedgecases.TANGLE_AT[0], ugbubbleedgecases.TANGLE_AT[-1]])
def test_unitig_bubble_edges(mods, tmp_path, name, k):
    bubble_edge_tests.test_against_the_restatement(mods["ug"], tmp_path, name, k)


@pytest.mark.parametrize("name", ugbubblecases.DIPLOID)
@pytest.mark.parametrize("k", ugbubblecases.KS_DIPLOID)
def test_unitig_bubbles_diploid(mods, tmp_path, name, k):
    bubble_tests.test_diploid_workload(mods["ug"], tmp_path, name, k)


# ---- the coverage filter and the scrubber

@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "2bit"])
@pytest.mark.parametrize("name", ufedgecases.names(pass2=False))
def test_filter_pass1(mods, tmp_path, name, packed):
    scrub_uf_edges.test_filter_pass1(mods, tmp_path, name, packed)


@pytest.mark.parametrize("packed", [False, True], ids=["bytes", "2bit"])
@pytest.mark.parametrize("name", ufedgecases.names(pass2=True))
def test_filter_pass2(mods, tmp_path, name, packed):
    scrub_uf_edges.test_filter_pass2(mods, tmp_path, name, packed)


@pytest.mark.parametrize("name", scrubedgecases.names())
def test_scrubber(mods, tmp_path, name):
    scrub_uf_edges.test_scrubber(mods, tmp_path, name)


# ---- the polisher

@pytest.mark.parametrize("name", pledgecases.names())
def test_polish_edges(pl, tmp_path, name):
    polish_edges.test_edge_case(pl, tmp_path, name)


def test_polish_ranked_two_primaries(pl, tmp_path):
    polish_rank.test_a_read_with_two_primaries_votes_with_both(pl, tmp_path)


def test_polish_ranked_repeat_copies(pl, tmp_path):
    polish_rank.test_a_read_on_two_repeat_copies_votes_at_min_mapq_0_only_and_a_secondary_never(pl, tmp_path)


def test_polish_two_rounds(pl, tmp_path):
    """polish.run(rounds=2) through the mapper, on the draft in three records: the restatement's second round on its first"""
    wl = pledgecases.planted_three_records()
    dp, rp, out = (os.path.join(str(tmp_path), n) for n in ("draft.fa", "reads.fa", "out.fa"))
    with open(dp, "wb") as f:
        f.write(wl["draft"])
    with open(rp, "wb") as f:
        f.write(wl["reads"])
    first, mapped_first = pledgecases.expected_planted_three_records()
    want, mapped = plcases.polish_round(first["text"], wl["reads"])
    tb = {}
    res = pl.run(dp, rp, out, tables=tb, rounds=2)
    assert [r["map"]["chains"] for r in res["rounds"]] == [len(mapped_first["chains"]), len(mapped["chains"])]
    with open(out, "rb") as h:
        text = h.read()
    polish_edges.base._same(pl, res, tb, text, want)


def test_polish_a_smaller_case_behind_a_larger_on_one_context(pl, tmp_path):
    """the context's kept buffers (its sequence store, its scalar block) behind a larger run, and an arena of poisoned blocks
    where a clean process would hand the smaller run the larger one's pages"""
    size = lambda n: sum(len(s) for _, s in pledgecases.cases()[n]["reads"]) + sum(len(s) for _, s in pledgecases.cases()[n]["draft"])
    small, large = sorted(("events_256", "records_300"), key=size)
    assert size(small) < size(large)
    with pl.Context() as ctx:
        a = polish_edges._run(pl, tmp_path, large, context=ctx)
        b = polish_edges._run(pl, tmp_path, small, context=ctx)
    polish_edges._check(pl, a, large)
    polish_edges._check(pl, b, small)


# ---- the mapper

@pytest.mark.parametrize("case", mapedgecases.CASES, ids=mapedgecases.case_id)
def test_mapper_edges(mp, tmp_path, case):
    mapper_edges.test_against_the_restatement(mp, tmp_path, case)


@pytest.mark.parametrize("case", [("small", {}), ("small", dict(exact=1))] + _small(mapcases.CASES), ids=mapcases.case_id)
def test_mapper_cases(mp, tmp_path, case):
    """the small workload with the default parameters in seed and exact mode; of the clean file's list the hand cases and the
    small workload in seed, exact and ava mode at every k, w and threshold"""
    mapper_tests.test_against_the_restatement(mp, tmp_path, case)


@pytest.mark.parametrize("case", _small(cigarcases.CASES), ids=mapcases.case_id)
def test_mapper_cigar(mp, tmp_path, case):
    """the hand cases, the small workload, and the link that reaches the slab class"""
    cigar_tests.test_against_the_restatement(mp, tmp_path, case)


@pytest.fixture(scope="module")
def stage(mp):
    """one mapper context for the table-level tests"""
    from muchsalsa_amd._stage import stage_context
    with stage_context("map", 0, mp.MapError) as st:
        yield st


@pytest.mark.parametrize("name", rankcases.NAMES)
def test_mapper_rank_tables(mp, stage, name):
    rank_tests.test_hand_made_tables(mp, stage, name)


# rule 11 through the mapper: the clean file's cases at the default band (the slab class), and one in the LDS class
EXTEND = _small(extendcases.CASES) + [("ends", dict(band=8), 16)]


@pytest.mark.parametrize("case", EXTEND, ids=lambda c: "%s-%d%s" % (c[0], c[2], "".join("-%s%d" % kv for kv in sorted(c[1].items()))))
def test_mapper_extend(mp, tmp_path, case):
    extend_tests.test_against_the_restatement(mp, tmp_path, case)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("band", extendcases.BANDS)
def test_extend_ends(mods, band, reverse):
    """msgpu_extend_ends on an arena of its own: both table classes, both sides of the LDS class's limit"""
    extend_tests.test_hand_made_pairs(band, reverse)


@pytest.mark.parametrize("name", sorted(cigarcases.pair_lists()))
def test_edit_script(mods, name):
    """msgpu_edit_script on an arena of its own"""
    edit_script_tests.test_words_match_the_restatement(name)


def test_mapper_through_an_index(mp, tmp_path):
    """the index's arena lives as long as the index: built under poison, verified after the build and when it is freed"""
    tp, qp = mapcases.write_inputs("small", tmp_path)
    out = os.path.join(str(tmp_path), "out.paf")
    with mp.Index(tp) as ix:
        for params in ({}, dict(exact=1), dict(ava=1, exact=1)):
            want = mapcases.expected("small_ava" if "ava" in params else "small", **{k: v for k, v in params.items() if k != "ava"})
            tb = {}
            res = mp.run(None, None if "ava" in params else qp, out, tables=tb, index=ix, **params)
            with open(out, "rb") as h:
                assert h.read() == tb["text"] == want["paf"]
            assert tb["chains"] == want["chains"] and res["lost_publications"] == 0
            for key in mapper_edges.KEYS:
                assert res[key] == want[key], key


# ---- the resident pair

def test_pair_filter_then_unitigs(mods, tmp_path, monkeypatch):
    """the pair is uploaded, filtered and assembled on poisoned memory; the reference is the run by files on clean memory"""
    kf, ug = mods["kf"], mods["ug"]
    recs = pair_tests.records(65)
    whole = pair_tests.write(tmp_path, "in", recs)
    with kf.Pair(whole[0], whole[1]) as pair:
        f21 = pair_tests.filter_of(kf, tmp_path, "p21", 21, pair=pair)
        u21 = pair_tests.unitigs_of(ug, tmp_path, "u21", 21, pair=pair, dropped=f21[1]["verdict"])
    with monkeypatch.context() as clean:
        clean.delenv("MSGPU_POISON")
        want_f = pair_tests.filter_of(kf, tmp_path, "f21", 21, in1=whole[0], in2=whole[1])
        want_u = pair_tests.unitigs_of(ug, tmp_path, "w21", 21, in_1=os.path.join(str(tmp_path), "f21.1.fq"),
                                       in_2=os.path.join(str(tmp_path), "f21.2.fq"))
    pair_tests.same_filter(f21, want_f)
    assert isinstance(want_u[0], dict) and isinstance(u21[0], dict), (want_u[0], u21[0])
    for key in pair_tests.SAME:
        assert u21[0][key] == want_u[0][key], key
    assert u21[1] == want_u[1] and u21[2] == want_u[2] and u21[0]["lost_publications"] == 0


# ---- the switch reaches the stage, and moves nothing

def test_the_switch_reaches_the_stage_and_moves_no_figure(mods, tmp_path, monkeypatch):
    """the mapper in batches (a reserved arena) with and without the switch, in this process: the same cut, the same bound and
    the same peak per batch, the same bytes; the poisoned run returns MSGPU_OK with no error text: its guards were checked"""
    _lib = mods["lib"]
    L = _lib.lib()
    one = batches_host.budgets("small", exact=1)[0]
    tp, qp = mapcases.write_inputs("small", tmp_path)
    want = mapcases.expected("small", exact=1)["paf"]

    def run():
        ctx, res, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert L.msgpu_map_create(0, C.byref(ctx)) == _lib.OK
        try:
            prm = _lib.MapParams()
            L.msgpu_map_default_params(C.byref(prm))
            prm.exact = 1
            rc = L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 0, one, C.byref(res))
            err = L.msgpu_map_last_error(ctx)
            assert (rc, err) == (_lib.OK, b"")
            text = C.string_at(L.msgpu_map_result_text(res, C.byref(n)), n.value)
            bp = C.POINTER(_lib.MapBatch)()
            assert L.msgpu_map_result_batches(res, C.byref(bp), C.byref(n)) == _lib.OK
            batches = [{f: int(getattr(bp[i], f)) for f, _ in _lib.MapBatch._fields_} for i in range(n.value)]
            budget = int(L.msgpu_map_result_budget(res))
            L.msgpu_map_result_free(res)
        finally:
            L.msgpu_map_destroy(ctx)
        return text, batches, budget

    assert os.environ.get("MSGPU_POISON") == "1"
    poisoned = run()
    with monkeypatch.context() as clean:
        clean.delenv("MSGPU_POISON")
        plain = run()
    assert poisoned[0] == plain[0] == want
    assert poisoned[1] == plain[1] and len(plain[1]) >= 3 and poisoned[2] == plain[2] == one
    assert all(0 < x["bytes_peak"] <= x["bytes_bound"] for x in plain[1] if x["n_anchors"])
