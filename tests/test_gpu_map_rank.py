"""Rule 12 (the mapper's primaries, secondaries and mapping quality) on the GPU: msgpu_map_rank_tables on the hand-made tables of
tests/rankcases.py, row for row, and ``mapper.run(..., rank=True)`` in seed, exact, cigar and ava mode, with extension, through an
index and in batches -- PAF bytes, rank rows and counts against the plain-Python restatement (tests/map_rank_oracle.py), without any
tolerance.  No test provokes a device fault: the tables that break the rule's order must end in an error before a ranking kernel
runs.  Every test runs under its own time limit."""
import ctypes as C
import faulthandler
import json
import os
import subprocess
import sys

import pytest

import cigarcases
import extendcases
import map_rank_oracle as ro
import mapcases
import plcases
import rankcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


@pytest.fixture(autouse=True)
def time_limit(mp):
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


@pytest.fixture(scope="module")
def stage(mp):
    """one mapper context for the table-level tests"""
    from muchsalsa_amd._stage import stage_context
    with stage_context("map", 0, mp.MapError) as st:
        yield st


# ---- 1. msgpu_map_rank_tables

def _rows_equal(got, want, chains, what):
    if got != want:
        bad = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: chain %d %r: row %r != %r" % (what, bad, chains[bad], got[bad], want[bad]))


@pytest.mark.parametrize("name", rankcases.NAMES)
def test_hand_made_tables(mp, stage, name):
    chains, note = rankcases.tables()[name]
    want, want_stats = rankcases.expected(name)
    st = {}
    got = mp.rank_tables(chains, context=stage, stats=st)
    print(name, note, st)
    _rows_equal(got, want, chains, name)
    assert {k: st[k] for k in ro.STATS} == want_stats
    assert st["lds_primaries"] == ro.LDS and st["ranking"] == 1 and st["seconds"]["rank"] >= 0


def test_a_table_that_breaks_the_order_is_an_error_and_the_context_goes_on(mp, stage):
    from muchsalsa_amd import _lib
    good, want = rankcases.tables()["sizes"][0], rankcases.expected("sizes")[0]
    for name, (chains, first, word) in sorted(rankcases.bad_tables().items()):
        with pytest.raises(mp.MapError) as e:
            mp.rank_tables(chains, context=stage)
        print(name, e.value)
        assert e.value.code == _lib.E_ARG and "chain %d: " % first in str(e.value) and word in str(e.value), name
        st = {}
        mp.rank_tables([], context=stage, stats=st)
        assert all(st[k] == 0 for k in ro.STATS)
        _rows_equal(mp.rank_tables(good, context=stage), want, good, "behind " + name)


def test_two_calls_on_one_context_give_the_same_rows(mp, stage):
    chains = rankcases.tables()["lds_far"][0]
    assert mp.rank_tables(chains, context=stage) == mp.rank_tables(chains, context=stage) == rankcases.expected("lds_far")[0]


# ---- 2. the mapper

def _ranked(base, chains_for_ranks=None):
    """the restatement's ranked result from an unranked one: rows by the chains as rule 7 leaves them"""
    chains = base["chains"] if chains_for_ranks is None else chains_for_ranks
    rows = ro.rank(chains)
    ro.invariants(chains, rows)
    return rows, ro.ranked_paf(base["paf"], rows), ro.stats(chains, rows)


def _run(mp, d, paths, **kw):
    out = os.path.join(str(d), "out.paf")
    tables = {}
    res = mp.run(paths[0], paths[1], out, tables=tables, **kw)
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"] and res["lost_publications"] == 0 and res["bytes_out"] == len(text)
    return res, tables, text


def _same(res, tb, text, base, rows, paf, stats):
    assert len(text) == len(paf) and text == paf
    assert tb["chains"] == base["chains"]  # the chain table is untouched
    _rows_equal(tb["ranks"], rows, base["chains"], "ranks")
    assert res["ranks"] == rows and {k: res["rank"][k] for k in ro.STATS} == stats
    assert res["rank"]["ranking"] == 1 and res["rank"]["seconds"]["rank"] >= 0


SEED_CASES = [("small", {}), ("small", dict(exact=1)), ("main", {}), ("main_ava", {}), ("small_ava", dict(exact=1)), ("two_chains", {}),
              ("empty_queries", {})]


@pytest.mark.parametrize("case", SEED_CASES, ids=mapcases.case_id)
def test_seed_exact_and_ava_mode(mp, tmp_path, case):
    """the repeat workloads (small: four copies of a repeat family; main) on both sides of the exact switch, reads against
    themselves, two chains of one group, and a run without a chain"""
    name, params = case
    base = mapcases.expected(name, **params)
    rows, paf, stats = _ranked(base)
    kw = dict(mapcases.hand_cases()[name][2], **params) if name in mapcases.HAND else dict(params)
    if name.endswith("_ava"):
        kw["ava"] = 1
    res, tb, text = _run(mp, tmp_path, mapcases.write_inputs(name, tmp_path), rank=True, **kw)
    print(mapcases.case_id(case), res["chains"], res["rank"])
    _same(res, tb, text, base, rows, paf, stats)
    if name in ("small", "main"):
        assert stats["n_secondaries"] > 0 and stats["n_segments_wave"] > 0 and 0 < stats["n_mapq0"]


@pytest.mark.parametrize("case", [("small", dict(k=32)), ("main", {})], ids=mapcases.case_id)
def test_cigar_mode(mp, tmp_path, case):
    name, params = case
    base = cigarcases.expected(name, **params)
    rows, paf, stats = _ranked(base)
    res, tb, text = _run(mp, tmp_path, cigarcases.write_inputs(name, tmp_path), rank=True, cigar=1, **cigarcases.params_of(name, **params))
    _same(res, tb, text, base, rows, paf, stats)
    assert tb["runs"] == base["packed"] and b"\tcg:Z:" in text and b"\ttp:A:" in text  # the run tables are untouched


def test_the_noisy_reads_against_their_draft(mp, tmp_path):
    """plcases' noisy workload (the polisher's input): cigar mode, ranks, counts; the device time is printed beside chain_ms and
    backtrack_ms"""
    base = plcases.expected_workload("noisy")[1]
    rows, paf, stats = _ranked(base)
    timings = {}
    res, tb, text = _run(mp, tmp_path, plcases.write_workload("noisy", tmp_path), rank=True, cigar=1, exact=1, timings=timings)
    _same(res, tb, text, base, rows, paf, stats)
    print("noisy: %d chains, %r; seconds: rank %.6f, chain %.6f, backtrack %.6f" % (res["chains"], stats, res["rank"]["seconds"]["rank"],
                                                                                   timings["chain"], timings["backtrack"]))


def test_with_extension_the_ranks_are_those_without(mp, tmp_path):
    """rule 11 moves the ranges in the PAF; rule 12 read them before: the rows equal those of the run without extension"""
    name, extend = "clean", 300
    base = extendcases.expected(name, extend)
    plain = cigarcases.expected(name)
    rows, paf, stats = _ranked(base, chains_for_ranks=plain["chains"])
    paths = extendcases.write_inputs(name, tmp_path)
    kw = extendcases.params_of(name)
    res, tb, text = _run(mp, tmp_path, paths, rank=True, cigar=1, extend=extend, **kw)
    _same(res, tb, text, base, rows, paf, stats)
    assert tb["ext"] == base["ext"] and tb["runs"] == base["packed"]
    off = _run(mp, tmp_path, paths, rank=True, cigar=1, **kw)
    assert off[1]["ranks"] == rows and off[2] == ro.ranked_paf(plain["paf"], rows)
    assert base["chains"] != plain["chains"]  # (the extension did move ranges)


def test_ranking_off_after_ranking_on_gives_the_old_bytes(mp, tmp_path):
    """on one index: on, off, on; and the setter alone, without the wrapper in between"""
    from muchsalsa_amd import _lib
    from muchsalsa_amd._stage import text_view
    L = _lib.lib()
    name = "small"
    base = mapcases.expected(name)
    rows, paf, stats = _ranked(base)
    tp, qp = mapcases.write_inputs(name, tmp_path)
    with mp.Index(tp) as ix:
        on = _run(mp, tmp_path, (None, qp), rank=True, index=ix)
        _same(*on, base, rows, paf, stats)
        res, tb, text = _run(mp, tmp_path, (None, qp), index=ix)
        assert text == base["paf"] and tb["chains"] == base["chains"] and "ranks" not in tb and "rank" not in res and "ranks" not in res
        assert b"tp:A:" not in text and b"s2:i:" not in text and b"\t255\tcm:i:" in text
        _same(*_run(mp, tmp_path, (None, qp), rank=True, index=ix), base, rows, paf, stats)
        assert L.msgpu_map_set_ranking(ix.stage.ctx, 1) == _lib.OK  # sticky: no setter between this and the run
        prm = mp._params(dict(mp.DEFAULTS))
        with ix.stage.run(C.byref(prm), ix.handle, os.fsencode(qp), 0, 0, fn="run_index") as r:
            assert bytes(text_view(L.msgpu_map_result_text, r)) == paf
            rp, m = C.POINTER(_lib.MapRank)(), C.c_uint64()
            assert L.msgpu_map_result_ranks(r, C.byref(rp), C.byref(m)) == _lib.OK and m.value == len(rows)
            assert [(rp[i].parent, rp[i].sub, rp[i].n_secondary, rp[i].mapq) for i in range(m.value)] == rows
        assert L.msgpu_map_set_ranking(ix.stage.ctx, 0) == _lib.OK
        with ix.stage.run(C.byref(prm), ix.handle, os.fsencode(qp), 0, 0, fn="run_index") as r:
            assert bytes(text_view(L.msgpu_map_result_text, r)) == base["paf"]
            rp, m = C.POINTER(_lib.MapRank)(), C.c_uint64(7)
            rst = _lib.MapRankStats()
            assert L.msgpu_map_result_ranks(r, C.byref(rp), C.byref(m)) == _lib.OK and m.value == 0
            assert L.msgpu_map_result_rank_stats(r, C.byref(rst)) == _lib.OK and rst.ranking == 0 and rst.n_segments == 0
    fresh = _run(mp, tmp_path, (tp, qp))
    assert fresh[2] == base["paf"]


def test_every_query_record_a_batch_of_its_own(mp, tmp_path):
    """the smallest budget at which every query record fits: the unbatched ranks with run-global parents, and
    bytes_peak <= bytes_bound == msgpu_map_batch_bytes_rank(...) <= budget for every batch"""
    import test_mapper_batches_host as host
    from muchsalsa_amd import _lib
    name = "small"
    base = mapcases.expected(name)
    rows, paf, stats = _ranked(base)
    a, b = host.record_counts(name)
    prm = _lib.MapParams()
    _lib.lib().msgpu_map_default_params(C.byref(prm))
    nbytes = lambda x, y: int(_lib.lib().msgpu_map_batch_bytes_rank(C.byref(prm), 0, 1, x, y))
    one = max(nbytes(x, y) for x, y in zip(a, b))
    res, tb, text = _run(mp, tmp_path, mapcases.write_inputs(name, tmp_path), rank=True, budget_mb=one / 2.0 ** 20)
    _same(res, tb, text, base, rows, paf, stats)
    bt = res["batches"]
    print("budget %d: %d batches, peaks %r" % (res["budget_bytes"], len(bt), [(x["bytes_peak"], x["bytes_bound"]) for x in bt][:8]))
    assert len(bt) >= 3 and any(r[0] != i and r[0] >= bt[0]["n_chains"] for i, r in enumerate(rows))  # a parent beyond batch 0
    for x in bt:
        assert x["bytes_bound"] == nbytes(x["n_anchors"], x["n_query_bases"])
        assert x["bytes_peak"] <= x["bytes_bound"] <= res["budget_bytes"]
    whole = _run(mp, tmp_path, mapcases.write_inputs(name, tmp_path), rank=True)[0]["batches"]
    assert len(whole) == 1 and whole[0]["bytes_peak"] <= whole[0]["bytes_bound"] == nbytes(sum(a), sum(b))


def test_the_command_line_in_a_fresh_process(mp, tmp_path):
    tp, qp = mapcases.write_inputs("small", tmp_path)
    out = os.path.join(str(tmp_path), "cli.paf")
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, "-m", "muchsalsa_amd.mapper", tp, qp, out, "--rank"], cwd=ROOT, env=env, capture_output=True,
                         timeout=LIMIT)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.decode().strip().splitlines()[-1])
    rows, paf, stats = _ranked(mapcases.expected("small"))
    with open(out, "rb") as h:
        assert h.read() == paf
    assert {k: line["rank"][k] for k in ro.STATS} == stats and "ranks" not in line and "rank" in line["rank"]["seconds"]
