"""Rule 13 (the mapper's mates) on the GPU: msgpu_map_mate_tables on the hand-made tables of tests/matecases.py, row for row, and
``mapper.run(..., mates=True)`` on a seeded workload of pairs with a two-copy repeat, in seed, rank, cigar and extend mode, through
an index and in batches -- PAF bytes, rows and counts against the plain-Python restatement (tests/map_mate_oracle.py), without any
tolerance.  No test provokes a device fault: the tables that break the rule's conditions must end in an error before a mates kernel
runs.  Every test runs under its own time limit."""
import ctypes as C
import faulthandler
import functools
import os

import pytest

import map_cigar_oracle
import map_extend_oracle
import map_mate_oracle as mo
import map_oracle
import map_rank_oracle
import matecases

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
MIN_SCORE = 40  # (the default of 100 is the score of a perfect 100-base read)


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


# ---- 1. msgpu_map_mate_tables

def _rows_equal(got, want, chains, what):
    if got != want:
        bad = next(i for i in range(len(want)) if got[i] != want[i])
        raise AssertionError("%s: chain %d %r: row %r != %r" % (what, bad, chains[bad], got[bad], want[bad]))


@pytest.mark.parametrize("name", matecases.NAMES)
def test_hand_made_tables(mp, stage, name):
    chains, max_insert, note = matecases.tables()[name]
    want, want_stats = matecases.expected(name)
    st = {}
    got = mp.mate_tables(chains, max_insert=max_insert, context=stage, stats=st)
    print(name, note, st)
    _rows_equal(got, want, chains, name)
    assert {k: st[k] for k in mo.STATS} == want_stats
    assert st["mates"] == 1 and st["max_insert"] == max_insert and st["seconds"]["mates"] >= 0


def test_a_table_that_breaks_the_conditions_is_an_error_and_the_context_goes_on(mp, stage):
    from muchsalsa_amd import _lib
    good, want = matecases.tables()["classes"][0], matecases.expected("classes")[0]
    for name, (chains, first, word) in sorted(matecases.bad_tables().items()):
        with pytest.raises(mp.MapError) as e:
            mp.mate_tables(chains, context=stage)
        print(name, e.value)
        assert e.value.code == _lib.E_ARG and str(e.value).endswith("chain %d: %s" % (first, word)), name
        st = {}
        mp.mate_tables([], context=stage, stats=st)
        assert all(st[k] == 0 for k in mo.STATS)
        _rows_equal(mp.mate_tables(good, context=stage), want, good, "behind " + name)


def test_max_insert_outside_its_range_is_an_error(mp, stage):
    from muchsalsa_amd import _lib
    chains = matecases.tables()["edges"][0]
    for bad in (0, 1 << 31, (1 << 32) - 1):
        with pytest.raises(mp.MapError) as e:
            mp.mate_tables(chains, max_insert=bad, context=stage)
        assert e.value.code == _lib.E_ARG and "max_insert = %d" % bad in str(e.value)
    assert mp.mate_tables(chains, context=stage) == matecases.expected("edges")[0]


def test_two_calls_on_one_context_give_the_same_rows(mp, stage):
    chains = matecases.tables()["classes"][0]
    assert mp.mate_tables(chains, context=stage) == mp.mate_tables(chains, context=stage) == matecases.expected("classes")[0]


# ---- 2. the mapper

@functools.lru_cache(maxsize=None)
def workload():
    from muchsalsa_amd import synth
    return synth.mates_workload(genome=4000, seed=1, coverage=8, read_len=100, insert=300, repeat_len=250, error=0.06)


@pytest.fixture(scope="module")
def paths(mp, tmp_path_factory):
    """the genome as a FASTA file, the two FASTQ files and their interleaved file"""
    d = tmp_path_factory.mktemp("mates")
    w = workload()
    names = {}
    for key, text in (("genome", b">g\n" + w["genome"] + b"\n"), ("illumina_1", w["illumina_1"]), ("illumina_2", w["illumina_2"])):
        names[key] = os.path.join(str(d), key + (".fa" if key == "genome" else ".fq"))
        with open(names[key], "wb") as h:
            h.write(text)
    names["pairs"] = os.path.join(str(d), "interleaved.fq")
    names["n_pairs"] = mp.interleave(names["illumina_1"], names["illumina_2"], names["pairs"])
    with open(names["pairs"], "rb") as h:
        names["queries"] = map_oracle.parse(h.read(), True)
    names["targets"] = [(b"g", w["genome"])]
    assert len(names["queries"]) == 2 * names["n_pairs"]
    return names


@functools.lru_cache(maxsize=None)
def _base(mode, t, q):
    """the restatement's run without mates: seed mode, cigar mode, or cigar mode with extend = 20"""
    t, q = list(t), list(q)
    if mode == "seed":
        return map_oracle.run(t, q, min_score=MIN_SCORE)
    cigar = map_cigar_oracle.cigar_run(t, q, min_score=MIN_SCORE, exact=1)
    return cigar if mode == "cigar" else map_extend_oracle.extend_run(t, q, 20, cigar_result=cigar)


def base_of(paths, mode):
    return _base(mode, tuple(paths["targets"]), tuple(paths["queries"]))


def _run(mp, d, paths, **kw):
    out = os.path.join(str(d), "out.paf")
    tables = {}
    res = mp.run(kw.pop("targets", paths["genome"]), paths["pairs"], out, tables=tables, min_score=MIN_SCORE, **kw)
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"] and res["lost_publications"] == 0 and res["bytes_out"] == len(text)
    return res, tables, text


def _same(res, tb, text, base, n_records, paf=None, max_insert=1000):
    rows, stats = mo.mates(base["chains"], max_insert, n_records=n_records)
    mo.invariants(base["chains"], rows, max_insert)
    want = mo.mated_paf(base["paf"] if paf is None else paf, rows)
    assert len(text) == len(want) and text == want
    assert tb["chains"] == base["chains"]
    _rows_equal(tb["mates"], rows, base["chains"], "mates")
    assert res["mates"] == rows and {k: res["mate"][k] for k in mo.STATS} == stats
    assert res["mate"]["mates"] == 1 and res["mate"]["max_insert"] == max_insert and res["mate"]["seconds"]["mates"] >= 0
    return rows, stats


def test_seed_mode(mp, tmp_path, paths):
    """rows, counts and PAF bytes; at 6 % of substitutions the workload has proper pairs, pairs with one mate mapped and pairs
    without a chain, and reads inside the repeat whose chains on the two copies score alike: there the mate decides"""
    base = base_of(paths, "seed")
    timings = {}
    res, tb, text = _run(mp, tmp_path, paths, mates=True, timings=timings)
    rows, stats = _same(res, tb, text, base, len(paths["queries"]))
    print("%d chains, %r; seconds: mates %.6f, chain %.6f" % (res["chains"], stats, res["mate"]["seconds"]["mates"], timings["chain"]))
    assert stats["n_pairs"] == paths["n_pairs"] and stats["n_proper"] > 100 and stats["n_pairs_lanes16"] > 0 and stats["n_single"] > 0 and stats["n_unmapped"] > 0
    assert stats["n_pairs"] == stats["n_proper"] + stats["n_discordant"] + stats["n_single"] + stats["n_unmapped"]
    ch = base["chains"]
    decided = 0  # a selected chain beside an unselected chain of the same read with the same score
    for i, r in enumerate(rows):
        decided += r[2] == 1 and any(j != i and c[0] == ch[i][0] and c[4] == ch[i][4] and rows[j][2] == 0 for j, c in enumerate(ch))
    assert decided > 0
    assert b"\tpr:A:P\tmi:i:" in text and b"\tpr:A:U\n" in text


def test_mates_off_gives_the_bytes_of_a_run_that_never_heard_of_them(mp, tmp_path, paths):
    """13.6; on one index: on, off, on"""
    base = base_of(paths, "seed")
    with mp.Index(paths["genome"]) as ix:
        _same(*_run(mp, tmp_path, paths, targets=None, mates=True, index=ix), base, len(paths["queries"]))
        res, tb, text = _run(mp, tmp_path, paths, targets=None, index=ix)
        assert text == base["paf"] and tb["chains"] == base["chains"] and "mates" not in tb and "mates" not in res and "mate" not in res
        assert b"pr:A:" not in text
        _same(*_run(mp, tmp_path, paths, targets=None, mates=True, index=ix), base, len(paths["queries"]))
    res, tb, text = _run(mp, tmp_path, paths)
    assert text == base["paf"] and "mates" not in tb


def test_with_ranking(mp, tmp_path, paths):
    base = base_of(paths, "seed")
    ranks = map_rank_oracle.rank(base["chains"])
    res, tb, text = _run(mp, tmp_path, paths, mates=True, rank=True)
    _same(res, tb, text, base, len(paths["queries"]), paf=map_rank_oracle.ranked_paf(base["paf"], ranks))
    assert tb["ranks"] == ranks and b"\ts2:i:0\tpr:A:" in text


def test_cigar_mode(mp, tmp_path, paths):
    base = base_of(paths, "cigar")
    res, tb, text = _run(mp, tmp_path, paths, mates=True, cigar=1, exact=1)
    _same(res, tb, text, base, len(paths["queries"]))
    assert tb["runs"] == base["packed"] and b"\tnb:i:1\tNM:i:" in text and b"\tcg:Z:" in text


def test_with_extension_the_rows_follow_the_extended_ranges(mp, tmp_path, paths):
    """rule 13 reads the table behind rule 11: tlen is that of the extended chains, and differs from the one without"""
    base, plain = base_of(paths, "extend"), base_of(paths, "cigar")
    res, tb, text = _run(mp, tmp_path, paths, mates=True, cigar=1, exact=1, extend=20)
    rows, _ = _same(res, tb, text, base, len(paths["queries"]))
    assert tb["ext"] == base["ext"] and tb["runs"] == base["packed"]
    before, _ = mo.mates(plain["chains"], 1000, n_records=len(paths["queries"]))
    moved = [i for i, (a, b) in enumerate(zip(rows, before)) if a[2] == b[2] == 1 and a[0] == b[0] and a[1] != b[1]]
    assert moved, "no pair whose tlen changes under the extension"
    i = moved[0]
    j = rows[i][0]
    f, r = (i, j) if base["chains"][i][2] == 0 else (j, i)
    assert rows[i][1] == base["chains"][r][9] - base["chains"][f][8] != plain["chains"][r][9] - plain["chains"][f][8] == before[i][1]


def test_batches_hold_whole_pairs(mp, tmp_path, paths):
    """a budget that gives at least three batches: every batch starts at an even record and holds an even number of them,
    bytes_peak <= bytes_bound == msgpu_map_batch_bytes_mates(...) <= budget, and the lines are the one-batch run's"""
    from muchsalsa_amd import _lib
    base = base_of(paths, "seed")
    prm = mp._params(dict(mp.DEFAULTS, min_score=MIN_SCORE))
    nbytes = lambda a, b: int(_lib.lib().msgpu_map_batch_bytes_mates(C.byref(prm), 0, 0, 1, a, b))
    whole = _run(mp, tmp_path, paths, mates=True)
    assert len(whole[0]["batches"]) == 1
    total = whole[0]["batches"][0]["n_anchors"]
    budget = nbytes(total // 4, 0)
    res, tb, text = _run(mp, tmp_path, paths, mates=True, budget_mb=budget / 2.0 ** 20)
    _same(res, tb, text, base, len(paths["queries"]))
    assert text == whole[2] and tb["mates"] == whole[1]["mates"]
    bt = res["batches"]
    print("budget %d: %d batches %r" % (res["budget_bytes"], len(bt), [(x["first_query"], x["n_queries"], x["bytes_peak"], x["bytes_bound"]) for x in bt]))
    assert len(bt) >= 3 and sum(x["n_queries"] for x in bt) == len(paths["queries"])
    assert any(r[2] == 1 and r[0] >= bt[0]["n_chains"] for r in tb["mates"])  # a mate beyond batch 0: the base is added
    for x in bt:
        assert x["first_query"] % 2 == 0 and x["n_queries"] % 2 == 0
        assert x["bytes_bound"] == nbytes(x["n_anchors"], x["n_query_bases"]) and x["bytes_peak"] <= x["bytes_bound"] <= res["budget_bytes"]
    # the restatement's cut by pairs, on the anchors of rules 1 to 4 of the restatement
    p = base["params"]
    index = map_oracle.build_index(paths["targets"], p["k"], p["w"], p["max_occ"])[0]
    a = [0] * len(paths["queries"])
    for (q, _, _), g in map_oracle.anchors(index, paths["queries"], p["k"], p["w"], 0).items():
        a[q] += len(g)
    want = mo.cut(nbytes, a, [len(s) for _, s in paths["queries"]], res["budget_bytes"])
    assert [(x["first_query"], x["n_queries"], x["n_anchors"], x["n_query_bases"], x["bytes_bound"]) for x in bt] == want


def test_a_pair_beyond_the_budget_is_named(mp, tmp_path, paths):
    from muchsalsa_amd import _lib
    with pytest.raises(mp.MapError) as e:
        _run(mp, tmp_path, paths, mates=True, budget_mb=(1 << 20) / 2.0 ** 20)
    print(e.value)
    assert e.value.code == _lib.E_NOMEM and "pair " in str(e.value) and "rule 13" in str(e.value)


def test_arguments_that_rule_13_refuses(mp, tmp_path, paths):
    from muchsalsa_amd import _lib
    odd = os.path.join(str(tmp_path), "odd.fq")
    with open(paths["pairs"], "rb") as h:
        lines = h.read().split(b"\n")
    with open(odd, "wb") as h:
        h.write(b"\n".join(lines[:4 * 7]) + b"\n")
    out = os.path.join(str(tmp_path), "never.paf")
    with pytest.raises(mp.MapError) as e:
        mp.run(paths["genome"], odd, out, mates=True, min_score=MIN_SCORE)
    assert e.value.code == _lib.E_ARG and "7 query records" in str(e.value)
    with pytest.raises(mp.MapError) as e:
        mp.run(paths["genome"], paths["genome"], out, mates=True, ava=1)
    assert e.value.code == _lib.E_ARG and "ava" in str(e.value)
    assert not os.path.exists(out)
    base = base_of(paths, "seed")
    with mp.Index(paths["genome"]) as ix:
        _same(*_run(mp, tmp_path, paths, targets=None, mates=True, max_insert=250, index=ix), base, len(paths["queries"]), max_insert=250)
        with pytest.raises(mp.MapError) as e:
            mp.run(None, paths["pairs"], out, index=ix, mates=True, max_insert=0, min_score=MIN_SCORE)
        assert e.value.code == _lib.E_ARG and "max_insert = 0" in str(e.value)
        # the previous value stays: a run by the C entry, without the wrapper's setter in between
        from muchsalsa_amd._stage import text_view
        prm = mp._params(dict(mp.DEFAULTS, min_score=MIN_SCORE))
        with ix.stage.run(C.byref(prm), ix.handle, os.fsencode(paths["pairs"]), 0, 0, fn="run_index") as r:
            rows, _ = mo.mates(base["chains"], 250, n_records=len(paths["queries"]))
            assert bytes(text_view(_lib.lib().msgpu_map_result_text, r)) == mo.mated_paf(base["paf"], rows)
            mst = _lib.MapMateStats()
            assert _lib.lib().msgpu_map_result_mate_stats(r, C.byref(mst)) == _lib.OK and mst.mates == 1 and mst.max_insert == 250
