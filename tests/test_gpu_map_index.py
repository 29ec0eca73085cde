"""The mapper index that outlives a run (msgpu_map_index): one index of the reads of the small workload
of tests/mapcases.py serves every run of this file, and each run equals, without any tolerance, ``mapper.run`` by files: the
PAF byte for byte, the chain table field for field, every count and the batches.  The reference is the stage by files, whose
own tests compare it with the restatement.  Bad arguments are rejected with an error code; no test provokes a device fault.
Every test runs under its own time limit."""
import ctypes as C
import faulthandler
import os

import pytest

import mapcases
import test_mapper_batches_host as host

pytestmark = pytest.mark.gpu

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
def files(tmp_path_factory):
    """reads (FASTQ, the targets), the unitigs, and the same unitigs in reverse record order"""
    d = tmp_path_factory.mktemp("map_index")
    reads, unitigs = mapcases.write_inputs("small", d)
    with open(unitigs, "rb") as h:
        recs = [b">" + r for r in h.read().split(b">")[1:]]
    assert len(recs) == mapcases.SMALL["n_unitigs"]
    back = os.path.join(str(d), "unitigs.reversed.fa")
    with open(back, "wb") as h:
        h.write(b"".join(reversed(recs)))
    return {"dir": d, "reads": reads, "unitigs": unitigs, "reversed": back}


@pytest.fixture(scope="module")
def index(mp, files):
    with mp.Index(files["reads"]) as ix:
        yield ix


def run(mp, files, tag, queries, index=None, **kw):
    out = os.path.join(str(files["dir"]), tag + ".paf")
    tables = {}
    res = mp.run(None if index is not None else files["reads"], queries, out, tables=tables, index=index, **kw)
    with open(out, "rb") as h:
        assert h.read() == tables["text"]
    return res, tables


def same(got, want, budget_given=False):
    """every count, the batches, the chain table, the PAF"""
    for key in want[0]:
        if key != "budget_bytes" or budget_given:  # (0 stands for the free memory, which is the run's own)
            assert got[0][key] == want[0][key], key
    assert got[1]["chains"] == want[1]["chains"] and got[1]["text"] == want[1]["text"]
    assert got[0]["lost_publications"] == 0


def one_record_budget(**params):
    """budget (i) of tests/test_gpu_mapper_batches.py: the smallest at which every query record fits a batch on its own"""
    return host.budgets("small", **params)[0] / 2.0 ** 20


def case(files, name):
    """-> (query file, parameters)"""
    if name.startswith("one_record_budget"):
        kw = dict(exact=1) if name.endswith("exact") else {}
        return files["unitigs"], dict(kw, budget_mb=one_record_budget(**kw))
    return {"seed": (files["unitigs"], {}),
            "reversed": (files["reversed"], {}),
            "ava": (None, dict(ava=1)),
            "exact_band8": (files["unitigs"], dict(exact=1, band=8)),
            "max_occ": (files["unitigs"], dict(max_occ=8))}[name]


@pytest.mark.parametrize("name", ["seed", "reversed", "ava", "exact_band8", "max_occ", "one_record_budget", "one_record_budget_exact"])
def test_a_run_on_the_index_equals_the_run_by_files(mp, files, index, name):
    queries, kw = case(files, name)
    want = run(mp, files, "files." + name, files["reads"] if kw.get("ava") else queries, **kw)
    got = run(mp, files, "index." + name, queries, index=index, **kw)
    print("%s: %d anchors, %d chains, %d keys capped, %d batches" % (name, got[0]["anchors"], got[0]["chains"], got[0]["keys_dropped"],
                                                                     len(got[0]["batches"])))
    same(got, want, "budget_mb" in kw)
    assert got[0]["chains"] > 0 and got[0]["records"][0] == mapcases.SMALL["n_reads"] == index.stats["records"]
    assert (got[0]["keys"], got[0]["minimizers"][0]) == (index.stats["keys"], index.stats["minimizers"])
    if name == "max_occ":
        assert got[0]["keys_dropped"] > 0 and got[0]["entries_dropped"] > 8 * got[0]["keys_dropped"]
    if name == "exact_band8":
        assert got[0]["pairs"] > 0 and got[0]["params"]["band"] == 8
    if name.startswith("one_record_budget"):
        assert len(got[0]["batches"]) > 1 and got[0]["records"][1] == mapcases.SMALL["n_unitigs"]
    if name == "reversed":
        fwd = run(mp, files, "index.fwd", files["unitigs"], index=index)
        assert got[0]["chains"] == fwd[0]["chains"] and sorted(got[1]["text"].splitlines()) == sorted(fwd[1]["text"].splitlines())


def test_another_k_is_a_code_and_the_next_run_is_right(mp, files, index):
    from muchsalsa_amd import _lib
    for kw in (dict(k=16), dict(w=6)):
        with pytest.raises(mp.MapError) as e:
            run(mp, files, "bad", files["unitigs"], index=index, **kw)
        assert e.value.code == _lib.E_ARG and "k = 15" in str(e.value) and ("k = 16" in str(e.value) or "w = 6" in str(e.value))
    with pytest.raises(mp.MapError) as e:  # a failure inside the run: the query file is missing
        run(mp, files, "bad", os.path.join(str(files["dir"]), "missing.fa"), index=index)
    assert e.value.code == _lib.E_IO
    with pytest.raises(mp.MapError) as e:  # ava takes no query file
        run(mp, files, "bad", files["unitigs"], index=index, ava=1)
    assert e.value.code == _lib.E_ARG
    assert not os.path.exists(os.path.join(str(files["dir"]), "bad.paf"))
    same(run(mp, files, "index.after", files["unitigs"], index=index), run(mp, files, "files.after", files["unitigs"]))


def test_a_second_create_before_the_free_is_a_state_error(mp, files, index):
    from muchsalsa_amd import _lib
    L, other, prm = _lib.lib(), C.c_void_p(), _lib.MapParams()
    L.msgpu_map_default_params(C.byref(prm))
    assert L.msgpu_map_index_create(index.stage.ctx, C.byref(prm), os.fsencode(files["reads"]), C.byref(other)) == _lib.E_STATE
    assert not other.value and b"free it first" in L.msgpu_map_last_error(index.stage.ctx)
    same(run(mp, files, "index.state", files["unitigs"], index=index), run(mp, files, "files.state", files["unitigs"]))


def test_create_and_free_twice_in_one_context(mp, files):
    want = run(mp, files, "files.twice", files["unitigs"], exact=1)
    with mp.Index(files["reads"]) as ix:
        a = run(mp, files, "index.twice.a", files["unitigs"], index=ix, exact=1)
        first = dict(ix.stats, seconds=None)
        ix.free()
        ix.create()
        b = run(mp, files, "index.twice.b", files["unitigs"], index=ix, exact=1)
        assert dict(ix.stats, seconds=None) == first
    same(a, want)
    same(b, want)
