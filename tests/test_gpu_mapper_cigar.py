"""The mapper's cigar mode on the GPU (rule 10): the PAF byte for byte, the chain table, the run tables and the counts against
the plain-Python restatement (tests/map_cigar_oracle.py over tests/map_oracle.py), without any tolerance, by files, in batches,
through an index and through the pipeline's driver.  No test provokes a device fault.  Every test runs under its own time
limit."""
import faulthandler
import hashlib
import os

import pytest

import cigarcases
import mapcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test
COUNTS = ("pairs_d0", "pairs_lds", "pairs_slab", "pairs_capped", "max_d", "x_columns", "i_columns", "d_columns", "script_words", "runs")


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


def _stage(mp, d, name, params, cigar=1, **how):
    tp, qp = cigarcases.write_inputs(name, d)
    out = os.path.join(str(d), "out.paf")
    tables = {}
    if "index" in how:
        tp, qp = None, (None if name.endswith("_ava") else qp)
    res = mp.run(tp, qp, out, tables=tables, cigar=cigar, **dict(cigarcases.params_of(name, **params), **how))
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"]
    return res, tables, text


def _same(res, tb, text, want):
    assert res["cigar"] == 1 and res["lost_publications"] == 0
    assert len(text) == len(want["paf"]) and text == want["paf"]
    assert res["chains"] == len(want["chains"]) and tb["chains"] == want["chains"]
    assert tb["runs"] == want["packed"] and tb["cigars"] == want["cigars"]
    got = {"pairs_d0": res["align"]["n_pairs_d0"], "pairs_lds": res["align"]["n_pairs_lds"], "pairs_slab": res["align"]["n_pairs_slab"],
           "pairs_capped": res["align"]["n_pairs_capped"], "runs": res["align"]["n_runs"]}
    got.update({key: res["align"][key] for key in COUNTS if key in res["align"]})
    assert got == want["align"]
    assert res["pairs"] == want["exact"]["pairs"] and res["capped"] == want["exact"]["capped"] == got["pairs_capped"]
    assert res["align"]["lds_max_d"] == 31 and res["align"]["slots"] >= 1 and res["align"]["n_inconsistent"] == 0
    assert res["bytes_out"] == len(text)


@pytest.mark.parametrize("case", cigarcases.CASES, ids=mapcases.case_id)
def test_against_the_restatement(mp, tmp_path, case):
    """clean at band 64 and 8, tiled, small at k = 32 and at (k, w) = (15, 1), main (both strands), main ava, the hand cases, and
    the link of 40 substitutions in 560 bases that reaches the slab class through the mapper"""
    want = cigarcases.expected(case[0], **case[1])
    res, tb, text = _stage(mp, tmp_path, case[0], case[1])
    print("%s %r: %d chains, %r" % (case[0], case[1], res["chains"], res["align"]))
    _same(res, tb, text, want)


def _budgets(mp, name):
    """(i) every record fits, (ii) one batch, (iii) half-way, as tests/test_gpu_mapper_batches.py, with cigar mode's bytes"""
    import ctypes as C
    import test_mapper_batches_host as host
    from muchsalsa_amd import _lib
    a, b = host.record_counts(name, exact=1)
    prm = _lib.MapParams()
    _lib.lib().msgpu_map_default_params(C.byref(prm))
    prm.exact = prm.cigar = 1
    nbytes = lambda x, y: int(_lib.lib().msgpu_map_batch_bytes(C.byref(prm), x, y))
    one, whole = max(nbytes(x, y) for x, y in zip(a, b)), nbytes(sum(a), sum(b))
    return (one, whole, (one + whole) // 2, 0), nbytes


def test_every_budget_gives_the_restatements_bytes(mp, tmp_path):
    want = cigarcases.expected("small")
    budgets, nbytes = _budgets(mp, "small")
    seen = []
    for budget in budgets:
        res, tb, text = _stage(mp, tmp_path, "small", {}, budget_mb=budget / 2.0 ** 20 if budget else None)
        _same(res, tb, text, want)
        bt = res["batches"]
        print("budget %d: %d batches, peaks %r" % (res["budget_bytes"], len(bt), [(x["bytes_peak"], x["bytes_bound"]) for x in bt]))
        for x in bt:
            assert x["bytes_bound"] == nbytes(x["n_anchors"], x["n_query_bases"])
            assert x["bytes_peak"] <= x["bytes_bound"] <= res["budget_bytes"]
        assert sum(x["n_pairs"] for x in bt) == res["pairs"]
        seen.append(len(bt))
    assert seen[0] >= 3 and seen[1] == 1 and seen[3] == 1


def test_through_an_index(mp, tmp_path):
    tp, _ = cigarcases.write_inputs("small", tmp_path)
    with mp.Index(tp) as ix:
        for name in ("small", "small_ava"):
            res, tb, text = _stage(mp, tmp_path, name, {}, index=ix)
            _same(res, tb, text, cigarcases.expected(name))


def test_runs_on_one_context_and_a_run_without_cigar_between_them(mp, tmp_path):
    """two cigar runs on one context give the same bytes, and a run with cigar = 0 on the same context gives exact mode's PAF"""
    tp, _ = cigarcases.write_inputs("main", tmp_path)
    want = cigarcases.expected("main")
    with mp.Index(tp) as ix:
        a = _stage(mp, tmp_path, "main", {}, index=ix)
        b = _stage(mp, tmp_path, "main", {}, index=ix)
        c = _stage(mp, tmp_path, "main", {}, cigar=0, index=ix)
    _same(*a, want)
    assert a[2] == b[2] and a[1] == b[1]
    assert c[2] == want["exact"]["paf"] and c[1]["chains"] == want["exact"]["chains"]
    assert c[0]["cigar"] == 0 and c[1]["runs"] == [] and c[1]["cigars"] == [] and c[0]["align"]["script_words"] == 0


def test_cigar_needs_exact(mp, tmp_path):
    from muchsalsa_amd import _lib
    tp, qp = mapcases.write_inputs("perfect", tmp_path)
    out = os.path.join(str(tmp_path), "no.paf")
    for kw in (dict(cigar=1), dict(cigar=1, exact=0), dict(cigar=2, exact=1)):
        with pytest.raises(mp.MapError) as e:
            mp.run(tp, qp, out, **kw)
        assert e.value.code == _lib.E_ARG and "cigar" in str(e.value), kw
    assert not os.path.exists(out)


def test_the_pipeline_accepts_the_cigar_paf(mp, tmp_path):
    """the cigar PAF of the tiled workload -> pipeline.run with the workload's files"""
    from muchsalsa_amd import pipeline
    wl = mapcases.workload("tiled")
    reads, unitigs = (os.path.join(str(tmp_path), n) for n in ("reads.fq", "unitigs.fa"))
    for path, key in ((reads, "reads"), (unitigs, "unitigs")):
        with open(path, "wb") as h:
            h.write(wl[key])
    paf = os.path.join(str(tmp_path), "contigs.paf")
    res = mp.run(reads, unitigs, paf, exact=1, cigar=1)
    assert res["chains"] >= 100
    with open(paf, "rb") as h:
        assert h.read() == cigarcases.expected("tiled")["paf"]
    out_dir = os.path.join(str(tmp_path), "out")
    os.mkdir(out_dir)
    got = pipeline.run(paf, unitigs, reads, out_dir)
    print(got)
    assert got["contigs"] >= 1 and os.path.getsize(os.path.join(out_dir, "temp_1.target.fa")) > 0


def test_the_driver_passes_cigar_on(mp, tmp_path):
    """hybrid.run(cigar=True) on the hybrid test's workload: every file written before the exact PAF is byte-equal to the default
    run's, the exact PAF's lines agree with the default run's in columns 1-9 and 12 and carry cg:Z:, and the run finishes"""
    import hybridcases
    from muchsalsa_amd import hybrid
    (tmp_path / "in").mkdir()
    inputs = hybridcases.write_inputs(tmp_path / "in")
    res = {}
    for key, kw in (("default", {}), ("cigar", dict(cigar=True))):
        out = str(tmp_path / key)
        res[key] = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out, **kw)
    assert res["cigar"]["map_exact"]["cigar"] == 1 and res["default"]["map_exact"]["cigar"] == 0
    names = hybrid.output_names(hybridcases.NAME, inputs[2])
    before = ("report", "unitigs", "unitigs_cut", "unitigs_paf", "corrected", "corrected_paf", "ava_paf", "scrubbed")
    for key in before:
        a, b = (open(res[k]["files"][key], "rb").read() for k in ("default", "cigar"))
        assert hashlib.sha256(a).digest() == hashlib.sha256(b).digest() and len(a) > 0, key
    assert set(before) < set(names)
    a, b = (open(res[k]["files"]["exact_paf"], "rb").read().splitlines() for k in ("default", "cigar"))
    assert len(a) == len(b) >= 1
    for x, y in zip(a, b):
        x, y = x.split(b"\t"), y.split(b"\t")
        assert x[:9] == y[:9] and x[11] == y[11] and y[-1].startswith(b"cg:Z:") and len(y) == len(x) + 1
    assert res["cigar"]["assembly"]["contigs"] >= 1 and os.path.getsize(res["cigar"]["files"]["assembly"]) > 0
