"""The polishing stage on the GPU: the FASTA byte for byte, the counts and the record table against the plain-Python restatement
(tests/pl_oracle.py; through the mapper: tests/map_oracle.py and tests/map_cigar_oracle.py in front of it), without any
tolerance, on hand-made tables, through the mapper, from the command line and through the pipeline's driver.  No test provokes
a device fault: the tables that break rule 1 must end in an error before a kernel walks a run.  Every test runs under its own
time limit."""
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import pytest

import pl_oracle
import plcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def pl():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import polish
    return polish


@pytest.fixture(autouse=True)
def time_limit(pl):
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _same(pl, res, tb, text, want):
    assert res["lost_publications"] == 0
    assert len(text) == len(want["text"]) and text == want["text"] == tb["text"]
    assert tb["records"] == want["records"]
    assert {k: res[pl._strip(k)] for k in pl_oracle.COUNTS} == {k: want[k] for k in pl_oracle.COUNTS}
    assert res["records"] == len(want["records"]) and res["bases"] == sum(r[0] for r in want["records"])


def _tables(pl, d, c, **how):
    dp, rp = plcases.write_case(c, d)
    out = os.path.join(str(d), "out.fa")
    if os.path.exists(out):
        os.remove(out)
    tb = {}
    res = pl.run_tables(dp, rp, out, c["chains"], c["runs"], tables=tb, **dict(c["params"], **how))
    with open(out, "rb") as h:
        return res, tb, h.read()


@pytest.mark.parametrize("name", plcases.HAND)
def test_hand_made_tables(pl, tmp_path, name):
    c = plcases.hand_cases()[name]
    res, tb, text = _tables(pl, tmp_path, c)
    print(name, c["note"], res)
    _same(pl, res, tb, text, plcases.expected_hand(name))


def test_a_polish_that_changes_nothing_is_the_identity(pl, tmp_path):
    c = plcases.hand_cases()["identity"]
    res, tb, text = _tables(pl, tmp_path, c)
    d = c["draft"][0][1]
    assert text == b">d0\n" + d[:60] + b"\n" + d[60:120] + b"\n" + d[120:] + b"\n" and res["pos_substituted"] == 0


def test_every_rule_1_violation_is_an_error_and_the_context_goes_on(pl, tmp_path):
    """each table that breaks rule 1 -> MSGPU_E_ARG naming the chain and what is wrong, nothing written; the same context then
    polishes a good table correctly"""
    from muchsalsa_amd import _lib
    out = os.path.join(str(tmp_path), "out.fa")
    good = plcases.hand_cases()["strand_1"]
    with pl.Context() as ctx:
        for name, (c, chain, what) in sorted(plcases.violations().items()):
            dp, rp = plcases.write_case(c, tmp_path)
            with pytest.raises(pl.PolishError) as e:
                pl.run_tables(dp, rp, out, c["chains"], c["runs"], context=ctx)
            print(name, e.value)
            assert e.value.code == _lib.E_ARG and "chain %d: %s (" % (chain, what) in str(e.value), name
            assert not os.path.exists(out)
            res, tb, text = _tables(pl, tmp_path, good, context=ctx)
            _same(pl, res, tb, text, plcases.expected_hand("strand_1"))
            os.remove(out)
        for kw in (dict(min_depth=0), dict(min_identity=101), dict(min_identity=-1)):
            with pytest.raises(pl.PolishError) as e:
                _tables(pl, tmp_path, good, context=ctx, **kw)
            assert e.value.code == _lib.E_ARG and "min_" in str(e.value)


def test_two_runs_on_one_context_give_the_same_bytes(pl, tmp_path):
    with pl.Context() as ctx:
        a = _tables(pl, tmp_path, plcases.hand_cases()["many_runs"], context=ctx)
        b = _tables(pl, tmp_path, plcases.hand_cases()["long_run"], context=ctx)
        c = _tables(pl, tmp_path, plcases.hand_cases()["many_runs"], context=ctx)
    assert a[2] == c[2] and a[1] == c[1] and a[0] == c[0]
    _same(pl, *a, plcases.expected_hand("many_runs"))
    _same(pl, *b, plcases.expected_hand("long_run"))


@pytest.fixture(scope="module")
def planted(pl, tmp_path_factory):
    """polish.run on the planted workload, once: (result, tables, text, draft path, reads path, timings)"""
    d = tmp_path_factory.mktemp("planted")
    dp, rp = plcases.write_workload("planted", d)
    out = os.path.join(str(d), "out.fa")
    tb, tm = {}, {}
    res = pl.run(dp, rp, out, tables=tb, timings=tm)
    assert sorted(os.listdir(str(d))) == ["draft.fa", "out.fa", "reads.fa"]  # the round's PAF is gone
    with open(out, "rb") as h:
        return res, tb, h.read(), dp, rp, tm


def test_planted_through_the_mapper(pl, planted):
    res, tb, text = planted[:3]
    want, mapped = plcases.expected_workload("planted")
    print(res, planted[5])
    assert res["rounds"][0]["map"]["chains"] == len(mapped["chains"])
    _same(pl, res, tb, text, want)
    assert res["pos_substituted"] >= 20 and res["pos_deleted"] >= 20 and res["ins_applied"] >= 20


def test_noisy_through_the_mapper(pl, tmp_path):
    dp, rp = plcases.write_workload("noisy", tmp_path)
    out, paf = os.path.join(str(tmp_path), "out.fa"), os.path.join(str(tmp_path), "kept.paf")
    tb, tm = {}, {}
    res = pl.run(dp, rp, out, tables=tb, timings=tm, paf=paf)
    want, mapped = plcases.expected_workload("noisy")
    print(res, tm)
    with open(out, "rb") as h:
        _same(pl, res, tb, h.read(), want)
    with open(paf, "rb") as h:
        assert h.read() == mapped["paf"]
    assert res["ins_usable"] >= 1000 and res["cols_x"] >= 1000 and res["cols_d"] >= 1000  # the error model reached the tables


def test_two_rounds_are_two_runs_of_one_round(pl, planted, tmp_path):
    text1, dp, rp = planted[2:5]
    again, twice = os.path.join(str(tmp_path), "again.fa"), os.path.join(str(tmp_path), "twice.fa")
    pl.run(os.path.join(os.path.dirname(dp), "out.fa"), rp, again)
    res = pl.run(dp, rp, twice, rounds=2)
    assert len(res["rounds"]) == 2 and sorted(os.listdir(str(tmp_path))) == ["again.fa", "twice.fa"]
    with open(again, "rb") as a, open(twice, "rb") as b:
        second = a.read()
        assert second == b.read() and len(second) > 0
    print("round 2 changes the text:", second != text1)


def test_the_command_line_in_a_fresh_process(pl, planted, tmp_path):
    text, dp, rp = planted[2:5]
    out = os.path.join(str(tmp_path), "cli.fa")
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, "-m", "muchsalsa_amd.polish", dp, rp, out, "--min-depth", "3"], cwd=ROOT, env=env,
                         capture_output=True, timeout=LIMIT)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.decode().strip().splitlines()[-1])
    with open(out, "rb") as h:
        assert h.read() == text
    assert line["bytes_out"] == len(text) and line["lost_publications"] == 0 and "pileup" in line["seconds"]
    assert line["params"] == {"min_depth": 3, "min_identity": 0}


def test_the_driver_polishes_on_request(pl, tmp_path):
    """hybrid.run(polish=1) on the hybrid test's workload: the polished file is polish.run's on the two files the run names, and
    every other file is that of a run without polish"""
    import hybridcases
    from muchsalsa_amd import hybrid
    (tmp_path / "in").mkdir()
    inputs = hybridcases.write_inputs(tmp_path / "in")
    res = {}
    for key, kw in (("default", {}), ("polish", dict(polish=1))):
        res[key] = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2],
                              str(tmp_path / key), **kw)
    names = hybrid.output_names(hybridcases.NAME, inputs[2])
    assert set(res["default"]["files"]) == set(names) and "polish" not in res["default"]
    assert set(res["polish"]["files"]) == set(names) | {"polished"}
    assert not os.path.exists(os.path.join(str(tmp_path / "default"), hybrid.POLISHED_NAME))
    for key in names:
        if key == "link":
            continue
        a, b = (open(res[k]["files"][key], "rb").read() for k in ("default", "polish"))
        assert hashlib.sha256(a).digest() == hashlib.sha256(b).digest(), key
    files = res["polish"]["files"]
    assert files["polished"] == os.path.join(os.path.realpath(str(tmp_path / "polish")), hybrid.POLISHED_NAME)
    alone = os.path.join(str(tmp_path), "alone.fa")
    got = pl.run(files["assembly"], files["scrubbed"], alone)
    with open(alone, "rb") as a, open(files["polished"], "rb") as b:
        text = a.read()
        assert text == b.read() and text.startswith(b">")
    print(res["polish"]["polish"])
    skip = ("seconds", "rounds", "bytes_peak")
    assert {k: v for k, v in res["polish"]["polish"].items() if k not in skip} == {k: v for k, v in got.items() if k not in skip}
    assert sorted(os.listdir(os.path.dirname(files["polished"]))) == sorted(os.listdir(str(tmp_path / "default")) + [hybrid.POLISHED_NAME])
