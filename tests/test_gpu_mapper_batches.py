"""The mapper's batches (rule 9) on the GPU: for every input and every budget the PAF, the chain table and the counts are the
restatement's (tests/map_oracle.py), without any tolerance, and the stage's cut is the greedy cut restated in
tests/test_mapper_batches_host.py.  The budgets are computed from the restatement's per-record anchors and bases and from
msgpu_map_batch_bytes: (i) every record fits on its own, (ii) one batch, (iii) half-way, and 0 (the free device memory).  A
record that does not fit is an error code returned before any batch runs; no test provokes a device fault.  Every test runs
under its own time limit: a watchdog ends the process when a stage call does not come back."""
import ctypes as C
import faulthandler
import json
import os
import subprocess
import sys

import pytest

import mapcases
import test_mapper_batches_host as host

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test

INPUTS = [("small", {}), ("small", dict(exact=1)), ("small_ava", dict(exact=1)), ("tiny", dict(k=4))] + [
    (name, {}) for name in ("perfect", "two_chains", "cut", "empty_queries", "over_max_occ", "short_stretch")]
BUDGETS = ("every record fits", "one batch", "half-way", "free memory")


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


def _params(name, params):
    return dict(mapcases.hand_cases()[name][2], **params) if name in mapcases.HAND else dict(params)


def _budget(name, params, which):
    """-> the budget in bytes (0: the free device memory)"""
    one, whole, half = host.budgets(name, **_params(name, params))
    return {"every record fits": one, "one batch": whole, "half-way": half, "free memory": 0}[which]


def _stage(mp, d, name, budget, **params):
    tp, qp = mapcases.write_inputs(name, d)
    out = os.path.join(str(d), "out.paf")
    tables = {}
    if name.endswith("_ava"):
        params["ava"] = 1
    res = mp.run(tp, qp, out, tables=tables, budget_mb=budget / 2.0 ** 20 if budget else None, **params)
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"]
    return res, tables, text


@pytest.mark.parametrize("which", BUDGETS)
@pytest.mark.parametrize("case", INPUTS, ids=mapcases.case_id)
def test_every_budget_gives_the_restatements_bytes(mp, tmp_path, case, which):
    name, params = case[0], _params(*case)
    want = mapcases.expected(name, **params)
    a, b = host.record_counts(name, **params)
    budget = _budget(name, case[1], which)
    res, tb, text = _stage(mp, tmp_path, name, budget, **params)
    print("%s %r, %s (%d bytes): %d batches, %r" % (name, params, which, res["budget_bytes"], len(res["batches"]), res["batches"]))
    for key in ("minimizers", "keys", "keys_dropped", "entries_dropped", "anchors", "n_groups", "groups_kept", "groups_small",
                "groups_large", "largest_group", "group_hist", "below_score", "below_count", "chains_cut", "pairs", "capped"):
        assert res[key] == want[key], key
    assert res["chains"] == len(want["chains"]) and tb["chains"] == want["chains"]
    assert len(text) == len(want["paf"]) and text == want["paf"]
    assert res["bytes_out"] == len(text) and res["lost_publications"] == 0
    bt = res["batches"]
    if budget:
        assert res["budget_bytes"] == budget
    else:
        assert len(bt) == (1 if a else 0)
        assert res["budget_bytes"] not in (0,) + host.budgets(name, **params)
    # a partition of the query records, in order and without gaps, and the restated cut
    assert res["records"][1] == len(a) and sum(x["n_queries"] for x in bt) == len(a)
    at = 0
    for x in bt:
        assert x["first_query"] == at and x["n_queries"] >= 1
        at += x["n_queries"]
    cut = host.greedy_cut(a, b, host.batch_bytes(params.get("exact", 0)), res["budget_bytes"])
    assert [(x["first_query"], x["n_queries"], x["n_anchors"], x["n_query_bases"]) for x in bt] == cut
    nbytes = host.batch_bytes(params.get("exact", 0))
    for x in bt:
        assert x["bytes_bound"] == nbytes(x["n_anchors"], x["n_query_bases"])
        assert x["bytes_peak"] <= x["bytes_bound"] <= res["budget_bytes"]
        assert (x["bytes_peak"] > 0) == (x["n_anchors"] > 0)
    for key, total in (("n_anchors", "anchors"), ("n_groups", "n_groups"), ("n_chains", "chains"), ("n_pairs", "pairs")):
        assert sum(x[key] for x in bt) == res[total], key
    if which == "every record fits" and name in ("small", "small_ava"):
        assert len(bt) >= 3
    if which == "every record fits" and name in ("small_ava", "short_stretch"):  # a record without anchors rides along
        assert any(sum(a[x["first_query"]:x["first_query"] + x["n_queries"]]) == x["n_anchors"] and
                   0 in a[x["first_query"]:x["first_query"] + x["n_queries"]] for x in bt)


def test_a_record_beyond_the_budget_is_an_error_and_the_context_goes_on(mp, tmp_path):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    a, b = host.record_counts("small")
    one = host.budgets("small")[0]
    heavy = a.index(max(a))
    tp, qp = mapcases.write_inputs("small", tmp_path)
    out = os.path.join(str(tmp_path), "no.paf")
    with pytest.raises(mp.MapError) as e:
        mp.run(tp, qp, out, budget_mb=(one - 1) / 2.0 ** 20)
    print(e.value)
    assert e.value.code == _lib.E_NOMEM
    assert "record %d " % heavy in str(e.value) and "%d anchors" % a[heavy] in str(e.value) and "%d bytes" % (one - 1) in str(e.value)
    assert not os.path.exists(out)
    ctx = C.c_void_p()
    assert L.msgpu_map_create(0, C.byref(ctx)) == _lib.OK
    try:
        prm = _lib.MapParams()
        L.msgpu_map_default_params(C.byref(prm))
        res = C.c_void_p()
        assert L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 0, one - 1, C.byref(res)) == _lib.E_NOMEM
        assert not res.value and b"record %d " % heavy in L.msgpu_map_last_error(ctx)
        assert L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 1, one, C.byref(res)) == _lib.E_ARG
        assert L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 0, one, C.byref(res)) == _lib.OK
        n = C.c_uint64()
        p = L.msgpu_map_result_text(res, C.byref(n))
        assert C.string_at(p, n.value) == mapcases.expected("small")["paf"]
        bp = C.POINTER(_lib.MapBatch)()
        assert L.msgpu_map_result_batches(res, C.byref(bp), C.byref(n)) == _lib.OK and n.value >= 3
        assert L.msgpu_map_result_budget(res) == one
        L.msgpu_map_result_free(res)
    finally:
        L.msgpu_map_destroy(ctx)


def test_runs_and_budgets_give_the_same_bytes(mp, tmp_path):
    one, whole, _ = host.budgets("small", exact=1)
    first = _stage(mp, tmp_path, "small", one, exact=1)
    again = _stage(mp, tmp_path, "small", one, exact=1)
    single = _stage(mp, tmp_path, "small", whole, exact=1)
    assert first[2] == again[2] == single[2] and len(first[2]) > 0
    assert first[1]["chains"] == again[1]["chains"] == single[1]["chains"]
    assert first[0]["batches"] == again[0]["batches"] and len(first[0]["batches"]) >= 3 and len(single[0]["batches"]) == 1


def test_poisoned_batch_buffers_give_the_same_bytes(mp, tmp_path):
    """MSGPU_POISON=1 in a fresh process (the command line): every batch starts on buffers filled with 0xA5, so a buffer that a
    batch reuses without its reset shows"""
    one = host.budgets("small", exact=1)[0]
    tp, qp = mapcases.write_inputs("small", tmp_path)
    out = os.path.join(str(tmp_path), "poison.paf")
    env = dict(os.environ, PYTHONPATH=ROOT, MSGPU_POISON="1")
    run = subprocess.run([sys.executable, "-m", "muchsalsa_amd.mapper", tp, qp, out, "--exact", "--budget-mb", repr(one / 2.0 ** 20)],
                         cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    res = json.loads(run.stdout.decode().strip().splitlines()[-1])
    assert res["budget_bytes"] == one and len(res["batches"]) >= 3
    with open(out, "rb") as h:
        assert h.read() == mapcases.expected("small", exact=1)["paf"]
