"""The mapper on the GPU: every test runs the stage on files and compares, without any tolerance (integers and bytes), with
the plain-Python restatement (tests/map_oracle.py): the PAF byte for byte, the chain table field for field and the counts.
Bad inputs are rejected with an error code; no test provokes a device fault.  Every test runs under its own time limit: a
watchdog ends the process when a stage call does not come back."""
import faulthandler
import os

import pytest

import mapcases

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


def _stage(mp, d, name, **params):
    tp, qp = mapcases.write_inputs(name, d)
    out = os.path.join(str(d), "out.paf")
    tables = {}
    if name.endswith("_ava"):
        params["ava"] = 1
    res = mp.run(tp, qp, out, tables=tables, **params)
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"]
    return res, tables, text


def _check(mp, d, name, **params):
    if name in mapcases.HAND:
        params = dict(mapcases.hand_cases()[name][2], **params)
    want = mapcases.expected(name, **params)
    res, tb, text = _stage(mp, d, name, **params)
    print("%s %r: %d anchors, %d groups (%d kept: %d of at most 16 anchors, %d larger; largest %d), %d chains, histogram %r" % (
        name, params, res["anchors"], res["n_groups"], res["groups_kept"], res["groups_small"], res["groups_large"],
        res["largest_group"], res["chains"], res["group_hist"]))
    for key in ("minimizers", "keys", "keys_dropped", "entries_dropped", "anchors", "n_groups", "groups_kept", "groups_small",
                "groups_large", "largest_group", "group_hist", "below_score", "below_count", "chains_cut", "pairs", "capped"):
        assert res[key] == want[key], key
    assert res["chains"] == len(want["chains"]) and tb["chains"] == want["chains"]
    assert len(text) == len(want["paf"]) and text == want["paf"]
    assert res["bytes_out"] == len(text) and res["lost_publications"] == 0
    assert {k: res["params"][k] for k in want["params"]} == want["params"]
    return res, tb, text, want


@pytest.mark.parametrize("case", mapcases.CASES, ids=mapcases.case_id)
def test_against_the_restatement(mp, tmp_path, case):
    _check(mp, tmp_path, case[0], **case[1])


def test_two_runs_give_the_same_bytes(mp, tmp_path):
    a = _stage(mp, tmp_path, "main", exact=1)[2]
    b = _stage(mp, tmp_path, "main", exact=1)[2]
    assert a == b and len(a) > 0


def test_a_context_serves_a_good_run_after_an_error(mp, tmp_path):
    import ctypes as C
    from muchsalsa_amd import _lib
    L = _lib.lib()
    tp, qp = mapcases.write_inputs("perfect", tmp_path)
    ctx = C.c_void_p()
    assert L.msgpu_map_create(0, C.byref(ctx)) == _lib.OK
    try:
        prm = _lib.MapParams()
        L.msgpu_map_default_params(C.byref(prm))
        assert (prm.k, prm.w, prm.max_occ, prm.max_pred, prm.band) == (15, 5, 200, 64, 64)
        res = C.c_void_p()
        missing = os.fsencode(os.path.join(str(tmp_path), "missing.fa"))
        assert L.msgpu_map_run(ctx, C.byref(prm), missing, os.fsencode(qp), 0, 0, C.byref(res)) == _lib.E_IO and not res.value
        assert b"missing.fa" in L.msgpu_map_last_error(ctx)
        prm.k = 33
        assert L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 0, 0, C.byref(res)) == _lib.E_ARG
        prm.k = 15
        assert L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 1, 0, C.byref(res)) == _lib.E_ARG
        assert L.msgpu_map_run(ctx, C.byref(prm), os.fsencode(tp), os.fsencode(qp), 0, 0, C.byref(res)) == _lib.OK
        n = C.c_uint64()
        p = L.msgpu_map_result_text(res, C.byref(n))
        assert C.string_at(p, n.value) == mapcases.expected("perfect")["paf"]
        L.msgpu_map_result_free(res)
    finally:
        L.msgpu_map_destroy(ctx)


def test_errors_write_nothing(mp, tmp_path):
    from muchsalsa_amd import _lib
    tp, qp = mapcases.write_inputs("perfect", tmp_path)
    out = os.path.join(str(tmp_path), "no.paf")
    for kw in (dict(k=3), dict(k=33), dict(w=0), dict(w=65), dict(max_occ=0), dict(band=0), dict(band=128), dict(exact=2),
               dict(max_gap=-1), dict(ava=1)):  # (ava with two different files)
        with pytest.raises(mp.MapError) as e:
            mp.run(tp, qp, out, **kw)
        assert e.value.code == _lib.E_ARG, kw
    with pytest.raises(mp.MapError) as e:
        mp.run(tp, os.path.join(str(tmp_path), "missing.fa"), out)
    assert e.value.code == _lib.E_IO
    assert not os.path.exists(out)


def test_the_scrubber_accepts_the_mappers_files(mp, tmp_path):
    """the stage's --ava PAF, its seed-mode PAF and the reads -> muchsalsa_amd.scrubber"""
    from muchsalsa_amd import scrubber
    wl = mapcases.workload("tiled")
    reads, unitigs = (os.path.join(str(tmp_path), n) for n in ("reads.fq", "unitigs.fa"))
    for path, key in ((reads, "reads"), (unitigs, "unitigs")):
        with open(path, "wb") as h:
            h.write(wl[key])
    anchors, ava, out = (os.path.join(str(tmp_path), n) for n in ("anchors.paf", "ava.paf", "scrubbed.fa"))
    a = mp.run(reads, unitigs, anchors)
    b = mp.run(reads, reads, ava, ava=1)
    assert a["chains"] > 0 and b["chains"] > 0
    with open(ava, "rb") as h:
        assert all(ln.split(b"\t")[0] != ln.split(b"\t")[5] for ln in h.read().splitlines())
    res = scrubber.run(anchors, reads, out, ava, subset_size=1000)
    print(res)
    assert res["records"] >= 1 and os.path.getsize(out) > 0


def test_the_pipeline_accepts_the_exact_paf(mp, tmp_path):
    """the exact-mode PAF of the tiled workload -> pipeline.run with the workload's files"""
    from muchsalsa_amd import pipeline
    wl = mapcases.workload("tiled")
    reads, unitigs = (os.path.join(str(tmp_path), n) for n in ("reads.fq", "unitigs.fa"))
    for path, key in ((reads, "reads"), (unitigs, "unitigs")):
        with open(path, "wb") as h:
            h.write(wl[key])
    paf = os.path.join(str(tmp_path), "contigs.paf")
    res = mp.run(reads, unitigs, paf, exact=1)
    assert res["chains"] >= 100
    out_dir = os.path.join(str(tmp_path), "out")
    os.mkdir(out_dir)
    got = pipeline.run(paf, unitigs, reads, out_dir)
    print(got)
    assert got["contigs"] >= 1 and os.path.getsize(os.path.join(out_dir, "temp_1.target.fa")) > 0
