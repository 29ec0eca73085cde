"""The kernels of the k-mer abundance filter and of the short-read unitig assembly at their edges, on the GPU: the inputs of
tests/kmeredgecases.py (tile phases, record counts and read lengths around the wavefront, the histogram's rows, the
threshold at 5, the table's load, keys with the top bits set and a thousand partitions for k_kf_*; tips of exactly the limits,
the snapshot rule, every degree, cycles of 2 ... 1000 k-mers, hairpins and self-complementary k-mers with 64-bit and 128-bit
keys for k_ug_*) through the stages on files, compared as tests/test_gpu_kmer_filter.py and tests/test_gpu_unitigs.py compare:
every table and every output byte against the plain-Python restatements (tests/kf_oracle.py, tests/ug_oracle.py), without any
tolerance.  The conditions the inputs meet are asserted in tests/test_kmer_edges_host.py.  No test provokes a device fault: the
out-of-memory case is the stage's own size check before any allocation.  Every test runs under its own time limit: a watchdog
ends the process when a stage call does not come back."""
import ctypes as C
import faulthandler
import os

import pytest

import kmeredgecases as E
import test_gpu_kmer_filter as filter_tests
import test_gpu_unitigs as unitig_tests

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def stages():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import kmer_filter, unitigs
    return {"kf": kmer_filter, "ug": unitigs}


@pytest.fixture(autouse=True)
def time_limit(stages):  # (after stages: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _check(stages, d, name, tag="x", budget=None):
    """test_gpu_kmer_filter._check / test_gpu_unitigs._check on a case of kmeredgecases"""
    stage, k, files, params = E.cases()[name]
    mb = None if budget is None else budget / 2.0 ** 20
    if stage == "kf":
        return filter_tests._check(stages["kf"], d, k, files[0], files[1], E.expected(name), tag=tag, budget_mb=mb)[0]
    return unitig_tests._check(stages["ug"], d, k, files, E.expected(name), tag=tag, budget_mb=mb, **E.oracle_params(params))[0]


@pytest.mark.parametrize("name", [n for n in E.names() if not n.startswith("parts-")])
def test_against_the_restatement(stages, tmp_path, name):
    res = _check(stages, tmp_path, name)
    assert res["k"] == E.cases()[name][1] and res["partitions"] == 1


@pytest.mark.parametrize("name", E.names(errors=True))
def test_a_format_error_on_the_line_at_byte_4096(stages, tmp_path, name):
    from muchsalsa_amd import _lib
    stage, k, files, _ = E.cases()[name]
    mod = stages[stage]
    p = (filter_tests if stage == "kf" else unitig_tests)._paths(tmp_path)
    for path, data in zip(p, files):
        with open(path, "wb") as h:
            h.write(data)
    with pytest.raises(mod.KmerFilterError if stage == "kf" else mod.UnitigError) as e:
        if stage == "kf":
            mod.run(k, *p, device=0)
        else:
            mod.run(k, p[0], p[1] if len(files) > 1 else None, p[2], p[3], device=0)
    assert (e.value.code, e.value.file, e.value.line) == (_lib.E_FORMAT,) + E.expected(name)["error"], str(e.value)
    assert not any(os.path.exists(x) for x in p[2:])


@pytest.mark.parametrize("stage", ["kf", "ug"])
def test_a_thousand_partitions_do_not_change_the_result(stages, tmp_path, stage):
    name = "parts-" + stage
    budget, parts, _ = E.parts_budgets(stage, E.K_PARTS[stage])
    one = _check(stages, tmp_path, name, "one")
    many = _check(stages, tmp_path, name, "many", budget)
    print(name, "partitions", many["partitions"], "largest", many["largest_partition"])
    assert one["partitions"] == 1 and many["partitions"] == parts >= 1024
    assert many["largest_partition"] * E.per_key(E.K_PARTS[stage]) <= budget


@pytest.mark.parametrize("stage", ["kf", "ug"])
def test_a_budget_below_the_finest_cut_is_refused(stages, tmp_path, stage):
    """MSGPU_E_NOMEM from the stage's size check, with the sizes in the message; the same context then serves a good run"""
    from muchsalsa_amd import _lib
    L = _lib.lib()
    name = "parts-" + stage
    _, k, files, params = E.cases()[name]
    _, _, below = E.parts_budgets(stage, k)
    want = E.expected(name)
    p = (filter_tests if stage == "kf" else unitig_tests)._paths(tmp_path)
    for path, data in zip(p, files):
        with open(path, "wb") as h:
            h.write(data)
    prm = _lib.UgParams(k, 1, -1, 0)
    head = (k,) if stage == "kf" else (C.byref(prm),)
    ctx, res = C.c_void_p(), C.c_void_p()

    def fn(what):
        return getattr(L, "msgpu_%s_%s" % (stage, what))

    def run(budget):
        return fn("run")(ctx, *head, os.fsencode(p[0]), os.fsencode(p[1]), 0, budget, C.byref(res))

    assert fn("create")(0, C.byref(ctx)) == _lib.OK
    try:
        assert run(below) == _lib.E_NOMEM and not res.value
        msg = fn("last_error")(ctx).decode()
        print(msg)
        sizes = (want["windows"], 8 if k <= 32 else 16, E.per_key(k))
        assert "%d windows of %d-byte keys need %d bytes per window" % sizes in msg
        assert "budget %d bytes" % below in msg and "%d hash bins" % E.BINS in msg
        assert run(below + 1) == _lib.OK and fn("last_error")(ctx) == b""
        n = C.c_uint64()
        if stage == "kf":
            st = _lib.KfStats()
            L.msgpu_kf_result_stats(res, C.byref(st))
            assert (st.n_windows, st.upper, st.n_abundant) == (want["windows"], want["upper"], len(want["abundant"]))
            assert st.n_partitions >= 1024
            for which, text in ((_lib.KF_TEXT_OUT_A, want["out1"]), (_lib.KF_TEXT_OUT_B, want["out2"])):
                assert C.string_at(L.msgpu_kf_result_text(res, which, C.byref(n)), n.value) == text
        else:
            st = _lib.UgStats()
            L.msgpu_ug_result_stats(res, C.byref(st))
            assert (st.n_windows, st.n_solid, st.n_unitigs) == (want["windows"], want["solid"], len(want["unitigs"]))
            assert st.n_partitions >= 1024
            assert C.string_at(L.msgpu_ug_result_text(res, _lib.UG_TEXT_ALL, C.byref(n)), n.value) == want["all"]
        fn("result_free")(res)
    finally:
        fn("destroy")(ctx)
    mod = stages[stage]
    with pytest.raises(mod.KmerFilterError if stage == "kf" else mod.UnitigError) as e:
        _check(stages, tmp_path, name, "low", below)
    assert e.value.code == _lib.E_NOMEM and "bytes per window" in str(e.value)
