"""Bubble popping of the short-read unitig assembly (rule 9) on the GPU: the stage with ``bubble`` set against the plain-Python
restatement (tests/ug_bubble_oracle.py) without any tolerance -- both FASTA texts, the unitig table, the tip rounds, the bubble
rounds (tip rounds in front, bubbles, branches removed, k-mers removed) and the counts -- on the diploid workload and the
hand-made cases of tests/ugbubblecases.py; and what must not depend on the feature: a run with bubble = 0, a context that was
switched on and off again, partitions, one file or two, the mask, a second run.  No test provokes a device fault.  Every test
runs under its own time limit: a watchdog ends the process when a stage call does not come back."""
import ctypes as C
import faulthandler
import os

import pytest

import ug_bubble_oracle as bo
import ugbubblecases as cases
import ugcases

pytestmark = pytest.mark.gpu

LIMIT = 300  # seconds per test
HAND_AT = cases.HAND_AT


@pytest.fixture(scope="module")
def ug():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitigs
    return unitigs


@pytest.fixture(autouse=True)
def time_limit(ug):  # (after ug: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _paths(d, tag="x"):
    return [os.path.join(str(d), tag + "." + n) for n in ("1.fq", "2.fq", "all.fa", "cut.fa")]


def _write(paths, datas):
    for path, data in zip(paths, datas):
        with open(path, "wb") as h:
            h.write(data)


def _read(path):
    with open(path, "rb") as h:
        return h.read()


def _stage(ug, d, k, datas, tag="x", **kw):
    p = _paths(d, tag)
    _write(p, datas)
    tables = {}
    res = ug.run(k, p[0], p[1] if len(datas) > 1 else None, p[2], p[3], device=0, tables=tables, **kw)
    return res, tables, [_read(x) for x in p[2:]]


def _equal(res, tb, texts, want, n_files=1):
    """a result of the stage is the restatement's: both texts, the tables, every count"""
    assert tb["rounds"] == want["rounds"] and res["tip_rounds"] == len(want["rounds"])
    assert [(b[0], b[2], b[3], b[4]) for b in tb["bubble_rounds"]] == [(b[0], b[2], b[3], b[4]) for b in want["bubble_rounds"]]
    assert [b[1] for b in tb["bubble_rounds"]] == [b[1] for b in want["bubble_rounds"]]  # the forks
    assert (res["bubble"], res["bubbles"], res["bubble_kmers"]) == (want["bubble"], want["bubbles"], want["bubble_kmers"])
    assert res["bubble_rounds"] == [[b[0], b[2], b[4]] for b in want["bubble_rounds"]]
    assert (res["records"][:n_files], res["windows"], res["distinct"], res["solid"], res["solid_after"]) == (
        want["records"], want["windows"], want["distinct"], want["solid"], want["solid_after"])
    assert (res["unitigs"], res["kept"], res["cycles"], res["longest"]) == (
        len(want["unitigs"]), want["kept"], want["cycles"], want["longest"])
    assert tb["unitigs"] == want["unitigs"]
    assert len(texts[0]) == len(want["all"]) and len(texts[1]) == len(want["cut"])
    assert texts[0] == want["all"] and texts[1] == want["cut"]
    assert res["bytes_out"] == [len(texts[0]), len(texts[1])] and res["lost_publications"] == 0


def _check(ug, d, name, k, tag="x", **kw):
    want = cases.expected(name, k)[0]
    res, tb, texts = _stage(ug, d, k, [cases.workload(name, k)[0]], tag, **dict(cases.params(name, k), **kw))
    print("%s k %d: tip rounds %r, bubble rounds %r, %d unitigs, longest %d" % (
        name, k, tb["rounds"], tb["bubble_rounds"], res["unitigs"], res["longest"]))
    _equal(res, tb, texts, want)
    return res, tb, texts


@pytest.mark.parametrize("name", cases.DIPLOID)
@pytest.mark.parametrize("k", cases.KS_DIPLOID)
def test_diploid_workload(ug, tmp_path, name, k):
    res, tb, _ = _check(ug, tmp_path, name, k)
    assert res["bubble"] == 3 * k and res["bubbles"] >= 5 and tb["bubble_rounds"][-1][4] == 0
    assert res["unitigs"] < len(cases.plain(name, k)["unitigs"])


@pytest.mark.parametrize("name,k", HAND_AT)
def test_hand_made_cases(ug, tmp_path, name, k):
    res, tb, texts = _check(ug, tmp_path, name, k)
    if name in ("overlapped", "palindrome"):
        assert res["bubble_kmers"] == 0 and texts[0] == cases.plain(name, k)["all"]
    if name == "edge":  # the limit itself: k pops, k - 1 does not
        for bubble in (k, k - 1):
            want = cases.expected(name, k, bubble=bubble)[0]
            r, t, x = _stage(ug, tmp_path, k, [cases.workload(name, k)[0]], "b%d" % bubble, **dict(cases.params(name, k), bubble=bubble))
            _equal(r, t, x, want)
            assert r["bubble_kmers"] == (k if bubble == k else 0)


class _Ctx:
    """one msgpu_ugctx by ctypes: runs by files, and what msgpu_ug_result_bubbles says about each"""

    def __init__(self):
        from muchsalsa_amd import _lib
        self.lib, self.L, self.ctx = _lib, _lib.lib(), C.c_void_p()
        assert self.L.msgpu_ug_create(0, C.byref(self.ctx)) == _lib.OK

    def close(self):
        self.L.msgpu_ug_destroy(self.ctx)

    def set(self, bubble):
        return self.L.msgpu_ug_set_bubbles(self.ctx, bubble)

    def run(self, k, paths, trim=-1, min_length=500, min_count=2):
        """-> (all text, cut text, tip rounds, bubble stats as a dict, bubble rounds)"""
        lib, L, res = self.lib, self.L, C.c_void_p()
        prm = lib.UgParams(k, min_count, trim, min_length)
        rc = L.msgpu_ug_run(self.ctx, C.byref(prm), os.fsencode(paths[0]), None, 0, 0, C.byref(res))
        assert rc == lib.OK, L.msgpu_ug_last_error(self.ctx)
        try:
            n = C.c_uint64()
            texts = [C.string_at(L.msgpu_ug_result_text(res, w, C.byref(n)), n.value) for w in (lib.UG_TEXT_ALL, lib.UG_TEXT_CUT)]
            rp = C.POINTER(lib.UgRound)()
            assert L.msgpu_ug_result_rounds(res, C.byref(rp), C.byref(n)) == lib.OK
            rounds = [(int(rp[i].limit), int(rp[i].removed)) for i in range(n.value)]
            bs, bp = lib.UgBubbleStats(), C.POINTER(lib.UgBubbleRound)()
            assert L.msgpu_ug_result_bubbles(res, C.byref(bs), C.byref(bp), C.byref(n)) == lib.OK
            stats = {name: getattr(bs, name) for name, _ in lib.UgBubbleStats._fields_}
            brounds = [(int(b.after_tip_rounds), int(b.forks), int(b.bubbles), int(b.branches_removed), int(b.removed))
                       for b in (bp[i] for i in range(n.value))]
            st = lib.UgStats()
            L.msgpu_ug_result_stats(res, C.byref(st))
            assert st.n_tip_rounds == len(rounds)
        finally:
            L.msgpu_ug_result_free(res)
        return texts[0], texts[1], rounds, stats, brounds


@pytest.fixture
def ctx(ug):
    c = _Ctx()
    yield c
    c.close()


def _all_zero(stats):
    return all(v == 0 for v in stats.values())


def test_bubble_zero_is_the_plain_stage(ug, ctx, tmp_path):
    """on the unitig tests' own workload and on the diploid one: no bubble argument, bubble = 0, and a context on which
    bubbles were set and reset"""
    small = ugcases.expected("small", 31)
    res, tb, texts = _stage(ug, tmp_path, 31, ugcases.files("small"), "s", bubble=0)
    assert texts == [small["all"], small["cut"]] and tb["rounds"] == small["rounds"] and tb["unitigs"] == small["unitigs"]
    assert (res["bubble"], res["bubbles"], res["bubble_rounds"], res["bubble_kmers"], tb["bubble_rounds"]) == (0, 0, [], 0, [])
    none = _stage(ug, tmp_path, 31, ugcases.files("small"), "n")
    assert none[2] == texts and none[1] == tb and none[0] == res
    want = cases.plain("diploid_err", 31)
    p = _paths(tmp_path, "d")
    _write(p, [cases.workload("diploid_err")[0]])
    fresh = ctx.run(31, p)
    assert fresh[:3] == (want["all"], want["cut"], want["rounds"]) and _all_zero(fresh[3]) and fresh[4] == []
    assert ctx.set(93) == ctx.lib.OK and ctx.set(0) == ctx.lib.OK
    again = ctx.run(31, p)
    assert again[:3] == fresh[:3] and _all_zero(again[3]) and again[4] == []


def test_one_context_with_without_with(ug, ctx, tmp_path):
    on, off = cases.expected("diploid_err", 31)[0], cases.plain("diploid_err", 31)
    p = _paths(tmp_path)
    _write(p, [cases.workload("diploid_err")[0]])
    assert ctx.set(93) == ctx.lib.OK
    first = ctx.run(31, p)
    assert ctx.set(0) == ctx.lib.OK
    second = ctx.run(31, p)
    assert ctx.set(93) == ctx.lib.OK
    third = ctx.run(31, p)
    for key in ("forks_ms", "walk_ms", "adjacency_ms"):  # (times differ from run to run)
        assert first[3].pop(key) > 0 and third[3].pop(key) > 0
    assert first == third and first[:3] == (on["all"], on["cut"], on["rounds"]) and first[4] == on["bubble_rounds"]
    assert first[3] == dict(bubble=93, n_phases=on["bubble_phases"], n_rounds=len(on["bubble_rounds"]), reserved=0,
                            n_bubbles=on["bubbles"], n_branches_removed=on["bubble_branches"], n_kmers_removed=on["bubble_kmers"],
                            max_forks=max(b[1] for b in on["bubble_rounds"]), reserved2=0)
    assert second[:3] == (off["all"], off["cut"], off["rounds"]) and _all_zero(second[3]) and second[4] == []


def test_a_bubble_above_the_cap_is_an_argument_error(ug, ctx, tmp_path):
    on = cases.expected("edge", 21)[0]
    p = _paths(tmp_path)
    _write(p, [cases.workload("edge")[0]])
    assert ctx.set(63) == ctx.lib.OK
    assert ctx.set(4097) == ctx.lib.E_ARG and b"4097" in ctx.L.msgpu_ug_last_error(ctx.ctx)
    got = ctx.run(21, p, min_length=cases.MIN_LENGTH)  # the previous value is in place, and the context serves the run
    assert got[:3] == (on["all"], on["cut"], on["rounds"]) and got[4] == on["bubble_rounds"] and got[3]["bubble"] == 63
    assert ctx.set(4096) == ctx.lib.OK
    assert ctx.run(21, p, min_length=cases.MIN_LENGTH)[0] == on["all"]
    with pytest.raises(ug.UnitigError) as e:
        ug.run(21, p[0], None, p[2], p[3], bubble=4097)
    assert e.value.code == ctx.lib.E_ARG
    with pytest.raises(ug.UnitigError) as e:
        ug.run(21, p[0], None, p[2], p[3], bubble=-1)
    assert e.value.code == ctx.lib.E_ARG and not os.path.exists(p[2])


def _budget_for(ug, d, k, datas, parts, per_key, windows, **kw):
    """a budget (MiB) under which the count cuts the keys into exactly ``parts`` partitions (a bisection: the number the
    stage reports falls as the budget grows)"""
    lo, hi = 0.0, 1.2 * windows * per_key / (1 << 20) + 1
    for _ in range(40):
        mid = (lo + hi) / 2
        try:
            got = _stage(ug, d, k, datas, "b", budget_mb=mid, **kw)[0]["partitions"]
        except ug.UnitigError:  # not even the finest cut fits
            got = 1 << 30
        if got == parts:
            return mid
        if got > parts:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no budget gives %d partitions" % parts)


@pytest.mark.parametrize("k,per_key", [(31, 20), (33, 36)])
def test_partitions_and_files_do_not_change_a_popped_result(ug, tmp_path, k, per_key):
    data = cases.workload("diploid_err")[0]
    want, prm = cases.expected("diploid_err", k)[0], cases.params("diploid_err", k)
    for parts in (1, 3, 8):
        mb = _budget_for(ug, tmp_path, k, [data], parts, per_key, want["windows"], **prm)
        res, tb, texts = _stage(ug, tmp_path, k, [data], "p%d" % parts, budget_mb=mb, **prm)
        assert res["partitions"] == parts
        _equal(res, tb, texts, want)
    recs = data.split(b"\n")
    cut = b"\n".join(recs[:4 * 700]) + b"\n"  # the first 700 records
    res, tb, texts = _stage(ug, tmp_path, k, [cut, data[len(cut):]], "two", **prm)
    _equal(res, tb, texts, dict(want, records=[700, want["records"][0] - 700]), n_files=2)


def test_a_masked_pair_equals_the_files_of_the_kept_records(ug, tmp_path):
    from muchsalsa_amd import kmer_filter
    k, prm = 31, cases.params("diploid_err", 31)
    lines = cases.workload("diploid_err")[0].split(b"\n")[:-1]
    recs = [b"\n".join(lines[i:i + 4]) + b"\n" for i in range(0, len(lines), 4)]
    half = len(recs) // 2
    a, b = recs[:half], recs[half:2 * half]
    mask = bytes(1 if i % 3 == 1 else 0 for i in range(half))
    whole, kept = _paths(tmp_path, "whole"), _paths(tmp_path, "kept")
    _write(whole, [b"".join(a), b"".join(b)])
    _write(kept, [b"".join(r for r, m in zip(x, mask) if not m) for x in (a, b)])
    t_files, t_pair = {}, {}
    by_files = ug.run(k, kept[0], kept[1], kept[2], kept[3], tables=t_files, **prm)
    with kmer_filter.Pair(whole[0], whole[1]) as pair:
        by_pair = ug.run(k, None, None, whole[2], whole[3], pair=pair, dropped=mask, tables=t_pair, **prm)
    assert by_files["bubbles"] >= 5 and t_pair == t_files
    assert [_read(x) for x in whole[2:]] == [_read(x) for x in kept[2:]]
    same = ("windows", "distinct", "solid", "solid_after", "unitigs", "kept", "cycles", "longest", "rounds", "tip_rounds",
            "bytes_out", "bubble", "bubbles", "bubble_rounds", "bubble_kmers")
    assert {key: by_pair[key] for key in same} == {key: by_files[key] for key in same}
    want = bo.run(k, [_read(kept[0]), _read(kept[1])], **prm)
    assert _read(kept[2]) == want["all"] and t_files["bubble_rounds"] == want["bubble_rounds"]


def test_two_runs_give_the_same_bytes(ug, tmp_path):
    data = [cases.workload("diploid_err")[0]]
    a = _stage(ug, tmp_path, 32, data, "r1", **cases.params("diploid_err", 32))
    b = _stage(ug, tmp_path, 32, data, "r2", **cases.params("diploid_err", 32))
    assert a[2] == b[2] and a[1] == b[1] and a[0] == b[0]
    assert a[2][0] == cases.expected("diploid_err", 32)[0]["all"]


def test_the_pipeline_passes_bubble_to_the_unitig_stage(ug, tmp_path):
    import hybridcases
    from muchsalsa_amd import hybrid, kmer_filter
    bubble = 3 * hybridcases.K_ASSEMBLY
    inputs = hybridcases.write_inputs(tmp_path)
    out = str(tmp_path / "out")
    res = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], out,
                     bubble=bubble)
    p, tables = _paths(tmp_path, "direct"), {}
    with kmer_filter.Pair(inputs[0], inputs[1]) as pair:
        kmer_filter.run(hybridcases.K_FILTER, None, None, str(tmp_path / "report.txt"), None, None, pair=pair, tables=tables)
        direct = ug.run(hybridcases.K_ASSEMBLY, None, None, p[2], p[3], pair=pair, dropped=tables["verdict"],
                        min_length=hybrid.MIN_LENGTH, bubble=bubble)
    assert direct["bubble"] == bubble and direct["bubbles"] > 0
    assert {k: v for k, v in res["unitigs"].items() if k != "seconds"} == direct
    assert _read(res["files"]["unitigs"]) == _read(p[2]) and _read(res["files"]["unitigs_cut"]) == _read(p[3])
    assert os.path.getsize(res["files"]["assembly"]) > 0


def test_no_device_memory_is_lost(ug, tmp_path):
    import torch
    p = _paths(tmp_path)
    _write(p, [cases.workload("diploid_err")[0]])

    def cycle():
        c = _Ctx()
        try:
            assert c.set(93) == c.lib.OK
            assert c.run(31, p)[3]["n_bubbles"] >= 5
        finally:
            c.close()

    cycle()  # warm-up: the runtime's pools, the kernels' code objects
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(2):
        cycle()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print("free device memory: %d bytes before the first create, %d after the last destroy" % (before, after))
    assert after >= before
