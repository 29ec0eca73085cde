"""Short-read unitig assembly on the GPU: every test runs the stage on files and compares, without any tolerance (integers
and bytes), with the plain-Python restatement (tests/ug_oracle.py): both FASTA texts, the per-unitig table, the rounds table
and the counts.  Malformed inputs are rejected by the stage's check kernel with an error code; no test provokes a device
fault.  Every test runs under its own time limit: a watchdog ends the process when a stage call does not come back."""
import faulthandler
import json
import math
import os
import subprocess
import sys

import pytest

import kf_oracle
import ug_oracle
import ugcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test


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


def _stage(ug, d, k, datas, tag="x", **kw):
    p = _paths(d, tag)
    for path, data in zip(p, datas):
        with open(path, "wb") as h:
            h.write(data)
    tables = {}
    res = ug.run(k, p[0], p[1] if len(datas) > 1 else None, p[2], p[3], device=0, tables=tables, **kw)
    texts = []
    for path in p[2:]:
        with open(path, "rb") as h:
            texts.append(h.read())
    return res, tables, texts


def _check(ug, d, k, datas, want=None, tag="x", budget_mb=None, **kw):
    """the stage against the restatement: both texts, both tables, every count"""
    want = ug_oracle.run(k, datas, **kw) if want is None else want
    res, tb, (all_text, cut_text) = _stage(ug, d, k, datas, tag, budget_mb=budget_mb, **kw)
    print("k %d: rounds %r, %d unitigs (%d kept, %d cycles), longest %d, doubling rounds %d" % (
        k, tb["rounds"], res["unitigs"], res["kept"], res["cycles"], res["longest"], res["doubling_rounds"]))
    assert tb["rounds"] == want["rounds"] and res["tip_rounds"] == len(want["rounds"])
    assert (res["records"][:len(datas)], res["windows"], res["distinct"], res["solid"], res["solid_after"]) == (
        want["records"], want["windows"], want["distinct"], want["solid"], want["solid_after"])
    assert (res["unitigs"], res["kept"], res["cycles"], res["longest"]) == (
        len(want["unitigs"]), want["kept"], want["cycles"], want["longest"])
    assert tb["unitigs"] == want["unitigs"]
    assert len(all_text) == len(want["all"]) and len(cut_text) == len(want["cut"])
    assert all_text == want["all"] and cut_text == want["cut"]
    assert res["bytes_out"] == [len(all_text), len(cut_text)] and res["lost_publications"] == 0
    return res, tb, want


@pytest.mark.parametrize("k", (2,) + ugcases.KS_SMALL)
def test_small_workload(ug, tmp_path, k):
    name = "tiny" if k == 2 else "small"
    res, _, want = _check(ug, tmp_path, k, ugcases.files(name), ugcases.expected(name, k))
    assert res["k"] == k and res["trim"] == k and res["partitions"] == 1
    if k > 2:
        assert 0 < res["kept"] < res["unitigs"] and res["solid_after"] < res["solid"] < res["distinct"]


@pytest.mark.parametrize("name", ugcases.HAND)
@pytest.mark.parametrize("k", ugcases.KS_HAND)
def test_hand_made_cases(ug, tmp_path, name, k):
    res, _, _ = _check(ug, tmp_path, k, ugcases.files(name), ugcases.expected(name, k, min_length=100), min_length=100)
    if name == "rings":
        assert res["cycles"] == 2 and res["longest"] == 300


@pytest.mark.parametrize("min_count", (1, 2, 3))
def test_min_count(ug, tmp_path, min_count):
    res, _, _ = _check(ug, tmp_path, 31, ugcases.files("small"), ugcases.expected("small", 31, min_count=min_count),
                       min_count=min_count)
    assert res["min_count"] == min_count


@pytest.mark.parametrize("k,trim", [(31, 0), (31, 1), (31, 16), (31, 31), (50, 7), (21, 40)])
def test_trim(ug, tmp_path, k, trim):
    res, tb, _ = _check(ug, tmp_path, k, ugcases.files("small"), ugcases.expected("small", k, trim=trim), trim=trim)
    assert res["trim"] == trim and [l for l, _ in tb["rounds"]][:len(ug_oracle.tip_limits(trim))] == ug_oracle.tip_limits(trim)


def test_min_length_splits_the_set(ug, tmp_path):
    a, _, _ = _check(ug, tmp_path, 31, ugcases.files("small"), ugcases.expected("small", 31, min_length=200), tag="a",
                     min_length=200)
    b, _, _ = _check(ug, tmp_path, 31, ugcases.files("small"), ugcases.expected("small", 31, min_length=1), tag="b",
                     min_length=1)
    assert 0 < a["kept"] < a["unitigs"] == b["kept"]


def test_one_file_or_two_is_the_same(ug, tmp_path):
    a, b = ugcases.files("small")
    want = ugcases.expected("small", 31)
    recs = a.split(b"\n")
    cut = b"\n".join(recs[:4 * 1000]) + b"\n"  # the first 1000 records
    assert a.startswith(cut)
    _, t1, (all1, cut1) = _stage(ug, tmp_path, 31, [a + b], "one")
    _, t2, (all2, cut2) = _stage(ug, tmp_path, 31, [cut, a[len(cut):] + b], "two")  # other record counts per file
    assert all1 == all2 == want["all"] and cut1 == cut2 == want["cut"] and t1 == t2
    res, _, _ = _check(ug, tmp_path, 31, [a + b], dict(want, records=[want["records"][0] + want["records"][1]]), tag="c")
    assert res["records"] == [sum(want["records"]), 0]


def _budget_for(ug, d, k, datas, parts, per_key, windows):
    """a budget (MiB) under which the count cuts the keys into exactly ``parts`` partitions (a bisection: the number the
    stage reports falls as the budget grows)"""
    lo, hi = 0.0, 1.2 * windows * per_key / (1 << 20) + 1
    for _ in range(40):
        mid = (lo + hi) / 2
        try:
            got = _stage(ug, d, k, datas, "b", budget_mb=mid)[0]["partitions"]
        except ug.UnitigError:  # not even the finest cut fits
            got = 1 << 30
        if got == parts:
            return mid
        if got > parts:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no budget gives %d partitions" % parts)


@pytest.mark.parametrize("k,per_key", [(21, 20), (50, 36)])
def test_partitions_do_not_change_the_result(ug, tmp_path, k, per_key):
    datas = ugcases.files("small")
    want = ugcases.expected("small", k)
    seen = []
    for parts in (1, 3, 8):
        mb = _budget_for(ug, tmp_path, k, datas, parts, per_key, want["windows"])
        res, tb, _ = _check(ug, tmp_path, k, datas, want, tag="p%d" % parts, budget_mb=mb)
        assert res["partitions"] == parts
        seen.append((tb["rounds"], tb["unitigs"]))
    assert seen[0] == seen[1] == seen[2]


def test_two_runs_give_the_same_bytes(ug, tmp_path):
    datas = ugcases.files("small")
    a = _stage(ug, tmp_path, 32, datas, "r1")
    b = _stage(ug, tmp_path, 32, datas, "r2")
    assert a[2] == b[2] and a[1] == b[1]
    assert a[2][0] == ugcases.expected("small", 32)["all"]


def test_the_kmer_filters_outputs_fed_straight_in(ug, tmp_path):
    from muchsalsa_amd import kmer_filter
    a, b = ugcases.files("small")
    p = [str(tmp_path / n) for n in ("1.fq", "2.fq", "report.txt", "o1.fq", "o2.fq", "all.fa", "cut.fa")]
    for path, data in zip(p, (a, b)):
        with open(path, "wb") as h:
            h.write(data)
    kf = kmer_filter.run(31, *p[:5], device=0)
    assert 0 < kf["pairs_out"] < kf["pairs_in"]
    o1, o2 = open(p[3], "rb").read(), open(p[4], "rb").read()
    want = ug_oracle.run(31, [o1, o2])
    tables = {}
    res = ug.run(31, p[3], p[4], p[5], p[6], device=0, tables=tables)
    assert open(p[5], "rb").read() == want["all"] and open(p[6], "rb").read() == want["cut"]
    assert tables["unitigs"] == want["unitigs"] and tables["rounds"] == want["rounds"]
    assert res["records"] == [kf["pairs_out"]] * 2 and res["solid"] == want["solid"] and len(want["unitigs"]) > 0


def test_clean_workload_doubling_depth(ug, tmp_path):
    want = ugcases.expected("clean", 31)
    assert ugcases.meets_conditions("clean", want) == []
    res, _, _ = _check(ug, tmp_path, 31, ugcases.files("clean"), want)
    assert res["longest"] >= 1 << 16 and res["unitigs"] == 1
    print("doubling rounds %d, longest chain %d" % (res["doubling_rounds"], res["longest"]))
    # a chain of n k-mers is resolved when 2^r >= n - 1; one more round sees that nothing is open
    assert res["doubling_rounds"] <= math.ceil(math.log2(res["longest"])) + 2


def _fq(seqs, mate=1, quals=None):
    return b"".join(b"@e%d/%d\n%s\n+\n%s\n" % (i, mate, s, (quals[i] if quals else b"I" * len(s)))
                    for i, s in enumerate(seqs))


_COMMON = [b"GATTACAGATTACAGATTACAGATTACA"] * 6
_RARE = [b"ACGGTCATGCCTAGGATCCGATAAGCTTGCATGCA", b"TTGACCGGTAACCGGTTAGCAGCATCGACGAGCTA", b"CCATGGCGCGCCTTAATTAAGGCCGGCCATATGCA",
         b"ACGGTCATGCCTAGGATCCGATA", b"TTGACCGGTAACCGGTTAGC", b"CCATGGCGCGCCTTAATT"]


def test_edge_inputs(ug, tmp_path):
    k = 5
    one = _COMMON + _RARE + [b"ACG", b"", b"NNNNNNNNNNNN", b"gattacagattaca", b"ACGTNACGTNACGTNACGT"]
    two = _RARE + _COMMON + [b"", b"AC", b"nnnnnn", b"ACGGTCATGCC", b"GATTANAGATT"]
    quals = [b"@" + b"I" * (len(s) - 1) if len(s) and i % 2 else b"I" * len(s) for i, s in enumerate(one)]
    a, b = _fq(one, 1, quals), _fq(two, 2)
    for n, (x, y) in enumerate(((a, b), (a[:-1], b), (a[:-1], b[:-1]))):  # with and without the final newline
        for mc in (1, 2):
            _check(ug, tmp_path, k, [x, y], tag="e%d%d" % (n, mc), min_count=mc, min_length=8)
    _check(ug, tmp_path, 5, [a], tag="one", min_length=8)  # no second file
    # no solid k-mer at all: every read shorter than k / no record / an empty second file
    for n, datas in enumerate(([_fq([b"ACGT"] * 12)], [b""], [b"", b""], [_fq(_COMMON), b""])):
        r, _, want = _check(ug, tmp_path, 20 if n == 0 else 5, datas, tag="z%d" % n, min_length=0)
        if n < 3:
            assert r["unitigs"] == 0 and want["all"] == want["cut"] == b"" and r["bytes_out"] == [0, 0]
    # homopolymers: self-loops are never joined
    r, tb, _ = _check(ug, tmp_path, 4, [_fq([b"A" * 30 + b"C" * 12 + b"G" * 9] * 2)], tag="h", min_length=0)
    assert r["unitigs"] >= 3


def test_errors(ug, tmp_path):
    from muchsalsa_amd import _lib
    good = _fq(_COMMON + _RARE)
    good2 = _fq(_RARE + _COMMON, 2)
    n = 4 * len(_COMMON + _RARE)

    def fails(k, a, b, code, file, line, tag, **kw):
        p = _paths(tmp_path, tag)
        for path, data in zip(p, (a, b)):
            with open(path, "wb") as h:
                h.write(data)
        with pytest.raises(ug.UnitigError) as e:
            ug.run(k, *p, device=0, **kw)
        assert (e.value.code, e.value.file, e.value.line) == (code, file, line), str(e.value)
        assert not any(os.path.exists(x) for x in p[2:])
        if code == _lib.E_FORMAT:
            with pytest.raises(kf_oracle.FastqError) as o:
                ug_oracle.parse_files([a, b])
            assert (o.value.file, o.value.line) == (file, line)

    # the k-mer filter's malformed inputs that still apply (record counts may differ here)
    lines = good.split(b"\n")
    no_at = b"\n".join(lines[:8] + [b"e2/1"] + lines[9:])
    fails(5, no_at, good2, _lib.E_FORMAT, 0, 9, "f1")
    no_plus = b"\n".join(lines[:6] + [b"-"] + lines[7:])
    fails(5, good, no_plus.replace(b"/1", b"/2"), _lib.E_FORMAT, 1, 7, "f2")
    unequal = b"\n".join(lines[:3] + [lines[3][:-1]] + lines[4:])
    fails(5, unequal, good2, _lib.E_FORMAT, 0, 4, "f3")
    fails(5, b"\n".join(lines[:n - 1]) + b"\n", good2, _lib.E_FORMAT, 0, n, "f4")  # a truncated record
    fails(5, good, b"\n".join(good2.split(b"\n")[:n - 2]), _lib.E_FORMAT, 1, n - 1, "f4b")
    fails(5, no_at, no_plus, _lib.E_FORMAT, 0, 9, "f6")  # file 0 is judged first
    fails(1, good, good2, _lib.E_ARG, 0, 0, "f7")
    fails(65, good, good2, _lib.E_ARG, 0, 0, "f8")
    fails(5, good, good2, _lib.E_ARG, 0, 0, "f9", min_count=0)
    fails(5, good, good2, _lib.E_ARG, 0, 0, "f10", trim=-2)
    p = _paths(tmp_path, "f12")
    with pytest.raises(ug.UnitigError) as e:
        ug.run(5, p[0] + ".missing", None, p[2], p[3], device=0)
    assert e.value.code == _lib.E_IO
    # unequal record counts are no error here
    _check(ug, tmp_path, 5, [good, good2 + _fq([b"ACGTACGT"], 2)], tag="f5", min_length=8)


def test_context_serves_a_good_run_after_an_error(ug, tmp_path):
    import ctypes as C
    from muchsalsa_amd import _lib
    L = _lib.lib()
    p = _paths(tmp_path)
    good, good2 = _fq(_COMMON + _RARE), _fq(_RARE + _COMMON, 2)
    bad = good.replace(b"+\n", b"\n", 1)
    for path, data in ((p[0], good), (p[1], good2), (p[2], bad)):
        with open(path, "wb") as h:
            h.write(data)
    ctx, res = C.c_void_p(), C.c_void_p()
    prm = _lib.UgParams(5, 2, -1, 8)
    assert L.msgpu_ug_create(0, C.byref(ctx)) == _lib.OK
    try:
        assert L.msgpu_ug_run(ctx, C.byref(prm), os.fsencode(p[2]), os.fsencode(p[1]), 0, 0, C.byref(res)) == _lib.E_FORMAT
        assert (L.msgpu_ug_error_file(ctx), L.msgpu_ug_error_line(ctx)) == (0, 3) and not res.value
        assert b"line 3" in L.msgpu_ug_last_error(ctx)
        assert L.msgpu_ug_run(ctx, C.byref(prm), os.fsencode(p[0]), os.fsencode(p[1]), 1, 0, C.byref(res)) == _lib.E_ARG  # flags
        assert L.msgpu_ug_run(ctx, C.byref(prm), os.fsencode(p[0]), os.fsencode(p[1]), 0, 0, C.byref(res)) == _lib.OK
        assert L.msgpu_ug_error_line(ctx) == 0 and L.msgpu_ug_last_error(ctx) == b""
        want = ug_oracle.run(5, [good, good2], min_length=8)
        st = _lib.UgStats()
        L.msgpu_ug_result_stats(res, C.byref(st))
        assert (st.n_windows, st.n_solid, st.n_unitigs, st.trim) == (want["windows"], want["solid"], len(want["unitigs"]), 5)
        n = C.c_uint64()
        assert C.string_at(L.msgpu_ug_result_text(res, _lib.UG_TEXT_ALL, C.byref(n)), n.value) == want["all"]
        assert C.string_at(L.msgpu_ug_result_text(res, _lib.UG_TEXT_CUT, C.byref(n)), n.value) == want["cut"]
        L.msgpu_ug_result_free(res)
    finally:
        L.msgpu_ug_destroy(ctx)


def test_command_line(ug, tmp_path):
    want = ugcases.expected("small", 21, min_count=3, trim=10, min_length=300)
    p = _paths(tmp_path)
    for path, data in zip(p, ugcases.files("small")):
        with open(path, "wb") as h:
            h.write(data)
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.unitigs", "21"] + p + ["--min-count", "3", "--trim", "10",
                                                                                       "--min-length", "300"],
                         cwd=ROOT, env=env, capture_output=True, timeout=LIMIT)
    assert out.returncode == 0, out.stderr.decode()
    js = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert (js["windows"], js["distinct"], js["solid"], js["solid_after"], js["unitigs"], js["kept"]) == (
        want["windows"], want["distinct"], want["solid"], want["solid_after"], len(want["unitigs"]), want["kept"])
    assert [tuple(r) for r in js["rounds"]] == want["rounds"] and js["seconds"]["total"] > 0
    assert open(p[2], "rb").read() == want["all"] and open(p[3], "rb").read() == want["cut"]
