"""K-mer abundance filter on the GPU: every test runs the stage on files and compares, without any tolerance (integers and
bytes), with the plain-Python restatement (tests/kf_oracle.py): histogram rows, q1 / q3 / upper, the abundant set with its
counts, the verdict of every pair, both output files and the report.  Malformed inputs are rejected by the stage's check
kernel with an error code; no test provokes a device fault.  Every test runs under its own time limit: a watchdog ends the
process when a stage call does not come back."""
import faulthandler
import json
import os
import subprocess
import sys

import pytest

import kf_oracle
import kfcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kmer_filter")
LIMIT = 600  # seconds per test
OUTPUTS = ("report.txt", "o1.fq", "o2.fq")


@pytest.fixture(scope="module")
def kf():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import kmer_filter
    return kmer_filter


@pytest.fixture(autouse=True)
def time_limit(kf):  # (after kf: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def _paths(d, tag="x"):
    return [os.path.join(str(d), tag + "." + n) for n in ("1.fq", "2.fq") + OUTPUTS]


def _stage(kf, d, k, a, b, tag="x", **kw):
    p = _paths(d, tag)
    for path, data in zip(p, (a, b)):
        with open(path, "wb") as h:
            h.write(data)
    tables = {}
    res = kf.run(k, *p, device=0, tables=tables, **kw)
    texts = []
    for path in p[2:]:
        with open(path, "rb") as h:
            texts.append(h.read())
    return res, tables, texts


def _check(kf, d, k, a, b, want=None, tag="x", **kw):
    """the stage against the restatement: every table, every file"""
    want = kf_oracle.run(k, a, b) if want is None else want
    res, tb, (report, o1, o2) = _stage(kf, d, k, a, b, tag, **kw)
    assert tb["histogram"] == want["histogram"]
    assert (res["q1"], res["q3"], res["upper"]) == (want["q1"], want["q3"], want["upper"])
    got = [((int(h) << 64) | int(l), int(c)) for h, l, c in zip(tb["key_hi"].tolist(), tb["key_lo"].tolist(),
                                                                tb["count"].tolist())]
    assert len(got) == len(want["abundant"]) == res["abundant"]
    assert got == want["abundant"]
    assert tb["verdict"].tolist() == want["verdict"]
    assert (res["pairs_in"], res["pairs_out"], res["windows"], res["distinct"]) == (
        want["pairs"], want["pairs"] - sum(want["verdict"]), want["windows"], want["distinct"])
    assert len(o1) == len(want["out1"]) and len(o2) == len(want["out2"])
    assert o1 == want["out1"] and o2 == want["out2"]
    assert report == want["report"]
    return res, tb, want


@pytest.mark.parametrize("k", (1,) + kfcases.KS_SMALL)
def test_small_workload(kf, tmp_path, k):
    name = "tiny" if k == 1 else "small"
    a, b = kfcases.workload(name)
    res, _, want = _check(kf, tmp_path, k, a, b, kfcases.expected(name, k))
    assert res["k"] == k and res["partitions"] == 1
    if k > 1:
        assert 0 < res["pairs_out"] < res["pairs_in"] and res["abundant"] > 0


@pytest.mark.parametrize("k", kfcases.KS_BIG)
def test_one_megabase_shape(kf, tmp_path, k):
    a, b = kfcases.workload("big")
    want = kfcases.expected("big", k)
    assert kfcases.meets_conditions(want) == []
    res, _, _ = _check(kf, tmp_path, k, a, b, want)
    assert res["windows"] > 20_000_000 and res["abundant"] > 1000


def test_row_10001(kf, tmp_path):
    a, b = kfcases.workload("poly_a")
    _, tb, want = _check(kf, tmp_path, 31, a, b, kfcases.expected("poly_a", 31))
    assert tb["histogram"][-1] == (10001, 1) and int(tb["count"][0]) == 14000


def _budget_for(kf, d, k, a, b, parts, per_key):
    """a budget (MiB) under which the stage cuts the keys into exactly ``parts`` partitions: the stage reports the number
    it chose, which falls as the budget grows, so the search is a bisection on the budget"""
    windows = kf_oracle.run(k, a, b)["windows"]
    lo, hi = 0.0, 1.2 * windows * per_key / (1 << 20) + 1  # hi: everything in one partition
    for _ in range(40):
        mid = (lo + hi) / 2
        try:
            got = _stage(kf, d, k, a, b, "b", budget_mb=mid)[0]["partitions"]
        except kf.KmerFilterError:  # not even the finest cut fits
            got = 1 << 30
        if got == parts:
            return mid
        if got > parts:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no budget gives %d partitions" % parts)


@pytest.mark.parametrize("k,per_key", [(21, 20), (50, 36)])
def test_partitions_do_not_change_the_result(kf, tmp_path, k, per_key):
    a, b = kfcases.workload("small")
    want = kfcases.expected("small", k)
    seen = []
    for parts in (1, 3, 8):
        mb = _budget_for(kf, tmp_path, k, a, b, parts, per_key)
        res, tb, _ = _check(kf, tmp_path, k, a, b, want, tag="p%d" % parts, budget_mb=mb)
        assert res["partitions"] == parts
        seen.append((tb["histogram"], tb["key_hi"].tobytes(), tb["key_lo"].tobytes(), tb["count"].tobytes(),
                     tb["verdict"].tobytes()))
    assert seen[0] == seen[1] == seen[2]


def _fq(seqs, mate=1, quals=None):
    return b"".join(b"@e%d/%d\n%s\n+\n%s\n" % (i, mate, s, (quals[i] if quals else b"I" * len(s)))
                    for i, s in enumerate(seqs))


# a block that makes GATTACAGATTACA's k-mers abundant at k = 5 next to a spread of rarer ones
_COMMON = [b"GATTACAGATTACAGATTACAGATTACA"] * 6
_RARE = [b"ACGGTCATGCCTAGGATCCGATAAGCTTGCATGCA", b"TTGACCGGTAACCGGTTAGCAGCATCGACGAGCTA", b"CCATGGCGCGCCTTAATTAAGGCCGGCCATATGCA",
         b"ACGGTCATGCCTAGGATCCGATA", b"TTGACCGGTAACCGGTTAGC", b"CCATGGCGCGCCTTAATT"]


def test_edge_inputs(kf, tmp_path):
    k = 5
    one = _COMMON + _RARE + [b"ACG", b"", b"NNNNNNNNNNNN", b"gattacagattaca", b"ACGTNACGTNACGTNACGT"]
    two = _RARE + _COMMON + [b"", b"AC", b"nnnnnn", b"ACGGTCATGCC", b"GATTANAGATT"]
    quals = [b"@" + b"I" * (len(s) - 1) if len(s) and i % 2 else b"I" * len(s) for i, s in enumerate(one)]
    a, b = _fq(one, 1, quals), _fq(two, 2)
    res, tb, want = _check(kf, tmp_path, k, a, b, tag="e1")
    assert 0 < res["pairs_out"] < res["pairs_in"] and tb["verdict"][len(_COMMON) + len(_RARE) + 3] == 1  # lower case folds
    _check(kf, tmp_path, k, a[:-1], b, tag="e2")  # no final newline, one file / both
    r2, _, _ = _check(kf, tmp_path, k, a[:-1], b[:-1], tag="e3")
    assert r2["pairs_out"] == res["pairs_out"]
    # every read of one file is shorter than k; nothing is abundant, no pair dropped
    r, _, _ = _check(kf, tmp_path, 20, _fq(_COMMON + _RARE), _fq([b"ACGT"] * 12, 2), tag="e4")
    assert r["pairs_out"] == r["pairs_in"] == 12 and r["abundant"] == 0
    # every pair dropped / no pair dropped
    r, _, _ = _check(kf, tmp_path, k, _fq(_COMMON + _RARE + _COMMON), _fq(_COMMON + _COMMON + _COMMON, 2), tag="e5")
    assert r["pairs_out"] == 0 and r["bytes_out"] == [0, 0]
    r, _, _ = _check(kf, tmp_path, 1, _fq([b"AAAAAAA", b"C"]), _fq([b"ACCN", b""], 2), tag="e6")
    assert r["pairs_out"] == r["pairs_in"] == 2 and r["abundant"] == 0
    # one pair only
    seq = b"A" * 30 + b"C" * 12 + b"G" * 9
    r, _, _ = _check(kf, tmp_path, 4, _fq([seq]), _fq([seq[::-1]], 2), tag="e7")
    assert r["pairs_in"] == 1


@pytest.mark.parametrize("fx", ["a", "b"])
def test_tiny_golden_pairs(kf, tmp_path, fx):
    with open(os.path.join(GOLD, "tiny_%s.json" % fx)) as f:
        meta = json.load(f)
    data = [open(os.path.join(GOLD, "tiny_%s.%d.fq" % (fx, m)), "rb").read() for m in (1, 2)]
    res, tb, _ = _check(kf, tmp_path, meta["k"], data[0], data[1])
    assert [list(x) for x in tb["histogram"]] == meta["histogram"] and res["upper"] == meta["upper"]
    assert tb["verdict"].tolist() == meta["verdict"]


def test_errors(kf, tmp_path):
    from muchsalsa_amd import _lib
    good = _fq(_COMMON + _RARE)
    good2 = _fq(_RARE + _COMMON, 2)
    n = 4 * len(_COMMON + _RARE)

    def fails(k, a, b, code, file, line, tag):
        p = _paths(tmp_path, tag)
        for path, data in zip(p, (a, b)):
            with open(path, "wb") as h:
                h.write(data)
        with pytest.raises(kf.KmerFilterError) as e:
            kf.run(k, *p, device=0)
        assert (e.value.code, e.value.file, e.value.line) == (code, file, line), str(e.value)
        assert not any(os.path.exists(x) for x in p[2:])
        if code == _lib.E_FORMAT:
            with pytest.raises(kf_oracle.FastqError) as o:
                kf_oracle.parse_pair(a, b)
            assert (o.value.file, o.value.line) == (file, line)

    lines = good.split(b"\n")
    no_at = b"\n".join(lines[:8] + [b"e2/1"] + lines[9:])
    fails(5, no_at, good2, _lib.E_FORMAT, 0, 9, "f1")
    no_plus = b"\n".join(lines[:6] + [b"-"] + lines[7:])
    fails(5, good, no_plus.replace(b"/1", b"/2"), _lib.E_FORMAT, 1, 7, "f2")
    unequal = b"\n".join(lines[:3] + [lines[3][:-1]] + lines[4:])
    fails(5, unequal, good2, _lib.E_FORMAT, 0, 4, "f3")
    fails(5, b"\n".join(lines[:n - 1]) + b"\n", good2, _lib.E_FORMAT, 0, n, "f4")  # a truncated record
    fails(5, good, b"\n".join(good2.split(b"\n")[:n - 2]), _lib.E_FORMAT, 1, n - 1, "f4b")
    fails(5, good, good2 + _fq([b"ACGT"], 2), _lib.E_FORMAT, 0, n + 1, "f5")  # unequal record counts
    fails(5, good + _fq([b"ACGT"]), good2, _lib.E_FORMAT, 1, n + 1, "f5b")
    fails(5, no_at, no_plus, _lib.E_FORMAT, 0, 9, "f6")  # file 0 is judged first
    fails(0, good, good2, _lib.E_ARG, 0, 0, "f7")
    fails(65, good, good2, _lib.E_ARG, 0, 0, "f8")
    fails(5, _fq([b"ACGTACGTAC"]), _fq([b"TTTTT"], 2), _lib.E_LAYOUT, 0, 0, "f9")  # one row besides a = 1: q3 is never set
    with pytest.raises(kf_oracle.DegenerateHistogram):
        kf_oracle.run(5, _fq([b"ACGTACGTAC"]), _fq([b"TTTTT"], 2))
    fails(5, b"", b"", _lib.E_LAYOUT, 0, 0, "f10")  # no record at all
    a, b = kfcases.workload("small")
    fails(1, a, b, _lib.E_LAYOUT, 0, 0, "f11")  # both k-mers in row 10001: q3 is never set
    p = _paths(tmp_path, "f12")
    with pytest.raises(kf.KmerFilterError) as e:
        kf.run(5, p[0] + ".missing", p[1], *p[2:], device=0)
    assert e.value.code == _lib.E_IO


def test_context_serves_a_good_run_after_an_error(kf, tmp_path):
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
    assert L.msgpu_kf_create(0, C.byref(ctx)) == _lib.OK
    try:
        assert L.msgpu_kf_run(ctx, 5, os.fsencode(p[2]), os.fsencode(p[1]), 0, 0, C.byref(res)) == _lib.E_FORMAT
        assert (L.msgpu_kf_error_file(ctx), L.msgpu_kf_error_line(ctx)) == (0, 3) and not res.value
        assert b"line 3" in L.msgpu_kf_last_error(ctx)
        assert L.msgpu_kf_run(ctx, 5, os.fsencode(p[0]), os.fsencode(p[1]), 1, 0, C.byref(res)) == _lib.E_ARG  # flags
        assert L.msgpu_kf_run(ctx, 5, os.fsencode(p[0]), os.fsencode(p[1]), 0, 0, C.byref(res)) == _lib.OK
        assert L.msgpu_kf_error_line(ctx) == 0 and L.msgpu_kf_last_error(ctx) == b""
        st = _lib.KfStats()
        L.msgpu_kf_result_stats(res, C.byref(st))
        want = kf_oracle.run(5, good, good2)
        assert (st.n_pairs, st.n_windows, st.upper, st.n_abundant) == (want["pairs"], want["windows"], want["upper"],
                                                                        len(want["abundant"]))
        n = C.c_uint64()
        text = C.string_at(L.msgpu_kf_result_text(res, _lib.KF_TEXT_KMERS, C.byref(n)), n.value)
        assert text == kf_oracle.dump_text(want["abundant"], 5)
        text = C.string_at(L.msgpu_kf_result_text(res, _lib.KF_TEXT_HISTO, C.byref(n)), n.value)
        assert text == kf_oracle.histogram_text(want["histogram"])
        L.msgpu_kf_result_free(res)
    finally:
        L.msgpu_kf_destroy(ctx)


@pytest.mark.parametrize("k", [21, 40])
def test_command_line(kf, tmp_path, k):
    a, b = kfcases.workload("small")
    want = kfcases.expected("small", k)
    p = _paths(tmp_path)
    for path, data in zip(p, (a, b)):
        with open(path, "wb") as h:
            h.write(data)
    histo, kmers = str(tmp_path / "k.histo"), str(tmp_path / "k.fa")
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.kmer_filter", str(k)] + p + ["--histo", histo, "--kmers", kmers],
                         cwd=ROOT, env=env, capture_output=True, timeout=LIMIT)
    assert out.returncode == 0, out.stderr.decode()
    js = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert (js["pairs_in"], js["pairs_out"], js["windows"], js["distinct"], js["q1"], js["q3"], js["upper"],
            js["abundant"]) == (want["pairs"], want["pairs"] - sum(want["verdict"]), want["windows"], want["distinct"],
                                want["q1"], want["q3"], want["upper"], len(want["abundant"]))
    assert js["partitions"] == 1 and js["seconds"]["total"] > 0
    for path, text in zip(p[2:] + [histo, kmers], (want["report"], want["out1"], want["out2"],
                                                   kf_oracle.histogram_text(want["histogram"]),
                                                   kf_oracle.dump_text(want["abundant"], k))):
        with open(path, "rb") as h:
            assert h.read() == text, path
    bad = subprocess.run([sys.executable, "-m", "muchsalsa_amd.kmer_filter", str(k)] + p[:3], cwd=ROOT, env=env,
                         capture_output=True, timeout=LIMIT)
    assert bad.returncode == 2
