"""Unitig coverage filter on the GPU: out.fa and the report byte for byte against the hand-derived fixtures and against
the per-base numpy restatement (tests/uf_oracle.py), every width class of pass 1 at its bounds, and the command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

import uf_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "unitig_filter")
PRIOR = "earlier step\nkept as it is\n"


@pytest.fixture(scope="module")
def uf():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitig_filter
    return unitig_filter


def _stage(uf, d, paf, fasta, packed=False, tag="x"):
    p, f = os.path.join(d, tag + ".paf"), os.path.join(d, tag + ".fa")
    rep, out = os.path.join(d, tag + ".report.txt"), os.path.join(d, tag + ".out.fa")
    with open(p, "wb") as h:
        h.write(paf)
    with open(f, "wb") as h:
        h.write(fasta)
    with open(rep, "w") as h:
        h.write(PRIOR)
    res = uf.run(p, f, rep, out, device=0, packed=packed)
    with open(out, "rb") as h:
        got = h.read()
    with open(rep) as h:
        report = h.read()
    assert report.startswith(PRIOR)
    return got, report[len(PRIOR):], res


def _check(uf, tmp_path, paf, fasta, packed=False, tag="x"):
    want, wrep = uf_oracle.run(paf, fasta)
    got, report, res = _stage(uf, str(tmp_path), paf, fasta, packed, tag)
    assert report == uf_oracle.report_lines(wrep)
    assert len(got) == len(want)
    assert got == want
    return res, wrep


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("fx", ["a", "b"])
def test_fixture_byte_identical(uf, tmp_path, fx, packed):
    with open(os.path.join(GOLD, fx + ".paf"), "rb") as h:
        paf = h.read()
    with open(os.path.join(GOLD, fx + ".fa"), "rb") as h:
        fasta = h.read()
    got, report, res = _stage(uf, str(tmp_path), paf, fasta, packed)
    with open(os.path.join(GOLD, fx + ".out.fa"), "rb") as h:
        assert got == h.read()
    with open(os.path.join(GOLD, fx + ".report.txt")) as h:
        assert report == h.read()
    assert res["outliers"] == 1 and res["rescued"] == 1


def _bases(n, seed):
    rng = np.random.default_rng(seed)
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes()


def _line(u, qlen, s, e, r):
    return b"%s\t%d\t%d\t%d\t+\t%s\t5000\t0\t%d\t%d\t%d\t60\n" % (u, qlen, s, e, r, max(e - s, 0), max(e - s, 0),
                                                                 max(e - s, 0))


def _block(name, n, qlen, seed, windows=None):
    """n lines on a unitig of qlen positions; reads drawn from a pool of ~n/3 names (repeats within the block), some
    empty intervals; windows: (period, width) -- the lines pile up in windows, the gaps become fragments"""
    rng = np.random.default_rng(seed)
    if windows:
        period, width = windows
        s = rng.integers(0, qlen // period, n) * period + rng.integers(0, width, n)
    else:
        s = rng.integers(0, qlen, n)
    e = np.minimum(qlen, s + rng.integers(1, 900, n))
    e[::29] = s[::29]  # empty intervals
    r = rng.integers(0, max(2, n // 3), n)
    return b"".join(_line(name, qlen, int(a), int(b), b"q%d" % c) for a, b, c in zip(s, e, r))


def _fillers(k, seed):
    """k small ids of value 1..2"""
    paf, fa = b"", b""
    for i in range(k):
        name = b"f%d" % i
        paf += _line(name, 300, 0, 100, b"a") + (_line(name, 300, 50, 150, b"b") if i % 2 else b"")
        fa += b">%s filler\n%s\n" % (name, _bases(300, seed + i))
    return paf, fa


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 20000])
def test_width_class_bounds(uf, tmp_path, n):
    qlen = 3000 + 2 * n
    blk = _block(b"T", n, qlen, n)
    seq = b">T test block\n" + _bases(qlen - 100, n) + b"\n"
    # two ids: the report's Q3 = v_T - (v_T - 1) / 4 shows the block's pass-1 value
    fpaf, ffa = _fillers(1, 11)
    res, wrep = _check(uf, tmp_path, fpaf + blk, ffa + seq, tag="two")
    want_class = "wave_blocks" if n <= 64 else "group_blocks" if n <= 1024 else "giant_blocks"
    assert res[want_class] >= 1
    # nine ids: the block is an outlier and its pass 2 runs too
    fpaf, ffa = _fillers(8, 12)
    res, wrep = _check(uf, tmp_path, fpaf + blk, ffa + seq, tag="nine")
    if n >= 63:
        assert wrep["outliers"] >= 1


def test_long_unitig_many_fragments(uf, tmp_path):
    qlen = 150000
    blk = _block(b"L", 20000, qlen, 3, windows=(10000, 3000))
    fpaf, ffa = _fillers(8, 13)
    res, wrep = _check(uf, tmp_path, fpaf + blk, ffa + b">L long\n" + _bases(qlen, 3) + b"\n", tag="long")
    assert res["giant_blocks"] == 1 and wrep["outliers"] == 1 and res["fragments"] >= 10


@pytest.mark.parametrize("packed", [False, True])
def test_workload_config1(uf, tmp_path, packed):
    from muchsalsa_amd import synth
    paf, fasta = synth.unitig_filter_workload(10000, 5000, 50000, 1)
    res, wrep = _check(uf, tmp_path, paf, fasta, packed)
    assert wrep["outliers"] > 0 and res["giant_blocks"] > 0 and res["fragments"] > 0


def test_workload_config2(uf, tmp_path):
    from muchsalsa_amd import synth
    paf, fasta = synth.unitig_filter_workload(100000, 10000, 500000, 2, n_repeats=40, n_long=4, n_dup=20000,
                                              n_again=3000)
    res, wrep = _check(uf, tmp_path, paf, fasta, packed=True)
    assert wrep["outliers"] > 0 and res["giant_blocks"] > 0


def test_command_line_matches_run(uf, tmp_path):
    from muchsalsa_amd import synth
    paf, fasta = synth.unitig_filter_workload(2000, 5000, 8000, 4, n_repeats=4, n_long=1, long_len=100000,
                                              long_hits=10000)
    got, report, _ = _stage(uf, str(tmp_path), paf, fasta, tag="api")
    p, f = str(tmp_path / "api.paf"), str(tmp_path / "api.fa")
    rep, out = str(tmp_path / "cli.report.txt"), str(tmp_path / "cli.out.fa")
    with open(rep, "w") as h:
        h.write(PRIOR)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "muchsalsa_amd.unitig_filter", p, f, rep, out],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import json
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["blocks"] > 0 and "seconds" in line
    with open(out, "rb") as h:
        assert h.read() == got
    with open(rep) as h:
        assert h.read() == PRIOR + report


def test_missing_unitig_writes_nothing(uf, tmp_path):
    p, f = tmp_path / "m.paf", tmp_path / "m.fa"
    p.write_bytes(_line(b"u1", 100, 0, 50, b"r") + _line(b"u2", 100, 0, 50, b"r"))
    f.write_bytes(b">u1\n" + _bases(100, 1) + b"\n")
    out, rep = tmp_path / "m.out.fa", tmp_path / "m.report.txt"
    with pytest.raises(uf.UnitigFilterError) as ei:
        uf.run(str(p), str(f), str(rep), str(out))
    assert ei.value.line == 2
    assert not out.exists() and not rep.exists()
