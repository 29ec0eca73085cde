"""Unitig assembly above k = 64, host side (no GPU): the restatement at any k (tests/ug_wide_oracle.py) against the 128-bit one
where both apply and against its own recorded results for the hand-made cases (tests/golden/unitigs_wide, made by
tools/make_unitig_wide_fixtures.py); the conditions the GPU tests rely on, checked on the restatement alone; the multi-word key
(csrc/msgpu_kmer_wide.h) in a stand-alone host program built with the undefined-behaviour sanitizer (tests/cpp/test_kmer_wide.cpp)
against vectors worked out on Python integers; the C-ABI's two new symbols and the command line's ``--wide``."""
import json
import os
import random
import subprocess
import sys

import pytest

import kf_oracle
import kmeredgecases as E
import ug_bubble_oracle
import ug_oracle
import ug_wide_oracle
import ugwidecases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "unitigs_wide")
CSRC = os.path.join(ROOT, "muchsalsa_amd", "csrc")


def test_the_wide_rc_is_the_narrow_one_and_an_involution():
    rnd = random.Random(7)
    for k in (31, 32, 33, 63, 64):
        for x in [0, (1 << (2 * k)) - 1] + [rnd.getrandbits(2 * k) for _ in range(300)]:
            assert ug_wide_oracle.rc(x, k) == ug_oracle.rc(x, k) == ug_wide_oracle.rc_by_rule(x, k)
    for k in (65, 96, 97, 127, 128):
        for x in [0, (1 << (2 * k)) - 1] + [rnd.getrandbits(2 * k) for _ in range(300)]:
            y = ug_wide_oracle.rc(x, k)
            assert y == ug_wide_oracle.rc_by_rule(x, k) and ug_wide_oracle.rc(y, k) == x and y < (1 << (2 * k))


def test_the_binding_is_put_back_and_the_wide_run_is_the_narrow_one_below_65():
    before = (ug_oracle.rc, ug_oracle.count_files, ug_bubble_oracle.rc)
    for name in ("ladder-33-33", "ladder-64-64", "selfcomp-64", "hairpin-63"):
        _, k, files, params = E.cases()[name]
        a, b = E.expected(name), ug_wide_oracle.run(k, files, **params)
        for key in ("records", "windows", "distinct", "solid", "solid_after", "rounds", "unitigs", "all", "cut", "chains", "blocked"):
            assert a[key] == b[key], (name, key)
    assert (ug_oracle.rc, ug_oracle.count_files, ug_bubble_oracle.rc) == before
    with pytest.raises(ValueError):
        ug_wide_oracle.run(129, [b""])
    reads = [r for f in cases.cases()["ladder-65-65"][1] for r in kf_oracle.parse_fastq(f)]  # the count assumes 128 bits: not used
    assert ug_wide_oracle.count_files([reads], 65)[1] == sum(max(len(r[1]) - 64, 0) for r in reads)


@pytest.mark.parametrize("name", cases.names(cases.HAND))
def test_restatement_against_its_recorded_results(name):
    with open(os.path.join(GOLD, name.replace("-", "_k") + ".json")) as f:
        want = json.load(f)
    k = want["k"]
    r = cases.expected(name)
    assert cases.cases()[name][2]["min_length"] == want["min_length"] and cases.cases()[name][0] == k
    assert [list(x) for x in r["rounds"]] == want["rounds"]
    assert [[t[0], t[1], kf_oracle.kmer_text(t[2], k), t[3], t[4]] for t in r["unitigs"]] == want["unitigs"]
    assert r["all"].decode() == want["all"] and r["cut"].decode() == want["cut"]
    for key in ("records", "windows", "distinct", "solid", "solid_after", "cycles", "alone", "blocked"):
        assert r[key] == want[key], key


def test_cases_are_what_they_are_made_for():
    for k in cases.KS:
        assert cases.expected("rings-%d" % k)["cycles"] == 2 and cases.expected("hairpin-%d" % k)["blocked"] >= 1
        assert cases.expected("ladder-%d-%d" % (k, k))["rounds"] == E.ladder_plan(k)
        if k % 2 == 0:
            r = cases.expected("selfcomp-%d" % k)
            assert r["alone"] >= 1 and len(r["unitigs"]) >= 3
    for k in cases.KS_EDGE:
        firsts = [t[2] for t in cases.expected("words-%d" % k)["unitigs"]]
        assert all(cases.kmer_of(t) in firsts for t in cases.words_reads(k)[1])
        for name in cases.BUBBLES:
            for flip in ("", "-flip"):
                assert cases.bubble_conditions("%s-%d%s" % (name, k, flip))[1] == []
        g = cases.expected("three_in-%d" % k)["graph"]
        assert g["adjacencies"] == 2 * len(g["links"]) - g["self_mirror"] >= 8
        assert cases.expected("hairpin_gfa-%d" % k)["graph"]["self_mirror"] >= 1
    for k in cases.KS_SMALL:
        r = cases.expected("small-%d" % k)
        assert any(removed for _, removed in r["rounds"]) and r["kept"] >= 2 and r["solid_after"] < r["solid"] < r["distinct"]


@pytest.fixture(scope="module")
def key_program(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("cpp") / "test_kmer_wide")
    # a host-only build: the header alone, no device code, nothing of the library
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Xarch_host", "-fsanitize=undefined", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "test_kmer_wide.cpp"), "-o", out], check=True, timeout=600)
    return out


def test_the_key_type_under_the_undefined_behaviour_sanitizer(key_program):
    r = subprocess.run([key_program, os.path.join(GOLD, "key_vectors.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ") and int(r.stdout.split()[1]) > 1500
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    with open(os.path.join(GOLD, "key_vectors.txt")) as f:
        assert [int(line.split()[1]) for line in f if line.startswith("k ")] == [65, 66, 95, 96, 97, 127, 128]


@pytest.fixture(scope="module")
def ug():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitigs
    return unitigs


def test_symbols_documents_and_the_command_line(ug):
    from muchsalsa_amd import _lib, hybrid
    L = _lib.lib()
    assert L.msgpu_ug_set_wide(None, 1) == _lib.E_ARG and L.msgpu_ug_result_first_kmers(None, None, None, None) == _lib.E_ARG
    assert L.msgpu_ug_result_peak_bytes(None) == 0
    words = "k (2..64, or 2..128 after msgpu_ug_set_wide)"
    with open(os.path.join(ROOT, "include", "msgpu.h")) as f:
        assert words in " ".join(f.read().replace(" * ", " ").split())
    assert words in " ".join(ug.__doc__.split()) and "--wide" in ug.__doc__ and "wide" in hybrid.run.__doc__
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.unitigs", "65", "a", "b", "c", "d", "--wide", "--bogus"], cwd=ROOT, env=env,
                         capture_output=True, timeout=120)
    assert out.returncode == 2 and b"--wide" in out.stderr
