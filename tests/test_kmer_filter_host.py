"""K-mer abundance filter, host side (no GPU): msgpu_kf_threshold and the restatement's threshold against the recorded
outputs of the reference pipeline's own script (tests/golden/kmer_filter/threshold.json, made by
tools/make_kmer_filter_fixtures.py), the restatement against hand cases and the tiny golden pairs, and the conditions the GPU
tests rely on, checked on the restatement alone.

Hand cases (k = 3 unless said): ``ACGTN``: windows ACG and CGT are one canonical k-mer (CGT's reverse complement is ACG), GTN
is none -> ACG: 2.  ``ACGT`` at k = 4 is its own reverse complement: it counts once per window.  tiny_a: AAA = 10 windows
of the twelve A, 8 of the ten T (TTT's reverse complement), 1 in ``ggatAAAc`` = 19; upper = 15, so AAA alone is abundant:
pair 0 falls by both mates, pair 2 by its second mate alone."""
import json
import os

import numpy as np
import pytest

import kf_oracle
import kfcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kmer_filter")


@pytest.fixture(scope="module")
def kf():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import kmer_filter
    return kmer_filter


def _cases():
    with open(os.path.join(GOLD, "threshold.json")) as f:
        return json.load(f)["cases"]


def _fq(seqs, mate=1):
    return b"".join(b"@r%d/%d\n%s\n+\n%s\n" % (i, mate, s, b"I" * len(s)) for i, s in enumerate(seqs))


def test_fixture_covers_what_it_should():
    cases = _cases()
    assert len(cases) >= 60
    names = {c["name"] for c in cases}
    assert {"issue_1", "issue_2_elif", "issue_3", "issue_4_q3_never", "issue_5_only_row_1", "round_ties"} <= names
    assert any(c["failed"] for c in cases) and any(c["printed"] is not None and c["printed"] <= 0 for c in cases)
    assert any(r[0] == 10001 for c in cases for r in c["rows"]) and any(all(r[0] != 1 for r in c["rows"]) for c in cases)
    by = {c["name"]: c["printed"] for c in cases}
    assert (by["issue_1"], by["issue_2_elif"], by["issue_3"], by["issue_4_q3_never"], by["issue_5_only_row_1"]) == (
        5, 5, 5, -14, None)
    # the pipeline's awk line sums every row but a = 1
    for c in cases:
        rest = [f for a, f in c["rows"] if a != 1]
        assert c["total"] == (str(sum(rest)) if rest else "")


@pytest.mark.parametrize("case", _cases(), ids=lambda c: c["name"])
def test_threshold_is_the_scripts(kf, case):
    rows = [tuple(r) for r in case["rows"]]
    good = (not case["failed"]) and case["printed"] > 0
    if good:
        assert kf.threshold(rows)[2] == case["printed"]
        assert kf_oracle.threshold(rows)[2] == case["printed"]
        assert kf.threshold(rows) == kf_oracle.threshold(rows)
    else:
        from muchsalsa_amd import _lib
        with pytest.raises(kf.KmerFilterError) as e:
            kf.threshold(rows)
        assert e.value.code == _lib.E_LAYOUT
        with pytest.raises(kf_oracle.DegenerateHistogram):
            kf_oracle.threshold(rows)


def test_threshold_of_no_rows_is_degenerate(kf):
    with pytest.raises(kf.KmerFilterError):
        kf.threshold([])
    with pytest.raises(kf_oracle.DegenerateHistogram):
        kf_oracle.threshold([])


def test_hand_cases():
    acg = 0b000110  # A C G
    r1, r2 = kf_oracle.parse_pair(_fq([b"ACGTN"]), _fq([b""], 2))
    assert kf_oracle.count(r1, r2, 3) == ({acg: 2}, 2)
    assert kf_oracle.canonical_kmers(b"GTN", 3) == []
    acgt = 0b00011011
    assert kf_oracle.canonical_kmers(b"ACGTACGT", 4)[0::4] == [acgt, acgt]  # a palindrome: once per window
    r1, r2 = kf_oracle.parse_pair(_fq([b"ACGT"]), _fq([b"ACGT"], 2))
    assert kf_oracle.count(r1, r2, 4) == ({acgt: 2}, 2)
    assert kf_oracle.canonical_kmers(b"acgTn", 3) == [acg, acg]  # lower case folds
    assert kf_oracle.canonical_kmers(b"ACGTACG", 8) == []  # shorter than k
    assert kf_oracle.canonical_kmers(b"AAAA", 1) == [0, 0, 0, 0] and kf_oracle.canonical_kmers(b"TG", 1) == [0, 1]
    assert kf_oracle.kmer_text(acgt, 4) == "ACGT"
    t64 = kf_oracle.canonical_kmers(b"T" * 64, 64)
    assert t64 == [0]  # poly-T is poly-A's reverse complement, at the widest key too
    assert kf_oracle.canonical_kmers(b"C" * 64, 64) == [int("01" * 64, 2)]


@pytest.mark.parametrize("k", [1, 2, 3, 5, 31, 32, 33, 47, 63, 64])
def test_vectorised_windows_are_the_plain_rule(k):
    rng = np.random.default_rng(k)
    seq = bytes(rng.choice(np.frombuffer(b"ACGTACGTACGTACGTacgtN", np.uint8), 400).tolist())
    hi, lo, ok = kf_oracle.windows_numpy(seq, k)
    got = [(int(h) << 64) | int(l) for h, l, o in zip(hi.tolist(), lo.tolist(), ok.tolist()) if o]
    assert got == kf_oracle.canonical_kmers(seq, k)


@pytest.mark.parametrize("fx", ["a", "b"])
def test_tiny_golden_pairs(fx):
    with open(os.path.join(GOLD, "tiny_%s.json" % fx)) as f:
        meta = json.load(f)
    data = [open(os.path.join(GOLD, "tiny_%s.%d.fq" % (fx, m)), "rb").read() for m in (1, 2)]
    r = kf_oracle.run(meta["k"], data[0], data[1])
    assert [list(x) for x in r["histogram"]] == meta["histogram"]
    assert (r["q1"], r["q3"], r["upper"], r["windows"], r["distinct"]) == (
        meta["q1"], meta["q3"], meta["upper"], meta["windows"], meta["distinct"])
    assert [[kf_oracle.kmer_text(x, meta["k"]), c] for x, c in r["abundant"]] == meta["abundant"]
    assert (r["verdict"], r["verdict1"], r["verdict2"]) == (meta["verdict"], meta["verdict1"], meta["verdict2"])
    recs = [kf_oracle.parse_fastq(d) for d in data]
    for m in (0, 1):
        want = b"".join(b"\n".join(rec) + b"\n" for rec, v in zip(recs[m], meta["verdict"]) if not v)
        assert r["out%d" % (m + 1)] == want
    assert r["report"] == b"abundance threshold for k-mer filtering:  %d\n" % meta["upper"]
    # the same counts by the plain rule, window by window
    plain = {}
    for rs in recs:
        for rec in rs:
            for x in kf_oracle.canonical_kmers(rec[1], meta["k"]):
                plain[x] = plain.get(x, 0) + 1
    assert kf_oracle.histogram(plain) == r["histogram"]
    if fx == "a":
        assert meta["abundant"] == [["AAA", 19]] and meta["upper"] == 15 and meta["verdict2"][2] == 1 and \
            meta["verdict1"][2] == 0


def test_fastq_rules_of_the_restatement():
    good = b"@a\nACGT\n+\nIIII\n"
    assert kf_oracle.parse_fastq(good) == kf_oracle.parse_fastq(good[:-1]) == [(b"@a", b"ACGT", b"+", b"IIII")]
    assert kf_oracle.parse_fastq(b"@a\n\n+\n\n") == [(b"@a", b"", b"+", b"")]
    assert kf_oracle.parse_fastq(b"@a\nAC\n+x\n@I\n")[0][3] == b"@I"  # a quality line may start with '@'
    for data, line in ((b"a\nAC\n+\nII\n", 1), (good + b"@b\nAC\n-\nII\n", 7), (good + b"@b\nAC\n+\nI\n", 8),
                       (good + b"@b\nAC\n+\n", 8), (good + b"@b\nAC\n", 7), (good + b"\n", 5), (b"\n", 1),
                       (b"@a\r\nAC\r\n+\r\nII\n", 4)):
        with pytest.raises(kf_oracle.FastqError) as e:
            kf_oracle.parse_fastq(data, 1)
        assert (e.value.file, e.value.line) == (1, line), data
    with pytest.raises(kf_oracle.FastqError) as e:
        kf_oracle.parse_pair(good + good, good)
    assert (e.value.file, e.value.line) == (1, 5)
    with pytest.raises(kf_oracle.FastqError) as e:
        kf_oracle.parse_pair(good, good + good + good)
    assert (e.value.file, e.value.line) == (0, 5)


@pytest.mark.parametrize("name,k", [("small", k) for k in kfcases.KS_SMALL] + [("big", kfcases.KS_BIG[0])])
def test_workload_meets_the_conditions_the_gpu_tests_rely_on(name, k):
    assert kfcases.meets_conditions(kfcases.expected(name, k)) == []


def test_special_workloads():
    r = kfcases.expected("tiny", 1)  # k = 1: two k-mers, both below 10001, nothing abundant
    assert len(r["histogram"]) == 2 and r["upper"] >= 5 and r["abundant"] == [] and sum(r["verdict"]) == 0
    with pytest.raises(kf_oracle.DegenerateHistogram):  # k = 1 on the small workload: both k-mers in row 10001
        kfcases.expected("small", 1)
    r = kfcases.expected("poly_a", 31)
    assert r["histogram"][-1] == (10001, 1) and r["abundant"][0] == (0, 2 * 100 * 70)
    assert kfcases.meets_conditions(r) == []
    assert sum(r["verdict"][-100:]) == 100


def test_workload_is_deterministic_and_well_formed():
    from muchsalsa_amd import synth
    a, b = synth.kmer_filter_workload(**kfcases.SMALL)
    assert (a, b) == kfcases.workload("small")
    r1, r2 = kf_oracle.parse_pair(a, b)
    assert len(r1) == 30000 * 30 // 200 and all(len(r[1]) == 100 for r in r1 + r2)
    assert r1[0][0] == b"@p0000/1" and r2[-1][0] == b"@p4499/2"
    assert any(r[3].startswith(b"@") for r in r1)
    assert any(b"N" in r[1] for r in r1) and any(r[1] != r[1].upper() for r in r2)


def test_no_device_means_an_error_not_a_fallback(kf, tmp_path):
    import torch
    if torch.cuda.is_available():
        return
    from muchsalsa_amd import _lib
    p = [str(tmp_path / n) for n in ("1.fq", "2.fq", "report.txt", "o1.fq", "o2.fq")]
    for x in p[:2]:
        open(x, "wb").write(b"@a\nACGT\n+\nIIII\n")
    with pytest.raises(kf.KmerFilterError) as e:
        kf.run(3, *p)
    assert e.value.code == _lib.E_NODEVICE and not any(os.path.exists(x) for x in p[2:])
