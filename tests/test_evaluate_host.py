"""Assembly evaluation without a GPU: the symbols and the struct sizes, rule 4 on its own (msgpu_ev_qv), the plain-Python
restatement (tests/ev_oracle.py) on cases small enough to verify by hand and against its recorded results, the conditions
every named case is built to meet, the command line's usage errors and the three statements of the rules."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import pytest

import ev_oracle
import evcases
import kf_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "evaluate")
RECORDED = tuple(n for n in evcases.EDGE_CASES if n != "poly_a")


@pytest.fixture(scope="module")
def ev():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import evaluate
    return evaluate


def test_abi_exports_every_evaluation_symbol(ev):
    from muchsalsa_amd import _lib
    names = ["msgpu_ev_" + n for n in ("create", "destroy", "last_error", "error_line", "error_file", "default_params", "table_open",
                                       "table_open_pair", "table_stats", "table_free", "run_table", "run", "result_stats",
                                       "result_records", "result_spectrum", "result_intervals", "result_text", "result_free", "qv")]
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in names:
        assert n in bound and hasattr(_lib.lib(), n), n
    assert C.sizeof(_lib.EvParams) == 16 and C.sizeof(_lib.EvRecord) == 24 and C.sizeof(_lib.EvInterval) == 24
    assert C.sizeof(_lib.EvTableStats) == 8 * 8 + 2 * 4 + 10 * 4 and C.sizeof(_lib.EvStats) == 10 * 8 + 2 * 4 + 10 * 4
    p = _lib.EvParams()
    _lib.lib().msgpu_ev_default_params(C.byref(p))
    assert (p.k, p.min_count, p.intervals) == (21, 2, 0)
    assert (_lib.EV_CLASSES, _lib.EV_ROWS) == (ev_oracle.CLASSES, ev_oracle.ROWS) == (5, 10002)


def test_qv_is_the_formula(ev):
    """both sides use libm: a few ulp in three calls bound the difference by about 1e-14; 1e-9 absolute is asked"""
    for k in (1, 2, 21, 31, 32, 33, 64):
        for missing, windows in ((1, 2), (1, 3), (1, 10), (7, 1000), (1, 10 ** 6), (3, 4 * 10 ** 9), (999, 1000), (1, (1 << 31) - 1),
                                 (123456, 5 * 10 ** 6)):
            p = missing / windows
            want = -10 * math.log10(-math.expm1(math.log1p(-p) / k)) + 0.0
            assert abs(ev.qv(missing, windows, k) - want) <= 1e-9, (k, missing, windows)
            assert abs(ev_oracle.qv(missing, windows, k) - want) <= 1e-9


def test_qv_inf_none_and_zero(ev):
    from muchsalsa_amd import _lib
    assert ev.qv(0, 10, 21) == math.inf and ev_oracle.qv(0, 10, 21) == math.inf and ev_oracle.qv_text(0, 10, 21) == "inf"
    assert math.isnan(ev.qv(0, 0, 21)) and ev_oracle.qv(0, 0, 21) is None and ev_oracle.qv_text(0, 0, 21) == "-"
    for k in (1, 31, 64):  # e = 1: 0.00, never -0.00
        v = ev.qv(5, 5, k)
        assert v == 0.0 and math.copysign(1.0, v) == 1.0 and "%.2f" % v == "0.00" == ev_oracle.qv_text(5, 5, k)
    for bad in ((6, 5, 21), (1, 5, 0), (1, 5, 65)):
        with pytest.raises(ev.EvaluateError) as e:
            ev.qv(*bad)
        assert e.value.code == _lib.E_ARG
    # small p: the naive 1 - (1 - p) ** (1 / k) loses every digit here, the stated form does not
    assert abs(ev.qv(1, 10 ** 15, 21) - (-10 * math.log10(1e-15 / 21))) < 1e-6


def test_the_restatement_by_hand():
    """reads ACGTA, assembly ACGTT, k = 3.  Assembly windows ACG, CGT (= ACG reversed), GTT (canonical AAC); read windows ACG,
    CGT, GTA.  So R = {ACG: 2, GTA: 1}, A = {ACG: 2, AAC: 1}: one window of three is missing, the last"""
    w = evcases.expected("tiny")
    assert w["records"] == [("c", 5, 3, 1)] and w["total"] == (5, 3, 1)
    assert w["spectrum"] == {(2, 2): 1, (0, 1): 1, (1, 0): 1}
    assert w["intervals"] == [(0, 2, 5)] and (w["solid"], w["found"]) == (2, 1)
    assert w["head"] == b"#k\t3\tmin_count\t1\n"
    assert w["report"] == (b"#assembly\tassembly.fa\nrecord\tlength\twindows\tmissing\tqv\nc\t5\t3\t1\t8.98\ntotal\t5\t3\t1\t8.98\n"
                           b"completeness\t1\t2\t50.0000\n")
    assert w["spectrum_text"] == b"#assembly\tassembly.fa\n0\t0\t1\t0\t0\t0\n1\t1\t0\t0\t0\t0\n2\t0\t0\t1\t0\t0\n"
    assert w["bed"] == b"#assembly\tassembly.fa\nc\t2\t5\n"
    # k = 1: C and G are one key, missing from reads of A and T; touching runs of two records stay two intervals
    w = evcases.expected("runs_k1")
    assert w["records"] == [("a", 3, 3, 1), ("b", 3, 3, 1), ("c", 3, 3, 3), ("d", 1, 1, 1)]
    assert w["intervals"] == [(0, 2, 3), (1, 0, 1), (2, 0, 3), (3, 0, 1)]
    assert w["spectrum"] == {(4, 9): 1, (4, 0): 1}
    # the palindrome: ACGT once in the reads and once in the assembly
    w = evcases.expected("palindrome")
    assert w["spectrum"][(1, 1)] >= 1 and w["records"] == [("p", 6, 3, 2)] and w["intervals"] == [(0, 0, 4), (0, 2, 6)]


def test_intervals_by_hand():
    k = 11
    w = evcases.expected("intervals")
    want = [(0, 0, k), (0, 200 - k, 200),  # the first window alone, the last window alone
            (1, 50 - k + 1, 50 + k), (1, 50 + 2, 50 + k + 1 + k),  # window 51 between them is present: they overlap
            (2, 2 * 256 + 3 - 400 - k + 1, 2 * 256 + 3 - 400 + k)]  # windows 105..115 of a record at 400: store 505..515
    assert w["intervals"] == want and want[2][2] > want[3][1]
    t = evcases.expected("tiles")
    recs = evcases.tiles()["records"]
    last, nxt = len(recs) - 2, len(recs) - 1
    assert (last, 3 * k - k, 3 * k) in t["intervals"] and (nxt, 0, k) in t["intervals"]
    by_name = {r[0]: r for r in t["records"]}
    assert by_name["t5"][1:3] == (k - 1, 0) and by_name["t6"][1:3] == (k, 1) and by_name["t7"][1:3] == (k + 1, 2)
    assert by_name["t8"][1:3] == (0, 0) and all(by_name["t%d" % i][1:3] == (1, 0) for i in range(9, 309))


@pytest.mark.parametrize("name", RECORDED)
def test_restatement_against_its_recorded_results(name):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_evaluate_fixtures
    with open(os.path.join(GOLD, name + ".json")) as f:
        assert make_evaluate_fixtures.fixture(name) == json.load(f)


def _column_sums(case, want):
    rs = [kf_oracle.parse_fastq(data, f) for f, data in enumerate(case["reads"])]
    counts, _ = kf_oracle.count(rs[0], rs[1] if len(rs) > 1 else [], case["k"])
    sums = {}
    for (c, a), n in want["spectrum"].items():
        if a >= 1:
            sums[a] = sums.get(a, 0) + n
    assert sorted(sums.items()) == kf_oracle.histogram(counts)
    assert all(c >= 1 for (c, a) in want["spectrum"] if a == 0)


@pytest.mark.parametrize("name", tuple(evcases.EDGE_CASES))
def test_spectrum_columns_are_the_filters_histogram(name):
    _column_sums(evcases.EDGE_CASES[name](), evcases.expected(name))


@pytest.mark.parametrize("k", evcases.KS_WIDTH)
def test_workload_at_every_key_width(k):
    case, want = evcases.workload(k), evcases.expected("workload", k)
    _column_sums(case, want)
    assert want["total"][0] == sum(len(s) for _, s in case["records"])
    assert want["total"][2] == sum(e - s - k + 1 for _, s, e in want["intervals"])
    if k > 2:  # at k = 1 and 2 the reads hold every k-mer there is (2 and 10 canonical ones): nothing can be missing
        assert evcases.meets_conditions(want) == []
    else:
        assert want["total"][2] == 0 and not want["intervals"]


def test_cases_are_what_they_are_made_for():
    w = evcases.expected("nothing_missing")
    assert w["total"][2] == 0 and w["report"].splitlines()[-2].endswith(b"\tinf") and not w["intervals"]
    w = evcases.expected("all_missing")
    assert w["total"][1] == w["total"][2] > 0 and w["found"] == 0 and w["report"].splitlines()[-2].endswith(b"\t0.00")
    w = evcases.expected("no_assembly_window")
    assert w["total"][1] == 0 and w["report"].splitlines()[-2].endswith(b"\t-") and w["found"] == 0 < w["solid"]
    w = evcases.expected("no_read_window")
    assert w["solid"] == 0 and w["report"].endswith(b"completeness\t0\t0\t-\n") and w["total"][1] == w["total"][2] > 0
    w = evcases.expected("copies")
    assert {c for (c, a) in w["spectrum"] if a > 0} == {0, 1, 2, 3, 4} and w["total"][2] == 0  # copy numbers 1..6: u1 .. u6
    assert sorted({r[0].split("_")[0] for r in w["records"]}) == ["u%d" % i for i in range(1, 7)]
    w = evcases.expected("poly_a")
    assert [n for (c, a), n in w["spectrum"].items() if a == ev_oracle.ROWS - 1] == [1] and (4, ev_oracle.ROWS - 1) in w["spectrum"]


def test_small_files_lie_back_to_back_in_the_store(ev, tmp_path):
    """what the tile cases rest on: the loader puts the records of a small file one behind the other"""
    from muchsalsa_amd import _lib
    L = _lib.lib()
    case = evcases.tiles()
    path = tmp_path / "assembly.fa"
    path.write_bytes(case["assembly"])
    f = C.c_void_p()
    assert L.msgpu_seq_parse(os.fsencode(str(path)), -1, C.byref(f)) == _lib.OK
    try:
        n = L.msgpu_seq_count(f)
        assert n == len(case["records"])
        assert [L.msgpu_seq_offset(f, i) for i in range(n)] == evcases.offsets(case["records"])
        assert [L.msgpu_seq_length(f, i) for i in range(n)] == [len(s) for _, s in case["records"]]
    finally:
        L.msgpu_seq_free(f)


def test_the_three_statements_of_the_rules_agree(ev):
    header = " ".join(open(os.path.join(ROOT, "include", "msgpu.h")).read().replace(" *", " ").split())
    doc = " ".join(ev.__doc__.split())
    for phrase in ("any byte outside ACGTacgt breaks the windows that hold it", "It never crosses two records",
                   "A record shorter than k has 0 windows", "e = -expm1(log1p(-p) / k)", "so that e = 1 prints 0.00, never -0.00",
                   "c = min(A(x), 4)", "row 10001 is the filter's cap row", "That makes 5 x 10002 counters",
                   "found is the same sum over c >= 1", "A run of windows s..e gives (record, s, e + k)",
                   "A run never continues into the next record", "At most 2^30 distinct read k-mers",
                   "a 3 Gb genome is out of scope", "else MSGPU_E_NOMEM naming the sizes"):
        assert phrase in header and phrase in doc, phrase


def test_command_line_rejects_bad_arguments(ev, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = [str(tmp_path / n) for n in ("1.fq", "2.fq", "report.tsv", "a.fa")]

    def code(*args):
        out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.evaluate"] + list(args), cwd=ROOT, env=env, capture_output=True,
                             timeout=300)
        if out.returncode == 2:
            assert b"python -m muchsalsa_amd.evaluate" in out.stderr
        return out.returncode

    assert code() == 2 and code("31", *p[:3]) == 2 and code("x", *p) == 2
    assert code("31", *p, "--min-count", "0") == 2 and code("31", *p, "--min-count", "10001") == 2 and code("31", *p, "--min-count") == 2
    assert code("31", *p, "--budget-mb", "0") == 2 and code("31", *p, "--what", "1") == 2 and code("31", *p, "--bed") == 2
    assert not os.path.exists(p[2])


def test_no_device_means_an_error_not_a_fallback(ev, tmp_path):
    import torch
    if torch.cuda.is_available():
        return
    from muchsalsa_amd import _lib
    ctx = C.c_void_p()
    assert _lib.lib().msgpu_ev_create(0, C.byref(ctx)) == _lib.E_NODEVICE and not ctx.value
    case = evcases.tiny()
    p = [str(tmp_path / n) for n in ("1.fq", "a.fa", "report.tsv")]
    open(p[0], "wb").write(case["reads"][0])
    open(p[1], "wb").write(case["assembly"])
    for assemblies in ([p[1]], [p[1], p[1]]):
        with pytest.raises(ev.EvaluateError) as e:
            ev.run(3, p[0], None, assemblies, p[2], min_count=1)
        assert e.value.code == _lib.E_NODEVICE and not os.path.exists(p[2])
