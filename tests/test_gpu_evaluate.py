"""Assembly evaluation on the GPU: every test runs the stage on files and compares, without any tolerance on an integer,
with the plain-Python restatement (tests/ev_oracle.py): the records, the total, the spectrum, the intervals, solid / found and
the three texts.  The report is compared field by field: integers equal, the qv column within 0.011 of the oracle's (two
decimals, so a last-ulp difference may move one unit of the last place).  Malformed inputs are rejected with an error code;
no test provokes a device fault.  Every test runs under its own time limit."""
import ctypes as C
import faulthandler
import json
import os

import numpy as np
import pytest

import ev_oracle
import evcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def ev():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import evaluate
    return evaluate


@pytest.fixture(autouse=True)
def time_limit(ev):  # (after ev: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def read(path):
    with open(path, "rb") as h:
        return h.read()


def write(d, case, tag="x", name="assembly.fa"):
    """the case's files -> (in1, in2 or None, assembly)"""
    d = os.path.join(str(d), tag)
    os.makedirs(d, exist_ok=True)
    paths = []
    for i, data in enumerate(case["reads"]):
        paths.append(os.path.join(d, "%d.fq" % (i + 1)))
        with open(paths[-1], "wb") as h:
            h.write(data)
    asm = os.path.join(d, name)
    with open(asm, "wb") as h:
        h.write(case["assembly"])
    return paths[0], paths[1] if len(paths) > 1 else None, asm


def same_report(got, want):
    """field by field: integers and names equal, qv within 0.011"""
    g, w = got.decode().split("\n"), want.decode().split("\n")
    assert len(g) == len(w)
    for a, b in zip(g, w):
        fa, fb = a.split("\t"), b.split("\t")
        if len(fb) == 5 and not b.startswith("#") and fb[0] != "record" and fb[4] not in ("inf", "-"):
            assert fa[:4] == fb[:4] and abs(float(fa[4]) - float(fb[4])) <= 0.011, (a, b)
        else:
            assert a == b


def spectrum_dict(s):
    return {(int(c), int(a)): int(s[c, a]) for c, a in zip(*np.nonzero(s))}


def same_tables(t, want):
    assert t["records"] == want["records"] and t["total"] == want["total"]
    assert spectrum_dict(t["spectrum"]) == want["spectrum"]
    assert t["intervals"] == want["intervals"]
    same_report(t["report"], want["report"])


def check(ev, d, case, want, tag="x", **kw):
    """the stage by files against the restatement: every table, every text"""
    in1, in2, asm = write(d, case, tag)
    out = [os.path.join(os.path.dirname(asm), n) for n in ("report.tsv", "spectrum.tsv", "runs.bed")]
    tables = {}
    res = ev.run(case["k"], in1, in2, asm, out[0], min_count=case["min_count"], spectrum=out[1], bed=out[2], tables=tables, **kw)
    assert len(tables["assemblies"]) == 1 == len(res["assemblies"])
    same_tables(tables["assemblies"][0], want)
    same_report(read(out[0]), want["head"] + want["report"])
    assert read(out[1]) == want["spectrum_text"] and read(out[2]) == want["bed"]
    r = res["assemblies"][0]
    assert (r["length"], r["windows"], r["missing"]) == want["total"] and (r["solid"], r["found"]) == (want["solid"], want["found"])
    assert r["intervals"] == len(want["intervals"]) and r["records"] == len(want["records"])
    assert r["missing_distinct"] == sum(n for (c, a), n in want["spectrum"].items() if a == 0)
    assert r["lost_publications"] == 0 and (res["k"], res["min_count"]) == (case["k"], case["min_count"])
    return res, tables["assemblies"][0]


@pytest.mark.parametrize("k", evcases.KS_WIDTH)
def test_workload_at_every_key_width(ev, tmp_path, k):
    check(ev, tmp_path, evcases.workload(k), evcases.expected("workload", k))


@pytest.mark.parametrize("name", tuple(evcases.EDGE_CASES))
def test_edge_cases(ev, tmp_path, name):
    check(ev, tmp_path, evcases.EDGE_CASES[name](), evcases.expected(name))


@pytest.mark.parametrize("name", tuple(evcases.EDGE_CASES))
def test_edge_cases_on_a_poisoned_arena(ev, tmp_path, monkeypatch, name):
    monkeypatch.setenv("MSGPU_POISON", "1")
    check(ev, tmp_path, evcases.EDGE_CASES[name](), evcases.expected(name))


def test_row_10001_and_the_palindrome(ev, tmp_path):
    _, t = check(ev, tmp_path, evcases.poly_a(), evcases.expected("poly_a"))
    assert int(t["spectrum"][4, ev_oracle.ROWS - 1]) == 1 and int(t["spectrum"][:, ev_oracle.ROWS - 1].sum()) == 1
    _, t = check(ev, tmp_path, evcases.extreme("palindrome"), evcases.expected("palindrome"), tag="p")
    assert int(t["spectrum"][1, 1]) >= 1


def _partitions(ev, in1, in2, k, mb):
    try:
        with ev.Table(k, in1, in2, budget_mb=mb) as t:
            return t.stats["partitions"]
    except ev.EvaluateError:  # not even the finest cut fits
        return 1 << 30


def _budget_for(ev, in1, in2, k, windows, parts, per_key):
    """a budget (MiB) under which the count cuts the keys into exactly ``parts`` partitions: the number the table reports
    falls as the budget grows, so the search is a bisection on the budget"""
    lo, hi = 0.0, 1.2 * windows * per_key / (1 << 20) + 1  # hi: everything in one partition
    for _ in range(40):
        mid = (lo + hi) / 2
        got = _partitions(ev, in1, in2, k, mid)
        if got == parts:
            return mid
        if got > parts:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no budget gives %d partitions" % parts)


@pytest.mark.parametrize("k,per_key", [(31, 20), (33, 36)])
def test_partitions_do_not_change_the_result(ev, tmp_path, k, per_key):
    case, want = evcases.workload(k), evcases.expected("workload", k)
    in1, in2, asm = write(tmp_path, case, "b")
    windows = sum(len(x) - k + 1 for data in case["reads"] for x in data.split(b"\n")[1::4] if len(x) >= k)
    seen = []
    for parts in (1, 3):
        mb = _budget_for(ev, in1, in2, k, windows, parts, per_key)
        res, t = check(ev, tmp_path, case, want, tag="p%d" % parts, budget_mb=mb)
        with ev.Table(k, in1, in2, budget_mb=mb) as table:
            assert table.stats["partitions"] == parts
        seen.append((t["records"], t["total"], t["spectrum"].tobytes(), t["intervals"], t["report"]))
    assert seen[0] == seen[1]


def test_two_assemblies_on_one_table_equal_two_runs(ev, tmp_path):
    """in both orders: the assembly counts of the first run must not reach the second"""
    k = 31
    a, b = evcases.workload(k), evcases.extreme("copies")
    b = dict(b, reads=a["reads"], k=k)
    wa = evcases.expected("workload", k)
    wb = ev_oracle.run(k, a["reads"], b["assembly"], name="second.fa", min_count=2)
    in1, in2, asm_a = write(tmp_path, a, "t")
    asm_b = write(tmp_path, b, "t", name="second.fa")[2]
    with ev.Table(k, in1, in2) as table:
        assert table.stats["records"] == [320, 320] and table.stats["distinct"] == sum(n for (c, x), n in wa["spectrum"].items() if x)
        for order in ((asm_a, asm_b), (asm_b, asm_a), (asm_a, asm_a)):
            tables = {}
            report = os.path.join(str(tmp_path), "both.tsv")
            res = ev.run(k, None, None, list(order), report, table=table, tables=tables)
            wants = [wa if p == asm_a else wb for p in order]
            for t, w in zip(tables["assemblies"], wants):
                same_tables(t, w)
            same_report(read(report), wa["head"] + b"".join(w["report"] for w in wants))
            assert all(r["lost_publications"] == 0 for r in res["assemblies"])
        with pytest.raises(ev.EvaluateError) as e:  # another k than the table's
            ev.run(21, None, None, asm_a, report, table=table)
        assert "k = 21" in str(e.value)
        with pytest.raises(ev.EvaluateError) as e:  # a second table in the context: as a second index in the mapper's
            from muchsalsa_amd import _lib
            h = C.c_void_p()
            table.stage.check(_lib.lib().msgpu_ev_table_open(table.stage.ctx, k, os.fsencode(in1), None, 0, C.byref(h)))
        assert e.value.code == _lib.E_STATE and "free it first" in str(e.value)
        same_tables_after = {}
        ev.run(k, None, None, asm_a, report, table=table, tables=same_tables_after)  # the table is still usable
        same_tables(same_tables_after["assemblies"][0], wa)


def test_a_table_from_a_pair_and_one_reads_file(ev, tmp_path):
    from muchsalsa_amd import kmer_filter
    k = 31
    case, want = evcases.workload(k), evcases.expected("workload", k)
    in1, in2, asm = write(tmp_path, case, "t")
    report = os.path.join(str(tmp_path), "r.tsv")
    with kmer_filter.Pair(in1, in2) as pair:
        with ev.Table(k, pair=pair) as table:
            tables = {}
            ev.run(k, None, None, asm, report, table=table, tables=tables)
            same_tables(tables["assemblies"][0], want)
            by_pair = table.stats
    with ev.Table(k, in1, in2) as table:
        assert {x: v for x, v in table.stats.items() if x != "seconds"} == {x: v for x, v in by_pair.items() if x != "seconds"}
    one = dict(case, reads=case["reads"][:1])
    check(ev, tmp_path, one, ev_oracle.run(k, one["reads"], one["assembly"]), tag="one")


def test_filter_then_evaluate_then_unitigs_on_one_pair(ev, tmp_path):
    """the pair is read, never written: each stage gives its by-files result"""
    from muchsalsa_amd import kmer_filter, unitigs
    k = 31
    case, want = evcases.workload(k), evcases.expected("workload", k)
    in1, in2, asm = write(tmp_path, case, "t")
    d = str(tmp_path)
    p = {n: os.path.join(d, n) for n in ("fr", "f1", "f2", "ua", "uc", "pr", "pa", "pc", "ev")}
    f_files = kmer_filter.run(21, in1, in2, p["fr"], p["f1"], p["f2"])
    u_files = unitigs.run(k, in1, in2, p["ua"], p["uc"], min_length=100)
    with kmer_filter.Pair(in1, in2) as pair:
        f_pair = kmer_filter.run(21, None, None, p["pr"], None, None, pair=pair)
        with ev.Table(k, pair=pair) as table:
            tables = {}
            ev.run(k, None, None, asm, p["ev"], table=table, tables=tables)
        u_pair = unitigs.run(k, None, None, p["pa"], p["pc"], pair=pair, min_length=100)
    same_tables(tables["assemblies"][0], want)
    same = ("pairs_in", "pairs_out", "windows", "distinct", "candidates", "q1", "q3", "upper", "abundant")
    assert [f_pair[x] for x in same] == [f_files[x] for x in same] and read(p["pr"]) == read(p["fr"])
    assert read(p["pa"]) == read(p["ua"]) and read(p["pc"]) == read(p["uc"]) and u_pair["unitigs"] == u_files["unitigs"] > 0


def test_errors_are_codes_with_their_text(ev, tmp_path):
    from muchsalsa_amd import _lib
    case = evcases.tiny()
    in1, _, asm = write(tmp_path, case, "e")
    report = os.path.join(str(tmp_path), "e.tsv")

    def fails(code, *words, **kw):
        args = dict(k=3, in1=in1, in2=None, assemblies=asm, min_count=1)
        args.update(kw)
        with pytest.raises(ev.EvaluateError) as e:
            ev.run(args.pop("k"), args.pop("in1"), args.pop("in2"), args.pop("assemblies"), report, **args)
        assert e.value.code == code and all(w in str(e.value) for w in words), str(e.value)
        assert not os.path.exists(report)
        return e.value

    for k in (0, 65):
        fails(_lib.E_ARG, "k = %d is outside 1..64" % k, k=k)
        fails(_lib.E_ARG, "k = %d is outside 1..64" % k, k=k, assemblies=[asm, asm])
    for m in (0, 10001):
        fails(_lib.E_ARG, "min_count = %d is outside 1..10000" % m, min_count=m)
    bad = os.path.join(str(tmp_path), "bad.fq")
    with open(bad, "wb") as h:
        h.write(b"@a\nACGT\n+\nIIII\n@b\nACGT\n-\nIIII\n")
    e = fails(_lib.E_FORMAT, "file 1 line 7", in2=bad)
    assert (e.file, e.line) == (1, 7)
    e = fails(_lib.E_FORMAT, "file 0 line 7", in1=bad)
    assert (e.file, e.line) == (0, 7)
    fails(_lib.E_IO, "cannot read", in1=os.path.join(str(tmp_path), "none.fq"))
    fails(_lib.E_IO, "assembly", "none.fa", assemblies=os.path.join(str(tmp_path), "none.fa"))
    fails(_lib.E_IO, "assembly", "none.fa", assemblies=[asm, os.path.join(str(tmp_path), "none.fa")])
    # the C entry points check min_count as well
    L, ctx, res = _lib.lib(), C.c_void_p(), C.c_void_p()
    assert L.msgpu_ev_create(0, C.byref(ctx)) == _lib.OK
    try:
        for m in (0, 10001):
            prm = _lib.EvParams(3, m, 0, 0)
            assert L.msgpu_ev_run(ctx, C.byref(prm), os.fsencode(in1), None, os.fsencode(asm), 0, 0, C.byref(res)) == _lib.E_ARG
            assert b"min_count" in L.msgpu_ev_last_error(ctx) and not res.value
        prm = _lib.EvParams(3, 1, 0, 0)
        assert L.msgpu_ev_run(ctx, C.byref(prm), os.fsencode(in1), None, os.fsencode(asm), 1, 0, C.byref(res)) == _lib.E_ARG  # flags
    finally:
        L.msgpu_ev_destroy(ctx)
    check(ev, tmp_path, case, evcases.expected("tiny"), tag="after")  # the stage is as usable as before

def test_a_pair_on_another_device_is_an_argument_error(ev, tmp_path):
    """needs two devices: a context cannot be made on a device that is not there"""
    import torch
    from muchsalsa_amd import _lib, kmer_filter
    if torch.cuda.device_count() < 2:  # (as tests/test_gpu_pair.py has it for msgpu_kf_run_pair)
        print("one device: the device check of msgpu_ev_table_open_pair was not run")
        return
    in1, _, _ = write(tmp_path, evcases.tiny(), "d")
    L, ctx, t = _lib.lib(), C.c_void_p(), C.c_void_p()
    with kmer_filter.Pair(in1, in1, device=0) as pair:
        assert L.msgpu_ev_create(1, C.byref(ctx)) == _lib.OK
        try:
            assert L.msgpu_ev_table_open_pair(ctx, 3, pair.handle, 0, C.byref(t)) == _lib.E_ARG and not t.value
            assert b"device" in L.msgpu_ev_last_error(ctx)
        finally:
            L.msgpu_ev_destroy(ctx)


def test_device_memory_returns(ev, tmp_path):
    """free memory after create / table / run / free / destroy is where it was"""
    import torch
    case = evcases.workload(31)
    in1, in2, asm = write(tmp_path, case, "m")
    report = os.path.join(str(tmp_path), "m.tsv")

    def every_path():
        with ev.Table(31, in1, in2) as table:
            ev.run(31, None, None, [asm, asm], report, table=table, bed=os.path.join(str(tmp_path), "m.bed"))
        ev.run(31, in1, in2, asm, report)

    every_path()  # warm-up: the runtime's pools, rocPRIM's kernels
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for _ in range(2):
        every_path()
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print("free device memory: %d bytes before the first create, %d after the last destroy" % (before, after))
    assert after >= before


# ---- the pipeline

@pytest.fixture(scope="module")
def hybrid_runs(ev, tmp_path_factory):
    """the driver with and without the stage, once each -> (inputs, with, folder, without, folder)"""
    import hybridcases
    from muchsalsa_amd import hybrid
    inputs = hybridcases.write_inputs(tmp_path_factory.mktemp("ev_hybrid_in"))
    args = (hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2])
    out_a = str(tmp_path_factory.mktemp("ev_hybrid_a") / "out")
    out_b = str(tmp_path_factory.mktemp("ev_hybrid_b") / "out")
    with_it = hybrid.run(*args, out_a, polish=1, evaluate=21)
    without = hybrid.run(*args, out_b, polish=1)
    print(json.dumps(with_it["evaluate"]))
    return inputs, with_it, out_a, without, out_b


def test_pipeline_writes_the_evaluation_and_nothing_else_changes(ev, hybrid_runs):
    from muchsalsa_amd import hybrid
    inputs, with_it, out_a, without, out_b = hybrid_runs
    assert with_it["files"]["evaluation"] == os.path.join(out_a, hybrid.EVALUATION_NAME) and "evaluation" not in without["files"]
    assert "evaluate" not in without and hybrid.EVALUATION_NAME not in hybrid.output_names("x", "y.fastq").values()
    seen = 0
    for folder, _, names in os.walk(out_b):
        for n in names:
            path = os.path.join(folder, n)
            if not os.path.islink(path):
                assert read(path) == read(os.path.join(out_a, os.path.relpath(path, out_b))), n
                seen += 1
    assert seen >= 14 and not os.path.exists(os.path.join(out_b, hybrid.EVALUATION_NAME))
    assert [a["assembly"] for a in with_it["evaluate"]["assemblies"]] == ["03.assembly.unpolished.fa", hybrid.POLISHED_NAME]


def test_pipeline_evaluation_equals_the_stage_by_files_and_the_oracle(ev, hybrid_runs, tmp_path):
    inputs, with_it, out_a, _, _ = hybrid_runs
    files = with_it["files"]
    report = os.path.join(str(tmp_path), "by_files.tsv")
    ev.run(21, inputs[0], inputs[1], [files["assembly"], files["polished"]], report)
    assert read(report) == read(files["evaluation"])
    reads = [read(inputs[0]), read(inputs[1])]
    R = ev_oracle.read_counts(21, reads)
    want = [ev_oracle.run(21, reads, read(files[key]), name=os.path.basename(files[key]), R=R) for key in ("assembly", "polished")]
    same_report(read(report), want[0]["head"] + want[0]["report"] + want[1]["report"])
    assert want[0]["total"][1] > 0
