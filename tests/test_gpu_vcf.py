"""The polisher's VCF output on the GPU (msgpu_vcf.hip; rules V1 - V9): every case of tests/plcases.py, tests/pledgecases.py and
tests/vcfcases.py through run_tables(vcf=...), the text byte for byte and the variant table row for row against the
plain-Python restatement (tests/vcf_oracle.py), then against the hand-written lines, without any tolerance; the FASTA, the
record table and the counts equal to those of the same run without ``vcf``; the ranked and the mates form against their
restatements' voters; V7's refusals with a good case on the same context behind each; a small run behind a large one on one
context; polish.run on the planted workload; the command line in a fresh process; the pipeline's driver.  ``check_case`` and
the tests that tests/test_gpu_vcf_poisoned.py repeats take what they need as arguments.  No test provokes a device fault: a
bad input ends in an error before any kernel reads through it.  Every test runs under its own time limit."""
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import pytest

import map_oracle
import pl_mate_oracle
import pl_oracle
import pl_rank_oracle
import plcases
import pledgecases
import vcf_oracle
import vcfcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test
CASES = [("hand", n) for n in plcases.HAND] + [("edge", n) for n in pledgecases.names()] + [("vcf", n) for n in vcfcases.names()]


@pytest.fixture(scope="module")
def pl():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import polish
    return polish


@pytest.fixture(scope="module")
def stage(pl):
    with pl.Context() as ctx:
        yield ctx


@pytest.fixture(autouse=True)
def time_limit(pl):  # (after pl: the build is not the test's time)
    faulthandler.dump_traceback_later(LIMIT, exit=True)  # works while the main thread sits in a native call
    yield
    faulthandler.cancel_dump_traceback_later()


def run_case(pl, d, c, vcf, **how):
    """run_tables on a case's files -> (the result, the tables, the FASTA, the VCF file's bytes or None)"""
    dp, rp = plcases.write_case(c, d)
    out, vp = os.path.join(str(d), "out.fa"), os.path.join(str(d), "out.vcf")
    for path in (out, vp):
        if os.path.exists(path):
            os.remove(path)
    tb = {}
    res = pl.run_tables(dp, rp, out, c["chains"], c["runs"], tables=tb, **dict(c["params"], **how), **({"vcf": vp} if vcf else {}))
    assert os.path.exists(vp) == bool(vcf)
    with open(out, "rb") as h:
        text = h.read()
    return res, tb, text, open(vp, "rb").read() if vcf else None


def same_vcf(pl, got, want):
    """the text, the rows and the counts against the restatement's"""
    from muchsalsa_amd import _lib
    res, tb, _, text = got
    assert len(text) == len(want["text"]) and text == want["text"] == tb["vcf"]
    assert tb["variants"] == want["rows"]
    v = res["vcf"]
    assert {k: v[pl._strip(k)] for k in vcf_oracle.COUNTS} == {k: want[k] for k in vcf_oracle.COUNTS}
    assert v["short"] == sum(r[9] <= _lib.VCF_SHORT_BYTES for r in want["rows"]) and v["short"] + v["long"] == len(want["rows"])
    assert v["bytes_peak"] == res["bytes_peak"] and res["lost_publications"] == 0


def check_case(pl, stage, d, c, want, lines=None, **how):
    """with ``vcf``: the restatement, then the literals; and everything else as in the same run without it"""
    got = run_case(pl, d, c, True, context=stage, **how)
    print(c.get("note", ""), got[0]["vcf"])
    same_vcf(pl, got, want)
    if lines is not None:
        assert got[3] == vcf_oracle.header(vcfcases.clean(c["draft"])) + b"".join(lines)
    plain = run_case(pl, d, c, False, context=stage, **how)
    assert "vcf" not in plain[0] and "vcf" not in plain[1] and "variants" not in plain[1]
    assert plain[2] == got[2] and plain[1]["text"] == got[1]["text"] and plain[1]["records"] == got[1]["records"]
    skip = ("bytes_peak", "vcf")
    assert {k: x for k, x in plain[0].items() if k not in skip} == {k: x for k, x in got[0].items() if k not in skip}
    assert plain[0]["bytes_peak"] <= got[0]["bytes_peak"]
    return got


def case_of(kind, name):
    """-> (the case, the restatement's VCF, the hand-written lines or None, the keywords of run_tables beside the parameters)"""
    if kind == "vcf":
        c = vcfcases.cases()[name]
        return c, vcfcases.expected(name), c["lines"], {}
    if kind == "hand":
        c = plcases.hand_cases()[name]
        return c, vcfcases.expected_of(c), None, {}
    c = pledgecases.cases()[name]
    if "ranks" not in c:
        return c, vcfcases.expected_of(c), None, {}
    voting = pl_rank_oracle.voters(c["chains"], c["ranks"], c["params"].get("min_identity", 0), c["min_mapq"])
    return c, vcfcases.expected_of(c, voting), None, dict(ranks=c["ranks"], min_mapq=c["min_mapq"])


@pytest.mark.parametrize("kind,name", CASES)
def test_case(pl, stage, tmp_path, kind, name):
    c, want, lines, how = case_of(kind, name)
    check_case(pl, stage, tmp_path, c, want, lines, **how)


def test_the_ranked_form_feeds_the_same_code(pl, stage, tmp_path):
    c, want, _, how = case_of("edge", "ranked_two_primaries_overlap")
    got = check_case(pl, stage, tmp_path, c, want, **how)
    u = c["draft"][0][1]
    assert got[3].endswith(vcfcases.ln(b"d0", 61, u[60:61], vcfcases.sw(u, 60), 3, 2, b"snp"))  # 2 X of one read against 1 '='


def test_the_mates_form_feeds_the_same_code(pl, stage, tmp_path):
    c, on_a, on_b = vcfcases.mates_case()
    draft = c["draft"][0][1]
    for rows, lines in ((on_a, []), (on_b, [vcfcases.ln(b"d0", 561, draft[560:561], draft[240:241], 3, 3, b"snp")])):
        want = vcfcases.expected_of(c, pl_mate_oracle.voters(c["chains"], rows, 0))
        check_case(pl, stage, tmp_path, c, want, lines, mates=rows)


def test_v7_refuses_a_name_and_the_context_goes_on(pl, stage, tmp_path):
    """each bad name -> MSGPU_E_ARG naming the record, neither file written; without ``vcf`` the same draft polishes; the same
    context then writes a good case's VCF"""
    from muchsalsa_amd import _lib
    out, vp = os.path.join(str(tmp_path), "out.fa"), os.path.join(str(tmp_path), "out.vcf")
    good = vcfcases.cases()["ins_trailing_slot"]
    for tag, (c, record, why) in vcfcases.bad_names().items():
        dp, rp = plcases.write_case(c, tmp_path)
        for path in (out, vp):
            if os.path.exists(path):
                os.remove(path)
        with pytest.raises(pl.PolishError) as e:
            pl.run_tables(dp, rp, out, c["chains"], c["runs"], context=stage, vcf=vp)
        print(tag, e.value)
        assert e.value.code == _lib.E_ARG and "VCF: draft record %d: %s" % (record, why) in str(e.value), tag
        assert not os.path.exists(out) and not os.path.exists(vp)
        res = pl.run_tables(dp, rp, out, c["chains"], c["runs"], context=stage)  # (the names are checked only when VCF is asked for)
        assert res["pos_substituted"] == 1 and os.path.exists(out)
        check_case(pl, stage, tmp_path, good, vcfcases.expected("ins_trailing_slot"), good["lines"])


def test_nothing_of_a_large_run_survives_into_the_next(pl, stage, tmp_path):
    runs = [check_case(pl, stage, tmp_path, *case_of("vcf", n)[:3]) for n in ("del_40000", "blocks_300", "snp_first", "del_40000")]
    assert runs[0][3] == runs[3][3] and runs[0][1] == runs[3][1]


@pytest.fixture(scope="module")
def planted(pl, tmp_path_factory):
    """polish.run(vcf=...) on the planted workload, once: (result, tables, FASTA, VCF, draft path, reads path, timings)"""
    d = tmp_path_factory.mktemp("planted")
    dp, rp = plcases.write_workload("planted", d)
    out, vp = os.path.join(str(d), "out.fa"), os.path.join(str(d), "out.vcf")
    tb, tm = {}, {}
    res = pl.run(dp, rp, out, tables=tb, timings=tm, vcf=vp)
    assert sorted(os.listdir(str(d))) == ["draft.fa", "out.fa", "out.vcf", "reads.fa"]
    return res, tb, open(out, "rb").read(), open(vp, "rb").read(), dp, rp, tm


def test_planted_through_the_mapper(pl, planted):
    res, tb, text, vcf = planted[:4]
    wl = plcases.workload("planted")
    want_pl, mapped = plcases.expected_workload("planted")
    draft, reads = map_oracle.parse(wl["draft"], False), map_oracle.parse(wl["reads"], False)
    want = vcf_oracle.run(draft, reads, mapped["chains"], mapped["packed"])
    print(res["vcf"], planted[6])
    same_vcf(pl, (res, tb, text, vcf), want)
    assert text == want_pl["text"] and "vcf" in planted[6]
    v = res["vcf"]
    assert v["variants"] == 132 and [v[t] for t in vcf_oracle.TYPES] == [want["n_" + t] for t in vcf_oracle.TYPES] == [13, 30, 39, 49, 1]
    assert [b for _, b in vcf_oracle.apply(draft, vcf)] == [b"".join(want_pl["text"].split(b"\n")[1:])]


def test_the_command_line_in_a_fresh_process(pl, planted, tmp_path):
    text, vcf, dp, rp = planted[2:6]
    out, vp = os.path.join(str(tmp_path), "cli.fa"), os.path.join(str(tmp_path), "cli.vcf")
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, "-m", "muchsalsa_amd.polish", dp, rp, out, "--vcf", vp], cwd=ROOT, env=env, capture_output=True, timeout=LIMIT)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.decode().strip().splitlines()[-1])
    assert open(out, "rb").read() == text and open(vp, "rb").read() == vcf
    assert line["vcf"]["variants"] == 132 and line["vcf"]["text_bytes"] == len(vcf) and "vcf" in line["seconds"]
    run = subprocess.run([sys.executable, "-m", "muchsalsa_amd.polish", dp, rp, out, "--vcf", vp, "--rounds", "2"], cwd=ROOT, env=env, capture_output=True,
                         timeout=LIMIT)
    assert run.returncode == 2 and b"--vcf F" in run.stderr


def test_the_driver_writes_the_vcf_beside_the_polished_file(pl, tmp_path):
    """hybrid.run(polish=1, vcf=True): every recorded file at its recorded digest, the polished file and the VCF those of
    polish.run on the two files the run names"""
    import hybridcases
    from muchsalsa_amd import hybrid
    (tmp_path / "in").mkdir()
    inputs = hybridcases.write_inputs(tmp_path / "in")
    res = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2], str(tmp_path / "out"), polish=1, vcf=True)
    out = os.path.realpath(str(tmp_path / "out"))
    wrong = []
    for rel, rec in sorted(hybridcases.expected()["files"].items()):
        data = open(os.path.join(out, rel), "rb").read()
        if (len(data), hashlib.sha256(data).hexdigest()) != (rec["bytes"], rec["sha256"]):
            wrong.append(rel)
    assert wrong == []
    files = res["files"]
    assert files["polished_vcf"] == os.path.join(out, hybrid.POLISHED_VCF_NAME) and "polished_mates_vcf" not in files
    alone, alone_vcf = os.path.join(str(tmp_path), "alone.fa"), os.path.join(str(tmp_path), "alone.vcf")
    got = pl.run(files["assembly"], files["scrubbed"], alone, vcf=alone_vcf)
    assert open(alone, "rb").read() == open(files["polished"], "rb").read()
    vcf = open(files["polished_vcf"], "rb").read()
    assert vcf == open(alone_vcf, "rb").read() and vcf.startswith(b"##fileformat=VCFv4.2\n")
    print(res["polish"]["vcf"])
    assert {k: x for k, x in res["polish"]["vcf"].items() if k != "bytes_peak"} == {k: x for k, x in got["vcf"].items() if k != "bytes_peak"}
    draft = map_oracle.parse(open(files["assembly"], "rb").read(), False)
    polished = map_oracle.parse(open(files["polished"], "rb").read(), False)
    assert [b for _, b in vcf_oracle.apply(draft, vcf)] == [vcf_oracle.folded(b) for _, b in polished]
    plain = {rel.split(os.sep)[0] for rel in hybrid.output_names(hybridcases.NAME, inputs[2]).values()}
    assert sorted(set(os.listdir(out)) - plain) == [hybrid.POLISHED_NAME, hybrid.POLISHED_VCF_NAME]
