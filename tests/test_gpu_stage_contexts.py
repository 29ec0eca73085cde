"""The five stage contexts (unitig filter, scrubber, k-mer filter, unitig assembly, mapper) on their one shared create /
destroy, device arena and error path: what the per-stage suites cannot see.  Each stage runs on its smallest recorded case,
through ``muchsalsa_amd._stage`` on the C ABI, and every text of its result is compared byte for byte with the stage's
plain-Python restatement (computed once)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import kf_oracle
import mapcases
import scrub_oracle
import uf_oracle
import ugcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
STAGES = ("uf", "scrub", "kf", "ug", "map")


def _gold(*name):
    with open(os.path.join(GOLD, *name), "rb") as f:
        return f.read()


def _write(d, name, data):
    p = os.path.join(d, name)
    with open(p, "wb") as f:
        f.write(data)
    return os.fsencode(p)


def _scrub_line(a, b, s, e, sb=None, eb=None):
    sb, eb = (s if sb is None else sb), (e if eb is None else eb)
    return b"%s\t4000\t%d\t%d\t+\t%s\t4000\t%d\t%d\t%d\t%d\t60\n" % (a, s, e, b, sb, eb, e - s, e - s)


class Case:
    """one stage on one input: ``args(bad)`` are msgpu_<prefix>_run's arguments between the context and the result (bad: the
    first input path does not exist), ``texts(res)`` every text of a result, ``want`` the restatement's"""

    def __init__(self, prefix, error_cls, args, texts, want, keep=()):
        self.prefix, self.error_cls, self.args, self.texts, self.want, self.keep = prefix, error_cls, args, texts, want, keep


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import _lib, kmer_filter, mapper, scrubber, unitig_filter, unitigs
    from muchsalsa_amd._stage import text_view
    L = _lib.lib()
    d = str(tmp_path_factory.mktemp("stages"))
    missing = os.fsencode(os.path.join(d, "missing.fa"))
    out = {}

    def one(fn):
        return lambda res: [bytes(text_view(fn, res))]

    def several(fn, which):
        return lambda res: [bytes(text_view(fn, res, w)) for w in which]

    # unitig filter: the smaller hand-derived fixture
    paf, fasta = _gold("unitig_filter", "b.paf"), _gold("unitig_filter", "b.fa")
    u = unitig_filter.UfPaf(os.fsdecode(_write(d, "uf.paf", paf)))
    fa = _write(d, "uf.fa", fasta)
    out["uf"] = Case("uf", unitig_filter.UnitigFilterError, lambda bad: (u.handle, missing if bad else fa, 0),
                     one(L.msgpu_uf_result_text), [uf_oracle.run(paf, fasta)[0]], keep=(u,))

    # scrubber: five reads in three chunks, subset size 3 (three batches; B and C are folded in two of them)
    anchors = (_scrub_line(b"u1", b"A", 0, 600, 300, 900) + _scrub_line(b"u1", b"B", 0, 600, 300, 900) +
               _scrub_line(b"u1", b"C", 0, 600, 3500, 3900) + _scrub_line(b"u2", b"B", 0, 600, 400, 800) +
               _scrub_line(b"u2", b"D", 0, 600, 300, 900) + _scrub_line(b"u3", b"C", 0, 600, 3400, 3950) +
               _scrub_line(b"u3", b"E", 0, 600, 300, 900))
    ava = _scrub_line(b"B", b"C", 0, 1000) + _scrub_line(b"C", b"B", 2000, 3000) + _scrub_line(b"B", b"C", 1200, 1900)
    rng = np.random.default_rng(0)
    reads = b"".join(b">%s\n%s\n" % (n, np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 4000)].tobytes())
                     for n in (b"A", b"B", b"C", b"D", b"E"))
    s = scrubber.ScrubPaf(os.fsdecode(_write(d, "sc.anchors.paf", anchors)), os.fsdecode(_write(d, "sc.ava.paf", ava)))
    rd = _write(d, "sc.reads.fa", reads)
    batches, st = scrub_oracle.scrub(anchors, ava, scrub_oracle.parse_fasta(reads), 3)
    assert st["batches"] == 3
    out["scrub"] = Case("scrub", scrubber.ScrubberError, lambda bad: (s.handle, missing if bad else rd, 3),
                        one(L.msgpu_scrub_result_text), [scrub_oracle.text(batches)], keep=(s,))

    # k-mer filter: the smaller recorded pair of files
    k = json.loads(_gold("kmer_filter", "tiny_a.json"))["k"]
    a, b = _gold("kmer_filter", "tiny_a.1.fq"), _gold("kmer_filter", "tiny_a.2.fq")
    pa, pb = _write(d, "kf.1.fq", a), _write(d, "kf.2.fq", b)
    want = kf_oracle.run(k, a, b)
    out["kf"] = Case("kf", kmer_filter.KmerFilterError, lambda bad: (k, missing if bad else pa, pb, 0, 0),
                     several(L.msgpu_kf_result_text, (_lib.KF_TEXT_OUT_A, _lib.KF_TEXT_OUT_B, _lib.KF_TEXT_REPORT)),
                     [want["out1"], want["out2"], want["report"]])

    # unitig assembly: the hand-made rings
    files = ugcases.files("rings")
    pu = [_write(d, "ug.%d.fq" % i, x) for i, x in enumerate(files)]
    prm_ug = _lib.UgParams(31, 2, -1, 100)
    want = ugcases.expected("rings", 31, min_length=100)
    out["ug"] = Case("ug", unitigs.UnitigError,
                     lambda bad: (C.byref(prm_ug), missing if bad else pu[0], pu[1] if len(pu) > 1 else None, 0, 0),
                     several(L.msgpu_ug_result_text, (_lib.UG_TEXT_ALL, _lib.UG_TEXT_CUT)), [want["all"], want["cut"]])

    # mapper: the hand-made perfect hit
    tp, qp = (os.fsencode(p) for p in mapcases.write_inputs("perfect", d))
    prm_map = _lib.MapParams()
    L.msgpu_map_default_params(C.byref(prm_map))
    out["map"] = Case("map", mapper.MapError, lambda bad: (C.byref(prm_map), missing if bad else tp, qp, 0, 0),
                      one(L.msgpu_map_result_text), [mapcases.expected("perfect")["paf"]])
    assert all(any(len(t) for t in c.want) for c in out.values())
    return out


def _run(case, bad=False):
    """a context of its own, one run, every text"""
    from muchsalsa_amd._stage import stage_context
    with stage_context(case.prefix, 0, case.error_cls) as stage:
        with stage.run(*case.args(bad)) as res:
            return case.texts(res)


@pytest.mark.parametrize("name", STAGES)
def test_two_contexts_two_identical_results(cases, name):
    first, second = _run(cases[name]), _run(cases[name])
    assert first == second
    assert [len(t) for t in first] == [len(t) for t in cases[name].want]
    assert first == cases[name].want


def test_no_device_memory_is_lost(cases):
    import torch
    for name in STAGES:  # warm-up: the runtime's pools, rocPRIM's kernels
        _run(cases[name])
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info(0)[0]
    for name in STAGES:
        for _ in range(2):
            assert _run(cases[name]) == cases[name].want
    torch.cuda.synchronize()
    after = torch.cuda.mem_get_info(0)[0]
    print("free device memory: %d bytes before the first create, %d after the last destroy" % (before, after))
    assert after >= before


@pytest.mark.parametrize("name", STAGES)
def test_a_failed_run_leaves_the_context_good(cases, name):
    from muchsalsa_amd import _lib
    from muchsalsa_amd._stage import stage_context
    case = cases[name]
    last_error = getattr(_lib.lib(), "msgpu_%s_last_error" % case.prefix)
    with stage_context(case.prefix, 0, case.error_cls) as stage:
        with pytest.raises(case.error_cls) as e:
            with stage.run(*case.args(True)):
                pass
        assert e.value.code == _lib.E_IO and "missing.fa" in str(e.value)
        assert last_error(stage.ctx) != b""
        with stage.run(*case.args(False)) as res:
            assert case.texts(res) == case.want
        assert last_error(stage.ctx) == b""
