"""Bubble popping of the short-read unitig assembly (rule 9), host side (no GPU): the plain-Python restatement
(tests/ug_bubble_oracle.py) against its own recorded results for the hand-made cases (tests/golden/unitigs_bubbles, made by
tools/make_unitig_bubble_fixtures.py), the conditions the GPU tests rely on (checked on the restatement alone), its strand
symmetry and invariants, the two new symbols of the C-ABI, the rule's sentences in the header and the docstring, and the
command line's argument check.

At k = 64 a 100-base read of the diploid workload holds 37 k-mers, 5.5 per haplotype position at 15x: too few of them are solid
for the issue's conditions (9 and 5 bubbles in the first round), so the conditions are asserted at k = 15, 31, 32, 33 and at
k = 64 only that bubbles are popped and the unitigs get fewer."""
import hashlib
import json
import os
import re
import subprocess
import sys

import pytest

import ug_bubble_oracle as bo
import ug_oracle
import ugbubblecases as cases
import ugcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "unitigs_bubbles")
HAND_AT = cases.HAND_AT


@pytest.fixture(scope="module")
def ug():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import unitigs
    return unitigs


@pytest.mark.parametrize("name,k", HAND_AT)
def test_restatement_against_its_recorded_results(name, k):
    with open(os.path.join(GOLD, "%s_k%d.json" % (name, k))) as f:
        want = json.load(f)
    assert cases.params(name, k) == {key: want[key] for key in ("bubble", "trim", "min_length")}
    r = cases.expected(name, k)[0]
    assert [list(x) for x in r["rounds"]] == want["rounds"] and [list(x) for x in r["bubble_rounds"]] == want["bubble_rounds"]
    for key in ("records", "windows", "distinct", "solid", "solid_after", "bubble_phases", "bubbles", "bubble_branches",
                "bubble_kmers", "longest"):
        assert r[key] == want[key], key
    assert len(r["unitigs"]) == want["unitigs"] and len(cases.plain(name, k)["unitigs"]) == want["unitigs_without"]
    assert hashlib.sha256(r["all"]).hexdigest() == want["all_sha256"]
    assert hashlib.sha256(r["cut"]).hexdigest() == want["cut_sha256"]


def test_the_prototypes_figures():
    """what the issue quotes for the hand-made cases at k = 21"""
    edge = cases.expected("edge", 21)[0]
    assert edge["bubble_kmers"] == 21 and (len(cases.plain("edge", 21)["unitigs"]), len(edge["unitigs"])) == (4, 1)
    assert [r[4] for r in cases.expected("nested", 21)[0]["bubble_rounds"]] == [21, 33, 0]
    three = cases.expected("three_way", 21)[0]["bubble_rounds"]
    assert three[0][2:] == (1, 2, 42)
    alt = cases.expected("alternate", 21)[0]
    assert alt["rounds"][-2:] == [(63, 37), (63, 0)] and alt["bubble_rounds"][-1] == (len(alt["rounds"]), 0, 0, 0, 0)


@pytest.mark.parametrize("name,k", HAND_AT)
def test_hand_cases_meet_their_conditions(name, k):
    assert cases.meets_conditions(name, k) == []


@pytest.mark.parametrize("name", cases.DIPLOID)
@pytest.mark.parametrize("k", cases.KS_DIPLOID)
def test_diploid_workload_meets_the_conditions(name, k):
    if k in cases.KS_CONDITIONS:
        assert cases.meets_conditions(name, k) == []
        return
    on, off = cases.expected(name, k)[0], cases.plain(name, k)
    assert on["bubbles"] >= 5 and len(on["unitigs"]) < len(off["unitigs"]) and on["longest"] > off["longest"]


def test_the_generators_are_deterministic():
    from muchsalsa_amd import synth
    assert synth.unitig_bubble_cases(21) == synth.unitig_bubble_cases(21)
    a, b = synth.diploid_workload(error=0.004), synth.diploid_workload(error=0.004)
    assert a == b and a[0] != synth.diploid_workload()[0]
    kinds = [v[1] for v in a[2]["variants"]]
    assert len(kinds) == 15 and 5 <= kinds.count("snp") <= 10 and "ins" in kinds and "del" in kinds
    h1, h2 = a[2]["haplotypes"]
    assert len(h1) == 6000 and h1 != h2 and a[0].count(b"\n") == 4 * (15 * len(h1) // 100 + 15 * len(h2) // 100)


def test_bubble_zero_is_the_plain_restatement():
    want = ugcases.expected("small", 31)
    got = bo.run(31, ugcases.files("small"), 0)
    assert (got["bubble"], got["bubble_rounds"], got["bubble_phases"], got["bubbles"], got["bubble_kmers"]) == (0, [], 0, 0, 0)
    assert {key: got[key] for key in want} == want


@pytest.mark.parametrize("name,k", [(n, 31) for n in cases.DIPLOID] + HAND_AT)
def test_strand_symmetry(name, k):
    a, b = cases.expected(name, k)[0], cases.expected(name, k, flip=True)[0]
    assert a["all"] == b["all"] and a["cut"] == b["cut"]
    assert (a["rounds"], a["bubble_rounds"], a["unitigs"]) == (b["rounds"], b["bubble_rounds"], b["unitigs"])


def _invariants(r, min_length):
    """test_unitigs_host._invariants for a popped result"""
    k = r["k"]
    seen = set()
    for chain in r["chains"]:
        for x in chain:
            c = ug_oracle.canon(x, k)
            assert c not in seen, "a k-mer lies in two unitigs"
            seen.add(c)
    assert seen == set(r["counts"])  # every surviving k-mer in exactly one unitig
    assert sum(t[0] - k + 1 for t in r["unitigs"]) == r["solid_after"] == len(r["counts"])
    removed = sum(n for _, n in r["rounds"]) + r["bubble_kmers"]
    assert r["solid"] - removed == r["solid_after"] and r["bubble_kmers"] == sum(b[4] for b in r["bubble_rounds"])
    recs = r["all"].split(b"\n")
    assert recs[-1] == b"" and len(recs) == 2 * len(r["unitigs"]) + 1
    firsts = [t[2] for t in r["unitigs"]]
    assert firsts == sorted(firsts)
    for i, (t, chain) in enumerate(zip(r["unitigs"], r["chains"])):
        head, seq = recs[2 * i], recs[2 * i + 1]
        assert head == b">%d %d %d" % (i, t[0], t[1]) and len(seq) == t[0] and seq == seq.upper()
        assert r["all"][t[3]:t[3] + t[0]] == seq
        assert t[1] == sum(r["counts"][ug_oracle.canon(x, k)] for x in chain)
        if t[4]:
            assert chain[0] == min(min(chain), min(ug_oracle.rc(x, k) for x in chain))
        else:
            assert chain[0] <= ug_oracle.rc(chain[-1], k)
    cut = r["cut"].split(b"\n")
    kept = [(recs[2 * i], recs[2 * i + 1]) for i, t in enumerate(r["unitigs"]) if t[0] >= min_length]
    assert list(zip(cut[0::2], cut[1::2])) == kept and r["kept"] == len(kept)
    # the table of the bubble rounds: the tip rounds in front of a round never get fewer, a phase ends in a round that removes
    # nothing, and a round that removes k-mers removes branches of a bubble
    br = r["bubble_rounds"]
    assert [b[0] for b in br] == sorted(b[0] for b in br) and (not br or br[-1][4] == 0)
    assert all((b[4] > 0) == (b[3] > 0) and b[3] >= b[2] and b[2] <= 2 * b[1] for b in br)  # a fork holds at most two bubbles


@pytest.mark.parametrize("name,k", [(n, k) for n in cases.DIPLOID for k in cases.KS_DIPLOID] + HAND_AT)
def test_restatement_invariants(name, k):
    _invariants(cases.expected(name, k)[0], cases.params(name, k)["min_length"])


def test_the_restatement_rejects_bad_parameters():
    for bad in (-1, 4097):
        with pytest.raises(ValueError):
            bo.run(21, [cases.workload("edge")[0]], bad)


def test_abi_exports_the_bubble_symbols(ug):
    import ctypes as C
    from muchsalsa_amd import _lib
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_ug_set_bubbles", "msgpu_ug_result_bubbles"):
        assert hasattr(_lib.lib(), n) and n in bound and n + "(" in header, n
    assert "#define MSGPU_UG_BUBBLE_MAX 4096" in header and ug.BUBBLE_MAX == bo.BUBBLE_MAX == 4096
    assert C.sizeof(_lib.UgBubbleStats) == 4 * 4 + 4 * 8 + 4 * 4 and C.sizeof(_lib.UgBubbleRound) == 2 * 4 + 4 * 8 + 2 * 4
    for struct, fields in (("msgpu_ug_bubble_stats", _lib.UgBubbleStats), ("msgpu_ug_bubble_round", _lib.UgBubbleRound)):
        body = header[header.index("typedef struct " + struct):header.index("} " + struct + ";")]
        at = 0
        for name, _ in fields._fields_:  # every field, in the header's order
            m = re.compile(r"\b%s\b" % name).search(body, at)
            assert m, (struct, name)
            at = m.end()
    import inspect
    from muchsalsa_amd import hybrid
    assert inspect.signature(ug.run).parameters["bubble"].default is None
    assert inspect.signature(hybrid.run).parameters["bubble"].default is None


def test_the_statements_of_rule_9_agree(ug):
    """the rule's paragraphs in include/msgpu.h, in the module docstring and in DESIGN.md carry the same sentences"""
    header = " ".join(open(os.path.join(ROOT, "include", "msgpu.h")).read().replace(" *", " ").split())
    doc = " ".join(ug.__doc__.split())
    design = " ".join(open(os.path.join(ROOT, "DESIGN.md")).read().split())
    for phrase in ("0 means off, and rules 1-8 alone apply",
                   "if |pred(t)| >= 2 the branch is path and its merge is t; otherwise, if |path| = bubble there is no branch",
                   "A successor of u that is itself a merge (|pred| >= 2) is no branch",
                   "A bubble is judged once, from the side whose fork is the smaller 2k-bit string: from u iff u < rc(t)",
                   "branch A beats branch B iff sum(A) len(B) > sum(B) len(A)",
                   "Among equals, the branch entered from the judging fork by the smaller base c wins",
                   "all losers leave together when the round ends",
                   "If the bubble phase removed nothing in total, or trim = 0, cleaning is done",
                   "the round at trim alone, repeated until it removes nothing",
                   "zero-length branches are left alone, and there is no erosion"):
        assert phrase in header and phrase in doc and phrase in design, phrase
    for word in ("bubble popping only on request", "erosion", "--bubble N"):
        assert word in doc, word


def test_command_line_rejects_a_bad_bubble(ug, tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT)
    p = [str(tmp_path / n) for n in ("1.fq", "2.fq", "all.fa", "cut.fa")]
    for args in (["--bubble", "-1"], ["--bubble", "5000"], ["--bubble", "x"], ["--bubble"]):
        out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.unitigs", "31"] + p + args, cwd=ROOT, env=env,
                             capture_output=True, timeout=300)
        assert out.returncode == 2 and b"[--bubble N]" in out.stderr, args
    assert not any(os.path.exists(x) for x in p[2:])
