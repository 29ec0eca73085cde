"""The polisher's VCF output without a GPU: the plain-Python restatement (tests/vcf_oracle.py) against the hand-written lines of
tests/vcfcases.py; its independent ``apply`` -- which parses the text alone -- reproducing the polished bases of the polisher's
restatement on every case of plcases, pledgecases and vcfcases and on the planted workload; the library's new symbols and
struct sizes; the constants of the header; the command's refusal of --vcf with --rounds 2; hybrid.output_names unchanged."""
import ctypes as C
import os
import re

import pytest

import map_oracle
import pl_mate_oracle
import pl_oracle
import pl_rank_oracle
import plcases
import pledgecases
import vcf_oracle
import vcfcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def polished_bases(fasta_text):
    """the records of the polisher's FASTA -> [bases]"""
    return [b"".join(rec.split(b"\n")[1:]) for rec in fasta_text.split(b">")[1:]]


def assert_applies(draft, polished_text, vcf_text):
    """vcf_oracle.apply on the draft gives the polished bases; compared folded, non-ACGT as N, since REF is folded"""
    got = vcf_oracle.apply(draft, vcf_text)
    assert [b for _, b in got] == [vcf_oracle.folded(b) for b in polished_bases(polished_text)]


@pytest.mark.parametrize("name", vcfcases.names())
def test_the_restatement_against_the_hand_written_lines(name):
    c, want = vcfcases.cases()[name], vcfcases.expected(name)
    head = vcf_oracle.header(vcfcases.clean(c["draft"]))
    assert want["lines"] == c["lines"]
    assert want["text"] == head + b"".join(c["lines"]) and want["header_bytes"] == len(head) and want["text_bytes"] == len(want["text"])
    assert [r[8:] for r in want["rows"]] == [(len(head) + sum(map(len, c["lines"][:i])), len(l)) for i, l in enumerate(c["lines"])]
    assert_applies(vcfcases.clean(c["draft"]), plcases.expected_tables(c)["text"], want["text"])


def test_the_cases_meet_what_they_were_built_for():
    from muchsalsa_amd import _lib
    c = vcfcases.cases()
    assert [len(c[n]["lines"][0]) - _lib.VCF_SHORT_BYTES for n in ("line_bound_minus_1", "line_bound", "line_bound_plus_1")] == [-1, 0, 1]
    assert len(c["del_40000"]["lines"][0]) > 40000 and len(c["blocks_300"]["lines"]) == 300 and len(c["records_300"]["draft"]) == 300
    assert [r[6:8] for r in vcfcases.expected("del_whole_record")["rows"]] == [(vcf_oracle.DEL, vcf_oracle.WHOLE)]
    assert [r[7] for r in vcfcases.expected("del_at_0")["rows"]] == [vcf_oracle.RIGHT]
    assert [r[7] for r in vcfcases.expected("del_at_end")["rows"]] == [vcf_oracle.LEFT]
    assert vcfcases.expected("no_edit")["rows"] == [] and vcfcases.expected("no_edit")["text"].endswith(b"FILTER\tINFO\n")
    assert {r[6] for n in vcfcases.names() for r in vcfcases.expected(n)["rows"]} == set(range(5))


@pytest.mark.parametrize("name", plcases.HAND)
def test_apply_reproduces_the_polish_on_the_hand_cases(name):
    c = plcases.hand_cases()[name]
    assert_applies(vcfcases.clean(c["draft"]), plcases.expected_hand(name)["text"], vcfcases.expected_of(c)["text"])


@pytest.mark.parametrize("name", pledgecases.names())
def test_apply_reproduces_the_polish_on_the_edge_cases(name):
    c = pledgecases.cases()[name]
    voting = pl_rank_oracle.voters(c["chains"], c["ranks"], c["params"].get("min_identity", 0), c["min_mapq"]) if "ranks" in c else None
    assert_applies(vcfcases.clean(c["draft"]), pledgecases.expected(name)["text"], vcfcases.expected_of(c, voting)["text"])


def test_apply_reproduces_the_polish_on_planted():
    wl = plcases.workload("planted")
    want, mapped = plcases.expected_workload("planted")
    draft, reads = map_oracle.parse(wl["draft"], False), map_oracle.parse(wl["reads"], False)
    got = vcf_oracle.run(draft, reads, mapped["chains"], mapped["packed"])
    assert_applies(draft, want["text"], got["text"])
    assert got["n_variants"] == 132 and [got["n_" + t] for t in vcf_oracle.TYPES] == [13, 30, 39, 49, 1]


def test_the_voters_are_an_argument():
    """the mates restatement's voters give another VCF than the plain ones where they differ"""
    c, on_a, on_b = vcfcases.mates_case()
    for rows in (on_a, on_b):
        pl_mate_oracle.check(c["draft"], c["reads"], c["chains"], c["runs"], rows)
    voting = pl_mate_oracle.voters(c["chains"], on_a, 0)
    assert voting == [1, 2, 4, 5, 7, 8] and pl_mate_oracle.voters(c["chains"], on_b, 0) == [0, 2, 3, 5, 6, 8]
    assert vcfcases.expected_of(c, voting)["rows"] == []
    draft = c["draft"][0][1]
    assert vcfcases.expected_of(c, pl_mate_oracle.voters(c["chains"], on_b, 0))["lines"] == [vcfcases.ln(b"d0", 561, draft[560:561], draft[240:241], 3, 3, b"snp")]


def test_the_bad_names_are_refused_by_the_restatement():
    for tag, (c, record, why) in vcfcases.bad_names().items():
        with pytest.raises(vcf_oracle.NameError_) as e:
            vcfcases.expected_of(c)
        assert (e.value.record, e.value.why) == (record, why), tag
    with pytest.raises(vcf_oracle.NameError_) as e:
        vcf_oracle.check_names([b"a", b"b", b"a"])
    assert (e.value.record, e.value.why) == (2, vcf_oracle.BAD_NAME[4])


def test_the_library_has_the_new_symbols_and_sizes():
    from muchsalsa_amd import _lib, polish
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    handle = C.CDLL(_lib.LIB_PATH)
    for name in ("msgpu_pl_result_vcf", "msgpu_pl_result_variants", "msgpu_pl_result_vcf_stats"):
        assert getattr(handle, name)
    assert C.sizeof(_lib.PlVariant) == 48 == _lib.PL_VARIANT_DTYPE.itemsize and C.sizeof(_lib.PlVcfStats) == 120 and C.sizeof(_lib.PlStats) == 256
    assert polish.VARIANT == vcf_oracle.ROW
    with open(os.path.join(ROOT, "include", "msgpu.h")) as h:
        text = h.read()
    defined = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (MSGPU_(?:PL_VCF|VCF_\w+)) (\d+)u", text)}
    assert defined == {"MSGPU_PL_VCF": _lib.PL_VCF, "MSGPU_VCF_SHORT_BYTES": _lib.VCF_SHORT_BYTES, "MSGPU_VCF_LINE_FIXED": _lib.VCF_LINE_FIXED}
    assert _lib.VCF_TYPES == vcf_oracle.TYPES


def test_vcf_with_two_rounds_is_usage_and_exit_status_2(capsys, tmp_path):
    from muchsalsa_amd import polish
    vcf = str(tmp_path / "x.vcf")
    assert polish.main(["draft.fa", "reads.fa", str(tmp_path / "out.fa"), "--vcf", vcf, "--rounds", "2"]) == 2
    assert "--vcf F" in capsys.readouterr().err and os.listdir(str(tmp_path)) == []
    assert polish.main(["draft.fa", "reads.fa", str(tmp_path / "out.fa"), "--vcf"]) == 2
    with pytest.raises(TypeError):
        polish.run("draft.fa", "reads.fa", str(tmp_path / "out.fa"), rounds=2, vcf=vcf)
    assert os.listdir(str(tmp_path)) == []


def test_the_driver_refuses_vcf_with_two_rounds_before_any_stage_and_its_names_stay(tmp_path):
    from muchsalsa_amd import hybrid
    inputs = []
    for n in ("a.fq", "b.fq", "n.fastq"):
        inputs.append(str(tmp_path / n))
        with open(inputs[-1], "wb") as h:
            h.write(b"@r\nACGT\n+\nIIII\n")
    for kw in (dict(polish=2), dict(polish_mates=2), dict(polish=1, polish_mates=3)):
        with pytest.raises(hybrid.HybridError) as e:
            hybrid.run(21, 31, "x", inputs[0], inputs[1], inputs[2], str(tmp_path / "out"), vcf=True, **kw)
        assert "rounds" in str(e.value) and not os.path.exists(str(tmp_path / "out"))
    names = hybrid.output_names("x", inputs[2])
    assert sorted(names) == ["align", "assembly", "ava_paf", "corrected", "corrected_paf", "exact_paf", "link", "query", "report", "scrubbed", "target",
                             "unitigs", "unitigs_cut", "unitigs_paf"]
    assert not {hybrid.POLISHED_VCF_NAME, hybrid.POLISHED_MATES_VCF_NAME} & set(names.values())
    assert (hybrid.POLISHED_VCF_NAME, hybrid.POLISHED_MATES_VCF_NAME) == ("04.assembly.polished.vcf", "05.assembly.polished.mates.vcf")
