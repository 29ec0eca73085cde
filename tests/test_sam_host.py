"""The SAM stage without a GPU: the restatement (tests/sam_oracle.py) against expected lines written by hand, and an
independent validator -- a reader of SAM text that shares no code with the restatement -- on every case of tests/samcases.py
whose input is upper-case A, C, G, T.  Beside them: the cases' violations of S1 as the restatement reports them, the rules
of the header word for word in the module's text, and the mapper's command line."""
import os
import re
import sys

import pytest

import sam_oracle
import samcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HEADER = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n@SQ\tSN:%s\tLN:%d\n@PG\tID:muchsalsa_amd\tPN:muchsalsa_amd\n"


def lines_of(text):
    return [ln for ln in text.decode("latin-1").split("\n") if ln and not ln.startswith("@")]


# ---- 1. by hand

def test_the_instance_of_the_rules_in_both_cigar_forms():
    c = samcases.case("instance")
    text, lines = sam_oracle.run(*samcases.tables(c), md=True)
    want = "q\t0\tt\t6\t60\t2S3=1X1D2=1I2=1S\t*\t0\t0\tTTCGTGGTAACG\t*\tNM:i:3\tAS:i:40\tcm:i:3\ts2:i:0\ttp:A:P\tMD:Z:3A0^C4\n"
    assert text.decode() == HEADER % ("t", 20) + want
    assert lines == [(0, 0, 0, len(HEADER % ("t", 20)))]
    text, _ = sam_oracle.run(*samcases.tables(c), eqx=False)
    assert lines_of(text) == ["q\t0\tt\t6\t60\t2S4M1D2M1I2M1S\t*\t0\t0\tTTCGTGGTAACG\t*\tNM:i:3\tAS:i:40\tcm:i:3\ts2:i:0\ttp:A:P"]


def test_its_reverse_strand_twin():
    """the stored read is the reverse complement, q 1..10 in its coordinates: the same line but for 0x10; the clips swap sides"""
    c = samcases.case("instance-reverse")
    assert c["queries"][0][1] == b"CGTTACCACGAA" and c["chains"][0][6:8] == (1, 10)
    text, _ = sam_oracle.run(*samcases.tables(c), md=True)
    assert lines_of(text) == ["q\t16\tt\t6\t60\t2S3=1X1D2=1I2=1S\t*\t0\t0\tTTCGTGGTAACG\t*\tNM:i:3\tAS:i:40\tcm:i:3\ts2:i:0\ttp:A:P\tMD:Z:3A0^C4"]


REF = b"ACGTTGCAAGGCTTAACCGGATCGATTACGCATGCAAGTCCGGTTAACGATCGGCTAAGC"


def hand_pairs():
    """three pairs on one target of 60 bases: proper (mate 2 reverse with a mismatch), one mate unmapped, both unmapped"""
    targets = [(b"ref", REF)]
    queries = [(b"a/1", b"GTTGCAAGGC"), (b"a/2", b"TCGTTTACCG"), (b"b/1", b"GTTGCAAGGC"), (b"b/2", b"acgtn"), (b"c/1", b"GGA"), (b"c/2", b"")]
    chains = [(0, 0, 0, 3, 50, 0, 0, 10, 2, 12, 10, 10), (1, 0, 1, 4, 44, 1, 0, 10, 40, 50, 9, 10), (2, 0, 0, 3, 50, 0, 0, 10, 2, 12, 10, 10)]
    ops = [10 << 4 | 7, 4 << 4 | 7, 1 << 4 | 8, 5 << 4 | 7, 10 << 4 | 7]
    off = [0, 1, 4, 5]
    ranks = [(0, 0, 0, 60), (1, 7, 0, 37), (2, 0, 0, 60)]
    mates = [(1, 48, 1, 1), (0, 48, 1, 1), (0xffffffff, 0, 0, 0)]
    return targets, queries, chains, ops, off, ranks, mates


def test_a_proper_pair_a_pair_with_one_mate_unmapped_and_an_unmapped_pair():
    text, lines = sam_oracle.run(*hand_pairs(), md=True)
    want = [
        "a\t99\tref\t3\t60\t10=\t=\t41\t48\tGTTGCAAGGC\t*\tNM:i:0\tAS:i:50\tcm:i:3\ts2:i:0\ttp:A:P\tnb:i:1\tMD:Z:10",
        "a\t147\tref\t41\t37\t4=1X5=\t=\t3\t-48\tCGGTAAACGA\t*\tNM:i:1\tAS:i:44\tcm:i:4\ts2:i:7\ttp:A:P\tnb:i:1\tMD:Z:4T5",
        "b\t73\tref\t3\t60\t10=\t=\t3\t0\tGTTGCAAGGC\t*\tNM:i:0\tAS:i:50\tcm:i:3\ts2:i:0\ttp:A:P\tMD:Z:10",
        "b\t133\tref\t3\t0\t*\t=\t3\t0\tACGTN\t*",
        "c\t77\t*\t0\t0\t*\t*\t0\t0\tGGA\t*",
        "c\t141\t*\t0\t0\t*\t*\t0\t0\t*\t*",
    ]
    assert text.decode() == HEADER % ("ref", 60) + "".join(ln + "\n" for ln in want)
    assert [ln[:3] for ln in lines] == [(0, 0, 99), (1, 1, 147), (2, 2, 73), (None, 3, 133), (None, 4, 77), (None, 5, 141)]
    # single-end, without the unmapped lines: the names keep their suffixes, no mate columns
    text, lines = sam_oracle.run(*hand_pairs()[:6], None, unmapped=False)
    assert lines_of(text) == ["a/1\t0\tref\t3\t60\t10=\t*\t0\t0\tGTTGCAAGGC\t*\tNM:i:0\tAS:i:50\tcm:i:3\ts2:i:0\ttp:A:P",
                              "a/2\t16\tref\t41\t37\t4=1X5=\t*\t0\t0\tCGGTAAACGA\t*\tNM:i:1\tAS:i:44\tcm:i:4\ts2:i:7\ttp:A:P",
                              "b/1\t0\tref\t3\t60\t10=\t*\t0\t0\tGTTGCAAGGC\t*\tNM:i:0\tAS:i:50\tcm:i:3\ts2:i:0\ttp:A:P"]


def test_roles_clips_and_md_by_hand():
    """a secondary (H clips, SEQ *, no s2), a supplementary (H clips, the aligned part) and MD's separators"""
    targets = [(b"t", REF)]
    queries = [(b"r", b"TTGCAAGGCTTAAGGCATGC")]  # REF[3:15], then GG, then REF[29:35]
    chains = [(0, 0, 0, 3, 60, 0, 0, 12, 3, 15, 12, 12), (0, 0, 0, 3, 30, 0, 14, 20, 29, 35, 6, 6), (0, 0, 0, 3, 20, 2, 14, 20, 33, 41, 4, 8)]
    ops = [12 << 4 | 7, 6 << 4 | 7, 2 << 4 | 7, 1 << 4 | 8, 2 << 4 | 2, 1 << 4 | 8, 2 << 4 | 7]
    off = [0, 1, 2, 7]
    ranks = [(0, 0, 0, 60), (1, 20, 1, 20), (1, 0, 0, 0)]
    text, _ = sam_oracle.run(targets, queries, chains, ops, off, ranks, md=True)
    assert lines_of(text) == [
        "r\t0\tt\t4\t60\t12=8S\t*\t0\t0\tTTGCAAGGCTTAAGGCATGC\t*\tNM:i:0\tAS:i:60\tcm:i:3\ts2:i:0\ttp:A:P\tMD:Z:12",
        "r\t2048\tt\t30\t20\t14H6=\t*\t0\t0\tGCATGC\t*\tNM:i:0\tAS:i:30\tcm:i:3\ts2:i:20\ttp:A:P\tMD:Z:6",
        "r\t256\tt\t34\t0\t14H2=1X2D1X2=\t*\t0\t0\t*\t*\tNM:i:2\tAS:i:20\tcm:i:3\ttp:A:S\tMD:Z:2A0^AG0T2",
    ]
    assert sam_oracle.md_string([3 << 4 | 7, 2 << 4 | 1, 4 << 4 | 7], b"ACGTACG") == "7"  # an insertion does not split a count
    assert sam_oracle.md_string([1 << 4 | 8, 5 << 4 | 7, 2 << 4 | 8], b"ACGTACGT") == "0A5G0T0"


# ---- 2. the independent validator

CIGAR_RE = re.compile(r"(\d+)([MIDNSHP=X])")
MD_RE = re.compile(r"(\d+)|\^([A-Z]+)|([A-Z])")


def parse_sam(text):
    """-> (target lengths by name, alignment records as dicts); every line has at least 11 columns"""
    sq, recs = {}, []
    for ln in text.decode("latin-1").split("\n"):
        if not ln:
            continue
        if ln.startswith("@"):
            if ln.startswith("@SQ"):
                f = dict(x.split(":", 1) for x in ln.split("\t")[1:])
                sq[f["SN"]] = int(f["LN"])
            continue
        col = ln.split("\t")
        assert len(col) >= 11, ln
        tags = {}
        for t in col[11:]:
            name, kind, value = t.split(":", 2)
            assert name not in tags
            tags[name] = int(value) if kind == "i" else value
        recs.append(dict(qname=col[0], flag=int(col[1]), rname=col[2], pos=int(col[3]), mapq=int(col[4]),
                         cigar=[(int(n), op) for n, op in CIGAR_RE.findall(col[5])] if col[5] != "*" else None, cigar_text=col[5],
                         rnext=col[6], pnext=int(col[7]), tlen=int(col[8]), seq=col[9], qual=col[10], tags=tags))
        if col[5] != "*":
            assert "".join("%d%s" % x for x in recs[-1]["cigar"]) == col[5]
    return sq, recs


def reference_from(rec):
    """the reference bases under the alignment, rebuilt from SEQ, CIGAR and MD alone"""
    seq, at, ref = rec["seq"], 0, []  # ref: per reference column the base, None where MD has to say
    for n, op in rec["cigar"]:
        if op == "S":
            at += n
        elif op in "M=X":
            ref.extend(seq[at:at + n])
            at += n
        elif op == "I":
            at += n
        elif op == "D":
            ref.extend([None] * n)
    assert at == len(seq)
    x = 0
    for count, deleted, mismatch in MD_RE.findall(rec["tags"]["MD"]):
        if count:
            for _ in range(int(count)):
                assert ref[x] is not None
                x += 1
        elif deleted:
            for b in deleted:
                assert ref[x] is None
                ref[x] = b
                x += 1
        else:
            assert ref[x] is not None and ref[x] != mismatch, "MD names a mismatch where SEQ agrees with it"
            ref[x] = mismatch
            x += 1
    assert x == len(ref)
    return "".join(ref)


def validate(c, text_eqx, text_m):
    """what a downstream reader relies on, checked on the text alone (and against the case's targets and mate rows)"""
    paired = c["mates"] is not None
    sq, recs = parse_sam(text_eqx)
    _, recs_m = parse_sam(text_m)
    tseq = {(n if isinstance(n, str) else n.decode()): s for n, s in c["targets"]}
    assert sq == {n: len(s) for n, s in tseq.items()}
    consumes_q, consumes_t = "MIS=X", "MDN=X"
    for k, r in enumerate(recs):
        if r["cigar"] is not None and r["seq"] != "*":
            assert sum(n for n, op in r["cigar"] if op in consumes_q) == len(r["seq"]), r
        assert r["qual"] == "*"
        assert bool(r["flag"] & 1) == paired and (not paired or bool(r["flag"] & 0x40) != bool(r["flag"] & 0x80))
        if r["flag"] & 4:
            assert r["cigar"] is None and not r["tags"] and r["mapq"] == 0 and not r["flag"] & 0x902
            continue
        assert r["rname"] in tseq and 1 <= r["pos"] and r["cigar"] is not None
        t_start = r["pos"] - 1
        t_end = t_start + sum(n for n, op in r["cigar"] if op in consumes_t)
        assert t_end <= len(tseq[r["rname"]])
        assert r["tags"]["tp"] == ("S" if r["flag"] & 0x100 else "P") and ("s2" in r["tags"]) == (not r["flag"] & 0x100)
        assert all(op in "SH=XID" for _, op in r["cigar"])
        assert all(op == ("H" if r["flag"] & 0x900 else "S") for _, op in r["cigar"] if op in "SH")
        if r["seq"] != "*":
            assert reference_from(r) == tseq[r["rname"]][t_start:t_end].decode(), r
            assert r["tags"]["NM"] == sum(n for n, op in r["cigar"] if op in "XID")
        # the M form says the same: the same line but for CIGAR, whose = and X runs are merged into M
        m = recs_m[k]
        merged = []
        for n, op in r["cigar"]:
            op = "M" if op in "=X" else op
            if merged and merged[-1][1] == "M" and op == "M":
                merged[-1] = (merged[-1][0] + n, "M")
            else:
                merged.append((n, op))
        assert m["cigar"] == merged and {k2: v for k2, v in m.items() if not k2.startswith("cigar")} == \
            {k2: v for k2, v in r.items() if not k2.startswith("cigar")}
    # a read's lines are neighbours (S3).  Exactly one line per mapped read is neither secondary nor supplementary; an
    # unmapped read has its one line
    by_read = []
    for r in recs:
        if by_read and (by_read[-1][0]["qname"], by_read[-1][0]["flag"] & 0xc0) == (r["qname"], r["flag"] & 0xc0) and not r["flag"] & 4 \
                and not by_read[-1][0]["flag"] & 4:
            by_read[-1].append(r)
        else:
            by_read.append([r])
    assert len(by_read) == len(c["queries"])
    for rs in by_read:
        assert sum(1 for r in rs if not r["flag"] & 0x900) == 1, rs[0]["qname"]
    if not paired:
        assert all(r["rnext"] == "*" and r["pnext"] == 0 and r["tlen"] == 0 for r in recs)
        return len(recs)
    # the two mate lines of a pair: the proper lines where there are any, else the two primary lines
    proper_tl = sorted(row[1] for row in c["mates"] if row[2] == 1)
    seen_tl = []
    for p in range(0, len(by_read), 2):
        one, two = by_read[p], by_read[p + 1]
        name = one[0]["qname"]
        assert one[0]["flag"] & 0x40 and two[0]["flag"] & 0x80, name
        a = [r for r in one if r["flag"] & 2] or [r for r in one if not r["flag"] & 0x900]
        b = [r for r in two if r["flag"] & 2] or [r for r in two if not r["flag"] & 0x900]
        assert len(a) == 1 and len(b) == 1 and bool(a[0]["flag"] & 2) == bool(b[0]["flag"] & 2), name
        a, b = a[0], b[0]
        for x, y in ((a, b), (b, a)):
            assert bool(x["flag"] & 8) == bool(y["flag"] & 4), name
            if y["flag"] & 4:
                if not x["flag"] & 4:  # the unmapped mate sits at the mapped one's place
                    assert (y["rname"], y["pos"]) == (x["rname"], x["pos"]) and x["rnext"] == "=" and x["pnext"] == x["pos"]
                continue
            assert bool(x["flag"] & 0x20) == bool(y["flag"] & 0x10), name
            assert x["pnext"] == y["pos"] and (x["rname"] if x["rnext"] == "=" else x["rnext"]) == y["rname"], name
            assert (x["rnext"] == "=") == (x["rname"] == y["rname"]), name
        assert a["tlen"] + b["tlen"] == 0, name
        if a["flag"] & 2:
            seen_tl.extend([abs(a["tlen"]), abs(b["tlen"])])
            assert a["tags"]["nb"] == b["tags"]["nb"] >= 1
        if not a["flag"] & 4 and not b["flag"] & 4 and a["rname"] != b["rname"]:
            assert a["tlen"] == 0
    assert sorted(seen_tl) == proper_tl  # a proper pair has |TLEN| = rule 13's tl
    return len(recs)


@pytest.mark.parametrize("name", [c["name"] for c in samcases.CASES if c["acgt"]])
def test_the_validator_accepts_every_case_on_acgt_input(name):
    c = samcases.case(name)
    text_eqx, lines = sam_oracle.run(*samcases.tables(c), md=True)
    text_m, _ = sam_oracle.run(*samcases.tables(c), md=True, eqx=False)
    assert validate(c, text_eqx, text_m) == len(lines)


def test_the_validator_validates():
    """it refuses a wrong base in MD, a wrong mate position and a TLEN with the wrong sign"""
    text, _ = sam_oracle.run(*hand_pairs(), md=True)
    c = dict(targets=hand_pairs()[0], queries=hand_pairs()[1], mates=hand_pairs()[6])
    validate(c, text, sam_oracle.run(*hand_pairs(), md=True, eqx=False)[0])
    for old, new in ((b"MD:Z:4T5", b"MD:Z:4A5"), (b"\t=\t41\t48", b"\t=\t42\t48"), (b"\t-48\t", b"\t48\t"), (b"\t10=\t=\t41", b"\t9=\t=\t41")):
        assert old in text
        with pytest.raises(AssertionError):
            validate(c, text.replace(old, new), sam_oracle.run(*hand_pairs(), md=True, eqx=False)[0].replace(old, new))


# ---- 3. S1, the line bounds, the texts

@pytest.mark.parametrize("name", [b[0] for b in samcases.BAD])
def test_the_restatement_reports_every_violation_of_s1(name):
    _, c, want = next(b for b in samcases.BAD if b[0] == name)
    with pytest.raises(sam_oracle.SamTableError) as e:
        sam_oracle.run(*samcases.tables(c))
    assert str(e.value).startswith(want)


def test_an_empty_name_is_refused():
    t, q, *rest = samcases.tables(samcases.case("instance"))
    with pytest.raises(sam_oracle.SamTableError, match="query record 0: an empty name"):
        sam_oracle.run(t, [(b"", q[0][1])], *rest)


def test_every_line_stays_below_its_text_bound():
    """S11's bound, on every case and form, the widest numbers included"""
    for c in samcases.CASES:
        targets, queries, chains, ops, off, ranks, mates = samcases.tables(c)
        for md in (False, True):
            text, lines = sam_oracle.run(targets, queries, chains, ops, off, ranks, mates, md=md)
            ends = [ln[3] for ln in lines[1:]] + [len(text)]
            for (chain, q, _, at), end in zip(lines, ends):
                ch = None if chain is None else chains[chain]
                assert end - at <= sam_oracle.line_bound(ch, 0 if chain is None else off[chain + 1] - off[chain], len(queries[q][1]), md)
    # the fixed part covers three names of 254 bytes and every number at its widest
    widest = 3 * 254 + len("\t2303\t\t2147483647\t4294967295\t\t\t2147483647\t-2147483647\t\t*\tNM:i:4294967295\tAS:i:-2147483648\tcm:i:4294967295"
                            "\ts2:i:-2147483648\ttp:A:P\tnb:i:4294967295\tMD:Z:\n")
    assert widest <= sam_oracle.LINE_FIXED


def test_the_rules_stand_word_for_word_in_the_module():
    with open(os.path.join(ROOT, "include", "msgpu.h")) as h:
        header = h.read()
    block = header[header.index(" *  S1. inputs and checks."):header.index("Out of scope: base qualities")]
    rules = " ".join(re.sub(r"^ \* ?", "", ln) for ln in block.split("\n")).split()
    with open(os.path.join(ROOT, "muchsalsa_amd", "sam.py")) as h:
        module = h.read().split()
    at = module.index("S1.")
    assert module[at:at + len(rules)] == rules
    with open(os.path.join(ROOT, "DESIGN.md")) as h:
        design = " ".join(h.read().split())
    for n in range(1, 12):
        assert ("S%d." % n) in design


def test_the_command_line_reaches_run(monkeypatch, capsys):
    from muchsalsa_amd import mapper as mp
    seen = {}

    def fake(*args, **kw):
        seen.update(kw, args=args)
        return {}
    monkeypatch.setattr(mp, "run", fake)
    assert mp.main(["t.fa", "q.fa", "o.paf", "--sam", "o.sam", "--md", "--cigar-m", "--mates"]) == 0
    assert seen["sam"] == "o.sam" and seen["sam_md"] is True and seen["sam_m"] is True and seen["mates"] is True
    seen.clear()
    assert mp.main(["t.fa", "q.fa", "o.paf", "--cigar"]) == 0
    assert "sam" not in seen and "sam_md" not in seen and "sam_m" not in seen  # (without the option the call is the one it always was)
    for bad in (["--md"], ["--cigar-m"], ["--sam"], ["--sam", "--md"]):
        assert mp.main(["t.fa", "q.fa", "o.paf"] + bad) == 2
    assert "[--sam F] [--md] [--cigar-m]" in mp.__doc__.split("\n\n")[1]
    capsys.readouterr()
