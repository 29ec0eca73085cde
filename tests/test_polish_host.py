"""The polishing stage without a GPU: the restatement (tests/pl_oracle.py) on paper cases for every rule and tie, the C-ABI, the
command line, the driver's file names, and the restatement's improvement on the planted workload."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import pl_oracle
import plcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I, D, EQ, X = pl_oracle.OP_I, pl_oracle.OP_D, pl_oracle.OP_EQ, pl_oracle.OP_X


@pytest.fixture(scope="module")
def pl():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import polish
    return polish


def bases(result):
    """the records' bases, unwrapped"""
    out = []
    for line in result["text"].split(b"\n")[:-1]:
        if line.startswith(b">"):
            out.append([])
        else:
            out[-1].append(line)
    return [b"".join(x) for x in out]


def polished(name):
    c = plcases.hand_cases()[name]
    return c, plcases.expected_hand(name), bases(plcases.expected_hand(name))


AT = 50  # where the hand cases edit their 130-base draft


def test_identity_is_the_identity_on_bytes():
    for name in ("identity", "identity_reads_differ_in_case"):
        c, r, b = polished(name)
        d = c["draft"][0][1]
        assert b == [d] and any(x in d for x in b"acgt") and b"N" in d
        assert r["text"] == b">d0\n" + d[:60] + b"\n" + d[60:120] + b"\n" + d[120:] + b"\n"
        assert r["pos_verbatim"] == 1 and r["pos_unchanged"] == 129 and r["records"] == [(130, 130, 0, 0, 0, 300)]
        assert r["cols_eq"] + r["cols_x"] == 390 and r["max_depth"] == 3


def test_rule_5_calls_and_ties():
    c, r, b = polished("sub_2of3")
    d = c["draft"][0][1]
    assert b == [d[:AT] + bytes([plcases.other(d[AT])]) + d[AT + 1:]] and r["pos_substituted"] == 1 and r["cols_x"] == 2
    for name in ("tie_draft", "del_ties_draft"):  # the draft's base is among the tied
        c, r, b = polished(name)
        assert b == [c["draft"][0][1]] and r["pos_substituted"] == r["pos_deleted"] == 0 and r["pos_unchanged"] == 130
    c, r, b = polished("tie_others")  # G in the draft, one T and one C: C comes first
    d = c["draft"][0][1]
    assert d[AT:AT + 1] == b"G" and b == [d[:AT] + b"C" + d[AT + 1:]]
    c, r, b = polished("del_wins")
    d = c["draft"][0][1]
    assert b == [d[:AT] + d[AT + 1:]] and r["pos_deleted"] == 1 and r["cols_d"] == 2 and r["records"] == [(130, 129, 0, 1, 0, 300)]
    c, r, b = polished("del_ties_other")  # a base before del
    d = c["draft"][0][1]
    assert b == [d[:AT] + bytes([plcases.other(d[AT])]) + d[AT + 1:]]
    c, r, b = polished("depth_edge")  # depth 2 at position 20, depth 3 at position 61
    d = c["draft"][0][1]
    assert b == [d[:61] + bytes([plcases.other(d[61])]) + d[62:]] and r["pos_verbatim"] == 40 and r["cols_x"] == 5


def test_rule_5_in_isolation():
    call = pl_oracle.call
    assert call([0, 0, 0, 0, 0, 5], ord("a"), 3) == ("verbatim", b"a")      # only "other" votes
    assert call([2, 0, 0, 0, 0, 0], ord("C"), 3) == ("verbatim", b"C")      # below min_depth
    assert call([2, 0, 0, 0, 0, 1], ord("C"), 3) == ("substituted", b"A")   # "other" counts for the depth alone
    assert call([0, 2, 0, 0, 2, 0], ord("c"), 1) == ("unchanged", b"c")     # the draft's folded base among the tied; case is kept
    assert call([0, 2, 0, 0, 2, 0], ord("N"), 1) == ("substituted", b"C")   # a draft byte that is no base is never among the tied
    assert call([0, 0, 0, 2, 2, 0], ord("A"), 1) == ("substituted", b"T")
    assert call([0, 0, 0, 1, 2, 0], ord("A"), 1) == ("deleted", b"")
    assert call([3, 3, 3, 3, 3, 0], ord("G"), 1) == ("unchanged", b"G")
    assert call([3, 3, 3, 3, 3, 0], ord("n"), 1) == ("substituted", b"A")


def test_rules_4_and_6_insertions():
    c, r, b = polished("ins_2of3")
    d = c["draft"][0][1]
    assert b == [d[:AT] + b"AC" + d[AT:]] and (r["ins_usable"], r["ins_applied"], r["bases_inserted"]) == (2, 1, 2)
    assert r["records"] == [(130, 132, 0, 0, 1, 300)] and r["cols_i"] == 4
    assert polished("ins_1of2")[2] == [d] and polished("ins_equal_counts")[2] == [d]
    assert polished("ins_3_against_1")[2] == [d[:AT] + b"AC" + d[AT:]]
    assert polished("ins_tie_shorter")[2] == [d[:AT] + b"T" + d[AT:]]       # AC and T, two each: the shorter
    assert polished("ins_tie_letters")[2] == [d[:AT] + b"AT" + d[AT:]]     # CA and AT, two each: the smaller letters
    c, r, b = polished("ins_32_and_33")
    assert len(b[0]) == 162 and b[0][:40] == d[:40] and b[0][72:] == d[40:] and (r["ins_usable"], r["ins_unusable"]) == (2, 2)
    c, r, b = polished("ins_with_n")
    assert b == [d] and (r["ins_usable"], r["ins_unusable"], r["cols_i"]) == (0, 2, 6)
    assert polished("ins_lower_case")[2] == [d[:AT] + b"AC" + d[AT:]]
    c, r, b = polished("ins_at_ends")
    assert b == [d] and (r["ins_at_ends"], r["ins_usable"], r["ins_unusable"]) == (6, 0, 0)
    c, r, b = polished("ins_at_record_edges")  # usable, and at no slot 0 < p < tlen
    assert b == [d] and (r["ins_at_ends"], r["ins_usable"], r["ins_applied"]) == (6, 6, 0)
    ins = pl_oracle.insertion
    assert ins({(2, 0b0110): 2, (1, 3): 1}, 3, 4, 3) == b"CG" and ins({(2, 0b0110): 2}, 4, 3, 3) == b"CG"
    assert ins({(2, 0b0110): 2}, 4, 4, 3) == b"" and ins({(2, 0b0110): 2}, 2, 9, 3) == b""


def test_rule_2_voters():
    c, r, b = polished("two_chains_equal")  # both chains of read 0 carry the substitution: 2 of 4 with one vote, 3 of 5 with two
    assert b == [c["draft"][0][1]] and (r["n_voters"], r["n_ignored"]) == (4, 1) and r["voters"] == [0, 2, 3, 4]
    assert plcases.expected_hand("two_chains_unequal")["voters"] == [1, 2, 3]
    assert plcases.expected_hand("two_chains_block")["voters"] == [1, 2, 3]
    c, r, b = polished("min_identity")
    assert b == [c["draft"][0][1]] and r["voters"] == [1, 2] and r["n_ignored"] == 1
    assert bases(pl_oracle.run(c["draft"], c["reads"], c["chains"], c["runs"], min_depth=2)) != b  # without the cut: 2 of 3
    v = pl_oracle.voters
    ch = lambda q, score, m, b: (q, 0, 0, 3, score, 0, 0, 0, 0, 0, m, b)
    assert v([ch(0, -5, 9, 10), ch(0, -7, 9, 10), ch(1, 1, 89, 100), ch(1, 0, 90, 100)], 90) == [0, 3]
    assert v([ch(0, 5, 0, 0)], 100) == [0] and v([ch(0, 5, 99, 100)], 100) == []


def test_rule_3_strand_and_offsets():
    c, r, b = polished("strand_1")
    d = c["draft"][0][1]
    o = plcases.other
    want = d[:35] + bytes([o(d[35]), o(d[36])]) + d[37:47] + b"ACG" + d[47:67] + d[69:]
    assert b == [want] and [ch[2] for ch in c["chains"]] == [1, 1, 0] and c["chains"][0][6:8] == (7, 112)
    assert r["records"] == [(130, 131, 2, 2, 1, 260)]
    assert pl_oracle.oriented(b"AcgTN", 1) == b"NAGCT" and pl_oracle.oriented(b"acgt", 0) == b"ACGT"  # lower case is not complemented
    c, r, b = polished("flanks")
    assert b == [d[:35] + bytes([o(d[35]), o(d[36])]) + d[37:]] and c["chains"][0][6:8] == (5, 107)


def test_long_run_many_runs_and_records():
    c, r, b = polished("long_run")
    d = c["draft"][0][1]
    assert len(c["runs"][0]) == 1 and c["runs"][0][0] == 5000 << 4 | EQ and len(d) == 6000 and r["pos_substituted"] == 7
    assert [i for i in range(6000) if b[0][i] != d[i]] == [500 + p for p in (0, 63, 64, 255, 256, 2500, 4999)]
    c, r, b = polished("many_runs")
    assert len(c["runs"][0]) == 200 and {x & 15 for x in c["runs"][0]} == {I, D, EQ, X} and r["ins_applied"] == 33
    c, r, b = polished("two_records")
    assert r["text"].startswith(b">first\n") and b">second\n" in r["text"] and b[0] == c["draft"][0][1] and b[1] != c["draft"][1][1]
    assert r["records"][0] == (130, 130, 0, 0, 0, 0)
    c, r, b = polished("all_deleted")
    assert r["text"].endswith(b">gone\n\n") and b == [c["draft"][0][1], b""] and r["records"][1] == (70, 0, 0, 70, 0, 300)
    assert all(ch[6] == ch[7] == 4 for ch in c["chains"] if ch[1] == 1)
    c, r, b = polished("zero_chains")
    assert b == [s for _, s in c["draft"]] and r["pos_verbatim"] == 220 and r["bytes_out"] == len(r["text"])


@pytest.mark.parametrize("name", sorted(plcases.violations()))
def test_rule_1_names_the_first_violation(name):
    c, chain, what = plcases.violations()[name]
    with pytest.raises(pl_oracle.PolishError) as e:
        plcases.expected_tables(c)
    assert (e.value.chain, e.value.what) == (chain, what) and str(e.value) == "chain %d: %s" % (chain, what)


def test_every_kind_of_violation_has_a_case():
    assert {what for _, _, what in plcases.violations().values()} == set(pl_oracle.WHAT)
    with pytest.raises(ValueError):
        pl_oracle.run([], [], [], [], min_depth=0)
    with pytest.raises(ValueError):
        pl_oracle.run([], [], [], [], min_identity=101)


def levenshtein(a, b, band):
    """the Levenshtein distance of a and b by a plain DP over the cells with |i - j| <= band: never below the true distance, and
    equal to it whenever an optimal path stays inside the band"""
    big = len(a) + len(b)
    prev = [j if j <= band else big for j in range(len(b) + 1)]
    for i in range(1, len(a) + 1):
        lo, hi = max(0, i - band), min(len(b), i + band)
        cur = [big] * (len(b) + 1)
        for j in range(lo, hi + 1):
            best = prev[j] + 1
            if j:
                best = min(best, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
            cur[j] = best
        prev = cur
    return prev[len(b)]


def test_levenshtein():
    assert levenshtein(b"ACGT", b"ACGT", 2) == 0 and levenshtein(b"ACGT", b"AGT", 2) == 1 and levenshtein(b"AAAA", b"TTTT", 2) == 4
    assert levenshtein(b"ACGTACGT", b"CGTACGTA", 3) == 2 and levenshtein(b"", b"AC", 2) == 2


def test_the_restatement_improves_the_planted_draft():
    """the planted workload: a 20 kb genome, a draft with an edit of 1-3 bases about every 150 bases, 40 error-free reads of 3 kb.
    The restatement's output is strictly closer to the genome than the draft is (DESIGN.md section 14 records both)."""
    wl = plcases.workload("planted")
    r, mapped = plcases.expected_workload("planted")
    draft = bases(dict(text=wl["draft"]))[0]
    out = bases(r)[0]
    before, after = levenshtein(wl["genome"], draft, 48), levenshtein(wl["genome"], out, 48)
    print("planted: distance to the genome %d before, %d after; %d chains, %d voters, counts %r" % (
        before, after, len(mapped["chains"]), r["n_voters"], {k: r[k] for k in pl_oracle.COUNTS}))
    assert len(draft) != len(wl["genome"]) or draft != wl["genome"]
    assert after < before
    assert r["n_voters"] >= 30 and r["pos_substituted"] >= 20 and r["pos_deleted"] >= 20 and r["ins_applied"] >= 20


def test_abi(pl):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_pl_create", "msgpu_pl_destroy", "msgpu_pl_last_error", "msgpu_pl_default_params", "msgpu_pl_run",
              "msgpu_pl_result_text", "msgpu_pl_result_stats", "msgpu_pl_result_records", "msgpu_pl_result_free"):
        assert hasattr(L, n) and n in bound and n + "(" in header, n
    assert C.sizeof(_lib.PlParams) == 8 and C.sizeof(_lib.PlStats) == 256 and C.sizeof(_lib.PlRecord) == 48
    assert _lib.PlStats.params.offset == 200 and _lib.PlStats.load_ms.offset == 208
    prm = _lib.PlParams()
    L.msgpu_pl_default_params(C.byref(prm))
    assert (prm.min_depth, prm.min_identity) == (3, 0) == tuple(pl.DEFAULTS[k] for k in ("min_depth", "min_identity"))
    assert pl.DEFAULTS == pl_oracle.PARAMS and pl.CHAIN_DTYPE.itemsize == C.sizeof(_lib.MapChain)
    assert tuple(pl._strip(n) for n in pl.COUNTS if n in pl_oracle.COUNTS) == tuple(pl._strip(n) for n in pl_oracle.COUNTS)
    n = C.c_uint64()
    assert L.msgpu_pl_result_stats(None, None) == _lib.E_ARG and L.msgpu_pl_result_records(None, None, C.byref(n)) == _lib.E_ARG
    assert L.msgpu_pl_run(None, None, None, None, None, 0, None, None, 0, None) == _lib.E_ARG
    for rule in range(1, 9):  # the rules stand in the header and in the module's docstring, numbered alike
        assert "\n *  %d. " % rule in header.split("pileup consensus")[1] and "\n %d. " % rule in pl.__doc__


def test_command_line(pl, tmp_path, monkeypatch, capsys):
    seen = []
    monkeypatch.setattr(pl, "run", lambda *a, **kw: seen.append((a, kw)) or {})
    p = [str(tmp_path / n) for n in ("draft.fa", "reads.fq", "out.fa")]
    assert pl.main(p) == 0 and seen[-1][0] == tuple(p) and seen[-1][1]["rounds"] == 1 and seen[-1][1]["paf"] is None
    assert pl.main(p + ["--rounds", "2", "--min-depth", "4", "--min-identity", "80", "--paf", "x.paf", "-k", "19", "--band", "32",
                        "--budget-mb", "64"]) == 0
    kw = seen[-1][1]
    assert (kw["rounds"], kw["min_depth"], kw["min_identity"], kw["paf"], kw["k"], kw["band"], kw["budget_mb"]) == (2, 4, 80, "x.paf", 19, 32, 64.0)
    capsys.readouterr()
    for bad in (p[:2], p + ["--rounds", "0"], p + ["--min-depth", "0"], p + ["--min-identity", "101"], p + ["--rounds"], p + ["--exact"],
                p + ["-k", "3"], p + ["--paf"]):
        assert pl.main(bad) == 2, bad
        assert "python -m muchsalsa_amd.polish" in capsys.readouterr().err
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.polish", p[0], p[1]], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert out.returncode == 2 and b"[--rounds N]" in out.stderr and out.stdout == b""


def test_unknown_keywords_are_rejected(pl, tmp_path):
    p = [str(tmp_path / n) for n in ("draft.fa", "reads.fa", "out.fa")]
    with pytest.raises(TypeError):
        pl.run_tables(p[0], p[1], p[2], [], [], min_dept=2)
    with pytest.raises(TypeError):
        pl.run(p[0], p[1], p[2], exact=1)
    with pytest.raises(TypeError):
        pl.run(p[0], p[1], p[2], rounds=0)
    assert not os.path.exists(p[2])


def test_the_drivers_file_names_are_unchanged(pl):
    from muchsalsa_amd import hybrid
    names = hybrid.output_names("asm", "/data/nano.fastq")
    assert sorted(names) == ["align", "assembly", "ava_paf", "corrected", "corrected_paf", "exact_paf", "link", "query", "report",
                             "scrubbed", "target", "unitigs", "unitigs_cut", "unitigs_paf"]
    assert names["assembly"] == "03.assembly.unpolished.fa" and names["scrubbed"] == "02_nano.scrubbed.fa"
    assert hybrid.POLISHED_NAME == "04.assembly.polished.fa" and hybrid.POLISHED_NAME not in names.values()
    assert hybrid.main(["21", "31", "asm"]) == 2  # the nine-argument command line: no tenth argument, no new option
    assert hybrid.main([str(x) for x in range(10)]) == 2


def test_no_device_means_an_error_not_a_fallback(pl, tmp_path):
    import torch
    from muchsalsa_amd import _lib
    c = plcases.hand_cases()["sub_2of3"]
    dp, rp = plcases.write_case(c, tmp_path)
    out = os.path.join(str(tmp_path), "out.fa")
    if torch.cuda.is_available():
        pl.run_tables(dp, rp, out, c["chains"], c["runs"])
        assert open(out, "rb").read() == plcases.expected_hand("sub_2of3")["text"]
        return
    with pytest.raises(pl.PolishError) as e:
        pl.run_tables(dp, rp, out, c["chains"], c["runs"])
    assert e.value.code == _lib.E_NODEVICE and not os.path.exists(out)
    h = C.c_void_p()
    assert _lib.lib().msgpu_pl_create(0, C.byref(h)) == _lib.E_NODEVICE and not h.value
