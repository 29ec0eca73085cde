"""Rule 13 (the mapper's mates), host side (no GPU): paper cases of the restatement (tests/map_mate_oracle.py) worked by hand for
every clause of 13.1 and every tie of 13.2, its invariants on every table the GPU file compares, what the tables were made to hold,
the C-ABI with its pinned sizes, the byte bound, the rule's text in its two places, the command lines and ``interleave``."""
import ctypes as C
import os

import pytest

import map_mate_oracle as mo
import matecases
from matecases import ch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = mo.EMPTY


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


def rows(chains, max_insert=1000):
    return mo.mates(chains, max_insert)[0]


# ---- the restatement

def test_paper_cases_of_concordance():
    f, r = ch(0, 100, 0, 100), ch(1, 90, 200, 300, 1)
    assert rows([f, r]) == [(1, 300, 1, 1), (0, 300, 1, 1)]  # tl = r.t_end - f.t_start
    assert rows([ch(0, 100, 200, 300, 1), ch(1, 90, 0, 100, 0)]) == [(1, 300, 1, 1), (0, 300, 1, 1)]  # either mate may be the forward one
    assert rows([f, ch(1, 90, 200, 300, 1, target=1)]) == [U, U]  # another target
    assert rows([f, ch(1, 90, 200, 300, 0)]) == [U, U] == rows([ch(0, 100, 0, 100, 1), r])  # equal strands
    assert rows([f, ch(1, 90, 900, 1000, 1)]) == [(1, 1000, 1, 1), (0, 1000, 1, 1)]  # tl == max_insert
    assert rows([f, ch(1, 90, 901, 1001, 1)]) == [U, U] and rows([f, ch(1, 90, 901, 1001, 1)], 1001)[0][2] == 1
    assert rows([ch(0, 100, 50, 150), ch(1, 90, 50, 150, 1)]) == [(1, 100, 1, 1), (0, 100, 1, 1)]  # both bounds equal
    assert rows([ch(0, 100, 51, 150), ch(1, 90, 50, 150, 1)]) == [U, U]  # the forward mate starts behind the reverse one
    assert rows([ch(0, 100, 200, 300), ch(1, 90, 0, 100, 1)]) == [U, U]  # outward-facing
    assert rows([ch(0, 100, 0, 400), ch(1, 90, 100, 300, 1)]) == [U, U]  # the forward mate passes the reverse one
    assert rows([ch(2, 100, 0, 100), ch(5, 90, 200, 300, 1)]) == [U, U]  # records 2 and 5 are of pairs 1 and 2
    assert rows([ch(3, 100, 0, 100), ch(4, 90, 200, 300, 1)]) == [U, U]  # 3 and 4 likewise: the pair is query >> 1
    assert rows([ch(4, 100, 0, 100), ch(5, 90, 200, 300, 1)], 1000)[0] == (1, 300, 1, 1)
    assert rows([ch(0, 100, 0, 100), ch(0, 90, 200, 300, 1)]) == [U, U]  # two chains of one mate are no pair
    assert rows([]) == [] and mo.mates([], 1)[1]["n_pairs"] == 0


def test_paper_cases_of_the_selection():
    # the greatest sum, whatever tl and the indices
    assert rows([ch(0, 100, 0, 100), ch(0, 101, 10, 110), ch(1, 50, 200, 300, 1), ch(1, 49, 150, 250, 1)]) == [U, (2, 290, 1, 1), (1, 290, 1, 1), U]
    # equal sums: the smaller tl; n_best counts both
    assert rows([ch(0, 100, 0, 100), ch(0, 100, 10, 110), ch(1, 50, 200, 300, 1)]) == [U, (2, 290, 1, 2), (1, 290, 1, 2)]
    # 100 + 50 == 90 + 60: a tie across different chains of both mates, decided by tl
    assert rows([ch(0, 100, 0, 100), ch(0, 90, 0, 100, 0, 1), ch(1, 50, 200, 300, 1), ch(1, 60, 200, 290, 1, 1)]) == [U, (3, 290, 1, 2), U, (1, 290, 1, 2)]
    # equal sums and tl: the smaller a, then the smaller b
    assert rows([ch(0, 100, 0, 100), ch(0, 100, 0, 100), ch(1, 50, 200, 300, 1), ch(1, 50, 200, 300, 1)]) == [(2, 300, 1, 4), U, (0, 300, 1, 4), U]
    assert rows([ch(0, 100, 5, 100), ch(0, 100, 0, 100), ch(1, 50, 200, 305, 1), ch(1, 50, 200, 300, 1)])[0] == (3, 295, 1, 4)  # (0, 3) and (1, 2) tie at 305 behind it
    # n_best counts the greatest sum only, whatever its tl; a closer combination of a smaller sum is nothing
    assert rows([ch(0, 100, 0, 100), ch(1, 50, 200, 300, 1), ch(1, 50, 200, 400, 1), ch(1, 49, 100, 110, 1)])[0] == (1, 300, 1, 2)
    # 64-bit sums
    hi, lo = 2147483647, -2147483648
    assert rows([ch(0, hi, 0, 100), ch(1, hi, 200, 300, 1), ch(1, hi - 1, 200, 250, 1)])[0] == (1, 300, 1, 1)
    assert rows([ch(0, lo, 0, 100), ch(1, lo, 200, 300, 1), ch(1, lo + 1, 200, 350, 1)])[0] == (2, 350, 1, 1)
    # the counts
    st = mo.mates([ch(0, 1, 0, 100), ch(1, 1, 200, 300, 1), ch(2, 1, 0, 100), ch(5, 1, 0, 9), ch(6, 1, 0, 100), ch(7, 1, 0, 100)], 1000, n_records=10)[1]
    assert (st["n_pairs"], st["n_proper"], st["n_single"], st["n_discordant"], st["n_unmapped"]) == (5, 1, 2, 1, 1)
    assert (st["tlen_sum"], st["tlen_min"], st["tlen_max"], st["largest_pair"], st["n_pairs_settled"]) == (300, 300, 300, 2, 4)
    # base is added to the mates alone
    assert mo.mates([ch(0, 1, 0, 100), ch(1, 1, 200, 300, 1)], 1000, base=7)[0] == [(8, 300, 1, 1), (7, 300, 1, 1)]


def test_a_bad_table_names_the_smallest_chain_and_the_first_word():
    for name, (chains, first, word) in matecases.bad_tables().items():
        with pytest.raises(mo.MateError) as e:
            mo.mates(chains)
        assert (e.value.chain, e.value.word) == (first, word) and str(e.value) == "chain %d: %s" % (first, word), name


@pytest.mark.parametrize("name", matecases.NAMES)
def test_invariants_on_every_table(name):
    chains, max_insert, _ = matecases.tables()[name]
    got, st = matecases.expected(name)
    mo.invariants(list(chains), got, max_insert)
    assert st["n_pairs"] == st["n_proper"] + st["n_discordant"] + st["n_single"] and st["n_unmapped"] == 0
    assert st["n_pairs"] == st["n_pairs_settled"] + st["n_pairs_lanes16"] + st["n_pairs_lanes64"] + st["n_pairs_list"]
    with pytest.raises(AssertionError):  # the invariants do notice a wrong row
        if not any(r[2] for r in got):
            raise AssertionError("nothing selected: nothing to spoil")
        i = next(i for i, r in enumerate(got) if r[2])
        mo.invariants(list(chains), got[:i] + [(got[i][0], got[i][1] + 1, 1, got[i][3])] + got[i + 1:], max_insert)


def test_the_tables_hold_what_they_were_made_for():
    ex = {n: matecases.expected(n) for n in matecases.NAMES}
    st = ex["classes"][1]
    assert (st["n_pairs_settled"], st["n_pairs_lanes16"], st["n_pairs_lanes64"], st["n_pairs_list"]) == (5, 5, 5, 5) and st["n_single"] == 2
    for group, key in ((matecases.SETTLED, "n_pairs_settled"), (matecases.LANES16, "n_pairs_lanes16"), (matecases.LANES64, "n_pairs_lanes64"),
                       (matecases.LIST, "n_pairs_list")):
        for n1, n2 in group:
            assert ex["alone_%d_%d" % (n1, n2)][1][key] == 1 and ex["alone_%d_%d" % (n1, n2)][1]["largest_pair"] == n1 + n2
    assert ex["alone_1_1_concordant"][1]["n_proper"] == 1 and ex["alone_1_1_discordant"][1]["n_discordant"] == 1
    for count in (1, 4, 5):
        assert ex["lanes16_x%d" % count][1]["n_pairs_lanes16"] == ex["lanes16_x%d" % count][1]["n_pairs"] == count
    # the planted combination is the only one, and it sits where the note says
    r = ex["last_lane_16"][0]
    assert sum(x[2] for x in r) == 10 and r[4 + 6 + 8 + 14] == (4 + 6 + 8 + 15, 400, 1, 1) and r[-1] == (34, 400, 1, 1)
    r = ex["last_lane_64"][0]
    assert r[62] == (63, 400, 1, 1) and r[64 + 63] == (64, 400, 1, 1) and r[128 + 31] == (128 + 63, 400, 1, 1)
    r = ex["last_of_last_tile"][0]
    assert r[129] == (429, 400, 1, 1) and r[430 + 64] == (430 + 65 + 256, 400, 1, 1) and ex["last_of_last_tile"][1]["n_pairs_list"] == 2
    r, st = ex["pair_ids"]
    assert r[0][2] == 1 and r[-1] == (len(r) - 2, 495, 1, 1) and st["n_single"] == 1 and matecases.tables()["pair_ids"][0][0][0] == 6
    # 13.1: the classifier's verdict and the lane kernel's agree, clause by clause
    r = ex["edges"][0]
    verdict = [r[5 * p][2] for p in range(13)]
    assert verdict == [r[5 * p + 2][2] for p in range(13)] == [1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0]
    assert [x[1] for x in r if x[2]][0:2] == [300, 300] and ex["edges"][1]["tlen_max"] == 1000
    assert [x[2] for x in ex["max_insert_1"][0][0::5]] == [1, 0, 1] and ex["max_insert_1"][1]["tlen_sum"] == 2
    assert [x[2] for x in ex["max_insert_max"][0][0::5]] == [1, 0, 0, 1] and ex["max_insert_max"][1]["tlen_max"] == (1 << 31) - 1
    assert ex["sum_then_tl"][0][1] == (4, 330, 1, 4) and ex["sum_then_tl"][0][0] == U
    assert ex["tl_then_a_then_b"][0][0] == (3, 350, 1, 9) and ex["tl_then_a_then_b"][0][6] == (8, 340, 1, 6)
    assert ex["negative"][0][0] == (2, 300, 1, 1) and ex["negative"][0][5] == (7, 300, 1, 1)
    assert ex["extremes"][0][0] == (2, 300, 1, 1) and ex["extremes"][0][4] == (7, 300, 1, 2) and ex["extremes"][0][8] == (11, 310, 1, 1)
    assert sorted({x[3] for x in ex["n_best"][0] if x[2]}) == [1, 2, 64, 65]
    assert ex["n_best_across_tl"][0][1] == (2, 280, 1, 4)
    assert ex["n_best_90000"][0][0] == (300, 300, 1, 90000) and ex["n_best_90000"][1]["n_pairs_list"] == 1
    assert len(matecases.tables()["chains_256"][0]) == 256 and len(matecases.tables()["chains_257"][0]) == 257


def test_mated_paf():
    paf = (b"q/1\t100\t0\t50\t+\tt\t400\t5\t55\t50\t50\t255\tcm:i:12\ts1:i:100\n"
           b"q/2\t100\t0\t50\t-\tt\t400\t205\t255\t48\t50\t255\tcm:i:9\ts1:i:80\tNM:i:2\tcg:Z:48=2X\n"
           b"q/2\t100\t0\t50\t-\tu\t400\t5\t55\t48\t50\t0\ttp:A:S\tcm:i:9\ts1:i:80\ts2:i:0\tNM:i:2\n")
    assert mo.mated_paf(paf, [(1, 250, 1, 1), (0, 250, 1, 1), U]) == (
        b"q/1\t100\t0\t50\t+\tt\t400\t5\t55\t50\t50\t255\tcm:i:12\ts1:i:100\tpr:A:P\tmi:i:1\ttl:i:250\tnb:i:1\n"
        b"q/2\t100\t0\t50\t-\tt\t400\t205\t255\t48\t50\t255\tcm:i:9\ts1:i:80\tpr:A:P\tmi:i:0\ttl:i:250\tnb:i:1\tNM:i:2\tcg:Z:48=2X\n"
        b"q/2\t100\t0\t50\t-\tu\t400\t5\t55\t48\t50\t0\ttp:A:S\tcm:i:9\ts1:i:80\ts2:i:0\tpr:A:U\tNM:i:2\n")
    assert mo.mated_paf(b"", []) == b""


def test_the_cut_by_pairs():
    f = lambda a, b: 1000 + 10 * a + b
    assert mo.cut(f, [], [], 5000) == []
    assert mo.cut(f, [10, 10, 10, 10, 10, 10], [0] * 6, 1000 + 10 * 40) == [(0, 4, 40, 0, 1400), (4, 2, 20, 0, 1200)]
    assert mo.cut(f, [39, 1, 1, 0], [0] * 4, 1400) == [(0, 2, 40, 0, 1400), (2, 2, 1, 0, 1010)]  # the pair is the unit: 39 + 1 fit, a third record does not
    assert mo.cut(f, [0, 0, 0, 0], [5, 5, 5, 5], 1010) == [(0, 2, 0, 10, 1010), (2, 2, 0, 10, 1010)]
    with pytest.raises(MemoryError) as e:
        mo.cut(f, [1, 1, 30, 11, 1, 1], [0] * 6, 1400)
    assert str(e.value) == "pair 1"


# ---- the library and the wrappers

def test_abi(mp):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_map_set_mates", "msgpu_map_result_mates", "msgpu_map_result_mate_stats", "msgpu_map_batch_bytes_mates",
              "msgpu_map_mate_tables", "msgpu_map_mate_tables_stats", "msgpu_pl_run_mates"):
        assert hasattr(L, n) and n in bound and n + "(" in header, n
    assert C.sizeof(_lib.MapMate) == 16 == _lib.MAP_MATE_DTYPE.itemsize and C.sizeof(_lib.MapMateStats) == 128
    assert "#define MSGPU_MAP_MATES_ANCHOR_BYTES %du" % _lib.MAP_MATES_ANCHOR_BYTES in header and _lib.MAP_MATES_ANCHOR_BYTES == mo.ANCHOR_BYTES
    assert "#define MSGPU_MAP_MATES_FIXED_BYTES (12u * 256u)" in header and _lib.MAP_MATES_FIXED_BYTES == mo.FIXED_BYTES == 12 * 256
    assert "#define MSGPU_MAP_MAX_INSERT_DEFAULT %du" % _lib.MAP_MAX_INSERT_DEFAULT in header and _lib.MAP_MAX_INSERT_DEFAULT == 1000
    # no pinned struct grew
    assert C.sizeof(_lib.MapChain) == 48 == _lib.MAP_CHAIN_DTYPE.itemsize and C.sizeof(_lib.MapParams) == 48
    assert C.sizeof(_lib.MapStats) == 424 and C.sizeof(_lib.MapRank) == 16 and C.sizeof(_lib.MapRankStats) == 88
    assert C.sizeof(_lib.PlParams) == 8 and C.sizeof(_lib.PlStats) == 256
    assert L.msgpu_map_set_mates(None, 1, 1000) == _lib.E_ARG and L.msgpu_map_mate_tables(None, None, 0, 1000, None) == _lib.E_ARG
    assert L.msgpu_map_result_mates(None, None, None) == _lib.E_ARG and L.msgpu_map_result_mate_stats(None, None) == _lib.E_ARG
    assert L.msgpu_map_mate_tables_stats(None, None) == _lib.E_ARG
    assert L.msgpu_pl_run_mates(None, None, None, None, None, 0, None, None, None, 0, None) == _lib.E_ARG


def test_batch_bytes_mates(mp, monkeypatch):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("MSGPU_ALIGN_SLOTS", raising=False)
    for kw in (dict(), dict(exact=1), dict(exact=1, cigar=1), dict(exact=1, cigar=1, band=8)):
        prm = _lib.MapParams()
        L.msgpu_map_default_params(C.byref(prm))
        for key, v in kw.items():
            setattr(prm, key, v)
        for extend in (0, 300):
            for ranking in (0, 1):
                for a in (0, 1, 17, 1000, 230181, (1 << 31) - 1):
                    for b in (0, 1000, 1 << 20):
                        rank = int(L.msgpu_map_batch_bytes_rank(C.byref(prm), extend, ranking, a, b))
                        assert int(L.msgpu_map_batch_bytes_mates(C.byref(prm), extend, ranking, 0, a, b)) == rank
                        on = int(L.msgpu_map_batch_bytes_mates(C.byref(prm), extend, ranking, 1, a, b))
                        assert on == rank + mo.ANCHOR_BYTES * a + mo.FIXED_BYTES == rank + 60 * a + 12 * 256  # rule 13.7
                        assert on == int(L.msgpu_map_batch_bytes_mates(C.byref(prm), extend, ranking, 7, a, b))  # (a switch)
    assert int(L.msgpu_map_batch_bytes_mates(C.byref(prm), 0, 0, 1, 1 << 54, 0)) == (1 << 64) - 1


def test_rule_13_is_written_down_alike(mp):
    """the rule's paragraph in include/msgpu.h and in the module docstring carry the same sentences (spot checks), and the
    polisher's rule 2 in mates form and check (k) likewise"""
    import re
    from muchsalsa_amd import hybrid, polish
    header = " ".join(re.sub(r"(?m)^ \*", " ", open(os.path.join(ROOT, "include", "msgpu.h")).read()).split())
    doc = " ".join(mp.__doc__.replace("``", "").split())
    for sentence in ("13. mates, on request", "The query file is interleaved: records 2p and 2p + 1 are mate 1 and mate 2 of pair p",
                     "an odd number of query records is MSGPU_E_ARG naming the count", "max_insert is 1..2^31 - 1, default 1000.",
                     "The rule reads the chain table as the run leaves it, behind rule 11's extension.",
                     "f.t_start <= r.t_start, f.t_end <= r.t_end", "tl = r.t_end - f.t_start <= max_insert",
                     "Either mate may be the forward one.",
                     "the greatest score(a) + score(b) (a 64-bit sum), then the smaller tl, then the smaller index of a, then the smaller index of b",
                     "whatever their tl, clamped to 2^32 - 1", "every other chain has {0xffffffff, 0, 0, 0}",
                     "pr:A:P or pr:A:U behind s1:i (behind s2:i with ranking on)", "mi:i:<the mate's line, 0-based>, tl:i:<tlen>, nb:i:<n_best>",
                     "With mates off every byte of every output is as before.",
                     "a batch starts at an even record and holds whole pairs",
                     "a pair that exceeds the budget on its own is MSGPU_E_NOMEM naming the pair",
                     "per anchor it adds 60 bytes", "a fixed 12 * 256 bytes",
                     "Orientation FR only, the selection order and n_best are choices modelled on short-read mappers, unchecked on real reads."):
        assert sentence in header and sentence in doc, sentence
    known = doc[doc.index("Known differences from minimap2"):]
    assert "pairs: none without --mates" in known and "orientation FR only" in known and "unchecked on real reads" in known
    pdoc = " ".join(polish.__doc__.replace("``", "").split())
    for sentence in ("a chain votes iff it is eligible, selected (cls == 1) and n_best == 1",
                     "a pair placed equally well twice does not vote, an unselected chain never votes",
                     "a check (k) is added and reported last", 'otherwise "chain <i>: mates"'):
        assert sentence in header and sentence in pdoc, sentence
    assert "[--mates] [--max-insert N]" in mp.__doc__.split("\n\n")[1] and "[--mates] [--max-insert N]" in polish.__doc__.split("\n\n")[1]
    assert hybrid.POLISHED_MATES_NAME == "05.assembly.polished.mates.fa" and hybrid.MATES_MAPPING == dict(min_score=40)
    assert "unchecked on real reads" in " ".join(hybrid.run.__doc__.split())


def test_command_lines(mp, tmp_path, monkeypatch, capsys):
    """--mates and --max-insert N reach mapper.run and polish.run as keywords; both stand in the usage texts, which bad values
    end in; without them the calls carry neither keyword"""
    from muchsalsa_amd import polish
    seen = []
    monkeypatch.setattr(mp, "run", lambda *a, **kw: seen.append((a, kw)) or {})
    p = [str(tmp_path / n) for n in ("t.fa", "q.fq", "out.paf")]
    assert mp.main(p + ["--mates"]) == 0 and seen[-1][1]["mates"] is True and seen[-1][1]["max_insert"] == 1000
    assert mp.main(p + ["--max-insert", "500"]) == 0 and seen[-1][1]["mates"] is True and seen[-1][1]["max_insert"] == 500
    assert mp.main(p + ["--mates", "--rank", "--extend", "16", "--max-insert", "2147483647"]) == 0
    assert seen[-1][1]["max_insert"] == (1 << 31) - 1 and seen[-1][1]["rank"] is True and seen[-1][1]["extend"] == 16
    assert mp.main(p) == 0 and "mates" not in seen[-1][1] and "max_insert" not in seen[-1][1]
    capsys.readouterr()
    for bad in (["--max-insert"], ["--max-insert", "0"], ["--max-insert", "2147483648"], ["--max-insert", "x"], ["--mate"]):
        assert mp.main(p + bad) == 2, bad
        assert "[--mates] [--max-insert N]" in capsys.readouterr().err
    assert mp.main([p[0], p[0], p[2], "--ava", "--mates"]) == 2
    seen_pl = []
    monkeypatch.setattr(polish, "run", lambda *a, **kw: seen_pl.append((a, kw)) or {})
    assert polish.main(p + ["--mates"]) == 0 and seen_pl[-1][1]["mates"] is True and seen_pl[-1][1]["max_insert"] == 1000
    assert polish.main(p + ["--max-insert", "400", "--min-score", "40"]) == 0
    assert seen_pl[-1][1]["mates"] is True and seen_pl[-1][1]["max_insert"] == 400 and seen_pl[-1][1]["min_score"] == 40
    assert polish.main(p) == 0 and "mates" not in seen_pl[-1][1]
    capsys.readouterr()
    for bad in (["--max-insert", "0"], ["--mates", "--min-mapq", "3"]):
        assert polish.main(p + bad) == 2, bad
        assert "[--mates] [--max-insert N]" in capsys.readouterr().err


def test_the_wrappers_pass_mates_on(mp, tmp_path, monkeypatch):
    """polish.run(mates=True) maps with mates on and hands the rows to run_tables; without it neither call carries a word of it
    (and tables["mates"] is not read); hybrid.run gives its stage the interleaved file and MATES_MAPPING"""
    import inspect
    from muchsalsa_amd import hybrid, polish
    maps, tabs, run_tables = [], [], polish.run_tables
    counts = dict(dict.fromkeys(("chains", "anchors", "pairs", "capped"), 0), mate={"n_pairs": 0})
    monkeypatch.setattr(mp, "run", lambda *a, tables=None, **kw: (maps.append(kw), tables.update(
        dict(chains=[], runs=[], mates=[("rows",)]) if kw.get("mates") else dict(chains=[], runs=[])), counts)[2])
    monkeypatch.setattr(polish, "run_tables", lambda *a, **kw: tabs.append(kw) or {})
    polish.run("d.fa", "r.fq", str(tmp_path / "o.fa"), mates=True)
    assert maps[-1]["mates"] is True and maps[-1]["max_insert"] == 1000 and maps[-1]["rank"] is False and tabs[-1]["mates"] == [("rows",)]
    polish.run("d.fa", "r.fq", str(tmp_path / "o.fa"), rounds=2, mates=True, max_insert=300, min_score=40)
    assert [(m["mates"], m["max_insert"], m["min_score"]) for m in maps[-2:]] == [(True, 300, 40)] * 2 and len(tabs) == 3
    polish.run("d.fa", "r.fa", str(tmp_path / "o.fa"))
    assert "mates" not in maps[-1] and "max_insert" not in maps[-1] and "mates" not in tabs[-1]
    with pytest.raises(TypeError):
        polish.run("d.fa", "r.fq", str(tmp_path / "o.fa"), mates=True, min_mapq=0)
    sig = inspect.signature(hybrid.run).parameters
    assert sig["polish_mates"].default is None and sig["max_insert"].default is None
    src = inspect.getsource(hybrid.run)
    assert "mates=True, **more, **MATES_MAPPING" in src and 'result["files"]["polished"] if polish else files["assembly"]' in src
    assert "polished_mates" not in hybrid.output_names("n", "r.fq") and "polished_mates" not in hybrid.output_names("n", "r.fq").values()
    with pytest.raises(polish.PolishError) as e:
        run_tables("d.fa", "r.fa", str(tmp_path / "o.fa"), [ch(0, 1, 0, 1)], [[1 << 4 | 7]], mates=[])
    assert "mate rows" in str(e.value)
    with pytest.raises(polish.PolishError) as e:
        run_tables("d.fa", "r.fa", str(tmp_path / "o.fa"), [ch(0, 1, 0, 1)], [[1 << 4 | 7]], mates=[(-1, 0, 0, 0)])
    assert "mate row 0" in str(e.value)


def _fq(names, length=8, quality=b"I"):
    return b"".join(b"@%s\n%s\n+\n%s\n" % (n, b"ACGT" * (length // 4), quality * length) for n in names)


def test_interleave(mp, tmp_path):
    one, two, out = (str(tmp_path / n) for n in ("1.fq", "2.fq", "out.fq"))
    a, b = [b"p%d/1" % i for i in range(5)], [b"p%d/2" % i for i in range(5)]
    with open(one, "wb") as h:
        h.write(_fq(a))
    with open(two, "wb") as h:
        h.write(_fq(b)[:-1])  # (no line feed behind the last record)
    assert mp.interleave(one, two, out) == 5
    with open(out, "rb") as h:
        assert h.read() == _fq([n for pair in zip(a, b) for n in pair])
    # a quality line that starts with '@' would be taken for a description line by the loader: its first byte becomes 'A'
    with open(one, "wb") as h:
        h.write(_fq(a[:1], quality=b"@"))
    with open(two, "wb") as h:
        h.write(_fq(b[:1]))
    assert mp.interleave(one, two, out) == 1
    with open(out, "rb") as h:
        assert h.read() == b"@p0/1\nACGTACGT\n+\nA@@@@@@@\n" + _fq(b[:1])
    # no records at all
    for path in (one, two):
        open(path, "wb").close()
    assert mp.interleave(one, two, out) == 0 and os.path.getsize(out) == 0
    # unequal counts, either way
    for n1, n2 in ((3, 2), (2, 3)):
        with open(one, "wb") as h:
            h.write(_fq(a[:n1]))
        with open(two, "wb") as h:
            h.write(_fq(b[:n2]))
        with pytest.raises(ValueError) as e:
            mp.interleave(one, two, out)
        assert "2 pairs read" in str(e.value) and not os.path.exists(out)
    # a truncated record, a record without '@', a quality line of another length
    for text in (_fq(a[:2])[:-12], _fq(a[:1]) + b">p1/1\nACGT\n+\nIIII\n", _fq(a[:1]) + b"@p1/1\nACGT\n+\nIII\n", _fq(a[:1]) + b"@p1/1\nACGT\n-\nIIII\n"):
        with open(one, "wb") as h:
            h.write(text)
        with open(two, "wb") as h:
            h.write(_fq(b[:2]))
        with pytest.raises(ValueError) as e:
            mp.interleave(one, two, out)
        assert "record 1" in str(e.value) and one in str(e.value) and not os.path.exists(out)


def test_no_device_means_an_error_not_a_fallback(mp, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the stage would run")
    from muchsalsa_amd import _lib
    with pytest.raises(mp.MapError) as e:
        mp.mate_tables(matecases.tables()["edges"][0])
    assert e.value.code == _lib.E_NODEVICE
    with pytest.raises(mp.MapError) as e:
        mp.mate_tables([])
    assert e.value.code == _lib.E_NODEVICE
