"""Rule 12 (the mapper's primaries, secondaries and mapping quality), host side (no GPU): paper cases of the restatement
(tests/map_rank_oracle.py) worked by hand, its invariants on every table the GPU file compares, what the tables were made to
hold, the C-ABI with its pinned sizes, the byte bound, the rule's text in its two places and the command lines."""
import ctypes as C
import os

import pytest

import map_rank_oracle as ro
import rankcases
from rankcases import ch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


# ---- the restatement

def test_paper_cases():
    # one chain: primary, sub 0, mapq = 60 * 100 * 10 / (10 * 100) = 60 with 12 anchors, 60 * 100 * 3 / 1000 = 18 with 3
    assert ro.rank([ch(0, 100, 0, 50)]) == [(0, 0, 0, 60)]
    assert ro.rank([ch(0, 100, 0, 50, anchors=3)]) == [(0, 0, 0, 18)]
    # two copies of a repeat with equal scores: the first is primary with sub = its own score, so mapq 0
    assert ro.rank([ch(0, 100, 0, 100), ch(0, 100, 0, 100)]) == [(0, 100, 1, 0), (0, 0, 0, 0)]
    # the better copy comes second in the table: it is visited first.  mapq = 60 * (200 - 150) * 10 / 2000 = 15; 1500 < 1800
    assert ro.rank([ch(0, 150, 0, 100), ch(0, 200, 0, 100)]) == [(1, 0, 0, 0), (1, 150, 0, 15)]
    # a split alignment: two disjoint halves are two primaries
    assert ro.rank([ch(0, 300, 0, 500), ch(0, 250, 500, 1000)]) == [(0, 0, 0, 60), (1, 0, 0, 60)]
    # 12.2: ov = 50 of a shorter length 100 is not more than half; ov = 51 is
    assert [r[0] for r in ro.rank([ch(0, 200, 0, 100), ch(0, 100, 50, 150)])] == [0, 1]
    assert [r[0] for r in ro.rank([ch(0, 200, 0, 100), ch(0, 100, 49, 149)])] == [0, 0]
    # the shorter of the two decides: ov = 20 of [50, 70) against [0, 100)
    assert [r[0] for r in ro.rank([ch(0, 200, 0, 100), ch(0, 100, 50, 70)])] == [0, 0]
    # 12.3: 90 counts against 100 (900 >= 900), 89 does not; sub is the greatest
    assert ro.rank([ch(0, 100, 0, 100), ch(0, 89, 0, 100), ch(0, 90, 0, 100)])[0] == (0, 90, 1, 6)
    # 12.4: n_anchors 9 -> 60 * 50 * 9 / 1000 = 27; 10 and 11 -> 30
    assert [ro.mapq(100, 50, a) for a in (9, 10, 11)] == [27, 30, 30]
    assert ro.mapq(0, 0, 12) == 0 and ro.mapq(-4, -9, 12) == 0 and ro.mapq(7, -100, 12) == 60 and ro.mapq(1000, 999, 10) == 0
    # the chains of another query record never meet
    assert ro.rank([ch(0, 100, 0, 100), ch(1, 100, 0, 100)]) == [(0, 0, 0, 60), (1, 0, 0, 60)]
    # the first overlapping primary in visiting order, not in table order: chain 3 meets chains 0 and 2, and 2 is visited first
    rows = ro.rank(rankcases.tables()["first_overlap"][0])
    assert [r[0] for r in rows] == [0, 2, 2, 2, 5, 5, 6]
    # base is added to every parent, and to nothing else
    assert ro.rank([ch(0, 100, 0, 100), ch(0, 100, 0, 100)], base=7) == [(7, 100, 1, 0), (7, 0, 0, 0)]
    assert ro.rank([]) == []


def test_ties_go_to_the_smaller_index():
    rows = ro.rank(rankcases.tables()["ties"][0])
    # [0,100) first; [10,110) and [20,120) are its secondaries; [200,300) is primary and [190,290) its secondary
    assert [r[0] for r in rows] == [0, 0, 2, 2, 0]
    assert rows[0] == (0, 100, 2, 0) and rows[2] == (2, 100, 1, 0)


@pytest.mark.parametrize("name", rankcases.NAMES)
def test_invariants_on_every_table(name):
    chains = rankcases.tables()[name][0]
    rows, st = rankcases.expected(name)
    assert len(rows) == len(chains)
    ro.invariants(chains, rows)
    assert st["n_primaries"] + st["n_secondaries"] == len(chains) and st["n_segments"] == len(ro.segments(chains))
    assert st["n_segments_single"] + st["n_segments_wave"] + st["n_segments_list"] == st["n_segments"]


def test_the_tables_hold_what_they_were_made_for():
    T, E = rankcases.tables(), rankcases.expected
    st = E("sizes")[1]
    assert (st["n_segments_single"], st["n_segments_wave"], st["n_segments_list"], st["largest_segment"]) == (1, 3, 3, 129)
    assert [e - f for f, e in ro.segments(T["sizes"][0])] == [1, 2, 63, 64, 65, 128, 129]
    assert 0 < st["n_secondaries"] and st["n_segments_spilled"] == 0
    assert E("lds_exact")[1]["n_primaries"] == ro.LDS and E("lds_exact")[1]["n_segments_spilled"] == 0
    rows, st = E("lds_plus_one")
    assert st["n_primaries"] == ro.LDS + 1 and st["n_segments_spilled"] == 1 and st["n_secondaries"] == 4
    assert [r[0] for r in rows[-4:]] == [0, ro.LDS - 1, ro.LDS, ro.LDS]  # the last two read the entry in the arena
    rows, st = E("lds_far")
    assert st["n_segments_spilled"] == 1 and st["n_segments_list"] == 2 and st["n_primaries"] > ro.LDS + 64 and st["n_secondaries"] > 64
    assert [r[0] for r in E("half")[0]] == [0, 1, 2, 2, 4, 4, 6, 7, 8, 8]  # (ov 50 of 70; ov 35 of 70; ov 36 of 70)
    assert E("ratio")[0][0] == (0, 100, 2, 0) and E("ratio")[0][4][:3] == (4, 7, 1)
    rows = E("low_scores")[0]
    assert all(r[3] == 0 for r in rows[:5]) and rows[2][:2] == (2, -2147483648) and rows[5] == (5, -2147483648, 0, 60)
    assert rows[7] == (7, -7, 0, 60)
    assert [r[3] for r in E("anchors")[0][0:6:2]] == [27, 30, 30] and E("anchors")[0][6][3] == 6
    st = E("singles_then_list")[1]
    assert (st["n_segments_single"], st["n_segments_list"], st["n_segments_wave"]) == (64, 1, 0)
    assert [r[0] for r in E("wide")[0]] == [0, 0, 0, 0]  # (all lie inside chain 0; 2 * ov = 2^32 in 32 bits would be 0)
    assert E("empty") == ([], dict.fromkeys(ro.STATS, 0))
    for name, (chains, first, word) in rankcases.bad_tables().items():
        with pytest.raises(ro.RankError) as e:
            ro.rank(chains)
        assert e.value.chain == first and word in str(e.value), name


def test_ranked_paf():
    paf = (b"q\t100\t0\t50\t+\tt\t400\t5\t55\t50\t50\t255\tcm:i:12\ts1:i:100\n"
           b"q\t100\t0\t50\t-\tu\t400\t5\t55\t48\t50\t255\tcm:i:9\ts1:i:80\tNM:i:2\tcg:Z:48=2X\n")
    rows = [(0, 80, 0, 12), (0, 0, 0, 0)]
    assert ro.ranked_paf(paf, rows) == (
        b"q\t100\t0\t50\t+\tt\t400\t5\t55\t50\t50\t12\ttp:A:P\tcm:i:12\ts1:i:100\ts2:i:80\n"
        b"q\t100\t0\t50\t-\tu\t400\t5\t55\t48\t50\t0\ttp:A:S\tcm:i:9\ts1:i:80\ts2:i:0\tNM:i:2\tcg:Z:48=2X\n")
    assert ro.ranked_paf(b"", []) == b""


# ---- the library and the wrappers

def test_abi(mp):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_map_set_ranking", "msgpu_map_result_ranks", "msgpu_map_result_rank_stats", "msgpu_map_batch_bytes_rank",
              "msgpu_map_rank_tables", "msgpu_map_rank_tables_stats", "msgpu_pl_run_ranked"):
        assert hasattr(L, n) and n in bound and n + "(" in header, n
    assert C.sizeof(_lib.MapRank) == 16 == _lib.MAP_RANK_DTYPE.itemsize and C.sizeof(_lib.MapRankStats) == 88
    assert "#define MSGPU_MAP_RANK_LDS %du" % _lib.MAP_RANK_LDS in header and _lib.MAP_RANK_LDS == ro.LDS
    # no pinned struct grew
    assert C.sizeof(_lib.MapChain) == 48 == _lib.MAP_CHAIN_DTYPE.itemsize and C.sizeof(_lib.MapParams) == 48
    assert C.sizeof(_lib.MapStats) == 424 and C.sizeof(_lib.PlParams) == 8 and C.sizeof(_lib.PlStats) == 256
    assert L.msgpu_map_set_ranking(None, 1) == _lib.E_ARG and L.msgpu_map_rank_tables(None, None, 0, None) == _lib.E_ARG
    assert L.msgpu_map_result_ranks(None, None, None) == _lib.E_ARG and L.msgpu_map_result_rank_stats(None, None) == _lib.E_ARG


def test_batch_bytes_rank(mp, monkeypatch):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("MSGPU_ALIGN_SLOTS", raising=False)
    for kw in (dict(), dict(exact=1), dict(exact=1, cigar=1), dict(exact=1, cigar=1, band=8)):
        prm = _lib.MapParams()
        L.msgpu_map_default_params(C.byref(prm))
        for key, v in kw.items():
            setattr(prm, key, v)
        for extend in (0, 300):
            for a in (0, 1, 17, 1000, 230181, (1 << 31) - 1):
                for b in (0, 1000, 1 << 20):
                    ext = int(L.msgpu_map_batch_bytes_ext(C.byref(prm), extend, a, b))
                    assert int(L.msgpu_map_batch_bytes_rank(C.byref(prm), extend, 0, a, b)) == ext
                    on = int(L.msgpu_map_batch_bytes_rank(C.byref(prm), extend, 1, a, b))
                    assert on >= ext and on == ext + 104 * a + 24 * 256  # rule 12.7's bytes per anchor and the fixed part
                    assert on == int(L.msgpu_map_batch_bytes_rank(C.byref(prm), extend, 7, a, b))  # (a switch: any value but 0)
    assert int(L.msgpu_map_batch_bytes_rank(C.byref(prm), 0, 1, 1 << 54, 0)) == (1 << 64) - 1


def test_rule_12_is_written_down_alike(mp):
    """the rule's paragraph in include/msgpu.h and in the module docstring carry the same sentences (spot checks), and the
    polisher's ranked rule 2 likewise"""
    from muchsalsa_amd import polish
    import re
    header = " ".join(re.sub(r"(?m)^ \*", " ", open(os.path.join(ROOT, "include", "msgpu.h")).read()).split())
    doc = " ".join(mp.__doc__.replace("``", "").split())
    for sentence in ("12. primaries, secondaries and mapping quality, on request",
                     "Rule 11 changes no rank: rule 12 reads the ranges as rule 7 leaves them, before any extension.",
                     "Visiting order: by (score descending, output index ascending).",
                     "the first primary p with 2 * ov(c, p) > min(len(c), len(p)) makes c secondary with parent(c) = p",
                     "The mask level is one half and the comparison is strict.",
                     "10 * score(s) >= 9 * score(p)", "(60 * (s1 - sub) * min(n_anchors, 10)) / (10 * s1)",
                     "With ranking off every byte is as before: 255, no tp, no s2.",
                     "unchecked on real reads"):
        assert sentence in header and sentence in doc, sentence
    pdoc = " ".join(polish.__doc__.split())
    for sentence in ("a chain votes iff it is eligible, primary (parent == its own index) and mapq >= min_mapq",
                     "a secondary never votes"):
        assert sentence in header and sentence in pdoc, sentence
    assert "no primary / secondary marking" not in mp.__doc__ and "no mapping quality" not in mp.__doc__


def test_command_lines(mp, tmp_path, monkeypatch, capsys):
    """--rank reaches mapper.run as the keyword; --min-mapq N reaches polish.run; both stand in the usage texts, which bad
    values end in"""
    from muchsalsa_amd import polish
    seen = []
    monkeypatch.setattr(mp, "run", lambda *a, **kw: seen.append((a, kw)) or {})
    p = [str(tmp_path / n) for n in ("t.fa", "q.fa", "out.paf")]
    assert mp.main(p + ["--rank"]) == 0 and seen[-1][1]["rank"] is True and seen[-1][1]["cigar"] == 0
    assert mp.main(p + ["--rank", "--extend", "16"]) == 0 and seen[-1][1]["rank"] is True and seen[-1][1]["extend"] == 16
    assert mp.main(p) == 0 and seen[-1][1]["rank"] is False
    capsys.readouterr()
    assert mp.main(p + ["--ranks"]) == 2 and "[--rank]" in capsys.readouterr().err
    seen_pl = []
    monkeypatch.setattr(polish, "run", lambda *a, **kw: seen_pl.append((a, kw)) or {})
    assert polish.main(p + ["--min-mapq", "1"]) == 0 and seen_pl[-1][1]["min_mapq"] == 1
    assert polish.main(p + ["--min-mapq", "0"]) == 0 and seen_pl[-1][1]["min_mapq"] == 0
    assert polish.main(p) == 0 and seen_pl[-1][1]["min_mapq"] is None
    capsys.readouterr()
    for bad in (["--min-mapq"], ["--min-mapq", "61"], ["--min-mapq", "-1"], ["--min-mapq", "x"]):
        assert polish.main(p + bad) == 2, bad
        assert "[--min-mapq N]" in capsys.readouterr().err


def test_the_wrappers_pass_ranking_on(mp, tmp_path, monkeypatch):
    """polish.run(min_mapq=N) maps with rank=True and hands the rows to run_tables; without it neither; hybrid.run has the
    keyword and gives it to the polish stage alone"""
    import inspect
    from muchsalsa_amd import hybrid, polish
    maps, tabs, run_tables = [], [], polish.run_tables
    monkeypatch.setattr(mp, "run", lambda *a, tables=None, **kw: (maps.append(kw), tables.update(chains=[], runs=[], ranks=[("rows",)]),
                                                                   dict.fromkeys(("chains", "anchors", "pairs", "capped"), 0))[2])
    monkeypatch.setattr(polish, "run_tables", lambda *a, **kw: tabs.append(kw) or {})
    polish.run("d.fa", "r.fa", str(tmp_path / "o.fa"), min_mapq=0)
    assert maps[-1]["rank"] is True and tabs[-1]["ranks"] == [("rows",)] and tabs[-1]["min_mapq"] == 0
    polish.run("d.fa", "r.fa", str(tmp_path / "o.fa"), rounds=2, min_mapq=7)
    assert [m["rank"] for m in maps[-2:]] == [True, True] and [t["min_mapq"] for t in tabs[-2:]] == [7, 7]
    polish.run("d.fa", "r.fa", str(tmp_path / "o.fa"))
    assert maps[-1]["rank"] is False and tabs[-1]["ranks"] is None
    assert inspect.signature(hybrid.run).parameters["min_mapq"].default is None
    src = inspect.getsource(hybrid.run)
    assert src.count("min_mapq=min_mapq") == 1 and "rank=" not in src  # the four mappings keep ranking off
    with pytest.raises(polish.PolishError) as e:
        run_tables("d.fa", "r.fa", str(tmp_path / "o.fa"), [ch(0, 1, 0, 1)], [[1 << 4 | 7]], ranks=[])
    assert "rank rows" in str(e.value)


def test_no_device_means_an_error_not_a_fallback(mp, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the stage would run")
    from muchsalsa_amd import _lib
    with pytest.raises(mp.MapError) as e:
        mp.rank_tables(rankcases.tables()["half"][0])
    assert e.value.code == _lib.E_NODEVICE
    with pytest.raises(mp.MapError) as e:
        mp.rank_tables([])
    assert e.value.code == _lib.E_NODEVICE
