"""Rule 11 (the mapper's end extension), host side (no GPU): paper cases of the restatement (tests/map_extend_oracle.py), every
tie of the end cell made visible, the early stop shown to change nothing, the validity of every script the GPU file compares,
the property that flanks without an edit are extended to the sequence end, the chain-level invariants of every mapper case the
GPU file uses, the C-ABI with its pinned struct sizes, the byte bound and the command lines."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import cigarcases
import extendcases
import map_cigar_oracle as co
import map_extend_oracle as xo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, D, I = co.X, co.D, co.I


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


def test_paper_cases():
    # n = 0, m = 0 and both: cell (0, 0) alone can win, and the bound n + m - 8 e ends the table at once
    assert xo.reach(b"", b"", 8) == ((0, 0, 0, 0, 0, 1), [0])
    assert xo.reach(b"ACGT", b"", 8) == ((0, 0, 0, 0, 0, 1), [0])
    assert xo.reach(b"", b"ACGT", 8) == ((0, 0, 0, 0, 0, 1), [0])
    # identical flanks, and a shorter side that matches the longer side's start: cell (0, 0) reaches the end
    assert xo.reach(b"ACGTACGTAC", b"ACGTACGTAC", 8) == ((0, 0, 10, 10, 20, 1), [10])
    assert xo.reach(b"ACGTAC", b"ACGTACGTAC", 8)[0][:5] == (0, 0, 6, 6, 12)
    assert xo.reach(b"ACGTACGTAC", b"ACGT", 8)[0][:5] == (0, 0, 4, 4, 8)
    # a mismatch at byte 0: three matches behind it do not pay for it (2 * 4 - 8 = 0 ties with no extension, the smaller e
    # wins), four do
    assert xo.reach(b"ACGT", b"TCGT", 8) == ((0, 0, 0, 0, 0, 1), [0])
    assert xo.reach(b"ACGTA", b"TCGTA", 8) == ((1, 0, 5, 5, 2, 2), [X << 30, 4])
    # band 0: row 0 only
    assert xo.reach(b"ACGTA", b"TCGTA", 0) == ((0, 0, 0, 0, 0, 1), [0])
    # an end cell that is not the corner: the good bytes are taken, the junk behind them is left
    a, b = b"ACGTTGCAAC" + b"AAAAAAAA", b"ACGTTGCAAC" + b"CCCCCCCC"
    assert xo.reach(a, b, 8)[0][:5] == (0, 0, 10, 10, 20)
    # a deletion and an insertion inside good flanks
    end, words = xo.reach(b"ACGTTGCAACGGTCAGTCA", b"ACGTTGCAAGGTCAGTCA", 8)
    assert end[:5] == (1, -1, 19, 18, 29) and words == [D << 30 | 9, 9]
    end, words = xo.reach(b"ACGTTGCAAGGTCAGTCA", b"ACGTTGCAACGGTCAGTCA", 8)
    assert end[:5] == (1, 1, 18, 19, 29) and words == [I << 30 | 9, 9]


def test_every_tie_of_the_end_cell():
    assert xo.better(3, 5, 0, 2, 0, 0) and not xo.better(2, 0, 0, 3, 5, 0)            # the score
    assert xo.better(3, 1, 4, 3, 2, 0) and not xo.better(3, 2, 0, 3, 1, 4)            # then the smaller e
    assert xo.better(3, 2, -1, 3, 2, 2) and not xo.better(3, 2, -2, 3, 2, 1)          # then the smaller |k|
    assert xo.better(3, 2, -1, 3, 2, 1) and not xo.better(3, 2, 1, 3, 2, -1)          # then the negative k
    assert not xo.better(3, 2, 1, 3, 2, 1)
    # equal scores in rows 0 and 1: no extension
    assert xo.reach(b"CCAC", b"ACAC", 4)[0][:5] == (0, 0, 0, 0, 0)
    # equal scores on the diagonals -2 and 0 of row 2: the smaller |k|
    end, words = xo.reach(b"ACACACAAGCACACACAC", b"ACACACACACACACACA", 2)
    assert end[:5] == (2, 0, 17, 17, 18) and words == [X << 30 | 7, X << 30, 8]
    # equal scores on the diagonals -1 and +1 of row 1: the negative k
    end, words = xo.reach(b"CACAC", b"ACACA", 4)
    assert end[:5] == (1, -1, 5, 4, 1) and words == [D << 30, 4]


def test_the_early_stop_never_changes_a_result():
    """the restatement with and without the stop at the first row that cannot win, over 400 seeded random pairs: the same end
    cell (``rows`` included) and the same words"""
    r = random.Random(11)
    stopped = 0
    for t in range(400):
        n = r.randrange(0, 120)
        a = bytes(r.choice(b"ACGT") for _ in range(n))
        b = bytearray(a)
        for _ in range(r.randrange(0, max(1, n // 4))):
            op, pos = r.randrange(3), r.randrange(len(b) + 1)
            if op == 0 and b:
                b[min(pos, len(b) - 1)] = r.choice(b"ACGT")
            elif op == 1:
                b.insert(pos, r.choice(b"ACGT"))
            elif b:
                del b[min(pos, len(b) - 1)]
        b = bytes(b[:r.randrange(len(b) + 1)] if t % 5 == 0 else b)
        band = (3, 8, 20, 40)[t % 4]
        full, short = xo.reach(a, b, band), xo.reach(a, b, band, early_stop=True)
        assert full == short, (a, b, band)
        xo.check_extension(a, b, *full)
        stopped += full[0][5] <= band
    assert 100 <= stopped <= 400


@pytest.mark.parametrize("key", list(extendcases.BANDS) + [("random", 0), ("random", 1)], ids=str)
def test_every_script_of_the_gpu_lists_is_valid(key):
    """expected_pairs() checks rule 11.4's properties on every pair; here: what the lists were made to hold"""
    ends, off, words = extendcases.expected_pairs(key)
    assert len(off) == len(ends) + 1 and off[-1] == len(words) and all(off[i + 1] - off[i] == e[0] + 1 for i, e in enumerate(ends))
    if isinstance(key, tuple):
        count, band, _ = extendcases.RANDOM[key[1]]
        assert len(ends) == count
        assert sum(1 for e in ends if e[0] > 0) > count // 4 and sum(1 for e in ends if e[5] == band + 1) >= 1
        assert (max(e[0] for e in ends) > 31) == (band > 31)
        return
    band, pairs = key, extendcases.hand_pairs(key)
    by_pair = dict(zip(pairs, ends))
    for n in extendcases.IDENTICAL:
        assert ends[1 + extendcases.IDENTICAL.index(n)][:5] == (0, 0, n, n, 2 * n)
    assert max(e[0] for e in ends) == band                     # an end cell in row `band`
    assert ends[-4][0] <= band and ends[-4][2] < len(pairs[-4][0])  # the pair that needs row band + 1 stops short of its end
    # two random flanks of 300 bytes: a few bytes at most, and every row runs (up to row 74: 600 - 8 * 75 cannot win any more)
    assert ends[-3][2] <= 8 and ends[-3][5] == min(band + 1, (600 - ends[-3][4] + 7) // 8)
    assert 138 <= ends[-2][2] <= 160                           # 150 good bytes, then random ones
    if band >= 70:
        ks = sorted(e[1] for p, e in by_pair.items() if len(p[0]) in (740, 803, 804, 805, 810) and len(p[1]) != len(p[0]))
        assert ks == [-70, -65, -64, -63, 63, 64, 65, 70]


def test_flanks_without_an_edit_reach_the_sequence_end():
    """rule 11.6 on mapcases' error-free contained queries: every chain then covers its whole query"""
    for name in ("perfect", "reverse"):
        want = extendcases.expected(name, 300)
        base = cigarcases.expected(name)
        assert len(want["chains"]) == len(base["chains"]) >= 1
        for ch, old, (left, right) in zip(want["chains"], base["chains"], want["ext"]):
            assert (ch[6], ch[7]) == (0, 200) and ch[5] == 0 and ch[10] == ch[11] == 200
            assert (old[6], old[7]) != (0, 200) and left[0] == right[0] == 0 and left[2] + right[2] == 200 - (old[7] - old[6])
            assert ch[:5] == old[:5]
        assert want["stats"]["n_ends_at_sequence_end"] == want["stats"]["n_ends"] == 2 * len(want["chains"])


@pytest.mark.parametrize("case", extendcases.CASES, ids=lambda c: "%s-%d" % (c[0], c[2]))
def test_chain_level_invariants(case):
    """on every mapper case of the GPU file (extend_run asserts that the runs consume the new ranges and that nm grows by the
    ends' edits): ranges inside the records and never smaller than without the extension, order and identity of the chains
    untouched, no end beyond extend"""
    name, params, extend = case
    want = extendcases.expected(name, extend, **params)
    base = want["cigar"]
    targets, queries = extendcases.records(name)
    assert len(want["chains"]) == len(base["chains"]) and want["stats"]["n_ends"] == 2 * len(base["chains"])
    for ch, old, ends in zip(want["chains"], base["chains"], want["ext"]):
        assert ch[:5] == old[:5]
        assert 0 <= ch[8] <= old[8] < old[9] <= ch[9] <= len(targets[ch[1]][1])
        assert 0 <= ch[6] <= old[6] < old[7] <= ch[7] <= len(queries[ch[0]][1])
        assert all(e[2] <= extend and e[3] <= extend and e[0] <= base["exact"]["params"]["band"] for e in ends)
    assert xo.extend_run(targets, queries, 0, cigar_result=base)["paf"] == base["paf"]
    if name == "ends" and extend == 300:
        by_query = {queries[ch[0]][0]: ch for ch in want["chains"] if ch[1] == 0}
        for q in (b"left", b"left_rc", b"left_noisy"):
            assert by_query[q][8] == 0, q                        # the extension stops at target byte 0
        for q in (b"right", b"right_rc"):
            assert by_query[q][9] == len(targets[0][1]), q       # and at its last byte
        for q in (b"inner", b"noisy", b"inner_rc", b"noisy_rc"):
            assert (by_query[q][6], by_query[q][7]) == (0, len(queries[by_query[q][0]][1])), q
        assert want["stats"]["x_columns"] >= 3 and want["stats"]["i_columns"] + want["stats"]["d_columns"] >= 1


def test_abi(mp):
    from muchsalsa_amd import _lib, sequences
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_map_set_extension", "msgpu_map_result_ext_stats", "msgpu_map_result_ext_ends", "msgpu_map_batch_bytes_ext",
              "msgpu_extend_ends"):
        assert hasattr(L, n) and n in bound and n + "(" in header, n
    # the five pinned sizes have not moved: the feature adds no field to any of them
    assert C.sizeof(_lib.MapParams) == 48 and C.sizeof(_lib.MapChain) == 48 and C.sizeof(_lib.MapStats) == 424
    assert C.sizeof(_lib.MapAlignStats) == 104 and C.sizeof(_lib.MapBatch) == 64
    assert C.sizeof(_lib.ExtEnd) == 24 == _lib.EXT_END_DTYPE.itemsize and C.sizeof(_lib.MapExtStats) == 104
    assert "#define MSGPU_MAP_EXTEND_MAX 65535u" in header and _lib.MAP_EXTEND_MAX == 65535
    assert "#define MSGPU_MAP_EXTEND_PENALTY 8" in header and _lib.MAP_EXTEND_PENALTY == xo.P == 8
    assert [n for n, _ in _lib.MapExtStats._fields_] == ["extend", "reserved", "n_ends", "n_ends_extended", "n_ends_at_sequence_end",
                                                         "t_bases", "q_bases", "x_columns", "i_columns", "d_columns", "max_e", "rows",
                                                         "n_inconsistent", "extend_ms"]
    assert [n for n, _ in _lib.ExtEnd._fields_] == ["e", "k", "x", "y", "score", "rows"]
    assert hasattr(sequences.SeqStore, "extend_ends")
    # null arguments are rejected before anything is touched
    n = C.c_uint64()
    assert L.msgpu_map_set_extension(None, 1) == _lib.E_ARG
    assert L.msgpu_map_result_ext_stats(None, None) == _lib.E_ARG
    assert L.msgpu_map_result_ext_ends(None, None, C.byref(n)) == _lib.E_ARG
    assert L.msgpu_extend_ends(None, None, None, None, 0, 64, 0, None, None, None, 0, C.byref(n)) == _lib.E_ARG


def test_rule_11_is_written_down_alike(mp):
    """the rule's paragraph in include/msgpu.h and in the module docstring carry the same sentences (spot checks)"""
    header = " ".join(open(os.path.join(ROOT, "include", "msgpu.h")).read().replace(" *", " ").split())
    doc = " ".join(mp.__doc__.replace("``", "'").split())
    header = header.replace("'='", "'").replace("``", "'")
    for sentence in ("11. end extension, on request", "The penalty is a constant of the rule, P = 8.",
                     "on equal scores the smaller e wins, then the smaller |k|, then the negative k.",
                     "a left flank's columns are written in reverse order.", "(6) With E = 0 every byte is as before."):
        assert sentence in header and sentence in doc, sentence
    assert "no end extension beyond the outermost seeds" not in mp.__doc__
    assert "rule 11 (unit costs, P = 8, no end bonus)" in mp.__doc__


def test_batch_bytes_ext(mp, monkeypatch):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("MSGPU_ALIGN_SLOTS", raising=False)

    def params(**kw):
        prm = _lib.MapParams()
        L.msgpu_map_default_params(C.byref(prm))
        for key, v in kw.items():
            setattr(prm, key, v)
        return prm

    sizes = [0, 1, 17, 1000, 230181, (1 << 31) - 1]
    for kw in (dict(), dict(exact=1), dict(exact=1, cigar=1), dict(exact=1, cigar=1, band=8), dict(exact=1, cigar=1, band=127)):
        prm = params(**kw)
        for a in sizes:
            for b in (0, 1000, 1 << 20):
                plain = int(L.msgpu_map_batch_bytes(C.byref(prm), a, b))
                assert int(L.msgpu_map_batch_bytes_ext(C.byref(prm), 0, a, b)) == plain
                ext = int(L.msgpu_map_batch_bytes_ext(C.byref(prm), 300, a, b))
                if not kw.get("cigar"):
                    assert ext == plain  # (such a run is rejected: nothing is added)
                    continue
                # per chain end (at most two per anchor): a descriptor, an end cell and band + 1 script words
                per = 2 * (24 + 24 + 4 * (kw.get("band", 64) + 1))
                assert plain + a * per <= ext <= plain + a * per + 4096
                assert ext == int(L.msgpu_map_batch_bytes_ext(C.byref(prm), 1, a, b)) == int(
                    L.msgpu_map_batch_bytes_ext(C.byref(prm), 65535, a, b))  # (the flanks are read in place: no copies)
    top = (1 << 64) - 1
    prm = params(exact=1, cigar=1, band=127)
    assert int(L.msgpu_map_batch_bytes_ext(C.byref(prm), 300, 1 << 50, 0)) == top
    assert int(L.msgpu_map_batch_bytes_ext(C.byref(prm), 300, (1 << 50) - 1, (1 << 62) - 1)) < top


def test_command_lines_take_extend(mp, tmp_path, monkeypatch, capsys):
    """--extend N implies --cigar (and so --exact) and reaches run() as the keyword, in the mapper and in the polisher; bad
    values end in the usage text"""
    from muchsalsa_amd import polish
    seen = []
    monkeypatch.setattr(mp, "run", lambda *a, **kw: seen.append((a, kw)) or {})
    p = [str(tmp_path / n) for n in ("t.fa", "q.fa", "out.paf")]
    assert mp.main(p + ["--extend", "300"]) == 0
    assert seen[-1][1]["extend"] == 300 and seen[-1][1]["cigar"] == 1 and seen[-1][1]["exact"] == 1
    assert mp.main(p + ["--cigar"]) == 0 and seen[-1][1]["extend"] == 0 and seen[-1][1]["cigar"] == 1
    assert mp.main(p) == 0 and seen[-1][1]["extend"] == 0 and seen[-1][1]["cigar"] == 0
    capsys.readouterr()
    for bad in (["--extend"], ["--extend", "0"], ["--extend", "65536"], ["--extend", "x"]):
        assert mp.main(p + bad) == 2, bad
        assert "[--extend N]" in capsys.readouterr().err
    seen_pl = []
    monkeypatch.setattr(polish, "run", lambda *a, **kw: seen_pl.append((a, kw)) or {})
    assert polish.main(p + ["--extend", "300"]) == 0 and seen_pl[-1][1]["extend"] == 300
    assert polish.main(p) == 0 and seen_pl[-1][1]["extend"] == 0
    capsys.readouterr()
    assert polish.main(p + ["--extend", "65536"]) == 2 and "[--extend N]" in capsys.readouterr().err
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.mapper", p[0], p[1], "--extend", "300"], cwd=ROOT, env=env,
                         capture_output=True, timeout=300)
    assert out.returncode == 2 and b"[--extend N]" in out.stderr


def test_the_drivers_names_are_unchanged():
    import inspect
    from muchsalsa_amd import hybrid, polish
    names = hybrid.output_names("x", "/data/reads.fastq")
    assert sorted(names) == sorted(["report", "unitigs", "unitigs_cut", "link", "unitigs_paf", "corrected_paf", "scrubbed", "exact_paf",
                                    "assembly", "corrected", "ava_paf", "target", "query", "align"])
    assert names["exact_paf"] == "02_contigs_corrected.to_reads.scrubbed.paf" and names["assembly"] == "03.assembly.unpolished.fa"
    assert inspect.signature(hybrid.run).parameters["extend"].default is None
    assert inspect.signature(polish.run).parameters["extend"].default == 0
    assert hybrid.main(["1", "2", "3"]) == 2  # (still the nine-argument command line: nothing else is taken)


def test_no_device_means_an_error_not_a_fallback(mp, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the stage would run")
    from muchsalsa_amd import _lib, sequences as S
    from muchsalsa_amd.overlap import MsgpuError
    tp, qp = cigarcases.write_inputs("perfect", tmp_path)
    out = os.path.join(str(tmp_path), "out.paf")
    with pytest.raises(mp.MapError) as e:
        mp.run(tp, qp, out, exact=1, cigar=1, extend=300)
    assert e.value.code == _lib.E_NODEVICE and not os.path.exists(out)
    with pytest.raises(MsgpuError) as e:
        with S.SeqStore(0) as st:
            st.extend_ends(0, 0, [], 64)
    assert e.value.code == _lib.E_NODEVICE
