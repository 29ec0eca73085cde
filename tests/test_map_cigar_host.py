"""Rule 10 and the mapper's cigar mode, host side (no GPU): the plain-Python restatement (tests/map_cigar_oracle.py) against
tests/map_oracle.py's banded distance and against the rule's own validity properties on every pair list the GPU file uses, the
tie rule made visible, the chain-level invariants on every mapper case the GPU file uses, the C-ABI, the byte bound of rule 9,
the command line and the error without a device."""
import ctypes as C
import os
import random
import subprocess
import sys

import pytest

import cigarcases
import map_cigar_oracle as co
import map_oracle
import mapcases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


def _check_pair(a, b, band, d, words):
    """rule 10's validity properties for one pair"""
    if d > band:
        assert d == band + 1 and words is None
        return
    assert len(words) == d + 1 and words[d] >> 30 == 0 and all(w >> 30 for w in words[:d])
    assert co.check_script(a, b, band, words) == d  # both lengths consumed, '=' equal, X unequal, d edits


def test_paper_cases():
    assert co.script(b"", b"", 4) == (0, [0])
    assert co.script(b"ACGT", b"ACGT", 0) == (0, [4]) and co.script(b"ACGT", b"ACGA", 0) == (1, None)
    assert co.script(b"A", b"", 4) == (1, [co.D << 30, 0])
    assert co.script(b"", b"ACGT", 4) == (4, [co.I << 30] * 4 + [0]) and co.script(b"", b"ACGT", 3) == (4, None)
    # one base against three: the two insertions come first (a D or X candidate never reaches further on this input)
    assert co.script(b"A", b"CCA", 4) == (2, [co.I << 30, co.I << 30, 1])
    assert co.script(b"CCA", b"A", 4) == (2, [co.D << 30, co.D << 30, 1])
    d, w = co.script(b"ACGT", b"TGCA", 8)
    assert d == map_oracle.banded_distance(b"ACGT", b"TGCA", 8) == 4 and co.check_script(b"ACGT", b"TGCA", 8, w) == 4
    # a homopolymer that loses five bases: the tie rule puts the deletions where X, D, I (in this order) first allow them
    d, w = co.script(b"A" * 30, b"A" * 25, 8)
    assert d == 5 and [x >> 30 for x in w] == [co.D] * 5 + [0] and sum(x & 0x3fffffff for x in w) == 25


def test_random_pairs_against_the_banded_distance():
    """a few thousand pairs of 0..40 bases over 2 and 4 letters, up to 12 edits, bands 1..64, empty and one-sided among them"""
    rng = random.Random(1)
    seen_capped = seen_empty = 0
    for t in range(4000):
        alpha = b"AC" if t % 2 else b"ACGT"
        a = bytes(rng.choice(alpha) for _ in range(rng.randrange(0, 41)))
        b = bytearray(a)
        for _ in range(rng.randrange(0, 13)):
            op, pos = rng.randrange(3), rng.randrange(len(b) + 1)
            if op == 0 and b:
                b[min(pos, len(b) - 1)] = rng.choice(alpha)
            elif op == 1:
                b.insert(pos, rng.choice(alpha))
            elif b:
                del b[min(pos, len(b) - 1)]
        b = b"" if t % 50 == 0 else bytes(b)
        band = rng.choice([1, 2, 3, 5, 8, 16, 64])
        d, w = co.script(a, b, band)
        assert d == map_oracle.banded_distance(a, b, band), (a, b, band)
        _check_pair(a, b, band, d, w)
        seen_capped += w is None
        seen_empty += not a or not b
    assert seen_capped >= 100 and seen_empty >= 80


@pytest.mark.parametrize("name", sorted(cigarcases.pair_lists()))
def test_every_pair_list_of_the_gpu_file(oracle, name):
    """d against the banded distance (tests/map_oracle.py for pairs of at most 400 bases, the compiled full DP or banded DP of the
    C oracle for the longer ones, as tests/test_gpu_edit_distance.py does) and the validity properties, for every pair"""
    pairs, band = cigarcases.pair_lists()[name]
    dist, off, words = cigarcases.expected_scripts(name)
    assert len(dist) == len(pairs) and off[-1] == len(words)
    for i, (a, b) in enumerate(pairs):
        if max(len(a), len(b)) <= 400:
            want = map_oracle.banded_distance(a, b, band)
        elif max(len(a), len(b)) > 5000:
            want = oracle.edit_distance_banded(a, b, band)
        else:
            want = oracle.edit_distance(a, b, band)
        assert dist[i] == want, (name, i)
        w = words[off[i]:off[i + 1]]
        assert len(w) == (dist[i] + 1 if dist[i] <= band else 0)
        _check_pair(a, b, band, dist[i], w if dist[i] <= band else None)


def test_the_pair_lists_meet_the_conditions_of_the_gpu_tests():
    """what keeps the GPU tests from passing on nothing: the sweep has every distance 1..127 and capped pairs, both classes of
    the kernel on either side of their boundary; the slab list has at least 50 pairs of the slab class with at least 50
    different distances; every kind of edit occurs"""
    dist = cigarcases.expected_scripts("sweep")[0]
    assert set(range(0, 128)) <= set(dist) and dist.count(128) >= 2
    assert {co.LDS_MAX_D, co.LDS_MAX_D + 1} <= set(dist)
    slab = [d for d in cigarcases.expected_scripts("slab")[0] if co.LDS_MAX_D < d <= 127]
    assert len(slab) >= 150 and len(set(slab)) >= 50
    kinds = {w >> 30 for w in cigarcases.expected_scripts("random-64")[2]}
    assert kinds == {0, co.X, co.D, co.I}
    d_edges = cigarcases.expected_scripts("edges")[0]
    assert d_edges[-4:] == [cigarcases.EDGE_BAND, cigarcases.EDGE_BAND, cigarcases.EDGE_BAND + 1, cigarcases.EDGE_BAND + 1]


def test_the_tie_rule_is_visible():
    """On the tie input (600 two-letter pairs over short tandem repeats, band 64) the order X, D, I of rule 10 decides: with X and
    D swapped 31 scripts change, with D and I swapped 14 (each must be at least 10), and every variant is still a valid script
    of d edits."""
    pairs = cigarcases.tie_pairs()
    base = [co.script(a, b, cigarcases.TIE_BAND) for a, b in pairs]
    changed = {}
    for order in ((co.D, co.X, co.I), (co.X, co.I, co.D)):
        alt = [co.script(a, b, cigarcases.TIE_BAND, order) for a, b in pairs]
        assert [x[0] for x in alt] == [x[0] for x in base]
        for (a, b), (d, w) in zip(pairs, alt):
            _check_pair(a, b, cigarcases.TIE_BAND, d, w)
        changed[order] = sum(1 for x, y in zip(base, alt) if x != y)
    print(changed)
    assert changed[(co.D, co.X, co.I)] == 31 and changed[(co.X, co.I, co.D)] == 14


def _consumed(runs):
    t = sum(ln for letter, ln in runs if letter in (b"=", b"X", b"D"))
    q = sum(ln for letter, ln in runs if letter in (b"=", b"X", b"I"))
    return t, q


@pytest.mark.parametrize("case", cigarcases.CASES, ids=mapcases.case_id)
def test_chain_invariants(case):
    r = cigarcases.expected(case[0], **case[1])
    exact = r["exact"]
    lines, old_lines = r["paf"].splitlines(), exact["paf"].splitlines()
    assert len(lines) == len(r["chains"]) == len(exact["chains"]) == len(r["runs"]) == len(old_lines)
    for ch, old, runs, capped, line, old_line in zip(r["chains"], exact["chains"], r["runs"], r["capped"], lines, old_lines):
        q, t, s, n, score, nm, qs, qe, ts, te, matches, block = ch
        assert ch[:5] == old[:5] and ch[6:10] == old[6:10]
        assert _consumed(runs) == (te - ts, qe - qs)  # the runs consume the line's two ranges
        col, old_col = line.split(b"\t"), old_line.split(b"\t")
        assert col[:9] == old_col[:9] and col[11:14] == old_col[11:14] and len(col) == 16
        assert sum(ln for letter, ln in runs if letter == b"=") == matches == int(col[9])
        assert sum(ln for _, ln in runs) == block == int(col[10]) and nm == block - matches
        assert col[14] == b"NM:i:%d" % nm and col[15] == b"cg:Z:" + b"".join(b"%d%s" % (ln, letter) for letter, ln in runs)
        assert all(a[0] != b[0] for a, b in zip(runs, runs[1:])) and all(ln > 0 for _, ln in runs)  # merged
        if not capped:
            assert matches >= old[10]
    assert sum(r["capped"]) == r["align"]["pairs_capped"] == exact["capped"]
    assert r["align"]["pairs_d0"] + r["align"]["pairs_lds"] + r["align"]["pairs_slab"] + r["align"]["pairs_capped"] == exact["pairs"]
    assert r["align"]["runs"] == sum(len(x) for x in r["runs"])


def test_the_cases_meet_the_conditions_of_the_gpu_tests():
    clean, clean8 = cigarcases.expected("clean"), cigarcases.expected("clean", band=8)
    assert clean["align"]["pairs_capped"] == 0 and sum(clean["capped"]) == 0
    assert any(new[10] > old[10] for new, old in zip(clean["chains"], clean["exact"]["chains"]))
    assert all(new[10] >= old[10] for new, old in zip(clean["chains"], clean["exact"]["chains"]))
    assert clean8["align"]["pairs_capped"] >= 1
    # a capped segment shows as a deletion or an insertion longer than the band, which no script within the band holds
    assert any(letter in (b"D", b"I") and ln > 8 for runs in clean8["runs"] for letter, ln in runs)
    assert not any(letter in (b"D", b"I") and ln > 64 for runs in clean["runs"] for letter, ln in runs)
    main = cigarcases.expected("main")
    strands = [c[2] for c in main["chains"]]
    assert strands.count(0) >= 10 and strands.count(1) >= 10
    assert main["align"]["x_columns"] and main["align"]["i_columns"] and main["align"]["d_columns"]
    slab = cigarcases.expected("slab_link")
    assert len(slab["chains"]) == 1 and slab["align"]["pairs_slab"] == 1 and slab["align"]["max_d"] == 40
    assert slab["cigars"][0].count("X") == 40
    assert cigarcases.expected("beyond_band")["align"]["pairs_capped"] == 1
    assert cigarcases.expected("one_sided")["cigars"][0].count("I") == 1 and "D" not in cigarcases.expected("one_sided")["cigars"][0]
    assert cigarcases.expected("empty_queries")["paf"] == b""
    perfect = cigarcases.expected("perfect")
    assert cigarcases.expected("reverse")["cigars"] == perfect["cigars"] == ["%d=" % perfect["chains"][0][11]]


def test_the_tiled_cigar_paf_passes_the_overlap_loader(mp, tmp_path):
    """at least 100 lines of the tiled workload's cigar PAF pass msgpu_parse_paf's default thresholds (a host call), and at least
    as many as of its exact PAF"""
    from muchsalsa_amd import overlap
    r = cigarcases.expected("tiled")
    n = {}
    for key, text in (("cigar", r["paf"]), ("exact", r["exact"]["paf"])):
        path = os.path.join(str(tmp_path), key + ".paf")
        with open(path, "wb") as f:
            f.write(text)
        n[key] = len(overlap.parse_paf(path).rows)
    print(n)
    assert n["cigar"] >= 100 and n["cigar"] >= n["exact"]


def test_abi(mp):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(ROOT, "include", "msgpu.h")).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for n in ("msgpu_edit_script", "msgpu_map_result_cigars", "msgpu_map_result_align_stats"):
        assert hasattr(L, n) and n in bound and n + "(" in header, n
    assert C.sizeof(_lib.MapParams) == 48 and C.sizeof(_lib.MapChain) == 48 and C.sizeof(_lib.MapStats) == 424
    assert C.sizeof(_lib.MapBatch) == 64 and C.sizeof(_lib.MapAlignStats) == 104
    assert "int32_t  cigar;" in header and _lib.MapParams.cigar.offset == 44
    prm = _lib.MapParams()
    L.msgpu_map_default_params(C.byref(prm))
    assert prm.cigar == 0 and prm.exact == 0
    assert "cigar" not in mp.DEFAULTS and mp.DEFAULTS == map_oracle.PARAMS
    # null arguments are rejected before anything is touched
    n = C.c_uint64()
    assert L.msgpu_map_result_cigars(None, None, None, C.byref(n)) == _lib.E_ARG
    assert L.msgpu_map_result_align_stats(None, None) == _lib.E_ARG
    assert L.msgpu_edit_script(None, None, None, None, 0, 64, None, None, None, 0, C.byref(n)) == _lib.E_ARG


# msgpu_map_batch_bytes of the commit before cigar mode: (exact, anchors, query bases) -> bytes, the same at every band
PARENT_BYTES = {(0, 0, 0): 1065472, (0, 1, 1000): 1065689, (0, 17, 0): 1069161, (0, 1000, 1000000): 1282472,
                (0, 230181, 1000): 51014749, (1, 0, 0): 1065472, (1, 0, 1000): 1067472, (1, 1, 0): 1065721,
                (1, 17, 1000): 1071705, (1, 1000, 1000000): 3314472, (1, 230181, 0): 58380541, (1, 230181, 1000000): 60380541}


def test_batch_bytes(mp, monkeypatch):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    monkeypatch.delenv("MSGPU_ALIGN_SLOTS", raising=False)

    def nbytes(a, b, **kw):
        prm = _lib.MapParams()
        L.msgpu_map_default_params(C.byref(prm))
        for key, v in kw.items():
            setattr(prm, key, v)
        return int(L.msgpu_map_batch_bytes(C.byref(prm), a, b))

    for (exact, a, b), want in PARENT_BYTES.items():
        for band in (1, 64, 127):
            assert nbytes(a, b, exact=exact, band=band) == want, (exact, a, b, band)
            assert nbytes(a, b, exact=exact, band=band, cigar=0) == want
    sizes = [0, 1, 17, 1000, 230181, (1 << 31) - 1]
    for band in (1, 8, 31, 32, 64, 127):
        slab = 1024 * (band + 1) ** 2 * 4 if band > 31 else 0  # (up to 31 edits a table lies in LDS: no slab class, no slab)
        for a in sizes:
            for b in (0, 1000, 1 << 20):
                with_cigar, without = nbytes(a, b, exact=1, cigar=1, band=band), nbytes(a, b, exact=1, band=band)
                # the slab (1024 slots of (band + 1)^2 words) and, per anchor, band + 1 words of script and 40 bytes beside them
                assert with_cigar >= without + slab + a * (4 * (band + 1) + 40)
                assert with_cigar <= without + slab + a * (4 * (band + 1) + 40) + 4096
        for a, a2 in zip(sizes, sizes[1:]):
            assert nbytes(a, 1000, exact=1, cigar=1, band=band) < nbytes(a2, 1000, exact=1, cigar=1, band=band)
    for lo, hi in zip((1, 8, 31, 32, 64), (8, 31, 32, 64, 127)):
        for a in sizes:
            one, other = nbytes(a, 1000, exact=1, cigar=1, band=lo), nbytes(a, 1000, exact=1, cigar=1, band=hi)
            assert one < other or (a == 0 and hi <= 31 and one == other)  # (without anchors and without a slab nothing grows)
    # MSGPU_ALIGN_SLOTS lowers the slab, and with it the bound
    monkeypatch.setenv("MSGPU_ALIGN_SLOTS", "3")
    assert nbytes(10, 0, exact=1, cigar=1) <= nbytes(10, 0, exact=1) + 3 * 65 * 65 * 4 + 10 * (4 * 65 + 40) + 4096
    # the guard against overflow: cigar mode's bytes per anchor are below 2^10, so 2^50 anchors and more are "too many"
    monkeypatch.delenv("MSGPU_ALIGN_SLOTS")
    top = (1 << 64) - 1
    assert nbytes(1 << 50, 0, exact=1, cigar=1, band=127) == top and nbytes((1 << 50) - 1, 0, exact=1, cigar=1, band=127) < top
    assert nbytes((1 << 50) - 1, (1 << 62) - 1, exact=1, cigar=1, band=127) < top


def test_command_line_takes_cigar(mp, tmp_path, monkeypatch, capsys):
    """--cigar implies --exact and reaches run() as the keyword; bad arguments still end in the usage text"""
    seen = []
    monkeypatch.setattr(mp, "run", lambda *a, **kw: seen.append((a, kw)) or {})
    p = [str(tmp_path / n) for n in ("t.fa", "q.fa", "out.paf")]
    assert mp.main(p + ["--cigar"]) == 0 and seen[-1][1]["cigar"] == 1 and seen[-1][1]["exact"] == 1
    assert mp.main(p + ["--cigar", "--exact", "--band", "8"]) == 0 and seen[-1][1]["cigar"] == 1 and seen[-1][1]["band"] == 8
    assert mp.main(p + ["--exact"]) == 0 and seen[-1][1]["cigar"] == 0 and seen[-1][1]["exact"] == 1
    assert mp.main(p) == 0 and seen[-1][1]["cigar"] == 0 and "exact" not in seen[-1][1]
    capsys.readouterr()
    assert mp.main(p + ["--cigar", "1"]) == 2
    assert "--cigar" in capsys.readouterr().err
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "muchsalsa_amd.mapper", p[0], p[1], "--cigar"], cwd=ROOT, env=env, capture_output=True,
                         timeout=300)
    assert out.returncode == 2 and b"[--cigar]" in out.stderr


def test_unknown_keywords_are_still_rejected(mp, tmp_path):
    tp, qp = mapcases.write_inputs("perfect", tmp_path)
    with pytest.raises(TypeError):
        mp.run(tp, qp, os.path.join(str(tmp_path), "x.paf"), cigars=1)


def test_no_device_means_an_error_not_a_fallback(mp, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the stage would run")
    from muchsalsa_amd import _lib
    tp, qp = mapcases.write_inputs("perfect", tmp_path)
    out = os.path.join(str(tmp_path), "out.paf")
    with pytest.raises(mp.MapError) as e:
        mp.run(tp, qp, out, exact=1, cigar=1)
    assert e.value.code == _lib.E_NODEVICE and not os.path.exists(out)
    from muchsalsa_amd import sequences as S
    from muchsalsa_amd.overlap import MsgpuError
    with pytest.raises(MsgpuError) as e:  # (the store of the primitive: there is none to call edit_script on)
        with S.SeqStore(0) as st:
            st.edit_script(0, 0, [], 64)
    assert e.value.code == _lib.E_NODEVICE
