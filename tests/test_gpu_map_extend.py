"""Rule 11 (the mapper's end extension) on the GPU: msgpu_extend_ends on hand-made and random flank pairs, forward and
reversed, and ``mapper.run(..., cigar=1, extend=E)`` by files, through an index, in batches, through the polisher, the
pipeline's driver and the command line -- end cells, words, PAF bytes, chain tables, run tables and counts against the
plain-Python restatement (tests/map_extend_oracle.py), without any tolerance.  No test provokes a device fault.  Every test runs
under its own time limit."""
import ctypes as C
import faulthandler
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarcases
import extendcases
import mapcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = 600  # seconds per test


@pytest.fixture(scope="module")
def mp():
    import __graft_entry__ as g
    g.build()
    from muchsalsa_amd import mapper
    return mapper


@pytest.fixture(autouse=True)
def time_limit(mp):
    faulthandler.dump_traceback_later(LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# ---- 1. msgpu_extend_ends

def _device(pairs, reverse):
    import torch
    from muchsalsa_amd._lib import ALIGN_PAIR_DTYPE
    a, b, desc = extendcases.layout(pairs, reverse)
    da = torch.frombuffer(bytearray(a or b"\0"), dtype=torch.uint8).cuda()  # (nothing behind the last flank's last byte)
    db = torch.frombuffer(bytearray(b or b"\0"), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return da, db, np.array(desc, dtype=ALIGN_PAIR_DTYPE)


def _extend(pairs, band, reverse):
    from muchsalsa_amd import sequences as S
    da, db, desc = _device(pairs, reverse)
    with S.SeqStore(0) as st:
        ends, off, words = st.extend_ends(da.data_ptr(), db.data_ptr(), desc, band, reverse=reverse)
    return [tuple(int(x) for x in e) for e in ends], [int(x) for x in off], [int(x) for x in words]


def _compare(pairs, got, want, what):
    ends, off, words = got
    if ends != want[0]:
        bad = next(i for i in range(len(ends)) if ends[i] != want[0][i])
        raise AssertionError("%s: pair %d (%d, %d bytes): end %r != %r" % (what, bad, len(pairs[bad][0]), len(pairs[bad][1]), ends[bad],
                                                                            want[0][bad]))
    assert off == want[1]
    if words != want[2]:  # (name the first pair that differs)
        bad = next(i for i in range(len(ends)) if words[off[i]:off[i + 1]] != want[2][off[i]:off[i + 1]])
        raise AssertionError("%s: pair %d: %r != %r" % (what, bad, words[off[bad]:off[bad + 1]], want[2][off[bad]:off[bad + 1]]))


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("band", extendcases.BANDS)
def test_hand_made_pairs(band, reverse):
    """identical flanks at match_run8's widths and the wide slide's stride, n != m, one edit of each kind at byte 0, in the middle
    and as the last byte, indels either side of the lane seam (band 127), an end cell in row band and one that would need row
    band + 1, random flanks, good bytes and then random ones; the first flank starts at buffer byte 0 and the last one ends at
    the buffer's last byte.  n_inconsistent == 0: an inconsistent table is MSGPU_E_STATE, which extend_ends raises."""
    pairs = extendcases.hand_pairs(band)
    _compare(pairs, _extend(pairs, band, reverse), extendcases.expected_pairs(band), "band %d" % band)


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
@pytest.mark.parametrize("which", [0, 1])
def test_random_pairs(which, reverse):
    """2,000 seeded pairs at 0-20 % edits, some cut short on one side: 1,500 in the LDS class, 500 in the slab class"""
    pairs, band = extendcases.random_pairs(which)
    _compare(pairs, _extend(pairs, band, reverse), extendcases.expected_pairs(("random", which)), "random %d" % which)


CHILD = """
import json, sys
sys.path.insert(0, %r)
import extendcases
import test_gpu_map_extend as T
pairs, band = extendcases.random_pairs(1)
print(json.dumps(T._extend(pairs, band, bool(%d))))
"""


@pytest.mark.parametrize("poison", [0, 1])
@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "reversed"])
def test_three_slots_serve_the_whole_slab_class(reverse, poison):
    """MSGPU_ALIGN_SLOTS=3 in a fresh child process (up to 1,024 pairs every pair has a slot of its own otherwise): the 500
    pairs of the slab class go through three tables, so every slot is reused many times; once more with the buffers poisoned.
    The end cells and the words do not depend on the number of slots"""
    env = dict(os.environ, PYTHONPATH=ROOT, MSGPU_ALIGN_SLOTS="3")
    if poison:
        env["MSGPU_POISON"] = "1"
    run = subprocess.run([sys.executable, "-c", CHILD % (os.path.join(ROOT, "tests"), reverse)], cwd=ROOT, env=env, capture_output=True,
                         timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    ends, off, words = json.loads(run.stdout.decode().strip().splitlines()[-1])
    pairs, band = extendcases.random_pairs(1)
    assert band > 31 and len(pairs) > 3
    _compare(pairs, ([tuple(e) for e in ends], off, words), extendcases.expected_pairs(("random", 1)), "three slots")


def test_no_pairs():
    from muchsalsa_amd import sequences as S
    with S.SeqStore(0) as st:
        ends, off, words = st.extend_ends(0, 0, [], 64)
    assert len(ends) == 0 and list(off) == [0] and len(words) == 0


def test_a_small_capacity_is_an_error_that_says_how_much_and_the_next_call_is_right():
    from muchsalsa_amd import _lib, sequences as S
    band = 8
    pairs, want = extendcases.hand_pairs(band), extendcases.expected_pairs(band)
    da, db, desc = _device(pairs, False)
    with S.SeqStore(0) as st:
        ends = np.zeros(len(pairs), dtype=_lib.EXT_END_DTYPE)
        off = np.zeros(len(pairs) + 1, dtype="<u8")
        words = np.full(len(want[2]), 0xdeadbeef, dtype="<u4")
        need = C.c_uint64()
        call = lambda cap, flags=0: st._L.msgpu_extend_ends(st._h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), desc.ctypes.data,
                                                            len(pairs), band, flags, ends.ctypes.data, off.ctypes.data, words.ctypes.data,
                                                            cap, C.byref(need))
        assert call(len(want[2]) - 1) == _lib.E_ARG
        assert need.value == len(want[2]) and [int(x) for x in off] == want[1] and [tuple(int(x) for x in e) for e in ends] == want[0]
        assert all(w == 0xdeadbeef for w in words)  # nothing was written
        assert b"words" in st._L.msgpu_seq_last_error(st._h)
        assert call(len(want[2])) == _lib.OK
        assert need.value == len(want[2]) and [int(w) for w in words] == want[2]
        assert call(len(want[2]), flags=2) == _lib.E_ARG and call(len(want[2]), flags=0) == _lib.OK  # (an unknown flag)
        got = st.extend_ends(da.data_ptr(), db.data_ptr(), desc, band)  # the Python wrapper grows its buffer by itself
        assert [int(w) for w in got[2]] == want[2]


# ---- 2. the mapper

STATS = ("n_ends", "n_ends_extended", "n_ends_at_sequence_end", "t_bases", "q_bases", "x_columns", "i_columns", "d_columns", "max_e",
         "rows", "n_inconsistent", "extend")


def _stage(mp, d, name, params, extend, cigar=1, **how):
    tp, qp = extendcases.write_inputs(name, d)
    out = os.path.join(str(d), "out.paf")
    tables = {}
    if "index" in how:
        tp = None
    res = mp.run(tp, qp, out, tables=tables, cigar=cigar, extend=extend, **dict(extendcases.params_of(name, **params), **how))
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"]
    return res, tables, text


def _same(res, tb, text, want):
    assert res["cigar"] == 1 and res["lost_publications"] == 0
    assert len(text) == len(want["paf"]) and text == want["paf"]
    assert res["chains"] == len(want["chains"]) and tb["chains"] == want["chains"]
    assert tb["runs"] == want["packed"] and tb["cigars"] == want["cigars"]
    assert tb["ext"] == want["ext"]
    assert {key: res["extend"][key] for key in STATS} == want["stats"]
    assert res["align"]["n_runs"] == want["n_runs"] and res["align"]["n_inconsistent"] == 0
    # rule 10's counts are those of the run without the extension
    assert {k: res["align"][k] for k in ("x_columns", "i_columns", "d_columns", "script_words", "max_d")} == {
        k: want["cigar"]["align"][k] for k in ("x_columns", "i_columns", "d_columns", "script_words", "max_d")}
    assert res["bytes_out"] == len(text) and res["extend"]["seconds"]["extend"] >= 0


@pytest.mark.parametrize("case", extendcases.CASES, ids=lambda c: "%s-%d" % (c[0], c[2]))
def test_against_the_restatement(mp, tmp_path, case):
    """clean (contained queries on both strands against noisy reads) at E = 1, 16, 300 and one larger than any record; chains
    whose extension stops at target byte 0 and at the target's last byte; the error-free hand cases"""
    name, params, extend = case
    want = extendcases.expected(name, extend, **params)
    res, tb, text = _stage(mp, tmp_path, name, params, extend)
    print("%s E = %d: %d chains, %r" % (name, extend, res["chains"], res["extend"]))
    _same(res, tb, text, want)


def test_through_an_index_and_back_to_zero(mp, tmp_path):
    """on one index: extend = 300, then 16, then 0 (the bytes of a run on a fresh context: the setter is sticky per run and it
    resets), then extend without cigar (MSGPU_E_ARG naming both) and a good run behind it"""
    from muchsalsa_amd import _lib
    tp, _ = extendcases.write_inputs("clean", tmp_path)
    plain = cigarcases.expected("clean")
    with mp.Index(tp) as ix:
        for extend in (300, 16):
            _same(*_stage(mp, tmp_path, "clean", {}, extend, index=ix), extendcases.expected("clean", extend))
        res, tb, text = _stage(mp, tmp_path, "clean", {}, 0, index=ix)
        assert text == plain["paf"] and tb["chains"] == plain["chains"] and tb["runs"] == plain["packed"]
        assert "extend" not in res and "ext" not in tb
        for kw in (dict(cigar=0), dict(cigar=0, exact=0)):
            with pytest.raises(mp.MapError) as e:
                _stage(mp, tmp_path, "clean", {}, 300, index=ix, **kw)
            assert e.value.code == _lib.E_ARG and "extend" in str(e.value) and "cigar" in str(e.value)
        _same(*_stage(mp, tmp_path, "clean", {}, 300, index=ix), extendcases.expected("clean", 300))
    fresh = _stage(mp, tmp_path, "clean", {}, 0)
    assert fresh[2] == text and fresh[1] == tb


def test_a_value_above_the_limit_keeps_the_previous_one(mp, tmp_path):
    from muchsalsa_amd import _lib
    L = _lib.lib()
    tp, qp = extendcases.write_inputs("ends", tmp_path)
    want = extendcases.expected("ends", 16)
    with mp.Index(tp) as ix:
        assert L.msgpu_map_set_extension(ix.stage.ctx, 16) == _lib.OK
        assert L.msgpu_map_set_extension(ix.stage.ctx, 65536) == _lib.E_ARG
        assert b"65536" in L.msgpu_map_last_error(ix.stage.ctx)
        prm = mp._params(dict(mp.DEFAULTS, exact=1, cigar=1))
        with ix.stage.run(C.byref(prm), ix.handle, os.fsencode(qp), 0, 0, fn="run_index") as res:  # (no setter in between)
            from muchsalsa_amd._stage import text_view
            assert bytes(text_view(L.msgpu_map_result_text, res)) == want["paf"]
            xst = _lib.MapExtStats()
            assert L.msgpu_map_result_ext_stats(res, C.byref(xst)) == _lib.OK and xst.extend == 16
        assert L.msgpu_map_set_extension(ix.stage.ctx, 65535) == _lib.OK and L.msgpu_map_set_extension(ix.stage.ctx, 0) == _lib.OK
    with pytest.raises(mp.MapError) as e:
        _stage(mp, tmp_path, "ends", {}, 65536)
    assert e.value.code == _lib.E_ARG and "65536" in str(e.value)


def test_every_query_record_a_batch_of_its_own(mp, tmp_path):
    """the smallest budget at which every query record fits: bytes_peak <= bytes_bound == msgpu_map_batch_bytes_ext(...)"""
    import test_mapper_batches_host as host
    from muchsalsa_amd import _lib
    name, extend = "clean", 300
    a, b = host.record_counts(name, exact=1)
    prm = _lib.MapParams()
    _lib.lib().msgpu_map_default_params(C.byref(prm))
    prm.exact = prm.cigar = 1
    nbytes = lambda x, y: int(_lib.lib().msgpu_map_batch_bytes_ext(C.byref(prm), extend, x, y))
    one = max(nbytes(x, y) for x, y in zip(a, b))
    res, tb, text = _stage(mp, tmp_path, name, {}, extend, budget_mb=one / 2.0 ** 20)
    _same(res, tb, text, extendcases.expected(name, extend))
    bt = res["batches"]
    print("budget %d: %d batches, peaks %r" % (res["budget_bytes"], len(bt), [(x["bytes_peak"], x["bytes_bound"]) for x in bt][:8]))
    assert len(bt) >= 3
    for x in bt:
        assert x["bytes_bound"] == nbytes(x["n_anchors"], x["n_query_bases"])
        assert x["bytes_peak"] <= x["bytes_bound"] <= res["budget_bytes"]
    whole = _stage(mp, tmp_path, name, {}, extend)[0]["batches"]
    assert len(whole) == 1 and whole[0]["bytes_peak"] <= whole[0]["bytes_bound"] == nbytes(sum(a), sum(b))


# ---- 3. the polisher, the driver, the command line

def test_the_polisher_votes_beyond_the_outermost_seeds(mp, tmp_path):
    """polish.run(..., extend=300) on ``planted`` against pl_oracle fed with extend_run's tables, byte for byte"""
    import map_oracle
    import map_extend_oracle
    import pl_oracle
    import plcases
    from muchsalsa_amd import polish as pl
    wl = plcases.workload("planted")
    draft, reads = map_oracle.parse(wl["draft"], False), map_oracle.parse(wl["reads"], False)
    mapped = map_extend_oracle.extend_run(draft, reads, 300, cigar_result=plcases.expected_workload("planted")[1])
    want = pl_oracle.run(draft, reads, mapped["chains"], mapped["packed"])
    dp, rp = plcases.write_workload("planted", tmp_path)
    out, paf = os.path.join(str(tmp_path), "out.fa"), os.path.join(str(tmp_path), "kept.paf")
    tb = {}
    res = pl.run(dp, rp, out, tables=tb, paf=paf, extend=300)
    with open(paf, "rb") as h:
        assert h.read() == mapped["paf"]
    with open(out, "rb") as h:
        text = h.read()
    assert len(text) == len(want["text"]) and text == want["text"] == tb["text"] and tb["records"] == want["records"]
    assert {k: res[pl._strip(k)] for k in pl_oracle.COUNTS} == {k: want[k] for k in pl_oracle.COUNTS}
    before = plcases.expected_workload("planted")[0]
    print("positions kept verbatim: %d without the extension, %d with it" % (before["pos_verbatim"], want["pos_verbatim"]))


def test_the_driver_passes_extend_on(mp, tmp_path):
    """hybrid.run(extend=300) on the hybrid test's workload: every file written before step 9's PAF is byte-equal to the default
    run's, and that PAF is mapper.run's with the same arguments"""
    import hybridcases
    from muchsalsa_amd import hybrid
    (tmp_path / "in").mkdir()
    inputs = hybridcases.write_inputs(tmp_path / "in")
    res = {}
    for key, kw in (("default", {}), ("extend", dict(extend=300))):
        res[key] = hybrid.run(hybridcases.K_FILTER, hybridcases.K_ASSEMBLY, hybridcases.NAME, inputs[0], inputs[1], inputs[2],
                              str(tmp_path / key), **kw)
    assert res["extend"]["map_exact"]["cigar"] == 1 and res["extend"]["map_exact"]["extend"]["extend"] == 300
    assert "extend" not in res["default"]["map_exact"] and res["default"]["map_exact"]["cigar"] == 0
    names = hybrid.output_names(hybridcases.NAME, inputs[2])
    assert set(res["extend"]["files"]) == set(names)
    for key in ("report", "unitigs", "unitigs_cut", "unitigs_paf", "corrected", "corrected_paf", "ava_paf", "scrubbed"):
        a, b = (open(res[k]["files"][key], "rb").read() for k in ("default", "extend"))
        assert hashlib.sha256(a).digest() == hashlib.sha256(b).digest() and len(a) > 0, key
    files = res["extend"]["files"]
    alone = os.path.join(str(tmp_path), "alone.paf")
    got = mp.run(files["scrubbed"], files["corrected"], alone, exact=1, cigar=1, extend=300)
    with open(alone, "rb") as a, open(files["exact_paf"], "rb") as b:
        text = a.read()
        assert text == b.read() and b"cg:Z:" in text
    assert got["extend"]["n_ends"] == 2 * got["chains"] >= 2 and got["extend"]["n_ends_extended"] >= 1
    assert res["extend"]["assembly"]["contigs"] >= 1 and os.path.getsize(files["assembly"]) > 0


def test_the_command_line_in_a_fresh_process(mp, tmp_path):
    tp, qp = extendcases.write_inputs("ends", tmp_path)
    out = os.path.join(str(tmp_path), "cli.paf")
    env = dict(os.environ, PYTHONPATH=ROOT)
    run = subprocess.run([sys.executable, "-m", "muchsalsa_amd.mapper", tp, qp, out, "--extend", "300"], cwd=ROOT, env=env,
                         capture_output=True, timeout=LIMIT)
    assert run.returncode == 0, run.stderr[-2000:]
    line = json.loads(run.stdout.decode().strip().splitlines()[-1])
    want = extendcases.expected("ends", 300)
    with open(out, "rb") as h:
        assert h.read() == want["paf"]
    assert line["cigar"] == 1 and line["params"]["exact"] == 1 and {k: line["extend"][k] for k in STATS} == want["stats"]
    assert "extend" in line["extend"]["seconds"]
