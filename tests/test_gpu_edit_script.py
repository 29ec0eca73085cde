"""msgpu_edit_script on the GPU: dist, off and words equal to the plain-Python restatement of rule 10
(tests/map_cigar_oracle.py), word for word, on the pair lists of tests/cigarcases.py (tests/test_map_cigar_host.py checks the
restatement on every one of them), and dist equal to msgpu_edit_distance's.  No test provokes a device fault."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cigarcases

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device_pairs(pairs_ab):
    import torch
    from muchsalsa_amd._lib import ALIGN_PAIR_DTYPE
    a = b"".join(p[0] for p in pairs_ab)
    b = b"".join(p[1] for p in pairs_ab)
    desc = np.zeros(len(pairs_ab), dtype=ALIGN_PAIR_DTYPE)
    ao = bo = 0
    for i, (x, y) in enumerate(pairs_ab):
        desc[i] = (ao, bo, len(x), len(y))
        ao += len(x)
        bo += len(y)
    da = torch.frombuffer(bytearray(a + b"\0"), dtype=torch.uint8).cuda()
    db = torch.frombuffer(bytearray(b + b"\0"), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return da, db, desc


def _run(name):
    """-> msgpu_edit_script's (dist, off, words) and msgpu_edit_distance's distances for a pair list, as lists"""
    from muchsalsa_amd import sequences as S
    pairs, band = cigarcases.pair_lists()[name]
    da, db, desc = _device_pairs(pairs)
    with S.SeqStore(0) as st:
        dist, off, words = st.edit_script(da.data_ptr(), db.data_ptr(), desc, band)
        meter = st.edit_distance(da.data_ptr(), db.data_ptr(), desc, band)
    return [int(x) for x in dist], [int(x) for x in off], [int(x) for x in words], [int(x) for x in meter]


def _compare(name, got):
    dist, off, words, meter = got
    want = cigarcases.expected_scripts(name)
    assert dist == want[0] == meter
    assert off == want[1]
    if words != want[2]:  # (name the first pair that differs)
        bad = next(i for i in range(len(dist)) if words[off[i]:off[i + 1]] != want[2][off[i]:off[i + 1]])
        raise AssertionError("%s: pair %d (d = %d): %r != %r" % (name, bad, dist[bad], words[off[bad]:off[bad + 1]],
                                                                want[2][off[bad]:off[bad + 1]]))


@pytest.mark.parametrize("name", sorted(cigarcases.pair_lists()))
def test_words_match_the_restatement(name):
    """random pairs at bands 127, 64, 8, 1, 0; single edits around the steps of the slides, 40 kb near-identical pairs and the
    pair that ends with the device buffer; 30 kb pairs; the sweep d = 0..129 across the two classes, the band and band + 1; the
    tie input; the matrix-edge cases; the slab class's list"""
    _compare(name, _run(name))


def test_no_pairs():
    from muchsalsa_amd import sequences as S
    with S.SeqStore(0) as st:
        dist, off, words = st.edit_script(0, 0, [], 64)
    assert len(dist) == 0 and list(off) == [0] and len(words) == 0


def test_a_small_capacity_is_an_error_that_says_how_much_and_the_next_call_is_right():
    import ctypes as C
    from muchsalsa_amd import _lib, sequences as S
    name = "edges"
    pairs, band = cigarcases.pair_lists()[name]
    want = cigarcases.expected_scripts(name)
    da, db, desc = _device_pairs(pairs)
    with S.SeqStore(0) as st:
        dist = np.zeros(len(pairs), dtype="<u4")
        off = np.zeros(len(pairs) + 1, dtype="<u8")
        words = np.full(len(want[2]), 0xdeadbeef, dtype="<u4")
        need = C.c_uint64()
        call = lambda cap: st._L.msgpu_edit_script(st._h, C.c_void_p(da.data_ptr()), C.c_void_p(db.data_ptr()), desc.ctypes.data,
                                                   len(pairs), band, dist.ctypes.data, off.ctypes.data, words.ctypes.data, cap,
                                                   C.byref(need))
        assert call(len(want[2]) - 1) == _lib.E_ARG
        assert need.value == len(want[2]) and list(dist) == want[0] and list(off) == want[1]
        assert all(w == 0xdeadbeef for w in words)  # nothing was written
        assert b"words" in st._L.msgpu_seq_last_error(st._h)
        assert call(len(want[2])) == _lib.OK
        assert need.value == len(want[2]) and [int(w) for w in words] == want[2]
        # the Python wrapper grows its buffer by itself
        got = st.edit_script(da.data_ptr(), db.data_ptr(), desc, band)
        assert [int(w) for w in got[2]] == want[2]


CHILD = """
import json, sys
sys.path.insert(0, %r)
import test_gpu_edit_script as T
print(json.dumps(T._run("slab")))
"""


@pytest.mark.parametrize("poison", [0, 1])
def test_three_slots_serve_the_whole_slab_class(poison):
    """MSGPU_ALIGN_SLOTS=3 in a fresh child process (the variable is read per call, but a fresh process also starts on fresh
    device memory): 180 pairs of the slab class with 60 different distances go through three tables, so every slot is reused
    many times; once more with the buffers poisoned"""
    env = dict(os.environ, PYTHONPATH=ROOT, MSGPU_ALIGN_SLOTS="3")
    if poison:
        env["MSGPU_POISON"] = "1"
    run = subprocess.run([sys.executable, "-c", CHILD % os.path.join(ROOT, "tests")], cwd=ROOT, env=env, capture_output=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]
    _compare("slab", json.loads(run.stdout.decode().strip().splitlines()[-1]))
