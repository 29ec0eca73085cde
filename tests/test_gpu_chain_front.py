"""The front of an edge in the chain kernels: k_emit_edges leaves one 32-byte descriptor per edge of at most 64 EdgeMatches
(edge, reads, count, first EdgeMatch, first candidate) where the size-sorted list used to hold the edge's index; k_chain
takes descriptor blockIdx.x with one scalar load, the groups of k_chain_sub_all / k_chain_sub<W> theirs with two 16-byte
loads, and a group past the end of its class takes descriptor 0 with n = 0.  k_chain_big and the mode without size classes
still start from edges[e] / edge_cand[e].  The inputs aim at what that can get wrong: a class of one descriptor, classes
that are empty (the stretches of the three classes lie back to back), class lengths one short of, equal to and one past a
workgroup's worth of groups, groups of both strands in one wavefront, a launch per class, and the largest ranks a candidate
can carry on either index path.  A candidate is ONE word, j | q << 16 (both row ranks); a job with a read of more than 65,535
rows keeps two arrays instead (the WIDE form of the kernels; MSGPU_CAND_WIDE=1 forces it).  Every GPU case compares all four
tables with the C oracle bit for bit."""
import numpy as np
import pytest

from helpers import assert_tables_equal
from test_golden_hand import row
from test_gpu_chain_classes import BOUNDS, STEP, _check, _rows, _run
from muchsalsa_amd.synth import ROW_DTYPE

gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("n", [1, 8, 9, 16, 17, 32, 33, 64])
def test_one_edge_alone_in_its_class(oracle, n):
    """the only descriptor of the list: the groups beside it in its wavefront take descriptor 0 with n = 0 (the widths 8, 16
    and 32), and the two other sub-wavefront classes and k_chain (or all three sub-wavefront classes) have nothing"""
    want = _check(oracle, _rows([(n, "mixed")], 300 + n), [n], "alone/%d" % n)
    assert len(want["edges"]) == 1 and len(want["orders"]) >= 1


@gpu
def test_big_edge_alone(oracle):
    """65 EdgeMatches: k_chain_big, from edges[e] / edge_cand[e], beside four empty classes (no descriptor is written)"""
    _check(oracle, _rows([(65, "mixed")], 365), [65], "big alone")


@gpu
@pytest.mark.parametrize("sizes", [(1, 2, 5, 8), (33, 40, 57, 64)], ids=["le8", "33to64"])
def test_empty_classes(oracle, sizes):
    """every edge in ONE class, the first or the last stretch of the descriptor list; the other three are empty"""
    specs = [(n, ("mixed", "both", "clean")[i % 3]) for i, n in enumerate(sizes * 3)]
    _check(oracle, _rows(specs, 41), [n for n, _ in specs], "only %s" % (sizes,))


@gpu
@pytest.mark.parametrize("extra", [-1, 0, 1])
@pytest.mark.parametrize("G,n", [(2, 20), (4, 12), (8, 5)])
def test_class_length_around_a_workgroup(oracle, G, n, extra):
    """4 G - 1, 4 G and 4 G + 1 edges of one width (G groups in each of a workgroup's four wavefronts): the last wavefront one
    group short, the workgroup exactly full, and a second workgroup with one group"""
    specs = [(n, "mixed")] * (4 * G + extra)
    _check(oracle, _rows(specs, 500 + 10 * G + extra), [n] * len(specs), "G=%d%+d" % (G, extra))


def _mixed_directions():
    kinds = ("clean", "both", "mixed", "both")
    return [(n, kinds[(i + r) % 4]) for r in range(3) for i, n in enumerate((3, 7, 8, 11, 16, 19, 30, 32, 34, 64))]


@gpu
@pytest.mark.parametrize("serial", [False, True], ids=["one_launch", "serial"])
def test_mixed_directions_in_one_wavefront(oracle, monkeypatch, serial):
    """groups of one strand beside groups of both in every width; also with a launch per class (MSGPU_CHAIN_SERIAL: the
    same descriptor stretches, through k_chain_sub<W>)"""
    if serial:
        monkeypatch.setenv("MSGPU_CHAIN_SERIAL", "1")
    specs = _mixed_directions()
    want = _check(oracle, _rows(specs, 77), [n for n, _ in specs], "directions, serial=%s" % serial)
    flags = want["orders"]["flags"].astype(np.int64)
    assert (flags & 4).any() and not (flags & 4).all()  # paths of both directions


def _rank_rows(n_a, n_b, shared):
    """read 0 with n_a rows and read 1 with n_b: anchors of their own, then `shared` common ones behind them on both reads, so
    the edge's candidates carry the LAST ranks of both row lists (j = n_a - shared .., q = n_b - shared ..).  Rows in (anchor,
    line) order, as the bin path wants them."""
    L = 2000 + STEP * max(n_a, n_b)
    out, line, anchor = [], 0, 0
    for read, n in ((0, n_a), (1, n_b)):
        for j in range(n - shared):
            out.append(row(anchor, read, L, 0, 599, 500 + STEP * j, 500 + STEP * j + 599, 520, line, True))
            anchor, line = anchor + 1, line + 1
    for k in range(shared):
        for read, n in ((0, n_a), (1, n_b)):
            p = 500 + STEP * (n - shared + k)
            out.append(row(anchor, read, L, 0, 599, p, p + 599, 530 + k, line, True))
            line += 1
        anchor += 1
    return np.array(out, dtype=ROW_DTYPE)


@gpu
def test_last_ranks_of_two_reads_of_256_rows(oracle):
    """the longest reads the bin path sorts: the candidates of the one edge have j = 254, 255 and q = 254, 255"""
    rows = _rank_rows(256, 256, 2)
    want = oracle.overlap(rows)
    assert [int(x) for x in want["edges"]["em_cnt"]] == [2]
    assert_tables_equal(_run(rows), want, "ranks 255")


@gpu
@pytest.mark.parametrize("n_a", [300, 1100])
def test_ranks_above_255_on_the_atomic_path(oracle, monkeypatch, n_a):
    """a read of 300 (1,100) rows shares its last three anchors with a short read, the index built without bins
    (MSGPU_NO_BIN): k_candidates_big writes ranks 297 .. 299 (1,097 .. 1,099)"""
    monkeypatch.setenv("MSGPU_NO_BIN", "1")
    rows = _rank_rows(n_a, 3, 3)
    want = oracle.overlap(rows)
    assert [int(x) for x in want["edges"]["em_cnt"]] == [3]
    assert_tables_equal(_run(rows), want, "ranks to %d" % (n_a - 1))


@gpu
@pytest.mark.parametrize("n_rows", [0, 1])
def test_empty_job_and_one_row(oracle, n_rows):
    """no descriptor at all, through the whole step: every launch of the chain stage is skipped or finds nothing"""
    rows = _rows([(2, "clean")], 5)[:n_rows]
    want = oracle.overlap(rows)
    assert len(want["edges"]) == 0
    assert_tables_equal(_run(rows), want, "%d rows" % n_rows)


@gpu
@pytest.mark.parametrize("kind", ["clean", "mixed", "both"])
def test_wide_form_on_the_class_bounds(oracle, monkeypatch, kind):
    """the two-array form of the candidates (every candidate and chain kernel in its WIDE instance) against the packed run
    and the oracle, on the class-bounds input of test_gpu_chain_classes with an edge for k_chain_big added"""
    specs = [(n, kind) for n in BOUNDS for _ in range(9)] + [(64, kind), (70, kind)]
    rows = _rows(specs, 11)
    want = oracle.overlap(rows)
    packed = _run(rows)
    monkeypatch.setenv("MSGPU_CAND_WIDE", "1")
    wide = _run(rows)
    assert_tables_equal(packed, want, "packed/%s" % kind)
    assert_tables_equal(wide, want, "wide/%s" % kind)


@gpu
@pytest.mark.parametrize("env", ["MSGPU_CHAIN_SERIAL", "MSGPU_NO_SUBWAVE", "MSGPU_NO_BIN"])
def test_wide_form_other_dispatches(oracle, monkeypatch, env):
    """WIDE through k_chain_sub<W>, through the mode without size classes, and behind the atomic index path"""
    monkeypatch.setenv("MSGPU_CAND_WIDE", "1")
    monkeypatch.setenv(env, "1")
    specs = _mixed_directions()
    _check(oracle, _rows(specs, 78), [n for n, _ in specs], "wide/%s" % env)


def test_host_chooses_the_wide_form_above_65535_rows():
    """no GPU: the host's choice of the form from the job's largest read_cnt (msgpu_cand_wide, what the index build's
    read-back feeds): one word while the largest read has at most 65,535 rows, two arrays from 65,536"""
    from muchsalsa_amd import _lib
    f = _lib.lib().msgpu_cand_wide
    assert [f(n) for n in (0, 1, 256, 257, 65535)] == [0] * 5
    assert [f(n) for n in (65536, 65537, 1 << 20, 0xffffffff)] == [1] * 4
