"""The sub-wavefront chain kernel (k_chain_sub_all: W = 8 / 16 / 32 lanes per edge) and k_chain at the bounds of their width
classes.  Edges of n = 2, 8, 9, 16, 17, 32 and 33 EdgeMatches, one strand and both strands, and wavefronts whose groups
hold edges of different sizes: edges built for the all-pairs-compatible shortcut (one strand, every pair compatible) beside
edges that need the pair sweep.  Most edges mix compatible pairs with incompatible ones (jittered anchors, and contained
anchors: orientation 0), as BASELINE data does.  The GPU's tables must equal the C oracle's bit for bit, also with the
shortcut off (MSGPU_NO_FASTPATH) and with a launch per width class (MSGPU_CHAIN_SERIAL)."""
import numpy as np
import pytest

from helpers import assert_tables_equal
from test_golden_hand import row
from muchsalsa_amd.synth import ROW_DTYPE

pytestmark = pytest.mark.gpu

BOUNDS = (2, 8, 9, 16, 17, 32, 33)
STEP = 800  # anchor spacing on both reads


def _edge(out, n, read0, anchor0, line0, rng, kind):
    """rows of one edge: reads read0 and read0 + 1 share n anchors.  kind: "clean" (one strand, every pair compatible),
    "mixed" (one strand, some anchors jittered past the wiggle room or contained in their neighbour), "both" (as mixed,
    with about a third of the anchors on the other strand of the second read)"""
    L = 2000 + STEP * n
    line = line0
    for j in range(n):
        p0 = 500 + STEP * j
        p1 = 700 + STEP * j + int(rng.integers(-60, 61))
        plus = True
        if kind != "clean":
            u = rng.random()
            if u < 0.2:
                p1 += int(rng.integers(-1500, 1501))  # far off the chain: incompatible with most
            elif u < 0.35 and j > 0:
                p1 = 700 + STEP * (j - 1)  # on its neighbour's range: contained, orientation 0
            if kind == "both" and rng.random() < 0.35:
                plus = False
        p1 = min(max(p1, 0), L - 600)
        if not plus:
            p1 = L - 600 - p1
        s0, s1 = int(rng.integers(440, 620)), int(rng.integers(440, 620))
        i_lo = int(rng.integers(0, 40))
        out.append(row(anchor0 + j, read0, L, 0, 599, p0, p0 + 599, s0, line, True))
        out.append(row(anchor0 + j, read0 + 1, L, i_lo, 599, p1, p1 + 599 - i_lo, s1, line + 1, plus))
        line += 2
    return line


def _rows(specs, seed):
    """one row table: an edge per (n, kind) of specs, each on a pair of reads of its own"""
    rng = np.random.default_rng(seed)
    out, anchor, line = [], 0, 0
    for e, (n, kind) in enumerate(specs):
        line = _edge(out, n, 2 * e, anchor, line, rng, kind)
        anchor += n
    return np.array(out, dtype=ROW_DTYPE)


def _run(rows):
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0, overlap.default_params()) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables()


def _check(oracle, rows, want_sizes, what):
    want = oracle.overlap(rows)
    sizes = sorted(int(x) for x in want["edges"]["em_cnt"])
    assert sizes == sorted(want_sizes), what  # every edge as built: one EdgeMatch per shared anchor
    got = _run(rows)
    assert_tables_equal(got, want, what)
    return want


ENVS = [None, "MSGPU_NO_FASTPATH", "MSGPU_CHAIN_SERIAL"]


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("kind", ["clean", "mixed", "both"])
def test_class_bounds(oracle, monkeypatch, env, kind):
    """edges at every class bound, several of each size (consecutive groups of a wavefront), one edge kind per table"""
    if env:
        monkeypatch.setenv(env, "1")
    specs = [(n, kind) for n in BOUNDS for _ in range(9)]
    want = _check(oracle, _rows(specs, 11), [n for n, _ in specs], "%s/%s" % (kind, env))
    assert len(want["orders"]) >= len(specs)


@pytest.mark.parametrize("env", ENVS)
def test_groups_of_different_sizes(oracle, monkeypatch, env):
    """every size from 2 to 33, every kind, interleaved: the groups of one wavefront differ in n, in the shortcut, and in
    whether their edge has one strand or two"""
    if env:
        monkeypatch.setenv(env, "1")
    kinds = ("clean", "mixed", "both")
    specs = [(n, kinds[(n + r) % 3]) for r in range(4) for n in range(2, 34)]
    want = _check(oracle, _rows(specs, 23), [n for n, _ in specs], "sizes/%s" % env)
    # the workload is what it claims to be: some edges chain past one anchor, some edges have paths on both strands
    flags = want["orders"]["flags"].astype(np.int64)
    assert (want["orders"]["ids_cnt"] > 1).any()
    by_edge = {}
    for o, f in zip(want["orders"]["edge_idx"], flags):
        by_edge.setdefault(int(o), set()).add(int(f) & 4)
    assert any(len(s) == 2 for s in by_edge.values())


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_sizes(oracle, seed):
    """random sizes around the bounds, random kinds, in random order"""
    rng = np.random.default_rng(100 + seed)
    ns = rng.choice(np.array([2, 3, 7, 8, 9, 10, 15, 16, 17, 18, 31, 32, 33, 34]), size=160)
    ks = rng.choice(np.array(["clean", "mixed", "both"]), size=160)
    specs = [(int(n), str(k)) for n, k in zip(ns, ks)]
    _check(oracle, _rows(specs, 200 + seed), [n for n, _ in specs], "random%d" % seed)
