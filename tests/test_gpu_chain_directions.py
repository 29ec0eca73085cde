"""The chain kernels on edges of one strand each, forward and reverse, as neighbouring groups of a wavefront.

k_chain_sub_all builds the path lists once per direction a group has (one pass for every group's first direction, a
second one only in a wavefront that holds an edge with both), emits each group's kept paths as one sequence (minus
first), and reduces its fp64 maxima with DPP moves; k_chain reduces the same way.  What the BASELINE workload consists
of -- all-forward and all-reverse edges of different sizes side by side -- is laid out here on purpose: the kinds "plus",
"minus" and "both" in every order of neighbours, wavefronts without a mixed edge and with exactly one, edges with
several kept paths beside edges with one, score ties and all-zero scores in both directions.  The GPU's four tables must
equal the C oracle's bit for bit.

The tests without the gpu mark state what each table is, on the oracle's output: they need no GPU.  The neighbours of a
wavefront are taken from the order the library documents for its class lists (k_emit_edges: a counting sort by the
number of EdgeMatches, descending, edges of one size in edge order)."""
import numpy as np
import pytest

import extremecases as X
from helpers import assert_tables_equal
from test_golden_hand import row
from muchsalsa_amd.synth import ROW_DTYPE

STEP = 800  # anchor spacing on both reads
KINDS = ("plus", "minus", "both")
# every ordered pair of kinds, pair after pair, and one edge more: 19 edges, so that the pairs sit at even positions of
# the class list for every second size (the two groups of a 32-wide wavefront) and sizes meet inside wavefronts
CYCLE = tuple(k for a in KINDS for b in KINDS for k in (a, b)) + ("minus",)
ENVS = [None, "MSGPU_NO_FASTPATH", "MSGPU_CHAIN_SERIAL"]
ORD_DIR = 4  # MSGPU_ORD_DIR


def _edge(out, n, read0, anchor0, line0, rng, kind, jitter=True):
    """rows of one edge: reads read0 and read0 + 1 share n anchors.  kind "plus": every anchor on the second read's
    forward strand; "minus": every one on its reverse strand; "both": about a third on the other strand.  With jitter
    some anchors lie off the chain or on their neighbour's range (incompatible pairs, contained anchors)."""
    L = 2000 + STEP * n
    line = line0
    for j in range(n):
        p0 = 500 + STEP * j
        p1 = 700 + STEP * j + int(rng.integers(-60, 61))
        if jitter:
            u = rng.random()
            if u < 0.2:
                p1 += int(rng.integers(-1500, 1501))
            elif u < 0.35 and j > 0:
                p1 = 700 + STEP * (j - 1)
        plus = kind == "plus"
        if kind == "both":
            plus = rng.random() >= 0.35
            if j < 2:
                plus = j == 0  # both strands, whatever the draw
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


def _run(rows, params=None):
    from muchsalsa_amd import overlap
    p = overlap.default_params()
    for k, v in (params or {}).items():
        setattr(p, k, v)
    with overlap.OverlapContext(0, p) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables()


def _kinds(want):
    """per edge of the oracle's tables: its number of EdgeMatches and the kind its EdgeMatches' strands make"""
    ed, ems = want["edges"], want["ems"]
    out = []
    for e in ed:
        d = ems["flags"][int(e["em_off"]): int(e["em_off"]) + int(e["em_cnt"])] & 1
        out.append((int(e["em_cnt"]), "plus" if d.all() else ("both" if d.any() else "minus")))
    return out


def _width(n):
    return 8 if n <= 8 else 16 if n <= 16 else 32 if n <= 32 else 64


def _wavefronts(want):
    """{W: the wavefronts of the W-wide class, each a list of (n, kind) of its 64 / W groups}"""
    kinds = _kinds(want)
    out = {}
    for W in (8, 16, 32):
        cls = sorted((k for k in kinds if _width(k[0]) == W), key=lambda k: -k[0])  # (stable: one size in edge order)
        out[W] = [cls[i: i + 64 // W] for i in range(0, len(cls), 64 // W)]
    return out


def _orders_per_edge(want):
    return np.bincount(want["orders"]["edge_idx"].astype(np.int64), minlength=len(want["edges"]))


# ---- the kinds as neighbours ---------------------------------------------------------------------------------------------
def interleaved_specs():
    """every size from 2 to 33, the 19 edges of CYCLE of each"""
    return [(n, k) for n in range(2, 34) for k in CYCLE]


def one_strand_specs():
    """sizes 2..33, plus and minus only: no wavefront holds an edge with both directions"""
    return [(n, ("plus", "minus")[(i + i // 3 + n) % 2]) for n in range(2, 34) for i in range(8)]


def one_mixed_specs():
    """as one_strand_specs, with ONE edge of both directions per width class (n = 5, 12 and 25)"""
    specs = one_strand_specs()
    for n in (5, 12, 25):
        specs[specs.index((n, "minus"))] = (n, "both")
    return specs


def _oracle_of(oracle, specs, seed):
    rows = _rows(specs, seed)
    want = oracle.overlap(rows)
    assert sorted(k for k in _kinds(want)) == sorted(specs)  # every edge as built, in size and in strands
    return rows, want


def test_interleaved_table_holds_every_pair_of_neighbours(oracle):
    _, want = _oracle_of(oracle, interleaved_specs(), 31)
    for W, waves in _wavefronts(want).items():
        pairs = {(a[1], b[1]) for w in waves for a, b in zip(w, w[1:])}
        assert pairs == {(a, b) for a in KINDS for b in KINDS}, W
        assert any(len({g[0] for g in w}) > 1 for w in waves), W  # groups of different sizes in one wavefront
    # paths on both strands of one edge, and orders of both strands
    flags = want["orders"]["flags"].astype(np.int64)
    assert (flags & ORD_DIR).any() and not (flags & ORD_DIR).all()
    by_edge = {}
    for o, f in zip(want["orders"]["edge_idx"], flags):
        by_edge.setdefault(int(o), set()).add(int(f) & ORD_DIR)
    assert any(len(s) == 2 for s in by_edge.values())


def test_one_strand_tables_are_what_they_claim(oracle):
    _, want = _oracle_of(oracle, one_strand_specs(), 41)
    for W, waves in _wavefronts(want).items():
        assert all(g[1] != "both" for w in waves for g in w), W            # the second pass runs nowhere
        assert any({g[1] for g in w} == {"plus", "minus"} for w in waves), W  # some wavefront has both strands
    _, want = _oracle_of(oracle, one_mixed_specs(), 41)
    for W, waves in _wavefronts(want).items():
        per_wave = sorted(sum(g[1] == "both" for g in w) for w in waves)
        assert per_wave[-1] == 1 and per_wave[-2] == 0, W  # one wavefront with exactly one mixed group, none in the others


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
def test_interleaved_kinds(oracle, monkeypatch, env):
    if env:
        monkeypatch.setenv(env, "1")
    rows, want = _oracle_of(oracle, interleaved_specs(), 31)
    assert_tables_equal(_run(rows), want, "interleaved/%s" % env)


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("which", ["none_mixed", "one_mixed"])
def test_second_pass_skipped_or_taken_once(oracle, monkeypatch, env, which):
    if env:
        monkeypatch.setenv(env, "1")
    rows, want = _oracle_of(oracle, one_strand_specs() if which == "none_mixed" else one_mixed_specs(), 41)
    assert_tables_equal(_run(rows), want, "%s/%s" % (which, env))


# ---- several kept paths beside one ------------------------------------------------------------------------------------------
def several_paths_rows():
    """edges of two disjoint chains of equal length (extremecases._alt_edge with m = q: the side chain's population
    equals the main chain's, above max * alt_frac) beside plain one-chain edges, both directions, sizes of every class;
    the two-chain edges alternate with the plain ones and their direction alternates at half that rate"""
    rng = np.random.default_rng(5)
    out, anchor, line, read, specs = [], 0, 0, 0, []
    for rep in range(3):
        for i, (m, q) in enumerate([(3, 3), (4, 4), (2, 2), (5, 4), (6, 6), (8, 7), (5, 5), (12, 12), (16, 15), (10, 10), (20, 20)]):
            plus = (i // 2 + rep) % 2 == 0
            line = X._alt_edge(out, m, q, read, anchor, line, plus)
            anchor, read = anchor + m + q, read + 2
            specs.append((m + q, "two"))
            n = m + q if rep < 2 else max(2, m + q - 1 - rep)
            line = _edge(out, n, read, anchor, line, rng, "minus" if plus else "plus", jitter=False)  # the other strand
            anchor, read = anchor + n, read + 2
            specs.append((n, "one"))
    return X.check_int32(np.array(out, dtype=ROW_DTYPE)), specs


def test_several_paths_table_is_what_it_claims(oracle):
    rows, specs = several_paths_rows()
    want = oracle.overlap(rows)
    assert [int(x) for x in want["edges"]["em_cnt"]] == [n for n, _ in specs]
    per_edge = _orders_per_edge(want)
    two = [int(per_edge[e]) for e, s in enumerate(specs) if s[1] == "two"]
    one = [int(per_edge[e]) for e, s in enumerate(specs) if s[1] == "one"]
    assert min(two) >= 2 and set(one) == {1}
    # an edge of several orders and an edge of one as neighbours of a wavefront, in every class and on both strands
    ed = want["edges"]
    for W in (8, 16, 32):
        cls = sorted((e for e in range(len(ed)) if _width(int(ed["em_cnt"][e])) == W), key=lambda e: -int(ed["em_cnt"][e]))
        G = 64 // W
        seen = set()
        for i in range(0, len(cls), G):
            for a, b in zip(cls[i: i + G], cls[i + 1: i + G]):
                if {int(per_edge[a]) >= 2, int(per_edge[b]) >= 2} == {True, False}:
                    many = a if per_edge[a] >= 2 else b
                    seen.add(bool(want["ems"]["flags"][int(ed["em_off"][many])] & 1))
        assert seen == {True, False}, W


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
def test_several_paths_beside_one(oracle, monkeypatch, env):
    if env:
        monkeypatch.setenv(env, "1")
    rows, _ = several_paths_rows()
    assert_tables_equal(_run(rows), oracle.overlap(rows), "several/%s" % env)


# ---- the maximum: ties between lanes and a best score of 0, both directions ---------------------------------------------------
TIE_SIZES = (2, 3, 7, 8, 11, 15, 16, 19, 23, 27, 31, 32, 33, 35, 47, 63, 64)  # 4 k + 3: the last two anchors are twins


def tie_rows(seed):
    """per size an equal-score edge with twins (extremecases._twin_edge: equal populations in two lanes, the first
    wins) and the same edge with every score 0 (no population above 0: the first lane of the direction wins), with the
    direction changing from edge to edge so that a wavefront's neighbours differ in strand"""
    rng = np.random.default_rng(seed)
    out, anchor, line, read, k = [], 0, 0, 0, 0
    for rep in range(3):
        for n in TIE_SIZES:
            for score in ((560, 540), (0, 0)):
                plus = (k + k // 3) % 2 == 0
                k += 1
                line = X._twin_edge(out, n, read, anchor, line, score, plus, rng)
                anchor, read = anchor + n, read + 2
    return X.check_int32(np.array(out, dtype=ROW_DTYPE))


def test_tie_table_is_what_it_claims(oracle):
    rows = tie_rows(9)
    want = oracle.overlap(rows)
    kinds = _kinds(want)
    assert {k[1] for k in kinds} == {"plus", "minus"}
    tied = {True: 0, False: 0}  # edges whose maximum sits in two lanes; edges whose best population is 0
    zero = {True: 0, False: 0}
    for _, plus, pop, _ in X.dp_populations(rows, want):
        best = max(pop)
        if best <= 0.0:
            zero[bool(plus)] += 1
        elif sum(1 for p in pop if p == best) >= 2:
            tied[bool(plus)] += 1
    assert min(tied.values()) >= 5 and min(zero.values()) >= 5, (tied, zero)
    for W, waves in _wavefronts(want).items():
        assert any({g[1] for g in w} == {"plus", "minus"} for w in waves), W


@pytest.mark.gpu
@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("frac", [0.75, 0.5])
def test_ties_and_zero_maxima(oracle, monkeypatch, env, frac):
    if env:
        monkeypatch.setenv(env, "1")
    rows = tie_rows(9)
    op = oracle.default_params()
    op.alt_frac = frac
    want = oracle.overlap(rows, op)
    assert_tables_equal(_run(rows, dict(alt_frac=frac)), want, "ties/%s/%s" % (env, frac))
