"""GPU parity away from msgpu_default_params(): wiggle room, the ratio rule, the alternative-path fraction and the overlap
threshold reach the chain kernels at run time (the lean and general sweeps of k_chain, k_chain_sub<8|16|32> and
k_chain_sub_all, k_chain_big, the all-pairs-compatible shortcut) and k_check_contraction.  Every parameter set runs on
workloads with edges in every width class, one-strand and mixed-strand, and must (a) equal the oracle's tables bit for bit
and (b) change those tables against the default set, so that a kernel that ignored or hard-coded the field would fail.
The hand-derived boundary cases of test_golden_hand.py replay here through the HIP path, padded into every width class."""
import numpy as np
import pytest

import test_golden_hand as H
from helpers import TABLES, assert_tables_equal

pytestmark = pytest.mark.gpu

U64 = 2 ** 64 - 1
# (name, msgpu_params fields)
SETS = [("wiggle%d" % w if w != U64 else "wiggle_u64max", dict(wiggle_room=w))
        for w in (0, 1, 3, 4, 50, 299, 301, 2000, 10 ** 6, U64)]
SETS += [("w%d_ratio%s" % (w, r), dict(wiggle_room=w, ratio_pct=r)) for w in (0, 300) for r in (0.0, 7.5, 100.0)]
SETS += [("w%d_alt%s" % (w, a), dict(wiggle_room=w, alt_frac=a)) for w in (0, 300) for a in (0.0, 0.5, 0.99, 1.0)]
SETS += [("th_overlap%d" % t, dict(th_overlap=t)) for t in (0, 400)]
# (workload, set) pairs whose tables equal the default set's.  No pair of these workloads is 299..301 apart after the
# ratio rule, at wiggle 300 the ratio rule decides no pair, and on one-strand input every compatible pair already passes
# at 300; the hand-derived cases (test_hand_cases_at_params: wiggle 299 / 301 boundaries, ratio 0 and 7.5 at wiggle 300)
# pin those fields instead.
NO_BITE = {(load, name) for load in ("clean", "mixed") for name in ("wiggle299", "wiggle301", "w300_ratio0.0", "w300_ratio7.5")}
NO_BITE |= {("clean", name) for name in ("wiggle2000", "wiggle1000000", "wiggle_u64max", "w300_ratio100.0")}


def _widths(n):
    """EdgeMatches per edge -> edge counts of the width classes <= 8, 9-16, 17-32, 33-64, 65-256, > 256"""
    return [int((n <= 8).sum()), int(((n > 8) & (n <= 16)).sum()), int(((n > 16) & (n <= 32)).sum()),
            int(((n > 32) & (n <= 64)).sum()), int(((n > 64) & (n <= 256)).sum()), int((n > 256).sum())]


def _join(parts):
    """row tables of disjoint read / anchor / line spaces, one after the other"""
    out, r0, a0, l0 = [], 0, 0, 0
    for p in parts:
        p = p.copy()
        p["read_id"] += r0
        p["anchor_id"] += a0
        p["line"] += l0
        r0, a0, l0 = int(p["read_id"].max()) + 1, int(p["anchor_id"].max()) + 1, int(p["line"].max()) + 1
        out.append(p)
    return np.concatenate(out)


@pytest.fixture(scope="module")
def loads():
    """clean: every read one strand (the shortcut's input); mixed: 30 % of the rows flipped (mixed-direction edges, both
    path lists).  Both hold edges of every width class of the chain kernels."""
    from muchsalsa_amd import synth
    clean = _join([synth.accepted_rows(synth.paf_table(400, 8000, 3200, 23, coverage=8))[0],
                   synth.accepted_rows(synth.paf_table(60, 40000, 3000, 5, coverage=6))[0]])
    mixed = clean.copy()
    rng = np.random.default_rng(29)
    mixed["flags"] ^= (rng.random(len(mixed)) < 0.3).astype(mixed["flags"].dtype)
    return {"clean": clean, "mixed": mixed}


@pytest.fixture(scope="module")
def defaults(oracle, loads):
    return {k: oracle.overlap(rows) for k, rows in loads.items()}


def _params(lib_default, kw):
    p = lib_default()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _run(rows, p):
    """the overlap path on one context -> (tables, counts)"""
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0, p) as ctx:
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        return ctx.tables(), ctx.counts()


def _differs(a, b):
    return any(a[k].tobytes() != b[k].tobytes() for k in TABLES)


def test_workloads_fill_every_width_class(defaults):
    for name, t in defaults.items():
        w = _widths(t["edges"]["em_cnt"])
        assert w[0] > 100 and w[1] > 100 and w[2] > 100 and w[3] > 100 and w[4] > 100 and w[5] > 20, (name, w)
    e, em = defaults["mixed"]["edges"], defaults["mixed"]["ems"]
    plus = np.bincount(np.repeat(np.arange(len(e)), e["em_cnt"]), weights=em["flags"] & 1, minlength=len(e))
    mixed = (plus > 0) & (plus < e["em_cnt"])
    assert mixed.sum() > 1000 and _widths(e["em_cnt"][mixed])[5] > 20


@pytest.mark.parametrize("name,kw", SETS, ids=[s[0] for s in SETS])
def test_build_overlaps_at_params(oracle, loads, defaults, name, kw):
    from muchsalsa_amd import overlap
    for load, rows in loads.items():
        want = oracle.overlap(rows, _params(oracle.default_params, kw))
        assert _differs(want, defaults[load]) == ((load, name) not in NO_BITE), (load, name)
        got, c = _run(rows, _params(overlap.default_params, kw))
        assert_tables_equal(got, want, "%s, %s" % (name, load))
        w = kw.get("wiggle_room", 300)
        if w <= 3:  # margin wiggle - 3 <= 0: no edge is provably all-compatible
            assert c.n_edges_fastpath == 0, (name, load)
        if w >= 2000 and load == "clean" and len(kw) == 1:
            assert c.n_edges_fastpath > 0, name
    if name == "wiggle_u64max":  # build_overlaps itself, at the reference's reading of wiggleRoom "-1"
        got = overlap.build_overlaps(loads["mixed"], params=_params(overlap.default_params, kw))
        assert_tables_equal(got, oracle.overlap(loads["mixed"], _params(oracle.default_params, kw)), name)


def test_shortcut_takes_no_more_edges_as_wiggle_grows(loads):
    """n_edges_fastpath is monotone in wiggle room (the margin min(wiggle, 2^40) - 3 only grows), 0 while the margin is
    <= 0, and constant from the saturation on: every clean edge is taken long before 2^40."""
    from muchsalsa_amd import overlap
    n = [_run(loads["clean"], _params(overlap.default_params, dict(wiggle_room=w)))[1].n_edges_fastpath
         for w in (0, 3, 4, 50, 300, 2000, 10 ** 6, 2 ** 40, U64)]
    assert n == sorted(n) and n[0] == n[1] == 0 and n[4] > 0 and n[6] == n[7] == n[8], n


DISPATCH = [("wiggle0", dict(wiggle_room=0)), ("wiggle4", dict(wiggle_room=4)), ("wiggle_u64max", dict(wiggle_room=U64)),
            ("w0_ratio0", dict(wiggle_room=0, ratio_pct=0.0)), ("w300_ratio0", dict(wiggle_room=300, ratio_pct=0.0))]


@pytest.mark.parametrize("name,kw", DISPATCH, ids=[s[0] for s in DISPATCH])
def test_dispatch_modes_agree_at_params(oracle, loads, monkeypatch, name, kw):
    """The same tables under the default dispatch, a launch per width (MSGPU_CHAIN_SERIAL), every edge <= 64 in k_chain
    (MSGPU_NO_SUBWAVE) and the full pair sweep for every edge (MSGPU_NO_FASTPATH)."""
    from muchsalsa_amd import overlap
    rows = loads["mixed"] if name != "wiggle_u64max" else loads["clean"]
    want = oracle.overlap(rows, _params(oracle.default_params, kw))
    assert_tables_equal(_run(rows, _params(overlap.default_params, kw))[0], want, name)
    for env in ("MSGPU_CHAIN_SERIAL", "MSGPU_NO_SUBWAVE", "MSGPU_NO_FASTPATH"):
        monkeypatch.setenv(env, "1")
        got, c = _run(rows, _params(overlap.default_params, kw))
        monkeypatch.delenv(env)
        assert_tables_equal(got, want, "%s, %s" % (name, env))
        if env == "MSGPU_NO_FASTPATH":
            assert c.n_edges_fastpath == 0


ENTRY = [("w0_ratio0_alt05", dict(wiggle_room=0, ratio_pct=0.0, alt_frac=0.5)), ("wiggle_u64max", dict(wiggle_room=U64)),
         ("w50_alt099_th400", dict(wiggle_room=50, alt_frac=0.99, th_overlap=400))]


@pytest.mark.parametrize("name,kw", ENTRY, ids=[s[0] for s in ENTRY])
def test_every_entry_point_takes_params(oracle, loads, monkeypatch, name, kw):
    """msgpu_overlap_batched (several windows; resident and not), msgpu_group of one, and a group of two rehearsed on one
    GPU (MSGPU_GROUP_TRANSPORT=copy) carry the params to their member contexts."""
    from muchsalsa_amd import distributed as D, overlap
    rows = loads["mixed"]
    want = oracle.overlap(rows, _params(oracle.default_params, kw))
    assert _differs(want, oracle.overlap(rows))
    with overlap.OverlapContext(0, _params(overlap.default_params, kw)) as ctx:
        for nb in (1, 4):
            got, info = ctx.overlap_batched(rows, nb)
            assert_tables_equal(got, want, "%s, %d windows" % (name, nb))
        got, _ = ctx.overlap_batched(rows, 3, resident=True, edgematches=False)
        assert got["ems"] is None
        assert_tables_equal(dict(got, ems=ctx.tables()["ems"]), want, "%s, resident" % name)
    with overlap.OverlapGroup([0], params=_params(overlap.default_params, kw)) as grp:
        t, info = grp.overlap(rows)
        assert info["n_members"] == 1
        assert_tables_equal(dict(t, ems=want["ems"]), want, "%s, group of one" % name)
    monkeypatch.setenv("MSGPU_GROUP_TRANSPORT", "copy")
    with overlap.OverlapGroup([0, 0], params=_params(overlap.default_params, kw)) as grp:
        t, info = grp.overlap(rows)
    monkeypatch.delenv("MSGPU_GROUP_TRANSPORT")
    assert info["n_members"] == 2 and info["n_ems"] == len(want["ems"])
    canon = D.canonicalize({k: t[k] for k in ("edges", "orders", "ids")})
    ref = {k: want[k].copy() for k in ("edges", "orders", "ids")}
    ref["edges"]["em_off"] = 0
    canon["edges"]["em_off"] = 0
    canon["ems"] = ref["ems"] = np.zeros(0, dtype=want["ems"].dtype)
    assert_tables_equal(canon, ref, "%s, group of two" % name)


@pytest.mark.parametrize("wiggle", [0, 50, 2000, U64])
def test_find_contraction_edges_at_wiggle(oracle, wiggle):
    """sanityCheck's (d1 + d2 + d3) < wiggleRoom (sc.cpp:29-90) in k_check_contraction reads the context's wiggle_room:
    tables of an overlap run at that wiggle (bit-exact themselves), then random order tables with offsets below 1000 (so
    that the wiggle test can decide) through the device-pointer form, against the oracle at the same wiggle."""
    import torch
    from graphcases import varlen_rows
    from muchsalsa_amd import overlap
    from test_graph_stage import random_tables
    with overlap.OverlapContext(0, _params(overlap.default_params, dict(wiggle_room=wiggle))) as ctx:
        rows = varlen_rows(400, 2500, 250_000, 2)
        ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        t = ctx.tables()
        n_reads = ctx.counts().n_reads
        assert_tables_equal(t, oracle.overlap(rows, _params(oracle.default_params, dict(wiggle_room=wiggle))), "overlap")
        assert np.array_equal(ctx.find_contraction_edges(), oracle.find_contraction_edges(t, n_reads, wiggle=wiggle))
        rng = np.random.default_rng(78)
        hits = differ = 0
        for trial in range(60):
            n_reads = int(rng.integers(5, 200))
            n_edges = int(rng.integers(n_reads // 2, min(n_reads * 4, n_reads * (n_reads - 1) // 2) + 1))
            t = random_tables(rng, n_reads, n_edges)
            o = t["orders"]
            o["flags"] |= np.where(rng.integers(0, 2, len(o)) == 0, 2, 0).astype(np.uint32)
            o["left_offset"] = rng.integers(0, 1000, len(o))
            o["right_offset"] = rng.integers(0, 1000, len(o))
            want = oracle.find_contraction_edges(t, n_reads, wiggle=wiggle)
            d_e = torch.from_numpy(t["edges"].view(np.uint8).copy()).cuda()
            d_o = torch.from_numpy(o.view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            got = ctx.find_contraction_edges(d_e.data_ptr(), len(t["edges"]), d_o.data_ptr(), len(o), n_reads)
            assert np.array_equal(got, want), trial
            hits += int((want >= 0).sum())
            differ += int((want != oracle.find_contraction_edges(t, n_reads, wiggle=300)).sum())
    assert hits > 100
    if wiggle >= 2000:  # (below 300 the wiggle test decides none of these candidates)
        assert differ > 0, wiggle


def _hand_runs():
    """(name, rows, params fields, check) for every hand case of test_golden_hand.py at every padding"""
    runs = []
    for name, rows, kw, want in H.PARAM_CASES:
        for cls, fill in [("w0", 0)] + sorted(H.PAD_FILL.items()):
            runs.append(("%s/%s" % (name, cls), H.pad(rows, fill), kw, lambda t, w=want: H.chained(t) == w))
    for name, best, alt, frac, taken in H.ALT_CASES:
        for cls, fill in [("w0", 0)] + sorted(H.PAD_FILL.items()):
            runs.append(("%s/%s" % (name, cls), H.pad(H.case_alt(best, alt), fill), dict(alt_frac=frac),
                         lambda t, k=taken: (1 in H.single_paths(t)) == k and not H.chained(t)))
    return runs


@pytest.mark.parametrize("env", [None, "MSGPU_NO_SUBWAVE"])
def test_hand_cases_at_params(oracle, monkeypatch, env):
    """The boundary cases (diff == wiggle, a ratio exactly at ratio_pct, d1 + d2 == wiggle on a mixed pair, an alternative
    exactly at alt_frac * max), each alone and padded into every width class with filler EdgeMatches of the other strand:
    the hand-derived verdict holds on the oracle's tables, and the GPU's tables equal the oracle's."""
    from muchsalsa_amd import overlap
    if env:
        monkeypatch.setenv(env, "1")
    by_params = {}
    for run in _hand_runs():
        by_params.setdefault(tuple(sorted(run[2].items())), []).append(run)
    n = 0
    for kwt, runs in by_params.items():
        kw = dict(kwt)
        with overlap.OverlapContext(0, _params(overlap.default_params, kw)) as ctx:
            for name, rows, _, check in runs:
                want = oracle.overlap(rows, _params(oracle.default_params, kw))
                assert check(want), name
                ctx.load_rows(rows)
                ctx.calculate_edges()
                ctx.chaining_and_overlaps()
                got = ctx.tables()
                assert_tables_equal(got, want, name)
                assert check(got), name
                n += 1
    assert n == 7 * (len(H.PARAM_CASES) + len(H.ALT_CASES))
