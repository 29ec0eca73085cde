"""The chain kernels at their corners (tests/extremecases.py) against the C oracle, bit for bit: ill-formed nanopore
ranges (the general pair sweeps of k_chain and k_chain_sub, the general nano_check masks, the ratio rule on zero and
negative diffs), fp64 ties of the chaining DP on edges the all-pairs-compatible shortcut accepts, equal and zero scores,
exact alternative-path thresholds, and values near the integer limits.  Under the default dispatch and with the shortcut
off, one launch per width class, and one edge per wavefront; through load_rows, load_rows_packed and the PAF loader.
Each workload asserts that it holds what it claims to test."""
import numpy as np
import pytest

import extremecases as X
import test_golden_hand as H
from helpers import assert_tables_equal

pytestmark = pytest.mark.gpu

ENVS = [None, "MSGPU_NO_FASTPATH", "MSGPU_CHAIN_SERIAL", "MSGPU_NO_SUBWAVE"]
A_PARAMS = [dict(), dict(wiggle_room=0), dict(wiggle_room=0, ratio_pct=100.0)]


def _ids(kw):
    return ",".join("%s=%s" % i for i in kw.items()) or "default"


def _set(p, kw):
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _want(oracle, rows, kw):
    return oracle.overlap(rows, _set(oracle.default_params(), kw))


def _run(rows, kw, packed=False, contraction=False):
    """the overlap path on one context -> (tables, counts[, find_contraction_edges])"""
    from muchsalsa_amd import overlap
    with overlap.OverlapContext(0, _set(overlap.default_params(), kw)) as ctx:
        if packed:
            p = overlap.PackedRows(rows, int(rows["read_id"].max()) + 1)
            ctx.load_rows_packed(p)
        else:
            ctx.load_rows(rows)
        ctx.calculate_edges()
        ctx.chaining_and_overlaps()
        out = (ctx.tables(), ctx.counts())
        if contraction:
            out += (ctx.find_contraction_edges(),)
        if packed:
            p.close()
        return out


def _env(monkeypatch, env):
    if env:
        monkeypatch.setenv(env, "1")


def _bug_a_padded():
    """the bug-A pair alone and padded into every width class (test_golden_hand.pad), one table per size"""
    return [("w2", X.bug_a_rows())] + [(w, H.pad(X.bug_a_rows(), f)) for w, f in H.PAD_FILL.items()]


@pytest.fixture(scope="module")
def ill_formed():
    """(a): every kind, one bad element or all, one strand or both, at every class bound; the bug-A pair in every width
    class; wavefronts of k_chain_sub that mix well-formed and ill-formed groups"""
    return X.join([X.rows_of(X.ill_formed_specs(), 5)] + [r for _, r in _bug_a_padded()] + [X.subwave_mix_rows(6)])


@pytest.fixture(scope="module")
def ill_formed_want(oracle, ill_formed):
    return {_ids(kw): _want(oracle, ill_formed, kw) for kw in A_PARAMS}


def test_ill_formed_coverage(ill_formed, ill_formed_want):
    """an edge with an ill-formed corrected range in every width class (<= 8, 9-16, 17-32, 33-64, 65-256, > 256), and
    mixed pairs whose signed diff sum is below -wiggle (chained by the reference, refused by a |d1 + d2| test) in the
    classes of k_chain"""
    for kw in A_PARAMS:
        per_class, neg_mixed = X.coverage_a(ill_formed, ill_formed_want[_ids(kw)], kw.get("wiggle_room", 300))
        # (the bug-A pair sits in the five classes up to 64)
        assert min(per_class) >= 4 and neg_mixed >= 5, (kw, per_class, neg_mixed)


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("kw", A_PARAMS, ids=_ids)
def test_ill_formed(ill_formed, ill_formed_want, monkeypatch, env, kw):
    _env(monkeypatch, env)
    got, _ = _run(ill_formed, kw)
    assert_tables_equal(got, ill_formed_want[_ids(kw)], "ill-formed/%s/%s" % (env, _ids(kw)))


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("wiggle", [300, 0])
def test_bug_a_pair_in_every_width_class(oracle, monkeypatch, env, wiggle):
    """the hand-derived verdict (extremecases.bug_a_verdict: chained, -889 <= wiggle) in every width class"""
    _env(monkeypatch, env)
    assert X.bug_a_verdict(wiggle)
    for w, rows in _bug_a_padded():
        want = _want(oracle, rows, dict(wiggle_room=wiggle))
        got, _ = _run(rows, dict(wiggle_room=wiggle))
        assert H.chained(want), w
        assert_tables_equal(got, want, "bug A/%s/%s/%d" % (w, env, wiggle))


def test_ill_formed_packed_and_contraction(oracle, ill_formed, ill_formed_want):
    """the same table through load_rows_packed (every score < 2^30), and findContractionEdges on its tables"""
    want = ill_formed_want["default"]
    got, _, co = _run(ill_formed, {}, packed=True, contraction=True)
    assert_tables_equal(got, want, "ill-formed/packed")
    want_co = oracle.find_contraction_edges(want, len(want["read_len"]))
    assert np.array_equal(co, want_co)
    for kw in A_PARAMS[1:]:
        w = ill_formed_want[_ids(kw)]
        _, _, co = _run(ill_formed, kw, contraction=True)
        assert np.array_equal(co, oracle.find_contraction_edges(w, len(w["read_len"]), wiggle=kw["wiggle_room"]))


@pytest.fixture(scope="module")
def ties_b():
    return X.shortcut_tie_rows(X.shortcut_tie_specs())


@pytest.mark.parametrize("env", ENVS)
def test_shortcut_ties(oracle, ties_b, monkeypatch, env):
    """(b): one-strand edges the shortcut accepts, each with an fp64 tie of the DP (the tiny anchor's score is absorbed,
    the next anchor takes the earlier predecessor) and a control twin without one"""
    import test_oracle_extremes as T
    _env(monkeypatch, env)
    want = _want(oracle, ties_b, {})
    if env is None:
        T._check_ties(ties_b, want)
    got, c = _run(ties_b, {})
    assert_tables_equal(got, want, "ties/%s" % env)
    n = want["edges"]["em_cnt"]
    twins = int((n[1::2] <= 64).sum())  # the shortcut is k_chain's and k_chain_sub's: edges of 64 or fewer
    assert twins > 50
    if env != "MSGPU_NO_FASTPATH":
        assert twins <= int(c.n_edges_fastpath) <= int((n <= 64).sum())


@pytest.fixture(scope="module")
def ties_c():
    return X.ties_rows(3)


def test_ties_and_zeros_coverage(oracle, ties_c):
    """(c) holds DP ties between equal predecessors, edges whose populations are all 0 (the argmax's best <= 0 branch)
    and populations equal to max * alt_frac, in both directions"""
    for frac in (0.75, 0.5):
        want = _want(oracle, ties_c, dict(alt_frac=frac))
        pops = X.dp_populations(ties_c, want)
        for d in (False, True):
            mine = [p for p in pops if p[1] == d]
            assert sum(p[3] for p in mine) >= 5
            assert sum(all(v == 0.0 for v in p[2]) for p in mine) >= len(X.BOUNDS)
            assert any(0 < v == max(p[2]) * frac for p in mine for v in p[2])


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("kw", [dict(), dict(alt_frac=0.5), dict(wiggle_room=0)], ids=_ids)
def test_ties_and_zeros(oracle, ties_c, monkeypatch, env, kw):
    _env(monkeypatch, env)
    got, _ = _run(ties_c, kw)
    assert_tables_equal(got, _want(oracle, ties_c, kw), "ties-zeros/%s/%s" % (env, _ids(kw)))


def test_ties_and_zeros_packed(oracle, ties_c):
    got, _ = _run(ties_c, {}, packed=True)
    assert_tables_equal(got, _want(oracle, ties_c, {}), "ties-zeros/packed")


@pytest.mark.parametrize("env", ENVS)
@pytest.mark.parametrize("kw", [dict(), dict(wiggle_room=0)], ids=_ids)
def test_magnitudes(oracle, monkeypatch, env, kw):
    """(d): av / bv just inside and outside +-1e9 (the shortcut takes the first and declines the second), coordinates
    near +-2^30, read length 2^31 - 1, scores 2^30 - 1, 2^30, 2^31 - 1 and 2^32 - 1 mixed"""
    _env(monkeypatch, env)
    rows = X.magnitude_rows(4)
    want = _want(oracle, rows, kw)
    if env is None and not kw:
        clean = [X.shortcut_predicate(e, 300) for e in X.elements(rows, want)]
        assert any(clean) and not all(clean)
        assert {int(s) for s in rows["score"]} == set(X.SCORES_D) and int(rows["read_len"].max()) == X.I32
    got, _ = _run(rows, kw)
    assert_tables_equal(got, want, "magnitudes/%s/%s" % (env, _ids(kw)))


def test_magnitudes_packed(oracle):
    rows = X.magnitude_rows(7, scores=(0, 1, 2 ** 30 - 1))
    got, _ = _run(rows, {}, packed=True)
    assert_tables_equal(got, _want(oracle, rows, {}), "magnitudes/packed")


@pytest.mark.parametrize("env", [None, "MSGPU_NO_SUBWAVE"])
def test_paf_text(oracle, tmp_path, monkeypatch, env):
    """the loader-reachable part as PAF text: columns 7 and 8 equal, reversed or negative, nmatch up to 2^31 - 1"""
    from muchsalsa_amd import overlap
    _env(monkeypatch, env)
    path = tmp_path / "x.paf"
    path.write_text(X.paf_text(X.loader_rows(8)))
    paf = overlap.parse_paf(str(path))
    ref = oracle.parse_paf(str(path))
    assert paf.rows.tobytes() == ref["rows"].tobytes()
    r = ref["rows"]
    assert (r["n_hi"] == r["n_lo"] - 1).any() and (r["n_hi"] < r["n_lo"] - 1).any() and (r["n_lo"] < 0).any()
    assert int(r["score"].max()) == 2 ** 31 - 1
    got, _ = _run(paf.rows, {})
    assert_tables_equal(got, oracle.overlap(ref["rows"]), "paf/%s" % env)
