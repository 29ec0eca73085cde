"""The C and Python restatements agree at the chain kernels' corners (tests/extremecases.py): ill-formed nanopore ranges,
fp64 ties of the chaining DP, zero scores, exact alternative thresholds and values near the integer limits.  Nothing
else pins the C oracle there; the GPU tests of the same families (test_gpu_chain_extremes.py) compare with it."""
import pytest

import extremecases as X
from test_oracle_cross import _compare

A_PARAMS = [dict(), dict(wiggle_room=0), dict(wiggle_room=0, ratio_pct=100.0)]


def _ids(kw):
    return ",".join("%s=%s" % i for i in kw.items()) or "default"


@pytest.mark.parametrize("kw", A_PARAMS, ids=_ids)
def test_ill_formed(oracle, kw):
    # the Python restatement is quadratic in the edge size: the 256 / 257 class bounds run once, one strand
    specs = X.ill_formed_specs(X.BOUNDS[:-2]) + [(n, "one", k, "one") for n in (256, 257) for k in ("point", "reversed")]
    rows = X.join([X.rows_of(specs, 5), X.bug_a_rows(), X.subwave_mix_rows(6)])
    _compare(rows, oracle, **kw)


@pytest.mark.parametrize("wiggle", [300, 0])
def test_bug_a_pair(oracle, wiggle):
    """the hand-derived verdict: chained at wiggle 300 (-889 <= 300) and at wiggle 0 (-889 <= 0)"""
    import test_golden_hand as H
    c, _ = _compare(X.bug_a_rows(), oracle, wiggle_room=wiggle)
    assert X.bug_a_verdict(wiggle) and H.chained(c)


def test_shortcut_ties(oracle):
    specs = [s for s in X.shortcut_tie_specs() if s[0] <= 40 or s[0] == 65]
    rows = X.shortcut_tie_rows(specs)
    c, _ = _compare(rows, oracle)
    _check_ties(rows, c)


def _check_ties(rows, c):
    """every tie edge passes the shortcut's predicate, its DP leaves the chain, and the best path (the first order of the
    edge: the one path) omits the tiny anchor; its twin passes the predicate without a tie"""
    els = X.elements(rows, c)
    assert len(els) % 2 == 0
    for e, (tie, twin) in enumerate(zip(els[0::2], els[1::2])):
        assert X.shortcut_predicate(tie, 300) and X.shortcut_predicate(twin, 300)
        assert X.has_tie([x["score"] for x in tie]) and not X.has_tie([x["score"] for x in twin])
        tiny = [x["anchor"] for x in tie if x["score"] < 1]
        assert len(tiny) == 1
        ed = c["edges"][2 * e]
        o = c["orders"][int(ed["order_off"])]
        ids = [int(v) for v in c["ids"][int(o["ids_off"]):int(o["ids_off"]) + int(o["ids_cnt"])]]
        assert int(ed["order_cnt"]) == 1 and len(ids) == len(tie) - 1 and tiny[0] not in ids


@pytest.mark.parametrize("kw", [dict(), dict(alt_frac=0.5)], ids=_ids)
def test_ties_and_zeros(oracle, kw):
    rows = X.ties_rows(3, sizes=X.BOUNDS[:-2])
    _compare(rows, oracle, **kw)


def test_magnitudes(oracle):
    _compare(X.magnitude_rows(4), oracle)
    _compare(X.magnitude_rows(7, scores=(0, 1, 2 ** 30 - 1, 2 ** 32 - 1)), oracle, wiggle_room=0)


def test_loader_rows(oracle, tmp_path):
    """the PAF view of the loader-reachable part: the C loader keeps what the Python one keeps, and the restatements
    agree on its rows"""
    import ms_oracle_py as P
    path = tmp_path / "x.paf"
    path.write_text(X.paf_text(X.loader_rows(8)))
    got = oracle.parse_paf(str(path))
    py_rows, rn, an = P.parse_paf_text(path.read_text())
    assert len(py_rows) == len(got["rows"]) and rn == got["read_names"] and an == got["anchor_names"]
    assert all(a[k] == int(b[k]) for a, b in zip(py_rows, got["rows"]) for k in a)
    assert (got["rows"]["n_hi"] < got["rows"]["n_lo"]).any() and (got["rows"]["n_lo"] < 0).any()
    assert int(got["rows"]["score"].max()) == 2 ** 31 - 1
    _compare(got["rows"], oracle)
