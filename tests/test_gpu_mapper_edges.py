"""The mapper's kernels at their edges, on the GPU: the inputs of tests/mapedgecases.py (tiles, record ends and hash ties for
k_mp_sketch; the 64-predecessor window, ties across a block of 64 lanes, the size classes and rows without a group for
k_mp_chain, k_mp_chain16, k_mp_classify and k_mp_walk) through the stage on files, compared as tests/test_gpu_mapper.py
compares: the PAF byte for byte, the chain table field for field and every count against the plain-Python restatement
(tests/map_oracle.py), without any tolerance.  The conditions the inputs meet are asserted in
tests/test_mapper_edges_host.py.  No test provokes a device fault.  Every test runs under its own time limit: a watchdog ends
the process when a stage call does not come back."""
import faulthandler
import os

import pytest

import mapedgecases as E
import test_mapper_batches_host as host
import test_mapper_edges_host as edges_host

pytestmark = pytest.mark.gpu

LIMIT = 600  # seconds per test
KEYS = ("minimizers", "keys", "keys_dropped", "entries_dropped", "anchors", "n_groups", "groups_kept", "groups_small",
        "groups_large", "largest_group", "group_hist", "below_score", "below_count", "chains_cut", "pairs", "capped")


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


def _stage(mp, d, name, budget=0, **params):
    tp, qp = E.write_inputs(name, d)
    out = os.path.join(str(d), "out.paf")
    tables = {}
    res = mp.run(tp, qp, out, tables=tables, budget_mb=budget / 2.0 ** 20 if budget else None, **params)
    with open(out, "rb") as h:
        text = h.read()
    assert text == tables["text"]
    return res, tables, text


def _check(mp, d, name, budget=0, **params):
    """test_gpu_mapper._check on an input of mapedgecases"""
    want = E.expected(name, **params)
    res, tb, text = _stage(mp, d, name, budget, **params)
    print("%s %r: %d anchors, %d groups (%d kept: %d of at most 16 anchors, %d larger; largest %d), %d chains, histogram %r" % (
        name, params, res["anchors"], res["n_groups"], res["groups_kept"], res["groups_small"], res["groups_large"],
        res["largest_group"], res["chains"], res["group_hist"]))
    for key in KEYS:
        assert res[key] == want[key], key
    assert res["chains"] == len(want["chains"]) and tb["chains"] == want["chains"]
    assert len(text) == len(want["paf"]) and text == want["paf"]
    assert res["bytes_out"] == len(text) and res["lost_publications"] == 0
    assert {k: res["params"][k] for k in want["params"]} == want["params"]
    for x in res["batches"]:
        assert x["bytes_peak"] <= x["bytes_bound"]
    return res, tb, text, want


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_against_the_restatement(mp, tmp_path, case):
    res = _check(mp, tmp_path, case[0], **case[1])[0]
    if E.is_readout(case[1]):  # every anchor is a chain: the table reads rules 1 to 4 out position by position
        assert res["chains"] == res["anchors"] > 0
        assert len(res["batches"]) == 1 and res["batches"][0]["n_chains"] == res["batches"][0]["n_anchors"] == res["anchors"]


@pytest.mark.parametrize("k,w", E.ENDS)
def test_the_record_starts_cover_the_tile_grid(mp, tmp_path, k, w):
    """the offsets the loader gives the short records in a device store: at least 128 of the 256 residues modulo 256"""
    from muchsalsa_amd import sequences
    with sequences.SeqStore(0) as store:
        n = edges_host.record_start_residues("ends-%d-%d" % (k, w), tmp_path, store)
    print("ends-%d-%d: %d residues" % (k, w, n))
    assert n >= 128


@pytest.mark.parametrize("name", ["sizes", "sizes-rc"])
def test_the_size_classes_a_record_at_a_time(mp, tmp_path, name):
    """the smallest budget: most launches of k_mp_chain16 have one row with a group, the last has three"""
    one = edges_host.edge_budgets(name, E.SIZES_PARAMS)[0]
    res = _check(mp, tmp_path, name, one, **E.SIZES_PARAMS)[0]
    a, b = edges_host.edge_record_counts(name, E.SIZES_PARAMS)
    cut = host.greedy_cut(a, b, host.batch_bytes(0), one)
    bt = res["batches"]
    assert res["budget_bytes"] == one and len(cut) == 9
    assert [(x["first_query"], x["n_queries"], x["n_anchors"], x["n_query_bases"]) for x in bt] == cut
    assert all(x["bytes_bound"] <= one for x in bt) and sum(x["n_chains"] for x in bt) == 24
