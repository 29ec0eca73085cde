"""The edge cases of the k-mer abundance filter and of the short-read unitig assembly (tests/kmeredgecases.py), host side (no
GPU): every condition that keeps tests/test_gpu_kmer_edges.py from passing on nothing, asserted on the plain-Python
restatements (tests/kf_oracle.py, tests/ug_oracle.py) alone; test_unitigs_host's invariants on every unitig case; and the
restatements against their recorded counts and digests (tests/golden/kmer_edges/cases.json, made by
tools/make_kmer_edge_fixtures.py)."""
import json
import os
import sys

import pytest

import kmeredgecases as E
import test_unitigs_host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(ROOT, "tests", "golden", "kmer_edges", "cases.json")) as f:
        return json.load(f)


def _cut_at_500(r):
    """the result as min_length = 500 gives it, which test_unitigs_host._invariants expects: the cut text is that subset of
    the records of the all text"""
    recs = r["all"].split(b"\n")
    keep = [i for i, t in enumerate(r["unitigs"]) if t[0] >= 500]
    return dict(r, cut=b"".join(recs[2 * i] + b"\n" + recs[2 * i + 1] + b"\n" for i in keep), kept=len(keep))


def test_the_fixture_lists_the_cases(recorded):
    assert sorted(E.cases()) == sorted(recorded)
    assert E.cases() is E.cases() and all(isinstance(d, bytes) for v in E.cases().values() for d in v[2])


@pytest.mark.parametrize("name", list(E.cases()))
def test_the_case_meets_its_conditions(name, recorded):
    import make_kmer_edge_fixtures
    r = E.expected(name)
    assert E.meets_conditions(name, r) == []
    assert make_kmer_edge_fixtures.record(name) == recorded[name]
    if E.cases()[name][0] == "ug" and "error" not in r:
        assert r["cut"] == r["all"] and r["kept"] == len(r["unitigs"])  # min_length = 0
        test_unitigs_host._invariants(_cut_at_500(r))


def test_the_families_meet_their_conditions():
    assert E.family_conditions() == []


def test_the_inputs_are_functions_of_their_seeds():
    E.rnd.cache_clear()
    assert E.tile_file(*E.TILE_FILES["8192o"]) == E.cases()["tile-8192o-kf"][2][0]
    assert E.fq(E.ladder_reads(33, 33)) == E.cases()["ladder-33-33"][2][0]
    assert list(E.hist_rows_files()) == E.cases()["hist_rows"][2]


def test_the_plans_of_the_ladders():
    assert E.ladder_lengths(31) == [1, 2, 3, 4, 5, 8, 9, 16, 17, 30, 31, 32]
    assert E.ladder_plan(31) == [(1, 1), (2, 2), (4, 7), (8, 13), (16, 25), (31, 78), (31, 0)]
    assert E.ladder_plan(33)[-3:] == [(32, 49), (33, 33), (33, 0)]  # the round at trim removes something at k = 33
    assert E.ladder_plan(1) == [(1, 1), (1, 0)] and E.ladder_plan(7) == [(1, 1), (2, 2), (4, 7), (7, 18), (7, 0)]


def test_the_restated_partitions():
    """kmeredgecases.pick_partitions on a hand-made set of bins, and the hash bin of two known keys"""
    import numpy as np
    import map_oracle
    bins = np.zeros(E.BINS, np.int64)
    bins[0], bins[1], bins[4095] = 3, 2, 4
    pre = np.concatenate(([0], np.cumsum(bins)))
    assert E.pick_partitions(pre, 21, 9 * 20) == (1, 9) and E.pick_partitions(pre, 21, 5 * 20) == (2, 5)
    assert E.pick_partitions(pre, 21, 4 * 20) == (4096, 4) and E.pick_partitions(pre, 21, 4 * 20 - 1) == (0, 0)
    assert E.pick_partitions(pre, 33, 4 * 36) == (4096, 4) and E.per_key(32) == 20 and E.per_key(33) == 36
    for key in (0, 12345678901234567, (1 << 64) - 1):
        assert E.kf_bin(key) == map_oracle.kf_hash(key) >> 52
    assert E.kf_bin(1 << 64) == map_oracle.kf_hash(0x9e3779b97f4a7c15) >> 52
