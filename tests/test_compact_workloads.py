"""What the workloads of test_gpu_compact_moves.py hold, asserted on the oracle's tables without a GPU: the chunks, the orders per
edge, the id runs and where they lie relative to the 64-lane wavefront, the 1024-dword stride of the flat id copy and its round of
8192 dwords.  A claim of a GPU case that is not asserted here does not count."""
import numpy as np
import pytest

import compactcases as CC


@pytest.fixture(scope="module")
def tables(oracle):
    cache = {}

    def get(name):
        if name not in cache:
            rows = CC.WORKLOADS[name]()
            cache[name] = (rows, oracle.overlap(rows))
        return cache[name]
    return get


def chunks(n_edges):
    return (n_edges + CC.CHUNK - 1) // CC.CHUNK


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2049])
def test_edge_counts(tables, n):
    rows, t = tables("count_%d" % n)
    print("count", n, "rows", len(rows), "orders", len(t["orders"]), "ids", len(t["ids"]))
    assert len(t["edges"]) == n and len(rows) == 4 * n and len(rows) < 10_000
    assert [int(c) for c in t["edges"]["em_cnt"]] == [2] * n          # edges of two anchors
    assert chunks(n) == {1: 1, 1023: 1, 1024: 1, 1025: 2, 2049: 3}[n]  # 2049: a chunk with more than one chunk before it
    runs = CC.edge_runs(t)
    assert [r[0] for r in runs] == [2 if e % 5 == 3 else 1 for e in range(n)]
    assert all(r[1] == 2 for r in runs) and len(t["ids"]) == 2 * n
    # entries behind the last edge of the last chunk: the only entries of no order the search meets
    assert chunks(n) * CC.CHUNK - n == {1: 1023, 1023: 1, 1024: 0, 1025: 1023, 2049: 1023}[n]
    if n >= 1024:  # a full chunk: more order slots than one round of the order move (4 x 256)
        assert sum(r[0] for r in runs[:CC.CHUNK]) == 1229 > 1024
    assert int(t["edges"]["order_cnt"].min()) >= 1  # (see compactcases: no row table gives an edge without an order)


def test_id_runs(tables):
    rows, t = tables("runs")
    print("runs rows", len(rows), "edges", len(t["edges"]), "ids", len(t["ids"]))
    runs = CC.edge_runs(t)
    assert len(runs) == len(CC.RUN_SPECS) and chunks(len(runs)) == 1
    assert [r[:2] for r in runs] == [(1, p) for p, _ in CC.RUN_SPECS]  # one order, one run of as many ids as anchors
    assert [r[1] for r in runs[:6]] == [1, 2, 63, 64, 65, 70]
    assert int(t["edges"]["em_cnt"][5]) == 70 and runs[5][1] == 70  # more than 64 EdgeMatches: k_chain_big, a run above 64
    assert runs[2][1:] == (63, 3) and (3, 63) in CC.straddles(runs, 64)   # the run of 63 lies across the first wavefront's end
    assert (66, 64) in CC.straddles(runs, 128) and (130, 65) in CC.straddles(runs, 192)
    assert CC.straddles(runs, 1024) == [(985, 64)]                          # across the copy's 1024-dword stride
    assert len(t["ids"]) > CC.IDS_ROUND and len(CC.straddles(runs, CC.IDS_ROUND)) == 1  # across the copy's round of 8192 dwords
    assert len(CC.straddles(runs, None, 64)) > 100
    sizes = sorted(set(int(c) for c in t["edges"]["em_cnt"]))
    assert sizes == [1, 2, 12, 24, 60, 61, 63, 64, 65, 70]  # every chain kernel: 8-, 16-, 32-wide, k_chain, k_chain_big


def test_order_mix(tables):
    rows, t = tables("mix")
    runs = CC.edge_runs(t)
    cnt = [r[0] for r in runs]
    print("mix rows", len(rows), "edges", len(runs), "orders per edge", sorted(set(cnt)))
    assert chunks(len(runs)) == 1
    n_mix = len(CC.MIX_SPECS)
    assert cnt[:n_mix] == [2 if (p and m) else 1 for p, m in CC.MIX_SPECS]  # both directions: two orders
    assert [r[1] for r in runs[:n_mix]] == [p + m for p, m in CC.MIX_SPECS]   # their ids: ONE run
    assert cnt[n_mix:n_mix + 6] == [2] * 6                                       # alternatives kept: two orders of one direction
    assert any(a >= 2 and b >= 2 for a, b in zip(cnt, cnt[1:])) and any(a == 1 and b >= 2 for a, b in zip(cnt, cnt[1:]))
    assert min(cnt) == 1  # no edge without an order exists (compactcases)
    both = [e for e, (p, m) in enumerate(CC.MIX_SPECS) if p and m]
    for e in both:  # minus first, then plus, the ids in that order
        o = t["orders"][int(t["edges"]["order_off"][e]):][:2]
        assert [int(x) for x in o["ids_cnt"]] == [CC.MIX_SPECS[e][1], CC.MIX_SPECS[e][0]]


def test_no_order_is_not_reachable(tables, oracle):
    """every edge of every workload, and of a synthetic job, has an order: the chunk without any order and the edge without
    one that the kernel's search steps over exist only as the entries behind the job's last edge"""
    from muchsalsa_amd import synth
    for name in CC.WORKLOADS:
        assert int(tables(name)[1]["edges"]["order_cnt"].min()) >= 1, name
    t = oracle.overlap(synth.synth_rows(2000, 5000, 10000, 7))
    assert int(t["edges"]["order_cnt"].min()) >= 1 and int(t["orders"]["ids_cnt"].min()) >= 1


def test_relaunch_sizes(tables):
    """the relaunch case: a job of one edge, then one whose tables cannot fit what the first left (a buffer grows by an eighth)"""
    small, big = tables("count_1")[1], tables("count_2049")[1]
    assert len(big["orders"]) > 100 * len(small["orders"]) and len(big["ids"]) > 100 * len(small["ids"])
