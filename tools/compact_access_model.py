#!/usr/bin/env python3
"""Wave-level memory requests and 64-byte sectors of k_compact per step, counted on the CPU from the oracle's tables: the
access pattern of the kernel up to profiles/r6_04 ("old": four lanes per edge, four rounds, order record -> id count -> ids in
16-byte pieces) and of the present one ("new": edge record as one 32-byte read, orders by slot, ids as a flat range).  A
request is one vector memory instruction of one wavefront with at least one active lane; its sectors are the distinct aligned
64-byte pieces its active lanes touch.  The chunk sums (the same in both) are left out.  Tables are taken as 64-byte aligned.

    python tools/compact_access_model.py [reads anchors rows seed]      (default: 20000 10000 100000 43, the cfg3 job)
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

CHUNK, ORD_ROUND, IDS_ROUND = 1024, 1024, 8192  # edges per workgroup; order slots and id dwords per round of the new moves


def _distinct(group, sector):
    """number of distinct (group, sector) pairs"""
    return len(np.unique(group.astype(np.int64) * (1 << 40) + sector.astype(np.int64)))


def _pieces(start, cnt):
    """the 16-byte pieces of runs of dwords (start, cnt): -> sectors they touch, one or two per piece"""
    n_p = (cnt + 3) // 4
    run = np.repeat(np.arange(len(cnt)), n_p)
    t = np.arange(int(n_p.sum())) - np.repeat(np.cumsum(n_p) - n_p, n_p)
    lo = start[run] + 4 * t
    hi = np.minimum(lo + 3, start[run] + cnt[run] - 1)
    return int(((hi * 4) // 64 - (lo * 4) // 64 + 1).sum())


def count(t):
    edges, orders = t["edges"], t["orders"]
    E, O, I = len(edges), len(orders), len(t["ids"])
    no = edges["order_cnt"].astype(np.int64)
    em = edges["em_off"].astype(np.int64)
    o_edge = np.repeat(np.arange(E), no)                       # edge of every order
    o_i = np.arange(O) - np.repeat(edges["order_off"].astype(np.int64), no)  # its place in the edge
    cnt = orders["ids_cnt"].astype(np.int64)
    dst = orders["ids_off"].astype(np.int64)
    ni = np.bincount(o_edge, weights=cnt, minlength=E).astype(np.int64)
    first = np.zeros(E, np.int64)
    first[1:] = np.cumsum(ni)[:-1]
    src = em[o_edge] + (dst - first[o_edge])                   # scratch: em_off + the order's place among the edge's ids
    waves = (E + 63) // 64
    out = {}

    # ---- old ----
    rd, rd_s, wr, wr_s = 0, 0, 0, 0
    rd += 3 * waves                                            # edge_norders, edge_nids, edges[].em_off: an edge per lane
    rd_s += 2 * ((E + 15) // 16) + (E + 1) // 2
    groups = (E + 15) // 16                                    # sixteen edges per wavefront and round
    wr += 3 * groups                                           # order_off, order_cnt, em_off: three partial stores
    wr_s += 3 * ((E + 1) // 2)
    g = o_edge // 16
    key = g * 65536 + o_i
    iters = len(np.unique(key))                                # iterations of the order loop over all groups = sum of max_no
    rd += iters
    wr += iters
    rd_s += O
    wr_s += O
    pc = (cnt + 3) // 4                                        # id pieces per order = iterations of its four lanes
    order = np.argsort(key, kind="stable")
    ks, ps = key[order], pc[order]
    lead = np.r_[True, ks[1:] != ks[:-1]]
    id_iters = int(np.maximum.reduceat(ps, np.flatnonzero(lead)).sum()) if O else 0
    rd += id_iters
    wr += id_iters
    rd_s += _pieces(src, cnt)
    wr_s += _pieces(dst, cnt)
    out["old"] = dict(read_requests=rd, read_sectors=rd_s, write_requests=wr, write_sectors=wr_s)

    # ---- new ----
    rd, rd_s, wr, wr_s = 0, 0, 0, 0
    rd += 2 * waves                                            # the edge record as two 16-byte halves
    rd_s += 2 * ((E + 1) // 2)
    wr += waves                                                # its second half, one store
    wr_s += (E + 1) // 2
    chunk_of_edge = np.arange(E) // CHUNK
    n_chunks = (E + CHUNK - 1) // CHUNK
    co = np.bincount(chunk_of_edge, weights=no, minlength=n_chunks).astype(np.int64)
    ci = np.bincount(chunk_of_edge, weights=ni, minlength=n_chunks).astype(np.int64)
    # orders: every wavefront of a round issues its load (a lane beyond the last slot reads the last slot); 16 slots a request
    rounds = (co + ORD_ROUND - 1) // ORD_ROUND
    real = (co + 15) // 16
    rd += int((rounds * (ORD_ROUND // 16)).sum())
    rd_s += O + int((rounds * (ORD_ROUND // 16) - real).sum())
    wr += int(real.sum())
    wr_s += O
    # ids: 64 consecutive dwords of the chunk's range a request
    rounds = (ci + IDS_ROUND - 1) // IDS_ROUND
    real = (ci + 63) // 64
    rd += int((rounds * (IDS_ROUND // 64)).sum())
    wr += int(real.sum())
    e_id = np.repeat(np.arange(E), ni)                         # edge of every id
    j = np.arange(I) - first[e_id]
    base_i = np.zeros(n_chunks, np.int64)
    base_i[1:] = np.cumsum(ci)[:-1]
    q = np.arange(I) - base_i[chunk_of_edge[e_id]]
    grp = chunk_of_edge[e_id] * (1 << 20) + q // 64
    rd_s += _distinct(grp, ((em[e_id] + j) * 4) // 64) + int((rounds * (IDS_ROUND // 64) - real).sum())
    wr_s += _distinct(grp, (np.arange(I) * 4) // 64)
    out["new"] = dict(read_requests=rd, read_sectors=rd_s, write_requests=wr, write_sectors=wr_s)
    out["job"] = dict(edges=E, orders=O, ids=I, chunks=int(n_chunks))
    return out


def main():
    import ms_oracle_ctypes as oracle
    from muchsalsa_amd import synth
    shape = [int(x) for x in sys.argv[1:5]] or [20_000, 10_000, 100_000, 43]
    oracle.build()
    c = count(oracle.overlap(synth.synth_rows(*shape)))
    print("job", c["job"])
    for k in ("old", "new"):
        print(k, c[k])
    for f in c["old"]:
        print("%-15s new / old = %.3f" % (f, c["new"][f] / max(c["old"][f], 1)))


if __name__ == "__main__":
    main()
