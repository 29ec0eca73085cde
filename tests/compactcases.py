"""Row tables aimed at k_compact's moves: the chunk of 1024 edges, the slot-to-edge search over the chunk's orders, and the flat
copy of the chunk's ids (consecutive lanes, consecutive dwords; 8 x 1024 dwords per round of the copy, 4 x 256 order slots per
round of the order move).

Edge e lies between reads 2e and 2e + 1 and has anchors of its own, ids in first-line order as in extremecases: the edge table is
in the order of the specs, so a spec's place decides the chunk and the position of its orders and ids in the flat ranges.

A spec is (plus, minus): `plus` anchors on the same strand of both reads and `minus` anchors with the second read reversed, in
turn along the first read.  Every chain is compatible, so the oracle emits one order per direction present, minus first, with
as many ids as the direction has anchors: (n, 0) is an edge of one order and one run of n ids, (a, b) one of two orders whose
ids are one run of a + b.  (The rows of a two-direction edge score below the primary threshold and a and b are both 1 or both
above 1: a primary path, or a longer one, would have the other direction's path filtered out, src/main.cpp:355-387.)
test_compact_workloads.py asserts all of that on the oracle's tables.

What no row table can hold: an edge WITHOUT an order.  Each direction that has an EdgeMatch yields a path, the filters of
src/main.cpp:355-387 keep at least one path of the union, and the four cases of getOverlap (ol.cpp:53-101) are exhaustive for
numbers that are not NaN; the overhangs are sums of int32 coordinates and quotients whose divisor rRatio has a positive numerator
(an EdgeMatch exists only where the two unitig intervals overlap, MatchMap.cpp:192), so no NaN arises.  The entries of no order
that k_compact's search does meet are the ones behind the last edge of the job's last chunk; the edge counts 1, 1023, 1025 and
2049 leave 1023, 1, 1023 and 1023 of them.
"""
import numpy as np

import extremecases as X
from muchsalsa_amd.synth import ROW_DTYPE

CHUNK = 1024        # edges per workgroup of k_compact
IDS_ROUND = 8192    # dwords per round of the flat id copy
STEP = 800


def rows_of(specs):
    out, anchor, line = [], 0, 0
    for e, (plus, minus) in enumerate(specs):
        n = plus + minus
        L = 4000 + STEP * n
        assert not (plus and minus) or (plus == minus == 1) or (plus > 1 and minus > 1)
        score = 400 if plus and minus else 500
        n_fwd = 0
        for j in range(n):
            fwd = (j % 2 == 0 and n_fwd < plus) or (j - n_fwd) >= minus
            n_fwd += fwd
            p0, p1 = 500 + STEP * j, 700 + STEP * j
            q1 = p1 if fwd else L - 600 - p1
            out.append(X.row(anchor + j, 2 * e, L, 0, 599, p0, p0 + 599, score, line, True))
            out.append(X.row(anchor + j, 2 * e + 1, L, 0, 599, q1, q1 + 599, score, line + 1, fwd))
            line += 2
        anchor += n
    return X.check_int32(np.array(out, dtype=ROW_DTYPE))


def count_specs(n_edges):
    """n_edges edges of two anchors; every fifth has one anchor per direction: two orders of one id instead of one order of two.
    A full chunk of them holds 1024 edges and 1229 orders: more than one round of the order move."""
    return [(1, 1) if e % 5 == 3 else (2, 0) for e in range(n_edges)]


# id runs of 1, 2, 63, 64 and 65; 63 lies on [3, 66) across dword 64; an edge of 70 EdgeMatches (k_chain_big) with a run of 70;
# twelve runs of 60 bring the range to 985, where a run of 64 lies across 1024; 120 runs of 61 take it past 8192 = the second
# round of the copy.  Edges of 12 and 24 rows for the 16- and 32-wide classes.
RUN_SPECS = [(1, 0), (2, 0), (63, 0), (64, 0), (65, 0), (70, 0)] + [(60, 0)] * 12 + [(64, 0)] + [(61, 0)] * 120 + [(12, 0), (24, 0)]

# 0 orders cannot be built (see above); 1 order, 2 orders by two directions of one, two and many anchors, in turn with edges of one
# order, and beside each other: the search crosses edges of several slots in a row
MIX_SPECS = [(2, 0), (1, 1), (3, 0), (2, 2), (5, 3), (1, 0), (1, 1), (1, 1), (20, 20), (4, 0), (33, 33), (2, 0), (6, 12)] * 3


def alt_rows():
    """edges whose alternative path is kept (extremecases._alt_edge with a side chain as strong as the main one): two orders of
    ONE direction"""
    out, anchor, line, read = [], 0, 0, 0
    for m, q in ((4, 4), (8, 8), (3, 3)):
        for plus in (True, False):
            line = X._alt_edge(out, m, q, read, anchor, line, plus)
            anchor, read = anchor + m + q, read + 2
    return X.check_int32(np.array(out, dtype=ROW_DTYPE))


def mix_rows():
    return X.join([rows_of(MIX_SPECS), alt_rows(), rows_of(MIX_SPECS[:5])])


WORKLOADS = {
    "count_1": lambda: rows_of(count_specs(1)),
    "count_1023": lambda: rows_of(count_specs(1023)),
    "count_1024": lambda: rows_of(count_specs(1024)),
    "count_1025": lambda: rows_of(count_specs(1025)),
    "count_2049": lambda: rows_of(count_specs(2049)),
    "runs": lambda: rows_of(RUN_SPECS),
    "mix": mix_rows,
}


def edge_runs(t):
    """per edge of a table set: (orders, ids, first id's position in the id table); asserts that an edge's ids are one run in
    the order of its orders, which is what the flat copy relies on"""
    out = []
    for e in t["edges"]:
        o = t["orders"][int(e["order_off"]):int(e["order_off"]) + int(e["order_cnt"])]
        first = int(o["ids_off"][0]) if len(o) else 0
        pos = first
        for x in o:
            assert int(x["ids_off"]) == pos
            pos += int(x["ids_cnt"])
        out.append((len(o), pos - first, first))
    return out


def straddles(runs, boundary, period=None):
    """the id runs (edge-wise) that lie across `boundary` (or across any multiple of `period`)"""
    hit = []
    for _, n, first in runs:
        if n < 2:
            continue
        if period:
            if first // period != (first + n - 1) // period:
                hit.append((first, n))
        elif first < boundary <= first + n - 1:
            hit.append((first, n))
    return hit
