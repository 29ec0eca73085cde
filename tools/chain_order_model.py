#!/usr/bin/env python3
"""The order loop of the chain kernels, counted from the source: the vector instructions one wavefront issues per trip of the
loop that emits an order, and per path for the truncation of its score, in the kernels up to profiles/r6_06 ("before": the
overhangs gathered into every lane, getOverlap's cases on wave-uniform values, the 64-byte msgpu_order assembled in lane 0)
and in the present ones ("now": a RAW record, the lanes f and l store their own numbers, k_compact finishes it).  A count by
reading: one line per source construct with the instructions it needs on gfx950 (a 64-bit select = two v_cndmask, an fp64
compare with two wave-uniform operands = the compare plus the moves that bring one operand back into vector registers, the
fp64 -> uint64 conversion = trunc, ldexp, floor, fma and two cvt).  Written down before the counter passes of
profiles/r6_07; the ranges are what the reading leaves open.

    python tools/chain_order_model.py
"""

# (what, low, high) vector instructions
BODY = {  # chain_body (k_chain): per emitted order
    "before": [("rl_f64 of L1, R1, L2, R2 (six, eight on a reverse path): v_readlane", 12, 16),
               ("the gathered values back in vector registers for the fp64 compares (one scalar operand per instruction)", 4, 8),
               ("eight fp64 compares of the four cases", 8, 8), ("four fp64 subtractions", 4, 4),
               ("lo, ro selected through the cases (64-bit selects)", 8, 12),
               ("the 16 dwords of the record into lane 0's registers", 10, 12)],
    "now": [("the v2 side by direction: two 64-bit selects", 4, 4), ("lane == f, lane == l", 2, 2),
            ("two unordered compares", 2, 2), ("quarters 0 and 2 into lane 0's registers", 5, 6),
            ("store addresses of the quarters", 2, 4)],
}
SUB = {  # chain_sub_body<32>: per trip of the order loop (all groups of the wavefront at once)
    "before": [("LDS addresses of the entries of lanes f and l in s_keep", 4, 4), ("eight fp64 compares", 8, 8),
               ("four fp64 subtractions", 4, 4), ("have, fl, lo, ro selected per lane through the cases", 16, 20),
               ("flags, start, end and the rest of the record", 10, 12)],
    "now": [("the v2 side by direction: two 64-bit selects", 4, 4), ("sl == f, sl == l", 2, 2),
            ("two unordered compares", 2, 2), ("raw flags, quarters 0 and 2", 6, 7), ("store addresses of the quarters", 3, 4)],
}
TRUNC = (6, 6)  # static_cast<uint64_t>(double), per path written by paths_of_direction / per trip of paths_of_direction_sub

# per wavefront, from cfg3 (profiles/r6_06): 1.03 M orders on 0.98 M edges; k_chain takes an edge per wavefront; a wavefront
# of k_chain_sub_all runs its order loop to the largest number of kept paths among its two to eight groups
TRIPS = {"k_chain": (1.0, 1.1), "k_chain_sub_all": (1.1, 1.5)}
PATHS = {"k_chain": (1.0, 1.5), "k_chain_sub_all": (1.5, 2.5)}  # executions of the truncation per wavefront
MEASURED_BEFORE = {"k_chain": 1202, "k_chain_sub_all": 1171}    # SQ_INSTS_VALU per wavefront, profiles/r6_06


def span(rows):
    return sum(r[1] for r in rows), sum(r[2] for r in rows)


def main():
    for name, tab, kern in (("chain_body", BODY, "k_chain"), ("chain_sub_body<32>", SUB, "k_chain_sub_all")):
        b, n = span(tab["before"]), span(tab["now"])
        print("%s, per trip of the order loop: before %d..%d, now %d..%d vector instructions" % (name, b[0], b[1], n[0], n[1]))
        for tree in ("before", "now"):
            for what, lo, hi in tab[tree]:
                print("    %-6s %2d..%2d  %s" % (tree, lo, hi, what))
        lo = (b[0] - n[1]) * TRIPS[kern][0] + TRUNC[0] * PATHS[kern][0]
        hi = (b[1] - n[0]) * TRIPS[kern][1] + TRUNC[1] * PATHS[kern][1]
        m = MEASURED_BEFORE[kern]
        print("  %s: predicted fall of SQ_INSTS_VALU per wavefront %.0f..%.0f (middle %.0f): %d -> %.0f..%.0f\n"
              % (kern, lo, hi, (lo + hi) / 2, m, m - hi, m - lo))


if __name__ == "__main__":
    main()
