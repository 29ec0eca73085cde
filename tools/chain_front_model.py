#!/usr/bin/env python3
"""The front of an edge in the chain kernels, counted from the source: the memory instructions one wavefront issues in its
element phase (from its first instruction to the two rows of every EdgeMatch in registers) and the levels of loads that
depend on each other, for the kernels up to profiles/r6_05 ("before": list entry -> edge record and candidate offset ->
candidate ranks and the reads' facts -> rows) and for the present ones ("now": descriptor -> candidate word and the reads'
facts -> rows).  k_chain takes what is wave-uniform through scalar loads, chain_sub_body<W> (k_chain_sub_all) per lane.  The
pair-table loads of the sweep are the same on both sides; their per-wavefront means come from the r6_05 counters
(SQ_INSTS_VMEM_RD per wavefront minus the element phase counted here).  k_chain's rows are as the disassembly has them: the
first version of this table took list[slot] for a vector load and predicted 13.3 vector reads per wavefront where 14.3 were
measured (profiles/r6_06/README.md); the kernel argument loads, which the scalar column leaves out, changed as well.

    python tools/chain_front_model.py
"""

# (name, vector loads, scalar loads, level) per wavefront; level = how many loads it has to wait for in a row, itself included
K_CHAIN = {
    "before": [("list[slot] (uniform address: the compiler makes it a scalar load)", 0, 1, 1),
               ("edges[e]: {v1, v2, em_off}, em_cnt", 0, 2, 2), ("edge_cand[e]", 0, 1, 2),
               ("read_cnt / read_len / read_off of v1, v2", 0, 6, 3), ("cand_j[cp + lane]", 1, 0, 3), ("cand_q[cp + lane]", 1, 0, 3),
               ("rows of v1 (2 x 16 bytes) and v2 (16 + 8 + 4 bytes)", 5, 0, 4)],
    "now": [("desc[blockIdx.x], two halves of four dwords around the n > 64 test", 0, 2, 1),
            ("read_cnt / read_len / read_off of v1, v2", 0, 6, 2), ("cand[cp + lane] = j | q << 16", 1, 0, 2),
            ("rows of v1 (2 x 16 bytes) and v2 (16 + 8 + 4 bytes)", 5, 0, 3)],
}
K_SUB = {
    "before": [("list[slot]", 1, 0, 1), ("edges[e]: {v1, v2, em_off}, em_cnt", 2, 0, 2), ("edge_cand[e]", 1, 0, 2),
               ("read_cnt / read_len / read_off of v1, v2", 6, 0, 3), ("cand_j[cp + sl]", 1, 0, 3),
               ("cand_q[cp + sl], and again behind the set-up", 2, 0, 3), ("rows of v1 and v2, 2 x 16 bytes each", 4, 0, 4)],
    "now": [("desc[slot], 2 x 16 bytes", 2, 0, 1),
            ("read_cnt / read_len / read_off of v1, v2", 6, 0, 2), ("cand[cp + sl] = j | q << 16", 1, 0, 2),
            ("rows of v1 and v2, 2 x 16 bytes each", 4, 0, 3)],
}
# profiles/r6_05/pmc_summary.csv: SQ_INSTS_VMEM_RD and SQ_INSTS_SMEM per wavefront
MEASURED_BEFORE = {"k_chain": (15.3, 20.0), "k_chain_sub_all": (27.2, 11.5)}


def totals(rows):
    return sum(r[1] for r in rows), sum(r[2] for r in rows), max(r[3] for r in rows)


def main():
    print("%-16s %-7s %7s %7s %7s   %s" % ("kernel", "tree", "vector", "scalar", "levels", "predicted VMEM_RD / SMEM per wavefront"))
    for name, tab in (("k_chain", K_CHAIN), ("k_chain_sub_all", K_SUB)):
        v0, s0, _ = totals(tab["before"])
        m_v, m_s = MEASURED_BEFORE[name]
        for tree in ("before", "now"):
            v, s, lv = totals(tab[tree])
            pred = "%.1f / %.1f" % (m_v - v0 + v, m_s - s0 + s)
            print("%-16s %-7s %7d %7d %7d   %s%s" % (name, tree, v, s, lv, pred, "  (measured, r6_05)" if tree == "before" else ""))
        print("  pair-table and other loads outside the element phase: %.1f vector per wavefront (both trees)" % (m_v - v0))
    for name, tab in (("k_chain", K_CHAIN), ("chain_sub_body<W>", K_SUB)):
        for tree in ("before", "now"):
            print("\n%s, %s:" % (name, tree))
            for what, v, s, lv in tab[tree]:
                print("  level %d  %d vector %d scalar  %s" % (lv, v, s, what))


if __name__ == "__main__":
    main()
