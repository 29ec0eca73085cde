#!/usr/bin/env python3
"""The chaining DP and the pair sweep of the chain kernels, counted from the source: the vector and LDS instructions one
wavefront issues per step of the DP and per step of the sweep in the kernels up to profiles/r6_07 ("before") and in the
present ones ("now"), over the sizes n of cfg3's edges.  A count by reading, written down before the counter passes of
profiles/r6_08; the ranges are what the reading leaves open.

  before, chain_body (k_chain), per DP step: 2 v_readlane_b32 (rl_f64(pop, k)) + v_add_f64 + v_add_co_u32 + v_cmp_gt_f64 +
          v_mov_b64 + v_mov_b32 = 7 vector instructions, no LDS instruction.
  now:    2 ds_bpermute_b32 (bpermute_f64, the source lane in the immediate offset) + the same five = 5 vector and 2 LDS
          instructions; per EIGHT steps one v_add_u32 (the address register) and one v_cndmask_b32 (the reversed word of
          the rows 32.. chosen at step 32: the compiler makes the branch a select); one v_mov_b32 in front of the loop.
  chain_sub_body<32>, per DP step, unchanged: group_bcast_f64<32, k> is two moves per half for k < 16 (row_bcast and the
          copy to the other row: 4 per step) and three for k >= 16 (row_bcast, the other row's bcast, v_permlane16_swap:
          6 per step), + the same five: 9 or 11 vector instructions.  (The issue estimated four for the broadcast.)
  nano_check<WF = true>, both bodies, per sweep step: t = lt_lo ? x : y is two v_cndmask_b32 per vertex, min(x, y) one
          v_min_f64: one less per vertex, two per step.  0 or 1 more may go with the select's condition (the compare
          feeds a ballot as well, so it stays): the range below.

The sizes: the oracle's edge table of a scaled sample of the workload (the generator keeps the density), or --em-cnt
FILE.npy: the em_cnt column of the edges dumped by `bench.py --dump-outputs`.  A wavefront of k_chain holds one edge of
33..64 rows; the band (B = 12) cuts its sweep to chain_band_pairs(n) pairs, 64 per step.  A wavefront of k_chain_sub_all
holds 64 / W edges of neighbouring sizes and runs its sweep to the largest of them, W pairs per group and step.  The
all-pairs shortcut takes 0.5 % of cfg3's edges (5,372 of 981,460: profiles/r6_07/bench_default.json) and the band falls
back on under 2 % of the banded ones: both left out.

    python tools/chain_dp_model.py [--scale 0.05] [--em-cnt edges_em_cnt.npy]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 12  # MSGPU_CHAIN_BAND


def band_pairs(n):
    return n * (n - 1) // 2 if n <= B + 1 else B * (B + 1) // 2 + (n - 1 - B) * B


def em_counts(scale, path):
    if path:
        return np.load(path).astype(np.int64)
    sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
    import bench
    import ms_oracle_ctypes as oracle
    from muchsalsa_amd import synth
    oracle.build()
    w = bench.WORKLOADS["cfg3"]
    rows = synth.synth_rows(int(w["n_reads"] * scale), w["read_len"], int(w["n_anchors"] * scale), w["seed"])
    return oracle.overlap(rows)["edges"]["em_cnt"].astype(np.int64)


def k_chain(ns):
    """per wavefront (= edge of 33..64 rows): (vector instructions shed low, high, LDS instructions added)"""
    steps = ns - 1
    eights = -(-steps // 8)
    dp_lo = 2 * steps - 2 * eights - 1
    dp_hi = 2 * steps - eights  # if the select at step 32 folds away
    sweep = -(-np.array([band_pairs(int(n)) for n in ns]) // 64)
    return dp_lo + 2 * sweep, dp_hi + 3 * sweep, 2 * steps, steps, sweep


def sub_all(ns):
    """k_chain_sub_all: the edges of 2..32 rows in size order, 64 / W of them per wavefront; per wavefront the sweep steps
    of its largest edge.  -> (wavefronts, vector instructions shed low, high) summed, and the DP's price today"""
    out = []
    for W, lo, hi in ((8, 2, 8), (16, 9, 16), (32, 17, 32)):
        c = np.sort(ns[(ns >= lo) & (ns <= hi)])
        G = 64 // W
        waves = -(-len(c) // G)
        if waves == 0:
            continue
        top = c[np.minimum(np.arange(waves) * G + G - 1, len(c) - 1)]
        sweep = -(-(top * (top - 1) // 2) // W)
        k = top - 1  # DP steps of the wavefront
        bcast = np.where(k <= 16, 4 * k, 64 + 6 * (k - 16)) if W == 32 else None
        out.append((W, waves, int(sweep.sum()), None if bcast is None else float(bcast.mean()), float(k.mean())))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--em-cnt", default=None)
    a = ap.parse_args()
    ns = em_counts(a.scale, a.em_cnt)
    big = ns[(ns >= 33) & (ns <= 64)]
    print("%d edges; %d of 33..64 rows (k_chain), mean n %.1f, median %d" % (len(ns), len(big), big.mean(), np.median(big)))
    lo, hi, lds, steps, sweep = k_chain(big)
    print("k_chain per wavefront: %.1f DP steps, %.1f sweep steps" % (steps.mean(), sweep.mean()))
    print("  part 1: vector instructions shed %.1f..%.1f, LDS instructions added %.1f" % (
        (lo - 2 * sweep).mean(), (hi - 3 * sweep).mean(), lds.mean()))
    print("  part 2: vector instructions shed %.1f..%.1f" % ((2 * sweep).mean(), (3 * sweep).mean()))
    print("  predicted fall of SQ_INSTS_VALU per wavefront: %.0f..%.0f (middle %.0f); SQ_INSTS_LDS rises by %.0f" % (
        lo.mean(), hi.mean(), (lo.mean() + hi.mean()) / 2, lds.mean()))
    tw = ts = 0
    for W, waves, sweep_sum, bcast, k in sub_all(ns):
        tw += waves
        ts += sweep_sum
        print("k_chain_sub_all, W = %2d: %d wavefronts, %.1f sweep steps and %.1f DP steps each%s" % (
            W, waves, sweep_sum / waves, k, "" if bcast is None else "; the DP's broadcast today: %.0f vector instructions" % bcast))
    print("  part 2: predicted fall of SQ_INSTS_VALU per wavefront of k_chain_sub_all: %.0f..%.0f" % (2 * ts / tw, 3 * ts / tw))


if __name__ == "__main__":
    main()
