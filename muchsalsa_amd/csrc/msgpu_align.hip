// msgpu_align.hip -- the wavefront alignment kernels: the banded edit distance in two forms, the edit script of a pair whose
// distance is known (rule 10) and the extension with a free end (rule 11), with their launchers.  They take device pointers
// and a stream and need nothing of a sequence store: msgpu_seq.hip's entry points and the mapper (msgpu_map.hip) launch them.
// The three furthest-reaching routines are built from one set of pieces ("the shared pieces"):
// fr_neighbours, fr_slide_row, fr_candidates, fr_store_row, fr_table_fence, fr_walk_back, and fr_wave_pairs for the two
// kernel shapes.  Kernel rules: vector stores and vector atomics only; no inline asm.
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "msgpu.h"
#include "msgpu_internal.h"

// =====================================================================================================================
// banded edit distance
// =====================================================================================================================
//
// The reference contains no sequence-level alignment; north_star asks for consensus sequences "within a
// stated edit-distance tolerance" of the reference's, so the tolerance needs a meter: this kernel measures the
// Levenshtein distance of pairs of sequences (e.g. our contig vs. another build's contig, or a query vs. its window of
// the target given by align.paf).  Unit costs, global alignment, band |j - i| <= W: exact whenever the true distance is
// <= W, otherwise reported as W + 1.
//
// One wavefront per pair.  The DP runs along anti-diagonals t = i + j: cell (i, j) on diagonal k = j - i needs
//   up   (i-1, j)   = diagonal k+1, anti-diagonal t-1
//   left (i, j-1)   = diagonal k-1, anti-diagonal t-1
//   diag (i-1, j-1) = diagonal k,   anti-diagonal t-2
// so one value per diagonal is all the state there is, and only diagonals with k = t (mod 2) are active in step t.
// Each lane owns four consecutive diagonals (two active per step), exchanges its edge values with the neighbour lanes
// by wavefront shuffle once per step, and reads the bases from LDS where both sequences were staged.

namespace msgpu {

constexpr int      ED_DPL   = 4;                 // diagonals per lane
constexpr int      ED_NDIAG = 64 * ED_DPL;       // 256 diagonals: k in [-128, 127]
static_assert(ED_MAXW < ED_NDIAG / 2, "the band lies within the diagonals");
#ifndef MSGPU_ED_LDS
#define MSGPU_ED_LDS (12 * 1024)
#endif
constexpr uint32_t ED_LDS   = MSGPU_ED_LDS; // bytes of LDS per sequence (12 KiB: 3 workgroups per CU; 24 KiB left one and
                                            // ran 2.5x slower on 7 kb queries); longer sequences stay in global memory
constexpr uint32_t ED_INF   = 0x3fffffffu;

template <bool IN_LDS>
__device__ __forceinline__ uint32_t edit_distance_wave(const uint8_t *a, uint32_t n, const uint8_t *b, uint32_t m,
                                                       uint32_t W, const uint8_t *la, const uint8_t *lb) {
  const int lane = threadIdx.x & 63;
  const int k0   = lane * ED_DPL - ED_NDIAG / 2; // first diagonal of this lane
  uint32_t  val[ED_DPL];
#pragma unroll
  for (int c = 0; c < ED_DPL; ++c) {
    const int k = k0 + c;
    val[c]      = (static_cast<uint32_t>(k < 0 ? -k : k) <= W) ? static_cast<uint32_t>(k < 0 ? -k : k) : ED_INF;
  }
  const int total = static_cast<int>(n + m);
  for (int t = 2; t <= total; ++t) {
    // values of the neighbouring lanes' edge diagonals (computed in step t-1, or boundary / INF)
    const uint32_t from_left  = __shfl_up(val[ED_DPL - 1], 1);  // diagonal k0 - 1
    const uint32_t from_right = __shfl_down(val[0], 1);         // diagonal k0 + ED_DPL
    const uint32_t nb_lo      = lane == 0 ? ED_INF : from_left;
    const uint32_t nb_hi      = lane == 63 ? ED_INF : from_right;
    const int      par        = (t - k0) & 1; // active diagonals: c = par, par + 2
#pragma unroll
    for (int cc = 0; cc < ED_DPL; cc += 2) {
      // written so that c is a compile-time pair {cc, cc+1} selected by `par` without dynamic register indexing
      const int      k_even = k0 + cc, k_odd = k0 + cc + 1;
      const int      k      = par ? k_odd : k_even;
      const uint32_t ak     = static_cast<uint32_t>(k < 0 ? -k : k);
      const int      i = (t - k) >> 1, j = (t + k) >> 1;
      const bool     ok = ak <= W && i >= 1 && j >= 1 && i <= static_cast<int>(n) && j <= static_cast<int>(m);
      // neighbours k-1 / k+1
      uint32_t left, up, self;
      if (!par) { // c = cc: left = (cc == 0 ? nb_lo : val[cc-1]), up = val[cc+1]
        left = cc == 0 ? nb_lo : val[cc - 1];
        up   = val[cc + 1];
        self = val[cc];
      } else { // c = cc+1: left = val[cc], up = (cc+2 == ED_DPL ? nb_hi : val[cc+2])
        left = val[cc];
        up   = cc + 2 == ED_DPL ? nb_hi : val[cc + 2];
        self = val[cc + 1];
      }
      uint32_t nv = self;
      if (ok) {
        const uint8_t ca = IN_LDS ? la[i - 1] : a[i - 1];
        const uint8_t cb = IN_LDS ? lb[j - 1] : b[j - 1];
        nv               = min(min(up, left) + 1u, self + (ca != cb ? 1u : 0u));
      }
      if (!par)
        val[cc] = nv;
      else
        val[cc + 1] = nv;
    }
  }
  // D[n][m] lives on diagonal k* = m - n
  const int ks = static_cast<int>(m) - static_cast<int>(n);
  if (static_cast<uint32_t>(ks < 0 ? -ks : ks) > W) return W + 1;
  const int idx = ks + ED_NDIAG / 2, src_lane = idx / ED_DPL, c = idx % ED_DPL;
  uint32_t  v   = c == 0 ? val[0] : c == 1 ? val[1] : c == 2 ? val[2] : val[3];
  v             = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), src_lane));
  return v > W ? W + 1 : v;
}

__global__ __launch_bounds__(128) void k_edit_distance_dp(const uint8_t *base_a, const uint8_t *base_b,
                                                       const msgpu_align_pair *pairs, uint32_t n_pairs, uint32_t W,
                                                       uint32_t *out) {
  __shared__ uint8_t s_a[2][ED_LDS], s_b[2][ED_LDS];
  const int      wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t p    = blockIdx.x * 2 + wave;
  if (p >= n_pairs) return;
  const msgpu_align_pair pr = pairs[p];
  const uint8_t *a = base_a + pr.a_off, *b = base_b + pr.b_off;
  uint32_t       d;
  if (pr.a_len <= ED_LDS && pr.b_len <= ED_LDS) {
    for (uint32_t i = lane; i < pr.a_len; i += 64) s_a[wave][i] = a[i];
    for (uint32_t i = lane; i < pr.b_len; i += 64) s_b[wave][i] = b[i];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    d = edit_distance_wave<true>(a, pr.a_len, b, pr.b_len, W, s_a[wave], s_b[wave]);
  } else {
    d = edit_distance_wave<false>(a, pr.a_len, b, pr.b_len, W, nullptr, nullptr);
  }
  if (lane == 0) out[p] = d;
}

// ---------------------------------------------------------------------------------------------------------------------
// The same distance by furthest-reaching points (Ukkonen 1985, Myers 1986): the DP over (edits e, diagonal k) instead of
// over (i, j).  F_e[k] = the largest i such that a[0, i) and b[0, i + k) are within e edits:
//     F_e[k] = slide(max(F_{e-1}[k] + 1, F_{e-1}[k-1], F_{e-1}[k+1] + 1)),   slide(i) = i + |common prefix of a[i..), b[i+k..)|
// and the distance is the first e with F_e[m - n] = n.  What k_edit_distance_dp spends on (n + m) anti-diagonal steps of
// 2W + 1 cells each, this form spends on at most W + 1 steps of 2e + 1 diagonals plus the slides -- for the pairs the
// meter exists for (a query against its window of the contig: a handful of edits in 7 kb) one slide over the sequence.
// The result is the same number for every input: the banded DP gives min(d, W + 1) because a path of d <= W edits never
// leaves the band, and so does this (tests: both kernels against the full-DP oracle and against each other).
//
// One wavefront per pair.  Lane l owns the diagonals k = l + 64 c - 128, c = 0..3 (neighbouring diagonals in neighbouring
// lanes: one shuffle per side and step).  A slide starts lane-local, 8 bytes per comparison; a lane that is still
// matching after 16 bytes hands its diagonal to the whole wavefront, which compares 512 bytes per round (8 per lane,
// first mismatch by ballot) -- the long slides of near-identical pairs run at the wavefront's width, not one lane's.
// No LDS: every base is read about once, straight from HBM/L2 (staging would be a second pass); 8 waves per SIMD.
// ---------------------------------------------------------------------------------------------------------------------

constexpr int FR_NONE = -(1 << 30);

// length of the common prefix of pa[0, valid) and pb[0, valid), valid <= 8 (nothing behind `valid` is read).  REV: the same
// run read backwards, pa[-1 - r] against pb[-1 - r]: an 8-byte load that ends at the position, and the leading zero bytes of
// the difference (nothing in front of pa[-valid] is read)
template <bool REV = false>
__device__ __forceinline__ int match_run8(const uint8_t *pa, const uint8_t *pb, int valid) {
  if (valid >= 8) {
    uint64_t x, y;
    __builtin_memcpy(&x, REV ? pa - 8 : pa, 8);
    __builtin_memcpy(&y, REV ? pb - 8 : pb, 8);
    const uint64_t d = x ^ y;
    if (REV) return d ? (__builtin_clzll(d) >> 3) : 8;
    return d ? (__builtin_ctzll(d) >> 3) : 8;
  }
  int r = 0;
  if (REV) {
    while (r < valid && pa[-1 - r] == pb[-1 - r]) ++r;
    return r;
  }
  while (r < valid && pa[r] == pb[r]) ++r;
  return r;
}

// The slides of one row, shared by the distance and the script kernels: every lane's points nf[c] (negative: none) on the
// diagonals |k| <= R move along the common prefix of a[x..) and b[x + k..), lane-local first, then at the wavefront's width.
// REV (rule 11's left flanks): byte i of a sequence is base[-1 - i], a and b name the byte behind their flank
template <bool REV = false>
__device__ __forceinline__ void fr_slide_row(const uint8_t *a, int n, const uint8_t *b, int m, int R, int lane, int (&nf)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (!(64 * c - 128 <= R && 64 * c - 65 >= -R)) continue; // (uniform: none of this c's diagonals is in reach)
    const int k = lane + 64 * c - 128;
    int       x = nf[c];
    bool      more = false;
    if (x >= 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int valid = min(8, min(n - x, m - (x + k)));
        const int run   = match_run8<REV>(REV ? a - x : a + x, REV ? b - (x + k) : b + (x + k), valid);
        x += run;
        more = run == 8;
        if (!more) break;
      }
    }
    unsigned long long mask = __ballot(more);
    while (mask) { // the diagonals that keep matching, one after the other at the wavefront's width
      const int L = __builtin_ctzll(mask);
      mask &= mask - 1;
      int       xs = __shfl(x, L);
      const int kk = L + 64 * c - 128;
      for (;;) {
        const int px    = xs + 8 * lane;
        const int valid = min(8, min(n - px, m - (px + kk)));
        const int run   = valid > 0 ? match_run8<REV>(REV ? a - px : a + px, REV ? b - (px + kk) : b + (px + kk), valid) : 0;
        const unsigned long long stop = __ballot(run < 8);
        if (stop) {
          const int F = __builtin_ctzll(stop);
          xs += 8 * F + __shfl(run, F);
          break;
        }
        xs += 512;
      }
      if (lane == L) x = xs;
    }
    nf[c] = x;
  }
}

// the points of the row before on the diagonals k - 1 (lo) and k + 1 (hi) of this lane's diagonal k = lane + 64 c - 128: the
// neighbour lanes' fr[c], and across the four diagonals a lane owns lane 63's fr[c - 1] and lane 0's fr[c + 1].  (Returned by
// value: with two reference parameters k_edit_distance did not compile to the code it had with the block written out.)
struct FrNeighbours {
  int lo, hi;
};
__device__ __forceinline__ FrNeighbours fr_neighbours(const int (&fr)[4], int c, int lane) {
  int       lo = __shfl_up(fr[c], 1), hi = __shfl_down(fr[c], 1);
  const int lo_edge = c > 0 ? __shfl(fr[c > 0 ? c - 1 : 0], 63) : FR_NONE;
  const int hi_edge = c < 3 ? __shfl(fr[c < 3 ? c + 1 : 3], 0) : FR_NONE;
  if (lane == 0) lo = lo_edge;
  if (lane == 63) hi = hi_edge;
  return FrNeighbours{lo, hi};
}

__device__ __forceinline__ uint32_t edit_distance_fr_wave(const uint8_t *a, int n, const uint8_t *b, int m, int W) {
  const int lane = threadIdx.x & 63;
  const int ks   = m - n;
  if ((ks < 0 ? -ks : ks) > W) return static_cast<uint32_t>(W + 1);
  int fr[4] = {FR_NONE, FR_NONE, FR_NONE, FR_NONE};
  for (int e = 0; e <= W; ++e) {
    int nf[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = lane + 64 * c - 128;
      int       x;
      if (e == 0) {
        x = k == 0 ? 0 : FR_NONE;
      } else {
        const FrNeighbours nb = fr_neighbours(fr, c, lane);
        x = max(max(fr[c] + 1, nb.lo), nb.hi + 1);
        const int ak = k < 0 ? -k : k;
        if (ak > W || ak > e) x = FR_NONE;
        x = min(x, min(n, m - k));
        if (x < 0 || x + k < 0) x = FR_NONE;
      }
      nf[c] = x;
    }
    fr_slide_row(a, n, b, m, e < W ? e : W, lane, nf);
#pragma unroll
    for (int c = 0; c < 4; ++c) fr[c] = nf[c];
    const int slot = ks + 128, cs = slot >> 6;
    const int v    = __shfl(cs == 0 ? fr[0] : cs == 1 ? fr[1] : cs == 2 ? fr[2] : fr[3], slot & 63);
    if (v >= n) return static_cast<uint32_t>(e);
  }
  return static_cast<uint32_t>(W + 1);
}

__global__ __launch_bounds__(256) void k_edit_distance(const uint8_t *base_a, const uint8_t *base_b,
                                                       const msgpu_align_pair *pairs, uint32_t n_pairs, uint32_t W,
                                                       uint32_t *out) {
  const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (p >= n_pairs) return; // (whole wavefronts leave)
  const msgpu_align_pair pr = pairs[p];
  const uint32_t d = edit_distance_fr_wave(base_a + pr.a_off, static_cast<int>(pr.a_len), base_b + pr.b_off,
                                           static_cast<int>(pr.b_len), static_cast<int>(W));
  if ((threadIdx.x & 63) == 0) out[p] = d;
}

void launch_edit_distance_pairs(hipStream_t st, const uint8_t *d_a, const uint8_t *d_b, const msgpu_align_pair *d_pairs, uint32_t n,
                                uint32_t band, uint32_t *d_out, bool dp) {
  if (!n) return;
  if (dp) hipLaunchKernelGGL(k_edit_distance_dp, dim3((n + 1) / 2), dim3(128), 0, st, d_a, d_b, d_pairs, n, band, d_out);
  else hipLaunchKernelGGL(k_edit_distance, dim3((n + 3) / 4), dim3(256), 0, st, d_a, d_b, d_pairs, n, band, d_out);
}

// ---------------------------------------------------------------------------------------------------------------------
// The edit script of a pair whose distance d <= band is known (include/msgpu.h, "unitig-to-read mapping", rule 10): the
// furthest-reaching table once more, rows 0..d, this time with rule 10's validity tests (only candidates that stay inside
// the matrix enter) and remembered: cell (e, k) is word e * e + k + e of a table of (d + 1)^2 words and holds op << 30 | G.
// The walk back from (d, m - n) is d dependent reads of that table: every lane follows it (the address is uniform), lane 0
// writes word e of the script.  Two classes of pairs: d <= ES_LDS_MAXD keeps the table in LDS, 4 KiB per wavefront, four
// wavefronts to a workgroup (16 KiB of the CU's 160 KiB: LDS does not limit the waves per SIMD; the VGPRs do, see the
// table of resources in DESIGN.md section 12); a larger d keeps it in a slot of (band + 1)^2 words of a slab in device
// memory, one slot per wavefront, and the wavefronts go through their class's pairs with the stride of the slots, so the
// slab does not grow with the input (a band of at most ES_LDS_MAXD has no such pairs and no slab).
// What the table must satisfy because d is the pair's distance (|m - n| <= d, G_d[m - n] = n, every op of the walk leads
// into row e - 1) is tested where a read or a write depends on it, and a pair that fails a test is counted in
// cnt[ES_CNT_BROKEN], which the callers report: nothing is skipped silently.
// ---------------------------------------------------------------------------------------------------------------------

constexpr int      ES_LDS_MAXD = 31;          // (ES_LDS_MAXD + 1)^2 words = 4 KiB
constexpr uint32_t ES_SLOTS    = 1024;        // slots of the slab (MSGPU_ALIGN_SLOTS lowers it)
constexpr uint32_t ES_RUN      = 0x3fffffffu; // the low 30 bits of a word: G in the table, a run of '=' in the script
enum { ES_X = 1, ES_D = 2, ES_I = 3 };

// ---- the pieces that the script (rule 10) and the extension (rule 11) share

// Row e of rule 10's recurrence before its slides: nf[c] = the largest valid candidate of this lane's cell (e, k), FR_NONE
// where there is none, and op[c] the edit that led to it.  Row 0 is the point (0, 0), without an edit
__device__ __forceinline__ void fr_candidates(const int (&fr)[4], int e, int n, int m, int lane, int (&nf)[4], uint32_t (&op)[4]) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = lane + 64 * c - 128;
    int       x = FR_NONE;
    uint32_t  o = 0;
    if (e == 0) {
      if (k == 0) x = 0;
    } else {
      const FrNeighbours nb = fr_neighbours(fr, c, lane);
      const int          lo = nb.lo, hi = nb.hi;
      if ((k < 0 ? -k : k) <= e) { // rule 10: the largest valid candidate, the first of X, D, I on a tie
        if (fr[c] >= 0 && fr[c] < min(n, m - k)) {
          x = fr[c] + 1;
          o = ES_X;
        }
        if (hi >= 0 && hi < n && hi + 1 > x) {
          x = hi + 1;
          o = ES_D;
        }
        if (lo >= 0 && lo + k <= m && lo > x) {
          x = lo;
          o = ES_I;
        }
      }
    }
    nf[c] = x;
    op[c] = o;
  }
}

// Row e behind its slides: every defined cell (e, k) is shown to cell(k, x) and becomes word e * e + k + e of the table,
// op << 30 | x; the row becomes fr.  (In this order: with the store first the extension's kernels came out 2 % longer and the
// slab class ran 1 % slower.)
template <class Cell>
__device__ __forceinline__ void fr_store_row(uint32_t *T, int e, int lane, const int (&nf)[4], const uint32_t (&op)[4], int (&fr)[4], Cell cell) {
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int k = lane + 64 * c - 128;
    if ((k < 0 ? -k : k) <= e && nf[c] >= 0) {
      cell(k, nf[c]);
      T[e * e + k + e] = (op[c] << 30) | static_cast<uint32_t>(nf[c]);
    }
    fr[c] = nf[c];
  }
}

// the table was written by all lanes and is read by each: LDS needs the wavefront's order, device memory the device's
__device__ __forceinline__ void fr_table_fence(bool in_lds) {
  if (in_lds) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  } else {
    __threadfence();
  }
}

// The walk back from cell (e, k), whose word is w, to row 0: e dependent reads of the table, which every lane follows (the
// address is uniform); lane 0 writes the words out[e..1] of the script.  What is left for out[0] comes back: the cell of row 0
// that the walk reached (k, w), the op that led out of it (carry), and whether an op of the walk did not lead into the row
// before it (bad)
struct FrWalk {
  int      k;
  uint32_t w, carry;
  bool     bad;
};
__device__ __forceinline__ FrWalk fr_walk_back(const uint32_t *T, int e, int k, uint32_t w, int lane, uint32_t *out) {
  uint32_t carry = 0;
  bool     bad = false;
  for (; e >= 1; --e) {
    const uint32_t o  = w >> 30;
    const int      ko = o == ES_X ? k : o == ES_D ? k + 1 : k - 1;
    const int      kp = max(-(e - 1), min(e - 1, ko)); // (no read leaves the table)
    bad |= o == 0 || kp != ko;
    const uint32_t wp = T[(e - 1) * (e - 1) + kp + (e - 1)];
    const uint32_t x0 = (wp & ES_RUN) + (o != ES_I ? 1u : 0u);
    if (lane == 0) out[e] = (carry << 30) | (((w & ES_RUN) - x0) & ES_RUN);
    carry = o;
    k     = kp;
    w     = wp;
  }
  return FrWalk{k, w, carry, bad};
}

// The two shapes of a kernel whose wavefronts each fill a table per pair.  IN_LDS: wavefront wv of the grid has the one pair
// i = wv and its workgroup's slice `lds` of LDS.  Otherwise it has slot wv of the slab, (W + 1)^2 words, and the pairs
// i = wv, wv + slots, ... one after the other.  pair(i, T) does the work; which pair i names is the caller's business
template <bool IN_LDS, class Pair>
__device__ __forceinline__ void fr_wave_pairs(uint32_t *lds, uint32_t *slab, uint32_t slots, uint32_t W, uint32_t n, Pair pair) {
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (IN_LDS) {
    if (wv < n) pair(wv, lds); // (whole wavefronts leave)
  } else {
    if (wv >= slots) return;
    uint32_t *const T = slab + static_cast<uint64_t>(wv) * (W + 1) * (W + 1);
    for (uint32_t i = wv; i < n; i += slots) pair(i, T);
  }
}

// ---- rule 10

__device__ __forceinline__ void edit_script_wave(const uint8_t *a, int n, const uint8_t *b, int m, int d, uint32_t *T, bool in_lds,
                                                 uint32_t *out, uint32_t *broken) {
  const int lane = threadIdx.x & 63;
  const int ks   = m - n;
  if ((ks < 0 ? -ks : ks) > d) { // (the walk would start outside row d)
    if (lane == 0) atomicAdd(broken, 1u);
    return;
  }
  int fr[4] = {FR_NONE, FR_NONE, FR_NONE, FR_NONE};
  for (int e = 0; e <= d; ++e) {
    int      nf[4];
    uint32_t op[4];
    fr_candidates(fr, e, n, m, lane, nf, op);
    fr_slide_row(a, n, b, m, e, lane, nf);
    fr_store_row(T, e, lane, nf, op, fr, [](int, int) {});
  }
  fr_table_fence(in_lds);
  const uint32_t w    = T[d * d + ks + d];
  const FrWalk   back = fr_walk_back(T, d, ks, w, lane, out);
  if (lane == 0) {
    out[0] = (back.carry << 30) | (back.w & ES_RUN);
    // row d does not end the pair (d is not its distance), or the walk left the table
    if ((w & ES_RUN) != static_cast<uint32_t>(n) || back.bad) atomicAdd(broken, 1u);
  }
}

// the pairs of a class, as k_edit_script_classes listed them: the LDS class from the front of `list`, the slab class from its back
template <bool IN_LDS>
__global__ __launch_bounds__(256) void k_edit_script(const uint8_t *base_a, const uint8_t *base_b, const msgpu_align_pair *pairs,
                                                     const uint32_t *dist, const uint64_t *off, const uint32_t *list, uint32_t n_pairs,
                                                     uint32_t *cnt, uint32_t W, uint32_t *slab, uint32_t slots, uint32_t *words) {
  __shared__ uint32_t s_t[IN_LDS ? 4 : 1][IN_LDS ? (ES_LDS_MAXD + 1) * (ES_LDS_MAXD + 1) : 1];
  const uint32_t n_cls = min(cnt[IN_LDS ? ES_CNT_LDS : ES_CNT_SLAB], n_pairs);
  fr_wave_pairs<IN_LDS>(s_t[IN_LDS ? threadIdx.x >> 6 : 0], slab, slots, W, n_cls, [&](uint32_t i, uint32_t *T) {
    const uint32_t         p = list[IN_LDS ? i : n_pairs - 1 - i];
    const msgpu_align_pair pr = pairs[p];
    const uint32_t         d = dist[p];
    if (d < 1 || d > (IN_LDS ? static_cast<uint32_t>(ES_LDS_MAXD) : W)) { // (the table would not fit its slice or slot)
      if ((threadIdx.x & 63) == 0) atomicAdd(&cnt[ES_CNT_BROKEN], 1u);
      return;
    }
    edit_script_wave(base_a + pr.a_off, static_cast<int>(pr.a_len), base_b + pr.b_off, static_cast<int>(pr.b_len), static_cast<int>(d), T,
                     IN_LDS, words + off[p], &cnt[ES_CNT_BROKEN]);
  });
}

// a thread per pair: its class; a pair without an edit gets its one word here (no table is needed)
__global__ __launch_bounds__(256) void k_edit_script_classes(const msgpu_align_pair *pairs, const uint32_t *dist, const uint64_t *off,
                                                             uint32_t n, uint32_t W, uint32_t *list, uint32_t *cnt, uint32_t *words) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t d = dist[i];
  if (d > W) {
    atomicAdd(&cnt[ES_CNT_CAPPED], 1u);
    return;
  }
  atomicMax(&cnt[ES_CNT_MAXD], d);
  if (d == 0) {
    words[off[i]] = pairs[i].a_len;
    atomicAdd(&cnt[ES_CNT_D0], 1u);
  } else if (d <= static_cast<uint32_t>(ES_LDS_MAXD)) {
    list[atomicAdd(&cnt[ES_CNT_LDS], 1u)] = i;
  } else {
    list[n - 1 - atomicAdd(&cnt[ES_CNT_SLAB], 1u)] = i;
  }
}

// the words of every pair's script, and a zero behind them: their exclusive scan gives the offsets
__global__ __launch_bounds__(256) void k_edit_script_lengths(const uint32_t *dist, uint32_t n, uint32_t W, uint32_t *len) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i > n) return;
  len[i] = i < n && dist[i] <= W ? dist[i] + 1 : 0;
}

void launch_edit_script_lengths(hipStream_t st, const uint32_t *d_dist, uint32_t n, uint32_t band, uint32_t *d_len) {
  hipLaunchKernelGGL(k_edit_script_lengths, dim3(n / 256 + 1), dim3(256), 0, st, d_dist, n, band, d_len);
}

uint32_t edit_script_slots() {
  const char *s = std::getenv("MSGPU_ALIGN_SLOTS");
  const long  v = s ? std::strtol(s, nullptr, 10) : 0;
  return v >= 1 && v < static_cast<long>(ES_SLOTS) ? static_cast<uint32_t>(v) : ES_SLOTS;
}
uint64_t edit_script_slab_words(uint32_t slots, uint32_t band) { // (a band within the LDS class has no slab class)
  return band > static_cast<uint32_t>(ES_LDS_MAXD) ? static_cast<uint64_t>(slots) * (band + 1) * (band + 1) : 0;
}
uint32_t edit_script_lds_max_d() { return ES_LDS_MAXD; }

hipError_t launch_edit_script_pairs(hipStream_t st, const uint8_t *d_a, const uint8_t *d_b, const msgpu_align_pair *d_pairs, uint32_t n,
                                    uint32_t band, const uint32_t *d_dist, const uint64_t *d_off, uint32_t *d_list, uint32_t *d_cnt,
                                    uint32_t *d_slab, uint32_t slots, uint32_t *d_words) {
  hipError_t e = hipMemsetAsync(d_cnt, 0, ES_CNT_COUNT * sizeof(uint32_t), st);
  if (e != hipSuccess || !n) return e;
  hipLaunchKernelGGL(k_edit_script_classes, dim3((n + 255) / 256), dim3(256), 0, st, d_pairs, d_dist, d_off, n, band, d_list, d_cnt, d_words);
  hipLaunchKernelGGL((k_edit_script<true>), dim3((n + 3) / 4), dim3(256), 0, st, d_a, d_b, d_pairs, d_dist, d_off, d_list, n, d_cnt, band,
                     d_slab, slots, d_words);
  if (band > static_cast<uint32_t>(ES_LDS_MAXD) && slots && d_slab)
    hipLaunchKernelGGL((k_edit_script<false>), dim3((slots + 3) / 4), dim3(256), 0, st, d_a, d_b, d_pairs, d_dist, d_off, d_list, n, d_cnt,
                       band, d_slab, slots, d_words);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Rule 11 (include/msgpu.h, "unitig-to-read mapping"): an alignment with a free end.  The table is rule 10's on a flank pair,
// rows 0..band, with nothing of its end test: every defined cell (e, k) scores x + y - EXT_P * e, and the end cell is the best
// one by (score, smaller e, smaller |k|, negative k).  A row is the script's (fr_candidates, the valid-candidate recurrence:
// here the values of all cells decide, so the clamped one of edit_distance_fr_wave will not do); every lane keeps the best
// of its own cells, one reduction per row gives the wavefront's best score, which ends the loop at the first row that
// cannot beat it (a cell of row e scores at most n + m - EXT_P * e, and on a tie the smaller e wins), and one reduction
// behind the loop applies the whole order.  The walk back from the end cell is the script's too (fr_walk_back), e* + 1 words.
// REV reads flank byte i as base[-1 - i] (a left flank: a and b name the byte behind it), so no reversed copy exists.
// A table that contradicts itself on the walk is counted in *broken.
// ---------------------------------------------------------------------------------------------------------------------

constexpr int EXT_P = MSGPU_MAP_EXTEND_PENALTY;

__device__ __forceinline__ bool ext_better(int s, int e, int k, int bs, int be, int bk) {
  if (s != bs) return s > bs;
  if (e != be) return e < be;
  const int ak = k < 0 ? -k : k, abk = bk < 0 ? -bk : bk;
  if (ak != abk) return ak < abk;
  return k < bk;
}

template <bool REV>
__device__ __forceinline__ void extend_wave(const uint8_t *a, int n, const uint8_t *b, int m, int band, uint32_t *T, bool in_lds,
                                            uint32_t *out, msgpu_ext_end *end, uint32_t *broken) {
  const int lane = threadIdx.x & 63;
  int       fr[4] = {FR_NONE, FR_NONE, FR_NONE, FR_NONE};
  int       bs = -(1 << 30), be = 0, bk = 0; // this lane's best cell
  int       top = -(1 << 30), rows = 0;      // the wavefront's best score so far; the rows that ran
  for (int e = 0; e <= band; ++e) {
    if (n + m - EXT_P * e <= top) break; // (uniform; never at e = 0)
    int      nf[4];
    uint32_t op[4];
    fr_candidates(fr, e, n, m, lane, nf, op);
    fr_slide_row<REV>(a, n, b, m, e, lane, nf);
    fr_store_row(T, e, lane, nf, op, fr, [&](int k, int x) {
      const int s = 2 * x + k - EXT_P * e;
      if (ext_better(s, e, k, bs, be, bk)) {
        bs = s;
        be = e;
        bk = k;
      }
    });
    top = bs;
    for (int o = 32; o > 0; o >>= 1) top = max(top, __shfl_xor(top, o));
    ++rows;
  }
  for (int o = 32; o > 0; o >>= 1) { // rule 11.3's order over the lanes' bests: every lane ends with the end cell
    const int os = __shfl_xor(bs, o), oe = __shfl_xor(be, o), ok = __shfl_xor(bk, o);
    if (ext_better(os, oe, ok, bs, be, bk)) {
      bs = os;
      be = oe;
      bk = ok;
    }
  }
  fr_table_fence(in_lds);
  const int      es = max(0, min(band, be)); // (no read leaves the table)
  const int      ke = max(-es, min(es, bk));
  const uint32_t w  = T[es * es + ke + es];
  const int      xs = static_cast<int>(w & ES_RUN);
  const FrWalk   back = fr_walk_back(T, es, ke, w, lane, out);
  if (lane == 0) {
    out[0] = (back.carry << 30) | (back.w & ES_RUN);
    *end   = msgpu_ext_end{static_cast<uint32_t>(es), bk, static_cast<uint32_t>(xs), static_cast<uint32_t>(xs + bk), bs,
                           static_cast<uint32_t>(rows)};
    // the end cell is not what the row loop saw, or the walk left the table or did not end at the point (0, 0)
    if (es != be || ke != bk || 2 * xs + ke - EXT_P * es != bs || back.bad || back.k != 0 || (back.w >> 30) != 0) atomicAdd(broken, 1u);
  }
}

// one wavefront per end; end p's words go to words[p * (W + 1) ..), e + 1 of them.  IN_LDS (W <= ES_LDS_MAXD): the table in
// LDS, four wavefronts to a workgroup; otherwise the wavefronts stride over the slots of the slab
template <bool IN_LDS, bool REV>
__global__ __launch_bounds__(256) void k_extend_ends(const uint8_t *base_a, const uint8_t *base_b, const msgpu_align_pair *pairs,
                                                     uint32_t n_pairs, uint32_t W, uint32_t *slab, uint32_t slots, msgpu_ext_end *ends,
                                                     uint32_t *words, uint32_t *broken) {
  __shared__ uint32_t s_t[IN_LDS ? 4 : 1][IN_LDS ? (ES_LDS_MAXD + 1) * (ES_LDS_MAXD + 1) : 1];
  const uint32_t n = IN_LDS && W > static_cast<uint32_t>(ES_LDS_MAXD) ? 0 : n_pairs; // (the table would not fit its slice)
  fr_wave_pairs<IN_LDS>(s_t[IN_LDS ? threadIdx.x >> 6 : 0], slab, slots, W, n, [&](uint32_t p, uint32_t *T) {
    const msgpu_align_pair pr = pairs[p];
    extend_wave<REV>(base_a + pr.a_off, static_cast<int>(pr.a_len), base_b + pr.b_off, static_cast<int>(pr.b_len), static_cast<int>(W), T,
                     IN_LDS, words + static_cast<uint64_t>(p) * (W + 1), ends + p, broken);
  });
}

hipError_t launch_extend_ends(hipStream_t st, const uint8_t *d_a, const uint8_t *d_b, const msgpu_align_pair *d_pairs, uint32_t n,
                              uint32_t band, bool rev, uint32_t *d_slab, uint32_t slots, msgpu_ext_end *d_ends, uint32_t *d_words,
                              uint32_t *d_broken) {
  if (!n) return hipSuccess;
  if (band <= static_cast<uint32_t>(ES_LDS_MAXD)) {
    const dim3 grid((n + 3) / 4);
    if (rev) hipLaunchKernelGGL((k_extend_ends<true, true>), grid, dim3(256), 0, st, d_a, d_b, d_pairs, n, band, d_slab, slots, d_ends, d_words, d_broken);
    else hipLaunchKernelGGL((k_extend_ends<true, false>), grid, dim3(256), 0, st, d_a, d_b, d_pairs, n, band, d_slab, slots, d_ends, d_words, d_broken);
  } else {
    if (!slots || !d_slab) return hipErrorInvalidValue;
    const dim3 grid((slots + 3) / 4);
    if (rev) hipLaunchKernelGGL((k_extend_ends<false, true>), grid, dim3(256), 0, st, d_a, d_b, d_pairs, n, band, d_slab, slots, d_ends, d_words, d_broken);
    else hipLaunchKernelGGL((k_extend_ends<false, false>), grid, dim3(256), 0, st, d_a, d_b, d_pairs, n, band, d_slab, slots, d_ends, d_words, d_broken);
  }
  return hipGetLastError();
}

} // namespace msgpu
