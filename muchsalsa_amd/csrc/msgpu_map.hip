// msgpu_map.hip -- the seed-and-chain mapper (include/msgpu.h, "unitig-to-read mapping").
//
// Both files go through the sequence loader (msgpu_seq_parse_upload): the bases lie as bytes in HBM, the host keeps names,
// lengths and offsets.  Everything behind that is count-then-write on the device:
//   k_mp_sketch    a workgroup per tile of 256 k-mer start positions: the (hash, key, strand) of the tile and of w - 1
//                  positions on either side go into LDS (every thread rolls k bytes through KfRoll), then a thread per
//                  position decides rule 2 from its 2 w - 1 neighbours.  Pass 1 counts per tile, pass 2 writes
//   index          one radix_sort_pairs over bits [0, 2k), run lengths and starts of the keys, k_kf_table over the
//                  distinct keys; the occurrence cap is applied where a query minimizer looks its key up
//   batches        rule 9: the index and the anchor counts stay, the query records go through everything below in batches
//                  under a budget of device bytes (mp_batch_bytes, mp_cut, mp_batch); k_mp_prefix gives the anchors in
//                  front of every query record, one reserved arena serves every batch
//   k_mp_anchors   count per query minimizer, exclusive scan, expansion; two stable radix sorts bring the anchors into
//                  (group, x, y) order; run lengths of the group keys are the groups; k_mp_classify applies rule 6's
//                  pre-filter and splits the kept groups into those of at most 16 anchors and the others
//   k_mp_chain     rule 5, a wavefront per group: lane l holds the anchors l, l + 64, ... of the group, so the 64
//                  predecessors of anchor i are one per lane; argmax by DPP / permlane moves (group_max_i64)
//   k_mp_chain16   the same for groups of at most 16 anchors, four to a wavefront, a row of 16 lanes each
//   k_mp_walk      rule 6 behind a segmented sort by (f descending, index ascending): a thread per group
//   k_mp_pairs     exact mode: the segment pairs of the emitted chains; distances by edit_distance_fr_wave (msgpu_align.hip)
//                  against a forward and a reverse-complemented copy of the queries (the existing gather, mp_oriented)
//   cigar mode     rule 10 behind the distances: the scripts' offsets (a scan), launch_edit_script_pairs (msgpu_align.hip),
//                  k_mp_columns per pair, two segmented reductions and k_mp_cigar per chain; the host merges the runs
//   ranking        rule 12, on request, behind k_mp_table: the chains of a query record are a segment (k_rk_heads, a scan);
//                  k_rk_wave ranks a segment of at most 64 chains in one wavefront, a lane per chain; k_rk_list walks a longer
//                  one in sorted order against its list of primaries (LDS, then the arena); k_rk_figures and k_rk_rows finish
//   mates          rule 13, on request, the last device step of a batch (behind rule 11's extension): the chains of a pair of
//                  query records are a segment (k_mt_heads, a scan); k_mt_classify settles a pair with one chain per mate or
//                  none on one, k_mt_lanes<16> and <64> take a pair in 16 lanes or a wavefront, a lane per mate-1 chain,
//                  k_mt_list a longer one in tiles (mate 2's in LDS); k_mt_rows writes the rows and the counts
// Integers only.  Kernel rules: vector stores and vector atomics only; no inline asm.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/device/device_segmented_reduce.hpp>

#include <memory>
#include <new>
#include <string>
#include <thread>

#include "host_pool.h"
#include "msgpu_device.h"
#include "msgpu_internal.h"
#include "msgpu_kmer_shared.h"

namespace msgpu {

constexpr long long MP_MIN = static_cast<long long>(0x8000000000000000ull);

constexpr int MP_TILE = 256, MP_SPAN = MP_TILE + 2 * 63;

// rule 2.  WRITE = false: minimizers per tile; WRITE = true: (key, record << 32 | position << 1 | strand) at the tile's offset
template <bool WRITE>
__global__ __launch_bounds__(256) void k_mp_sketch(SeqRecs R, int k, int w, uint32_t *tile_cnt, const uint64_t *tile_off,
                                                   uint64_t *keys, uint64_t *vals, uint64_t cap) {
  __shared__ uint64_t s_h[MP_SPAN], s_key[MP_SPAN];
  __shared__ uint8_t  s_v[MP_SPAN]; // bit 0: a k-mer starts here, bit 1: its strand
  __shared__ uint32_t s_wave[4];
  const long long base = static_cast<long long>(blockIdx.x) * MP_TILE - (w - 1);
  const int       span = MP_TILE + 2 * (w - 1);
  for (int e = threadIdx.x; e < span; e += 256) {
    const long long p = base + e;
    uint8_t         v = 0;
    uint64_t        h = 0, key = 0;
    if (p >= 0 && static_cast<uint64_t>(p) < R.n_bases) {
      const uint32_t r = seq_record(R, static_cast<uint64_t>(p));
      if (r != REC_NONE && static_cast<uint64_t>(p) + k <= R.off[r] + R.len[r]) {
        KfRoll<uint64_t> roll(k);
        bool             ok = false;
        for (int j = 0; j < k; ++j) ok = roll.step(R.bases[p + j], key);
        if (ok) {
          v = static_cast<uint8_t>(1u | (roll.rc < roll.fw ? 2u : 0u));
          h = kf_hash(key);
        }
      }
    }
    s_h[e]   = h;
    s_key[e] = key;
    s_v[e]   = v;
  }
  __syncthreads();
  const int e = static_cast<int>(threadIdx.x) + (w - 1);
  bool      is_min = false;
  if (s_v[e]) { // the positions it beats on either side, as far as a window reaches
    const uint64_t h = s_h[e];
    int            gl = 0, gr = 0;
    while (gl < w - 1 && s_v[e - gl - 1] && h < s_h[e - gl - 1]) ++gl;
    while (gl + gr < w - 1 && s_v[e + gr + 1] && h <= s_h[e + gr + 1]) ++gr;
    is_min = gl + gr >= w - 1;
  }
  uint32_t       total;
  const uint32_t at = block_excl_scan_256(is_min ? 1u : 0u, s_wave, &total);
  if (!WRITE) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
    return;
  }
  if (!is_min) return;
  const uint64_t p = static_cast<uint64_t>(base + e), slot = tile_off[blockIdx.x] + at;
  const uint32_t r = seq_record(R, p);
  if (slot < cap && r != REC_NONE) {
    keys[slot] = s_key[e];
    vals[slot] = (static_cast<uint64_t>(r) << 32) | ((p - R.off[r]) << 1) | (s_v[e] >> 1);
  }
}

// the keys rule 3 leaves out
__global__ __launch_bounds__(256) void k_mp_occ(const uint32_t *cnt, uint32_t n, uint32_t max_occ, kf_ull *keys_out, kf_ull *entries_out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool     over = i < n && cnt[i] > max_occ;
  wave_count(over, keys_out);
  if (over) atomicAdd(entries_out, static_cast<kf_ull>(cnt[i]));
}

struct MpIndex {
  const uint64_t *ukeys;  // the distinct keys, ascending
  const uint32_t *ucnt, *ustart, *slots;
  uint32_t        mask, max_occ;
  const uint64_t *vals;   // the entries in key order
};

// rule 4 for the query minimizers [m0, m1).  WRITE = false: anchors per query minimizer; WRITE = true: the anchors, from
// slot 0 for the first anchor of minimizer m0 (off: the anchors in front of every minimizer of the file)
template <bool WRITE>
__global__ __launch_bounds__(256) void k_mp_anchors(MpIndex X, const uint64_t *qkeys, const uint64_t *qvals, uint64_t m0, uint64_t m1,
                                                    const uint32_t *qlen, int k, int ava, uint32_t *cnt, const uint64_t *off,
                                                    uint64_t *g, uint64_t *xy, uint64_t cap) {
  const uint64_t i = m0 + static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= m1) return;
  const uint32_t j = kf_find(X.ukeys, X.slots, X.mask, qkeys[i]);
  uint32_t       c = 0;
  if (j != KF_EMPTY && X.ucnt[j] <= X.max_occ) {
    const uint64_t  qv = qvals[i];
    const uint32_t  q = static_cast<uint32_t>(qv >> 32), qpos = static_cast<uint32_t>(qv & 0xffffffffu) >> 1, qs = qv & 1u;
    const uint64_t *ent = X.vals + X.ustart[j];
    const uint32_t  m = X.ucnt[j];
    if (!WRITE && !ava) c = m;
    else
      for (uint32_t e = 0; e < m; ++e) {
        const uint64_t tv = ent[e];
        const uint32_t t = static_cast<uint32_t>(tv >> 32);
        if (ava && q >= t) continue;
        if (WRITE) {
          const uint32_t s = qs ^ static_cast<uint32_t>(tv & 1u), x = static_cast<uint32_t>(tv & 0xffffffffu) >> 1;
          const uint32_t y = s ? qlen[q] - static_cast<uint32_t>(k) - qpos : qpos;
          const uint64_t slot = off[i] - off[m0] + c;
          if (slot < cap) {
            g[slot]  = (static_cast<uint64_t>(q) << 32) | (static_cast<uint64_t>(t) << 1) | s;
            xy[slot] = (static_cast<uint64_t>(x) << 32) | y;
          }
        }
        ++c;
      }
  }
  if (!WRITE) cnt[i] = c;
}

// rule 9's prefixes, a thread per query record r <= n_rec: the record's first minimizer (a lower bound: the record index is in
// the top 32 bits of vals, and vals ascend) and the anchors in front of it
__global__ __launch_bounds__(256) void k_mp_prefix(const uint64_t *qvals, uint64_t nq, const uint64_t *aoff, uint32_t n_rec,
                                                   uint64_t *first_min, uint64_t *anchors_before) {
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r > n_rec) return;
  uint64_t lo = 0, hi = nq;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((qvals[mid] >> 32) < r) lo = mid + 1;
    else hi = mid;
  }
  first_min[r]      = lo;
  anchors_before[r] = aoff[lo];
}

// rule 6's pre-filter and the size classes
__global__ __launch_bounds__(256) void k_mp_classify(const uint32_t *gcnt, uint32_t n_groups, int k, int min_score, int min_count,
                                                     uint32_t *flag_small, uint32_t *flag_large, kf_ull *hist, kf_ull *largest) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_groups) return;
  const uint32_t n = gcnt[i];
  const bool     keep = static_cast<long long>(n) >= min_count && static_cast<long long>(n) * k >= min_score;
  flag_small[i] = keep && n <= 16;
  flag_large[i] = keep && n > 16;
  if (keep) {
    atomicAdd(&hist[31 - __clz(n | 1u)], 1ull);
    atomicMax(largest, static_cast<kf_ull>(n));
  }
}

__global__ __launch_bounds__(256) void k_mp_lists(const uint32_t *gcnt, const uint32_t *gstart, uint32_t n_groups, const uint32_t *flag_small,
                                                  const uint32_t *flag_large, const uint32_t *pos_small, const uint32_t *pos_large,
                                                  uint32_t *list_small, uint32_t *list_large, uint32_t *list_kept, uint32_t *seg_begin,
                                                  uint32_t *seg_end) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_groups) return;
  if (flag_small[i]) list_small[pos_small[i]] = i;
  if (flag_large[i]) list_large[pos_large[i]] = i;
  if (flag_small[i] || flag_large[i]) {
    const uint32_t kk = pos_small[i] + pos_large[i];
    list_kept[kk] = i;
    seg_begin[kk] = gstart[i];
    seg_end[kk]   = gstart[i] + gcnt[i];
  }
}

struct MpChainArgs {
  const uint32_t *list;
  uint32_t        n_list;
  const uint32_t *gstart, *gcnt;
  const uint64_t *xy;
  int32_t        *f, *pred;
  uint64_t       *sortkey; // f << 32 | ~index: descending order is (f descending, index ascending)
  int             k, max_gap, bandwidth;
};

// what predecessor j offers anchor i, packed with its distance d = i - 1 - j so that the largest value is the best score and,
// among equals, the largest j; MP_MIN: j is no predecessor
__device__ __forceinline__ long long mp_offer(const MpChainArgs &a, int xi, int yi, int xj, int yj, int fj, int d, bool there) {
  const int dx = xi - xj, dy = yi - yj;
  if (!there || dx <= 0 || dy <= 0 || dx > a.max_gap || dy > a.max_gap) return MP_MIN;
  const uint32_t dd = static_cast<uint32_t>(dx > dy ? dx - dy : dy - dx);
  if (dd > static_cast<uint32_t>(a.bandwidth)) return MP_MIN;
  const int       gain = min(min(dx, dy), a.k);
  const long long pen = dd ? static_cast<long long>((static_cast<uint64_t>(dd) * static_cast<uint32_t>(a.k)) / 100u) + ((31 - __clz(dd)) >> 1) : 0;
  return (static_cast<long long>(fj) + gain - pen) * 64 + (63 - d);
}

__global__ __launch_bounds__(256) void k_mp_chain(MpChainArgs a) {
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int      lane = threadIdx.x & 63;
  if (wv >= a.n_list) return; // (whole wavefronts leave)
  const uint32_t gi = a.list[wv], s0 = a.gstart[gi], n = a.gcnt[gi];
  int            px = 0, py = 0, pf = 0; // the block of 64 anchors in front of the current one
  for (uint32_t b0 = 0; b0 < n; b0 += 64) {
    const uint32_t idx = b0 + lane;
    const bool     have = idx < n;
    const uint64_t v = have ? a.xy[s0 + idx] : 0;
    const int      cx = static_cast<int>(v >> 32), cy = static_cast<int>(static_cast<uint32_t>(v));
    int            cf = 0, cp = -1;
    const int      m = static_cast<int>(min(64u, n - b0));
    for (int c = 0; c < m; ++c) {
      const int  xi = rl_i32(cx, c), yi = rl_i32(cy, c);
      const bool cur = lane < c;
      const int  d = cur ? c - 1 - lane : c + 63 - lane;
      long long  best = mp_offer(a, xi, yi, cur ? cx : px, cur ? cy : py, cur ? cf : pf, d, cur || b0 > 0);
      best = group_max_i64<64>(best);
      if (lane == c) {
        const long long score = best >> 6;
        if (best != MP_MIN && score > a.k) {
          cf = static_cast<int>(score);
          cp = static_cast<int>(b0) + c - 1 - (63 - static_cast<int>(best & 63));
        } else {
          cf = a.k;
        }
      }
    }
    if (have) {
      a.f[s0 + idx]       = cf;
      a.pred[s0 + idx]    = cp;
      a.sortkey[s0 + idx] = (static_cast<uint64_t>(static_cast<uint32_t>(cf)) << 32) | (0xffffffffu - idx);
    }
    px = cx;
    py = cy;
    pf = cf;
  }
}

// lane c of every row of 16 to all lanes of the row (row_newbcast)
template <int C> __device__ __forceinline__ int mp_row_bcast(int v) { return __builtin_amdgcn_mov_dpp(v, 0x150 + C, 0xf, 0xf, false); }

template <int C> __device__ __forceinline__ void mp_step16(const MpChainArgs &a, int r, uint32_t n, int cx, int cy, int &cf, int &cp) {
  const int xi = mp_row_bcast<C>(cx), yi = mp_row_bcast<C>(cy);
  long long best = mp_offer(a, xi, yi, cx, cy, cf, C - 1 - r, r < C && static_cast<uint32_t>(C) < n);
  best = group_max_i64<16>(best);
  if (r == C) {
    const long long score = best >> 6;
    if (best != MP_MIN && score > a.k) {
      cf = static_cast<int>(score);
      cp = C - 1 - (63 - static_cast<int>(best & 63));
    } else {
      cf = a.k;
    }
  }
}

// groups of at most 16 anchors: one per row of 16 lanes, lane r holds anchor r from start to end
__global__ __launch_bounds__(256) void k_mp_chain16(MpChainArgs a) {
  const uint32_t sg = blockIdx.x * 16 + (threadIdx.x >> 4);
  const int      r = threadIdx.x & 15;
  uint32_t       s0 = 0, n = 0;
  if (sg < a.n_list) { // (a row without a group stays: the reductions need all lanes)
    const uint32_t gi = a.list[sg];
    s0 = a.gstart[gi];
    n  = a.gcnt[gi];
  }
  const bool     have = static_cast<uint32_t>(r) < n;
  const uint64_t v = have ? a.xy[s0 + r] : 0;
  const int      cx = static_cast<int>(v >> 32), cy = static_cast<int>(static_cast<uint32_t>(v));
  int            cf = 0, cp = -1;
  mp_step16<0>(a, r, n, cx, cy, cf, cp);
  mp_step16<1>(a, r, n, cx, cy, cf, cp);
  mp_step16<2>(a, r, n, cx, cy, cf, cp);
  mp_step16<3>(a, r, n, cx, cy, cf, cp);
  mp_step16<4>(a, r, n, cx, cy, cf, cp);
  mp_step16<5>(a, r, n, cx, cy, cf, cp);
  mp_step16<6>(a, r, n, cx, cy, cf, cp);
  mp_step16<7>(a, r, n, cx, cy, cf, cp);
  mp_step16<8>(a, r, n, cx, cy, cf, cp);
  mp_step16<9>(a, r, n, cx, cy, cf, cp);
  mp_step16<10>(a, r, n, cx, cy, cf, cp);
  mp_step16<11>(a, r, n, cx, cy, cf, cp);
  mp_step16<12>(a, r, n, cx, cy, cf, cp);
  mp_step16<13>(a, r, n, cx, cy, cf, cp);
  mp_step16<14>(a, r, n, cx, cy, cf, cp);
  mp_step16<15>(a, r, n, cx, cy, cf, cp);
  if (have) {
    a.f[s0 + r]       = cf;
    a.pred[s0 + r]    = cp;
    a.sortkey[s0 + r] = (static_cast<uint64_t>(static_cast<uint32_t>(cf)) << 32) | (0xffffffffu - static_cast<uint32_t>(r));
  }
}

struct MpLink { // rule 7 on one link
  uint32_t c, lt, lq;
};
__device__ inline MpLink mp_link(uint64_t vi, uint64_t vj, int k) {
  const uint32_t dx = static_cast<uint32_t>(vi >> 32) - static_cast<uint32_t>(vj >> 32);
  const uint32_t dy = static_cast<uint32_t>(vi) - static_cast<uint32_t>(vj);
  const uint32_t c = min(min(dx, dy), static_cast<uint32_t>(k));
  return MpLink{c, dx - c, dy - c};
}

struct MpRaw { // a chain as the walk leaves it, in the slot of its group's e-th anchor
  uint32_t first, last; // local indices: the start of the walk (the largest x) and its end (the smallest)
  uint32_t n_anchors, block, seed_matches, n_pairs;
  int32_t  score;
};

// rule 6: a thread per kept group
__global__ __launch_bounds__(64) void k_mp_walk(const uint32_t *list_kept, uint32_t n_kept, const uint32_t *gstart, const uint32_t *gcnt,
                                                const uint64_t *xy, const int32_t *f, const int32_t *pred, const uint64_t *sorted,
                                                uint8_t *used, int k, int min_score, int min_count, MpRaw *raw, uint32_t *n_emit,
                                                kf_ull *drop_score, kf_ull *drop_count, kf_ull *cut_chains) {
  const uint32_t kk = blockIdx.x * 64 + threadIdx.x;
  uint32_t       by_score = 0, by_count = 0, cuts = 0;
  if (kk < n_kept) {
    const uint32_t gi = list_kept[kk], s0 = gstart[gi], n = gcnt[gi];
    uint32_t       emitted = 0;
    for (uint32_t p = 0; p < n; ++p) {
      const uint32_t first = 0xffffffffu - static_cast<uint32_t>(sorted[s0 + p]);
      if (used[s0 + first]) continue;
      MpRaw    c{first, first, 0, static_cast<uint32_t>(k), static_cast<uint32_t>(k), 0, f[s0 + first]};
      bool     cut = false;
      for (uint32_t cur = first;;) {
        used[s0 + cur] = 1;
        ++c.n_anchors;
        c.last = cur;
        const int32_t pr = pred[s0 + cur];
        if (pr < 0) break;
        if (used[s0 + pr]) {
          c.score -= f[s0 + pr];
          cut = true;
          break;
        }
        const MpLink l = mp_link(xy[s0 + cur], xy[s0 + pr], k);
        c.block += l.c + max(l.lt, l.lq);
        c.seed_matches += l.c;
        c.n_pairs += (l.lt | l.lq) ? 1u : 0u;
        cur = static_cast<uint32_t>(pr);
      }
      if (c.score >= min_score && static_cast<long long>(c.n_anchors) >= min_count) {
        raw[s0 + emitted++] = c;
        cuts += cut;
      } else if (c.score < min_score) {
        ++by_score;
      } else {
        ++by_count;
      }
    }
    n_emit[kk] = emitted;
  }
  for (int o = 32; o > 0; o >>= 1) {
    by_score += __shfl_xor(by_score, o);
    by_count += __shfl_xor(by_count, o);
    cuts += __shfl_xor(cuts, o);
  }
  if ((threadIdx.x & 63) == 0) {
    if (by_score) atomicAdd(drop_score, static_cast<kf_ull>(by_score));
    if (by_count) atomicAdd(drop_count, static_cast<kf_ull>(by_count));
    if (cuts) atomicAdd(cut_chains, static_cast<kf_ull>(cuts));
  }
}

struct MpWhere { // where a chain's anchors are
  uint32_t s0, first;
};

// the chain table in output order (rule 8), without the exact-mode figures
__global__ __launch_bounds__(256) void k_mp_table(const uint32_t *list_kept, uint32_t n_kept, const uint32_t *gstart, const uint64_t *ug,
                                                  const uint64_t *xy, const MpRaw *raw, const uint32_t *n_emit, const uint32_t *chain_off,
                                                  const uint32_t *qlen, int k, msgpu_map_chain *out, MpWhere *where, uint32_t *n_pairs,
                                                  uint32_t cap) {
  const uint32_t kk = blockIdx.x * 256 + threadIdx.x;
  if (kk >= n_kept) return;
  const uint32_t gi = list_kept[kk], s0 = gstart[gi];
  const uint64_t g = ug[gi];
  const uint32_t q = static_cast<uint32_t>(g >> 32), t = static_cast<uint32_t>(g & 0xffffffffu) >> 1, s = g & 1u;
  for (uint32_t e = 0; e < n_emit[kk]; ++e) {
    const uint32_t at = chain_off[kk] + e;
    if (at >= cap) return;
    const MpRaw    c = raw[s0 + e];
    const uint64_t lo = xy[s0 + c.last], hi = xy[s0 + c.first];
    const uint32_t y0 = static_cast<uint32_t>(lo), y1 = static_cast<uint32_t>(hi);
    msgpu_map_chain o;
    o.query     = q;
    o.target    = t;
    o.strand    = s;
    o.n_anchors = c.n_anchors;
    o.score     = c.score;
    o.nm        = 0;
    o.t_start   = static_cast<uint32_t>(lo >> 32);
    o.t_end     = static_cast<uint32_t>(hi >> 32) + k;
    o.q_start   = s ? qlen[q] - y1 - k : y0;
    o.q_end     = s ? qlen[q] - y0 : y1 + k;
    o.matches   = c.seed_matches;
    o.block     = c.block;
    out[at]     = o;
    where[at]   = MpWhere{s0, c.first};
    n_pairs[at] = c.n_pairs;
  }
}

// exact mode: the segment pairs of every emitted chain, from its last link to its first.  The targets lie in their store
// (toff); the batch's query records lie one behind the other in its oriented buffer, the first at 0 (qpre: the bases in front
// of every query record of the file, q_base: in front of the batch's first), the reverse complements rc_base further on
__global__ __launch_bounds__(256) void k_mp_pairs(const msgpu_map_chain *chains, const MpWhere *where, uint32_t n_chains, const uint64_t *xy,
                                                  const int32_t *pred, const uint32_t *pair_off, const uint64_t *toff, const uint64_t *qpre,
                                                  uint64_t q_base, uint64_t rc_base, int k, msgpu_align_pair *pairs, uint32_t cap,
                                                  uint32_t *trail, uint32_t *head) {
  const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= n_chains) return;
  const msgpu_map_chain c = chains[ci];
  const uint32_t        s0 = where[ci].s0;
  const uint64_t        ta = toff[c.target], qa = qpre[c.query] - q_base + (c.strand ? rc_base : 0);
  uint32_t              at = pair_off[ci], cur = where[ci].first;
  uint32_t              run = 0; // cigar mode: the seed columns ('=') behind the segment that comes next, i.e. in front of `cur`
  for (uint32_t l = 1; l < c.n_anchors; ++l) {
    if (pred[s0 + cur] < 0) break; // (a chain of n_anchors has n_anchors - 1 links)
    const uint32_t pr = static_cast<uint32_t>(pred[s0 + cur]);
    const uint64_t vi = xy[s0 + cur];
    const MpLink   L = mp_link(vi, xy[s0 + pr], k);
    if ((L.lt | L.lq) && at < cap) {
      const uint32_t xe = static_cast<uint32_t>(vi >> 32) + k - L.c, ye = static_cast<uint32_t>(vi) + k - L.c;
      if (trail) trail[at] = run + L.c;
      pairs[at++] = msgpu_align_pair{ta + xe - L.lt, qa + ye - L.lq, L.lt, L.lq};
      run = 0;
    } else {
      run += L.c;
    }
    cur = pr;
  }
  if (head) head[ci] = run + static_cast<uint32_t>(k); // (anchor 0's k columns lead the alignment)
}

__global__ __launch_bounds__(256) void k_mp_exact(msgpu_map_chain *chains, uint32_t n_chains, const uint32_t *nm) {
  const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= n_chains) return;
  chains[ci].nm      = nm[ci];
  chains[ci].matches = chains[ci].block - nm[ci];
}

// rule 10's figures of a segment pair: its '=' columns and all its columns (a capped pair: none, and lt + lq); the X, D
// and I columns of the scripts are counted on the way (xid[0..2])
__global__ __launch_bounds__(256) void k_mp_columns(const msgpu_align_pair *pairs, const uint32_t *dist, const uint64_t *off,
                                                    const uint32_t *words, uint32_t n, uint32_t band, uint32_t *eq, uint32_t *cols,
                                                    kf_ull *xid) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  uint32_t       cnt[3] = {0, 0, 0};
  if (i < n) {
    const uint32_t d = dist[i];
    if (d > band) {
      eq[i]   = 0;
      cols[i] = pairs[i].a_len + pairs[i].b_len;
    } else {
      uint32_t e = 0;
      for (uint64_t w = off[i]; w < off[i + 1]; ++w) {
        const uint32_t v = words[w];
        e += v & 0x3fffffffu;
        if (v >> 30) ++cnt[(v >> 30) - 1];
      }
      eq[i]   = e;
      cols[i] = e + d;
    }
  }
  for (int o = 32; o > 0; o >>= 1)
    for (int j = 0; j < 3; ++j) cnt[j] += __shfl_xor(cnt[j], o);
  if ((threadIdx.x & 63) == 0)
    for (int j = 0; j < 3; ++j)
      if (cnt[j]) atomicAdd(&xid[j], static_cast<kf_ull>(cnt[j]));
}

// cigar mode's figures of a chain: its seed columns (matches as k_mp_table left it) and its segments' columns
__global__ __launch_bounds__(256) void k_mp_cigar(msgpu_map_chain *chains, uint32_t n_chains, const uint32_t *eq, const uint32_t *cols) {
  const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= n_chains) return;
  const uint32_t seed = chains[ci].matches;
  chains[ci].matches  = seed + eq[ci];
  chains[ci].block    = seed + cols[ci];
  chains[ci].nm       = cols[ci] - eq[ci];
}

// rule 11.1: the flank pairs of every chain.  The left ends, read backwards (their offsets name the byte behind the flank),
// are pairs[0, n_chains); the right ends lie behind them.  The oriented query range is rule 7's, turned back
__global__ __launch_bounds__(256) void k_mp_ends(const msgpu_map_chain *chains, uint32_t n_chains, const uint64_t *toff, const uint32_t *tlen,
                                                 const uint64_t *qpre, const uint32_t *qlen, uint64_t q_base, uint64_t rc_base, uint32_t E,
                                                 msgpu_align_pair *pairs) {
  const uint32_t ci = blockIdx.x * 256 + threadIdx.x;
  if (ci >= n_chains) return;
  const msgpu_map_chain c = chains[ci];
  const uint32_t        ql = qlen[c.query], tl = tlen[c.target];
  const uint32_t        y0 = c.strand ? ql - c.q_end : c.q_start, ye = c.strand ? ql - c.q_start : c.q_end;
  const uint64_t        ta = toff[c.target], qa = qpre[c.query] - q_base + (c.strand ? rc_base : 0);
  pairs[ci]            = msgpu_align_pair{ta + c.t_start, qa + y0, min(E, c.t_start), min(E, y0)};
  pairs[n_chains + ci] = msgpu_align_pair{ta + c.t_end, qa + ye, min(E, tl - c.t_end), min(E, ql - ye)};
}

__global__ __launch_bounds__(256) void k_mp_capped(const uint32_t *dist, uint32_t n, uint32_t band, kf_ull *capped) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  wave_count(i < n && dist[i] > band, capped);
}

// ---- rule 12: primaries, secondaries and mapping quality over the chains of a query record ("segment": the chains of one
// query record, consecutive in the table).  k_rk_heads marks where `query` changes (and, for a table from the host, looks for
// the first chain that breaks the table's order), a scan numbers the segments, k_rk_classify settles the segments of one chain
// and splits the others into those of at most 64 chains (k_rk_wave: a lane per chain) and the longer ones (k_rk_list: the
// chains in 12.1's order by one segmented sort, the primaries found so far in LDS and, beyond MSGPU_MAP_RANK_LDS of them, in
// the segment's stretch of the arena).  Both write `parent` only; k_rk_figures gathers sub and n_secondary per primary (an
// integer maximum and an integer sum: no order reaches the output) and k_rk_rows writes the rows in output order.

enum { RK_PRIM = 0, RK_SEC, RK_MAPQ0, RK_LARGEST, RK_SINGLE, RK_WAVE, RK_LIST, RK_SPILL, RK_BAD, RK_COUNT };

struct RkPrim { // a primary of the segment being visited
  uint32_t qs, qe, idx;
};

// 12.2's test of a chain's query range against a primary's: 2 * ov > min(len, len)
__device__ __forceinline__ bool rk_masks(uint32_t cs, uint32_t ce, uint32_t ps, uint32_t pe) {
  const uint32_t lo = max(cs, ps), hi = min(ce, pe);
  const uint64_t ov = hi > lo ? hi - lo : 0;
  return 2 * ov > min(ce - cs, pe - ps);
}

__device__ __forceinline__ uint64_t rk_key(int32_t score, uint32_t i) { // descending: (score descending, index ascending)
  return (static_cast<uint64_t>(static_cast<uint32_t>(score) ^ 0x80000000u) << 32) | (0xffffffffu - i);
}

__global__ __launch_bounds__(256) void k_rk_heads(const msgpu_map_chain *chains, uint32_t n, int validate, uint32_t *head, kf_ull *bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = chains[i].query, qp = i ? chains[i - 1].query : 0;
  head[i] = !i || q != qp;
  if (validate && ((i && q < qp) || chains[i].q_start > chains[i].q_end)) atomicMin(bad, static_cast<kf_ull>(i));
}

__global__ __launch_bounds__(256) void k_rk_classify(const uint32_t *start, uint32_t n_seg, uint32_t *flag_wave, uint32_t *flag_list,
                                                     uint32_t *parent, kf_ull *cnt) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  const uint32_t n = s < n_seg ? start[s + 1] - start[s] : 0;
  if (s < n_seg) {
    flag_wave[s] = n >= 2 && n <= 64;
    flag_list[s] = n > 64;
    if (n == 1) parent[start[s]] = start[s]; // settled: a primary without a secondary
  }
  wave_count(n == 1, cnt + RK_SINGLE);
  wave_count(n >= 2 && n <= 64, cnt + RK_WAVE);
  wave_count(n > 64, cnt + RK_LIST);
  wave_max(n, cnt + RK_LARGEST);
}

__global__ __launch_bounds__(256) void k_rk_lists(const uint32_t *start, uint32_t n_seg, const uint32_t *flag_wave, const uint32_t *flag_list,
                                                  const uint32_t *pos_wave, const uint32_t *pos_list, uint32_t *list_wave,
                                                  uint32_t *list_list, uint32_t *seg_begin, uint32_t *seg_end) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s >= n_seg) return;
  if (flag_wave[s]) list_wave[pos_wave[s]] = s;
  if (flag_list[s]) {
    list_list[pos_list[s]] = s;
    seg_begin[pos_list[s]] = start[s];
    seg_end[pos_list[s]]   = start[s + 1];
  }
}

// segments of 2 to 64 chains: a wavefront per segment.  Every lane counts the chains in front of its own in 12.1's order, the
// chains move to the lane of their rank, and the visit is n uniform steps: step t gives chain t's range to the primaries in the
// lanes below t, and the lowest lane that answers is the first primary in visiting order
__global__ __launch_bounds__(256) void k_rk_wave(const msgpu_map_chain *chains, const uint32_t *start, const uint32_t *list, uint32_t n_list,
                                                 uint32_t *parent) {
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63;
  if (wv >= n_list) return; // (whole wavefronts leave)
  const uint32_t s = list[wv], s0 = start[s], n = start[s + 1] - s0;
  const bool     have = lane < n;
  int            score = 0, qs = 0, qe = 0;
  if (have) {
    score = chains[s0 + lane].score;
    qs    = static_cast<int>(chains[s0 + lane].q_start);
    qe    = static_cast<int>(chains[s0 + lane].q_end);
  }
  uint32_t r = 0;
  for (uint32_t j = 0; j < n; ++j) {
    const int sj = __shfl(score, static_cast<int>(j));
    r += sj > score || (sj == score && j < lane);
  }
  if (!have) r = lane; // (the ranks of the chains are 0..n-1: the other lanes keep their place)
  const int to = static_cast<int>(r * 4);
  qs = __builtin_amdgcn_ds_permute(to, qs);
  qe = __builtin_amdgcn_ds_permute(to, qe);
  const uint32_t idx = static_cast<uint32_t>(__builtin_amdgcn_ds_permute(to, static_cast<int>(lane))); // lane r holds chain idx
  bool     prim = false;
  uint32_t par = lane;
  for (uint32_t t = 0; t < n; ++t) {
    const uint32_t bs = static_cast<uint32_t>(__shfl(qs, static_cast<int>(t))), be = static_cast<uint32_t>(__shfl(qe, static_cast<int>(t)));
    const uint64_t who = __ballot(lane < t && prim && rk_masks(bs, be, static_cast<uint32_t>(qs), static_cast<uint32_t>(qe)));
    if (lane == t) {
      if (who) par = static_cast<uint32_t>(__ffsll(static_cast<long long>(who))) - 1;
      else prim = true;
    }
  }
  const uint32_t pidx = static_cast<uint32_t>(__shfl(static_cast<int>(idx), static_cast<int>(par)));
  if (have) parent[s0 + idx] = s0 + pidx;
}

__global__ __launch_bounds__(256) void k_rk_keys(const msgpu_map_chain *chains, uint32_t n, uint64_t *keys) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) keys[i] = rk_key(chains[i].score, i);
}

// segments of more than 64 chains: a wavefront (a workgroup of one) per segment walks the chains in 12.1's order, 64 at a time
// in registers.  The primaries found so far are a list in visiting order: entry e lies in LDS for e < MSGPU_MAP_RANK_LDS, else
// at far[e], the segment's own stretch of `spill` (entry e of a segment of n chains has e < n).  A visited chain reads the list
// 64 entries per ballot and stops at the first ballot that is not empty: its lowest lane is the parent
__global__ __launch_bounds__(64) void k_rk_list(const msgpu_map_chain *chains, const uint32_t *start, const uint32_t *list,
                                                const uint64_t *sorted, uint32_t *parent, RkPrim *spill, kf_ull *spilled) {
  __shared__ RkPrim s_p[MSGPU_MAP_RANK_LDS];
  const uint32_t s = list[blockIdx.x], s0 = start[s], n = start[s + 1] - s0, lane = threadIdx.x;
  RkPrim        *far = spill + s0;
  uint32_t       np = 0;
  for (uint32_t b0 = 0; b0 < n; b0 += 64) {
    const bool     have = b0 + lane < n;
    const uint32_t idx = have ? 0xffffffffu - static_cast<uint32_t>(sorted[s0 + b0 + lane]) : 0;
    const int      qs = have ? static_cast<int>(chains[idx].q_start) : 0, qe = have ? static_cast<int>(chains[idx].q_end) : 0;
    const uint32_t m = min(64u, n - b0);
    for (uint32_t t = 0; t < m; ++t) {
      const uint32_t bs = static_cast<uint32_t>(__shfl(qs, static_cast<int>(t))), be = static_cast<uint32_t>(__shfl(qe, static_cast<int>(t)));
      const uint32_t bi = static_cast<uint32_t>(__shfl(static_cast<int>(idx), static_cast<int>(t)));
      uint32_t       par = bi;
      bool           found = false;
      for (uint32_t e0 = 0; e0 < np && !found; e0 += 64) {
        const uint32_t e = e0 + lane;
        RkPrim         p{0, 0, 0};
        if (e < np) p = e < MSGPU_MAP_RANK_LDS ? s_p[e] : far[e];
        const uint64_t who = __ballot(e < np && rk_masks(bs, be, p.qs, p.qe));
        if (who) {
          par   = static_cast<uint32_t>(__shfl(static_cast<int>(p.idx), __ffsll(static_cast<long long>(who)) - 1));
          found = true;
        }
      }
      if (!found) { // (uniform: `who` is a ballot) a new primary, behind every earlier one
        if (lane == 0) {
          if (np < MSGPU_MAP_RANK_LDS) s_p[np] = RkPrim{bs, be, bi};
          else far[np] = RkPrim{bs, be, bi};
        }
        ++np;
        __syncthreads();
      }
      if (lane == 0) parent[bi] = par;
    }
  }
  if (lane == 0 && np > MSGPU_MAP_RANK_LDS) atomicAdd(spilled, 1ull);
}

// 12.3: sub as the greatest (score biased to unsigned) + 1, so that 0 is "no secondary"
__global__ __launch_bounds__(256) void k_rk_figures(const msgpu_map_chain *chains, const uint32_t *parent, uint32_t n, kf_ull *sub,
                                                    uint32_t *n_sec) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t p = parent[i];
  if (p == i) return;
  const int32_t sc = chains[i].score;
  atomicMax(sub + p, static_cast<kf_ull>(static_cast<uint32_t>(sc) ^ 0x80000000u) + 1);
  if (10ll * sc >= 9ll * chains[p].score) atomicAdd(n_sec + p, 1u);
}

// 12.4 and the rows, in output order; `base`: the chains of the run in front of this table
__global__ __launch_bounds__(256) void k_rk_rows(const msgpu_map_chain *chains, const uint32_t *parent, const kf_ull *sub, const uint32_t *n_sec,
                                                 uint32_t n, uint32_t base, msgpu_map_rank *rows, kf_ull *cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool           prim = false, zero = false;
  if (i < n) {
    const uint32_t p = parent[i];
    msgpu_map_rank r{base + p, 0, 0, 0};
    prim = p == i;
    if (prim) {
      const long long s1 = chains[i].score;
      r.sub         = sub[i] ? static_cast<int32_t>(static_cast<uint32_t>(sub[i] - 1) ^ 0x80000000u) : 0;
      r.n_secondary = n_sec[i];
      if (s1 > 0) {
        const long long v = (60ll * (s1 - r.sub) * min(chains[i].n_anchors, 10u)) / (10ll * s1);
        r.mapq = static_cast<uint32_t>(v < 0 ? 0 : v > 60 ? 60 : v);
      }
    }
    zero    = r.mapq == 0;
    rows[i] = r;
  }
  wave_count(prim, cnt + RK_PRIM);
  wave_count(i < n && !prim, cnt + RK_SEC);
  wave_count(i < n && zero, cnt + RK_MAPQ0);
}

// ---- rule 13: mates.  A segment is the chains of one pair (query >> 1), consecutive in the table, mate 1's chains in front:
// a start and the two counts n1, n2.  k_mt_heads marks where the pair changes (and, for a table from the host, looks for the
// first chain that breaks 13's conditions), a scan numbers the segments, k_mt_classify settles with a lane per pair the pairs
// with n1 * n2 = 0 and with n1 = n2 = 1 and appends the others to three lists: at most 16 chains (k_mt_lanes<16>: four pairs
// per wavefront, a row of 16 lanes each), at most 64 (k_mt_lanes<64>: a wavefront per pair), more (k_mt_list: tiles of 64
// mate-1 chains in registers against tiles of mate-2 chains in LDS).  All three leave one MtSel per pair; k_mt_rows writes
// the rows in output order and the counts.  The lists are in no fixed order: a pair's selection depends on its chains alone.

enum { MT_PROPER = 0, MT_AMBIG, MT_DISCORD, MT_SINGLE, MT_SETTLED, MT_L16, MT_L64, MT_LIST, MT_LARGEST, MT_TLSUM, MT_TLMIN, MT_TLMAX, MT_BAD,
       MT_COUNT };
constexpr uint32_t MT_NONE = 0xffffffffu, MT_TILE = 256;

struct MtChain { // what 13.1 and 13.2 read of a chain, behind rule 11's extension
  uint32_t target, ts, te, strand;
  int32_t  score;
};
struct MtSel { // the selection of a pair: a, b index the table (MT_NONE: no concordant combination)
  uint32_t a, b, tl, n_best;
};
struct MtAcc { // a lane's best combination so far as 13.2's key in two words (greater is better), and the combinations at its best sum
  uint64_t hi, lo, cnt;
};

// chain i of a table of n; ends (rule 11, or null): the left end cells, then the right ones, whose x move the target range
__device__ __forceinline__ MtChain mt_load(const msgpu_map_chain *chains, const msgpu_ext_end *ends, uint32_t n, uint32_t i) {
  const msgpu_map_chain c = chains[i];
  MtChain m{c.target, c.t_start, c.t_end, c.strand, c.score};
  if (ends) {
    m.ts -= ends[i].x;
    m.te += ends[n + i].x;
  }
  return m;
}

// 13.1; *tl is written for a concordant combination
__device__ __forceinline__ bool mt_concordant(const MtChain &a, const MtChain &b, uint32_t max_insert, uint32_t *tl) {
  if (a.target != b.target || a.strand == b.strand) return false;
  const MtChain &f = a.strand ? b : a, &r = a.strand ? a : b;
  if (f.ts > r.ts || f.te > r.te || r.te < f.ts) return false;
  const uint32_t d = r.te - f.ts;
  *tl = d;
  return d <= max_insert;
}

// 13.2's key without truncation: hi = (sum + 2^32) in 33 bits, then 2^31 - 1 - tl in 31 (tl <= max_insert < 2^31);
// lo = the complements of the two indices inside the pair.  lo > 0: an index is below 2^32 - 1
__device__ __forceinline__ void mt_take(MtAcc &acc, const MtChain &a, const MtChain &b, uint32_t ia, uint32_t ib, uint32_t max_insert) {
  uint32_t tl;
  if (!mt_concordant(a, b, max_insert, &tl)) return;
  const uint64_t sum = static_cast<uint64_t>(static_cast<long long>(a.score) + b.score + (1ll << 32));
  const uint64_t hi = (sum << 31) | (0x7fffffffu - tl), lo = (static_cast<uint64_t>(~ia) << 32) | static_cast<uint32_t>(~ib);
  const uint64_t best = acc.hi >> 31;
  if (!acc.cnt || sum > best) acc.cnt = 1;
  else if (sum == best) ++acc.cnt;
  if (hi > acc.hi || (hi == acc.hi && lo > acc.lo)) {
    acc.hi = hi;
    acc.lo = lo;
  }
}

// the sum of every aligned group of W lanes (W = 16 or 64), in all of its lanes: group_max_i64's exchanges.  All 64 lanes active
template <int CTRL> __device__ __forceinline__ uint64_t mt_dpp_add(uint64_t v) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(static_cast<uint32_t>(v)), CTRL, 0xf, 0xf, false));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(static_cast<uint32_t>(v >> 32)), CTRL, 0xf, 0xf, false));
  return v + ((static_cast<uint64_t>(hi) << 32) | lo);
}
template <int W> __device__ __forceinline__ uint64_t mt_group_sum(uint64_t v) {
  static_assert(W == 16 || W == 64, "group width");
  v = mt_dpp_add<0xb1>(v);  // quad_perm:[1,0,3,2]
  v = mt_dpp_add<0x4e>(v);  // quad_perm:[2,3,0,1]
  v = mt_dpp_add<0x141>(v); // row_half_mirror
  v = mt_dpp_add<0x140>(v); // row_mirror
  if constexpr (W == 64) {
    auto lo = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(v), static_cast<uint32_t>(v), false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(v >> 32), static_cast<uint32_t>(v >> 32), false, false);
    v = ((static_cast<uint64_t>(hi[0]) << 32) | lo[0]) + ((static_cast<uint64_t>(hi[1]) << 32) | lo[1]);
    lo = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(v), static_cast<uint32_t>(v), false, false);
    hi = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(v >> 32), static_cast<uint32_t>(v >> 32), false, false);
    v = ((static_cast<uint64_t>(hi[0]) << 32) | lo[0]) + ((static_cast<uint64_t>(hi[1]) << 32) | lo[1]);
  }
  return v;
}

// the lanes' accumulators of a group of W lanes -> the pair's selection, in every lane of the group.  Two maxima (the first
// word, then the second among the lanes that hold the first) and one sum (the counts of the lanes whose best sum is the
// pair's); a lane without a combination has cnt = 0 and the smallest key.  s0: the pair's first chain, n1: its mate-1 chains
template <int W> __device__ __forceinline__ MtSel mt_select(const MtAcc &acc, uint32_t s0, uint32_t n1) {
  constexpr long long SIGN = static_cast<long long>(0x8000000000000000ull);
  const uint64_t any = mt_group_sum<W>(acc.cnt ? 1 : 0);
  const uint64_t hi = static_cast<uint64_t>(group_max_i64<W>(static_cast<long long>(acc.hi) ^ SIGN) ^ SIGN);
  const uint64_t lo = static_cast<uint64_t>(group_max_i64<W>(acc.cnt && acc.hi == hi ? static_cast<long long>(acc.lo) ^ SIGN : SIGN) ^ SIGN);
  const uint64_t nb = mt_group_sum<W>(acc.cnt && (acc.hi >> 31) == (hi >> 31) ? acc.cnt : 0);
  if (!any) return MtSel{MT_NONE, MT_NONE, 0, 0};
  return MtSel{s0 + ~static_cast<uint32_t>(lo >> 32), s0 + n1 + ~static_cast<uint32_t>(lo), 0x7fffffffu - static_cast<uint32_t>(hi & 0x7fffffffu),
               static_cast<uint32_t>(min(nb, static_cast<uint64_t>(0xffffffffu)))};
}

__global__ __launch_bounds__(256) void k_mt_heads(const msgpu_map_chain *chains, uint32_t n, int validate, uint32_t *head, kf_ull *bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t q = chains[i].query, qp = i ? chains[i - 1].query : 0;
  head[i] = !i || (q >> 1) != (qp >> 1);
  if (validate && ((i && q < qp) || chains[i].strand > 1 || chains[i].t_start > chains[i].t_end)) atomicMin(bad, static_cast<kf_ull>(i));
}

// a lane per pair: n1 by a binary search for the pair's first chain of mate 2 (no step for a pair of one or two chains)
__global__ __launch_bounds__(256) void k_mt_classify(const msgpu_map_chain *chains, const msgpu_ext_end *ends, uint32_t n_chains,
                                                     const uint32_t *start, uint32_t n_seg, uint32_t max_insert, uint32_t *n1_out, MtSel *sel,
                                                     uint32_t *list16, uint32_t *list64, uint32_t *listL, kf_ull *cursor, kf_ull *cnt) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  uint32_t       n = 0, n1 = 0, s0 = 0;
  if (s < n_seg) {
    s0 = start[s];
    n  = start[s + 1] - s0;
    uint32_t lo = 0, hi = n; // the first chain of the segment with an odd query record
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (chains[s0 + mid].query & 1u) hi = mid;
      else lo = mid + 1;
    }
    n1        = lo;
    n1_out[s] = n1;
  }
  const uint32_t n2 = n - n1;
  const bool     both = n1 && n2, one = both && n == 2;
  const bool     c16 = both && n > 2 && n <= 16, c64 = both && n > 16 && n <= 64, cl = both && n > 64;
  if (s < n_seg && !c16 && !c64 && !cl) {
    MtSel r{MT_NONE, MT_NONE, 0, 0};
    if (one) {
      uint32_t tl;
      if (mt_concordant(mt_load(chains, ends, n_chains, s0), mt_load(chains, ends, n_chains, s0 + 1), max_insert, &tl)) r = MtSel{s0, s0 + 1, tl, 1};
    }
    sel[s] = r;
  }
  const uint64_t a16 = wave_append(c16, cursor + 0), a64 = wave_append(c64, cursor + 1), al = wave_append(cl, cursor + 2);
  if (c16) list16[a16] = s;
  if (c64) list64[a64] = s;
  if (cl) listL[al] = s;
  wave_count(s < n_seg && !c16 && !c64 && !cl, cnt + MT_SETTLED);
  wave_count(c16, cnt + MT_L16);
  wave_count(c64, cnt + MT_L64);
  wave_count(cl, cnt + MT_LIST);
  wave_count(s < n_seg && !both, cnt + MT_SINGLE);
  wave_max(n, cnt + MT_LARGEST);
}

// pairs of at most W chains, 64 / W of them per wavefront: lane l of a group holds chain l of mate 1 and chain l of mate 2
// (n1, n2 < W), takes the mate-2 chains one by one through shuffles inside its group and keeps its best combination
template <int W>
__global__ __launch_bounds__(256) void k_mt_lanes(const msgpu_map_chain *chains, const msgpu_ext_end *ends, uint32_t n_chains, const uint32_t *start,
                                                  const uint32_t *n1s, const uint32_t *list, uint32_t n_list, uint32_t max_insert, MtSel *sel) {
  constexpr uint32_t PER = 64 / W;
  const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, gl = lane & (W - 1);
  if (wv * PER >= n_list) return; // (whole wavefronts leave; the reductions below need all 64 lanes)
  const uint32_t g = wv * PER + lane / W;
  const bool     live = g < n_list;
  const uint32_t s = live ? list[g] : 0, s0 = live ? start[s] : 0, n1 = live ? n1s[s] : 0, n2 = live ? start[s + 1] - s0 - n1 : 0;
  MtChain a{0, 0, 0, 0, 0}, b{0, 0, 0, 0, 0};
  if (gl < n1) a = mt_load(chains, ends, n_chains, s0 + gl);
  if (gl < n2) b = mt_load(chains, ends, n_chains, s0 + n1 + gl);
  MtAcc acc{0, 0, 0};
  for (uint32_t j = 0; j < W - 1 && __ballot(j < n2); ++j) {
    MtChain bj;
    bj.target = static_cast<uint32_t>(__shfl(static_cast<int>(b.target), static_cast<int>(j), W));
    bj.ts     = static_cast<uint32_t>(__shfl(static_cast<int>(b.ts), static_cast<int>(j), W));
    bj.te     = static_cast<uint32_t>(__shfl(static_cast<int>(b.te), static_cast<int>(j), W));
    bj.strand = static_cast<uint32_t>(__shfl(static_cast<int>(b.strand), static_cast<int>(j), W));
    bj.score  = __shfl(b.score, static_cast<int>(j), W);
    if (gl < n1 && j < n2) mt_take(acc, a, bj, gl, j, max_insert);
  }
  const MtSel r = mt_select<W>(acc, s0, n1);
  if (live && gl == 0) sel[s] = r;
}

// pairs of more than 64 chains: a wavefront (a workgroup of one) per pair.  Lane l holds chain a0 + l of mate 1; the mate-2
// chains pass through LDS MT_TILE at a time and every lane reads them all (one address per read: a broadcast)
__global__ __launch_bounds__(64) void k_mt_list(const msgpu_map_chain *chains, const msgpu_ext_end *ends, uint32_t n_chains, const uint32_t *start,
                                                const uint32_t *n1s, const uint32_t *list, uint32_t max_insert, MtSel *sel) {
  __shared__ MtChain s_b[MT_TILE];
  const uint32_t s = list[blockIdx.x], s0 = start[s], n1 = n1s[s], n2 = start[s + 1] - s0 - n1, lane = threadIdx.x;
  MtAcc          acc{0, 0, 0};
  for (uint32_t b0 = 0; b0 < n2; b0 += MT_TILE) {
    const uint32_t m = min(MT_TILE, n2 - b0);
    __syncthreads(); // (the tile before this one has been read)
    for (uint32_t e = lane; e < m; e += 64) s_b[e] = mt_load(chains, ends, n_chains, s0 + n1 + b0 + e);
    __syncthreads();
    for (uint32_t a0 = 0; a0 < n1; a0 += 64) {
      const bool    have = a0 + lane < n1;
      const MtChain a = have ? mt_load(chains, ends, n_chains, s0 + a0 + lane) : MtChain{0, 0, 0, 0, 0};
      if (have)
        for (uint32_t j = 0; j < m; ++j) mt_take(acc, a, s_b[j], a0 + lane, b0 + j, max_insert);
    }
  }
  const MtSel r = mt_select<64>(acc, s0, n1);
  if (lane == 0) sel[s] = r;
}

// 13.3 in output order; `base`: the chains of the run in front of this table.  The chain that opens a pair counts it
__global__ __launch_bounds__(256) void k_mt_rows(const uint32_t *head, const uint32_t *segid, const uint32_t *n1s, const uint32_t *start,
                                                 const MtSel *sel, uint32_t n, uint32_t base, msgpu_map_mate *rows, kf_ull *cnt) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  bool           proper = false, ambig = false, discord = false;
  uint32_t       tl = 0;
  if (i < n) {
    const uint32_t s = segid[i] + head[i] - 1; // (segid: the heads in front of chain i)
    const MtSel    r = sel[s];
    msgpu_map_mate row{MT_NONE, 0, 0, 0};
    if (r.a == i) row = msgpu_map_mate{base + r.b, r.tl, 1, r.n_best};
    else if (r.b == i) row = msgpu_map_mate{base + r.a, r.tl, 1, r.n_best};
    rows[i] = row;
    if (head[i]) {
      const uint32_t n1 = n1s[s], n2 = start[s + 1] - start[s] - n1;
      proper  = r.a != MT_NONE;
      ambig   = proper && r.n_best > 1;
      discord = !proper && n1 && n2;
      tl      = proper ? r.tl : 0;
    }
  }
  wave_count(proper, cnt + MT_PROPER);
  wave_count(ambig, cnt + MT_AMBIG);
  wave_count(discord, cnt + MT_DISCORD);
  wave_add(tl, cnt + MT_TLSUM);
  wave_max(tl, cnt + MT_TLMAX);
  wave_max(proper ? 0x80000000u - tl : 0u, cnt + MT_TLMIN); // (the smallest tl as the greatest 2^31 - tl; 0: no proper pair)
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_mapctx : msgpu::StageCtx {
  SeqCtxHold       seq;
  ScalarBlock      sc;
  msgpu_map_index *index = nullptr; // the one index the context holds (its targets lie in one of seq's two stores)
  uint32_t         extend = 0;      // rule 11's parameter (msgpu_map_set_extension)
  uint32_t         ranking = 0;     // rule 12's switch (msgpu_map_set_ranking)
  msgpu_map_rstats table_rstats{};  // of the last msgpu_map_rank_tables
  uint32_t         mates = 0, max_insert = 1000; // rule 13's switch and parameter (msgpu_map_set_mates)
  msgpu_map_mstats table_mstats{};  // of the last msgpu_map_mate_tables
  ~msgpu_mapctx();
  int open() {
    const int rc = msgpu_seq_create(device, &seq.p);
    return rc != MSGPU_OK ? rc : sc.create();
  }
};

struct msgpu_map_result {
  msgpu_map_stats              stats{};
  std::vector<msgpu_map_chain> chains;
  std::vector<msgpu_map_batch> batches; // rule 9's cut, in order
  uint64_t                     budget = 0; // the bytes a batch had: budget_bytes, or what it stood for
  std::string                  text;
  // cigar mode.  What comes back with the chain table, the batches one behind the other: per chain its '=' columns in front
  // of the first segment and its pairs (c_poff, n + 1 entries); per pair lt, lq, the '=' columns behind it and its words
  // (p_woff, pairs + 1 entries; none for a capped pair).  A chain's pairs lie from its last link to its first.
  msgpu_map_astats      astats{};
  std::vector<uint32_t> c_head, p_lt, p_lq, p_trail, words;
  std::vector<uint64_t> c_poff{0}, p_woff{0};
  std::vector<uint32_t> cg_ops;      // the run tables (msgpu_map_result_cigars)
  std::vector<uint64_t> cg_off{0};
  // rule 11.  Two ends per chain, the left one first; end j owns x_words[x_woff[j] .. x_woff[j + 1]), in its flank's order
  msgpu_map_xstats           xstats{};
  std::vector<msgpu_ext_end> x_ends;
  std::vector<uint32_t>      x_words;
  std::vector<uint64_t>      x_woff{0};
  // rule 12.  A row per chain when ranking was on
  msgpu_map_rstats            rstats{};
  std::vector<msgpu_map_rank> ranks;
  // rule 13.  A row per chain when mates was on
  msgpu_map_mstats            mstats{};
  std::vector<msgpu_map_mate> mates;
};

namespace {

enum { MP_SC_DROPK = 0, MP_SC_DROPE, MP_SC_LARGEST, MP_SC_TOTAL, MP_SC_TOTAL2, MP_SC_TOTAL3, MP_SC_DROP_SCORE, MP_SC_DROP_COUNT, MP_SC_CUT,
       MP_SC_CAPPED };
static_assert(MP_SC_CAPPED < SC_COUNT, "the scalar block");

inline kf_ull *mp_slot(msgpu_mapctx *c, int slot) { return reinterpret_cast<kf_ull *>(c->sc.d + slot); }

struct MpSketch {
  uint64_t *keys = nullptr, *vals = nullptr;
  uint64_t  n = 0;
};

int mp_sketch(msgpu_mapctx *c, DevArena &D, StageClock &clock, float *ms, const SeqRecs &R, int k, int w, const char *what, MpSketch &S) {
  hipStream_t    st = c->stream;
  const uint32_t tiles = grid_of(R.n_bases, MP_TILE);
  uint32_t      *d_cnt;
  uint64_t      *d_off;
  STAGE_HIP(c, D.get_zeroed(&d_cnt, tiles + 1ull, st));
  STAGE_HIP(c, D.get(&d_off, tiles + 1ull));
  STAGE_HIP(c, clock.begin(ms));
  if (tiles) hipLaunchKernelGGL((k_mp_sketch<false>), dim3(tiles), dim3(256), 0, st, R, k, w, d_cnt, nullptr, nullptr, nullptr, 0);
  STAGE_HIP(c, hipGetLastError());
  // (the last word is the zero above: d_off[tiles] is the total; every scan of this file reads through a const pointer, one
  // instantiation per output type)
  STAGE_HIP(c, stage_scan_total(D, st, d_cnt, d_off, tiles, c->sc, MP_SC_TOTAL));
  STAGE_HIP(c, clock.end());
  int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  S.n = c->sc.h[MP_SC_TOTAL];
  if (S.n >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "%s: %llu minimizers; the limit is 2^31 - 1", what, static_cast<kf_ull>(S.n));
    return MSGPU_E_ARG;
  }
  STAGE_HIP(c, D.get(&S.keys, S.n));
  STAGE_HIP(c, D.get(&S.vals, S.n));
  STAGE_HIP(c, clock.begin(ms));
  if (S.n) hipLaunchKernelGGL((k_mp_sketch<true>), dim3(tiles), dim3(256), 0, st, R, k, w, nullptr, d_off, S.keys, S.vals, S.n);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  D.drop(d_cnt);
  D.drop(d_off);
  return MSGPU_OK;
}

// rule 10: the merged runs of chain i as (BAM code, length), in target-forward order
constexpr uint32_t CG_INS = 1, CG_DEL = 2, CG_EQ = 7, CG_X = 8;
void mp_runs(const msgpu_map_result &r, uint64_t i, std::vector<std::pair<uint32_t, uint64_t>> &runs) {
  runs.clear();
  auto push = [&](uint32_t op, uint64_t len) {
    if (!len) return;
    if (!runs.empty() && runs.back().first == op) runs.back().second += len;
    else runs.emplace_back(op, len);
  };
  static const uint32_t code[4] = {CG_EQ, CG_X, CG_DEL, CG_INS};
  const bool ext = r.x_woff.size() > 2 * i + 2; // rule 11: the left end's columns in reverse order in front, the right end's behind
  if (ext)
    for (uint64_t w = r.x_woff[2 * i + 1]; w-- > r.x_woff[2 * i];) {
      if (r.x_words[w] >> 30) push(code[r.x_words[w] >> 30], 1);
      push(CG_EQ, r.x_words[w] & 0x3fffffffu);
    }
  push(CG_EQ, r.c_head[i]);
  for (uint64_t p = r.c_poff[i + 1]; p-- > r.c_poff[i];) { // (stored from the last link to the first)
    if (r.p_woff[p + 1] == r.p_woff[p]) { // capped
      push(CG_DEL, r.p_lt[p]);
      push(CG_INS, r.p_lq[p]);
    } else {
      for (uint64_t w = r.p_woff[p]; w < r.p_woff[p + 1]; ++w) {
        push(CG_EQ, r.words[w] & 0x3fffffffu);
        if (r.words[w] >> 30) push(code[r.words[w] >> 30], 1);
      }
    }
    push(CG_EQ, r.p_trail[p]);
  }
  if (ext)
    for (uint64_t w = r.x_woff[2 * i + 1]; w < r.x_woff[2 * i + 2]; ++w) {
      push(CG_EQ, r.x_words[w] & 0x3fffffffu);
      if (r.x_words[w] >> 30) push(code[r.x_words[w] >> 30], 1);
    }
}

void mp_format(const msgpu_map_chain &ch, const msgpu_seqfile *T, const msgpu_seqfile *Q, bool exact, std::string &out,
               const std::vector<std::pair<uint32_t, uint64_t>> *runs = nullptr, const msgpu_map_rank *rk = nullptr, bool primary = false,
               const msgpu_map_mate *mt = nullptr) {
  char buf[224];
  out += msgpu_seq_name(Q, ch.query);
  int n = snprintf(buf, sizeof(buf), "\t%llu\t%u\t%u\t%c\t", static_cast<kf_ull>(msgpu_seq_length(Q, ch.query)), ch.q_start, ch.q_end,
                   ch.strand ? '-' : '+');
  out.append(buf, n);
  out += msgpu_seq_name(T, ch.target);
  if (rk) // rule 12.5
    n = snprintf(buf, sizeof(buf), "\t%llu\t%u\t%u\t%u\t%u\t%u\ttp:A:%c\tcm:i:%u\ts1:i:%d\ts2:i:%d",
                 static_cast<kf_ull>(msgpu_seq_length(T, ch.target)), ch.t_start, ch.t_end, ch.matches, ch.block, rk->mapq, primary ? 'P' : 'S',
                 ch.n_anchors, ch.score, rk->sub);
  else
    n = snprintf(buf, sizeof(buf), "\t%llu\t%u\t%u\t%u\t%u\t255\tcm:i:%u\ts1:i:%d", static_cast<kf_ull>(msgpu_seq_length(T, ch.target)),
                 ch.t_start, ch.t_end, ch.matches, ch.block, ch.n_anchors, ch.score);
  out.append(buf, n);
  if (mt) { // rule 13.5
    if (mt->cls) n = snprintf(buf, sizeof(buf), "\tpr:A:P\tmi:i:%u\ttl:i:%u\tnb:i:%u", mt->mate, mt->tlen, mt->n_best);
    else n = snprintf(buf, sizeof(buf), "\tpr:A:U");
    out.append(buf, n);
  }
  if (exact) {
    n = snprintf(buf, sizeof(buf), "\tNM:i:%u", ch.nm);
    out.append(buf, n);
  }
  if (runs) {
    out += "\tcg:Z:";
    for (const auto &r : *runs) {
      n = snprintf(buf, sizeof(buf), "%llu%c", static_cast<kf_ull>(r.second), r.first == CG_EQ ? '=' : r.first == CG_X ? 'X' : r.first == CG_DEL ? 'D' : 'I');
      out.append(buf, n);
    }
  }
  out += '\n';
}

// ---- rule 9: the bytes of a batch and the cut

// What mp_batch takes from its reserved arena for A anchors and B query bases, allocation by allocation.  Groups, kept
// groups, chains and segment pairs are each at most the anchors (a chain holds an anchor that no other chain holds, and a
// chain of m anchors has m - 1 links).
constexpr uint64_t MP_BYTES_ANCHOR = 4 * 8           // g and xy, twice each: the grouping sorts go from one to the other; the
                                                     // second pair carries the sort keys of rule 6 afterwards
                                     + 8 + 2 * 4     // ug, gcnt, gstart
                                     + 9 * 4         // the class flags, their scans and the five lists
                                     + 2 * 4 + 1     // f, pred, used
                                     + sizeof(MpRaw) // raw
                                     + 2 * 4         // emit, coff
                                     + sizeof(msgpu_map_chain) + sizeof(MpWhere) + 2 * 4; // the chain table, where, np, poff
constexpr uint64_t MP_BYTES_ANCHOR_EXACT = sizeof(msgpu_align_pair) + 4 + 4;              // pairs, dist, nm
// The rocPRIM temporary, one buffer that the largest call sizes.  That call is radix_sort_pairs on separate input and output
// arrays: it keeps a second copy of the keys and of the values (2 * 8 bytes per anchor) and, per block of the one-sweep
// kernel, 256 look-back words of 4 bytes; a block sorts at least 256 items, so that is at most 4 bytes per anchor.
// segmented_radix_sort_keys keeps one copy of the keys and two segment indices per segment (8 + 2 * 4), run_length_encode,
// the scans and segmented_reduce keep a few words per block.  24 bytes per anchor cover the largest, and the fixed part
// (digit histograms of 8 places * 256 * 8 bytes, the merge sort's and the partitioner's block states) stays far below 1 MiB.
constexpr uint64_t MP_BYTES_ANCHOR_TMP = 24, MP_BYTES_TMP_FIXED = 1ull << 20;
// every allocation is rounded up to DevArena::ALIGN (fewer than 64 of them per batch), the arrays with one more word than
// items, the oriented copies' 16 bytes of slack
constexpr uint64_t MP_BYTES_FIXED = MP_BYTES_TMP_FIXED + 64 * DevArena::ALIGN + 64 * 8;
static_assert(sizeof(MpRaw) == 28 && sizeof(MpWhere) == 8 && sizeof(msgpu_align_pair) == 24, "rule 9's bytes per anchor");

// cigar mode (rule 10), per segment pair beside its band + 1 words of script: len, off (64 bits), list, trail, eq, cols; per
// chain: head and the two sums; fixed: the slab, the classes' counters and the column counters (two allocations)
constexpr uint64_t MP_BYTES_ANCHOR_CIGAR = 4 + 8 + 4 + 4 + 4 + 4 + 3 * 4, MP_BYTES_FIXED_CIGAR = 2 * DevArena::ALIGN;
// rule 11 (extend > 0), per chain two ends: a descriptor and an end cell each beside the band + 1 words of its script; fixed:
// the counter of inconsistent ends and the rounding of the three arrays (the slab is cigar mode's, allocated once)
constexpr uint64_t MP_BYTES_ANCHOR_EXT = 2 * (sizeof(msgpu_align_pair) + sizeof(msgpu_ext_end)), MP_BYTES_FIXED_EXT = 4 * DevArena::ALIGN;
static_assert(sizeof(msgpu_ext_end) == 24, "rule 11's bytes per end");
// rule 12 (ranking on), per chain, and a chain holds an anchor of its own: head, segment number, segment start, the two class
// flags and their scans (seven words); the two class lists and the sort's segment bounds (four words); parent, n_secondary
// and the 64-bit sub; the row; the sort keys twice; the primary's entry in the list class's stretch.  The sort is
// segmented_radix_sort_keys over at most as many keys as rule 6's, inside MP_BYTES_ANCHOR_TMP as that one is.  Fixed: the
// counters and the rounding of the nineteen arrays, each with at most one more word than items
constexpr uint64_t MP_BYTES_ANCHOR_RANK = 7 * 4 + 4 * 4 + 4 + 4 + 8 + sizeof(msgpu_map_rank) + 2 * 8 + sizeof(RkPrim);
constexpr uint64_t MP_BYTES_FIXED_RANK = 24 * DevArena::ALIGN;
static_assert(sizeof(msgpu_map_rank) == 16 && sizeof(RkPrim) == 12 && RK_COUNT * 8 <= DevArena::ALIGN, "rule 12's bytes per chain");

// rule 13 (mates on), per chain: head, segment number and segment start (three words), n1, the three class lists (three
// words), the pair's selection (16 bytes, one per segment) and the row (16 bytes).  The scan is the one rule 12 runs, inside
// MP_BYTES_ANCHOR_TMP.  Fixed: the counters with the lists' cursors and the rounding of the ten arrays, three of them with one
// more word than items
constexpr uint64_t MP_BYTES_ANCHOR_MATES = 3 * 4 + 4 + 3 * 4 + sizeof(MtSel) + sizeof(msgpu_map_mate);
constexpr uint64_t MP_BYTES_FIXED_MATES = 12 * DevArena::ALIGN;
static_assert(MP_BYTES_ANCHOR_MATES == MSGPU_MAP_MATES_ANCHOR_BYTES && MP_BYTES_FIXED_MATES == MSGPU_MAP_MATES_FIXED_BYTES &&
              sizeof(msgpu_map_mate) == 16 && sizeof(MtSel) == 16 && (MT_COUNT + 3) * 8 <= DevArena::ALIGN, "rule 13's bytes per chain");

uint64_t mp_batch_bytes(const msgpu_map_params &prm, uint32_t extend, uint32_t ranking, uint64_t n_anchors, uint64_t n_query_bases,
                        uint32_t mates = 0) {
  const bool     exact = prm.exact != 0, cigar = exact && prm.cigar != 0;
  const uint64_t band1 = static_cast<uint64_t>(prm.band < 0 ? 0 : prm.band > 127 ? 127 : prm.band) + 1;
  const bool     ext = cigar && extend != 0;
  const uint64_t per = MP_BYTES_ANCHOR + MP_BYTES_ANCHOR_TMP + (exact ? MP_BYTES_ANCHOR_EXACT : 0) +
                       (cigar ? MP_BYTES_ANCHOR_CIGAR + 4 * band1 : 0) + (ext ? MP_BYTES_ANCHOR_EXT + 2 * 4 * band1 : 0) +
                       (ranking ? MP_BYTES_ANCHOR_RANK : 0) + (mates ? MP_BYTES_ANCHOR_MATES : 0);
  // beyond every device, and no overflow: per < 2^8 (2^10 in cigar mode: band + 1 words of script per anchor beside the rest;
  // below 2^12 with rule 11's two more scripts, descriptors and end cells)
  if (n_anchors >= (1ull << (cigar ? 50 : 54)) || n_query_bases >= (1ull << 62)) return ~0ull;
  const uint64_t fixed = MP_BYTES_FIXED + (cigar ? MP_BYTES_FIXED_CIGAR + DevArena::aligned(4 * edit_script_slab_words(edit_script_slots(), static_cast<uint32_t>(band1 - 1))) : 0) +
                         (ext ? MP_BYTES_FIXED_EXT : 0) + (ranking ? MP_BYTES_FIXED_RANK : 0) + (mates ? MP_BYTES_FIXED_MATES : 0);
  return fixed + per * n_anchors + (exact ? 2 * n_query_bases : 0);
}

// The greedy cut of rule 9 over the prefix sums of the records' anchors and bases (n + 1 entries each): a binary search per
// batch for the last record that still fits.  Returns the first record that fits no batch on its own, or n.  With mates
// (rule 13.7; n is even) the unit is the pair: `unit` = 2 records, and the first record of the pair that does not fit
uint32_t mp_cut(const msgpu_map_params &prm, uint32_t extend, uint32_t ranking, uint32_t mates, const uint64_t *apre, const uint64_t *bpre,
                uint32_t n, uint64_t budget, std::vector<msgpu_map_batch> &out) {
  const uint32_t unit = mates ? 2 : 1;
  for (uint32_t first = 0; first < n;) {
    auto fits = [&](uint32_t end) {
      const uint64_t a = apre[end] - apre[first];
      return a < (1ull << 31) && mp_batch_bytes(prm, extend, ranking, a, bpre[end] - bpre[first], mates) <= budget;
    };
    if (!fits(first + unit)) return first;
    uint32_t lo = 1, hi = (n - first) / unit; // the last end that fits, in units behind `first`
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo + 1) >> 1);
      if (fits(first + mid * unit)) lo = mid;
      else hi = mid - 1;
    }
    lo = first + lo * unit;
    msgpu_map_batch b{};
    b.first_query   = first;
    b.n_queries     = lo - first;
    b.n_anchors     = apre[lo] - apre[first];
    b.n_query_bases = bpre[lo] - bpre[first];
    b.bytes_bound   = mp_batch_bytes(prm, extend, ranking, b.n_anchors, b.n_query_bases, mates);
    out.push_back(b);
    first = lo;
  }
  return n;
}

struct MpRun { // what stays on the device for the whole run (rule 9), as a batch sees it
  msgpu_mapctx           *c;
  const msgpu_map_params &prm;
  const StageFile        &Tf, &Qf;
  const MpSketch         &Qs;
  MpIndex                 X;
  const uint64_t         *d_aoff; // the anchors in front of every query minimizer
  const uint64_t         *d_bpre; // the bases in front of every query record
  const uint64_t         *first_min, *bpre; // on the host: every query record's first minimizer, and d_bpre
  int                     qkind;  // the store the query records lie in
  uint32_t               *d_nruns;
  kf_ull                 *d_hist; // 32 bins, summed over the batches
  StageClock             &clock;
  msgpu_map_result       *res;
  uint32_t                extend; // rule 11's parameter
  uint32_t                ranking; // rule 12's switch
  uint32_t                mates, max_insert; // rule 13's switch and parameter
};

// ---- rule 12 on a chain table that lies on the device

// n chains in output order -> n rows; `base` is added to every parent; `validate`: the table comes from the host and the first
// chain that breaks its order is an error before any ranking kernel runs (*bad: that chain, else ~0).  cnt: RK_COUNT
// counters on the host, valid after the caller's next synchronisation; the segments are added to S at once.
int mp_rank(msgpu_mapctx *c, DevArena &B, StageClock &clock, const msgpu_map_chain *d_chains, uint32_t n, uint32_t base, bool validate,
            msgpu_map_rank *d_rows, kf_ull *h_cnt, msgpu_map_rstats &S, uint64_t *bad) {
  hipStream_t st = c->stream;
  uint32_t   *d_head, *d_segid, *d_start, *d_fw, *d_fl, *d_pw, *d_pl, *d_lw, *d_ll, *d_parent, *d_nsec;
  kf_ull     *d_sub, *d_cnt;
  for (uint32_t **p : {&d_head, &d_segid, &d_start, &d_fw, &d_fl, &d_pw, &d_pl}) STAGE_HIP(c, B.get(p, n + 1ull));
  for (uint32_t **p : {&d_lw, &d_ll, &d_parent}) STAGE_HIP(c, B.get(p, n));
  STAGE_HIP(c, B.get_zeroed(&d_nsec, n, st));
  STAGE_HIP(c, B.get_zeroed(&d_sub, n, st));
  STAGE_HIP(c, B.get_zeroed(&d_cnt, RK_COUNT, st));
  STAGE_HIP(c, hipMemsetAsync(d_cnt + RK_BAD, 0xff, sizeof(kf_ull), st));
  STAGE_HIP(c, hipMemsetAsync(d_head + n, 0, 4, st));
  STAGE_HIP(c, clock.begin(&S.rank_ms));
  hipLaunchKernelGGL(k_rk_heads, dim3(grid256(n)), dim3(256), 0, st, d_chains, n, validate ? 1 : 0, d_head, d_cnt + RK_BAD);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(B, st, d_head, d_segid, n, c->sc, MP_SC_TOTAL));
  hipLaunchKernelGGL(k_stage_put<kf_ull>, dim3(1), dim3(64), 0, st, c->sc.d, MP_SC_TOTAL2, d_cnt + RK_BAD);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint32_t n_seg = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]);
  *bad = c->sc.h[MP_SC_TOTAL2];
  if (validate && *bad != ~0ull) return MSGPU_E_ARG; // (the caller names the chain)
  STAGE_HIP(c, hipMemsetAsync(d_fw + n_seg, 0, 4, st));
  STAGE_HIP(c, hipMemsetAsync(d_fl + n_seg, 0, 4, st));
  STAGE_HIP(c, clock.begin(&S.rank_ms));
  hipLaunchKernelGGL(k_stage_seg_starts<uint32_t>, dim3(grid256(n + 1ull)), dim3(256), 0, st, d_head, d_segid, n, d_start);
  hipLaunchKernelGGL(k_rk_classify, dim3(grid256(n_seg)), dim3(256), 0, st, d_start, n_seg, d_fw, d_fl, d_parent, d_cnt);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(B, st, d_fw, d_pw, n_seg, c->sc, MP_SC_TOTAL2));
  STAGE_HIP(c, stage_scan_total(B, st, d_fl, d_pl, n_seg, c->sc, MP_SC_TOTAL3));
  STAGE_HIP(c, clock.end());
  rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint32_t n_wave = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL2]), n_list = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL3]);
  uint32_t *d_sb = nullptr, *d_se = nullptr;
  uint64_t *d_key[2] = {nullptr, nullptr};
  RkPrim   *d_spill = nullptr;
  if (n_list) {
    STAGE_HIP(c, B.get(&d_sb, n_list));
    STAGE_HIP(c, B.get(&d_se, n_list));
    STAGE_HIP(c, B.get(&d_key[0], n));
    STAGE_HIP(c, B.get(&d_key[1], n));
    STAGE_HIP(c, B.get(&d_spill, n));
  }
  STAGE_HIP(c, clock.begin(&S.rank_ms));
  hipLaunchKernelGGL(k_rk_lists, dim3(grid256(n_seg)), dim3(256), 0, st, d_start, n_seg, d_fw, d_fl, d_pw, d_pl, d_lw, d_ll, d_sb, d_se);
  if (n_wave) hipLaunchKernelGGL(k_rk_wave, dim3(grid_of(n_wave, 4)), dim3(256), 0, st, d_chains, d_start, d_lw, n_wave, d_parent);
  STAGE_HIP(c, hipGetLastError());
  if (n_list) {
    hipLaunchKernelGGL(k_rk_keys, dim3(grid256(n)), dim3(256), 0, st, d_chains, n, d_key[0]);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_rocprim(B, [&](void *tmp, size_t &bytes) {
      return rocprim::segmented_radix_sort_keys_desc(tmp, bytes, d_key[0], d_key[1], n, n_list, d_sb, d_se, 0, 64, st);
    }));
    hipLaunchKernelGGL(k_rk_list, dim3(n_list), dim3(64), 0, st, d_chains, d_start, d_ll, d_key[1], d_parent, d_spill, d_cnt + RK_SPILL);
    STAGE_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_rk_figures, dim3(grid256(n)), dim3(256), 0, st, d_chains, d_parent, n, d_sub, d_nsec);
  hipLaunchKernelGGL(k_rk_rows, dim3(grid256(n)), dim3(256), 0, st, d_chains, d_parent, d_sub, d_nsec, n, base, d_rows, d_cnt);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipMemcpyAsync(h_cnt, d_cnt, RK_COUNT * sizeof(kf_ull), hipMemcpyDeviceToHost, st));
  S.n_segments += n_seg;
  return MSGPU_OK;
}

void mp_rank_counts(const kf_ull *h, msgpu_map_rstats &S) { // behind the synchronisation
  S.n_primaries += h[RK_PRIM];
  S.n_secondaries += h[RK_SEC];
  S.n_mapq0 += h[RK_MAPQ0];
  S.largest_segment = std::max<uint64_t>(S.largest_segment, h[RK_LARGEST]);
  S.n_segments_single += h[RK_SINGLE];
  S.n_segments_wave += h[RK_WAVE];
  S.n_segments_list += h[RK_LIST];
  S.n_segments_spilled += h[RK_SPILL];
}

// ---- rule 13 on a chain table that lies on the device

// n chains in output order -> n rows; d_ends: rule 11's end cells of these chains (the left ones, then the right ones) or null;
// `base` is added to every mate; `validate` and *bad as in mp_rank.  h_cnt: MT_COUNT counters on the host, valid after the
// caller's next synchronisation; *n_seg: the pairs with a chain.
int mp_mates(msgpu_mapctx *c, DevArena &B, StageClock &clock, const msgpu_map_chain *d_chains, const msgpu_ext_end *d_ends, uint32_t n,
             uint32_t base, uint32_t max_insert, bool validate, msgpu_map_mate *d_rows, kf_ull *h_cnt, float *ms, uint64_t *n_seg_out,
             uint64_t *bad) {
  hipStream_t st = c->stream;
  uint32_t   *d_head, *d_segid, *d_start, *d_n1, *d_l16, *d_l64, *d_ll;
  MtSel      *d_sel;
  kf_ull     *d_cnt; // the counters, then the three cursors of the class lists
  for (uint32_t **p : {&d_head, &d_segid, &d_start}) STAGE_HIP(c, B.get(p, n + 1ull));
  for (uint32_t **p : {&d_n1, &d_l16, &d_l64, &d_ll}) STAGE_HIP(c, B.get(p, n));
  STAGE_HIP(c, B.get(&d_sel, n));
  STAGE_HIP(c, B.get_zeroed(&d_cnt, MT_COUNT + 3, st));
  STAGE_HIP(c, hipMemsetAsync(d_cnt + MT_BAD, 0xff, sizeof(kf_ull), st));
  STAGE_HIP(c, hipMemsetAsync(d_head + n, 0, 4, st));
  STAGE_HIP(c, clock.begin(ms));
  hipLaunchKernelGGL(k_mt_heads, dim3(grid256(n)), dim3(256), 0, st, d_chains, n, validate ? 1 : 0, d_head, d_cnt + MT_BAD);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(B, st, d_head, d_segid, n, c->sc, MP_SC_TOTAL));
  hipLaunchKernelGGL(k_stage_put<kf_ull>, dim3(1), dim3(64), 0, st, c->sc.d, MP_SC_TOTAL2, d_cnt + MT_BAD);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint32_t n_seg = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]);
  *bad = c->sc.h[MP_SC_TOTAL2];
  if (validate && *bad != ~0ull) return MSGPU_E_ARG; // (the caller names the chain)
  STAGE_HIP(c, clock.begin(ms));
  hipLaunchKernelGGL(k_stage_seg_starts<uint32_t>, dim3(grid256(n + 1ull)), dim3(256), 0, st, d_head, d_segid, n, d_start);
  hipLaunchKernelGGL(k_mt_classify, dim3(grid256(n_seg)), dim3(256), 0, st, d_chains, d_ends, n, d_start, n_seg, max_insert, d_n1, d_sel, d_l16,
                     d_l64, d_ll, d_cnt + MT_COUNT, d_cnt);
  STAGE_HIP(c, hipGetLastError());
  for (int k = 0; k < 3; ++k) hipLaunchKernelGGL(k_stage_put<kf_ull>, dim3(1), dim3(64), 0, st, c->sc.d, MP_SC_TOTAL + k, d_cnt + MT_COUNT + k);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint32_t n16 = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]), n64 = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL2]),
                 nl = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL3]);
  STAGE_HIP(c, clock.begin(ms));
  if (n16) hipLaunchKernelGGL(k_mt_lanes<16>, dim3(grid_of(n16, 16)), dim3(256), 0, st, d_chains, d_ends, n, d_start, d_n1, d_l16, n16, max_insert, d_sel);
  if (n64) hipLaunchKernelGGL(k_mt_lanes<64>, dim3(grid_of(n64, 4)), dim3(256), 0, st, d_chains, d_ends, n, d_start, d_n1, d_l64, n64, max_insert, d_sel);
  if (nl) hipLaunchKernelGGL(k_mt_list, dim3(nl), dim3(64), 0, st, d_chains, d_ends, n, d_start, d_n1, d_ll, max_insert, d_sel);
  hipLaunchKernelGGL(k_mt_rows, dim3(grid256(n)), dim3(256), 0, st, d_head, d_segid, d_n1, d_start, d_sel, n, base, d_rows, d_cnt);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipMemcpyAsync(h_cnt, d_cnt, MT_COUNT * sizeof(kf_ull), hipMemcpyDeviceToHost, st));
  *n_seg_out = n_seg;
  return MSGPU_OK;
}

void mp_mate_counts(const kf_ull *h, uint64_t n_seg, msgpu_map_mstats &S) { // behind the synchronisation
  S.n_pairs += n_seg; // (the pairs with a chain; a run adds its pairs without one at its end)
  S.n_proper += h[MT_PROPER];
  S.n_ambiguous += h[MT_AMBIG];
  S.n_discordant += h[MT_DISCORD];
  S.n_single += h[MT_SINGLE];
  S.n_pairs_settled += h[MT_SETTLED];
  S.n_pairs_lanes16 += h[MT_L16];
  S.n_pairs_lanes64 += h[MT_L64];
  S.n_pairs_list += h[MT_LIST];
  S.largest_pair = std::max<uint64_t>(S.largest_pair, h[MT_LARGEST]);
  S.tlen_sum += h[MT_TLSUM];
  S.tlen_max = std::max<uint64_t>(S.tlen_max, h[MT_TLMAX]);
  if (h[MT_TLMIN]) {
    const uint64_t lo = 0x80000000ull - h[MT_TLMIN];
    S.tlen_min = S.n_proper == h[MT_PROPER] ? lo : std::min(S.tlen_min, lo); // (the first batch with a proper pair sets it)
  }
}

// ---- the batch's oriented query records, for exact mode's segment pairs and for rule 11's flanks

struct MpOriented { // the batch's query records as they are and reverse-complemented, one record behind the other, one copy behind the other
  uint8_t           *d = nullptr;    // 2 * n_query_bases + 16 bytes of the batch arena; null: not made yet
  msgpu_gather_plan *plan = nullptr; // (the gather reads it: it lives until the batch's last synchronisation)
  ~MpOriented() { msgpu_gather_plan_free(plan); }
};

// once per batch, by whoever needs the copies first.  ms: a span of the clock that begins in front of the gather and stays open
int mp_oriented(const MpRun &R, DevArena &B, const msgpu_map_batch &bt, float *ms, MpOriented &O) {
  msgpu_mapctx           *c = R.c;
  const uint32_t          q0 = bt.first_query, q1 = q0 + bt.n_queries, from = R.qkind ? MSGPU_COPY_ILLUMINA : 0u;
  const uint64_t          NB = bt.n_query_bases, b0 = R.bpre[q0];
  std::vector<msgpu_copy> pieces;
  try {
    pieces.reserve(2ull * bt.n_queries);
    for (uint32_t i = q0; i < q1; ++i) {
      const uint64_t o = msgpu_seq_offset(R.Qf.f, i), at = R.bpre[i] - b0;
      const uint32_t L = static_cast<uint32_t>(msgpu_seq_length(R.Qf.f, i));
      pieces.push_back(msgpu_copy{o, at, L, from});
      pieces.push_back(msgpu_copy{o, NB + at, L, from | MSGPU_COPY_REVCOMP});
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  int rc = msgpu_gather_plan_create(c->seq, pieces.data(), pieces.size(), &O.plan);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "gather plan: %s", msgpu_seq_last_error(c->seq));
    return rc;
  }
  STAGE_HIP(c, B.get(&O.d, 2 * NB + 16));
  if (ms) STAGE_HIP(c, R.clock.begin(ms));
  rc = msgpu_gather_run(c->seq, O.plan, O.d, 2 * NB + 16, c->stream);
  if (rc != MSGPU_OK) snprintf(c->err, sizeof(c->err), "gather: %s", msgpu_seq_last_error(c->seq));
  return rc;
}

// ---- rule 11: the ends of a batch's chains

struct MpExtBatch { // what the extension of a batch leaves for the host, valid after the batch's last synchronisation
  std::vector<msgpu_ext_end> ends;  // the left ends of the batch's chains, then the right ends
  std::vector<uint32_t>      words; // band + 1 words per end, e + 1 of them the script
  uint32_t                   broken = 0;
  const msgpu_ext_end       *d_ends = nullptr; // the same cells in the batch arena: rule 13 reads the target ranges behind them
};

// the descriptors (k_mp_ends), the extension of the left ends and of the right ends (launch_extend_ends), and their way back
int mp_extend(const MpRun &R, DevArena &B, const msgpu_map_batch &bt, const msgpu_map_chain *d_chains, uint32_t C_n, MpOriented &O,
              uint32_t *d_slab, MpExtBatch &xb) {
  msgpu_mapctx  *c = R.c;
  hipStream_t    st = c->stream;
  const uint32_t band = static_cast<uint32_t>(R.prm.band), slots = edit_script_slots();
  const uint64_t NB = bt.n_query_bases, b0 = R.bpre[bt.first_query], stride = band + 1ull, slab_words = edit_script_slab_words(slots, band);
  if (!O.d) { // (a batch without a segment pair)
    const int rc = mp_oriented(R, B, bt, nullptr, O);
    if (rc != MSGPU_OK) return rc;
  }
  const uint8_t *const d_or = O.d;
  if (!d_slab && slab_words) STAGE_HIP(c, B.get(&d_slab, slab_words));
  msgpu_align_pair *d_pairs;
  msgpu_ext_end    *d_ends;
  uint32_t         *d_words, *d_broken;
  STAGE_HIP(c, B.get(&d_pairs, 2ull * C_n));
  STAGE_HIP(c, B.get(&d_ends, 2ull * C_n));
  STAGE_HIP(c, B.get(&d_words, 2ull * C_n * stride));
  STAGE_HIP(c, B.get(&d_broken, 1));
  try {
    xb.ends.resize(2ull * C_n);
    xb.words.resize(2ull * C_n * stride);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, hipMemsetAsync(d_broken, 0, 4, st));
  STAGE_HIP(c, R.clock.begin(&R.res->xstats.extend_ms));
  hipLaunchKernelGGL(k_mp_ends, dim3(grid256(C_n)), dim3(256), 0, st, d_chains, C_n, R.Tf.recs.off, R.Tf.recs.len, R.d_bpre, R.Qf.recs.len, b0, NB, R.extend,
                     d_pairs);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, launch_extend_ends(st, R.Tf.recs.bases, d_or, d_pairs, C_n, band, true, d_slab, slots, d_ends, d_words, d_broken));
  STAGE_HIP(c, launch_extend_ends(st, R.Tf.recs.bases, d_or, d_pairs + C_n, C_n, band, false, d_slab, slots, d_ends + C_n,
                                  d_words + C_n * stride, d_broken));
  STAGE_HIP(c, R.clock.end());
  STAGE_HIP(c, R.clock.begin(&R.res->stats.copy_ms));
  STAGE_HIP(c, hipMemcpyAsync(xb.ends.data(), d_ends, xb.ends.size() * sizeof(msgpu_ext_end), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(xb.words.data(), d_words, xb.words.size() * 4, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(&xb.broken, d_broken, 4, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, R.clock.end());
  xb.d_ends = d_ends;
  return MSGPU_OK;
}

// rule 11.5 on the host: the last C_n chains of the result are the batch's; their ranges and figures grow by the ends' columns
int mp_extend_apply(const MpRun &R, uint32_t C_n, const MpExtBatch &xb) {
  msgpu_mapctx     *c = R.c;
  msgpu_map_result &res = *R.res;
  msgpu_map_xstats &X = res.xstats;
  const uint32_t    band = static_cast<uint32_t>(R.prm.band);
  const uint64_t    stride = band + 1ull;
  const size_t      have = res.chains.size() - C_n;
  X.n_inconsistent += xb.broken;
  try {
    for (uint32_t i = 0; i < C_n; ++i) {
      msgpu_map_chain &ch = res.chains[have + i];
      const uint64_t   tlen = msgpu_seq_length(R.Tf.f, ch.target), qlen = msgpu_seq_length(R.Qf.f, ch.query);
      for (int side = 0; side < 2; ++side) { // the left end, then the right one
        const size_t         j = side ? C_n + i : i;
        const msgpu_ext_end &E = xb.ends[j];
        const uint32_t      *w = xb.words.data() + j * stride;
        // what the cell claims is checked before anything is moved by it: its row, its words and the room the chain has
        const uint64_t t_room = side ? tlen - ch.t_end : ch.t_start;
        const uint64_t q_room = (side != 0) != (ch.strand != 0) ? qlen - ch.q_end : ch.q_start;
        uint64_t       eq = 0, cnt[4] = {0, 0, 0, 0};
        bool           bad = E.e > band || E.x > t_room || E.y > q_room;
        for (uint32_t t = 0; !bad && t <= E.e; ++t) {
          eq += w[t] & 0x3fffffffu;
          ++cnt[w[t] >> 30];
          bad = (t < E.e) != ((w[t] >> 30) != 0);
        }
        bad = bad || eq + cnt[1] + cnt[2] != E.x || eq + cnt[1] + cnt[3] != E.y;
        if (bad) {
          ++X.n_inconsistent;
          res.x_ends.push_back(msgpu_ext_end{0, 0, 0, 0, 0, E.rows});
          res.x_words.push_back(0);
          res.x_woff.push_back(res.x_words.size());
          continue;
        }
        if (side) ch.t_end += E.x;
        else ch.t_start -= E.x;
        if ((side != 0) != (ch.strand != 0)) ch.q_end += E.y;
        else ch.q_start -= E.y;
        ch.matches += static_cast<uint32_t>(eq);
        ch.block += static_cast<uint32_t>(eq) + E.e;
        ch.nm += E.e;
        res.x_ends.push_back(E);
        res.x_words.insert(res.x_words.end(), w, w + E.e + 1);
        res.x_woff.push_back(res.x_words.size());
        X.n_ends_extended += (E.x | E.y) != 0;
        X.n_ends_at_sequence_end += E.x == t_room || E.y == q_room;
        X.t_bases += E.x;
        X.q_bases += E.y;
        X.x_columns += cnt[1];
        X.d_columns += cnt[2];
        X.i_columns += cnt[3];
        X.max_e = std::max<uint64_t>(X.max_e, E.e);
        X.rows += E.rows;
      }
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  X.n_ends += 2ull * C_n;
  if (X.n_inconsistent) {
    snprintf(c->err, sizeof(c->err), "the tables of %llu chain ends contradict themselves (a defect of the extension kernel)",
             static_cast<kf_ull>(X.n_inconsistent));
    return MSGPU_E_STATE;
  }
  return MSGPU_OK;
}

// ---- rules 4 to 8 for the query records of one batch, a function per step (mp_batch calls them in order).  Every array is taken
// from the reserved arena B and indexed from the batch's first anchor; the record indices in g and in the chain table are the
// file's.  The counters of the scalar block and the histogram are sums (the largest group: a maximum) over the batches so
// far: nothing resets them.

struct MpBatch { // what a batch carries from step to step
  uint32_t A = 0, G = 0, n_small = 0, n_large = 0, n_kept = 0, C_n = 0, P = 0; // anchors, groups (of <= 16 anchors, of more, both), chains, pairs
  uint64_t Wn = 0;                                                              // the words of the scripts
  // rule 4: the anchors in (group, x, y) order, the groups' keys, sizes and starts; rule 6's sort keys in the sorts' spare buffers
  const uint64_t *d_xys = nullptr;
  uint64_t       *d_ug = nullptr, *d_sk[2] = {nullptr, nullptr};
  uint32_t       *d_gcnt = nullptr, *d_gstart = nullptr;
  // rule 6's pre-filter: the lists of the small, the large and the kept groups, the kept groups' stretches of the sort keys
  uint32_t *d_ls = nullptr, *d_ll = nullptr, *d_lk = nullptr, *d_sb = nullptr, *d_se = nullptr;
  // rule 5 and rule 6's walk: scores and predecessors, the anchors taken, the raw chains, their count per group and its scan
  int32_t  *d_f = nullptr, *d_pred = nullptr;
  uint8_t  *d_used = nullptr;
  MpRaw    *d_raw = nullptr;
  uint32_t *d_emit = nullptr, *d_coff = nullptr;
  // the chain table, where a chain lies, its pairs and their scan; rule 12's rows
  msgpu_map_chain *d_chains = nullptr;
  MpWhere         *d_where = nullptr;
  uint32_t        *d_np = nullptr, *d_poff = nullptr;
  msgpu_map_rank  *d_rows = nullptr;
  // rule 7: the pairs and their distances; cigar mode: the '=' columns behind a pair and in front of a chain's first
  msgpu_align_pair *d_pairs = nullptr;
  uint32_t         *d_dist = nullptr, *d_trail = nullptr, *d_head = nullptr;
  uint32_t         *d_slab = nullptr; // the tables of the slab class (cigar mode with a segment pair; rule 11 takes its own otherwise)
  MpOriented O;  // exact mode with a segment pair makes the copies, rule 11 otherwise
  MpExtBatch xb; // rule 11: what comes back with the chain table
  kf_ull     h_rk[RK_COUNT] = {}; // rule 12: the counters, likewise
  // rule 13: the rows, the counters and the pairs with a chain
  msgpu_map_mate *d_mrows = nullptr;
  kf_ull          h_mt[MT_COUNT] = {};
  uint64_t        n_mseg = 0;
};

// rule 4: expand, two stable sorts, the groups
int mp_expand(const MpRun &R, DevArena &B, msgpu_map_batch &bt, MpBatch &b) {
  msgpu_mapctx    *c = R.c;
  msgpu_map_stats &S = R.res->stats;
  hipStream_t      st = c->stream;
  const uint32_t   A = b.A;
  const uint64_t   m0 = R.first_min[bt.first_query], m1 = R.first_min[bt.first_query + bt.n_queries];
  uint64_t        *d_g[2], *d_xy[2];
  for (int i = 0; i < 2; ++i) {
    STAGE_HIP(c, B.get(&d_g[i], A));
    STAGE_HIP(c, B.get(&d_xy[i], A));
  }
  STAGE_HIP(c, B.get(&b.d_ug, A));
  STAGE_HIP(c, B.get(&b.d_gcnt, A + 1ull));
  STAGE_HIP(c, B.get(&b.d_gstart, A + 1ull));
  STAGE_HIP(c, R.clock.begin(&S.anchors_ms));
  hipLaunchKernelGGL((k_mp_anchors<true>), dim3(grid256(m1 - m0)), dim3(256), 0, st, R.X, R.Qs.keys, R.Qs.vals, m0, m1, R.Qf.recs.len, R.prm.k,
                     R.prm.ava, nullptr, R.d_aoff, d_g[0], d_xy[0], A);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  STAGE_HIP(c, R.clock.begin(&S.group_ms));
  STAGE_HIP(c, stage_sort_pairs(B, st, d_xy[0], d_xy[1], d_g[0], d_g[1], A)); // by (x, y)
  STAGE_HIP(c, stage_sort_pairs(B, st, d_g[1], d_g[0], d_xy[1], d_xy[0], A)); // then, stable, by group
  STAGE_HIP(c, stage_rocprim(B, [&](void *tmp, size_t &bytes) {
    return rocprim::run_length_encode(tmp, bytes, d_g[0], A, b.d_ug, b.d_gcnt, R.d_nruns, st);
  }));
  hipLaunchKernelGGL(k_stage_put<uint32_t>, dim3(1), dim3(64), 0, st, c->sc.d, MP_SC_TOTAL, R.d_nruns);
  STAGE_HIP(c, R.clock.end());
  const int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  b.G = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]);
  STAGE_HIP(c, hipMemsetAsync(b.d_gcnt + b.G, 0, 4, st));
  STAGE_HIP(c, stage_scan<const uint32_t *>(B, st, b.d_gcnt, b.d_gstart, b.G + 1ull));
  bt.n_groups = b.G;
  S.n_groups += b.G;
  b.d_xys   = d_xy[0];
  b.d_sk[0] = d_g[1]; // (free behind the sorts)
  b.d_sk[1] = d_xy[1];
  return MSGPU_OK;
}

// rule 6's pre-filter, the size classes
int mp_classes(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx    *c = R.c;
  msgpu_map_stats &S = R.res->stats;
  hipStream_t      st = c->stream;
  const uint32_t   G = b.G;
  const int        k = R.prm.k;
  uint32_t        *d_fs, *d_fl, *d_ps, *d_pl;
  for (uint32_t **p : {&d_fs, &d_fl, &d_ps, &d_pl}) STAGE_HIP(c, B.get(p, G + 1ull));
  for (uint32_t **p : {&b.d_ls, &b.d_ll, &b.d_lk, &b.d_sb, &b.d_se}) STAGE_HIP(c, B.get(p, G));
  STAGE_HIP(c, hipMemsetAsync(d_fs + G, 0, 4, st));
  STAGE_HIP(c, hipMemsetAsync(d_fl + G, 0, 4, st));
  STAGE_HIP(c, R.clock.begin(&S.group_ms));
  hipLaunchKernelGGL(k_mp_classify, dim3(grid256(G)), dim3(256), 0, st, b.d_gcnt, G, k, R.prm.min_score, R.prm.min_count, d_fs, d_fl, R.d_hist,
                     mp_slot(c, MP_SC_LARGEST));
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(B, st, d_fs, d_ps, G, c->sc, MP_SC_TOTAL2));
  STAGE_HIP(c, stage_scan_total(B, st, d_fl, d_pl, G, c->sc, MP_SC_TOTAL3));
  hipLaunchKernelGGL(k_mp_lists, dim3(grid256(G)), dim3(256), 0, st, b.d_gcnt, b.d_gstart, G, d_fs, d_fl, d_ps, d_pl, b.d_ls, b.d_ll, b.d_lk, b.d_sb,
                     b.d_se);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  const int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  b.n_small = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL2]);
  b.n_large = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL3]);
  b.n_kept  = b.n_small + b.n_large;
  S.n_groups_small += b.n_small;
  S.n_groups_large += b.n_large;
  S.n_groups_kept += b.n_kept;
  S.largest_group = c->sc.h[MP_SC_LARGEST];
  if (S.largest_group * static_cast<uint64_t>(k) >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "a group of %llu anchors: its scores do not fit 31 bits at k = %d", static_cast<kf_ull>(S.largest_group), k);
    return MSGPU_E_ARG;
  }
  return MSGPU_OK;
}

// rule 5
int mp_chain(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx *c = R.c;
  hipStream_t   st = c->stream;
  STAGE_HIP(c, B.get(&b.d_f, b.A));
  STAGE_HIP(c, B.get(&b.d_pred, b.A));
  STAGE_HIP(c, B.get_zeroed(&b.d_used, b.A, st));
  STAGE_HIP(c, B.get(&b.d_raw, b.A));
  STAGE_HIP(c, B.get_zeroed(&b.d_emit, b.n_kept + 1ull, st));
  STAGE_HIP(c, B.get(&b.d_coff, b.n_kept + 1ull));
  MpChainArgs ca{b.d_ll, b.n_large, b.d_gstart, b.d_gcnt, b.d_xys, b.d_f, b.d_pred, b.d_sk[0], R.prm.k, R.prm.max_gap, R.prm.bandwidth};
  STAGE_HIP(c, R.clock.begin(&R.res->stats.chain_ms));
  if (b.n_large) hipLaunchKernelGGL(k_mp_chain, dim3(grid_of(b.n_large, 4)), dim3(256), 0, st, ca);
  ca.list   = b.d_ls;
  ca.n_list = b.n_small;
  if (b.n_small) hipLaunchKernelGGL(k_mp_chain16, dim3(grid_of(b.n_small, 16)), dim3(256), 0, st, ca);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  return MSGPU_OK;
}

// rule 6: the walk back through every kept group, the chains per group and their count
int mp_walk(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx *c = R.c;
  hipStream_t   st = c->stream;
  STAGE_HIP(c, R.clock.begin(&R.res->stats.backtrack_ms));
  STAGE_HIP(c, stage_rocprim(B, [&](void *tmp, size_t &bytes) {
    return rocprim::segmented_radix_sort_keys_desc(tmp, bytes, b.d_sk[0], b.d_sk[1], b.A, b.n_kept, b.d_sb, b.d_se, 0, 64, st);
  }));
  hipLaunchKernelGGL(k_mp_walk, dim3(grid_of(b.n_kept, 64)), dim3(64), 0, st, b.d_lk, b.n_kept, b.d_gstart, b.d_gcnt, b.d_xys, b.d_f, b.d_pred, b.d_sk[1],
                     b.d_used, R.prm.k, R.prm.min_score, R.prm.min_count, b.d_raw, b.d_emit, mp_slot(c, MP_SC_DROP_SCORE),
                     mp_slot(c, MP_SC_DROP_COUNT), mp_slot(c, MP_SC_CUT));
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(B, st, b.d_emit, b.d_coff, b.n_kept, c->sc, MP_SC_TOTAL));
  STAGE_HIP(c, R.clock.end());
  const int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  b.C_n = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]);
  return MSGPU_OK;
}

// the chain table
int mp_table(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx  *c = R.c;
  hipStream_t    st = c->stream;
  const uint32_t C_n = b.C_n;
  STAGE_HIP(c, B.get(&b.d_chains, C_n));
  STAGE_HIP(c, B.get(&b.d_where, C_n));
  STAGE_HIP(c, B.get(&b.d_np, C_n + 1ull));
  STAGE_HIP(c, B.get(&b.d_poff, C_n + 1ull));
  STAGE_HIP(c, hipMemsetAsync(b.d_np + C_n, 0, 4, st));
  STAGE_HIP(c, R.clock.begin(&R.res->stats.backtrack_ms));
  hipLaunchKernelGGL(k_mp_table, dim3(grid256(b.n_kept)), dim3(256), 0, st, b.d_lk, b.n_kept, b.d_gstart, b.d_ug, b.d_xys, b.d_raw, b.d_emit, b.d_coff,
                     R.Qf.recs.len, R.prm.k, b.d_chains, b.d_where, b.d_np, C_n);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  return MSGPU_OK;
}

// rule 12, directly behind the table: query, score and the query range are final here, and no extension has moved them
int mp_rank_batch(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx  *c = R.c;
  const uint64_t before = R.res->chains.size();
  if (before + b.C_n >= (1ull << 32)) {
    snprintf(c->err, sizeof(c->err), "%llu chains; with ranking on the limit of a run is 2^32 - 1 (rule 12)", static_cast<kf_ull>(before + b.C_n));
    return MSGPU_E_ARG;
  }
  uint64_t bad;
  STAGE_HIP(c, B.get(&b.d_rows, b.C_n));
  return mp_rank(c, B, R.clock, b.d_chains, b.C_n, static_cast<uint32_t>(before), false, b.d_rows, b.h_rk, R.res->rstats, &bad);
}

// rule 13, the last device step of a batch: behind the extension, whose end cells move the target ranges it reads.  (An end
// cell that the host would refuse ends the run with MSGPU_E_STATE in mp_extend_apply, so the rows of such a run reach nobody.)
int mp_mates_batch(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx  *c = R.c;
  const uint64_t before = R.res->chains.size();
  if (before + b.C_n >= (1ull << 32)) {
    snprintf(c->err, sizeof(c->err), "%llu chains; with mates on the limit of a run is 2^32 - 1 (rule 13)", static_cast<kf_ull>(before + b.C_n));
    return MSGPU_E_ARG;
  }
  uint64_t bad;
  STAGE_HIP(c, B.get(&b.d_mrows, b.C_n));
  return mp_mates(c, B, R.clock, b.d_chains, R.extend ? b.xb.d_ends : nullptr, b.C_n, static_cast<uint32_t>(before), R.max_insert, false, b.d_mrows,
                  b.h_mt, &R.res->mstats.mate_ms, &b.n_mseg, &bad);
}

// rule 7 in exact mode: the pairs of the batch (b.P; none: nothing more), their distances, and without cigar mode NM
int mp_pairs(const MpRun &R, DevArena &B, msgpu_map_batch &bt, MpBatch &b) {
  msgpu_mapctx    *c = R.c;
  msgpu_map_stats &S = R.res->stats;
  hipStream_t      st = c->stream;
  const bool       cigar = R.prm.cigar != 0;
  const uint32_t   C_n = b.C_n, band = static_cast<uint32_t>(R.prm.band);
  STAGE_HIP(c, stage_scan_total(B, st, b.d_np, b.d_poff, C_n, c->sc, MP_SC_TOTAL));
  int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint32_t P = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]); // (fewer than the anchors)
  b.P        = P;
  bt.n_pairs = P;
  S.n_pairs += P;
  if (!P) return MSGPU_OK;
  const uint64_t NB = bt.n_query_bases, b0 = R.bpre[bt.first_query];
  uint32_t      *d_nm = nullptr;
  rc = mp_oriented(R, B, bt, &S.pairs_ms, b.O); // (the gather opens the span of the pairs)
  if (rc != MSGPU_OK) return rc;
  STAGE_HIP(c, B.get(&b.d_pairs, P));
  STAGE_HIP(c, B.get(&b.d_dist, P));
  if (!cigar) STAGE_HIP(c, B.get(&d_nm, C_n));
  if (cigar) {
    STAGE_HIP(c, B.get(&b.d_trail, P));
    STAGE_HIP(c, B.get(&b.d_head, C_n));
  }
  hipLaunchKernelGGL(k_mp_pairs, dim3(grid256(C_n)), dim3(256), 0, st, b.d_chains, b.d_where, C_n, b.d_xys, b.d_pred, b.d_poff, R.Tf.recs.off, R.d_bpre,
                     b0, NB, R.prm.k, b.d_pairs, P, b.d_trail, b.d_head);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  STAGE_HIP(c, R.clock.begin(&S.distance_ms));
  launch_edit_distance_pairs(st, R.Tf.recs.bases, b.O.d, b.d_pairs, P, band, b.d_dist, false);
  STAGE_HIP(c, hipGetLastError());
  if (!cigar)
    STAGE_HIP(c, stage_rocprim(B, [&](void *tmp, size_t &bytes) {
      return rocprim::segmented_reduce(tmp, bytes, b.d_dist, d_nm, C_n, b.d_poff, b.d_poff + 1, rocprim::plus<uint32_t>(), 0u, st);
    }));
  hipLaunchKernelGGL(k_mp_capped, dim3(grid256(P)), dim3(256), 0, st, b.d_dist, P, band, mp_slot(c, MP_SC_CAPPED));
  if (!cigar) hipLaunchKernelGGL(k_mp_exact, dim3(grid256(C_n)), dim3(256), 0, st, b.d_chains, C_n, d_nm);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  return MSGPU_OK;
}

// rule 10: the scripts' offsets, the scripts, the figures of the pairs and of the chains; what the host needs for the runs comes
// back here, behind a synchronisation of its own
int mp_scripts(const MpRun &R, DevArena &B, MpBatch &b) {
  msgpu_mapctx     *c = R.c;
  msgpu_map_result &res = *R.res;
  msgpu_map_astats &AS = res.astats;
  hipStream_t       st = c->stream;
  const uint32_t    C_n = b.C_n, P = b.P, band = static_cast<uint32_t>(R.prm.band), slots = edit_script_slots();
  uint32_t         *d_len, *d_list, *d_cnt, *d_words, *d_eq, *d_cols;
  const uint64_t    slab_words = edit_script_slab_words(slots, band); // (none for a band within the LDS class)
  uint64_t         *d_off;
  kf_ull           *d_xid;
  STAGE_HIP(c, B.get(&d_len, P + 1ull));
  STAGE_HIP(c, B.get(&d_off, P + 1ull));
  STAGE_HIP(c, B.get(&d_list, P));
  STAGE_HIP(c, B.get(&d_cnt, ES_CNT_COUNT));
  STAGE_HIP(c, B.get_zeroed(&d_xid, 4, st));
  if (slab_words) STAGE_HIP(c, B.get(&b.d_slab, slab_words));
  STAGE_HIP(c, B.get(&d_eq, P));
  STAGE_HIP(c, B.get(&d_cols, P));
  STAGE_HIP(c, R.clock.begin(&AS.align_ms));
  launch_edit_script_lengths(st, b.d_dist, P, band, d_len);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(B, st, d_len, d_off, P, c->sc, MP_SC_TOTAL2));
  STAGE_HIP(c, R.clock.end());
  const int rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint64_t Wn = b.Wn = c->sc.h[MP_SC_TOTAL2]; // (at most P * (band + 1))
  STAGE_HIP(c, B.get(&d_words, Wn));
  STAGE_HIP(c, R.clock.begin(&AS.align_ms));
  STAGE_HIP(c, launch_edit_script_pairs(st, R.Tf.recs.bases, b.O.d, b.d_pairs, P, band, b.d_dist, d_off, d_list, d_cnt, b.d_slab, slots, d_words));
  hipLaunchKernelGGL(k_mp_columns, dim3(grid256(P)), dim3(256), 0, st, b.d_pairs, b.d_dist, d_off, d_words, P, band, d_eq, d_cols, d_xid);
  STAGE_HIP(c, hipGetLastError());
  uint32_t *d_seq, *d_scols; // the sums per chain
  STAGE_HIP(c, B.get(&d_seq, C_n));
  STAGE_HIP(c, B.get(&d_scols, C_n));
  STAGE_HIP(c, stage_rocprim(B, [&](void *tmp, size_t &bytes) {
    return rocprim::segmented_reduce(tmp, bytes, d_eq, d_seq, C_n, b.d_poff, b.d_poff + 1, rocprim::plus<uint32_t>(), 0u, st);
  }));
  STAGE_HIP(c, stage_rocprim(B, [&](void *tmp, size_t &bytes) {
    return rocprim::segmented_reduce(tmp, bytes, d_cols, d_scols, C_n, b.d_poff, b.d_poff + 1, rocprim::plus<uint32_t>(), 0u, st);
  }));
  hipLaunchKernelGGL(k_mp_cigar, dim3(grid256(C_n)), dim3(256), 0, st, b.d_chains, C_n, d_seq, d_scols);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, R.clock.end());
  // ---- what the host needs for the runs comes back with the chain table
  const size_t                  c0 = res.c_head.size(), p0 = res.p_lt.size(), w0 = res.words.size();
  std::vector<msgpu_align_pair> h_pairs;
  std::vector<uint32_t>         h_poff;
  std::vector<uint64_t>         h_off;
  uint32_t                      h_cnt[ES_CNT_COUNT];
  kf_ull                        h_xid[4];
  try {
    h_pairs.resize(P);
    h_poff.resize(C_n + 1ull);
    h_off.resize(P + 1ull);
    res.c_head.resize(c0 + C_n);
    res.p_trail.resize(p0 + P);
    res.p_lt.resize(p0 + P);
    res.p_lq.resize(p0 + P);
    res.words.resize(w0 + Wn);
    res.c_poff.resize(c0 + C_n + 1);
    res.p_woff.resize(p0 + P + 1);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, R.clock.begin(&res.stats.copy_ms));
  STAGE_HIP(c, hipMemcpyAsync(h_pairs.data(), b.d_pairs, P * sizeof(msgpu_align_pair), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(h_poff.data(), b.d_poff, (C_n + 1ull) * 4, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(h_off.data(), d_off, (P + 1ull) * 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(res.c_head.data() + c0, b.d_head, C_n * 4ull, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(res.p_trail.data() + p0, b.d_trail, P * 4ull, hipMemcpyDeviceToHost, st));
  if (Wn) STAGE_HIP(c, hipMemcpyAsync(res.words.data() + w0, d_words, Wn * 4, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(h_xid, d_xid, sizeof(h_xid), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, R.clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  for (uint32_t i = 0; i < P; ++i) {
    res.p_lt[p0 + i]       = h_pairs[i].a_len;
    res.p_lq[p0 + i]       = h_pairs[i].b_len;
    res.p_woff[p0 + i + 1] = w0 + h_off[i + 1];
  }
  for (uint32_t i = 0; i < C_n; ++i) res.c_poff[c0 + i + 1] = p0 + h_poff[i + 1];
  AS.n_pairs_d0 += h_cnt[ES_CNT_D0];
  AS.n_pairs_lds += h_cnt[ES_CNT_LDS];
  AS.n_pairs_slab += h_cnt[ES_CNT_SLAB];
  AS.n_pairs_capped += h_cnt[ES_CNT_CAPPED];
  AS.n_inconsistent += h_cnt[ES_CNT_BROKEN];
  AS.max_d = std::max<uint64_t>(AS.max_d, h_cnt[ES_CNT_MAXD]);
  AS.x_columns += h_xid[0];
  AS.d_columns += h_xid[1];
  AS.i_columns += h_xid[2];
  AS.script_words += Wn;
  return MSGPU_OK;
}

// the batch's chain table (and rule 12's rows) behind those of the batches before it
int mp_tables_back(const MpRun &R, MpBatch &b) {
  msgpu_mapctx     *c = R.c;
  msgpu_map_result &res = *R.res;
  hipStream_t       st = c->stream;
  const size_t      have = res.chains.size();
  try {
    res.chains.resize(have + b.C_n);
    if (R.ranking) res.ranks.resize(have + b.C_n);
    if (R.mates) res.mates.resize(have + b.C_n);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, R.clock.begin(&res.stats.copy_ms));
  STAGE_HIP(c, hipMemcpyAsync(res.chains.data() + have, b.d_chains, b.C_n * sizeof(msgpu_map_chain), hipMemcpyDeviceToHost, st));
  if (R.ranking) STAGE_HIP(c, hipMemcpyAsync(res.ranks.data() + have, b.d_rows, b.C_n * sizeof(msgpu_map_rank), hipMemcpyDeviceToHost, st));
  if (R.mates) STAGE_HIP(c, hipMemcpyAsync(res.mates.data() + have, b.d_mrows, b.C_n * sizeof(msgpu_map_mate), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, R.clock.end());
  return MSGPU_OK;
}

// the host work behind the batch's last synchronisation
int mp_batch_host(const MpRun &R, const MpBatch &b) {
  msgpu_map_result &res = *R.res;
  if (R.prm.cigar && res.c_head.size() < res.chains.size()) { // a batch without a segment pair: a chain is its seed columns
    try {
      for (size_t i = res.c_head.size(); i < res.chains.size(); ++i) {
        res.c_head.push_back(res.chains[i].matches);
        res.c_poff.push_back(res.p_lt.size());
      }
    } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  }
  if (R.ranking && b.C_n) mp_rank_counts(b.h_rk, res.rstats);
  if (R.mates && b.C_n) mp_mate_counts(b.h_mt, b.n_mseg, res.mstats);
  return R.extend && b.C_n ? mp_extend_apply(R, b.C_n, b.xb) : MSGPU_OK;
}

int mp_batch(const MpRun &R, DevArena &B, msgpu_map_batch &bt) {
  msgpu_mapctx *c = R.c;
  const bool    exact = R.prm.exact != 0, cigar = R.prm.cigar != 0;
  MpBatch       b;
  int           rc;
  b.A = static_cast<uint32_t>(bt.n_anchors);
  STAGE_HIP(c, B.rewind());
  if (!b.A) return MSGPU_OK;
  if ((rc = mp_expand(R, B, bt, b)) != MSGPU_OK) return rc;
  if ((rc = mp_classes(R, B, b)) != MSGPU_OK) return rc;
  if ((rc = mp_chain(R, B, b)) != MSGPU_OK) return rc;
  if (b.n_kept && (rc = mp_walk(R, B, b)) != MSGPU_OK) return rc;
  bt.n_chains = b.C_n;
  R.res->stats.n_chains += b.C_n;
  if (b.C_n) {
    if ((rc = mp_table(R, B, b)) != MSGPU_OK) return rc;
    if (R.ranking && (rc = mp_rank_batch(R, B, b)) != MSGPU_OK) return rc;
    if (exact && (rc = mp_pairs(R, B, bt, b)) != MSGPU_OK) return rc;
    if (exact && cigar && b.P && (rc = mp_scripts(R, B, b)) != MSGPU_OK) return rc;
    // rule 11: the ends of every chain, behind the scripts (the slab is theirs first)
    if (R.extend && (rc = mp_extend(R, B, bt, b.d_chains, b.C_n, b.O, b.d_slab, b.xb)) != MSGPU_OK) return rc;
    if (R.mates && (rc = mp_mates_batch(R, B, b)) != MSGPU_OK) return rc;
    if ((rc = mp_tables_back(R, b)) != MSGPU_OK) return rc;
  }
  STAGE_HIP(c, hipStreamSynchronize(c->stream));
  if ((rc = mp_batch_host(R, b)) != MSGPU_OK) return rc;
  R.clock.collect();
  bt.bytes_peak = B.peak;
  return stage_verify(c, B);
}

} // namespace

// Everything of a run that depends on the targets, k and w only: the target file in its store, the per-record offsets and
// lengths, the target sketch, and the index over it (sorted entries, distinct keys, counts, starts, hash table).  The
// occurrence cap is applied at look-up, so max_occ is no part of it.
struct msgpu_map_index {
  msgpu_mapctx *owner = nullptr;
  int           kind = 1; // the store of owner->seq that holds the targets; a run's queries go into the other one
  int           k = 0, w = 0;
  DevArena      D;
  StageFile     Tf;
  MpSketch      Ts;
  uint64_t     *d_ivals = nullptr, *d_ukeys = nullptr;
  uint32_t     *d_ucnt = nullptr, *d_ustart = nullptr, *d_slots = nullptr;
  uint32_t      n_keys = 0, slots_n = 0;
  float         load_ms = 0.f, sketch_ms = 0.f, sort_ms = 0.f, table_ms = 0.f, wall_ms = 0.f;
  ~msgpu_map_index() { // (on the owner's device, behind its stream; nobody takes an error here: one line)
    char err[256];
    if (D.verify(nullptr, err, sizeof(err)) != hipSuccess) fprintf(stderr, "msgpu_map_index_free: %s\n", err);
  }
};

msgpu_mapctx::~msgpu_mapctx() { delete index; }

namespace {

int mp_index_build(msgpu_mapctx *c, int k, int w, const char *tpath, msgpu_map_index &I) {
  hipStream_t      st = c->stream;
  DevArena        &D = I.D;
  StageClock       clock(st);
  const StageTimer wall;
  I.k = k;
  I.w = w;
  int rc = stage_load(c, D, tpath, I.kind, "targets", I.Tf);
  if (rc != MSGPU_OK) return rc;
  I.load_ms = wall.ms();

  // ---- rule 2 on the targets, rule 3
  MpSketch &Ts = I.Ts;
  rc = mp_sketch(c, D, clock, &I.sketch_ms, I.Tf.recs, k, w, "targets", Ts);
  if (rc != MSGPU_OK) return rc;
  const uint32_t NT = static_cast<uint32_t>(Ts.n);
  uint64_t      *d_ikeys;
  uint32_t      *d_nruns;
  STAGE_HIP(c, D.get(&d_ikeys, NT));
  STAGE_HIP(c, D.get(&I.d_ivals, NT));
  STAGE_HIP(c, D.get(&I.d_ukeys, NT));
  STAGE_HIP(c, D.get(&I.d_ucnt, NT + 1ull));
  STAGE_HIP(c, D.get(&I.d_ustart, NT + 1ull));
  STAGE_HIP(c, D.get(&d_nruns, 1));
  STAGE_HIP(c, hipMemsetAsync(d_nruns, 0, 4, st));
  uint32_t n_keys = 0;
  if (NT) {
    STAGE_HIP(c, clock.begin(&I.sort_ms));
    STAGE_HIP(c, stage_sort_pairs(D, st, Ts.keys, d_ikeys, Ts.vals, I.d_ivals, NT, 2 * k));
    STAGE_HIP(c, stage_rocprim(D, [&](void *tmp, size_t &bytes) {
      return rocprim::run_length_encode(tmp, bytes, d_ikeys, NT, I.d_ukeys, I.d_ucnt, d_nruns, st);
    }));
    hipLaunchKernelGGL(k_stage_put<uint32_t>, dim3(1), dim3(64), 0, st, c->sc.d, MP_SC_TOTAL, d_nruns);
    STAGE_HIP(c, clock.end());
    rc = c->sc.read(c);
    if (rc != MSGPU_OK) return rc;
    n_keys = static_cast<uint32_t>(c->sc.h[MP_SC_TOTAL]);
    D.drop_tmp();
    STAGE_HIP(c, hipMemsetAsync(I.d_ucnt + n_keys, 0, 4, st));
    STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, I.d_ucnt, I.d_ustart, n_keys + 1ull));
    STAGE_HIP(c, hipStreamSynchronize(st));
    D.drop_tmp();
  }
  D.drop(d_ikeys); // (the distinct keys stand for them from here on)
  D.drop(d_nruns);
  if (n_keys > (1u << 30)) { // (the table has 2^31 slots at most)
    snprintf(c->err, sizeof(c->err), "%u distinct target minimizers; the limit is 2^30", n_keys);
    return MSGPU_E_ARG;
  }
  uint32_t sn = 64;
  while (sn < 2ull * n_keys) sn <<= 1;
  STAGE_HIP(c, D.get(&I.d_slots, sn));
  STAGE_HIP(c, hipMemsetAsync(I.d_slots, 0xff, sn * 4ull, st));
  STAGE_HIP(c, clock.begin(&I.table_ms));
  if (n_keys) hipLaunchKernelGGL(k_kf_table<uint64_t>, dim3(grid256(n_keys)), dim3(256), 0, st, I.d_ukeys, n_keys, I.d_slots, sn - 1);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  clock.collect();
  I.n_keys  = n_keys;
  I.slots_n = sn;
  I.wall_ms = wall.ms();
  return stage_verify(c, D);
}

// a run on an index: the query side, rule 3's cap at this run's max_occ, rules 4 to 9
int mp_run(msgpu_mapctx *c, const msgpu_map_params &prm, const msgpu_map_index &I, const char *qpath, uint64_t budget_bytes,
           msgpu_map_result *res) {
  msgpu_map_stats &S = res->stats;
  hipStream_t      st = c->stream;
  DevArena         D; // the run's own: the index is read, never written
  StageClock       clock(st);
  const int  k = prm.k, w = prm.w;
  const bool ava = prm.ava != 0, exact = prm.exact != 0;
  const StageTimer wall;
  STAGE_HIP(c, hipMemsetAsync(c->sc.d, 0, SC_COUNT * sizeof(uint64_t), st));

  // ---- the query file (ava: the index's own store and sketch)
  const StageFile &Tf = I.Tf;
  StageFile     Qf_own;
  int           rc;
  if (!ava) {
    rc = stage_load(c, D, qpath, 1 - I.kind, "queries", Qf_own);
    if (rc != MSGPU_OK) return rc;
  }
  const StageFile &Qf = ava ? Tf : Qf_own;
  const int     qkind = ava ? I.kind : 1 - I.kind;
  S.n_records[0] = Tf.recs.n;
  S.n_records[1] = Qf.recs.n;
  S.n_bases[0]   = Tf.recs.n_bases;
  S.n_bases[1]   = Qf.recs.n_bases;
  S.load_ms      = ava ? 0.f : wall.ms();
  if (c->mates && (Qf.recs.n & 1u)) {
    snprintf(c->err, sizeof(c->err), "%u query records; with mates on the file is interleaved and holds an even number (rule 13)", Qf.recs.n);
    return MSGPU_E_ARG;
  }

  // ---- rule 2 on the queries, rule 3's cap
  const MpSketch &Ts = I.Ts;
  MpSketch        Qs_own;
  if (!ava) {
    rc = mp_sketch(c, D, clock, &S.sketch_ms, Qf.recs, k, w, "queries", Qs_own);
    if (rc != MSGPU_OK) return rc;
  }
  const MpSketch &Qs = ava ? Ts : Qs_own;
  S.n_minimizers[0]  = Ts.n;
  S.n_minimizers[1]  = Qs.n;
  const uint32_t NT = static_cast<uint32_t>(Ts.n), n_keys = I.n_keys;
  uint32_t      *d_nruns;
  STAGE_HIP(c, D.get(&d_nruns, 1));
  STAGE_HIP(c, hipMemsetAsync(d_nruns, 0, 4, st));
  STAGE_HIP(c, clock.begin(&S.table_ms));
  if (n_keys)
    hipLaunchKernelGGL(k_mp_occ, dim3(grid256(n_keys)), dim3(256), 0, st, I.d_ucnt, n_keys, prm.max_occ, mp_slot(c, MP_SC_DROPK),
                       mp_slot(c, MP_SC_DROPE));
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  S.n_keys          = n_keys;
  S.n_index_entries = NT;
  const MpIndex X{I.d_ukeys, I.d_ucnt, I.d_ustart, I.d_slots, I.slots_n - 1, prm.max_occ, I.d_ivals};

  // ---- rule 4's counts: anchors per query minimizer and in front of it; anchors and bases in front of every query record
  const uint64_t NQ = Qs.n;
  const uint32_t NR = Qf.recs.n;
  uint32_t      *d_acnt;
  uint64_t      *d_aoff, *d_pre; // d_pre: NR + 1 words each of anchors in front, bases in front, first minimizer
  kf_ull        *d_hist;
  STAGE_HIP(c, D.get(&d_acnt, NQ + 1));
  STAGE_HIP(c, D.get(&d_aoff, NQ + 1));
  STAGE_HIP(c, D.get(&d_pre, 3 * (NR + 1ull)));
  STAGE_HIP(c, D.get_zeroed(&d_hist, 32, st));
  STAGE_HIP(c, hipMemsetAsync(d_acnt + NQ, 0, 4, st));
  STAGE_HIP(c, clock.begin(&S.anchors_ms));
  if (NQ)
    hipLaunchKernelGGL((k_mp_anchors<false>), dim3(grid256(NQ)), dim3(256), 0, st, X, Qs.keys, Qs.vals, 0, NQ, Qf.recs.len, k, prm.ava, d_acnt,
                       nullptr, nullptr, nullptr, 0);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_acnt, d_aoff, NQ + 1));
  hipLaunchKernelGGL(k_mp_prefix, dim3(grid256(NR + 1ull)), dim3(256), 0, st, Qs.vals, NQ, d_aoff, NR, d_pre + 2 * (NR + 1ull), d_pre);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, Qf.recs.len, d_pre + (NR + 1ull), NR + 1ull)); // (stage_load: a zero behind the lengths)
  STAGE_HIP(c, clock.end());
  std::vector<uint64_t> pre;
  try {
    pre.resize(3 * (NR + 1ull));
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, hipMemcpyAsync(pre.data(), d_pre, pre.size() * 8, hipMemcpyDeviceToHost, st));
  rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  STAGE_HIP(c, hipStreamSynchronize(st));
  D.drop_tmp();
  S.n_keys_dropped    = c->sc.h[MP_SC_DROPK];
  S.n_entries_dropped = c->sc.h[MP_SC_DROPE];
  const uint64_t *apre = pre.data(), *bpre = apre + (NR + 1ull), *first_min = bpre + (NR + 1ull);
  S.n_anchors = apre[NR];

  // ---- rule 9: the budget, the cut, one reservation for the largest batch
  uint64_t budget = budget_bytes;
  if (!budget) {
    size_t free_b = 0, total_b = 0;
    STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
    budget = free_b;
  }
  DevArena B;
  for (;;) {
    res->budget = budget;
    res->batches.clear();
    const uint32_t bad = mp_cut(prm, c->extend, c->ranking, c->mates, apre, bpre, NR, budget, res->batches);
    if (bad < NR && c->mates) { // rule 13.7: the unit is the pair
      const uint64_t a = apre[bad + 2] - apre[bad], b = bpre[bad + 2] - bpre[bad];
      if (a >= (1ull << 31)) {
        snprintf(c->err, sizeof(c->err), "pair %u (query records %u and %u) has %llu anchors; the limit of a batch is 2^31 - 1 (rule 13: a pair is "
                 "not split)", bad / 2, bad, bad + 1, static_cast<kf_ull>(a));
        return MSGPU_E_ARG;
      }
      snprintf(c->err, sizeof(c->err), "pair %u (query records %u and %u) with %llu anchors and %llu bases needs %llu bytes on its own; the budget "
               "of a batch is %llu bytes (rule 13: a pair is not split)", bad / 2, bad, bad + 1, static_cast<kf_ull>(a), static_cast<kf_ull>(b),
               static_cast<kf_ull>(mp_batch_bytes(prm, c->extend, c->ranking, a, b, 1)), static_cast<kf_ull>(budget));
      return MSGPU_E_NOMEM;
    }
    if (bad < NR) {
      const uint64_t a = apre[bad + 1] - apre[bad], b = bpre[bad + 1] - bpre[bad];
      if (a >= (1ull << 31)) {
        snprintf(c->err, sizeof(c->err), "query record %u has %llu anchors; the limit of a batch is 2^31 - 1 (rule 9: a record is not split)",
                 bad, static_cast<kf_ull>(a));
        return MSGPU_E_ARG;
      }
      snprintf(c->err, sizeof(c->err), "query record %u with %llu anchors and %llu bases needs %llu bytes on its own (%llu of them for its "
               "oriented copies); the budget of a batch is %llu bytes (rule 9: a record is not split)", bad, static_cast<kf_ull>(a),
               static_cast<kf_ull>(b), static_cast<kf_ull>(mp_batch_bytes(prm, c->extend, c->ranking, a, b)), static_cast<kf_ull>(exact ? 2 * b : 0),
               static_cast<kf_ull>(budget));
      return MSGPU_E_NOMEM;
    }
    uint64_t reserve = 0;
    for (const msgpu_map_batch &b : res->batches)
      if (b.n_anchors) reserve = std::max(reserve, b.bytes_bound);
    const hipError_t e = reserve ? B.reserve(reserve) : hipSuccess;
    if (e == hipErrorOutOfMemory && !budget_bytes && budget > MP_BYTES_FIXED) {
      // the free memory is not one block's: the budget that 0 stands for shrinks by an eighth until the reservation succeeds
      (void)hipGetLastError();
      budget -= budget / 8;
      continue;
    }
    STAGE_HIP(c, e);
    break;
  }

  // ---- rules 4 to 8, batch by batch
  const MpRun run{c, prm, Tf, Qf, Qs, X, d_aoff, d_pre + (NR + 1ull), first_min, bpre, qkind, d_nruns, d_hist, clock, res, c->extend, c->ranking, c->mates, c->max_insert};
  res->xstats.extend = c->extend;
  res->rstats.ranking = c->ranking;
  res->rstats.lds_primaries = MSGPU_MAP_RANK_LDS;
  res->mstats.mates = c->mates;
  res->mstats.max_insert = c->mates ? c->max_insert : 0;
  for (msgpu_map_batch &b : res->batches) {
    rc = mp_batch(run, B, b);
    if (rc != MSGPU_OK) return rc;
  }
  if (c->mates) { // the pairs without a chain never reached a table
    res->mstats.n_unmapped = NR / 2 - res->mstats.n_pairs;
    res->mstats.n_pairs    = NR / 2;
  }
  rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  S.n_chains_below_score = c->sc.h[MP_SC_DROP_SCORE];
  S.n_chains_below_count = c->sc.h[MP_SC_DROP_COUNT];
  S.n_chains_cut         = c->sc.h[MP_SC_CUT];
  S.n_pairs_capped       = c->sc.h[MP_SC_CAPPED];
  const uint64_t C_n     = res->chains.size();

  // ---- the figures come back; the host formats the lines
  kf_ull hist[32];
  STAGE_HIP(c, hipMemcpyAsync(hist, d_hist, sizeof(hist), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));
  clock.collect();
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;
  for (int i = 0; i < 32; ++i) S.group_hist[i < 15 ? i : 15] += hist[i];
  const StageTimer formatting;
  try {
    unsigned nt = std::thread::hardware_concurrency();
    nt          = nt == 0 ? 1 : (nt > 16 ? 16 : nt);
    if (C_n < 4096) nt = 1;
    const bool cigar = prm.cigar != 0;
    std::vector<std::string>           part(nt);
    std::vector<std::vector<uint32_t>> part_ops(nt), part_cnt(nt); // cigar mode: the packed runs of a range, and how many per chain
    std::vector<float>                 part_ms(nt, 0.f);
    msgpu::HostPool::get().run(nt, nt, [&](size_t t) {
      const uint64_t a = static_cast<uint64_t>(C_n) * t / nt, b = static_cast<uint64_t>(C_n) * (t + 1) / nt;
      part[t].reserve((b - a) * 112);
      std::vector<std::pair<uint32_t, uint64_t>> runs;
      for (uint64_t i = a; i < b; ++i) {
        const msgpu_map_rank *rk = res->ranks.empty() ? nullptr : &res->ranks[i];
        const bool            prim = rk && rk->parent == i;
        const msgpu_map_mate *mt = c->mates ? &res->mates[i] : nullptr;
        if (!cigar) {
          mp_format(res->chains[i], Tf.f, Qf.f, exact, part[t], nullptr, rk, prim, mt);
          continue;
        }
        const StageTimer merging;
        mp_runs(*res, i, runs);
        uint32_t n_packed = 0;
        for (const auto &r : runs) // (a run of 2^28 columns or more takes several entries of the table: 28 bits of length)
          for (uint64_t left = r.second; left; ++n_packed) {
            const uint64_t piece = std::min<uint64_t>(left, (1ull << 28) - 1);
            part_ops[t].push_back(static_cast<uint32_t>(piece << 4) | r.first);
            left -= piece;
          }
        part_cnt[t].push_back(n_packed);
        part_ms[t] += merging.ms();
        mp_format(res->chains[i], Tf.f, Qf.f, exact, part[t], &runs, rk, prim, mt);
      }
    });
    size_t total = 0;
    for (const std::string &p : part) total += p.size();
    res->text.reserve(total);
    for (const std::string &p : part) res->text += p;
    if (cigar) {
      for (unsigned t = 0; t < nt; ++t) {
        res->cg_ops.insert(res->cg_ops.end(), part_ops[t].begin(), part_ops[t].end());
        for (uint32_t n : part_cnt[t]) res->cg_off.push_back(res->cg_off.back() + n);
        res->astats.cigar_host_ms += part_ms[t];
      }
      res->astats.n_runs     = res->cg_ops.size();
      res->astats.slots      = edit_script_slots();
      res->astats.lds_max_d  = edit_script_lds_max_d();
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  S.host_ms   = formatting.ms();
  S.bytes_out = res->text.size();
  S.wall_ms   = wall.ms();
  return MSGPU_OK;
}

} // namespace

extern "C" {

void msgpu_map_default_params(msgpu_map_params *p) {
  if (!p) return;
  *p = msgpu_map_params{15, 5, 200, 10000, 2000, 64, 100, 3, 0, 64, 0, 0};
}

uint64_t msgpu_map_batch_bytes(const msgpu_map_params *p, uint64_t n_anchors, uint64_t n_query_bases) {
  msgpu_map_params prm{};
  if (p) prm = *p;
  return mp_batch_bytes(prm, 0, 0, n_anchors, n_query_bases);
}

uint64_t msgpu_map_batch_bytes_ext(const msgpu_map_params *p, uint32_t extend, uint64_t n_anchors, uint64_t n_query_bases) {
  msgpu_map_params prm{};
  if (p) prm = *p;
  return mp_batch_bytes(prm, extend, 0, n_anchors, n_query_bases);
}

uint64_t msgpu_map_batch_bytes_rank(const msgpu_map_params *p, uint32_t extend, uint32_t ranking, uint64_t n_anchors, uint64_t n_query_bases) {
  msgpu_map_params prm{};
  if (p) prm = *p;
  return mp_batch_bytes(prm, extend, ranking, n_anchors, n_query_bases);
}

int msgpu_map_set_ranking(msgpu_mapctx *c, int on) {
  if (!c) return MSGPU_E_ARG;
  c->err[0]  = 0;
  c->ranking = on != 0;
  return MSGPU_OK;
}

uint64_t msgpu_map_batch_bytes_mates(const msgpu_map_params *p, uint32_t extend, uint32_t ranking, uint32_t mates, uint64_t n_anchors,
                                     uint64_t n_query_bases) {
  msgpu_map_params prm{};
  if (p) prm = *p;
  return mp_batch_bytes(prm, extend, ranking, n_anchors, n_query_bases, mates);
}

int msgpu_map_set_mates(msgpu_mapctx *c, int on, uint32_t max_insert) {
  if (!c) return MSGPU_E_ARG;
  c->err[0] = 0;
  if (max_insert < 1 || max_insert > 0x7fffffffu) {
    snprintf(c->err, sizeof(c->err), "max_insert = %u; it is 1..2^31 - 1 (rule 13)", max_insert);
    return MSGPU_E_ARG;
  }
  c->mates      = on != 0;
  c->max_insert = max_insert;
  return MSGPU_OK;
}

int msgpu_map_set_extension(msgpu_mapctx *c, uint32_t extend) {
  if (!c) return MSGPU_E_ARG;
  c->err[0] = 0;
  if (extend > MSGPU_MAP_EXTEND_MAX) {
    snprintf(c->err, sizeof(c->err), "extend = %u; the limit is %u (0 switches the extension off)", extend, MSGPU_MAP_EXTEND_MAX);
    return MSGPU_E_ARG;
  }
  c->extend = extend;
  return MSGPU_OK;
}

int  msgpu_map_create(int device, msgpu_mapctx **out) { return stage_create(device, out); }
void msgpu_map_destroy(msgpu_mapctx *c) { stage_destroy(c); }

const char *msgpu_map_last_error(const msgpu_mapctx *c) { return c ? c->err : "null context"; }

static int mp_check_params(msgpu_mapctx *c, const msgpu_map_params &p) {
  if (p.k < 4 || p.k > 32 || p.w < 1 || p.w > 64 || p.max_occ < 1 || p.max_gap < 0 || p.bandwidth < 0 || p.max_pred != 64 ||
      p.band < 1 || p.band > 127 || (p.exact != 0 && p.exact != 1) || (p.ava != 0 && p.ava != 1) || (p.cigar != 0 && p.cigar != 1) ||
      (p.cigar && !p.exact)) {
    snprintf(c->err, sizeof(c->err), "parameters: k = %d (4..32), w = %d (1..64), max_occ = %u (>= 1), max_gap = %d, bandwidth = %d "
             "(>= 0), max_pred = %d (64), band = %d (1..127), exact = %d, ava = %d (0 / 1), cigar = %d (0 / 1; 1 needs exact = 1)", p.k, p.w,
             p.max_occ, p.max_gap, p.bandwidth, p.max_pred, p.band, p.exact, p.ava, p.cigar);
    return MSGPU_E_ARG;
  }
  if (c->mates && p.ava) {
    snprintf(c->err, sizeof(c->err), "parameters: mates needs a query file of pairs; the run has ava = 1 (rule 13)");
    return MSGPU_E_ARG;
  }
  if (c->extend && !p.cigar) {
    snprintf(c->err, sizeof(c->err), "parameters: extend = %u needs cigar = 1 (and so exact = 1); the run has cigar = %d (rule 11)", c->extend,
             p.cigar);
    return MSGPU_E_ARG;
  }
  return MSGPU_OK;
}

// the index of targets_path in store `kind` of the context
static int mp_index_create(msgpu_mapctx *c, int k, int w, const char *targets_path, int kind, msgpu_map_index **out) {
  if (c->index) {
    snprintf(c->err, sizeof(c->err), "the context holds an index already (k = %d, w = %d): free it first", c->index->k, c->index->w);
    return MSGPU_E_STATE;
  }
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_map_index> I;
  try {
    I.reset(new msgpu_map_index());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  I->owner = c;
  I->kind  = kind;
  const int rc = mp_index_build(c, k, w, targets_path, *I);
  if (rc != MSGPU_OK) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  c->index = I.get();
  *out     = I.release();
  return MSGPU_OK;
}

int msgpu_map_index_create(msgpu_mapctx *c, const msgpu_map_params *params, const char *targets_path, msgpu_map_index **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out      = nullptr;
  c->err[0] = 0;
  if (!params || !targets_path) return MSGPU_E_ARG;
  if (params->k < 4 || params->k > 32 || params->w < 1 || params->w > 64) {
    snprintf(c->err, sizeof(c->err), "parameters: k = %d (4..32), w = %d (1..64)", params->k, params->w);
    return MSGPU_E_ARG;
  }
  return mp_index_create(c, params->k, params->w, targets_path, 1, out);
}

void msgpu_map_index_free(msgpu_map_index *index) {
  if (!index) return;
  msgpu_mapctx *c = index->owner;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->index == index) c->index = nullptr;
  delete index;
}

int msgpu_map_index_stats(const msgpu_map_index *index, msgpu_map_istats *out) {
  if (!index || !out) return MSGPU_E_ARG;
  *out = msgpu_map_istats{index->Tf.recs.n, index->Tf.recs.n_bases, index->Ts.n,      index->n_keys,   index->Ts.n,
                               index->k,         index->w,               index->load_ms,   index->sketch_ms, index->sort_ms,
                               index->table_ms,  index->wall_ms,         0};
  return MSGPU_OK;
}

int msgpu_map_run_index(msgpu_mapctx *c, const msgpu_map_params *params, const msgpu_map_index *index, const char *queries_path,
                        uint32_t flags, uint64_t budget_bytes, msgpu_map_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out      = nullptr;
  c->err[0] = 0;
  if (!params || !index || flags) return MSGPU_E_ARG;
  const msgpu_map_params p = *params;
  int                    rc = mp_check_params(c, p);
  if (rc != MSGPU_OK) return rc;
  if (index != c->index) {
    snprintf(c->err, sizeof(c->err), "the index is not this context's");
    return MSGPU_E_ARG;
  }
  if (p.k != index->k || p.w != index->w) {
    snprintf(c->err, sizeof(c->err), "the run has k = %d, w = %d; the index was built with k = %d, w = %d", p.k, p.w, index->k, index->w);
    return MSGPU_E_ARG;
  }
  if (p.ava ? queries_path != nullptr : !queries_path) {
    snprintf(c->err, sizeof(c->err), p.ava ? "ava: the index's own records are the queries" : "no query file");
    return MSGPU_E_ARG;
  }
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_map_result> res;
  try {
    res.reset(new msgpu_map_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  const uint64_t lost0 = c->sc.lost;
  rc = mp_run(c, p, *index, queries_path, budget_bytes, res.get());
  if (rc != MSGPU_OK) {
    (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  res->stats.n_lost_publications = c->sc.lost - lost0;
  res->stats.params              = p;
  *out                           = res.release();
  return MSGPU_OK;
}

// create + run + free
int msgpu_map_run(msgpu_mapctx *c, const msgpu_map_params *params, const char *targets_path, const char *queries_path, uint32_t flags,
                  uint64_t budget_bytes, msgpu_map_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out      = nullptr;
  c->err[0] = 0;
  if (!params || !targets_path || flags) return MSGPU_E_ARG;
  const msgpu_map_params p = *params;
  int                    rc = mp_check_params(c, p);
  if (rc != MSGPU_OK) return rc;
  if (p.ava ? (queries_path && strcmp(queries_path, targets_path) != 0) : !queries_path) {
    snprintf(c->err, sizeof(c->err), p.ava ? "ava: the query file is the target file" : "no query file");
    return MSGPU_E_ARG;
  }
  const StageTimer wall;
  const uint64_t   lost0 = c->sc.lost;
  msgpu_map_index *index = nullptr;
  rc = mp_index_create(c, p.k, p.w, targets_path, p.ava ? 0 : 1, &index); // (the stores the stage has always used)
  if (rc != MSGPU_OK) return rc;
  rc = msgpu_map_run_index(c, &p, index, p.ava ? nullptr : queries_path, 0, budget_bytes, out);
  if (rc == MSGPU_OK) {
    msgpu_map_stats &S = (*out)->stats;
    S.load_ms += index->load_ms;
    S.sketch_ms += index->sketch_ms;
    S.sort_ms += index->sort_ms;
    S.table_ms += index->table_ms;
    S.n_lost_publications = c->sc.lost - lost0;
  }
  msgpu_map_index_free(index);
  if (rc == MSGPU_OK) (*out)->stats.wall_ms = wall.ms();
  return rc;
}

int msgpu_map_result_stats(const msgpu_map_result *r, msgpu_map_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

int msgpu_map_result_chains(const msgpu_map_result *r, const msgpu_map_chain **chains, uint64_t *n) {
  if (!r || !chains || !n) return MSGPU_E_ARG;
  *chains = r->chains.data();
  *n      = r->chains.size();
  return MSGPU_OK;
}

int msgpu_map_result_batches(const msgpu_map_result *r, const msgpu_map_batch **batches, uint64_t *n) {
  if (!r || !batches || !n) return MSGPU_E_ARG;
  *batches = r->batches.data();
  *n       = r->batches.size();
  return MSGPU_OK;
}

uint64_t msgpu_map_result_budget(const msgpu_map_result *r) { return r ? r->budget : 0; }

int msgpu_map_result_cigars(const msgpu_map_result *r, const uint32_t **ops, const uint64_t **off, uint64_t *n) {
  if (!r || !ops || !off || !n) return MSGPU_E_ARG;
  *ops = r->cg_ops.data();
  *off = r->cg_off.data();
  *n   = r->cg_off.size() - 1;
  return MSGPU_OK;
}

int msgpu_map_result_align_stats(const msgpu_map_result *r, msgpu_map_astats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->astats;
  return MSGPU_OK;
}

int msgpu_map_result_ext_stats(const msgpu_map_result *r, msgpu_map_xstats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->xstats;
  return MSGPU_OK;
}

int msgpu_map_result_ext_ends(const msgpu_map_result *r, const msgpu_ext_end **ends, uint64_t *n) {
  if (!r || !ends || !n) return MSGPU_E_ARG;
  *ends = r->x_ends.data();
  *n    = r->x_ends.size();
  return MSGPU_OK;
}

int msgpu_map_result_ranks(const msgpu_map_result *r, const msgpu_map_rank **ranks, uint64_t *n) {
  if (!r || !ranks || !n) return MSGPU_E_ARG;
  *ranks = r->ranks.data();
  *n     = r->ranks.size();
  return MSGPU_OK;
}

int msgpu_map_result_rank_stats(const msgpu_map_result *r, msgpu_map_rstats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->rstats;
  return MSGPU_OK;
}

// rule 12 on a chain table of the host
int msgpu_map_rank_tables(msgpu_mapctx *c, const msgpu_map_chain *chains, uint64_t n, msgpu_map_rank *ranks_out) {
  if (!c) return MSGPU_E_ARG;
  c->err[0]       = 0;
  c->table_rstats = msgpu_map_rstats{};
  c->table_rstats.ranking       = 1;
  c->table_rstats.lds_primaries = MSGPU_MAP_RANK_LDS;
  if (n && (!chains || !ranks_out)) return MSGPU_E_ARG;
  if (n >= (1ull << 32)) {
    snprintf(c->err, sizeof(c->err), "%llu chains; the limit of a table is 2^32 - 1 (rule 12)", static_cast<kf_ull>(n));
    return MSGPU_E_ARG;
  }
  if (!n) return MSGPU_OK;
  STAGE_HIP(c, hipSetDevice(c->device));
  hipStream_t      st = c->stream;
  DevArena         D;
  StageClock       clock(st);
  msgpu_map_chain *d_chains;
  msgpu_map_rank  *d_rows;
  kf_ull           h_cnt[RK_COUNT] = {};
  uint64_t         bad = ~0ull;
  STAGE_HIP(c, D.get(&d_chains, n));
  STAGE_HIP(c, D.get(&d_rows, n));
  STAGE_HIP(c, hipMemcpyAsync(d_chains, chains, n * sizeof(msgpu_map_chain), hipMemcpyHostToDevice, st));
  int rc = mp_rank(c, D, clock, d_chains, static_cast<uint32_t>(n), 0, true, d_rows, h_cnt, c->table_rstats, &bad);
  if (rc == MSGPU_OK) {
    const hipError_t e = hipMemcpyAsync(ranks_out, d_rows, n * sizeof(msgpu_map_rank), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) rc = stage_fail(c, MSGPU_E_HIP, "rows", e);
  }
  const hipError_t e = hipStreamSynchronize(st);
  if (rc == MSGPU_OK && e != hipSuccess) rc = stage_fail(c, MSGPU_E_HIP, "hipStreamSynchronize", e);
  clock.collect();
  if (rc == MSGPU_OK) rc = stage_verify(c, D);
  if (rc == MSGPU_E_ARG && bad != ~0ull && bad < n) {
    c->table_rstats = msgpu_map_rstats{};
    if (chains[bad].q_start > chains[bad].q_end)
      snprintf(c->err, sizeof(c->err), "chain %llu: q_start %u > q_end %u", static_cast<kf_ull>(bad), chains[bad].q_start, chains[bad].q_end);
    else
      snprintf(c->err, sizeof(c->err), "chain %llu: query record %u behind %u (the table is ordered by query record)", static_cast<kf_ull>(bad),
               chains[bad].query, chains[bad - 1].query);
  }
  if (rc == MSGPU_OK) mp_rank_counts(h_cnt, c->table_rstats);
  return rc;
}

int msgpu_map_rank_tables_stats(const msgpu_mapctx *c, msgpu_map_rstats *out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = c->table_rstats;
  return MSGPU_OK;
}

int msgpu_map_result_mates(const msgpu_map_result *r, const msgpu_map_mate **mates, uint64_t *n) {
  if (!r || !mates || !n) return MSGPU_E_ARG;
  *mates = r->mates.data();
  *n     = r->mates.size();
  return MSGPU_OK;
}

int msgpu_map_result_mate_stats(const msgpu_map_result *r, msgpu_map_mstats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->mstats;
  return MSGPU_OK;
}

// rule 13 on a chain table of the host
int msgpu_map_mate_tables(msgpu_mapctx *c, const msgpu_map_chain *chains, uint64_t n, uint32_t max_insert, msgpu_map_mate *rows_out) {
  if (!c) return MSGPU_E_ARG;
  c->err[0]       = 0;
  c->table_mstats = msgpu_map_mstats{};
  if (n && (!chains || !rows_out)) return MSGPU_E_ARG;
  if (max_insert < 1 || max_insert > 0x7fffffffu) {
    snprintf(c->err, sizeof(c->err), "max_insert = %u; it is 1..2^31 - 1 (rule 13)", max_insert);
    return MSGPU_E_ARG;
  }
  if (n >= (1ull << 32)) {
    snprintf(c->err, sizeof(c->err), "%llu chains; the limit of a table is 2^32 - 1 (rule 13)", static_cast<kf_ull>(n));
    return MSGPU_E_ARG;
  }
  c->table_mstats.mates      = 1;
  c->table_mstats.max_insert = max_insert;
  if (!n) return MSGPU_OK;
  STAGE_HIP(c, hipSetDevice(c->device));
  hipStream_t      st = c->stream;
  DevArena         D;
  StageClock       clock(st);
  msgpu_map_chain *d_chains;
  msgpu_map_mate  *d_rows;
  kf_ull           h_cnt[MT_COUNT] = {};
  uint64_t         bad = ~0ull, n_seg = 0;
  STAGE_HIP(c, D.get(&d_chains, n));
  STAGE_HIP(c, D.get(&d_rows, n));
  STAGE_HIP(c, hipMemcpyAsync(d_chains, chains, n * sizeof(msgpu_map_chain), hipMemcpyHostToDevice, st));
  int rc = mp_mates(c, D, clock, d_chains, nullptr, static_cast<uint32_t>(n), 0, max_insert, true, d_rows, h_cnt, &c->table_mstats.mate_ms, &n_seg,
                    &bad);
  if (rc == MSGPU_OK) {
    const hipError_t e = hipMemcpyAsync(rows_out, d_rows, n * sizeof(msgpu_map_mate), hipMemcpyDeviceToHost, st);
    if (e != hipSuccess) rc = stage_fail(c, MSGPU_E_HIP, "rows", e);
  }
  const hipError_t e = hipStreamSynchronize(st);
  if (rc == MSGPU_OK && e != hipSuccess) rc = stage_fail(c, MSGPU_E_HIP, "hipStreamSynchronize", e);
  clock.collect();
  if (rc == MSGPU_OK) rc = stage_verify(c, D);
  if (rc == MSGPU_E_ARG && bad != ~0ull && bad < n) { // the first violated of the three, in 13's order
    const msgpu_map_chain &ch = chains[bad];
    c->table_mstats = msgpu_map_mstats{};
    snprintf(c->err, sizeof(c->err), "chain %llu: %s", static_cast<kf_ull>(bad),
             bad && ch.query < chains[bad - 1].query ? "order" : ch.strand > 1 ? "strand" : "range");
  }
  if (rc == MSGPU_OK) mp_mate_counts(h_cnt, n_seg, c->table_mstats);
  return rc;
}

int msgpu_map_mate_tables_stats(const msgpu_mapctx *c, msgpu_map_mstats *out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = c->table_mstats;
  return MSGPU_OK;
}

const char *msgpu_map_result_text(const msgpu_map_result *r, uint64_t *len) {
  if (len) *len = r ? r->text.size() : 0;
  return r ? r->text.data() : "";
}

void msgpu_map_result_free(msgpu_map_result *r) {
  if (r) delete r;
}

} // extern "C"
