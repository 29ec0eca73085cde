// msgpu_device.h -- device-side helpers shared by the kernel files (msgpu_kernels.hip, msgpu_index.hip): 32-byte and 16-byte row
// loads / stores, readlane of wide types, wavefront and workgroup scans; the stage files' small idioms (wavefront-aggregated
// counters and append, the search of a segment table, k_stage_put, k_stage_seg_starts); and the records of a sequence store
// with their lookup (msgpu_map.hip, msgpu_polish.hip).  gfx950, wave64.
#ifndef MSGPU_DEVICE_H
#define MSGPU_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msgpu.h"
#include "msgpu_internal.h"

namespace msgpu {

__device__ __forceinline__ IRow load_irow(const IRow *p) {
  const uint4 *q = reinterpret_cast<const uint4 *>(p);
  uint4        a = q[0], b = q[1];
  IRow         r;
  r.n_lo  = static_cast<int>(a.x);
  r.n_hi  = static_cast<int>(a.y);
  r.i_lo  = static_cast<int>(a.z);
  r.i_hi  = static_cast<int>(a.w);
  r.score = b.x;
  r.line  = b.y;
  r.other = b.z;
  r.pf    = b.w;
  return r;
}
__device__ __forceinline__ void store_irow(IRow *p, const IRow &r) {
  uint4 *q = reinterpret_cast<uint4 *>(p);
  q[0]     = make_uint4(static_cast<uint32_t>(r.n_lo), static_cast<uint32_t>(r.n_hi), static_cast<uint32_t>(r.i_lo),
                        static_cast<uint32_t>(r.i_hi));
  q[1]     = make_uint4(r.score, r.line, r.other, r.pf);
}

__device__ __forceinline__ IRow make_irow(const msgpu_row &row, uint32_t other, uint32_t rank) {
  IRow out;
  out.n_lo  = row.n_lo;
  out.n_hi  = row.n_hi;
  out.i_lo  = row.i_lo;
  out.i_hi  = row.i_hi;
  out.score = row.score;
  out.line  = row.line;
  out.other = other;
  out.pf    = ((row.flags & MSGPU_ROW_DIR) ? PF_DIR : 0u) | ((row.flags & MSGPU_ROW_PRIMARY) ? PF_PRIM : 0u) |
           (rank & PF_POS_MASK);
  return out;
}

// the 16-byte scaffold row: one vector load, one vector store
__device__ __forceinline__ SRow load_srow(const SRow *p) {
  const uint4 a = *reinterpret_cast<const uint4 *>(p);
  SRow        r;
  r.i_lo = static_cast<int>(a.x);
  r.i_hi = static_cast<int>(a.y);
  r.read = a.z;
  r.pf   = a.w;
  return r;
}
__device__ __forceinline__ void store_srow(SRow *p, const SRow &r) {
  *reinterpret_cast<uint4 *>(p) = make_uint4(static_cast<uint32_t>(r.i_lo), static_cast<uint32_t>(r.i_hi), r.read, r.pf);
}
// the scaffold row of a by_read row: same interval and flags, the read in place of the anchor, the rank in the read attached
__device__ __forceinline__ SRow make_srow(const IRow &row, uint32_t read, uint32_t rank) {
  SRow out;
  out.i_lo = row.i_lo;
  out.i_hi = row.i_hi;
  out.read = read;
  out.pf   = (row.pf & ~PF_POS_MASK) | (rank & PF_POS_MASK);
  return out;
}
__device__ __forceinline__ SRow make_srow(const msgpu_row &row, uint32_t read, uint32_t rank) {
  SRow out;
  out.i_lo = row.i_lo;
  out.i_hi = row.i_hi;
  out.read = read;
  out.pf   = ((row.flags & MSGPU_ROW_DIR) ? PF_DIR : 0u) | ((row.flags & MSGPU_ROW_PRIMARY) ? PF_PRIM : 0u) |
           (rank & PF_POS_MASK);
  return out;
}

// readlane of wider types (lane index must be wave-uniform)
__device__ __forceinline__ int rl_i32(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ uint32_t rl_u32(uint32_t v, int lane) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(v), lane));
}
__device__ __forceinline__ uint64_t rl_u64(uint64_t v, int lane) {
  uint32_t lo = rl_u32(static_cast<uint32_t>(v), lane), hi = rl_u32(static_cast<uint32_t>(v >> 32), lane);
  return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ double rl_f64(double v, int lane) {
  return __longlong_as_double(static_cast<long long>(rl_u64(static_cast<uint64_t>(__double_as_longlong(v)), lane)));
}

// v of lane (addr + OFF) / 4 (mod 64) through the LDS crossbar: two ds_bpermute_b32 with the instruction's immediate offset,
// which the builtin does not fold an addition into.  No vector-ALU instruction and no LDS memory; every lane must be active
// (an inactive source lane yields 0).  The compiler does not count an LDS instruction inside an asm statement, so the wait
// stands in the same statement and the outputs are early-clobber; nothing but the two results is written (no SCC, no EXEC,
// no memory).
template <int OFF> __device__ __forceinline__ double bpermute_f64(uint32_t addr, double v) {
  static_assert(OFF >= 0 && OFF < 65536, "16-bit unsigned offset");
  int lo, hi;
  asm volatile("ds_bpermute_b32 %0, %2, %3 offset:%5\n\t"
               "ds_bpermute_b32 %1, %2, %4 offset:%5\n\t"
               "s_waitcnt lgkmcnt(0)"
               : "=&v"(lo), "=&v"(hi)
               : "v"(addr), "v"(__double2loint(v)), "v"(__double2hiint(v)), "i"(OFF));
  return __hiloint2double(hi, lo);
}

// lane K of this lane's quad, to the whole quad (quad_perm:[K,K,K,K]: DPP control K * 0x55); the four lanes must be active
template <int K> __device__ __forceinline__ uint32_t quad_bcast(uint32_t v) {
  static_assert(K >= 0 && K < 4, "quad lane");
  return static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(v), K * 0x55, 0xf, 0xf, false));
}

// getOverlap (ol.cpp:53-101) on the four overhangs of a path -- L = the first anchor's on v1 / v2, R = the last anchor's, the
// v2 side already chosen by direction (main.cpp:73-76) -- and the rest of an order that follows from them: start / end / base
// from the edge's reads, the score truncated like path_t's std::size_t (a score in [0, 2^64): anything else is not a path
// score).  ONE copy of the arithmetic: k_compact finishes the chain kernels' RAW records with it (ORD_RAW, msgpu_internal.h),
// the host entry msgpu_order_finish lets a test without a GPU call it.  raw_flags: DIR and PRIMARY (the marker is dropped).
//
// The four cases are tried in the reference's order.  With s1 = sign(L1 ? L2), s2 = sign(R1 ? R2) and no NaN among the four:
//   (<,<) (<,=) (=,<) (=,=) -> case 1      (=,>) (>,=) (>,>) -> case 2      (>,<) -> case 3      (<,>) -> case 4
// so every ordered combination has a case, and `have` is false exactly when one of the four values is a NaN (every compare
// with a NaN is false).  The chain kernels decide `have` by that test alone; a record they emit always has its case here.
struct OrderFinish {
  bool     have;
  uint32_t flags; // MSGPU_ORD_*
  double   lo, ro;
  uint64_t score;
  uint32_t start, end, base;
};
__host__ __device__ inline OrderFinish order_finish(uint32_t raw_flags, double score, double L1, double L2, double R1, double R2,
                                                    uint32_t v1, uint32_t v2) {
  // (selects, not branches: the four lanes of a slot and the slots of a wavefront take different cases in k_compact.  The
  // offsets are the reference's own subtractions, L2 - L1 in the cases 1 and 4, R2 - R1 in the cases 1 and 3.)
  const bool c1 = (L1 <= L2) & (R1 <= R2);
  const bool c2 = !c1 & (L1 >= L2) & (R1 >= R2);
  const bool c3 = !c1 & !c2 & (L1 > L2) & (R1 < R2);
  const bool c4 = !c1 & !c2 & !c3 & (L1 < L2) & (R1 > R2);
  OrderFinish    o;
  o.have            = c1 | c2 | c3 | c4;
  const uint32_t fl = c1 ? (MSGPU_ORD_START_V1 | MSGPU_ORD_CONTAINED) : c2 ? MSGPU_ORD_CONTAINED : c3 ? MSGPU_ORD_START_V1 : 0u;
  const double   dl = L2 - L1, dl_ = L1 - L2, dr = R2 - R1, dr_ = R1 - R2;
  o.lo    = (c1 | c4) ? dl : (c2 | c3) ? dl_ : 0.0;
  o.ro    = (c1 | c3) ? dr : (c2 | c4) ? dr_ : 0.0;
  o.flags = fl | (raw_flags & (MSGPU_ORD_DIR | MSGPU_ORD_PRIMARY));
  o.score = static_cast<uint64_t>(score);
  o.start = (fl & MSGPU_ORD_START_V1) ? v1 : v2;
  o.end   = (fl & MSGPU_ORD_START_V1) ? v2 : v1;
  o.base  = v1;
  return o;
}

// The read-back of the scalar block without a copy or a stream synchronisation, called by one whole wavefront:
// lane k holds the value of slot k.  The words go into the mapped host mirror, a system-scope fence makes them visible, then
// lane 0 release-stores the sequence number the host polls for.  Fence and store are the wavefront's own, so nothing else needs
// to wait: no barrier (in a workgroup of several wavefronts only the calling one gets here).  p.seq == 0: nothing is published.
__device__ __forceinline__ void publish_to_host(const HostPublish &p, int lane, uint64_t v) {
  if (!p.seq) return;
  if (lane < SC_COUNT) p.host[lane] = v;
  __threadfence_system();
  if (lane == 0) __hip_atomic_store(&p.host[SC_COUNT], p.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// std::max / std::min on doubles with the library's tie and NaN behaviour (NOT fmax/fmin)
__device__ __forceinline__ double std_max(double a, double b) { return (a < b) ? b : a; }
__device__ __forceinline__ double std_min(double a, double b) { return (b < a) ? b : a; }

// block-wide exclusive scan of one value per thread, NT threads; returns exclusive prefix, total through *total
// inclusive scan over the wavefront with data-parallel-primitive moves (vector-ALU latency; __shfl_up is a ds_bpermute, one
// LDS round trip per step): Hillis-Steele inside the rows of 16 lanes (lanes without a source add 0), then lane 15 of
// rows 0 / 2 into rows 1 / 3 (row_bcast:15, row mask 0xa) and lane 31 into rows 2 and 3 (row_bcast:31, row mask 0xc)
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) {
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x111, 0xf, 0xf, false)); // row_shr:1
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x112, 0xf, 0xf, false)); // row_shr:2
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x114, 0xf, 0xf, false)); // row_shr:4
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x118, 0xf, 0xf, false)); // row_shr:8
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x142, 0xa, 0xf, false)); // row_bcast:15
  v += static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x143, 0xc, 0xf, false)); // row_bcast:31
  return v;
}

// the same scan of 32-bit items with a 64-bit result
__device__ __forceinline__ uint64_t wave_incl_scan64(uint32_t v) {
  uint64_t inc = v;
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  return inc;
}
// sum over the wavefront, the same value in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(wave_incl_scan(v)), 63));
}

// fp64 maxima over lanes without LDS.  Every step is fmax(v, v moved by a DPP control): two v_mov_b32_dpp and one
// v_max_f64, where a __shfl_xor / __shfl_up step is index arithmetic, two ds_bpermute and a wait for the LDS round trip.
// The maximum is __builtin_fmax's (a NaN operand is skipped); a lane without a DPP source keeps its own value (the
// moves' `old` operand is the value itself), so no identity constant takes part.  All 64 lanes must be active.
// PERMUTES: the control gives every lane a source (quad_perm, the mirrors), so the moves need no `old` operand -- and no
// copy of the value to tie it to.
template <int CTRL, int ROW_MASK = 0xf, bool PERMUTES = false> __device__ __forceinline__ double dpp_max_step(double v) {
  const unsigned long long b  = __builtin_bit_cast(unsigned long long, v);
  const int                lo = static_cast<int>(static_cast<uint32_t>(b)), hi = static_cast<int>(static_cast<uint32_t>(b >> 32));
  uint32_t                 ml, mh;
  if constexpr (PERMUTES) {
    static_assert(ROW_MASK == 0xf, "every row takes part in a permutation");
    ml = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(lo, CTRL, 0xf, 0xf, false));
    mh = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(hi, CTRL, 0xf, 0xf, false));
  } else {
    ml = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false));
    mh = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false));
  }
  return __builtin_fmax(v, __builtin_bit_cast(double, (static_cast<unsigned long long>(mh) << 32) | ml));
}
// the maximum of every aligned group of W lanes (W = 8, 16, 32, 64), in all of its lanes.  Inside a row of 16 lanes:
// quad_perm:[1,0,3,2] and [2,3,0,1] make the quads uniform, row_half_mirror exchanges the two quads of a half-row,
// row_mirror the two half-rows.  Across rows one exchange per level: v_permlane16_swap of the value with itself returns
// (row 0, row 0, row 2, row 2) and (row 1, row 1, row 3, row 3), v_permlane32_swap the lower and the upper 32 lanes twice.
template <int W> __device__ __forceinline__ double group_max_f64(double v) {
  static_assert(W == 8 || W == 16 || W == 32 || W == 64, "group width");
  v = dpp_max_step<0xb1, 0xf, true>(v);  // quad_perm:[1,0,3,2]
  v = dpp_max_step<0x4e, 0xf, true>(v);  // quad_perm:[2,3,0,1]
  v = dpp_max_step<0x141, 0xf, true>(v); // row_half_mirror
  if constexpr (W >= 16) v = dpp_max_step<0x140, 0xf, true>(v); // row_mirror
  if constexpr (W >= 32) {
    const unsigned long long b  = __builtin_bit_cast(unsigned long long, v);
    const auto               lo = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(b), static_cast<uint32_t>(b), false, false);
    const auto               hi = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(b >> 32), static_cast<uint32_t>(b >> 32), false, false);
    v = __builtin_fmax(__builtin_bit_cast(double, (static_cast<unsigned long long>(hi[0]) << 32) | lo[0]),
                       __builtin_bit_cast(double, (static_cast<unsigned long long>(hi[1]) << 32) | lo[1]));
  }
  if constexpr (W == 64) {
    const unsigned long long b  = __builtin_bit_cast(unsigned long long, v);
    const auto               lo = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(b), static_cast<uint32_t>(b), false, false);
    const auto               hi = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(b >> 32), static_cast<uint32_t>(b >> 32), false, false);
    v = __builtin_fmax(__builtin_bit_cast(double, (static_cast<unsigned long long>(hi[0]) << 32) | lo[0]),
                       __builtin_bit_cast(double, (static_cast<unsigned long long>(hi[1]) << 32) | lo[1]));
  }
  return v;
}
// The same exchanges on 64-bit integers: the maximum of every aligned group of W lanes (W = 16 or 64), in all of its lanes.
// The mapper's chain kernels (msgpu_map.hip) reduce (score, predecessor) packed into one word with it.  All 64 lanes must
// be active.
template <int CTRL> __device__ __forceinline__ long long dpp_perm_max_i64(long long v) {
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(static_cast<uint32_t>(v)), CTRL, 0xf, 0xf, false));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_mov_dpp(static_cast<int>(static_cast<uint32_t>(static_cast<unsigned long long>(v) >> 32)), CTRL, 0xf, 0xf, false));
  const long long o = static_cast<long long>((static_cast<unsigned long long>(hi) << 32) | lo);
  return o > v ? o : v;
}
template <int W> __device__ __forceinline__ long long group_max_i64(long long v) {
  static_assert(W == 16 || W == 64, "group width");
  v = dpp_perm_max_i64<0xb1>(v);  // quad_perm:[1,0,3,2]
  v = dpp_perm_max_i64<0x4e>(v);  // quad_perm:[2,3,0,1]
  v = dpp_perm_max_i64<0x141>(v); // row_half_mirror
  v = dpp_perm_max_i64<0x140>(v); // row_mirror
  if constexpr (W == 64) {
    const unsigned long long b = static_cast<unsigned long long>(v);
    auto lo = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(b), static_cast<uint32_t>(b), false, false);
    auto hi = __builtin_amdgcn_permlane16_swap(static_cast<uint32_t>(b >> 32), static_cast<uint32_t>(b >> 32), false, false);
    long long x = static_cast<long long>((static_cast<unsigned long long>(hi[0]) << 32) | lo[0]);
    long long y = static_cast<long long>((static_cast<unsigned long long>(hi[1]) << 32) | lo[1]);
    v = x > y ? x : y;
    const unsigned long long d = static_cast<unsigned long long>(v);
    lo = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(d), static_cast<uint32_t>(d), false, false);
    hi = __builtin_amdgcn_permlane32_swap(static_cast<uint32_t>(d >> 32), static_cast<uint32_t>(d >> 32), false, false);
    x = static_cast<long long>((static_cast<unsigned long long>(hi[0]) << 32) | lo[0]);
    y = static_cast<long long>((static_cast<unsigned long long>(hi[1]) << 32) | lo[1]);
    v = x > y ? x : y;
  }
  return v;
}
// inclusive prefix maximum over the wavefront: lane l gets the maximum of lanes 0..l (wave_incl_scan's moves)
__device__ __forceinline__ double wave_prefix_max_f64(double v) {
  v = dpp_max_step<0x111>(v);      // row_shr:1
  v = dpp_max_step<0x112>(v);      // row_shr:2
  v = dpp_max_step<0x114>(v);      // row_shr:4
  v = dpp_max_step<0x118>(v);      // row_shr:8
  v = dpp_max_step<0x142, 0xa>(v); // row_bcast:15 into rows 1 and 3
  v = dpp_max_step<0x143, 0xc>(v); // row_bcast:31 into rows 2 and 3
  return v;
}

template <int NT> __device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *s_wave /*[NT / 64]*/, uint32_t *total) {
  const int      lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t inc  = wave_incl_scan(v);
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const uint32_t x = s_wave[w];
    base += w < wave ? x : 0u;
    tot += x;
  }
  *total = tot;
  __syncthreads();
  return base + inc - v;
}
__device__ __forceinline__ uint32_t block_excl_scan_256(uint32_t v, uint32_t *s_wave /*[4]*/, uint32_t *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t  inc  = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint32_t t = __shfl_up(inc, d);
    if (lane >= d) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
  uint32_t base = (wave > 0 ? w0 : 0) + (wave > 1 ? w1 : 0) + (wave > 2 ? w2 : 0);
  *total        = w0 + w1 + w2 + w3;
  __syncthreads();
  return base + inc - v;
}

// The Vertex of a read is made at its first line (Graph.cpp:148: nanoporeLength and metaDatum(0) of that line).  key =
// line << 32 | source row index of a lane's row (all ones for a lane without one); every lane of the wavefront calls.
__device__ __forceinline__ void note_first_row(int lane, unsigned long long key, uint32_t r, const msgpu_row *rows,
                                               int32_t *read_len, uint32_t *read_first) {
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o =
        (static_cast<unsigned long long>(static_cast<uint32_t>(__shfl_xor(static_cast<int>(key >> 32), d))) << 32) |
        static_cast<uint32_t>(__shfl_xor(static_cast<int>(key), d));
    key = o < key ? o : key;
  }
  if (lane == 0) {
    read_first[r] = static_cast<uint32_t>(key >> 32);
    read_len[r]   = rows[static_cast<uint32_t>(key)].read_len;
  }
}

// ---- the small idioms of the stage files, one copy of each

// Counters that a whole wavefront feeds with one atomic.  Every lane of the wavefront calls these.
// `each` for every lane that says `mine`, added by the first of them
__device__ inline void wave_count(bool mine, unsigned long long *counter, unsigned long long each = 1) {
  const uint64_t who = __ballot(mine);
  if (who && (threadIdx.x & 63) == static_cast<uint32_t>(__ffsll(static_cast<long long>(who)) - 1)) atomicAdd(counter, each * __popcll(who));
}
// the sum of the lanes' values (a sum of zero adds nothing)
__device__ inline void wave_add(unsigned long long v, unsigned long long *counter) {
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0 && v) atomicAdd(counter, v);
}
// the maximum of the lanes' values (unsigned, of 32 or 64 bits; a maximum of zero changes nothing)
template <class T> __device__ inline void wave_max(T v, unsigned long long *counter) {
  for (int o = 32; o; o >>= 1) {
    const T w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  if ((threadIdx.x & 63) == 0 && v) atomicMax(counter, static_cast<unsigned long long>(v));
}

// Append behind a 64-bit cursor, one atomic per wavefront: the lanes that `take` get consecutive slots, in lane order.  Every
// lane of the wavefront calls; the answer means something to the takers only, and whether the slot lies inside the
// destination is the caller's test.
__device__ inline uint64_t wave_append(bool take, unsigned long long *cursor) {
  const uint64_t who = __ballot(take);
  if (!who) return 0;
  const int          lane = threadIdx.x & 63, first = __ffsll(static_cast<long long>(who)) - 1;
  unsigned long long at = 0;
  if (lane == first) at = atomicAdd(cursor, static_cast<unsigned long long>(__popcll(who)));
  at = __shfl(at, first);
  return at + __popcll(who & ((1ull << lane) - 1));
}

// the last i in [lo, hi) with a[i] <= x (a ascending, a[lo] <= x): the segment of element x in a table of segment offsets
__device__ inline uint32_t last_le(const uint64_t *a, uint32_t lo, uint32_t hi, uint64_t x) {
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

// decimal text, of the stages that format on the device (msgpu_sam.hip, msgpu_vcf.hip): the digits of a value, and the value
// in a width that the caller took from them
__device__ inline uint32_t dec_dig(uint64_t v) { // decimal digits
  uint32_t d = 1;
  for (uint64_t p = 10; d < 20 && v >= p; p *= 10) ++d;
  return d;
}
__device__ inline uint32_t dec_sdig(long long v) { return v < 0 ? 1 + dec_dig(0ull - static_cast<uint64_t>(v)) : dec_dig(static_cast<uint64_t>(v)); }
__device__ inline void dec_put(uint8_t *p, uint64_t v, uint32_t w) { // v in w digits
  for (uint32_t i = w; i--;) {
    p[i] = static_cast<uint8_t>('0' + v % 10);
    v /= 10;
  }
}
__device__ inline void dec_sput(uint8_t *p, long long v, uint32_t w) { // v in w bytes, the sign among them
  if (v < 0) {
    p[0] = '-';
    dec_put(p + 1, 0ull - static_cast<uint64_t>(v), w - 1);
  } else dec_put(p, static_cast<uint64_t>(v), w);
}
// a base as the text formats write it: upper case, anything but A, C, G, T -> N, the complement on request
__device__ inline uint8_t text_base(uint8_t b, uint32_t comp) {
  if (b >= 'a' && b <= 'z') b -= 32;
  if (b != 'A' && b != 'C' && b != 'G' && b != 'T') return 'N';
  if (comp) b = b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : 'C';
  return b;
}

// a device word into a slot of the scalar block (msgpu_stage.h, stage_scan_total, launches it behind a scan)
template <class T> __global__ void k_stage_put(uint64_t *scalars, int slot, const T *src) {
  if (threadIdx.x == 0 && blockIdx.x == 0) scalars[slot] = static_cast<uint64_t>(*src);
}

// Segment starts.  head[i] = element i opens a segment, id = the exclusive scan of head over n + 1 words (a zero behind the
// heads), so id[n] = the segments: start[s] = the first element of segment s, start[segments] = n.  A grid over n + 1:
// thread n writes the closing entry, whatever n is
template <class T> __global__ __launch_bounds__(256) void k_stage_seg_starts(const T *head, const T *id, T n, T *start) {
  const T i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && head[i]) start[id[i]] = i;
  if (i == n) start[id[n]] = n;
}

// ---- the records of a sequence store as the kernels of the stages see them (msgpu_stage.h, stage_load, fills one)

constexpr uint32_t REC_NONE = 0xffffffffu;

struct SeqRecs {
  const uint8_t  *bases;
  const uint64_t *off; // ascending
  const uint32_t *len; // (a zero behind the n lengths)
  uint32_t        n;
  uint64_t        n_bases;
};

// the record that holds byte p of the store, or REC_NONE (padding between records)
__device__ inline uint32_t seq_record(const SeqRecs &R, uint64_t p) {
  uint32_t lo = 0, hi = R.n; // the last r with off[r] <= p
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (R.off[mid] <= p) lo = mid + 1;
    else hi = mid;
  }
  if (!lo) return REC_NONE;
  const uint32_t r = lo - 1;
  return p < R.off[r] + R.len[r] ? r : REC_NONE;
}

__device__ __forceinline__ bool key_less(int alo, int ahi, uint32_t aan, int blo, int bhi, uint32_t ban) {
  return alo < blo || (alo == blo && (ahi < bhi || (ahi == bhi && aan < ban)));
}

} // namespace msgpu

#endif
