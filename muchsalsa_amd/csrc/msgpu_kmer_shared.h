// msgpu_kmer_shared.h -- what the k-mer abundance filter (msgpu_kmer.hip) and the short-read unitig assembly
// (msgpu_unitig.hip) both use, defined once: the rolling window, the hash and the partitions cut from its bins, the window
// kernels (bins, extract), the selection of (key, count) pairs, the open-addressing table of indices over a sorted key array,
// and on the host the partitioned exact count and the gathering of its chunks into one sorted array (on the stage
// scaffolding of msgpu_stage.h).  The file upload, the line starts and the FASTQ check live in msgpu_kmer.hip and are
// declared here.
#ifndef MSGPU_KMER_SHARED_H
#define MSGPU_KMER_SHARED_H

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "msgpu.h"
#include "msgpu_internal.h"
#include "msgpu_kmer_wide.h"
#include "msgpu_stage.h"

namespace msgpu {

typedef unsigned long long     kf_ull; // (kf_u128 and the key of three and of four words: msgpu_kmer_wide.h)
constexpr uint32_t KF_TILE   = 4096;  // bytes of a file per workgroup in the line kernels (16 per thread)
constexpr uint32_t KF_BINS   = 4096;  // hash bins the partitions are cut from
constexpr uint32_t KF_KEEP   = 5;     // a k-mer below this count can never reach the threshold (upper >= 5)
constexpr uint32_t KF_HIGH   = 10001; // jellyfish histo's last row
constexpr uint32_t KF_LOWBIN = 1024;  // histogram bins privatised per workgroup
constexpr uint32_t KF_EMPTY  = 0xffffffffu;

struct KfIn { // the files as the kernels see them: read t < n_first is record t of file 0, the others follow in file 1
  const uint8_t  *buf[2];
  const uint64_t *ls[2]; // line starts, n_lines + 1 entries: line l is [ls[l], ls[l + 1] - 1)
  uint64_t        n_first, n_reads;
  int             k;
  const uint8_t  *dropped = nullptr; // a byte per pair, 1 = the pair's two reads count as empty (msgpu_ug_run_pair); null: no mask
};

// splitmix64's finaliser over both halves of the key
__device__ inline uint64_t kf_mix(uint64_t lo, uint64_t hi) {
  uint64_t x = lo ^ (hi * 0x9e3779b97f4a7c15ull);
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
__device__ inline uint64_t kf_hash(uint64_t k) { return kf_mix(k, 0); }
__device__ inline uint64_t kf_hash(kf_u128 k) { return kf_mix(static_cast<uint64_t>(k), static_cast<uint64_t>(k >> 64)); }
// every word of a wider key, folded pairwise
__device__ inline uint64_t kf_hash(const KfWide<3> &k) { return kf_mix(kf_mix(k.w[0], k.w[1]), k.w[2]); }
__device__ inline uint64_t kf_hash(const KfWide<4> &k) { return kf_mix(kf_mix(k.w[0], k.w[1]), kf_mix(k.w[2], k.w[3])); }
template <class K> __device__ inline uint32_t kf_bin(K key) { return static_cast<uint32_t>(kf_hash(key) >> 52); } // KF_BINS = 2^12
__device__ inline uint32_t kf_part(uint32_t bin, uint32_t P) { return (bin * P) >> 12; }

// the rolling window: step() takes one byte of a sequence line and says whether a window ends on it (a key of W words has a
// step of its own, msgpu_kmer_wide.h)
template <class K> struct KfRoll {
  K        fw = 0, rc = 0, mask;
  uint32_t run = 0, k;
  int      top;
  __device__ explicit KfRoll(int k_) : k(static_cast<uint32_t>(k_)), top(2 * (k_ - 1)) {
    mask = (2 * k_ == static_cast<int>(sizeof(K) * 8)) ? ~static_cast<K>(0) : ((static_cast<K>(1) << (2 * k_)) - 1);
  }
  __device__ bool step(uint8_t b, K &key) {
    const uint32_t u = b & 0xdfu; // case folded
    if (!(u == 'A' || u == 'C' || u == 'G' || u == 'T')) {
      run = 0;
      return false;
    }
    const uint32_t c = ((u >> 1) & 3u) ^ ((u >> 2) & 1u); // A 0, C 1, G 2, T 3
    fw = ((fw << 2) | static_cast<K>(c)) & mask;
    rc = (rc >> 2) | (static_cast<K>(3u - c) << top);
    if (++run < k) return false;
    key = fw < rc ? fw : rc;
    return true;
  }
};

// read t of n_reads (file 0 first): its sequence line
__device__ inline void kf_read(const KfIn &in, uint64_t t, const uint8_t *&s, uint64_t &len) {
  const int      f = t >= in.n_first;
  const uint64_t r = t - (f ? in.n_first : 0);
  const uint64_t a = in.ls[f][4 * r + 1], e = in.ls[f][4 * r + 2] - 1;
  s   = in.buf[f] + a;
  len = (in.dropped && in.dropped[r]) ? 0 : e - a; // (with a mask both files have n_first records: r is the pair)
}

// windows per hash bin
template <class K> __global__ __launch_bounds__(256) void k_kf_bins(KfIn in, kf_ull *bins) {
  __shared__ uint32_t h[KF_BINS];
  for (uint32_t i = threadIdx.x; i < KF_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const uint64_t n = in.n_reads, stride = static_cast<uint64_t>(gridDim.x) * 256;
  for (uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x; t < n; t += stride) {
    const uint8_t *s;
    uint64_t       len;
    kf_read(in, t, s, len);
    KfRoll<K> roll(in.k);
    K         key;
    for (uint64_t i = 0; i < len; ++i)
      if (roll.step(s[i], key)) atomicAdd(&h[kf_bin(key)], 1u);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < KF_BINS; i += 256)
    if (h[i]) atomicAdd(&bins[i], static_cast<kf_ull>(h[i]));
}

// the canonical keys of partition p.  Sweep 1 counts the lane's keys; the wavefront reserves one range; sweep 2 walks the
// 64 reads in step and writes each step's keys side by side.
template <class K>
__global__ __launch_bounds__(256) void k_kf_extract(KfIn in, uint32_t P, uint32_t p, K *out, uint64_t cap, kf_ull *cursor) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int      lane = threadIdx.x & 63;
  const uint8_t *s = nullptr;
  uint64_t       len = 0;
  if (t < in.n_reads) kf_read(in, t, s, len);
  uint32_t mine = 0;
  {
    KfRoll<K> roll(in.k);
    K         key;
    for (uint64_t i = 0; i < len; ++i)
      if (roll.step(s[i], key) && kf_part(kf_bin(key), P) == p) ++mine;
  }
  uint64_t sum = mine, longest = len;
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o);
    longest = max(longest, static_cast<uint64_t>(__shfl_xor(longest, o)));
  }
  if (!sum) return; // (the whole wavefront)
  kf_ull at = 0;
  if (lane == 0) at = atomicAdd(cursor, static_cast<kf_ull>(sum));
  at = __shfl(at, 0);
  KfRoll<K> roll(in.k);
  for (uint64_t i = 0; i < longest; ++i) {
    K          key = 0;
    const bool put = i < len && roll.step(s[i], key) && kf_part(kf_bin(key), P) == p;
    const uint64_t who = __ballot(put);
    if (put) {
      const uint64_t slot = at + __popcll(who & ((1ull << lane) - 1));
      if (slot < cap) out[slot] = key;
    }
    at += __popcll(who);
  }
}

// the (key, count) with count >= least.  WRITE = false only counts them (into *cursor).
template <class K, bool WRITE>
__global__ __launch_bounds__(256) void k_kf_select(const K *keys, const uint32_t *cnt, uint64_t n, uint32_t least, K *out_k,
                                                   uint32_t *out_c, uint64_t cap, kf_ull *cursor) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool     take = i < n && cnt[i] >= least;
  const uint64_t slot = wave_append(take, cursor);
  if (WRITE && take && slot < cap) {
    out_k[slot] = keys[i];
    out_c[slot] = cnt[i];
  }
}

// open addressing over the abundant set: a slot holds an index into the sorted keys
template <class K> __global__ __launch_bounds__(256) void k_kf_table(const K *keys, uint32_t n, uint32_t *slots, uint32_t mask) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (uint32_t h = static_cast<uint32_t>(kf_hash(keys[i])) & mask;; h = (h + 1) & mask)
    if (atomicCAS(&slots[h], KF_EMPTY, i) == KF_EMPTY) return; // (the table has at least 2 n slots)
}

// the index of `key` in the sorted keys, or KF_EMPTY
template <class K> __device__ inline uint32_t kf_find(const K *keys, const uint32_t *slots, uint32_t mask, K key) {
  for (uint32_t h = static_cast<uint32_t>(kf_hash(key)) & mask;; h = (h + 1) & mask) {
    const uint32_t j = slots[h];
    if (j == KF_EMPTY || keys[j] == key) return j;
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------

// rocPRIM's radix sorts over the key's bits [0, end_bit): a built-in integer as it is, a key of W words through a decomposer
// whose tuple names the words from the top one down, so that bit 0 is bit 0 of w[0] and the bits at and above end_bit stay
// out of the sort
template <int W> struct KfWideDecomposer;
template <> struct KfWideDecomposer<3> {
  __host__ __device__ rocprim::tuple<uint64_t &, uint64_t &, uint64_t &> operator()(KfWide<3> &key) const {
    return rocprim::tuple<uint64_t &, uint64_t &, uint64_t &>(key.w[2], key.w[1], key.w[0]);
  }
};
template <> struct KfWideDecomposer<4> {
  __host__ __device__ rocprim::tuple<uint64_t &, uint64_t &, uint64_t &, uint64_t &> operator()(KfWide<4> &key) const {
    return rocprim::tuple<uint64_t &, uint64_t &, uint64_t &, uint64_t &>(key.w[3], key.w[2], key.w[1], key.w[0]);
  }
};
template <class K, class Size>
hipError_t kf_sort_keys(void *tmp, size_t &bytes, rocprim::double_buffer<K> &db, Size n, int end_bit, hipStream_t st) {
  return rocprim::radix_sort_keys(tmp, bytes, db, n, 0, end_bit, st);
}
template <int W, class Size>
hipError_t kf_sort_keys(void *tmp, size_t &bytes, rocprim::double_buffer<KfWide<W>> &db, Size n, int end_bit, hipStream_t st) {
  return rocprim::radix_sort_keys(tmp, bytes, db, n, KfWideDecomposer<W>{}, 0u, static_cast<unsigned int>(end_bit), st);
}
template <class K, class V, class Size>
hipError_t kf_sort_pairs(void *tmp, size_t &bytes, K *kin, K *kout, V *vin, V *vout, Size n, int end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, 0, end_bit, st);
}
template <int W, class V, class Size>
hipError_t kf_sort_pairs(void *tmp, size_t &bytes, KfWide<W> *kin, KfWide<W> *kout, V *vin, V *vout, Size n, int end_bit, hipStream_t st) {
  return rocprim::radix_sort_pairs(tmp, bytes, kin, kout, vin, vout, n, KfWideDecomposer<W>{}, 0u, static_cast<unsigned int>(end_bit), st);
}

struct KfFile {
  uint8_t  *d = nullptr;
  uint64_t  size = 0, n_lines = 0;
  uint64_t *ls = nullptr;
  bool      open_end = false; // the last line has no '\n'
};

} // namespace msgpu

// What kf_upload and kf_records leave on the device, kept until msgpu_pair_close: the bytes of one or two FASTQ files,
// their line starts, the format check done.  A run reads it and writes nothing into it.
struct msgpu_pair {
  int             device = 0;
  int             n_files = 0;
  msgpu::DevArena D;
  msgpu::KfFile   F[2]; // (one file: F[1] points at F[0]'s bytes and has no lines, so no read of it is ever asked for)
  float           load_ms = 0.f, records_ms = 0.f;
};

namespace msgpu {

// defined in msgpu_kmer.hip
int kf_upload(StageCtx *c, DevArena &D, const char *path, int which, KfFile &f); // mmap -> page-locked ring -> device
int kf_lines(StageCtx *c, DevArena &D, KfFile &f);                                // the line starts of a file on the device
int kf_format_error(StageCtx *c, int which, uint64_t line, const char *what);
int kf_records(StageCtx *c, DevArena &D, KfFile *F, int n_files); // line starts and the FASTQ rules of every file, file 0 first
// both of the above for one or two files (path_b may be null) into a new msgpu_pair on c's device; c takes the error
int  kf_pair_open(StageCtx *c, const char *path_a, const char *path_b, msgpu_pair **out);
void kf_pair_close(msgpu_pair *p);

// ---- the partitions: P ranges of the KF_BINS hash bins
inline uint32_t kf_first_bin(uint32_t p, uint32_t P) { return static_cast<uint32_t>((uint64_t(p) * KF_BINS + P - 1) / P); }
struct KfParts {
  uint32_t P = 0;       // 0: no cut fits
  uint64_t largest = 0; // windows of the largest partition
};
// the smallest number of partitions whose largest stays within the budget and below 2^31 windows; pre = prefix sums of the bins
inline KfParts kf_pick_partitions(const std::vector<uint64_t> &pre, uint64_t per_key, uint64_t budget) {
  KfParts r;
  for (uint32_t q = 1; q <= KF_BINS && !r.P; ++q) {
    uint64_t m = 0;
    for (uint32_t p = 0; p < q; ++p) m = std::max(m, pre[kf_first_bin(p + 1, q)] - pre[kf_first_bin(p, q)]);
    if (m < (1ull << 31) && m * per_key <= budget) {
      r.P       = q;
      r.largest = m;
    }
  }
  return r;
}

// windows per hash bin -> their prefix sums (KF_BINS + 1 entries)
template <class K> int kf_bin_prefix(StageCtx *c, DevArena &D, StageClock &clock, const KfIn &in, float *ms, std::vector<uint64_t> &pre) {
  hipStream_t st = c->stream;
  kf_ull     *d_bins;
  STAGE_HIP(c, D.get(&d_bins, KF_BINS));
  STAGE_HIP(c, hipMemsetAsync(d_bins, 0, KF_BINS * 8, st));
  STAGE_HIP(c, clock.begin(ms));
  const uint32_t read_grid = grid256(in.n_reads);
  if (in.n_reads) hipLaunchKernelGGL(k_kf_bins<K>, dim3(std::min<uint32_t>(read_grid, 4096)), dim3(256), 0, st, in, d_bins);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  std::vector<kf_ull> bins(KF_BINS);
  STAGE_HIP(c, hipMemcpyAsync(bins.data(), d_bins, KF_BINS * 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));
  pre.assign(KF_BINS + 1, 0);
  for (uint32_t b = 0; b < KF_BINS; ++b) pre[b + 1] = pre[b] + bins[b];
  D.drop(d_bins);
  return MSGPU_OK;
}

template <class K> struct KfChunk { // the (key, count) a partition keeps
  K        *k;
  uint32_t *c;
  uint64_t  n;
};
struct KfCountMs {
  float *extract, *sort, *runs, *select;
};

// The exact count: per partition extract, sort, run lengths; `each(run lengths, runs)` sees every partition's counts (the
// filter's histogram); the (key, count) with count >= least stay on the device as one chunk per partition.
template <class K, class Each>
int kf_count(StageCtx *c, DevArena &D, StageClock &clock, const KfIn &in, const std::vector<uint64_t> &pre, const KfParts &parts, int k,
             uint32_t least, const KfCountMs &ms, kf_ull *d_cur, Each &&each, std::vector<KfChunk<K>> &chunks, uint64_t &n_distinct,
             uint64_t &n_kept) {
  hipStream_t    st = c->stream;
  const uint32_t P = parts.P, read_grid = grid256(in.n_reads);
  const uint64_t largest = parts.largest;
  K             *d_a, *d_b;
  uint32_t      *d_rl, *d_nruns;
  STAGE_HIP(c, D.get(&d_a, largest));
  STAGE_HIP(c, D.get(&d_b, largest));
  STAGE_HIP(c, D.get(&d_rl, largest));
  STAGE_HIP(c, D.get(&d_nruns, 1));
  size_t need_sort = 0, need_rle = 0;
  {
    rocprim::double_buffer<K> db(d_a, d_b);
    STAGE_HIP(c, kf_sort_keys(nullptr, need_sort, db, largest, 2 * k, st));
    STAGE_HIP(c, rocprim::run_length_encode(nullptr, need_rle, d_a, static_cast<unsigned int>(largest), d_b, d_rl, d_nruns, st));
  }
  const size_t tmp_bytes = std::max(need_sort, need_rle);
  uint8_t     *d_tmp;
  STAGE_HIP(c, D.get(&d_tmp, tmp_bytes));
  for (uint32_t p = 0; p < P; ++p) {
    const uint64_t n = pre[kf_first_bin(p + 1, P)] - pre[kf_first_bin(p, P)];
    if (!n) continue;
    STAGE_HIP(c, hipMemsetAsync(d_cur, 0, 8, st));
    STAGE_HIP(c, clock.begin(ms.extract));
    hipLaunchKernelGGL(k_kf_extract<K>, dim3(read_grid), dim3(256), 0, st, in, P, p, d_a, n, d_cur);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    rocprim::double_buffer<K> db(d_a, d_b);
    size_t                    tb = tmp_bytes;
    STAGE_HIP(c, clock.begin(ms.sort));
    STAGE_HIP(c, kf_sort_keys(d_tmp, tb, db, n, 2 * k, st));
    STAGE_HIP(c, clock.end());
    K *sorted = db.current(), *uniq = db.alternate();
    tb = tmp_bytes;
    STAGE_HIP(c, clock.begin(ms.runs));
    STAGE_HIP(c, rocprim::run_length_encode(d_tmp, tb, sorted, static_cast<unsigned int>(n), uniq, d_rl, d_nruns, st));
    STAGE_HIP(c, clock.end());
    uint32_t runs = 0;
    kf_ull   written = 0;
    STAGE_HIP(c, hipMemcpyAsync(&runs, d_nruns, 4, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(&written, d_cur, 8, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipStreamSynchronize(st));
    if (written != n) { // the two window passes disagree: never seen; a result built on it would be wrong
      snprintf(c->err, sizeof(c->err), "partition %u: %llu keys extracted where %llu were counted", p, written,
               static_cast<kf_ull>(n));
      return MSGPU_E_STATE;
    }
    n_distinct += runs;
    const uint32_t run_grid = grid256(runs);
    STAGE_HIP(c, hipMemsetAsync(d_cur, 0, 8, st));
    const int rc = each(d_rl, runs);
    if (rc != MSGPU_OK) return rc;
    STAGE_HIP(c, clock.begin(ms.select));
    hipLaunchKernelGGL((k_kf_select<K, false>), dim3(run_grid), dim3(256), 0, st, uniq, d_rl, runs, least, nullptr, nullptr, 0,
                       d_cur);
    STAGE_HIP(c, hipGetLastError());
    kf_ull kept = 0;
    STAGE_HIP(c, hipMemcpyAsync(&kept, d_cur, 8, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipStreamSynchronize(st));
    if (kept) {
      KfChunk<K> ch{nullptr, nullptr, kept};
      STAGE_HIP(c, D.get(&ch.k, kept));
      STAGE_HIP(c, D.get(&ch.c, kept));
      STAGE_HIP(c, hipMemsetAsync(d_cur, 0, 8, st));
      hipLaunchKernelGGL((k_kf_select<K, true>), dim3(run_grid), dim3(256), 0, st, uniq, d_rl, runs, least, ch.k, ch.c, kept,
                         d_cur);
      STAGE_HIP(c, hipGetLastError());
      chunks.push_back(ch);
      n_kept += kept;
    }
    STAGE_HIP(c, clock.end());
  }
  STAGE_HIP(c, hipStreamSynchronize(st));
  D.drop(d_a);
  D.drop(d_b);
  D.drop(d_rl);
  D.drop(d_tmp);
  D.drop(d_nruns);
  return MSGPU_OK;
}

// how many (key, count) of the chunks have count >= least
template <class K> int kf_count_selected(StageCtx *c, const std::vector<KfChunk<K>> &chunks, uint32_t least, kf_ull *d_cur, kf_ull &n) {
  hipStream_t st = c->stream;
  STAGE_HIP(c, hipMemsetAsync(d_cur, 0, 8, st));
  for (const KfChunk<K> &ch : chunks)
    hipLaunchKernelGGL((k_kf_select<K, false>), dim3(grid256(ch.n)), dim3(256), 0, st, ch.k, ch.c,
                       ch.n, least, nullptr, nullptr, 0, d_cur);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, hipMemcpyAsync(&n, d_cur, 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));
  return MSGPU_OK;
}

// those n pairs as one array sorted ascending by key (the chunks are freed), and the open-addressing table of indices over it
template <class K>
int kf_gather_sorted(StageCtx *c, DevArena &D, std::vector<KfChunk<K>> &chunks, uint32_t least, uint64_t n, int k, kf_ull *d_cur,
                     K **keys, uint32_t **counts, uint32_t **slots, uint32_t *slots_n) {
  hipStream_t st = c->stream;
  K          *d_k = nullptr, *d_k_in;
  uint32_t   *d_c = nullptr, *d_c_in;
  STAGE_HIP(c, D.get(&d_k, n));
  STAGE_HIP(c, D.get(&d_c, n));
  if (n) {
    STAGE_HIP(c, D.get(&d_k_in, n));
    STAGE_HIP(c, D.get(&d_c_in, n));
    STAGE_HIP(c, hipMemsetAsync(d_cur, 0, 8, st));
    for (const KfChunk<K> &ch : chunks)
      hipLaunchKernelGGL((k_kf_select<K, true>), dim3(grid256(ch.n)), dim3(256), 0, st, ch.k, ch.c,
                         ch.n, least, d_k_in, d_c_in, n, d_cur);
    STAGE_HIP(c, hipGetLastError());
    size_t need = 0;
    STAGE_HIP(c, kf_sort_pairs(nullptr, need, d_k_in, d_k, d_c_in, d_c, n, 2 * k, st));
    uint8_t *tmp;
    STAGE_HIP(c, D.get(&tmp, need));
    STAGE_HIP(c, kf_sort_pairs(tmp, need, d_k_in, d_k, d_c_in, d_c, n, 2 * k, st));
    STAGE_HIP(c, hipStreamSynchronize(st));
    D.drop(tmp);
    D.drop(d_k_in);
    D.drop(d_c_in);
  }
  for (const KfChunk<K> &ch : chunks) {
    D.drop(ch.k);
    D.drop(ch.c);
  }
  chunks.clear();
  uint32_t sn = 64;
  while (sn < 2 * n) sn <<= 1;
  uint32_t *d_slots;
  STAGE_HIP(c, D.get(&d_slots, sn));
  STAGE_HIP(c, hipMemsetAsync(d_slots, 0xff, sn * 4ull, st));
  if (n)
    hipLaunchKernelGGL(k_kf_table<K>, dim3(grid256(n)), dim3(256), 0, st, d_k, static_cast<uint32_t>(n),
                       d_slots, sn - 1);
  STAGE_HIP(c, hipGetLastError());
  *keys    = d_k;
  *counts  = d_c;
  *slots   = d_slots;
  *slots_n = sn;
  return MSGPU_OK;
}

} // namespace msgpu

#endif
