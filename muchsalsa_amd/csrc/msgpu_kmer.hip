// msgpu_kmer.hip -- the Illumina k-mer abundance filter (include/msgpu.h, "k-mer abundance filter").
//
// Both FASTQ files live whole in HBM as raw bytes.  The device finds the lines (count '\n' per tile, scan, write the line
// starts), checks the four-line format (one atomicMin keeps the smallest offending line), and forms the canonical k-mers of
// every read with a rolling pair (forward, reverse complement): one thread per read, k <= 32 in one 64-bit word, 33..64
// in unsigned __int128.  Counting is sort-and-count in P partitions by a mixing hash of the canonical key:
//   k_kf_bins      windows per hash bin (KF_BINS bins, privatised in LDS)  -> the host picks P, every buffer has its exact size
//   k_kf_extract   the keys of partition p (two sweeps: count, reserve one range per wavefront, write coalesced)
//   rocPRIM        radix_sort_keys over bits [0, 2k) on a double buffer, run_length_encode -> (key, count)
//   k_kf_hist      counts -> the 10001 bins (the low bins privatised in LDS)
//   k_kf_select    (key, count) with count >= KF_KEEP -> the candidate table; after the threshold, count >= upper -> the
//                  abundant set, sorted ascending, and an open-addressing table of indices over it (k_kf_table)
//   k_kf_verdict   the windows again, each looked up; any hit in either mate sets the pair's byte
//   k_kf_copy      the surviving records, whole, one wavefront per record, to offsets from a scan of their byte lengths
//
// Kernel rules: vector stores and vector atomics only; no inline asm.
#include <hip/hip_runtime.h>
#include <rocprim/block/block_scan.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "msgpu.h"

namespace msgpu {

typedef unsigned __int128      kf_u128;
typedef unsigned long long     kf_ull;
constexpr uint32_t KF_TILE   = 4096;  // bytes of a file per workgroup in the line kernels (16 per thread)
constexpr uint32_t KF_BINS   = 4096;  // hash bins the partitions are cut from
constexpr uint32_t KF_KEEP   = 5;     // a k-mer below this count can never reach the threshold (upper >= 5)
constexpr uint32_t KF_HIGH   = 10001; // jellyfish histo's last row
constexpr uint32_t KF_LOWBIN = 1024;  // histogram bins privatised per workgroup
constexpr uint32_t KF_EMPTY  = 0xffffffffu;

struct KfIn { // the two files as the kernels see them
  const uint8_t  *buf[2];
  const uint64_t *ls[2]; // line starts, n_lines + 1 entries: line l is [ls[l], ls[l + 1] - 1)
  uint64_t        n_pairs;
  int             k;
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
template <class K> __device__ inline uint32_t kf_bin(K key) { return static_cast<uint32_t>(kf_hash(key) >> 52); } // KF_BINS = 2^12
__device__ inline uint32_t kf_part(uint32_t bin, uint32_t P) { return (bin * P) >> 12; }

// the rolling window: step() takes one byte of a sequence line and says whether a window ends on it
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

// read t of 2 * n_pairs (file 0 first): its sequence line
__device__ inline void kf_read(const KfIn &in, uint64_t t, const uint8_t *&s, uint64_t &len) {
  const int      f = t >= in.n_pairs;
  const uint64_t r = t - (f ? in.n_pairs : 0);
  const uint64_t a = in.ls[f][4 * r + 1], e = in.ls[f][4 * r + 2] - 1;
  s   = in.buf[f] + a;
  len = e - a;
}

// 16 bytes at `base` (a multiple of 16; the buffer is padded): bit i = byte i is '\n' and lies inside the file
__device__ inline uint32_t kf_nl_mask(const uint8_t *buf, uint64_t base, uint64_t size) {
  if (base >= size) return 0;
  const uint4    v = *reinterpret_cast<const uint4 *>(buf + base);
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
  uint32_t       m = 0;
  for (int i = 0; i < 16; ++i)
    if (((w[i >> 2] >> (8 * (i & 3))) & 0xffu) == '\n') m |= 1u << i;
  const uint64_t left = size - base;
  return left >= 16 ? m : (m & ((1u << left) - 1));
}

// WRITE = false: '\n' per tile.  WRITE = true: the line starts, at the scanned tile offsets.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_kf_lines(const uint8_t *buf, uint64_t size, uint32_t *tile_cnt,
                                                  const uint64_t *tile_off, uint64_t *ls, uint64_t n_lines) {
  using Scan = rocprim::block_scan<uint32_t, 256>;
  __shared__ typename Scan::storage_type tmp;
  const uint64_t base = (static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x) * 16;
  const uint32_t m = kf_nl_mask(buf, base, size);
  uint32_t       before = 0, total = 0;
  Scan().exclusive_scan(static_cast<uint32_t>(__popc(m)), before, 0u, total, tmp);
  if (!WRITE) {
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
    return;
  }
  uint64_t at = tile_off[blockIdx.x] + before + 1;
  for (uint32_t mm = m; mm; mm &= mm - 1, ++at)
    if (at <= n_lines) ls[at] = base + static_cast<uint32_t>(__ffs(mm));
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ls[0] = 0;
    if (size && (tile_off[gridDim.x] < n_lines)) ls[n_lines] = size + 1; // a last line without '\n'
  }
}

struct KfWiden {
  __device__ uint64_t operator()(uint32_t x) const { return x; }
};

// the FASTQ rules per line; *bad keeps the smallest offending 1-based line
__global__ __launch_bounds__(256) void k_kf_check(const uint8_t *buf, const uint64_t *ls, uint64_t n_lines, kf_ull *bad) {
  const uint64_t l = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (l >= n_lines) return;
  const uint64_t a = ls[l], e = ls[l + 1] - 1;
  const uint32_t m = static_cast<uint32_t>(l & 3);
  bool           wrong = false;
  if (m == 0) wrong = e == a || buf[a] != '@';
  else if (m == 2) wrong = e == a || buf[a] != '+';
  else if (m == 3) wrong = (e - a) != (ls[l - 1] - 1 - ls[l - 2]);
  if (wrong) atomicMin(bad, static_cast<kf_ull>(l + 1));
}

// windows per hash bin
template <class K> __global__ __launch_bounds__(256) void k_kf_bins(KfIn in, kf_ull *bins) {
  __shared__ uint32_t h[KF_BINS];
  for (uint32_t i = threadIdx.x; i < KF_BINS; i += 256) h[i] = 0;
  __syncthreads();
  const uint64_t n = 2 * in.n_pairs, stride = static_cast<uint64_t>(gridDim.x) * 256;
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
  if (t < 2 * in.n_pairs) kf_read(in, t, s, len);
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

// run lengths -> the bins 1..KF_HIGH
__global__ __launch_bounds__(256) void k_kf_hist(const uint32_t *cnt, uint32_t n, kf_ull *hist) {
  __shared__ uint32_t h[KF_LOWBIN];
  for (uint32_t i = threadIdx.x; i < KF_LOWBIN; i += 256) h[i] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t c = cnt[i];
    if (c < KF_LOWBIN) atomicAdd(&h[c], 1u);
    else atomicAdd(&hist[min(c, KF_HIGH)], 1ull);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < KF_LOWBIN; i += 256)
    if (h[i]) atomicAdd(&hist[i], static_cast<kf_ull>(h[i]));
}

// the (key, count) with count >= least.  WRITE = false only counts them (into *cursor).
template <class K, bool WRITE>
__global__ __launch_bounds__(256) void k_kf_select(const K *keys, const uint32_t *cnt, uint64_t n, uint32_t least, K *out_k,
                                                   uint32_t *out_c, uint64_t cap, kf_ull *cursor) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int      lane = threadIdx.x & 63;
  const bool     take = i < n && cnt[i] >= least;
  const uint64_t who = __ballot(take);
  if (!who) return;
  kf_ull at = 0;
  if (lane == __ffsll(static_cast<long long>(who)) - 1) at = atomicAdd(cursor, static_cast<kf_ull>(__popcll(who)));
  at = __shfl(at, __ffsll(static_cast<long long>(who)) - 1);
  if (WRITE && take) {
    const uint64_t slot = at + __popcll(who & ((1ull << lane) - 1));
    if (slot < cap) {
      out_k[slot] = keys[i];
      out_c[slot] = cnt[i];
    }
  }
}

// open addressing over the abundant set: a slot holds an index into the sorted keys
template <class K> __global__ __launch_bounds__(256) void k_kf_table(const K *keys, uint32_t n, uint32_t *slots, uint32_t mask) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (uint32_t h = static_cast<uint32_t>(kf_hash(keys[i])) & mask;; h = (h + 1) & mask)
    if (atomicCAS(&slots[h], KF_EMPTY, i) == KF_EMPTY) return; // (the table has at least 2 n slots)
}

template <class K>
__global__ __launch_bounds__(256) void k_kf_verdict(KfIn in, const K *keys, const uint32_t *slots, uint32_t mask,
                                                    uint8_t *verdict) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= 2 * in.n_pairs) return;
  const uint8_t *s;
  uint64_t       len;
  kf_read(in, t, s, len);
  KfRoll<K> roll(in.k);
  K         key;
  for (uint64_t i = 0; i < len; ++i) {
    if (!roll.step(s[i], key)) continue;
    for (uint32_t h = static_cast<uint32_t>(kf_hash(key)) & mask;; h = (h + 1) & mask) {
      const uint32_t j = slots[h];
      if (j == KF_EMPTY) break;
      if (keys[j] == key) {
        verdict[t >= in.n_pairs ? t - in.n_pairs : t] = 1;
        return;
      }
    }
  }
}

// byte length of every surviving record (0 for a dropped one); entry n_pairs = 0 so that the scan ends on the total
__global__ __launch_bounds__(256) void k_kf_rec_len(const uint64_t *ls, const uint8_t *verdict, uint64_t n_pairs,
                                                    uint64_t *len) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i > n_pairs) return;
  len[i] = (i == n_pairs || verdict[i]) ? 0 : ls[4 * i + 4] - ls[4 * i];
}

// one wavefront per surviving record
__global__ __launch_bounds__(256) void k_kf_copy(const uint8_t *buf, const uint64_t *ls, const uint8_t *verdict,
                                                 const uint64_t *off, uint64_t n_pairs, uint8_t *out, uint64_t cap) {
  const uint64_t r = static_cast<uint64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6);
  if (r >= n_pairs || verdict[r]) return;
  const uint64_t a = ls[4 * r], n = ls[4 * r + 4] - a, o = off[r];
  if (o + n > cap) return;
  for (uint64_t i = threadIdx.x & 63; i < n; i += 64) out[o + i] = buf[a + i];
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_kfctx {
  int         device = 0;
  hipStream_t stream = nullptr;
  char        err[384] = {0};
  uint64_t    err_line = 0;
  int         err_file = 0;
};

struct msgpu_kf_result {
  msgpu_kf_stats        stats{};
  std::vector<uint64_t> hist_a, hist_f, key_hi, key_lo;
  std::vector<uint32_t> count;
  std::vector<uint8_t>  verdict;
  char                 *out[2] = {nullptr, nullptr}; // page-locked
  uint64_t              out_len[2] = {0, 0};
  std::string           report, histo, dump;
  bool                  dump_made = false;
  ~msgpu_kf_result() {
    for (char *p : out)
      if (p) (void)hipHostFree(p);
  }
};

namespace {

int kfail(msgpu_kfctx *c, int code, const char *what, hipError_t e) {
  snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
  return code;
}
#define KHIP(c, expr)                                                                                                  \
  do {                                                                                                                 \
    hipError_t _e = (expr);                                                                                            \
    if (_e != hipSuccess) return kfail((c), _e == hipErrorOutOfMemory ? MSGPU_E_NOMEM : MSGPU_E_HIP, #expr, _e);        \
  } while (0)

struct KfDev { // device memory freed on every way out of msgpu_kf_run
  std::vector<void *> p;
  ~KfDev() {
    for (void *x : p) (void)hipFree(x);
  }
  template <class T> hipError_t get(T **out, size_t count) {
    void      *m = nullptr;
    hipError_t e = hipMalloc(&m, (count ? count : 1) * sizeof(T));
    if (e == hipSuccess) p.push_back(m);
    *out = static_cast<T *>(m);
    return e;
  }
  void drop(void *x) {
    auto it = std::find(p.begin(), p.end(), x);
    if (it != p.end()) p.erase(it);
    (void)hipFree(x);
  }
};

struct KfClock { // device steps by event pairs, summed per step after the run's last synchronisation
  struct Span {
    hipEvent_t a, b;
    float     *acc;
  };
  std::vector<Span> spans;
  hipStream_t       st;
  ~KfClock() {
    for (auto &s : spans) {
      (void)hipEventDestroy(s.a);
      (void)hipEventDestroy(s.b);
    }
  }
  hipError_t begin(float *acc) {
    Span       s{nullptr, nullptr, acc};
    hipError_t e = hipEventCreate(&s.a);
    if (e == hipSuccess) e = hipEventCreate(&s.b);
    if (e == hipSuccess) e = hipEventRecord(s.a, st);
    spans.push_back(s);
    return e;
  }
  hipError_t end() { return hipEventRecord(spans.back().b, st); }
  void       collect() { // (after a synchronisation)
    for (auto &s : spans) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) *s.acc += ms;
      (void)hipEventDestroy(s.a);
      (void)hipEventDestroy(s.b);
    }
    spans.clear();
  }
};

struct KfFile {
  uint8_t  *d = nullptr;
  uint64_t  size = 0, n_lines = 0;
  uint64_t *ls = nullptr;
  bool      open_end = false; // the last line has no '\n'
};

constexpr size_t KF_SLOT = size_t(16) << 20; // page-locked ring: two slots

// mmap -> page-locked ring -> device; the host keeps no copy
int kf_upload(msgpu_kfctx *c, KfDev &D, const char *path, int which, KfFile &f) {
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  struct stat st;
  if (fd < 0 || fstat(fd, &st) != 0) {
    if (fd >= 0) close(fd);
    c->err_file = which;
    snprintf(c->err, sizeof(c->err), "cannot read %s", path);
    return MSGPU_E_IO;
  }
  f.size = static_cast<uint64_t>(st.st_size);
  if (f.size >= (1ull << 40)) {
    close(fd);
    c->err_file = which;
    snprintf(c->err, sizeof(c->err), "%s has %llu bytes; the limit is 2^40 - 1", path, static_cast<kf_ull>(f.size));
    return MSGPU_E_ARG;
  }
  const char *data = nullptr;
  if (f.size) {
    void *m = mmap(nullptr, f.size, PROT_READ, MAP_PRIVATE, fd, 0);
    close(fd);
    if (m == MAP_FAILED) {
      c->err_file = which;
      snprintf(c->err, sizeof(c->err), "cannot map %s", path);
      return MSGPU_E_IO;
    }
    data = static_cast<const char *>(m);
    (void)madvise(m, f.size, MADV_SEQUENTIAL);
  } else close(fd);
  struct Unmap {
    const char *p;
    size_t      n;
    ~Unmap() {
      if (p) munmap(const_cast<char *>(p), n);
    }
  } unmap{data, f.size};
  f.open_end = f.size && data[f.size - 1] != '\n';
  const uint64_t padded = (f.size + 15) / 16 * 16 + 16;
  KHIP(c, D.get(&f.d, padded));
  KHIP(c, hipMemsetAsync(f.d + f.size, '\n', padded - f.size, c->stream)); // (byte `size` closes a last open line)
  char      *ring = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  KHIP(c, hipHostMalloc(reinterpret_cast<void **>(&ring), 2 * KF_SLOT, hipHostMallocDefault));
  struct FreeRing {
    char       *r;
    hipEvent_t *e;
    ~FreeRing() {
      (void)hipHostFree(r);
      for (int i = 0; i < 2; ++i)
        if (e[i]) (void)hipEventDestroy(e[i]);
    }
  } free_ring{ring, ev};
  for (auto &e : ev) KHIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  int slot = 0;
  for (uint64_t at = 0; at < f.size; at += KF_SLOT, slot ^= 1) {
    const size_t n = static_cast<size_t>(std::min<uint64_t>(KF_SLOT, f.size - at));
    KHIP(c, hipEventSynchronize(ev[slot])); // (a fresh event is complete)
    memcpy(ring + slot * KF_SLOT, data + at, n);
    KHIP(c, hipMemcpyAsync(f.d + at, ring + slot * KF_SLOT, n, hipMemcpyHostToDevice, c->stream));
    KHIP(c, hipEventRecord(ev[slot], c->stream));
  }
  KHIP(c, hipStreamSynchronize(c->stream));
  return MSGPU_OK;
}

// the line starts of a file on the device
int kf_lines(msgpu_kfctx *c, KfDev &D, KfFile &f) {
  hipStream_t    st = c->stream;
  const uint32_t tiles = static_cast<uint32_t>((f.size + KF_TILE - 1) / KF_TILE);
  uint32_t      *d_cnt;
  uint64_t      *d_off;
  KHIP(c, D.get(&d_cnt, tiles + 1));
  KHIP(c, D.get(&d_off, tiles + 1));
  KHIP(c, hipMemsetAsync(d_cnt, 0, (tiles + 1) * sizeof(uint32_t), st));
  if (tiles) hipLaunchKernelGGL(k_kf_lines<false>, dim3(tiles), dim3(256), 0, st, f.d, f.size, d_cnt, nullptr, nullptr, 0);
  KHIP(c, hipGetLastError());
  auto   in = rocprim::make_transform_iterator(d_cnt, KfWiden());
  size_t need = 0;
  KHIP(c, rocprim::exclusive_scan(nullptr, need, in, d_off, uint64_t(0), tiles + 1, rocprim::plus<uint64_t>(), st));
  uint8_t *tmp;
  KHIP(c, D.get(&tmp, need));
  KHIP(c, rocprim::exclusive_scan(tmp, need, in, d_off, uint64_t(0), tiles + 1, rocprim::plus<uint64_t>(), st));
  uint64_t nl = 0;
  KHIP(c, hipMemcpyAsync(&nl, d_off + tiles, 8, hipMemcpyDeviceToHost, st));
  KHIP(c, hipStreamSynchronize(st));
  f.n_lines = nl + (f.open_end ? 1 : 0);
  KHIP(c, D.get(&f.ls, f.n_lines + 1));
  KHIP(c, hipMemsetAsync(f.ls, 0, 8, st)); // (an empty file launches nothing)
  if (tiles) hipLaunchKernelGGL(k_kf_lines<true>, dim3(tiles), dim3(256), 0, st, f.d, f.size, nullptr, d_off, f.ls, f.n_lines);
  KHIP(c, hipGetLastError());
  KHIP(c, hipStreamSynchronize(st));
  D.drop(tmp);
  D.drop(d_cnt);
  D.drop(d_off);
  return MSGPU_OK;
}

int kf_format_error(msgpu_kfctx *c, int which, uint64_t line, const char *what) {
  c->err_file = which;
  c->err_line = line;
  snprintf(c->err, sizeof(c->err), "file %d line %llu: %s", which, static_cast<kf_ull>(line), what);
  return MSGPU_E_FORMAT;
}

template <class K> void kf_split(const K *keys, size_t n, std::vector<uint64_t> &hi, std::vector<uint64_t> &lo);
template <> void kf_split<uint64_t>(const uint64_t *keys, size_t n, std::vector<uint64_t> &hi, std::vector<uint64_t> &lo) {
  hi.assign(n, 0);
  lo.assign(keys, keys + n);
}
template <> void kf_split<kf_u128>(const kf_u128 *keys, size_t n, std::vector<uint64_t> &hi, std::vector<uint64_t> &lo) {
  hi.resize(n);
  lo.resize(n);
  for (size_t i = 0; i < n; ++i) {
    hi[i] = static_cast<uint64_t>(keys[i] >> 64);
    lo[i] = static_cast<uint64_t>(keys[i]);
  }
}

// everything behind the format check, for one key width
template <class K>
int kf_stage(msgpu_kfctx *c, KfDev &D, const KfFile *F, uint64_t n_pairs, int k, uint64_t budget,
             msgpu_kf_result *res) {
  msgpu_kf_stats &S = res->stats;
  hipStream_t     st = c->stream;
  KfClock         clock;
  clock.st = st;
  const KfIn     in{{F[0].d, F[1].d}, {F[0].ls, F[1].ls}, n_pairs, k};
  const uint64_t n_reads = 2 * n_pairs;
  const uint32_t read_grid = static_cast<uint32_t>((n_reads + 255) / 256);

  // ---- windows per hash bin, the partitions
  kf_ull *d_bins, *d_hist, *d_cur;
  KHIP(c, D.get(&d_bins, KF_BINS));
  KHIP(c, D.get(&d_hist, KF_HIGH + 1));
  KHIP(c, D.get(&d_cur, 1));
  KHIP(c, hipMemsetAsync(d_bins, 0, KF_BINS * 8, st));
  KHIP(c, hipMemsetAsync(d_hist, 0, (KF_HIGH + 1) * 8, st));
  KHIP(c, clock.begin(&S.bins_ms));
  if (n_reads) hipLaunchKernelGGL(k_kf_bins<K>, dim3(std::min<uint32_t>(read_grid, 4096)), dim3(256), 0, st, in, d_bins);
  KHIP(c, hipGetLastError());
  KHIP(c, clock.end());
  std::vector<kf_ull> bins(KF_BINS);
  KHIP(c, hipMemcpyAsync(bins.data(), d_bins, KF_BINS * 8, hipMemcpyDeviceToHost, st));
  KHIP(c, hipStreamSynchronize(st));
  std::vector<uint64_t> pre(KF_BINS + 1, 0);
  for (uint32_t b = 0; b < KF_BINS; ++b) pre[b + 1] = pre[b] + bins[b];
  S.n_windows = pre[KF_BINS];
  size_t free_b = 0, total_b = 0;
  KHIP(c, hipMemGetInfo(&free_b, &total_b));
  const uint64_t out_bytes = F[0].size + F[1].size + 2; // the outputs are no larger than the inputs
  const uint64_t per_key = 2 * sizeof(K) + 4;           // two key buffers and the run lengths
  if (!budget) budget = free_b > out_bytes ? (free_b - out_bytes) / 2 : 0;
  auto first_bin = [](uint32_t p, uint32_t P) { return static_cast<uint32_t>((uint64_t(p) * KF_BINS + P - 1) / P); };
  uint32_t P = 0;
  uint64_t largest = 0;
  for (uint32_t q = 1; q <= KF_BINS && !P; ++q) {
    uint64_t m = 0;
    for (uint32_t p = 0; p < q; ++p) m = std::max(m, pre[first_bin(p + 1, q)] - pre[first_bin(p, q)]);
    if (m < (1ull << 31) && m * per_key <= budget) {
      P       = q;
      largest = m;
    }
  }
  if (!P || largest * per_key + out_bytes > free_b) {
    snprintf(c->err, sizeof(c->err),
             "%llu windows of %zu-byte keys need %llu bytes per window in partition buffers (budget %llu bytes, %u hash "
             "bins) next to %llu bytes of output; %zu bytes of device memory are free",
             static_cast<kf_ull>(S.n_windows), sizeof(K), static_cast<kf_ull>(per_key), static_cast<kf_ull>(budget),
             KF_BINS, static_cast<kf_ull>(out_bytes), free_b);
    return MSGPU_E_NOMEM;
  }
  S.n_partitions = P;
  S.largest_partition = largest;

  // ---- count: per partition extract, sort, run lengths, histogram, candidates
  K        *d_a, *d_b;
  uint32_t *d_rl, *d_nruns;
  KHIP(c, D.get(&d_a, largest));
  KHIP(c, D.get(&d_b, largest));
  KHIP(c, D.get(&d_rl, largest));
  KHIP(c, D.get(&d_nruns, 1));
  size_t need_sort = 0, need_rle = 0;
  {
    rocprim::double_buffer<K> db(d_a, d_b);
    KHIP(c, rocprim::radix_sort_keys(nullptr, need_sort, db, largest, 0, 2 * k, st));
    KHIP(c, rocprim::run_length_encode(nullptr, need_rle, d_a, static_cast<unsigned int>(largest), d_b, d_rl, d_nruns, st));
  }
  const size_t tmp_bytes = std::max(need_sort, need_rle);
  uint8_t     *d_tmp;
  KHIP(c, D.get(&d_tmp, tmp_bytes));
  struct Chunk {
    K        *k;
    uint32_t *c;
    uint64_t  n;
  };
  std::vector<Chunk> chunks;
  for (uint32_t p = 0; p < P; ++p) {
    const uint64_t n = pre[first_bin(p + 1, P)] - pre[first_bin(p, P)];
    if (!n) continue;
    KHIP(c, hipMemsetAsync(d_cur, 0, 8, st));
    KHIP(c, clock.begin(&S.extract_ms));
    hipLaunchKernelGGL(k_kf_extract<K>, dim3(read_grid), dim3(256), 0, st, in, P, p, d_a, n, d_cur);
    KHIP(c, hipGetLastError());
    KHIP(c, clock.end());
    rocprim::double_buffer<K> db(d_a, d_b);
    size_t                    tb = tmp_bytes;
    KHIP(c, clock.begin(&S.sort_ms));
    KHIP(c, rocprim::radix_sort_keys(d_tmp, tb, db, n, 0, 2 * k, st));
    KHIP(c, clock.end());
    K *sorted = db.current(), *uniq = db.alternate();
    tb = tmp_bytes;
    KHIP(c, clock.begin(&S.runs_ms));
    KHIP(c, rocprim::run_length_encode(d_tmp, tb, sorted, static_cast<unsigned int>(n), uniq, d_rl, d_nruns, st));
    KHIP(c, clock.end());
    uint32_t runs = 0;
    kf_ull   written = 0;
    KHIP(c, hipMemcpyAsync(&runs, d_nruns, 4, hipMemcpyDeviceToHost, st));
    KHIP(c, hipMemcpyAsync(&written, d_cur, 8, hipMemcpyDeviceToHost, st));
    KHIP(c, hipStreamSynchronize(st));
    if (written != n) { // the two window passes disagree: never seen; a result built on it would be wrong
      snprintf(c->err, sizeof(c->err), "partition %u: %llu keys extracted where %llu were counted", p, written,
               static_cast<kf_ull>(n));
      return MSGPU_E_STATE;
    }
    S.n_distinct += runs;
    const uint32_t run_grid = (runs + 255) / 256;
    KHIP(c, hipMemsetAsync(d_cur, 0, 8, st));
    KHIP(c, clock.begin(&S.hist_ms));
    hipLaunchKernelGGL(k_kf_hist, dim3(std::min<uint32_t>(run_grid, 2048)), dim3(256), 0, st, d_rl, runs, d_hist);
    KHIP(c, hipGetLastError());
    KHIP(c, clock.end());
    KHIP(c, clock.begin(&S.select_ms));
    hipLaunchKernelGGL((k_kf_select<K, false>), dim3(run_grid), dim3(256), 0, st, uniq, d_rl, runs, KF_KEEP, nullptr, nullptr,
                       0, d_cur);
    KHIP(c, hipGetLastError());
    kf_ull kept = 0;
    KHIP(c, hipMemcpyAsync(&kept, d_cur, 8, hipMemcpyDeviceToHost, st));
    KHIP(c, hipStreamSynchronize(st));
    if (kept) {
      Chunk ch{nullptr, nullptr, kept};
      KHIP(c, D.get(&ch.k, kept));
      KHIP(c, D.get(&ch.c, kept));
      KHIP(c, hipMemsetAsync(d_cur, 0, 8, st));
      hipLaunchKernelGGL((k_kf_select<K, true>), dim3(run_grid), dim3(256), 0, st, uniq, d_rl, runs, KF_KEEP, ch.k, ch.c, kept,
                         d_cur);
      KHIP(c, hipGetLastError());
      chunks.push_back(ch);
      S.n_candidates += kept;
    }
    KHIP(c, clock.end());
  }
  std::vector<kf_ull> hist(KF_HIGH + 1);
  KHIP(c, hipMemcpyAsync(hist.data(), d_hist, (KF_HIGH + 1) * 8, hipMemcpyDeviceToHost, st));
  KHIP(c, hipStreamSynchronize(st));
  D.drop(d_a);
  D.drop(d_b);
  D.drop(d_rl);
  D.drop(d_tmp);

  // ---- threshold (host: at most 10001 rows)
  for (uint32_t a = 1; a <= KF_HIGH; ++a)
    if (hist[a]) {
      res->hist_a.push_back(a);
      res->hist_f.push_back(hist[a]);
    }
  S.n_hist_rows = res->hist_a.size();
  int rc = msgpu_kf_threshold(res->hist_a.data(), res->hist_f.data(), res->hist_a.size(), &S.q1, &S.q3, &S.upper);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "degenerate histogram (%llu rows, q1 %lld, q3 %lld): no abundance threshold",
             static_cast<kf_ull>(S.n_hist_rows), static_cast<long long>(S.q1), static_cast<long long>(S.q3));
    return rc;
  }

  // ---- the abundant set, ascending, and the table over it
  const uint32_t least = static_cast<uint32_t>(std::min<int64_t>(S.upper, 0xffffffffll));
  KHIP(c, hipMemsetAsync(d_cur, 0, 8, st));
  KHIP(c, clock.begin(&S.select_ms));
  for (const Chunk &ch : chunks)
    hipLaunchKernelGGL((k_kf_select<K, false>), dim3(static_cast<uint32_t>((ch.n + 255) / 256)), dim3(256), 0, st, ch.k, ch.c,
                       ch.n, least, nullptr, nullptr, 0, d_cur);
  KHIP(c, hipGetLastError());
  kf_ull n_ab = 0;
  KHIP(c, hipMemcpyAsync(&n_ab, d_cur, 8, hipMemcpyDeviceToHost, st));
  KHIP(c, hipStreamSynchronize(st));
  if (n_ab >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "%llu abundant k-mers; the limit is 2^31 - 1", n_ab);
    return MSGPU_E_ARG;
  }
  S.n_abundant = n_ab;
  K        *d_abk = nullptr, *d_abk_in;
  uint32_t *d_abc = nullptr, *d_abc_in;
  KHIP(c, D.get(&d_abk, n_ab));
  KHIP(c, D.get(&d_abc, n_ab));
  if (n_ab) {
    KHIP(c, D.get(&d_abk_in, n_ab));
    KHIP(c, D.get(&d_abc_in, n_ab));
    KHIP(c, hipMemsetAsync(d_cur, 0, 8, st));
    for (const Chunk &ch : chunks)
      hipLaunchKernelGGL((k_kf_select<K, true>), dim3(static_cast<uint32_t>((ch.n + 255) / 256)), dim3(256), 0, st, ch.k,
                         ch.c, ch.n, least, d_abk_in, d_abc_in, n_ab, d_cur);
    KHIP(c, hipGetLastError());
    size_t need = 0;
    KHIP(c, rocprim::radix_sort_pairs(nullptr, need, d_abk_in, d_abk, d_abc_in, d_abc, n_ab, 0, 2 * k, st));
    uint8_t *tmp;
    KHIP(c, D.get(&tmp, need));
    KHIP(c, rocprim::radix_sort_pairs(tmp, need, d_abk_in, d_abk, d_abc_in, d_abc, n_ab, 0, 2 * k, st));
    KHIP(c, hipStreamSynchronize(st));
    D.drop(tmp);
    D.drop(d_abk_in);
    D.drop(d_abc_in);
  }
  for (const Chunk &ch : chunks) {
    D.drop(ch.k);
    D.drop(ch.c);
  }
  uint32_t slots_n = 64;
  while (slots_n < 2 * n_ab) slots_n <<= 1;
  uint32_t *d_slots;
  KHIP(c, D.get(&d_slots, slots_n));
  KHIP(c, hipMemsetAsync(d_slots, 0xff, slots_n * 4ull, st));
  if (n_ab)
    hipLaunchKernelGGL(k_kf_table<K>, dim3(static_cast<uint32_t>((n_ab + 255) / 256)), dim3(256), 0, st, d_abk,
                       static_cast<uint32_t>(n_ab), d_slots, slots_n - 1);
  KHIP(c, hipGetLastError());
  KHIP(c, clock.end());

  // ---- verdicts
  uint8_t *d_verdict;
  KHIP(c, D.get(&d_verdict, n_pairs));
  KHIP(c, hipMemsetAsync(d_verdict, 0, n_pairs ? n_pairs : 1, st));
  KHIP(c, clock.begin(&S.verdict_ms));
  if (n_reads)
    hipLaunchKernelGGL(k_kf_verdict<K>, dim3(read_grid), dim3(256), 0, st, in, d_abk, d_slots, slots_n - 1, d_verdict);
  KHIP(c, hipGetLastError());
  KHIP(c, clock.end());

  // ---- output: lengths, scan, copy, per file
  uint64_t *d_len, *d_off;
  KHIP(c, D.get(&d_len, n_pairs + 1));
  KHIP(c, D.get(&d_off, n_pairs + 1));
  size_t need = 0;
  KHIP(c, rocprim::exclusive_scan(nullptr, need, d_len, d_off, uint64_t(0), n_pairs + 1, rocprim::plus<uint64_t>(), st));
  uint8_t *d_scan;
  KHIP(c, D.get(&d_scan, need));
  uint8_t *d_out[2];
  for (int f = 0; f < 2; ++f) {
    KHIP(c, clock.begin(&S.output_ms));
    hipLaunchKernelGGL(k_kf_rec_len, dim3(static_cast<uint32_t>((n_pairs + 256) / 256)), dim3(256), 0, st, F[f].ls, d_verdict,
                       n_pairs, d_len);
    KHIP(c, hipGetLastError());
    KHIP(c, rocprim::exclusive_scan(d_scan, need, d_len, d_off, uint64_t(0), n_pairs + 1, rocprim::plus<uint64_t>(), st));
    KHIP(c, hipMemcpyAsync(&res->out_len[f], d_off + n_pairs, 8, hipMemcpyDeviceToHost, st));
    KHIP(c, hipStreamSynchronize(st));
    const uint64_t n = res->out_len[f];
    KHIP(c, D.get(&d_out[f], n));
    if (n)
      hipLaunchKernelGGL(k_kf_copy, dim3(static_cast<uint32_t>((n_pairs + 3) / 4)), dim3(256), 0, st, F[f].d, F[f].ls,
                         d_verdict, d_off, n_pairs, d_out[f], n);
    KHIP(c, hipGetLastError());
    KHIP(c, clock.end());
  }
  KHIP(c, clock.begin(&S.copy_ms));
  for (int f = 0; f < 2; ++f)
    if (res->out_len[f]) {
      KHIP(c, hipHostMalloc(reinterpret_cast<void **>(&res->out[f]), res->out_len[f], hipHostMallocDefault));
      KHIP(c, hipMemcpyAsync(res->out[f], d_out[f], res->out_len[f], hipMemcpyDeviceToHost, st));
    }
  std::vector<K> abk;
  try {
    res->verdict.resize(n_pairs);
    res->count.resize(n_ab);
    abk.resize(n_ab);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (n_pairs) KHIP(c, hipMemcpyAsync(res->verdict.data(), d_verdict, n_pairs, hipMemcpyDeviceToHost, st));
  if (n_ab) {
    KHIP(c, hipMemcpyAsync(res->count.data(), d_abc, n_ab * 4, hipMemcpyDeviceToHost, st));
    KHIP(c, hipMemcpyAsync(abk.data(), d_abk, n_ab * sizeof(K), hipMemcpyDeviceToHost, st));
  }
  KHIP(c, clock.end());
  KHIP(c, hipStreamSynchronize(st));
  clock.collect();
  try {
    kf_split<K>(abk.data(), abk.size(), res->key_hi, res->key_lo);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  for (uint64_t i = 0; i < n_pairs; ++i) S.n_pairs_out += res->verdict[i] ? 0 : 1;
  return MSGPU_OK;
}

} // namespace

extern "C" {

// setAbundanceThresholdFromHisto.py on the rows, `total` as the pipeline's awk line sums it (every row but a = 1).
// nearbyint in the default rounding mode is Python's round() here: (total + 1) * 0.25 is exact below 2^51.
int msgpu_kf_threshold(const uint64_t *abundance, const uint64_t *frequency, size_t n, int64_t *q1, int64_t *q3,
                       int64_t *upper) {
  if (!q1 || !q3 || !upper || (n && (!abundance || !frequency))) return MSGPU_E_ARG;
  *q1 = *q3 = *upper = 0;
  uint64_t total = 0;
  bool     any = false;
  for (size_t i = 0; i < n; ++i)
    if (abundance[i] != 1) {
      any = true;
      total += frequency[i];
    }
  if (!any) return MSGPU_E_LAYOUT; // awk prints an empty sum and the script dies on it
  if (total >= (1ull << 51)) return MSGPU_E_ARG;
  const double   t1 = static_cast<double>(total + 1);
  const uint64_t q1_th = static_cast<uint64_t>(std::nearbyint(t1 * 0.25)), q3_th = static_cast<uint64_t>(std::nearbyint(t1 * 0.75));
  uint64_t       cur = 0;
  for (size_t i = 0; i < n; ++i) {
    if (abundance[i] <= 1) continue;
    cur += frequency[i];
    if (*q1 == 0 && cur >= q1_th) *q1 = static_cast<int64_t>(abundance[i]);
    else if (*q3 == 0 && cur >= q3_th) { // (the elif: the row that set q1 never sets q3)
      *q3 = static_cast<int64_t>(abundance[i]);
      break;
    }
  }
  *upper = *q3 + 2 * (*q3 - *q1);
  return (*q3 == 0 || *upper <= 0) ? MSGPU_E_LAYOUT : MSGPU_OK;
}

int msgpu_kf_create(int device, msgpu_kfctx **out) {
  if (!out) return MSGPU_E_ARG;
  *out     = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MSGPU_E_NODEVICE;
  if (device < 0 || device >= ndev) return MSGPU_E_ARG;
  auto *c = new (std::nothrow) msgpu_kfctx();
  if (!c) return MSGPU_E_NOMEM;
  c->device = device;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    msgpu_kf_destroy(c);
    return MSGPU_E_HIP;
  }
  *out = c;
  return MSGPU_OK;
}

void msgpu_kf_destroy(msgpu_kfctx *c) {
  if (!c) return;
  if (c->stream) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  delete c;
}

const char *msgpu_kf_last_error(const msgpu_kfctx *c) { return c ? c->err : "null context"; }
uint64_t    msgpu_kf_error_line(const msgpu_kfctx *c) { return c ? c->err_line : 0; }
int         msgpu_kf_error_file(const msgpu_kfctx *c) { return c ? c->err_file : 0; }

int msgpu_kf_run(msgpu_kfctx *c, int k, const char *path_a, const char *path_b, uint32_t flags, uint64_t budget_bytes,
                 msgpu_kf_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out        = nullptr;
  c->err[0]   = 0;
  c->err_line = 0;
  c->err_file = 0;
  if (!path_a || !path_b || flags) return MSGPU_E_ARG;
  if (k < 1 || k > 64) {
    snprintf(c->err, sizeof(c->err), "k = %d is outside 1..64", k);
    return MSGPU_E_ARG;
  }
  const auto w0 = std::chrono::steady_clock::now();
  auto       since = [](std::chrono::steady_clock::time_point a) {
    return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - a).count();
  };
  KHIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_kf_result> res;
  try {
    res.reset(new msgpu_kf_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  msgpu_kf_stats &S = res->stats;
  S.k               = static_cast<uint32_t>(k);
  KfDev       D;
  KfFile      F[2];
  const char *paths[2] = {path_a, path_b};
  for (int f = 0; f < 2; ++f) {
    const int rc = kf_upload(c, D, paths[f], f, F[f]);
    if (rc != MSGPU_OK) return rc;
    S.bytes_in[f] = F[f].size;
  }
  S.load_ms = since(w0);

  // ---- records: line starts, the format rules
  const auto r0 = std::chrono::steady_clock::now();
  kf_ull    *d_bad;
  KHIP(c, D.get(&d_bad, 1));
  for (int f = 0; f < 2; ++f) {
    int rc = kf_lines(c, D, F[f]);
    if (rc != MSGPU_OK) return rc;
    kf_ull bad = ~0ull;
    KHIP(c, hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, c->stream));
    if (F[f].n_lines)
      hipLaunchKernelGGL(k_kf_check, dim3(static_cast<uint32_t>((F[f].n_lines + 255) / 256)), dim3(256), 0, c->stream, F[f].d,
                         F[f].ls, F[f].n_lines, d_bad);
    KHIP(c, hipGetLastError());
    KHIP(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    KHIP(c, hipStreamSynchronize(c->stream));
    if (bad != ~0ull) {
      const char *what[4] = {"a record's first line must start with '@'", "", "a record's third line must start with '+'",
                             "the quality line and the sequence line differ in length"};
      return kf_format_error(c, f, bad, what[(bad - 1) & 3]);
    }
    if (F[f].n_lines & 3) return kf_format_error(c, f, F[f].n_lines + 1, "the file ends inside a record");
    if ((F[f].n_lines >> 2) >= (1ull << 32)) {
      c->err_file = f;
      snprintf(c->err, sizeof(c->err), "file %d has %llu records; the limit is 2^32 - 1", f, static_cast<kf_ull>(F[f].n_lines >> 2));
      return MSGPU_E_ARG;
    }
  }
  if (F[0].n_lines != F[1].n_lines) {
    const int f = F[0].n_lines < F[1].n_lines ? 0 : 1;
    return kf_format_error(c, f, F[f].n_lines + 1, "the two files differ in their number of records");
  }
  const uint64_t n_pairs = F[0].n_lines >> 2;
  S.n_pairs    = n_pairs;
  S.records_ms = since(r0);

  const int rc = k <= 32 ? kf_stage<uint64_t>(c, D, F, n_pairs, k, budget_bytes, res.get())
                         : kf_stage<kf_u128>(c, D, F, n_pairs, k, budget_bytes, res.get());
  if (rc != MSGPU_OK) return rc;
  char buf[96];
  snprintf(buf, sizeof(buf), "abundance threshold for k-mer filtering:  %lld\n", static_cast<long long>(S.upper));
  try {
    res->report = buf;
    for (size_t i = 0; i < res->hist_a.size(); ++i) {
      snprintf(buf, sizeof(buf), "%llu %llu\n", static_cast<kf_ull>(res->hist_a[i]), static_cast<kf_ull>(res->hist_f[i]));
      res->histo += buf;
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  S.bytes_out[0] = res->out_len[0];
  S.bytes_out[1] = res->out_len[1];
  S.wall_ms      = since(w0);
  *out           = res.release();
  return MSGPU_OK;
}

int msgpu_kf_result_stats(const msgpu_kf_result *r, msgpu_kf_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

int msgpu_kf_result_histogram(const msgpu_kf_result *r, const uint64_t **abundance, const uint64_t **frequency, uint64_t *n) {
  if (!r || !abundance || !frequency || !n) return MSGPU_E_ARG;
  *abundance = r->hist_a.data();
  *frequency = r->hist_f.data();
  *n         = r->hist_a.size();
  return MSGPU_OK;
}

int msgpu_kf_result_abundant(const msgpu_kf_result *r, const uint64_t **key_hi, const uint64_t **key_lo, const uint32_t **count,
                             uint64_t *n) {
  if (!r || !key_hi || !key_lo || !count || !n) return MSGPU_E_ARG;
  *key_hi = r->key_hi.data();
  *key_lo = r->key_lo.data();
  *count  = r->count.data();
  *n      = r->count.size();
  return MSGPU_OK;
}

int msgpu_kf_result_verdicts(const msgpu_kf_result *r, const uint8_t **verdict, uint64_t *n) {
  if (!r || !verdict || !n) return MSGPU_E_ARG;
  *verdict = r->verdict.data();
  *n       = r->verdict.size();
  return MSGPU_OK;
}

const char *msgpu_kf_result_text(msgpu_kf_result *r, int which, uint64_t *len) {
  if (len) *len = 0;
  if (!r) return "";
  const char *p = "";
  uint64_t    n = 0;
  if (which == MSGPU_KF_TEXT_OUT_A || which == MSGPU_KF_TEXT_OUT_B) {
    p = r->out[which] ? r->out[which] : "";
    n = r->out_len[which];
  } else if (which == MSGPU_KF_TEXT_REPORT) {
    p = r->report.data();
    n = r->report.size();
  } else if (which == MSGPU_KF_TEXT_HISTO) {
    p = r->histo.data();
    n = r->histo.size();
  } else if (which == MSGPU_KF_TEXT_KMERS) {
    if (!r->dump_made) { // jellyfish dump's records, ">count\nKMER\n", ascending
      const int k = static_cast<int>(r->stats.k);
      char      buf[16];
      try {
        for (size_t i = 0; i < r->count.size(); ++i) {
          snprintf(buf, sizeof(buf), ">%u\n", r->count[i]);
          r->dump += buf;
          for (int j = k - 1; j >= 0; --j) {
            const uint64_t w = j >= 32 ? r->key_hi[i] >> (2 * (j - 32)) : r->key_lo[i] >> (2 * j);
            r->dump += "ACGT"[w & 3];
          }
          r->dump += '\n';
        }
      } catch (std::bad_alloc const &) { return ""; }
      r->dump_made = true;
    }
    p = r->dump.data();
    n = r->dump.size();
  }
  if (len) *len = n;
  return p;
}

void msgpu_kf_result_free(msgpu_kf_result *r) {
  if (r) delete r;
}

} // extern "C"
