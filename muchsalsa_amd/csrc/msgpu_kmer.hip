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
// What the short-read unitig assembly (msgpu_unitig.hip) uses as well -- the rolling window, the hash, the partitions, k_kf_bins /
// k_kf_extract / k_kf_select / k_kf_table, the partitioned count and the sorted gather -- is defined in msgpu_kmer_shared.h;
// the upload ring, the line starts and the FASTQ check are defined here and declared there.
//
// Kernel rules: vector stores and vector atomics only; no inline asm.
#include <hip/hip_runtime.h>
#include <rocprim/block/block_scan.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <memory>
#include <new>
#include <string>

#include "msgpu_kmer_shared.h"

namespace msgpu {

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

template <class K>
__global__ __launch_bounds__(256) void k_kf_verdict(KfIn in, const K *keys, const uint32_t *slots, uint32_t mask,
                                                    uint8_t *verdict) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= in.n_reads) return;
  const uint8_t *s;
  uint64_t       len;
  kf_read(in, t, s, len);
  KfRoll<K> roll(in.k);
  K         key;
  for (uint64_t i = 0; i < len; ++i) {
    if (!roll.step(s[i], key)) continue;
    if (kf_find(keys, slots, mask, key) != KF_EMPTY) {
      verdict[t >= in.n_first ? t - in.n_first : t] = 1;
      return;
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

// ---- host side, shared with msgpu_unitig.hip (msgpu_kmer_shared.h) ---------------------------------------------------

constexpr size_t KF_SLOT = size_t(16) << 20; // page-locked ring: two slots

// mmap -> page-locked ring -> device; the host keeps no copy
int kf_upload(StageCtx *c, DevArena &D, const char *path, int which, KfFile &f) {
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
  STAGE_HIP(c, D.get(&f.d, padded));
  STAGE_HIP(c, hipMemsetAsync(f.d + f.size, '\n', padded - f.size, c->stream)); // (byte `size` closes a last open line)
  char     *ring = nullptr;
  EventHold ev[2];
  STAGE_HIP(c, hipHostMalloc(reinterpret_cast<void **>(&ring), 2 * KF_SLOT, hipHostMallocDefault));
  struct FreeRing {
    char *r;
    ~FreeRing() { (void)hipHostFree(r); }
  } free_ring{ring};
  for (auto &e : ev) STAGE_HIP(c, e.create(hipEventDisableTiming));
  int slot = 0;
  for (uint64_t at = 0; at < f.size; at += KF_SLOT, slot ^= 1) {
    const size_t n = static_cast<size_t>(std::min<uint64_t>(KF_SLOT, f.size - at));
    STAGE_HIP(c, hipEventSynchronize(ev[slot])); // (a fresh event is complete)
    memcpy(ring + slot * KF_SLOT, data + at, n);
    STAGE_HIP(c, hipMemcpyAsync(f.d + at, ring + slot * KF_SLOT, n, hipMemcpyHostToDevice, c->stream));
    STAGE_HIP(c, hipEventRecord(ev[slot], c->stream));
  }
  STAGE_HIP(c, hipStreamSynchronize(c->stream));
  return MSGPU_OK;
}

// the line starts of a file on the device
int kf_lines(StageCtx *c, DevArena &D, KfFile &f) {
  hipStream_t    st = c->stream;
  const uint32_t tiles = static_cast<uint32_t>((f.size + KF_TILE - 1) / KF_TILE);
  uint32_t      *d_cnt;
  uint64_t      *d_off;
  STAGE_HIP(c, D.get(&d_cnt, tiles + 1));
  STAGE_HIP(c, D.get(&d_off, tiles + 1));
  STAGE_HIP(c, hipMemsetAsync(d_cnt, 0, (tiles + 1) * sizeof(uint32_t), st));
  if (tiles) hipLaunchKernelGGL(k_kf_lines<false>, dim3(tiles), dim3(256), 0, st, f.d, f.size, d_cnt, nullptr, nullptr, 0);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan(D, st, rocprim::make_transform_iterator(d_cnt, KfWiden()), d_off, tiles + 1));
  uint64_t nl = 0;
  STAGE_HIP(c, hipMemcpyAsync(&nl, d_off + tiles, 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));
  f.n_lines = nl + (f.open_end ? 1 : 0);
  STAGE_HIP(c, D.get(&f.ls, f.n_lines + 1));
  STAGE_HIP(c, hipMemsetAsync(f.ls, 0, 8, st)); // (an empty file launches nothing)
  if (tiles) hipLaunchKernelGGL(k_kf_lines<true>, dim3(tiles), dim3(256), 0, st, f.d, f.size, nullptr, d_off, f.ls, f.n_lines);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, hipStreamSynchronize(st));
  D.drop(d_cnt);
  D.drop(d_off);
  return MSGPU_OK;
}

int kf_format_error(StageCtx *c, int which, uint64_t line, const char *what) {
  c->err_file = which;
  c->err_line = line;
  snprintf(c->err, sizeof(c->err), "file %d line %llu: %s", which, static_cast<kf_ull>(line), what);
  return MSGPU_E_FORMAT;
}

// the line starts of every file and the FASTQ rules, file 0 first
int kf_records(StageCtx *c, DevArena &D, KfFile *F, int n_files) {
  kf_ull *d_bad;
  STAGE_HIP(c, D.get(&d_bad, 1));
  for (int f = 0; f < n_files; ++f) {
    int rc = kf_lines(c, D, F[f]);
    if (rc != MSGPU_OK) return rc;
    kf_ull bad = ~0ull;
    STAGE_HIP(c, hipMemcpyAsync(d_bad, &bad, 8, hipMemcpyHostToDevice, c->stream));
    if (F[f].n_lines)
      hipLaunchKernelGGL(k_kf_check, dim3(grid256(F[f].n_lines)), dim3(256), 0, c->stream, F[f].d,
                         F[f].ls, F[f].n_lines, d_bad);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, hipMemcpyAsync(&bad, d_bad, 8, hipMemcpyDeviceToHost, c->stream));
    STAGE_HIP(c, hipStreamSynchronize(c->stream));
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
  return MSGPU_OK;
}

int kf_pair_open(StageCtx *c, const char *path_a, const char *path_b, msgpu_pair **out) {
  std::unique_ptr<msgpu_pair> p;
  try {
    p.reset(new msgpu_pair());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  p->device  = c->device;
  p->n_files = path_b ? 2 : 1;
  const StageTimer load;
  const char      *paths[2] = {path_a, path_b};
  for (int f = 0; f < p->n_files; ++f) {
    const int rc = kf_upload(c, p->D, paths[f], f, p->F[f]);
    if (rc != MSGPU_OK) return rc;
  }
  p->load_ms = load.ms();
  const StageTimer records;
  const int        rc = kf_records(c, p->D, p->F, p->n_files);
  if (rc != MSGPU_OK) return rc;
  if (p->n_files == 1) {
    p->F[1].d  = p->F[0].d;
    p->F[1].ls = p->F[0].ls;
  }
  p->records_ms = records.ms();
  if (stage_verify(c, p->D) != MSGPU_OK) return MSGPU_E_HIP;
  *out          = p.release();
  return MSGPU_OK;
}

void kf_pair_close(msgpu_pair *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  char err[256]; // (nobody takes an error here: one line)
  if (p->D.verify(nullptr, err, sizeof(err)) != hipSuccess) fprintf(stderr, "msgpu_pair_close: %s\n", err);
  delete p;
}

} // namespace msgpu

using namespace msgpu;

struct msgpu_kfctx : msgpu::StageCtx {};

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

// everything behind the format check, for one key width
template <class K>
int kf_stage(msgpu_kfctx *c, DevArena &D, const KfFile *F, uint64_t n_pairs, int k, uint64_t budget,
             msgpu_kf_result *res) {
  msgpu_kf_stats &S = res->stats;
  hipStream_t     st = c->stream;
  StageClock      clock(st);
  const uint64_t n_reads = 2 * n_pairs;
  const KfIn     in{{F[0].d, F[1].d}, {F[0].ls, F[1].ls}, n_pairs, n_reads, k};
  const uint32_t read_grid = grid256(n_reads);

  // ---- windows per hash bin, the partitions
  kf_ull *d_hist, *d_cur;
  STAGE_HIP(c, D.get(&d_hist, KF_HIGH + 1));
  STAGE_HIP(c, D.get(&d_cur, 1));
  STAGE_HIP(c, hipMemsetAsync(d_hist, 0, (KF_HIGH + 1) * 8, st));
  std::vector<uint64_t> pre;
  int                   rc = kf_bin_prefix<K>(c, D, clock, in, &S.bins_ms, pre);
  if (rc != MSGPU_OK) return rc;
  S.n_windows = pre[KF_BINS];
  size_t free_b = 0, total_b = 0;
  STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
  const uint64_t out_bytes = F[0].size + F[1].size + 2; // the outputs are no larger than the inputs
  const uint64_t per_key = 2 * sizeof(K) + 4;           // two key buffers and the run lengths
  if (!budget) budget = free_b > out_bytes ? (free_b - out_bytes) / 2 : 0;
  const KfParts parts = kf_pick_partitions(pre, per_key, budget);
  if (!parts.P || parts.largest * per_key + out_bytes > free_b) {
    snprintf(c->err, sizeof(c->err),
             "%llu windows of %zu-byte keys need %llu bytes per window in partition buffers (budget %llu bytes, %u hash "
             "bins) next to %llu bytes of output; %zu bytes of device memory are free",
             static_cast<kf_ull>(S.n_windows), sizeof(K), static_cast<kf_ull>(per_key), static_cast<kf_ull>(budget),
             KF_BINS, static_cast<kf_ull>(out_bytes), free_b);
    return MSGPU_E_NOMEM;
  }
  S.n_partitions = parts.P;
  S.largest_partition = parts.largest;

  // ---- count: per partition extract, sort, run lengths, histogram, candidates
  std::vector<KfChunk<K>> chunks;
  auto                    histogram = [&](const uint32_t *d_rl, uint32_t runs) -> int {
    STAGE_HIP(c, clock.begin(&S.hist_ms));
    hipLaunchKernelGGL(k_kf_hist, dim3(std::min<uint32_t>(grid256(runs), 2048)), dim3(256), 0, st, d_rl, runs, d_hist);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    return MSGPU_OK;
  };
  rc = kf_count<K>(c, D, clock, in, pre, parts, k, KF_KEEP, KfCountMs{&S.extract_ms, &S.sort_ms, &S.runs_ms, &S.select_ms}, d_cur,
                   histogram, chunks, S.n_distinct, S.n_candidates);
  if (rc != MSGPU_OK) return rc;
  std::vector<kf_ull> hist(KF_HIGH + 1);
  STAGE_HIP(c, hipMemcpyAsync(hist.data(), d_hist, (KF_HIGH + 1) * 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));

  // ---- threshold (host: at most 10001 rows)
  for (uint32_t a = 1; a <= KF_HIGH; ++a)
    if (hist[a]) {
      res->hist_a.push_back(a);
      res->hist_f.push_back(hist[a]);
    }
  S.n_hist_rows = res->hist_a.size();
  rc = msgpu_kf_threshold(res->hist_a.data(), res->hist_f.data(), res->hist_a.size(), &S.q1, &S.q3, &S.upper);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "degenerate histogram (%llu rows, q1 %lld, q3 %lld): no abundance threshold",
             static_cast<kf_ull>(S.n_hist_rows), static_cast<long long>(S.q1), static_cast<long long>(S.q3));
    return rc;
  }

  // ---- the abundant set, ascending, and the table over it
  const uint32_t least = static_cast<uint32_t>(std::min<int64_t>(S.upper, 0xffffffffll));
  STAGE_HIP(c, clock.begin(&S.select_ms));
  kf_ull n_ab = 0;
  rc = kf_count_selected<K>(c, chunks, least, d_cur, n_ab);
  if (rc != MSGPU_OK) return rc;
  if (n_ab >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "%llu abundant k-mers; the limit is 2^31 - 1", n_ab);
    return MSGPU_E_ARG;
  }
  S.n_abundant = n_ab;
  K        *d_abk = nullptr;
  uint32_t *d_abc = nullptr, *d_slots = nullptr, slots_n = 0;
  rc = kf_gather_sorted<K>(c, D, chunks, least, n_ab, k, d_cur, &d_abk, &d_abc, &d_slots, &slots_n);
  if (rc != MSGPU_OK) return rc;
  STAGE_HIP(c, clock.end());

  // ---- verdicts
  uint8_t *d_verdict;
  STAGE_HIP(c, D.get(&d_verdict, n_pairs));
  STAGE_HIP(c, hipMemsetAsync(d_verdict, 0, n_pairs ? n_pairs : 1, st));
  STAGE_HIP(c, clock.begin(&S.verdict_ms));
  if (n_reads)
    hipLaunchKernelGGL(k_kf_verdict<K>, dim3(read_grid), dim3(256), 0, st, in, d_abk, d_slots, slots_n - 1, d_verdict);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());

  // ---- output: lengths, scan, copy, per file
  uint64_t *d_len, *d_off;
  STAGE_HIP(c, D.get(&d_len, n_pairs + 1));
  STAGE_HIP(c, D.get(&d_off, n_pairs + 1));
  uint8_t *d_out[2];
  for (int f = 0; f < 2; ++f) {
    STAGE_HIP(c, clock.begin(&S.output_ms));
    hipLaunchKernelGGL(k_kf_rec_len, dim3(grid256(n_pairs + 1)), dim3(256), 0, st, F[f].ls, d_verdict,
                       n_pairs, d_len);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_scan(D, st, d_len, d_off, n_pairs + 1));
    STAGE_HIP(c, hipMemcpyAsync(&res->out_len[f], d_off + n_pairs, 8, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipStreamSynchronize(st));
    const uint64_t n = res->out_len[f];
    STAGE_HIP(c, D.get(&d_out[f], n));
    if (n)
      hipLaunchKernelGGL(k_kf_copy, dim3(grid_of(n_pairs, 4)), dim3(256), 0, st, F[f].d, F[f].ls,
                         d_verdict, d_off, n_pairs, d_out[f], n);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
  }
  STAGE_HIP(c, clock.begin(&S.copy_ms));
  for (int f = 0; f < 2; ++f)
    if (res->out_len[f]) {
      STAGE_HIP(c, hipHostMalloc(reinterpret_cast<void **>(&res->out[f]), res->out_len[f], hipHostMallocDefault));
      STAGE_HIP(c, hipMemcpyAsync(res->out[f], d_out[f], res->out_len[f], hipMemcpyDeviceToHost, st));
    }
  std::vector<K> abk;
  try {
    res->verdict.resize(n_pairs);
    res->count.resize(n_ab);
    abk.resize(n_ab);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (n_pairs) STAGE_HIP(c, hipMemcpyAsync(res->verdict.data(), d_verdict, n_pairs, hipMemcpyDeviceToHost, st));
  if (n_ab) {
    STAGE_HIP(c, hipMemcpyAsync(res->count.data(), d_abc, n_ab * 4, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(abk.data(), d_abk, n_ab * sizeof(K), hipMemcpyDeviceToHost, st));
  }
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  clock.collect();
  try {
    res->key_hi.resize(abk.size());
    res->key_lo.resize(abk.size());
    for (size_t i = 0; i < abk.size(); ++i) key_split(abk[i], res->key_hi[i], res->key_lo[i]);
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

int  msgpu_kf_create(int device, msgpu_kfctx **out) { return stage_create(device, out); }
void msgpu_kf_destroy(msgpu_kfctx *c) { stage_destroy(c); }

const char *msgpu_kf_last_error(const msgpu_kfctx *c) { return c ? c->err : "null context"; }
uint64_t    msgpu_kf_error_line(const msgpu_kfctx *c) { return c ? c->err_line : 0; }
int         msgpu_kf_error_file(const msgpu_kfctx *c) { return c ? c->err_file : 0; }

// every entry point starts with no error
static void kf_enter(msgpu_kfctx *c) {
  c->err[0]   = 0;
  c->err_line = 0;
  c->err_file = 0;
}

int msgpu_kf_open_pair(msgpu_kfctx *c, const char *path_a, const char *path_b, msgpu_pair **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  kf_enter(c);
  if (!path_a || !path_b) return MSGPU_E_ARG;
  STAGE_HIP(c, hipSetDevice(c->device));
  return kf_pair_open(c, path_a, path_b, out);
}

void msgpu_pair_close(msgpu_pair *pair) { kf_pair_close(pair); }

int msgpu_kf_run_pair(msgpu_kfctx *c, int k, const msgpu_pair *pair, uint32_t flags, uint64_t budget_bytes, msgpu_kf_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  kf_enter(c);
  if (!pair || flags) return MSGPU_E_ARG;
  if (pair->device != c->device || pair->n_files != 2) {
    snprintf(c->err, sizeof(c->err), "the pair holds %d file(s) on device %d; the filter's context is on device %d and takes two",
             pair->n_files, pair->device, c->device);
    return MSGPU_E_ARG;
  }
  if (k < 1 || k > 64) {
    snprintf(c->err, sizeof(c->err), "k = %d is outside 1..64", k);
    return MSGPU_E_ARG;
  }
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_kf_result> res;
  try {
    res.reset(new msgpu_kf_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  msgpu_kf_stats &S = res->stats;
  S.k               = static_cast<uint32_t>(k);
  const KfFile *F = pair->F;
  S.bytes_in[0]   = F[0].size;
  S.bytes_in[1]   = F[1].size;
  if (F[0].n_lines != F[1].n_lines) {
    const int f = F[0].n_lines < F[1].n_lines ? 0 : 1;
    return kf_format_error(c, f, F[f].n_lines + 1, "the two files differ in their number of records");
  }
  const uint64_t n_pairs = F[0].n_lines >> 2;
  S.n_pairs = n_pairs;

  DevArena  D; // the run's own: the pair's bytes are read, never written
  const int rc = k <= 32 ? kf_stage<uint64_t>(c, D, F, n_pairs, k, budget_bytes, res.get())
                         : kf_stage<kf_u128>(c, D, F, n_pairs, k, budget_bytes, res.get());
  if (rc != MSGPU_OK) {
    (void)hipStreamSynchronize(c->stream); // (nothing of the run is still reading the pair when the arena goes)
    return rc;
  }
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;
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
  S.wall_ms      = wall.ms();
  *out           = res.release();
  return MSGPU_OK;
}

// open + run on the pair + close
int msgpu_kf_run(msgpu_kfctx *c, int k, const char *path_a, const char *path_b, uint32_t flags, uint64_t budget_bytes,
                 msgpu_kf_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  kf_enter(c);
  if (!path_a || !path_b || flags) return MSGPU_E_ARG;
  if (k < 1 || k > 64) {
    snprintf(c->err, sizeof(c->err), "k = %d is outside 1..64", k);
    return MSGPU_E_ARG;
  }
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  msgpu_pair *pair = nullptr;
  int         rc = kf_pair_open(c, path_a, path_b, &pair);
  if (rc != MSGPU_OK) return rc;
  rc = msgpu_kf_run_pair(c, k, pair, 0, budget_bytes, out);
  if (rc == MSGPU_OK) {
    (*out)->stats.load_ms    = pair->load_ms;
    (*out)->stats.records_ms = pair->records_ms;
  }
  kf_pair_close(pair);
  if (rc == MSGPU_OK) (*out)->stats.wall_ms = wall.ms();
  return rc;
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
