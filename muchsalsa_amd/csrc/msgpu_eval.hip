// msgpu_eval.hip -- assembly evaluation: consensus QV and completeness of an assembly from the k-mers of the short reads
// (include/msgpu.h, "assembly evaluation").
//
// The table of the reads is the k-mer filter's exact count (msgpu_kmer_shared.h: kf_bin_prefix, kf_pick_partitions, kf_count
// with least = 1 and no histogram hook, kf_gather_sorted): the distinct canonical keys ascending, R per key, and the
// open-addressing table of indices over them.  It is built once and serves any number of assemblies.  A run:
//   k_ev_windows    the hot path.  A workgroup owns EV_TILE consecutive positions of the assembly's store; it stages the 2-bit
//                   codes (16 per word) and the validity bits of its tile and of the EV_HALO positions behind it in LDS, so
//                   that no thread reads k bytes from HBM.  A thread finds its record (binary search over the offsets), cuts
//                   the 2k bits of its window out of the LDS words, forms the canonical key in one or two words, and makes one
//                   kf_find probe: a hit adds 1 to A of the key (a 32-bit integer atomic), a miss is counted (one atomic
//                   per wavefront).  Every position gets a flag byte.
//   k_ev_missing_keys   count-then-write: once the number of missing windows is known their keys go into a list of that exact
//                   size, behind a ballot-aggregated cursor
//   rocPRIM         segmented_reduce of the flags over the record offsets -> windows and missing per record, no atomics;
//                   radix_sort_keys and run_length_encode over the missing keys -> row a = 0 by copy class (k_ev_row0)
//   k_ev_spectrum   over the distinct read keys: S[min(A, 4)][min(R, 10001)], the low rows privatised in LDS
//   k_ev_run_heads / k_ev_intervals   on request: run starts by a neighbour compare on the flags (the record boundary
//                   included), a scan, a compacting write of (record, start, end)
// No floating point on the device: QV and completeness are host arithmetic on the integers.
//
// Kernel rules: vector stores and vector atomics only; no inline asm.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_reduce.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <cmath>
#include <memory>
#include <new>
#include <string>

#include "msgpu_kmer_shared.h"

namespace msgpu {

constexpr uint32_t EV_TILE  = 256; // positions of the store per workgroup, one per thread
constexpr uint32_t EV_HALO  = 64;  // positions staged behind the tile: a window reaches k - 1 <= 63 of them
constexpr uint32_t EV_SPAN  = EV_TILE + EV_HALO;
constexpr uint32_t EV_ROWS  = MSGPU_EV_ROWS;
constexpr uint32_t EV_CLASS = MSGPU_EV_CLASSES;
static_assert(EV_ROWS == KF_HIGH + 1, "row 10001 is the filter's cap row");
enum : uint8_t { EV_NO_WINDOW = 0, EV_PRESENT = 1, EV_MISSING = 2 }; // the flag byte of a position

// bits [s, s + 32) of hi:lo, s in 0..31
__device__ __forceinline__ uint32_t ev_cut(uint32_t lo, uint32_t hi, uint32_t s) {
  return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> s);
}
// the 32 two-bit fields of x in reverse order
__device__ __forceinline__ uint64_t ev_rev_pairs(uint64_t x) {
  x = __brevll(x);
  return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
}
// The canonical key of a window from its bases as LDS holds them: base j in bits [2j, 2j + 2) of hi:lo (hi matters for the
// 128-bit key alone: k in 33..64).  That order is the reverse complement's but for the complement (3 - c = ~c in two bits); the
// forward key is the fields reversed.
template <class K> __device__ __forceinline__ K ev_canonical(uint64_t lo, uint64_t hi, int k) {
  if constexpr (sizeof(K) == 8) {
    const uint64_t m = k == 32 ? ~0ull : ((1ull << (2 * k)) - 1);
    lo &= m;
    const uint64_t rc = ~lo & m, fw = ev_rev_pairs(lo) >> (64 - 2 * k);
    return fw < rc ? fw : rc;
  } else {
    const kf_u128 m = k == 64 ? ~static_cast<kf_u128>(0) : ((static_cast<kf_u128>(1) << (2 * k)) - 1);
    const kf_u128 x = ((static_cast<kf_u128>(hi) << 64) | lo) & m;
    const kf_u128 rc = ~x & m;
    const kf_u128 fw = ((static_cast<kf_u128>(ev_rev_pairs(static_cast<uint64_t>(x))) << 64) | ev_rev_pairs(static_cast<uint64_t>(x >> 64))) >> (128 - 2 * k);
    return fw < rc ? fw : rc;
  }
}

// the record that starts at byte p of the store, if one does
__device__ inline bool ev_starts_record(const SeqRecs &R, uint64_t p) {
  const uint32_t r = seq_record(R, p);
  return r != REC_NONE && R.off[r] == p;
}

template <class K>
__global__ __launch_bounds__(256) void k_ev_windows(SeqRecs R, int k, const K *keys, const uint32_t *slots, uint32_t mask, uint32_t *acount,
                                                    kf_ull *n_missing, uint8_t *flags) {
  __shared__ uint8_t  s_code[EV_SPAN];      // 0..3, or 4 for a byte outside ACGTacgt or behind the store
  __shared__ uint32_t s_word[EV_SPAN / 16]; // the codes, 16 per word, the first in the lowest bits
  __shared__ uint32_t s_ok[EV_SPAN / 32];   // bit i: position i holds a base
  const uint64_t tile = static_cast<uint64_t>(blockIdx.x) * EV_TILE;
  const uint32_t tid = threadIdx.x;
  for (uint32_t i = tid; i < EV_SPAN; i += 256) {
    const uint64_t p = tile + i;
    const uint32_t u = p < R.n_bases ? (R.bases[p] & 0xdfu) : 0u; // case folded
    const bool     base = u == 'A' || u == 'C' || u == 'G' || u == 'T';
    s_code[i] = base ? static_cast<uint8_t>(((u >> 1) & 3u) ^ ((u >> 2) & 1u)) : static_cast<uint8_t>(4); // A 0, C 1, G 2, T 3
  }
  __syncthreads();
  if (tid < EV_SPAN / 16) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; ++j) w |= static_cast<uint32_t>(s_code[16 * tid + j] & 3u) << (2 * j);
    s_word[tid] = w;
  } else if (tid >= 64 && tid < 64 + EV_SPAN / 32) {
    const uint32_t t = tid - 64;
    uint32_t       w = 0;
#pragma unroll
    for (uint32_t j = 0; j < 32; ++j) w |= (s_code[32 * t + j] < 4 ? 1u : 0u) << j;
    s_ok[t] = w;
  }
  __syncthreads();
  const uint64_t p = tile + tid;
  // k bases from position tid on: bits [tid, tid + k) of s_ok (three words hold them: tid & 31 <= 31, k <= 64)
  const uint32_t ow = tid >> 5, os = tid & 31;
  const uint32_t o0 = s_ok[ow], o1 = s_ok[ow + 1], o2 = s_ok[ow + 2]; // (ow + 2 <= 9: the halo's words)
  const uint64_t okbits = (static_cast<uint64_t>(ev_cut(o1, o2, os)) << 32) | ev_cut(o0, o1, os);
  const uint64_t kmask = k == 64 ? ~0ull : ((1ull << k) - 1);
  bool           window = p < R.n_bases && (okbits & kmask) == kmask;
  if (window) { // all k of them in one record
    const uint32_t r = seq_record(R, p);
    window = r != REC_NONE && p + static_cast<uint64_t>(k) <= R.off[r] + R.len[r];
  }
  bool missing = false;
  if (window) {
    // bits [2 tid, 2 tid + 2k) of s_word: five words hold them (2 (tid & 15) <= 30, 2k <= 128)
    const uint32_t cw = tid >> 4, cs = 2 * (tid & 15);
    const uint32_t w0 = s_word[cw], w1 = s_word[cw + 1], w2 = s_word[cw + 2], w3 = s_word[cw + 3], w4 = s_word[cw + 4]; // (cw + 4 <= 19)
    const uint64_t lo = (static_cast<uint64_t>(ev_cut(w1, w2, cs)) << 32) | ev_cut(w0, w1, cs);
    const uint64_t hi = (static_cast<uint64_t>(ev_cut(w3, w4, cs)) << 32) | ev_cut(w2, w3, cs);
    const uint32_t j = kf_find(keys, slots, mask, ev_canonical<K>(lo, hi, k));
    if (j != KF_EMPTY) atomicAdd(&acount[j], 1u);
    else missing = true;
  }
  wave_count(missing, n_missing); // (every lane of the wavefront is here)
  if (p < R.n_bases) flags[p] = !window ? EV_NO_WINDOW : missing ? EV_MISSING : EV_PRESENT;
}

// The keys of the missing windows, compacted behind a ballot-aggregated cursor, once their number is known: the list has its
// exact size.  A missing window is rare in an assembly worth evaluating, so its k bases are read where they lie.
template <class K> __global__ __launch_bounds__(256) void k_ev_missing_keys(SeqRecs R, int k, const uint8_t *flags, uint32_t n, K *miss, uint64_t cap, kf_ull *cursor) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  const bool     take = p < n && flags[p] == EV_MISSING;
  K              key = 0;
  if (take) {
    KfRoll<K> roll(k);
    for (int j = 0; j < k; ++j) (void)roll.step(R.bases[static_cast<uint64_t>(p) + j], key); // (a window: k bases of one record, so the last step gives the key)
  }
  const uint64_t at = wave_append(take, cursor); // (every lane of the wavefront is here)
  if (take && at < cap) miss[at] = key;
}

// a flag as (windows, missing windows << 32): one sum gives both
struct EvFlagSum {
  __device__ uint64_t operator()(uint8_t f) const { return (f != EV_NO_WINDOW ? 1ull : 0ull) | (f == EV_MISSING ? 1ull << 32 : 0ull); }
};

// row a = 0: the copy numbers of the distinct missing keys by class (1..4); *n_runs of them
__global__ __launch_bounds__(256) void k_ev_row0(const uint32_t *cnt, const uint32_t *n_runs, kf_ull *spec) {
  const uint32_t n = *n_runs;
  for (uint32_t base = blockIdx.x * 256; base < n; base += gridDim.x * 256) { // (whole wavefronts stay together)
    const uint32_t i = base + threadIdx.x;
    const uint32_t c = i < n ? min(cnt[i], EV_CLASS - 1) : 0;
    for (uint32_t cls = 1; cls < EV_CLASS; ++cls) wave_count(c == cls, &spec[static_cast<uint64_t>(cls) * EV_ROWS]);
  }
}

// S[min(A, 4)][min(R, 10001)] over the distinct read keys; rows below KF_LOWBIN privatised per workgroup
__global__ __launch_bounds__(256) void k_ev_spectrum(const uint32_t *rcount, const uint32_t *acount, uint32_t n, kf_ull *spec) {
  __shared__ uint32_t h[EV_CLASS * KF_LOWBIN];
  for (uint32_t i = threadIdx.x; i < EV_CLASS * KF_LOWBIN; i += 256) h[i] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint32_t a = min(rcount[i], KF_HIGH), c = min(acount[i], EV_CLASS - 1);
    if (a < KF_LOWBIN) atomicAdd(&h[c * KF_LOWBIN + a], 1u);
    else atomicAdd(&spec[static_cast<uint64_t>(c) * EV_ROWS + a], 1ull);
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < EV_CLASS * KF_LOWBIN; i += 256)
    if (h[i]) atomicAdd(&spec[static_cast<uint64_t>(i / KF_LOWBIN) * EV_ROWS + i % KF_LOWBIN], static_cast<kf_ull>(h[i]));
}

// head[p] = a run of missing windows starts at p; a zero behind them, so that the scan ends on the number of runs
__global__ __launch_bounds__(256) void k_ev_run_heads(SeqRecs R, const uint8_t *flags, uint32_t n, uint32_t *head) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p > n) return;
  bool h = p < n && flags[p] == EV_MISSING;
  if (h && p && flags[p - 1] == EV_MISSING) h = ev_starts_record(R, p); // (k = 1 only: with k >= 2 a record's last position has no window)
  head[p] = h ? 1u : 0u;
}

// run i in position order: (record, first window, last window + k).  The thread at the first window writes record and start,
// the thread at the last one writes the end
__global__ __launch_bounds__(256) void k_ev_intervals(SeqRecs R, const uint8_t *flags, uint32_t n, const uint32_t *head, const uint32_t *idx, int k,
                                                      msgpu_ev_interval *out, uint32_t cap) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n || flags[p] != EV_MISSING) return;
  const bool first = head[p] != 0;
  const bool last = p + 1 == n || flags[p + 1] != EV_MISSING || ev_starts_record(R, p + 1ull);
  if (!first && !last) return;
  const uint32_t r = seq_record(R, p);
  if (r == REC_NONE) return; // (a window lies in a record)
  const uint64_t w = p - R.off[r];
  if (first && idx[p] < cap) {
    out[idx[p]].start    = w;
    out[idx[p]].record   = r;
    out[idx[p]].reserved = 0;
  }
  const uint32_t i = idx[p] + (first ? 1u : 0u) - 1u; // the run this position lies in
  if (last && i < cap) out[i].end = w + static_cast<uint64_t>(k);
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_evctx : msgpu::StageCtx {
  SeqCtxHold      seq;
  ScalarBlock     sc;
  msgpu_ev_table *table = nullptr; // the one table the context holds
  int             open() {
    const int rc = msgpu_seq_create(device, &seq.p);
    return rc != MSGPU_OK ? rc : sc.create();
  }
  ~msgpu_evctx();
};

// Everything of a run that depends on the reads and k only: the distinct canonical keys ascending, R and A per key, the
// open-addressing table over the keys
struct msgpu_ev_table {
  msgpu_evctx    *owner = nullptr;
  int             k = 0;
  DevArena        D;
  void           *d_keys = nullptr; // uint64_t for k <= 32, kf_u128 above
  uint32_t       *d_rcount = nullptr, *d_acount = nullptr, *d_slots = nullptr;
  uint32_t        n = 0, slots_n = 0;
  msgpu_ev_tstats stats{};
  ~msgpu_ev_table() { // (on the owner's device, behind its stream; nobody takes an error here: one line)
    char err[256];
    if (D.verify(nullptr, err, sizeof(err)) != hipSuccess) fprintf(stderr, "msgpu_ev_table_free: %s\n", err);
  }
};

msgpu_evctx::~msgpu_evctx() { delete table; }

struct msgpu_ev_result {
  msgpu_ev_stats                 stats{};
  std::vector<msgpu_ev_record>   records;
  msgpu_ev_record                total{};
  std::vector<uint64_t>          spectrum;
  std::vector<msgpu_ev_interval> intervals;
  std::string                    head, report, spectrum_text, bed;
};

namespace {

enum { EV_SC_MISSING = SC_TOTAL_A, EV_SC_LISTED = SC_TOTAL_B, EV_SC_INTERVALS = SC_TOTAL_C }; // (side by side: one memset zeroes them)

struct EvPinned { // a page-locked buffer the tables come back through
  void *p = nullptr;
  ~EvPinned() {
    if (p) (void)hipHostFree(p);
  }
};

inline void ev_enter(msgpu_evctx *c) {
  c->err[0]   = 0;
  c->err_line = 0;
  c->err_file = 0;
}

inline int ev_check_k(msgpu_evctx *c, int k) {
  if (k >= 1 && k <= 64) return MSGPU_OK;
  snprintf(c->err, sizeof(c->err), "k = %d is outside 1..64", k);
  return MSGPU_E_ARG;
}

// the table of the files of a pair, for one key width
template <class K> int ev_table_build(msgpu_evctx *c, const KfFile *F, int n_files, int k, uint64_t budget, msgpu_ev_table &T) {
  msgpu_ev_tstats &S = T.stats;
  hipStream_t      st = c->stream;
  DevArena        &D = T.D;
  StageClock       clock(st);
  const uint64_t   n_first = F[0].n_lines >> 2, n_reads = n_first + (n_files == 2 ? F[1].n_lines >> 2 : 0);
  const KfIn       in{{F[0].d, F[1].d}, {F[0].ls, F[1].ls}, n_first, n_reads, k};
  kf_ull          *d_cur;
  STAGE_HIP(c, D.get(&d_cur, 1));
  std::vector<uint64_t> pre;
  int                   rc = kf_bin_prefix<K>(c, D, clock, in, &S.bins_ms, pre);
  if (rc != MSGPU_OK) return rc;
  S.n_windows = pre[KF_BINS];
  size_t free_b = 0, total_b = 0;
  STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
  const uint64_t per_key = 2 * sizeof(K) + 4; // two key buffers and the run lengths
  if (!budget) budget = free_b / 2;
  const KfParts parts = kf_pick_partitions(pre, per_key, budget);
  if (!parts.P || parts.largest * per_key > free_b) {
    snprintf(c->err, sizeof(c->err),
             "%llu windows of %zu-byte keys need %llu bytes per window in partition buffers (budget %llu bytes, %u hash "
             "bins); %zu bytes of device memory are free",
             static_cast<kf_ull>(S.n_windows), sizeof(K), static_cast<kf_ull>(per_key), static_cast<kf_ull>(budget), KF_BINS, free_b);
    return MSGPU_E_NOMEM;
  }
  S.n_partitions      = parts.P;
  S.largest_partition = parts.largest;
  std::vector<KfChunk<K>> chunks;
  uint64_t                kept = 0;
  rc = kf_count<K>(c, D, clock, in, pre, parts, k, 1u, KfCountMs{&S.extract_ms, &S.sort_ms, &S.runs_ms, &S.select_ms}, d_cur,
                   [](const uint32_t *, uint32_t) { return MSGPU_OK; }, chunks, S.n_distinct, kept);
  if (rc != MSGPU_OK) return rc;
  if (kept > (1ull << 30)) { // (the table has 2^31 slots at most: its slot count and mask are 32 bits wide)
    snprintf(c->err, sizeof(c->err), "%llu distinct read k-mers; the limit is 2^30", static_cast<kf_ull>(kept));
    return MSGPU_E_ARG;
  }
  // what the gather holds at its widest: the chunks, their copy, the sorted arrays and the sort's buffer; then the table and A
  uint64_t slots = 64;
  while (slots < 2 * kept) slots <<= 1;
  const uint64_t pair_bytes = kept * (sizeof(K) + 4), need = 3 * pair_bytes + slots * 4 + kept * 4;
  STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
  if (need > free_b) {
    snprintf(c->err, sizeof(c->err),
             "%llu distinct read k-mers of %zu-byte keys need %llu bytes next to their chunks (sorted copy, sort buffer, %llu table "
             "slots, assembly counts); %zu bytes of device memory are free",
             static_cast<kf_ull>(kept), sizeof(K), static_cast<kf_ull>(need), static_cast<kf_ull>(slots), free_b);
    return MSGPU_E_NOMEM;
  }
  const StageTimer gather;
  K               *d_keys = nullptr;
  rc = kf_gather_sorted<K>(c, D, chunks, 1u, kept, k, d_cur, &d_keys, &T.d_rcount, &T.d_slots, &T.slots_n);
  if (rc != MSGPU_OK) return rc;
  T.d_keys = d_keys;
  T.n      = static_cast<uint32_t>(kept);
  STAGE_HIP(c, D.get(&T.d_acount, kept));
  STAGE_HIP(c, hipStreamSynchronize(st));
  S.table_ms = gather.ms();
  clock.collect();
  D.drop(d_cur);
  S.bytes_resident = D.live;
  return stage_verify(c, D);
}

int ev_table_create(msgpu_evctx *c, int k, const msgpu_pair *pair, uint64_t budget, msgpu_ev_table **out) {
  if (c->table) {
    snprintf(c->err, sizeof(c->err), "the context holds a table already (k = %d): free it first", c->table->k);
    return MSGPU_E_STATE;
  }
  const StageTimer                wall;
  std::unique_ptr<msgpu_ev_table> T;
  try {
    T.reset(new msgpu_ev_table());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  T->owner = c;
  T->k     = k;
  msgpu_ev_tstats &S = T->stats;
  S.k = static_cast<uint32_t>(k);
  for (int f = 0; f < pair->n_files; ++f) {
    S.bytes_in[f]  = pair->F[f].size;
    S.n_records[f] = pair->F[f].n_lines >> 2;
  }
  const int rc = k <= 32 ? ev_table_build<uint64_t>(c, pair->F, pair->n_files, k, budget, *T)
                         : ev_table_build<kf_u128>(c, pair->F, pair->n_files, k, budget, *T);
  if (rc != MSGPU_OK) {
    (void)hipStreamSynchronize(c->stream); // (nothing of the build is still reading the pair when the arena goes)
    return rc;
  }
  S.wall_ms = wall.ms();
  c->table  = T.get();
  *out      = T.release();
  return MSGPU_OK;
}

void ev_qv_text(uint64_t missing, uint64_t windows, int k, char *buf, size_t n) {
  double qv = 0;
  (void)msgpu_ev_qv(missing, windows, k, &qv);
  if (!windows) snprintf(buf, n, "-");
  else if (!missing) snprintf(buf, n, "inf");
  else snprintf(buf, n, "%.2f", qv);
}

// one assembly on the table, for one key width
template <class K> int ev_run_stage(msgpu_evctx *c, msgpu_ev_table &T, const msgpu_ev_params &prm, const char *path, msgpu_ev_result *res) {
  msgpu_ev_stats  &S = res->stats;
  hipStream_t      st = c->stream;
  DevArena         D; // the run's own: of the table it writes A alone
  StageClock       clock(st);
  const int        k = prm.k;
  const StageTimer load;
  StageFile        F;
  int              rc = stage_load(c, D, path, 1, "assembly", F);
  if (rc != MSGPU_OK) return rc;
  S.load_ms = load.ms();
  const SeqRecs &R = F.recs;
  const uint32_t NR = R.n;
  S.n_records = NR;
  if (R.n_bases >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "assembly %s: %llu bases in the store; the limit is 2^31 - 1 (fewer than 2^31 windows)", path,
             static_cast<kf_ull>(R.n_bases));
    return MSGPU_E_ARG;
  }
  const uint32_t        NB = static_cast<uint32_t>(R.n_bases);
  std::vector<uint64_t> ends;
  try {
    ends.resize(NR);
    res->records.resize(NR);
    res->spectrum.assign(static_cast<size_t>(EV_CLASS) * EV_ROWS, 0);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  for (uint32_t i = 0; i < NR; ++i) {
    const uint64_t L = msgpu_seq_length(F.f, i);
    ends[i] = msgpu_seq_offset(F.f, i) + L;
    res->records[i].length = L;
    S.n_bases += L;
  }
  size_t free_b = 0, total_b = 0;
  STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
  const uint64_t interval_bytes = prm.intervals ? 8ull * (NB + 1ull) : 0; // (the intervals themselves: 24 bytes per run, checked where their number is known)
  const uint64_t need = NB + NR * 16ull + static_cast<uint64_t>(EV_CLASS) * EV_ROWS * 8 + interval_bytes;
  if (need > free_b) {
    snprintf(c->err, sizeof(c->err),
             "assembly %s: %u flag bytes, %u records and %llu bytes of run starts need %llu bytes; %zu bytes of device memory are free", path, NB,
             NR, static_cast<kf_ull>(interval_bytes), static_cast<kf_ull>(need), free_b);
    return MSGPU_E_NOMEM;
  }
  const K  *d_keys = static_cast<const K *>(T.d_keys);
  uint8_t  *d_flags;
  kf_ull   *d_spec;
  uint64_t *d_end, *d_rec;
  STAGE_HIP(c, D.get(&d_flags, NB + 1ull));
  STAGE_HIP(c, D.get_zeroed(&d_spec, static_cast<size_t>(EV_CLASS) * EV_ROWS, st));
  STAGE_HIP(c, D.get(&d_end, NR));
  STAGE_HIP(c, D.get(&d_rec, NR));
  if (NR) STAGE_HIP(c, hipMemcpyAsync(d_end, ends.data(), NR * 8ull, hipMemcpyHostToDevice, st));
  kf_ull *sc_d = reinterpret_cast<kf_ull *>(c->sc.d);
  STAGE_HIP(c, hipMemsetAsync(c->sc.d + EV_SC_MISSING, 0, 3 * 8, st));
  STAGE_HIP(c, hipMemsetAsync(T.d_acount, 0, (T.n ? T.n : 1) * 4ull, st)); // A is this run's

  // ---- the windows
  STAGE_HIP(c, clock.begin(&S.window_ms));
  if (NB)
    hipLaunchKernelGGL(k_ev_windows<K>, dim3(grid_of(NB, EV_TILE)), dim3(256), 0, st, R, k, d_keys, T.d_slots, T.slots_n - 1, T.d_acount,
                       sc_d + EV_SC_MISSING, d_flags);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());

  // ---- per record: windows and missing, one sum of (windows, missing << 32); the scalar block comes back behind it
  STAGE_HIP(c, clock.begin(&S.reduce_ms));
  if (NR)
    STAGE_HIP(c, stage_rocprim(D, [&](void *tmp, size_t &bytes) {
      return rocprim::segmented_reduce(tmp, bytes, rocprim::make_transform_iterator(d_flags, EvFlagSum()), d_rec, NR, R.off, static_cast<const uint64_t *>(d_end),
                                       rocprim::plus<uint64_t>(), uint64_t(0), st);
    }));
  STAGE_HIP(c, clock.end());
  rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint64_t n_miss = c->sc.h[EV_SC_MISSING];
  if (n_miss > NB) { // never seen: a position has one window at most
    snprintf(c->err, sizeof(c->err), "%llu missing windows at %u positions", static_cast<kf_ull>(n_miss), NB);
    return MSGPU_E_STATE;
  }

  // ---- row a = 0: the missing keys, listed at their exact number, sorted, counted by copy number
  bool listed_known = !n_miss;
  STAGE_HIP(c, clock.begin(&S.missing_ms));
  if (n_miss) {
    K        *d_miss = nullptr, *d_sorted = nullptr, *d_uniq = nullptr;
    uint32_t *d_cnt = nullptr, *d_nruns = nullptr;
    size_t    sort_tmp = 0, rle_tmp = 0; // (rocPRIM answers the sizes without touching a buffer)
    STAGE_HIP(c, rocprim::radix_sort_keys(nullptr, sort_tmp, d_miss, d_sorted, static_cast<unsigned int>(n_miss), 0, 2 * k, st));
    STAGE_HIP(c, rocprim::run_length_encode(nullptr, rle_tmp, d_sorted, static_cast<unsigned int>(n_miss), d_uniq, d_cnt, d_nruns, st));
    const uint64_t list_bytes = n_miss * (3 * sizeof(K) + 4), tmp_bytes = std::max(sort_tmp, rle_tmp);
    STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
    if (list_bytes + tmp_bytes + interval_bytes > free_b) {
      snprintf(c->err, sizeof(c->err),
               "assembly %s: %llu missing windows of %zu-byte keys need %llu bytes (list, sorted list, distinct keys, copy numbers), %llu bytes "
               "of sort buffer and %llu bytes of run starts; %zu bytes of device memory are free",
               path, static_cast<kf_ull>(n_miss), sizeof(K), static_cast<kf_ull>(list_bytes), static_cast<kf_ull>(tmp_bytes),
               static_cast<kf_ull>(interval_bytes), free_b);
      return MSGPU_E_NOMEM;
    }
    STAGE_HIP(c, D.get(&d_miss, n_miss));
    STAGE_HIP(c, D.get(&d_sorted, n_miss));
    STAGE_HIP(c, D.get(&d_uniq, n_miss));
    STAGE_HIP(c, D.get(&d_cnt, n_miss));
    STAGE_HIP(c, D.get(&d_nruns, 1));
    hipLaunchKernelGGL(k_ev_missing_keys<K>, dim3(grid256(NB)), dim3(256), 0, st, R, k, d_flags, NB, d_miss, n_miss, sc_d + EV_SC_LISTED);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_rocprim(D, [&](void *tmp, size_t &bytes) {
      return rocprim::radix_sort_keys(tmp, bytes, d_miss, d_sorted, static_cast<unsigned int>(n_miss), 0, 2 * k, st);
    }));
    STAGE_HIP(c, stage_rocprim(D, [&](void *tmp, size_t &bytes) {
      return rocprim::run_length_encode(tmp, bytes, d_sorted, static_cast<unsigned int>(n_miss), d_uniq, d_cnt, d_nruns, st);
    }));
    hipLaunchKernelGGL(k_ev_row0, dim3(std::min<uint32_t>(grid256(n_miss), 1024)), dim3(256), 0, st, d_cnt, d_nruns, d_spec);
    STAGE_HIP(c, hipGetLastError());
  }
  STAGE_HIP(c, clock.end());

  // ---- the spectrum over the read keys
  STAGE_HIP(c, clock.begin(&S.spectrum_ms));
  if (T.n) hipLaunchKernelGGL(k_ev_spectrum, dim3(std::min<uint32_t>(grid256(T.n), 1024)), dim3(256), 0, st, T.d_rcount, T.d_acount, T.n, d_spec);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());

  // ---- rule 7
  uint32_t           NI = 0;
  msgpu_ev_interval *d_iv = nullptr;
  STAGE_HIP(c, clock.begin(&S.intervals_ms));
  if (prm.intervals && n_miss) {
    uint32_t *d_head, *d_idx;
    STAGE_HIP(c, D.get(&d_head, NB + 1ull));
    STAGE_HIP(c, D.get(&d_idx, NB + 1ull));
    hipLaunchKernelGGL(k_ev_run_heads, dim3(grid256(NB + 1ull)), dim3(256), 0, st, R, d_flags, NB, d_head);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_scan_total(D, st, d_head, d_idx, NB, c->sc, EV_SC_INTERVALS));
    rc = c->sc.read(c);
    if (rc != MSGPU_OK) return rc;
    NI = static_cast<uint32_t>(c->sc.h[EV_SC_INTERVALS]);
    listed_known = true; // (the block as it stood behind the list kernel)
    STAGE_HIP(c, D.get(&d_iv, NI));
    if (NI) hipLaunchKernelGGL(k_ev_intervals, dim3(grid256(NB)), dim3(256), 0, st, R, d_flags, NB, d_head, d_idx, k, d_iv, NI);
    STAGE_HIP(c, hipGetLastError());
  }
  STAGE_HIP(c, clock.end());

  if (!listed_known) {
    rc = c->sc.read(c);
    if (rc != MSGPU_OK) return rc;
  }
  if (n_miss && c->sc.h[EV_SC_LISTED] != n_miss) { // the two passes over the flags disagree: never seen
    snprintf(c->err, sizeof(c->err), "%llu missing keys listed where %llu windows were counted missing", static_cast<kf_ull>(c->sc.h[EV_SC_LISTED]),
             static_cast<kf_ull>(n_miss));
    return MSGPU_E_STATE;
  }

  // ---- the tables, through page-locked memory
  const size_t spec_bytes = static_cast<size_t>(EV_CLASS) * EV_ROWS * 8, rec_bytes = NR * 8ull, iv_bytes = NI * sizeof(msgpu_ev_interval);
  EvPinned     pin;
  STAGE_HIP(c, hipHostMalloc(&pin.p, spec_bytes + rec_bytes + iv_bytes + 8, hipHostMallocDefault));
  uint8_t *h = static_cast<uint8_t *>(pin.p);
  STAGE_HIP(c, clock.begin(&S.copy_ms));
  STAGE_HIP(c, hipMemcpyAsync(h, d_spec, spec_bytes, hipMemcpyDeviceToHost, st));
  if (NR) STAGE_HIP(c, hipMemcpyAsync(h + spec_bytes, d_rec, rec_bytes, hipMemcpyDeviceToHost, st));
  if (NI) STAGE_HIP(c, hipMemcpyAsync(h + spec_bytes + rec_bytes, d_iv, iv_bytes, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  clock.collect();
  memcpy(res->spectrum.data(), h, spec_bytes);
  for (uint32_t i = 0; i < NR; ++i) {
    uint64_t v;
    memcpy(&v, h + spec_bytes + i * 8ull, 8);
    res->records[i].windows = v & 0xffffffffull;
    res->records[i].missing = v >> 32;
    res->total.length += res->records[i].length;
    res->total.windows += res->records[i].windows;
    res->total.missing += res->records[i].missing;
  }
  try {
    res->intervals.resize(NI);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (NI) memcpy(res->intervals.data(), h + spec_bytes + rec_bytes, iv_bytes);
  S.n_windows   = res->total.windows;
  S.n_missing   = res->total.missing;
  S.n_intervals = NI;
  if (S.n_missing != n_miss) { // the flags and the list disagree: never seen; a result built on it would be wrong
    snprintf(c->err, sizeof(c->err), "%llu missing windows in the flags where %llu keys were listed", static_cast<kf_ull>(S.n_missing),
             static_cast<kf_ull>(n_miss));
    return MSGPU_E_STATE;
  }
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;
  S.bytes_peak = D.peak;

  // ---- rule 6 and the texts (host)
  const StageTimer host;
  const uint64_t  *sp = res->spectrum.data();
  for (uint32_t cls = 0; cls < EV_CLASS; ++cls) {
    S.n_missing_distinct += sp[static_cast<size_t>(cls) * EV_ROWS];
    for (uint32_t a = prm.min_count; a < EV_ROWS; ++a) {
      S.solid += sp[static_cast<size_t>(cls) * EV_ROWS + a];
      if (cls) S.found += sp[static_cast<size_t>(cls) * EV_ROWS + a];
    }
  }
  try {
    char        buf[256], qv[32];
    const char *slash = strrchr(path, '/');
    const std::string name_line = std::string("#assembly\t") + (slash ? slash + 1 : path) + "\n";
    snprintf(buf, sizeof(buf), "#k\t%d\tmin_count\t%u\n", k, prm.min_count);
    res->head   = buf;
    res->report = name_line + "record\tlength\twindows\tmissing\tqv\n";
    for (uint32_t i = 0; i <= NR; ++i) {
      const msgpu_ev_record &r = i < NR ? res->records[i] : res->total;
      ev_qv_text(r.missing, r.windows, k, qv, sizeof(qv));
      res->report += i < NR ? msgpu_seq_name(F.f, i) : "total";
      snprintf(buf, sizeof(buf), "\t%llu\t%llu\t%llu\t%s\n", static_cast<kf_ull>(r.length), static_cast<kf_ull>(r.windows),
               static_cast<kf_ull>(r.missing), qv);
      res->report += buf;
    }
    if (S.solid) snprintf(qv, sizeof(qv), "%.4f", 100.0 * static_cast<double>(S.found) / static_cast<double>(S.solid));
    else snprintf(qv, sizeof(qv), "-");
    snprintf(buf, sizeof(buf), "completeness\t%llu\t%llu\t%s\n", static_cast<kf_ull>(S.found), static_cast<kf_ull>(S.solid), qv);
    res->report += buf;
    res->spectrum_text = name_line;
    for (uint32_t a = 0; a < EV_ROWS; ++a) {
      uint64_t row[EV_CLASS], any = 0;
      for (uint32_t cls = 0; cls < EV_CLASS; ++cls) any |= row[cls] = sp[static_cast<size_t>(cls) * EV_ROWS + a];
      if (!any) continue;
      snprintf(buf, sizeof(buf), "%u\t%llu\t%llu\t%llu\t%llu\t%llu\n", a, static_cast<kf_ull>(row[0]), static_cast<kf_ull>(row[1]),
               static_cast<kf_ull>(row[2]), static_cast<kf_ull>(row[3]), static_cast<kf_ull>(row[4]));
      res->spectrum_text += buf;
    }
    if (prm.intervals) {
      res->bed = name_line;
      for (const msgpu_ev_interval &iv : res->intervals) {
        res->bed += msgpu_seq_name(F.f, iv.record);
        snprintf(buf, sizeof(buf), "\t%llu\t%llu\n", static_cast<kf_ull>(iv.start), static_cast<kf_ull>(iv.end));
        res->bed += buf;
      }
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  S.host_ms = host.ms();
  return MSGPU_OK;
}

int ev_params(msgpu_evctx *c, const msgpu_ev_params *params, msgpu_ev_params &prm) {
  prm = *params;
  const int rc = ev_check_k(c, prm.k);
  if (rc != MSGPU_OK) return rc;
  if (prm.min_count < 1 || prm.min_count > 10000) {
    snprintf(c->err, sizeof(c->err), "min_count = %u is outside 1..10000", prm.min_count);
    return MSGPU_E_ARG;
  }
  return MSGPU_OK;
}

} // namespace

extern "C" {

void msgpu_ev_default_params(msgpu_ev_params *p) {
  if (p) *p = msgpu_ev_params{21, 2, 0, 0};
}

// rule 4
int msgpu_ev_qv(uint64_t missing, uint64_t windows, int k, double *qv) {
  if (!qv || k < 1 || k > 64 || missing > windows) return MSGPU_E_ARG;
  if (!windows) *qv = std::nan("");
  else if (!missing) *qv = INFINITY;
  else {
    const double p = static_cast<double>(missing) / static_cast<double>(windows);
    const double e = -std::expm1(std::log1p(-p) / static_cast<double>(k));
    *qv            = -10.0 * std::log10(e) + 0.0;
  }
  return MSGPU_OK;
}

int  msgpu_ev_create(int device, msgpu_evctx **out) { return stage_create(device, out); }
void msgpu_ev_destroy(msgpu_evctx *c) { stage_destroy(c); }

const char *msgpu_ev_last_error(const msgpu_evctx *c) { return c ? c->err : "null context"; }
uint64_t    msgpu_ev_error_line(const msgpu_evctx *c) { return c ? c->err_line : 0; }
int         msgpu_ev_error_file(const msgpu_evctx *c) { return c ? c->err_file : 0; }

int msgpu_ev_table_open_pair(msgpu_evctx *c, int k, const msgpu_pair *pair, uint64_t budget_bytes, msgpu_ev_table **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  ev_enter(c);
  if (!pair) return MSGPU_E_ARG;
  const int rc = ev_check_k(c, k);
  if (rc != MSGPU_OK) return rc;
  if (pair->device != c->device) {
    snprintf(c->err, sizeof(c->err), "the pair is on device %d, the context on device %d", pair->device, c->device);
    return MSGPU_E_ARG;
  }
  STAGE_HIP(c, hipSetDevice(c->device));
  return ev_table_create(c, k, pair, budget_bytes, out);
}

// open the files + the table of the pair + close
int msgpu_ev_table_open(msgpu_evctx *c, int k, const char *path_a, const char *path_b, uint64_t budget_bytes, msgpu_ev_table **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  ev_enter(c);
  if (!path_a) return MSGPU_E_ARG;
  int rc = ev_check_k(c, k);
  if (rc != MSGPU_OK) return rc;
  STAGE_HIP(c, hipSetDevice(c->device));
  msgpu_pair *pair = nullptr;
  rc = kf_pair_open(c, path_a, path_b, &pair);
  if (rc != MSGPU_OK) return rc;
  rc = ev_table_create(c, k, pair, budget_bytes, out);
  if (rc == MSGPU_OK) {
    (*out)->stats.load_ms    = pair->load_ms;
    (*out)->stats.records_ms = pair->records_ms;
    (*out)->stats.wall_ms += pair->load_ms + pair->records_ms;
  }
  kf_pair_close(pair);
  return rc;
}

int msgpu_ev_table_stats(const msgpu_ev_table *table, msgpu_ev_tstats *out) {
  if (!table || !out) return MSGPU_E_ARG;
  *out = table->stats;
  return MSGPU_OK;
}

void msgpu_ev_table_free(msgpu_ev_table *table) {
  if (!table) return;
  msgpu_evctx *c = table->owner;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->table == table) c->table = nullptr;
  delete table;
}

int msgpu_ev_run_table(msgpu_evctx *c, const msgpu_ev_params *params, msgpu_ev_table *table, const char *assembly_path, uint32_t flags,
                       msgpu_ev_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  ev_enter(c);
  if (!params || !table || !assembly_path || flags) return MSGPU_E_ARG;
  msgpu_ev_params prm;
  int             rc = ev_params(c, params, prm);
  if (rc != MSGPU_OK) return rc;
  if (table != c->table) {
    snprintf(c->err, sizeof(c->err), "the table is not this context's");
    return MSGPU_E_ARG;
  }
  if (prm.k != table->k) {
    snprintf(c->err, sizeof(c->err), "the run has k = %d; the table was built with k = %d", prm.k, table->k);
    return MSGPU_E_ARG;
  }
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_ev_result> res;
  try {
    res.reset(new msgpu_ev_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  res->stats.k         = static_cast<uint32_t>(prm.k);
  res->stats.min_count = prm.min_count;
  const uint64_t lost0 = c->sc.lost;
  rc = prm.k <= 32 ? ev_run_stage<uint64_t>(c, *table, prm, assembly_path, res.get()) : ev_run_stage<kf_u128>(c, *table, prm, assembly_path, res.get());
  if (rc != MSGPU_OK) {
    (void)hipStreamSynchronize(c->stream); // (nothing of the run is still reading the table when the arena goes)
    return rc;
  }
  res->stats.n_lost_publications = c->sc.lost - lost0;
  res->stats.wall_ms             = wall.ms();
  *out                           = res.release();
  return MSGPU_OK;
}

// table_open + run_table + table_free
int msgpu_ev_run(msgpu_evctx *c, const msgpu_ev_params *params, const char *path_a, const char *path_b, const char *assembly_path, uint32_t flags,
                 uint64_t budget_bytes, msgpu_ev_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out = nullptr;
  ev_enter(c);
  if (!params || !path_a || !assembly_path || flags) return MSGPU_E_ARG;
  msgpu_ev_params prm;
  int             rc = ev_params(c, params, prm);
  if (rc != MSGPU_OK) return rc;
  const StageTimer wall;
  msgpu_ev_table  *table = nullptr;
  rc = msgpu_ev_table_open(c, prm.k, path_a, path_b, budget_bytes, &table);
  if (rc != MSGPU_OK) return rc;
  rc = msgpu_ev_run_table(c, &prm, table, assembly_path, 0, out);
  msgpu_ev_table_free(table);
  if (rc == MSGPU_OK) (*out)->stats.wall_ms = wall.ms();
  return rc;
}

int msgpu_ev_result_stats(const msgpu_ev_result *r, msgpu_ev_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

int msgpu_ev_result_records(const msgpu_ev_result *r, const msgpu_ev_record **records, const msgpu_ev_record **total, uint64_t *n) {
  if (!r || !records || !total || !n) return MSGPU_E_ARG;
  *records = r->records.data();
  *total   = &r->total;
  *n       = r->records.size();
  return MSGPU_OK;
}

int msgpu_ev_result_spectrum(const msgpu_ev_result *r, const uint64_t **spectrum) {
  if (!r || !spectrum) return MSGPU_E_ARG;
  *spectrum = r->spectrum.data();
  return MSGPU_OK;
}

int msgpu_ev_result_intervals(const msgpu_ev_result *r, const msgpu_ev_interval **intervals, uint64_t *n) {
  if (!r || !intervals || !n) return MSGPU_E_ARG;
  *intervals = r->intervals.data();
  *n         = r->intervals.size();
  return MSGPU_OK;
}

const char *msgpu_ev_result_text(const msgpu_ev_result *r, int which, uint64_t *len) {
  if (len) *len = 0;
  if (!r) return "";
  const std::string *s = which == MSGPU_EV_TEXT_HEAD ? &r->head : which == MSGPU_EV_TEXT_REPORT ? &r->report
                       : which == MSGPU_EV_TEXT_SPECTRUM ? &r->spectrum_text : which == MSGPU_EV_TEXT_BED ? &r->bed : nullptr;
  if (!s) return "";
  if (len) *len = s->size();
  return s->data();
}

void msgpu_ev_result_free(msgpu_ev_result *r) { delete r; }

} // extern "C"
