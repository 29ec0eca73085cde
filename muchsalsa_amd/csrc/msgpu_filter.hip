// msgpu_filter.hip -- the unitig coverage filter (include/msgpu.h, "unitig coverage filter"; DESIGN.md section
// "Unitig coverage filter").
//
// Pass 1 computes, per block of the PAF, the maximum coverage by the first line of each read id in three width classes:
//   * <= UF_WAVE lines    k_uf_wave    one wavefront per block, one line per lane: de-duplication and depth by shuffles;
//                                      the maximum depth is reached at a kept interval's start, so no sort is needed;
//   * <= UF_GROUP lines   k_uf_group   one workgroup per block, the lines staged in LDS, the same all-pairs rule;
//   * larger              giant        de-duplication by a segmented sort of (read, line), then a segmented sort of the
//                                      interval endpoints and one wavefront per block sweeping them (k_uf_sweep_max).
// Per unitig id the value of its last block is taken (k_uf_id_values), copied back (4 bytes per id) and the quartiles
// are order statistics on the host (nth_element).  Pass 2 sorts the endpoints of ALL lines of the outlier blocks and
// sweeps each block twice (count, then emit at the scanned offsets), so fragments come out in (block, position) order
// whatever the scheduling.  The output is one gather of whole records and fragments and one FASTA wrapping launch on the
// sequence store of msgpu_seq.hip.
//
// Kernel rules: vector stores only; no inline asm; this file is built with -ffp-contract=off (q1 / q3 / upper).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "msgpu.h"
#include "msgpu_stage.h"

namespace msgpu {

constexpr uint32_t UF_WAVE  = 64;   // lines of a block in the wavefront class
constexpr uint32_t UF_GROUP = 1024; // lines of a block in the workgroup class (LDS: 16 bytes per line)
constexpr uint32_t UF_RUN   = 500;  // shortest fragment

// one wavefront per block; 4 blocks per 256-thread workgroup
__global__ __launch_bounds__(256) void k_uf_wave(const uint32_t *blocks, uint32_t n_blocks, const uint32_t *bfirst,
                                                 const uint32_t *bn, const uint32_t *qs, const uint32_t *qe,
                                                 const uint32_t *rd, uint32_t *val) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n_blocks) return; // (the whole wavefront leaves together)
  const int      lane = threadIdx.x & 63;
  const uint32_t b = blocks[w], n = bn[b], f = bfirst[b];
  const bool     have = static_cast<uint32_t>(lane) < n;
  const uint32_t s = have ? qs[f + lane] : 0, e = have ? qe[f + lane] : 0, r = have ? rd[f + lane] : 0xffffffffu;
  bool           kept = have && s < e;
  for (int j = 0; j < 64; ++j) { // the first line of a read id in the block counts, later ones add nothing
    const uint32_t rj = __shfl(r, j);
    if (j < lane && static_cast<uint32_t>(j) < n && rj == r) kept = false;
  }
  uint32_t depth = 0; // lines of the block covering this line's start
  for (int j = 0; j < 64; ++j) {
    const uint32_t sj = __shfl(s, j), ej = __shfl(e, j);
    const int      kj = __shfl(static_cast<int>(kept), j);
    if (kj && sj <= s && s < ej) ++depth;
  }
  uint32_t m = kept ? depth : 0;
  for (int o = 32; o > 0; o >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(m, o)));
  if (lane == 0) val[b] = m;
}

// one workgroup per block, lines in LDS; all pairs, 256 threads
__global__ __launch_bounds__(256) void k_uf_group(const uint32_t *blocks, const uint32_t *bfirst, const uint32_t *bn,
                                                  const uint32_t *qs, const uint32_t *qe, const uint32_t *rd,
                                                  uint32_t *val) {
  __shared__ uint32_t ls[UF_GROUP], le[UF_GROUP], lr[UF_GROUP], lk[UF_GROUP];
  __shared__ uint32_t wmax[4];
  const uint32_t      b = blocks[blockIdx.x], n = min(bn[b], UF_GROUP), f = bfirst[b];
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    ls[i] = qs[f + i];
    le[i] = qe[f + i];
    lr[i] = rd[f + i];
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    bool kept = ls[i] < le[i];
    for (uint32_t j = 0; j < i && kept; ++j)
      if (lr[j] == lr[i]) kept = false;
    lk[i] = kept;
  }
  __syncthreads();
  uint32_t m = 0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) {
    if (!lk[i]) continue;
    const uint32_t s = ls[i];
    uint32_t       depth = 0;
    for (uint32_t j = 0; j < n; ++j) depth += (lk[j] && ls[j] <= s && s < le[j]) ? 1u : 0u;
    m = max(m, depth);
  }
  for (int o = 32; o > 0; o >>= 1) m = max(m, static_cast<uint32_t>(__shfl_xor(m, o)));
  if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) val[b] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
}

// giant blocks, step 1: (read << 32 | line inside the block) per line
__global__ __launch_bounds__(256) void k_uf_read_keys(const uint32_t *blocks, const uint64_t *seg_off, uint32_t n_seg,
                                                      const uint32_t *bfirst, const uint32_t *rd, uint64_t *keys) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= seg_off[n_seg]) return;
  const uint32_t g = last_le(seg_off, 0, n_seg, i), local = static_cast<uint32_t>(i - seg_off[g]);
  keys[i] = (static_cast<uint64_t>(rd[bfirst[blocks[g]] + local]) << 32) | local;
}

// endpoint keys: (pos << 1 | 1) for a start, (pos << 1) for an end, so that at one position the ends come first.  A line
// that does not count (a repeated read id in pass 1, an empty interval) gives the neutral pair (end 0, start 0).
__device__ inline void uf_put_events(uint64_t *ev, uint64_t at, bool counts, uint32_t s, uint32_t e) {
  const uint64_t a = counts ? ((static_cast<uint64_t>(s) << 1) | 1) : 1, z = counts ? (static_cast<uint64_t>(e) << 1) : 0;
  ev[2 * at]     = a;
  ev[2 * at + 1] = z;
}

// giant blocks, step 2: the sorted (read, line) keys -> endpoint keys of the lines that count
__global__ __launch_bounds__(256) void k_uf_dedup_events(const uint32_t *blocks, const uint64_t *seg_off, uint32_t n_seg,
                                                         const uint32_t *bfirst, const uint32_t *qs, const uint32_t *qe,
                                                         const uint64_t *sorted, uint64_t *ev) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= seg_off[n_seg]) return;
  const uint32_t g     = last_le(seg_off, 0, n_seg, i);
  const uint64_t k     = sorted[i];
  const bool     first = i == seg_off[g] || (sorted[i - 1] >> 32) != (k >> 32); // stable by line: the read's first line
  const uint32_t line  = bfirst[blocks[g]] + static_cast<uint32_t>(k & 0xffffffffu);
  const uint32_t s = qs[line], e = qe[line];
  uf_put_events(ev, i, first && s < e, s, e);
}

// pass 2: endpoint keys of every line of the outlier blocks
__global__ __launch_bounds__(256) void k_uf_all_events(const uint32_t *blocks, const uint64_t *seg_off, uint32_t n_seg,
                                                       const uint32_t *bfirst, const uint32_t *qs, const uint32_t *qe,
                                                       uint64_t *ev) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= seg_off[n_seg]) return;
  const uint32_t g    = last_le(seg_off, 0, n_seg, i);
  const uint32_t line = bfirst[blocks[g]] + static_cast<uint32_t>(i - seg_off[g]);
  const uint32_t s = qs[line], e = qe[line];
  uf_put_events(ev, i, s < e, s, e);
}

// giant blocks, step 3: one wavefront per block sweeps its sorted endpoints 64 at a time (inclusive scan of +1 / -1);
// the maximum of the running depth after a start is the block's value
__global__ __launch_bounds__(256) void k_uf_sweep_max(const uint32_t *blocks, const uint64_t *seg_off, uint32_t n_seg,
                                                      const uint64_t *ev, uint32_t *val) {
  const uint32_t g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= n_seg) return;
  const int      lane = threadIdx.x & 63;
  const uint64_t e0 = 2 * seg_off[g], e1 = 2 * seg_off[g + 1];
  int32_t        carry = 0, m = 0;
  for (uint64_t t = e0; t < e1; t += 64) {
    const uint64_t i    = t + lane;
    const uint64_t k    = i < e1 ? ev[i] : 0;
    int32_t        x    = i < e1 ? ((k & 1) ? 1 : -1) : 0;
    for (int o = 1; o < 64; o <<= 1) {
      const int32_t y = __shfl_up(x, o);
      if (lane >= o) x += y;
    }
    const int32_t depth = carry + x;
    int32_t       c     = (i < e1 && (k & 1)) ? depth : 0;
    for (int o = 32; o > 0; o >>= 1) c = max(c, __shfl_xor(c, o));
    m = max(m, c);
    carry += __shfl(x, 63);
  }
  if (lane == 0) val[blocks[g]] = static_cast<uint32_t>(m);
}

__global__ __launch_bounds__(256) void k_uf_id_values(const uint32_t *last_block, uint32_t n_ids, const uint32_t *val,
                                                      uint32_t *id_val) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u < n_ids) id_val[u] = val[last_block[u]];
}

// pass 2: one thread per outlier block walks its sorted endpoints.  Coverage is constant between two distinct endpoint
// positions; runs of cov <= t of >= UF_RUN positions are fragments.  EMIT = false: count them; true: write them at
// frag_off[g] (in position order).
template <bool EMIT>
__global__ __launch_bounds__(256) void k_uf_runs(const uint32_t *blocks, const uint64_t *seg_off, uint32_t n_seg,
                                                 const uint32_t *bqlen, const uint64_t *ev, int64_t t, uint32_t *count,
                                                 const uint32_t *frag_off, uint2 *frags) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= n_seg) return;
  const uint64_t e1 = 2 * seg_off[g + 1];
  const uint32_t qlen = bqlen[blocks[g]];
  uint32_t       k = 0, at = EMIT ? frag_off[g] : 0;
  int64_t        depth = 0, run = -1; // run: start of the open run of good positions (-1: none)
  uint32_t       cur = 0;             // coverage is `depth` on [cur, next endpoint)
  auto           segment = [&](uint32_t a, uint32_t z) { // [a, z) with coverage depth
    if (depth <= t) {
      if (run < 0) run = a;
    } else if (run >= 0) {
      if (a - static_cast<uint32_t>(run) >= UF_RUN) {
        if (EMIT) frags[at + k] = make_uint2(static_cast<uint32_t>(run), a - 1);
        ++k;
      }
      run = -1;
    }
  };
  for (uint64_t i = 2 * seg_off[g]; i < e1;) {
    const uint32_t p = static_cast<uint32_t>(ev[i] >> 1);
    if (p > cur) segment(cur, p);
    for (; i < e1 && static_cast<uint32_t>(ev[i] >> 1) == p; ++i) depth += (ev[i] & 1) ? 1 : -1;
    cur = p;
  }
  if (qlen > cur) segment(cur, qlen);
  if (run >= 0 && qlen - static_cast<uint32_t>(run) >= UF_RUN) {
    if (EMIT) frags[at + k] = make_uint2(static_cast<uint32_t>(run), qlen - 1);
    ++k;
  }
  if (!EMIT) count[g] = k;
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_ufctx : msgpu::StageCtx {
  SeqCtxHold seq;
  int        open() { return msgpu_seq_create(device, &seq.p); }
};

struct msgpu_uf_result {
  msgpu_uf_stats    stats{};
  std::vector<char> text;
};

namespace {

inline bool uf_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r'); }

// The description line (text after '>', trailing whitespace removed) of the first record of every unitig id the PAF
// names: what the output's header of a normal block is.  A record is a line starting with '>' (seq_loader.cpp's FASTA
// rule), its id the description cut at the first whitespace.
int uf_descriptions(const char *path, const msgpu_uf *u, uint32_t n_ids, std::vector<std::string> &desc) {
  int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return MSGPU_E_IO;
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    return MSGPU_E_IO;
  }
  const size_t len  = static_cast<size_t>(st.st_size);
  const char  *data = nullptr;
  if (len) {
    void *m = mmap(nullptr, len, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m == MAP_FAILED) {
      close(fd);
      return MSGPU_E_IO;
    }
    data = static_cast<const char *>(m);
  }
  close(fd);
  desc.assign(n_ids, std::string());
  std::vector<char> seen(n_ids, 0);
  std::string       id;
  for (const char *q = data, *end = data + len; q < end;) {
    const void *nlp = memchr(q, '\n', static_cast<size_t>(end - q));
    const char *ls = q, *le = nlp ? static_cast<const char *>(nlp) : end;
    q = nlp ? le + 1 : end;
    if (*ls != '>') continue;
    const char *ds = ls + 1, *de = le;
    while (de > ds && uf_space(de[-1])) --de;
    const char *ie = ds;
    while (ie < de && !uf_space(*ie) && *ie) ++ie;
    id.assign(ds, ie);
    const uint32_t k = msgpu_uf_unitig_id(u, id.c_str());
    if (k < n_ids && !seen[k]) {
      seen[k] = 1;
      desc[k].assign(ds, de);
    }
  }
  if (data) munmap(const_cast<char *>(data), len);
  return MSGPU_OK;
}

} // namespace

extern "C" {

// numpy.percentile, method "linear": virtual index (n - 1) q, neighbours floor / floor + 1 (the last value at or beyond
// n - 1), numpy's lerp a + (b - a) t, or b - (b - a)(1 - t) for t >= 0.5.  Integer values: b - a is exact.
int msgpu_uf_quartiles(const uint32_t *values, size_t n, double *q1, double *q3, double *upper) {
  if (!values || !n || !q1 || !q3 || !upper) return MSGPU_E_ARG;
  try {
    std::vector<uint32_t> v(values, values + n);
    auto at = [&](size_t k) {
      std::nth_element(v.begin(), v.begin() + k, v.end());
      return static_cast<int64_t>(v[k]);
    };
    auto q = [&](double p) {
      const double vi   = static_cast<double>(n - 1) * p; // exact: p is 0.25 or 0.75
      const double prev = std::floor(vi);
      size_t       i0   = static_cast<size_t>(prev), i1 = i0 + 1;
      if (vi >= static_cast<double>(n - 1)) i0 = i1 = n - 1;
      const double  t = vi - prev;
      const int64_t a = at(i0), b = at(i1);
      const double  d = static_cast<double>(b - a);
      return t >= 0.5 ? static_cast<double>(b) - d * (1.0 - t) : static_cast<double>(a) + d * t;
    };
    *q1    = q(0.25);
    *q3    = q(0.75);
    *upper = *q3 + 1.5 * (*q3 - *q1);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  return MSGPU_OK;
}

int  msgpu_uf_create(int device, msgpu_ufctx **out) { return stage_create(device, out); }
void msgpu_uf_destroy(msgpu_ufctx *c) { stage_destroy(c); }

const char *msgpu_uf_last_error(const msgpu_ufctx *c) { return c ? c->err : "null context"; }
uint64_t    msgpu_uf_error_line(const msgpu_ufctx *c) { return c ? c->err_line : 0; }

int msgpu_uf_run(msgpu_ufctx *c, const msgpu_uf *u, const char *unitigs_path, uint32_t flags, msgpu_uf_result **out) {
  if (!c || !u || !unitigs_path || !out) return MSGPU_E_ARG;
  *out        = nullptr;
  c->err[0]   = 0;
  c->err_line = 0;
  msgpu_uf_tables tb;
  if (msgpu_uf_get_tables(u, &tb) != MSGPU_OK || !tb.n_lines) return MSGPU_E_ARG;
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  const uint32_t NB = tb.n_blocks, NI = tb.n_unitigs;
  std::unique_ptr<msgpu_uf_result> res;
  try {
    res.reset(new msgpu_uf_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  msgpu_uf_stats &S = res->stats;
  S.n_lines         = tb.n_lines;
  S.n_blocks        = NB;
  S.n_ids           = NI;

  // ---- the unitigs: bases to the store, ids, descriptions
  SeqFileHold f;
  int         rc = msgpu_seq_parse_upload(c->seq, 1, unitigs_path, 0, &f.f);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "unitigs %s: %s", unitigs_path, msgpu_seq_last_error(c->seq));
    return rc;
  }
  std::vector<uint32_t>    rec_ids, rec_of;
  std::vector<std::string> desc;
  try {
    const uint32_t b = stage_first_records(f, [&](const char *name) { return msgpu_uf_unitig_id(u, name); }, NI, tb.block_unitig, NB,
                                           rec_ids, rec_of);
    if (b != STAGE_NONE) { // a unitig the FASTA lacks: the first block naming it
      c->err_line = static_cast<uint64_t>(tb.block_first[b]) + 1;
      snprintf(c->err, sizeof(c->err), "unitig %s (PAF line %llu) is not in %s", msgpu_uf_unitig_name(u, tb.block_unitig[b]),
               static_cast<unsigned long long>(c->err_line), unitigs_path);
      return MSGPU_E_IDS;
    }
    rc = uf_descriptions(unitigs_path, u, NI, desc);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (rc != MSGPU_OK) return rc;
  rc = msgpu_seq_set_ids(c->seq, 1, f, rec_ids.data(), NI);
  if (rc == MSGPU_OK && (flags & MSGPU_UF_PACKED)) rc = msgpu_seq_pack_store(c->seq, 1);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "sequence store: %s", msgpu_seq_last_error(c->seq));
    return rc;
  }
  S.load_ms = wall.ms();

  // ---- width classes
  std::vector<uint32_t> wave, group, giant;
  std::vector<uint64_t> giant_off(1, 0);
  for (uint32_t b = 0; b < NB; ++b) {
    const uint32_t n = tb.block_n[b];
    if (n <= UF_WAVE) wave.push_back(b);
    else if (n <= UF_GROUP) group.push_back(b);
    else {
      giant.push_back(b);
      giant_off.push_back(giant_off.back() + n);
    }
  }
  S.n_wave  = static_cast<uint32_t>(wave.size());
  S.n_group = static_cast<uint32_t>(group.size());
  S.n_giant = static_cast<uint32_t>(giant.size());

  hipStream_t st = c->stream;
  StageClock  clock(st);
  DevArena    D;
  uint32_t *d_qs, *d_qe, *d_rd, *d_bfirst, *d_bn, *d_bqlen, *d_last, *d_val, *d_idval, *d_cls;
  const size_t NL = tb.n_lines;
  STAGE_HIP(c, D.get(&d_qs, NL));
  STAGE_HIP(c, D.get(&d_qe, NL));
  STAGE_HIP(c, D.get(&d_rd, NL));
  STAGE_HIP(c, D.get(&d_bfirst, NB));
  STAGE_HIP(c, D.get(&d_bn, NB));
  STAGE_HIP(c, D.get(&d_bqlen, NB));
  STAGE_HIP(c, D.get(&d_last, NI));
  STAGE_HIP(c, D.get(&d_val, NB));
  STAGE_HIP(c, D.get(&d_idval, NI));
  STAGE_HIP(c, D.get(&d_cls, NB)); // the block lists of the classes, back to back: wave, group, giant
  uint64_t *d_goff;
  STAGE_HIP(c, D.get(&d_goff, giant_off.size()));
  std::vector<uint32_t> cls;
  cls.reserve(NB);
  cls.insert(cls.end(), wave.begin(), wave.end());
  cls.insert(cls.end(), group.begin(), group.end());
  cls.insert(cls.end(), giant.begin(), giant.end());
  STAGE_HIP(c, clock.begin(&S.upload_ms));
  STAGE_HIP(c, hipMemcpyAsync(d_qs, tb.line_qs, NL * 4, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_qe, tb.line_qe, NL * 4, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_rd, tb.line_read, NL * 4, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_bfirst, tb.block_first, NB * 4ull, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_bn, tb.block_n, NB * 4ull, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_bqlen, tb.block_qlen, NB * 4ull, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_last, tb.unitig_last_block, NI * 4ull, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_cls, cls.data(), NB * 4ull, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_goff, giant_off.data(), giant_off.size() * 8, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, clock.begin(&S.pass1_ms)); // (from the same point of the stream)

  // rocprim's segmented radix sort, on the arena's temporary buffer
  auto sort = [&](const uint64_t *in, uint64_t *outk, size_t n, uint32_t nseg, const uint64_t *off, int end_bit) -> hipError_t {
    return stage_rocprim(D, [&](void *tmp, size_t &bytes) {
      return rocprim::segmented_radix_sort_keys(tmp, bytes, in, outk, static_cast<unsigned int>(n), nseg, off, off + 1, 0, end_bit, st);
    });
  };

  // ---- pass 1
  if (!wave.empty())
    hipLaunchKernelGGL(k_uf_wave, dim3((S.n_wave + 3) / 4), dim3(256), 0, st, d_cls, S.n_wave, d_bfirst, d_bn, d_qs, d_qe,
                       d_rd, d_val);
  if (!group.empty())
    hipLaunchKernelGGL(k_uf_group, dim3(S.n_group), dim3(256), 0, st, d_cls + S.n_wave, d_bfirst, d_bn, d_qs, d_qe, d_rd,
                       d_val);
  STAGE_HIP(c, hipGetLastError());
  const uint64_t GL = giant_off.back();
  if (GL) {
    if (GL >= 0x7fffffffull) {
      snprintf(c->err, sizeof(c->err), "more than 2^31 - 1 lines in giant blocks");
      return MSGPU_E_ARG;
    }
    const uint32_t *d_gb = d_cls + S.n_wave + S.n_group;
    uint64_t *d_k0, *d_k1, *d_e0, *d_e1;
    STAGE_HIP(c, D.get(&d_k0, GL));
    STAGE_HIP(c, D.get(&d_k1, GL));
    STAGE_HIP(c, D.get(&d_e0, 2 * GL));
    STAGE_HIP(c, D.get(&d_e1, 2 * GL));
    uint64_t *d_eoff; // the endpoint segments: twice the line segments
    std::vector<uint64_t> eoff(giant_off.size());
    for (size_t i = 0; i < eoff.size(); ++i) eoff[i] = 2 * giant_off[i];
    STAGE_HIP(c, D.get(&d_eoff, eoff.size()));
    STAGE_HIP(c, hipMemcpyAsync(d_eoff, eoff.data(), eoff.size() * 8, hipMemcpyHostToDevice, st));
    const uint32_t grid = grid256(GL);
    hipLaunchKernelGGL(k_uf_read_keys, dim3(grid), dim3(256), 0, st, d_gb, d_goff, S.n_giant, d_bfirst, d_rd, d_k0);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, sort(d_k0, d_k1, GL, S.n_giant, d_goff, 64));
    hipLaunchKernelGGL(k_uf_dedup_events, dim3(grid), dim3(256), 0, st, d_gb, d_goff, S.n_giant, d_bfirst, d_qs, d_qe, d_k1,
                       d_e0);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, sort(d_e0, d_e1, 2 * GL, S.n_giant, d_eoff, 33));
    hipLaunchKernelGGL(k_uf_sweep_max, dim3((S.n_giant + 3) / 4), dim3(256), 0, st, d_gb, d_goff, S.n_giant, d_e1, d_val);
    STAGE_HIP(c, hipGetLastError());
  }
  hipLaunchKernelGGL(k_uf_id_values, dim3(grid256(NI)), dim3(256), 0, st, d_last, NI, d_val, d_idval);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  std::vector<uint32_t> idval(NI);
  STAGE_HIP(c, hipMemcpyAsync(idval.data(), d_idval, NI * 4ull, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));

  // ---- quartiles, outliers (host: one value per id)
  rc = msgpu_uf_quartiles(idval.data(), NI, &S.q1, &S.q3, &S.upper);
  if (rc != MSGPU_OK) return rc;
  std::vector<uint32_t> outl;
  std::vector<uint64_t> ooff(1, 0);
  for (uint32_t b = 0; b < NB; ++b)
    if (static_cast<double>(idval[tb.block_unitig[b]]) > S.upper) {
      outl.push_back(b);
      ooff.push_back(ooff.back() + tb.block_n[b]);
    }
  const uint32_t NO = static_cast<uint32_t>(outl.size());
  S.n_outliers      = NO;

  // ---- pass 2: count, scan, emit
  std::vector<uint32_t> fcount(NO), foff(NO + 1, 0);
  std::vector<uint2>    frags;
  STAGE_HIP(c, clock.begin(&S.pass2_ms));
  if (NO) {
    const uint64_t OL = ooff.back();
    if (OL >= 0x3fffffffull) {
      snprintf(c->err, sizeof(c->err), "more than 2^30 - 1 lines in outlier blocks");
      return MSGPU_E_ARG;
    }
    uint32_t *d_ob, *d_cnt, *d_foff;
    uint64_t *d_ooff, *d_e0, *d_e1, *d_eoff;
    STAGE_HIP(c, D.get(&d_ob, NO));
    STAGE_HIP(c, D.get(&d_cnt, NO));
    STAGE_HIP(c, D.get(&d_foff, NO));
    STAGE_HIP(c, D.get(&d_ooff, NO + 1));
    STAGE_HIP(c, D.get(&d_eoff, NO + 1));
    STAGE_HIP(c, D.get(&d_e0, 2 * OL));
    STAGE_HIP(c, D.get(&d_e1, 2 * OL));
    std::vector<uint64_t> eoff(NO + 1);
    for (uint32_t i = 0; i <= NO; ++i) eoff[i] = 2 * ooff[i];
    STAGE_HIP(c, hipMemcpyAsync(d_ob, outl.data(), NO * 4ull, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_ooff, ooff.data(), (NO + 1) * 8ull, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_eoff, eoff.data(), (NO + 1) * 8ull, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_uf_all_events, dim3(grid256(OL)), dim3(256), 0, st, d_ob, d_ooff, NO,
                       d_bfirst, d_qs, d_qe, d_e0);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, sort(d_e0, d_e1, 2 * OL, NO, d_eoff, 33));
    const int64_t t = static_cast<int64_t>(std::floor(S.q3)); // cov <= q3 <=> cov <= floor(q3) for an integer cov
    hipLaunchKernelGGL(k_uf_runs<false>, dim3(grid256(NO)), dim3(256), 0, st, d_ob, d_ooff, NO, d_bqlen, d_e1, t,
                       d_cnt, nullptr, nullptr);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, hipMemcpyAsync(fcount.data(), d_cnt, NO * 4ull, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipStreamSynchronize(st));
    for (uint32_t i = 0; i < NO; ++i) foff[i + 1] = foff[i] + fcount[i];
    S.n_fragments = foff[NO];
    for (uint32_t i = 0; i < NO; ++i) S.n_rescued += fcount[i] ? 1 : 0;
    if (S.n_fragments) {
      uint2 *d_frag;
      STAGE_HIP(c, D.get(&d_frag, S.n_fragments));
      STAGE_HIP(c, hipMemcpyAsync(d_foff, foff.data(), NO * 4ull, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_uf_runs<true>, dim3(grid256(NO)), dim3(256), 0, st, d_ob, d_ooff, NO, d_bqlen, d_e1, t,
                         nullptr, d_foff, d_frag);
      STAGE_HIP(c, hipGetLastError());
      frags.resize(S.n_fragments);
      STAGE_HIP(c, hipMemcpyAsync(frags.data(), d_frag, S.n_fragments * sizeof(uint2), hipMemcpyDeviceToHost, st));
    }
  }
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));

  // ---- output plan: per block in PAF order the whole record or the fragments
  FastaOut F;
  try {
    auto add = [&](uint32_t id, uint64_t start, uint64_t stop, const char *h, size_t hn) { // bases [start, stop) of id
      const uint32_t i = rec_of[id];
      const uint64_t L = msgpu_seq_length(f, i);
      const uint64_t e = std::min(stop, L), s = std::min(start, e);
      F.add(msgpu_seq_offset(f, i) + s, e - s, MSGPU_COPY_ILLUMINA, h, hn);
    };
    std::string h;
    char        buf[96];
    for (uint32_t b = 0, o = 0; b < NB; ++b) {
      const uint32_t id = tb.block_unitig[b];
      if (o < NO && outl[o] == b) {
        for (uint32_t k = 0; k < fcount[o]; ++k) {
          const uint2 fr = frags[foff[o] + k];
          h.assign(">").append(msgpu_uf_unitig_name(u, id));
          snprintf(buf, sizeof(buf), "_%u %u %u %u\n", k, fr.y - fr.x + 1, fr.x, fr.y);
          h.append(buf);
          add(id, fr.x, static_cast<uint64_t>(fr.y) + 1, h.data(), h.size());
        }
        ++o;
      } else {
        h.assign(">").append(desc[id]).append("\n");
        add(id, 0, ~0ull, h.data(), h.size());
      }
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  S.n_records  = F.recs.size();
  S.bases      = F.raw;
  S.text_bytes = F.text;
  if ((rc = F.emit(c, D, clock, nullptr, &S.plan_ms, &S.gather_ms, &S.format_ms, &S.copy_ms, res->text)) != MSGPU_OK) return rc;
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;
  S.wall_ms = wall.ms();
  *out      = res.release();
  return MSGPU_OK;
}

int msgpu_uf_result_stats(const msgpu_uf_result *r, msgpu_uf_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

const char *msgpu_uf_result_text(const msgpu_uf_result *r, uint64_t *len) {
  if (len) *len = r ? r->text.size() : 0;
  return r && !r->text.empty() ? r->text.data() : "";
}

void msgpu_uf_result_free(msgpu_uf_result *r) { delete r; }

} // extern "C"
