// msgpu_scrub.hip -- the read scrubber (include/msgpu.h, "read scrubber"; DESIGN.md section "Read scrubber").
//
// Read graph: the edges are the pairs of counting lines inside a chunk.  Pair p of the pair space (chunk after chunk, inside
// a chunk by (later line j, earlier line i)) is numbered in the order the script would add it, so p itself is the edge's
// time.  k_scrub_pairs writes (low node, high node) -> p, a stable radix sort brings the pairs of one edge together with
// the first one in front, a scan compacts the first ones and each gives two directed entries (node, p) -> other node; a
// second sort by (node, p) is the CSR with every row in insertion order.
// Batching is rule 2 on the host (msgpu_scrub_plan_create) and does not depend on the fold, so all batches are known before
// the first fold launch.
// Fold: every surviving read-to-read line gives two directed entries, sorted once by (owner, partner) with the lines of a
// group in file order (stable sort).  A group's state (S, E, D) lives at its first entry.  Per batch k_scrub_stamp marks the
// subset and k_scrub_fold gives every subset node a wavefront whose lanes take the node's groups: a lane whose partner is
// in the subset walks the group's lines on top of the state.
// Union: a centre node leaves the graph, so its groups are final after its batch and ONE union over all nodes at the end is
// the union of every batch.  A node's slots are its anchor ranges and its entries (a slot that is no group's first entry,
// or whose group has no state, holds a sentinel that sorts last); segmented sort, count, scan, emit (the pattern of
// k_uf_runs).  Output: one gather and one FASTA wrapping launch on the sequence store of msgpu_seq.hip.
//
// Kernel rules: vector stores only; no inline asm.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <new>
#include <string>
#include <vector>

#include "msgpu.h"
#include "msgpu_stage.h"

namespace msgpu {

constexpr uint32_t SC_NONE     = 0xffffffffu;
constexpr uint64_t SC_SENTINEL = ~0ull;
constexpr int32_t  SC_NEAR     = 500; // two lines of a pair join when an end of one is nearer than this to the other's
constexpr int64_t  SC_TRIM     = 200; // bases dropped at both ends of a read

// pair p -> its chunk and its two lines i < j (p = pair_off[chunk] + j (j - 1) / 2 + i)
__global__ __launch_bounds__(256) void k_scrub_pairs(const uint64_t *pair_off, uint32_t n_chunks, const uint32_t *chunk_first,
                                                     const uint32_t *hit_node, uint64_t *keys, uint32_t *ord) {
  const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= pair_off[n_chunks]) return;
  const uint32_t c     = last_le(pair_off, 0, n_chunks, p);
  const uint64_t local = p - pair_off[c];
  uint64_t       j     = static_cast<uint64_t>((1.0 + sqrt(1.0 + 8.0 * static_cast<double>(local))) * 0.5);
  while (j > 1 && j * (j - 1) / 2 > local) --j;
  while ((j + 1) * j / 2 <= local) ++j;
  const uint64_t i = local - j * (j - 1) / 2;
  const uint32_t f = chunk_first[c];
  const uint32_t a = hit_node[f + i], b = hit_node[f + j];
  keys[p] = (static_cast<uint64_t>(min(a, b)) << 32) | max(a, b);
  ord[p]  = static_cast<uint32_t>(p);
}

__global__ __launch_bounds__(256) void k_scrub_first(const uint64_t *keys, uint64_t n, uint32_t *flag) {
  const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p < n) flag[p] = (p == 0 || keys[p] != keys[p - 1]) ? 1u : 0u;
}

// the first pair of every edge -> (low, time) -> high and (high, time) -> low
__global__ __launch_bounds__(256) void k_scrub_directed(const uint64_t *keys, const uint32_t *ord, const uint32_t *flag,
                                                        const uint32_t *pos, uint64_t n, uint64_t *dkey, uint32_t *dval) {
  const uint64_t p = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= n || !flag[p]) return;
  const uint64_t e  = 2ull * pos[p];
  const uint32_t lo = static_cast<uint32_t>(keys[p] >> 32), hi = static_cast<uint32_t>(keys[p]);
  dkey[e]     = (static_cast<uint64_t>(lo) << 32) | ord[p];
  dval[e]     = hi;
  dkey[e + 1] = (static_cast<uint64_t>(hi) << 32) | ord[p];
  dval[e + 1] = lo;
}

// row_off[x] = the first of the n sorted keys whose high half is >= x, for x = 0 .. n_nodes
__global__ __launch_bounds__(256) void k_scrub_rows(const uint64_t *keys, uint64_t n, uint32_t n_nodes, uint64_t *row_off) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x > n_nodes) return;
  uint64_t lo = 0, hi = n; // keys[< lo] are below x, keys[>= hi] are not
  while (lo < hi) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((keys[mid] >> 32) < x) lo = mid + 1;
    else hi = mid;
  }
  row_off[x] = lo;
}

// surviving line l -> entries 2 l (owner = column 0's node) and 2 l + 1 (owner = column 5's node)
__global__ __launch_bounds__(256) void k_scrub_entries(const uint32_t *ava_a, const uint32_t *ava_b, uint64_t n_ava,
                                                       uint64_t *keys, uint32_t *idx) {
  const uint64_t m = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (m >= 2 * n_ava) return;
  const uint32_t a = ava_a[m >> 1], b = ava_b[m >> 1];
  keys[m] = (m & 1) ? ((static_cast<uint64_t>(b) << 32) | a) : ((static_cast<uint64_t>(a) << 32) | b);
  idx[m]  = static_cast<uint32_t>(m);
}

__global__ __launch_bounds__(256) void k_scrub_stamp(const uint32_t *subset, uint32_t n, uint32_t batch, uint32_t *stamp) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) stamp[subset[i]] = batch;
}

// one wavefront per subset node, one lane per group of the node (a group = a run of equal keys; its state is kept at the
// run's first entry); 4 nodes per 256-thread workgroup
__global__ __launch_bounds__(256) void k_scrub_fold(const uint32_t *subset, uint32_t n, uint32_t batch, const uint32_t *stamp,
                                                    const uint64_t *ent_off, const uint64_t *keys, const uint32_t *idx,
                                                    const int32_t *sa, const int32_t *ea, const int32_t *sb,
                                                    const int32_t *eb, const uint32_t *strand, int32_t *st_s, int32_t *st_e,
                                                    uint32_t *st_d) {
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= n) return; // (the whole wavefront leaves together)
  const uint32_t lane = threadIdx.x & 63;
  const uint32_t x    = subset[w];
  const uint64_t e0 = ent_off[x], e1 = ent_off[x + 1];
  for (uint64_t i = e0 + lane; i < e1; i += 64) {
    const uint64_t k = keys[i];
    if (i > e0 && keys[i - 1] == k) continue;                 // not a group's first entry
    if (stamp[static_cast<uint32_t>(k)] != batch) continue;   // the partner is outside the subset
    int32_t  S = st_s[i], E = st_e[i];
    uint32_t D = st_d[i];
    for (uint64_t j = i; j < e1 && keys[j] == k; ++j) {
      const uint32_t m = idx[j], l = m >> 1;
      const int32_t  s = (m & 1) ? sb[l] : sa[l], e = (m & 1) ? eb[l] : ea[l];
      const uint32_t d = strand[l];
      if (D == SC_NONE) {
        S = s;
        E = e;
        D = d;
      } else if (d == D && (abs(S - e) < SC_NEAR || abs(s - E) < SC_NEAR)) {
        S = min(s, S);
        E = max(e, E);
      }
    }
    st_s[i] = S;
    st_e[i] = E;
    st_d[i] = D;
  }
}

__global__ __launch_bounds__(256) void k_scrub_slot_off(const uint64_t *anc_off, const uint64_t *ent_off, uint32_t n_nodes,
                                                        uint64_t *slot_off) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x <= n_nodes) slot_off[x] = anc_off[x] + ent_off[x];
}

// slot t of node x: its anchor ranges, then one slot per entry ((s << 32) | e, both non-negative: sorts as the pair)
__global__ __launch_bounds__(256) void k_scrub_intervals(const uint64_t *slot_off, const uint64_t *anc_off,
                                                         const uint64_t *ent_off, uint32_t n_nodes, const int32_t *anc_s,
                                                         const int32_t *anc_e, const uint64_t *keys, const int32_t *st_s,
                                                         const int32_t *st_e, const uint32_t *st_d, uint64_t *iv) {
  const uint64_t t = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= slot_off[n_nodes]) return;
  const uint32_t x     = last_le(slot_off, 0, n_nodes, t);
  const uint64_t local = t - slot_off[x], na = anc_off[x + 1] - anc_off[x];
  uint64_t       v = SC_SENTINEL;
  if (local < na) {
    const uint64_t h = anc_off[x] + local;
    v = (static_cast<uint64_t>(static_cast<uint32_t>(anc_s[h])) << 32) | static_cast<uint32_t>(anc_e[h]);
  } else {
    const uint64_t e0 = ent_off[x], i = e0 + (local - na);
    if ((i == e0 || keys[i - 1] != keys[i]) && st_d[i] != SC_NONE)
      v = (static_cast<uint64_t>(static_cast<uint32_t>(st_s[i])) << 32) | static_cast<uint32_t>(st_e[i]);
  }
  iv[t] = v;
}

// one thread per node walks its sorted ranges and merges left to right.  EMIT = false: count the covered ranges; true:
// write them at rec_off[x].
template <bool EMIT>
__global__ __launch_bounds__(256) void k_scrub_merge(const uint64_t *slot_off, uint32_t n_nodes, const uint64_t *iv,
                                                     uint32_t *count, const uint32_t *rec_off, int2 *ranges) {
  const uint32_t x = blockIdx.x * 256 + threadIdx.x;
  if (x >= n_nodes) return;
  uint32_t k = 0;
  const uint32_t at = EMIT ? rec_off[x] : 0;
  int32_t  cs = 0, ce = 0;
  bool     have = false;
  for (uint64_t t = slot_off[x]; t < slot_off[x + 1]; ++t) {
    const uint64_t v = iv[t];
    if (v == SC_SENTINEL) break;
    const int32_t s = static_cast<int32_t>(v >> 32), e = static_cast<int32_t>(v & 0xffffffffu);
    if (have && cs <= e && s <= ce) {
      cs = min(s, cs);
      ce = max(e, ce);
    } else {
      if (have) {
        if (EMIT) ranges[at + k] = make_int2(cs, ce);
        ++k;
      }
      cs   = s;
      ce   = e;
      have = true;
    }
  }
  if (have) {
    if (EMIT) ranges[at + k] = make_int2(cs, ce);
    ++k;
  }
  if (!EMIT) count[x] = k;
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_scrubctx : msgpu::StageCtx {
  SeqCtxHold seq;
  int        open() { return msgpu_seq_create(device, &seq.p); }
};

struct msgpu_scrub_result {
  msgpu_scrub_stats     stats{};
  std::vector<char>     text;
  std::vector<uint64_t> row_off;
  std::vector<uint32_t> adj;
};

namespace {

bool ends_with(const char *s, const char *tail) {
  const size_t n = strlen(s), m = strlen(tail);
  return n >= m && memcmp(s + n - m, tail, m) == 0;
}

} // namespace

extern "C" {

int  msgpu_scrub_create(int device, msgpu_scrubctx **out) { return stage_create(device, out); }
void msgpu_scrub_destroy(msgpu_scrubctx *c) { stage_destroy(c); }

const char *msgpu_scrub_last_error(const msgpu_scrubctx *c) { return c ? c->err : "null context"; }
uint64_t    msgpu_scrub_error_line(const msgpu_scrubctx *c) { return c ? c->err_line : 0; }

int msgpu_scrub_run(msgpu_scrubctx *c, const msgpu_scrub *s, const char *reads_path, uint32_t subset_size,
                    msgpu_scrub_result **out) {
  if (!c || !s || !reads_path || !out || !subset_size) return MSGPU_E_ARG;
  *out        = nullptr;
  c->err[0]   = 0;
  c->err_line = 0;
  msgpu_scrub_tables tb;
  if (msgpu_scrub_get_tables(s, &tb) != MSGPU_OK || !tb.n_nodes) return MSGPU_E_ARG;
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  const uint32_t N = tb.n_nodes, NC = tb.n_chunks;
  const uint64_t H = tb.n_hits, A = tb.n_ava, M = 2 * A;
  std::unique_ptr<msgpu_scrub_result> res;
  try {
    res.reset(new msgpu_scrub_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  msgpu_scrub_stats &S = res->stats;
  S.n_nodes            = N;
  S.n_hits             = H;
  S.n_ava              = A;

  // ---- the reads: bases to the nanopore store; every node needs a record (the first of its name)
  const int      is_fastq = (ends_with(reads_path, "fa") || ends_with(reads_path, "fasta")) ? 0 : 1;
  SeqFileHold    f;
  int            rc       = msgpu_seq_parse_upload(c->seq, 0, reads_path, is_fastq, &f.f);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "reads %s: %s", reads_path, msgpu_seq_last_error(c->seq));
    return rc;
  }
  std::vector<uint32_t> rec_ids, rec_of;
  uint32_t              x = STAGE_NONE;
  try {
    x = stage_first_records(f, [&](const char *name) { return msgpu_scrub_node_id(s, name); }, N, nullptr, N, rec_ids, rec_of);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (x != STAGE_NONE) { // nodes are numbered by their first line: the first missing one has the smallest line
    c->err_line = static_cast<uint64_t>(tb.node_line[x]) + 1;
    snprintf(c->err, sizeof(c->err), "read %.200s (anchor PAF line %llu) is not in the reads file", msgpu_scrub_node_name(s, x),
             static_cast<unsigned long long>(c->err_line));
    return MSGPU_E_IDS;
  }
  rc = msgpu_seq_set_ids(c->seq, 0, f, rec_ids.data(), N);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "sequence store: %s", msgpu_seq_last_error(c->seq));
    return rc;
  }
  S.load_ms = wall.ms();

  // ---- host tables of the device steps: the pair space, the anchor ranges by node
  std::vector<uint64_t> pair_off, anc_off;
  std::vector<int32_t>  anc_s, anc_e;
  try {
    pair_off.assign(static_cast<size_t>(NC) + 1, 0);
    for (uint32_t k = 0; k < NC; ++k) {
      const uint64_t n = tb.chunk_n[k];
      pair_off[k + 1]  = pair_off[k] + n * (n - 1) / 2;
    }
    anc_off.assign(static_cast<size_t>(N) + 1, 0);
    for (uint64_t h = 0; h < H; ++h) ++anc_off[tb.hit_node[h] + 1];
    for (uint32_t x = 0; x < N; ++x) anc_off[x + 1] += anc_off[x];
    anc_s.resize(H);
    anc_e.resize(H);
    std::vector<uint64_t> at(anc_off.begin(), anc_off.end() - 1);
    for (uint64_t h = 0; h < H; ++h) {
      const uint64_t k = at[tb.hit_node[h]]++;
      anc_s[k]         = tb.hit_s[h];
      anc_e[k]         = tb.hit_e[h];
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  const uint64_t P = pair_off[NC], T = H + M;
  S.n_pairs        = P;
  if (P >= 0x7fffffffull || M >= 0x7fffffffull || T >= 0x7fffffffull) {
    snprintf(c->err, sizeof(c->err), "more than 2^31 - 1 pairs (%llu), directed entries (%llu) or interval slots (%llu)",
             static_cast<unsigned long long>(P), static_cast<unsigned long long>(M), static_cast<unsigned long long>(T));
    return MSGPU_E_ARG;
  }

  hipStream_t st = c->stream;
  StageClock  clock(st);
  DevArena    D;

  // ---- read graph
  uint64_t *d_row_off;
  STAGE_HIP(c, D.get(&d_row_off, static_cast<size_t>(N) + 1));
  STAGE_HIP(c, clock.begin(&S.graph_ms));
  uint64_t E2 = 0; // directed entries of the graph = 2 x edges
  try {
    res->row_off.assign(static_cast<size_t>(N) + 1, 0);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (P) {
    uint64_t *d_pair_off, *d_k0, *d_k1;
    uint32_t *d_cfirst, *d_hnode, *d_o0, *d_o1, *d_flag, *d_pos;
    STAGE_HIP(c, D.get(&d_pair_off, pair_off.size()));
    STAGE_HIP(c, D.get(&d_cfirst, NC));
    STAGE_HIP(c, D.get(&d_hnode, H));
    STAGE_HIP(c, D.get(&d_k0, P));
    STAGE_HIP(c, D.get(&d_k1, P));
    STAGE_HIP(c, D.get(&d_o0, P));
    STAGE_HIP(c, D.get(&d_o1, P));
    STAGE_HIP(c, D.get(&d_flag, P));
    STAGE_HIP(c, D.get(&d_pos, P));
    STAGE_HIP(c, hipMemcpyAsync(d_pair_off, pair_off.data(), pair_off.size() * 8, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_cfirst, tb.chunk_first, NC * 4ull, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_hnode, tb.hit_node, H * 4ull, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_scrub_pairs, dim3(grid256(P)), dim3(256), 0, st, d_pair_off, NC, d_cfirst, d_hnode, d_k0, d_o0);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_sort_pairs(D, st, d_k0, d_k1, d_o0, d_o1, P)); // stable: of the pairs of one edge the earliest comes first
    hipLaunchKernelGGL(k_scrub_first, dim3(grid256(P)), dim3(256), 0, st, d_k1, P, d_flag);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_scan(D, st, d_flag, d_pos, P));
    uint32_t last[2] = {0, 0};
    STAGE_HIP(c, hipMemcpyAsync(&last[0], d_pos + (P - 1), 4, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(&last[1], d_flag + (P - 1), 4, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipStreamSynchronize(st));
    E2 = 2ull * (static_cast<uint64_t>(last[0]) + last[1]);
    uint64_t *d_dk0, *d_dk1;
    uint32_t *d_dv0, *d_dv1;
    STAGE_HIP(c, D.get(&d_dk0, E2));
    STAGE_HIP(c, D.get(&d_dk1, E2));
    STAGE_HIP(c, D.get(&d_dv0, E2));
    STAGE_HIP(c, D.get(&d_dv1, E2));
    hipLaunchKernelGGL(k_scrub_directed, dim3(grid256(P)), dim3(256), 0, st, d_k1, d_o1, d_flag, d_pos, P, d_dk0, d_dv0);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_sort_pairs(D, st, d_dk0, d_dk1, d_dv0, d_dv1, E2));
    hipLaunchKernelGGL(k_scrub_rows, dim3(grid256(static_cast<uint64_t>(N) + 1)), dim3(256), 0, st, d_dk1, E2, N, d_row_off);
    STAGE_HIP(c, hipGetLastError());
    try {
      res->adj.resize(E2);
    } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
    STAGE_HIP(c, hipMemcpyAsync(res->row_off.data(), d_row_off, (static_cast<size_t>(N) + 1) * 8, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(res->adj.data(), d_dv1, E2 * 4, hipMemcpyDeviceToHost, st));
  }
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  S.n_edges = E2 / 2;

  // ---- batches (host)
  const StageTimer         batching;
  msgpu_scrub_plan        *plan_raw = nullptr;
  msgpu_scrub_plan_tables  pt{};
  {
    std::vector<uint32_t> by_name;
    try {
      by_name.resize(N);
    } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
    msgpu_scrub_name_order(s, by_name.data());
    uint32_t bad = SC_NONE;
    rc = msgpu_scrub_plan_create(N, by_name.data(), res->row_off.data(), res->adj.data(), subset_size, &plan_raw, &bad);
    if (rc == MSGPU_E_LAYOUT) {
      snprintf(c->err, sizeof(c->err),
               "the batch that starts at read %.200s has an empty centre with subset size %u: every node of the subset has a "
               "neighbour outside it",
               msgpu_scrub_node_name(s, bad), subset_size);
      return rc;
    }
    if (rc != MSGPU_OK) return rc;
  }
  struct FreeBatches {
    msgpu_scrub_plan *p;
    ~FreeBatches() { msgpu_scrub_plan_free(p); }
  } free_batches{plan_raw};
  msgpu_scrub_plan_get(plan_raw, &pt);
  const uint32_t NB  = pt.n_batches;
  const uint64_t NS  = pt.subset_off[NB];
  S.n_batches        = NB;
  S.n_subset_total   = NS;
  S.batch_ms         = batching.ms();

  // ---- fold
  uint64_t *d_ent_off, *d_ek = nullptr;
  int32_t  *d_st_s = nullptr, *d_st_e = nullptr;
  uint32_t *d_st_d = nullptr;
  STAGE_HIP(c, D.get(&d_ent_off, static_cast<size_t>(N) + 1));
  STAGE_HIP(c, clock.begin(&S.fold_ms));
  if (M) {
    uint64_t *d_ek0;
    uint32_t *d_a, *d_b, *d_strand, *d_ei0, *d_ei, *d_stamp, *d_subset;
    int32_t  *d_sa, *d_ea, *d_sb, *d_eb;
    STAGE_HIP(c, D.get(&d_a, A));
    STAGE_HIP(c, D.get(&d_b, A));
    STAGE_HIP(c, D.get(&d_strand, A));
    STAGE_HIP(c, D.get(&d_sa, A));
    STAGE_HIP(c, D.get(&d_ea, A));
    STAGE_HIP(c, D.get(&d_sb, A));
    STAGE_HIP(c, D.get(&d_eb, A));
    STAGE_HIP(c, D.get(&d_ek0, M));
    STAGE_HIP(c, D.get(&d_ek, M));
    STAGE_HIP(c, D.get(&d_ei0, M));
    STAGE_HIP(c, D.get(&d_ei, M));
    STAGE_HIP(c, D.get(&d_st_s, M));
    STAGE_HIP(c, D.get(&d_st_e, M));
    STAGE_HIP(c, D.get(&d_st_d, M));
    STAGE_HIP(c, D.get(&d_stamp, N));
    STAGE_HIP(c, D.get(&d_subset, NS));
    STAGE_HIP(c, hipMemcpyAsync(d_a, tb.ava_a, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_b, tb.ava_b, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_strand, tb.ava_strand, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_sa, tb.ava_sa, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_ea, tb.ava_ea, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_sb, tb.ava_sb, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_eb, tb.ava_eb, A * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_subset, pt.subset, NS * 4, hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemsetAsync(d_stamp, 0xff, N * 4ull, st));
    STAGE_HIP(c, hipMemsetAsync(d_st_d, 0xff, M * 4, st));
    STAGE_HIP(c, hipMemsetAsync(d_st_s, 0, M * 4, st));
    STAGE_HIP(c, hipMemsetAsync(d_st_e, 0, M * 4, st));
    hipLaunchKernelGGL(k_scrub_entries, dim3(grid256(M)), dim3(256), 0, st, d_a, d_b, A, d_ek0, d_ei0);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_sort_pairs(D, st, d_ek0, d_ek, d_ei0, d_ei, M)); // stable: a group's lines stay in file order
    hipLaunchKernelGGL(k_scrub_rows, dim3(grid256(static_cast<uint64_t>(N) + 1)), dim3(256), 0, st, d_ek, M, N, d_ent_off);
    STAGE_HIP(c, hipGetLastError());
    for (uint32_t b = 0; b < NB; ++b) {
      const uint32_t  n   = static_cast<uint32_t>(pt.subset_off[b + 1] - pt.subset_off[b]);
      const uint32_t *sub = d_subset + pt.subset_off[b];
      hipLaunchKernelGGL(k_scrub_stamp, dim3(grid256(n)), dim3(256), 0, st, sub, n, b, d_stamp);
      hipLaunchKernelGGL(k_scrub_fold, dim3((n + 3) / 4), dim3(256), 0, st, sub, n, b, d_stamp, d_ent_off, d_ek, d_ei, d_sa,
                         d_ea, d_sb, d_eb, d_strand, d_st_s, d_st_e, d_st_d);
      STAGE_HIP(c, hipGetLastError());
    }
  } else {
    STAGE_HIP(c, hipMemsetAsync(d_ent_off, 0, (static_cast<size_t>(N) + 1) * 8, st));
  }
  STAGE_HIP(c, clock.end());

  // ---- union over all nodes
  uint64_t *d_anc_off, *d_slot_off, *d_iv0, *d_iv1;
  int32_t  *d_anc_s, *d_anc_e;
  uint32_t *d_cnt, *d_rec_off;
  STAGE_HIP(c, D.get(&d_anc_off, static_cast<size_t>(N) + 1));
  STAGE_HIP(c, D.get(&d_slot_off, static_cast<size_t>(N) + 1));
  STAGE_HIP(c, D.get(&d_anc_s, H));
  STAGE_HIP(c, D.get(&d_anc_e, H));
  STAGE_HIP(c, D.get(&d_iv0, T));
  STAGE_HIP(c, D.get(&d_iv1, T));
  STAGE_HIP(c, D.get(&d_cnt, N));
  STAGE_HIP(c, D.get(&d_rec_off, N));
  STAGE_HIP(c, clock.begin(&S.union_ms));
  STAGE_HIP(c, hipMemcpyAsync(d_anc_off, anc_off.data(), anc_off.size() * 8, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_anc_s, anc_s.data(), H * 4, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_anc_e, anc_e.data(), H * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_scrub_slot_off, dim3(grid256(static_cast<uint64_t>(N) + 1)), dim3(256), 0, st, d_anc_off, d_ent_off, N,
                     d_slot_off);
  hipLaunchKernelGGL(k_scrub_intervals, dim3(grid256(T)), dim3(256), 0, st, d_slot_off, d_anc_off, d_ent_off, N, d_anc_s,
                     d_anc_e, d_ek, d_st_s, d_st_e, d_st_d, d_iv0);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_rocprim(D, [&](void *tmp, size_t &bytes) {
    return rocprim::segmented_radix_sort_keys(tmp, bytes, d_iv0, d_iv1, static_cast<unsigned int>(T), N, d_slot_off, d_slot_off + 1, 0, 64,
                                              st);
  }));
  hipLaunchKernelGGL(k_scrub_merge<false>, dim3(grid256(N)), dim3(256), 0, st, d_slot_off, N, d_iv1, d_cnt, nullptr, nullptr);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan(D, st, d_cnt, d_rec_off, N));
  std::vector<uint32_t> rec_off, cnt;
  std::vector<int2>     ranges;
  try {
    rec_off.resize(N);
    cnt.resize(N);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, hipMemcpyAsync(rec_off.data(), d_rec_off, N * 4ull, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(cnt.data(), d_cnt, N * 4ull, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));
  const uint64_t NR = static_cast<uint64_t>(rec_off[N - 1]) + cnt[N - 1];
  S.n_intervals     = T;
  int2 *d_ranges;
  STAGE_HIP(c, D.get(&d_ranges, NR));
  hipLaunchKernelGGL(k_scrub_merge<true>, dim3(grid256(N)), dim3(256), 0, st, d_slot_off, N, d_iv1, nullptr, d_rec_off,
                     d_ranges);
  STAGE_HIP(c, hipGetLastError());
  try {
    ranges.resize(NR);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (NR) STAGE_HIP(c, hipMemcpyAsync(ranges.data(), d_ranges, NR * sizeof(int2), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));

  // ---- output plan: batch after batch, the centre nodes by id, a node's covered ranges in order
  FastaOut F;
  try {
    F.pieces.reserve(NR);
    F.recs.reserve(NR);
    std::string h;
    char        buf[32];
    for (uint64_t k = 0; k < pt.centre_off[NB]; ++k) {
      const uint32_t x    = pt.centre[k];
      const uint32_t i    = rec_of[x];
      const int64_t  L    = static_cast<int64_t>(msgpu_seq_length(f, i));
      const char    *name = msgpu_scrub_node_name(s, x);
      for (uint32_t r = 0; r < cnt[x]; ++r) {
        const int2    cr = ranges[rec_off[x] + r];
        const int64_t lo = std::max<int64_t>(cr.x, SC_TRIM);
        const int64_t hi = std::min<int64_t>(cr.y, static_cast<int64_t>(tb.node_length[x]) - SC_TRIM); // >= 0: length >= 200
        const int64_t e  = std::min<int64_t>(hi + 1, L), b = std::min<int64_t>(lo, L);
        h.assign(">").append(name);
        snprintf(buf, sizeof(buf), "_%u\n", r);
        h.append(buf);
        F.add(msgpu_seq_offset(f, i) + static_cast<uint64_t>(b), e > b ? static_cast<uint64_t>(e - b) : 0, 0, h.data(), h.size());
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

int msgpu_scrub_result_stats(const msgpu_scrub_result *r, msgpu_scrub_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

const char *msgpu_scrub_result_text(const msgpu_scrub_result *r, uint64_t *len) {
  if (len) *len = r ? r->text.size() : 0;
  return r && !r->text.empty() ? r->text.data() : "";
}

int msgpu_scrub_result_graph(const msgpu_scrub_result *r, const uint64_t **row_off, const uint32_t **adj) {
  if (!r || !row_off || !adj) return MSGPU_E_ARG;
  *row_off = r->row_off.data();
  *adj     = r->adj.data();
  return MSGPU_OK;
}

void msgpu_scrub_result_free(msgpu_scrub_result *r) { delete r; }

} // extern "C"
