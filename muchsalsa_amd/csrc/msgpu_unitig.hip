// msgpu_unitig.hip -- the short-read unitig assembly (include/msgpu.h, "short-read unitig assembly").
//
// The count is the k-mer filter's (msgpu_kmer_shared.h) with least = min_count and no histogram: the solid k-mers come out
// as one ascending key array with their counts and an open-addressing table of indices over it.  A k-mer is its rank r in
// that array, an oriented node is 2 r + strand (strand 0: the canonical string, strand 1: its reverse complement; a
// self-complementary k-mer has strand 0 only).
//   k_ug_adj     one byte per k-mer: which of the 4 successors (bits 0..3) and 4 predecessors (bits 4..7) of the canonical
//                string are alive.  The first fill makes 8 look-ups; behind a tip round only the bits still set are asked again
//   k_ug_tips    a thread per dead-end oriented node walks at most `limit` nodes, one look-up per step; a tip's k-mers are
//                marked in an array of their own, so the round sees a snapshot
//   k_ug_apply   marks -> alive; the number removed goes into the scalar block, read back by the publication protocol
//   k_ug_forks   rule 9 (on request): the oriented nodes with two or more successors, from the byte alone, compacted by ballot
//   k_ug_bubbles rule 9: a quad of lanes per fork walks its up to four branches (at most `bubble` look-ups each), compares
//                them by shuffles inside the quad and marks the losers; k_ug_apply and k_ug_adj close the round as behind tips
//   k_ug_next    rule 5: next[o] = the node o is joined to.  prev(o) = next[o ^ 1] ^ 1: the mirror chain is the same joins
//   k_ug_double  pointer doubling towards the chain head: ptr[o] and the distance from it, ping-pong buffers.  A round counts
//                the nodes that do not point at a head yet; when that number stops falling, what is left lies on cycles
//   k_ug_cyc_*   cycles: a min-reduction by doubling finds the smallest oriented node, the cycle is cut in front of it
//                and doubled again as a linear chain
//   k_ug_heads   the heads that are emitted (rule 5's mirror choice), with their first k-mer; rocPRIM sorts them by it
//   k_ug_cover   coverage: 64-bit atomics per unitig
//   k_ug_write   every node writes one base at offset + distance + k - 1, the head writes its k bases and the closing byte
//   k_ug_links   rule 10 (on request): a quad of lanes per unitig end, lane c resolves the unitig behind the successor by
//                base c (one look-up) and appends the link's 64-bit key unless the mirror link is the smaller; rocPRIM
//                sorts the keys
//   k_ug_link_*  rule 10: the link table and the byte length of every L line; behind a 64-bit scan a lane per link writes
//                its line into the GFA text, where k_ug_write has put the segments' bases
// No kernel loops over a unitig or over rounds: the longest loops are `limit` <= trim steps (k_ug_tips), `bubble` steps
// (k_ug_bubbles), k bases and the ten digits of an id.
// Kernel rules: vector stores and vector atomics only; no inline asm.
#include <hip/hip_runtime.h>

#include <deque>
#include <memory>
#include <new>
#include <string>

#include "msgpu_internal.h"
#include "msgpu_kmer_shared.h"

namespace msgpu {

constexpr uint32_t UG_NONE = 0xffffffffu;

template <class K> struct UgGraph { // the solid set as the kernels see it
  const K        *keys;             // ascending
  const uint32_t *slots;            // the table over them
  uint32_t        mask, n;
  int             k, top;           // top = 2 (k - 1)
  K               kmask;
};

// the reverse complement (ug_rev2, and ug_rc of a key of W words: msgpu_kmer_wide.h)
__device__ inline uint64_t ug_rc(uint64_t x, int k) { return (~ug_rev2(x)) >> (64 - 2 * k); }
__device__ inline kf_u128 ug_rc(kf_u128 x, int k) {
  const kf_u128 f = (static_cast<kf_u128>(ug_rev2(static_cast<uint64_t>(x))) << 64) | ug_rev2(static_cast<uint64_t>(x >> 64));
  return (~f) >> (128 - 2 * k);
}
__device__ inline uint32_t ug_rev4(uint32_t b) { return ((b & 1) << 3) | ((b & 2) << 1) | ((b & 4) >> 1) | ((b & 8) >> 3); }

template <class K> __device__ inline K ug_seq(const UgGraph<K> &g, uint32_t o) {
  const K x = g.keys[o >> 1];
  return (o & 1) ? ug_rc(x, g.k) : x;
}
// the oriented node of the string t, or UG_NONE when its k-mer is not in the set
template <class K> __device__ inline uint32_t ug_node(const UgGraph<K> &g, K t) {
  const K        r = ug_rc(t, g.k);
  const uint32_t j = kf_find(g.keys, g.slots, g.mask, t < r ? t : r);
  return j == KF_EMPTY ? UG_NONE : 2 * j + (t > r ? 1u : 0u);
}
template <class K> __device__ inline K ug_succ(const UgGraph<K> &g, K s, uint32_t c) { return ((s << 2) | static_cast<K>(c)) & g.kmask; }
template <class K> __device__ inline K ug_pred(const UgGraph<K> &g, K s, uint32_t c) { return (s >> 2) | (static_cast<K>(c) << g.top); }
// the same two steps on a key of W words: carried shifts by 2, the mask's top word, the first base's place in the top word
template <int W> __device__ inline KfWide<W> ug_succ(const UgGraph<KfWide<W>> &g, KfWide<W> s, uint32_t c) {
  s.push_low(c, g.kmask.w[W - 1]);
  return s;
}
template <int W> __device__ inline KfWide<W> ug_pred(const UgGraph<KfWide<W>> &g, KfWide<W> s, uint32_t c) {
  s.push_high(c, g.top - 64 * (W - 1));
  return s;
}
// the successor / predecessor bits of an oriented node from its k-mer's byte: the reverse strand's successor by base c is
// the mirror of the canonical string's predecessor by base 3 - c
__device__ inline uint32_t ug_out(uint32_t byte, uint32_t o) { return (o & 1) ? ug_rev4(byte >> 4) : (byte & 0xfu); }
__device__ inline uint32_t ug_in(uint32_t byte, uint32_t o) { return (o & 1) ? ug_rev4(byte & 0xfu) : (byte >> 4); }

template <class K, bool FIRST>
__global__ __launch_bounds__(256) void k_ug_adj(UgGraph<K> g, const uint8_t *alive, uint8_t *adj) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= g.n) return;
  if (!alive[r]) {
    adj[r] = 0;
    return;
  }
  const K        s = g.keys[r];
  const uint32_t ask = FIRST ? 0xffu : adj[r];
  uint32_t       b = 0;
  for (uint32_t c = 0; c < 4; ++c) {
    if (ask & (1u << c)) {
      const uint32_t t = ug_node(g, ug_succ(g, s, c));
      if (t != UG_NONE && alive[t >> 1]) b |= 1u << c;
    }
    if (ask & (16u << c)) {
      const uint32_t t = ug_node(g, ug_pred(g, s, c));
      if (t != UG_NONE && alive[t >> 1]) b |= 16u << c;
    }
  }
  adj[r] = static_cast<uint8_t>(b);
}

// rule 4, one round: alive / adj are the snapshot, mark receives the tips' k-mers
template <class K>
__global__ __launch_bounds__(256) void k_ug_tips(UgGraph<K> g, const uint8_t *alive, const uint8_t *adj, uint32_t limit, uint8_t *mark) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 2ull * g.n) return;
  const uint32_t o = static_cast<uint32_t>(i);
  if (!alive[o >> 1] || ug_in(adj[o >> 1], o)) return;
  const K first = ug_seq(g, o);
  if ((o & 1) && first == g.keys[o >> 1]) return; // a self-complementary k-mer is one node
  K        s = first;
  uint32_t cur = o, len = 1;
  bool     tip = false;
  for (;;) { // at most `limit` turns
    const uint32_t out = ug_out(adj[cur >> 1], cur);
    if (__popc(out) != 1) break;
    const K        ts = ug_succ(g, s, static_cast<uint32_t>(__ffs(out)) - 1);
    const uint32_t t = ug_node(g, ts);
    if (t == UG_NONE) break; // (the byte said it is there)
    if (__popc(ug_in(adj[t >> 1], t)) >= 2) {
      tip = true;
      break;
    }
    if (len == limit) break;
    s   = ts;
    cur = t;
    ++len;
  }
  if (!tip) return;
  s   = first;
  cur = o;
  for (uint32_t j = 0;; ++j) { // the same `len` nodes again
    mark[cur >> 1] = 1;
    if (j + 1 == len) break;
    s   = ug_succ(g, s, static_cast<uint32_t>(__ffs(ug_out(adj[cur >> 1], cur))) - 1);
    cur = ug_node(g, s);
    if (cur == UG_NONE) break;
  }
}

__global__ __launch_bounds__(256) void k_ug_apply(uint32_t n, uint8_t *alive, uint8_t *mark, kf_ull *removed) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  const bool     go = r < n && mark[r];
  if (go) {
    alive[r] = 0;
    mark[r]  = 0;
  }
  wave_count(go, removed);
}

// rule 9, the forks of a round: the oriented nodes with two or more successors, compacted into a list (any order)
template <class K>
__global__ __launch_bounds__(256) void k_ug_forks(UgGraph<K> g, const uint8_t *alive, const uint8_t *adj, uint32_t *forks, uint64_t cap,
                                                  kf_ull *cursor) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const uint32_t o = static_cast<uint32_t>(i);
  bool           take = false;
  if (i < 2ull * g.n && alive[o >> 1] && __popc(ug_out(adj[o >> 1], o)) >= 2)
    take = !(o & 1) || ug_rc(g.keys[o >> 1], g.k) != g.keys[o >> 1]; // a self-complementary k-mer is one node
  const uint64_t slot = wave_append(take, cursor);
  if (take && slot < cap) forks[slot] = o;
}

// rule 9, one round: a quad of lanes per fork, lane c walks the branch entered by base c (at most `bubble` look-ups) and
// keeps (merge, length, sum of counts); the quad compares its branches by shuffles, and every losing lane walks its branch
// again to mark it.  alive / adj are the snapshot, mark receives the losers' k-mers
template <class K>
__global__ __launch_bounds__(256) void k_ug_bubbles(UgGraph<K> g, const uint8_t *adj, const uint32_t *count, const uint32_t *forks,
                                                    uint32_t n_forks, uint32_t bubble, uint8_t *mark, kf_ull *n_bubbles,
                                                    kf_ull *n_branches) {
  const uint64_t f = (static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x) >> 2;
  const uint32_t c = threadIdx.x & 3;
  uint32_t       u = 0, first = UG_NONE, merge = UG_NONE, len = 0;
  kf_ull         sum = 0;
  K              su = 0, bs = 0, ms = 0;
  if (f < n_forks) {
    u  = forks[f];
    su = ug_seq(g, u);
    if (ug_out(adj[u >> 1], u) & (1u << c)) {
      bs    = ug_succ(g, su, c);
      first = ug_node(g, bs);
    }
  }
  if (first != UG_NONE && __popc(ug_in(adj[first >> 1], first)) == 1) {
    K        s = bs;
    uint32_t cur = first;
    len = 1;
    sum = count[first >> 1];
    for (;;) { // at most `bubble` turns
      const uint32_t out = ug_out(adj[cur >> 1], cur);
      if (__popc(out) != 1) break;
      const K        ts = ug_succ(g, s, static_cast<uint32_t>(__ffs(out)) - 1);
      const uint32_t t = ug_node(g, ts);
      if (t == UG_NONE) break; // (the byte said it is there)
      if (__popc(ug_in(adj[t >> 1], t)) >= 2) {
        merge = t;
        ms    = ts;
        break;
      }
      if (len == bubble) break;
      s   = ts;
      cur = t;
      ++len;
      sum += count[t >> 1];
    }
  }
  // (b), (c) inside the quad: the branches of this fork with my merge, and whether one of them beats mine
  const bool has = merge != UG_NONE;
  bool       others = false, beaten = false;
  for (int x = 1; x < 4; ++x) {
    const uint32_t om = __shfl_xor(merge, x), ol = __shfl_xor(len, x);
    const kf_ull   os = __shfl_xor(sum, x);
    if (has && om == merge) {
      others = true;
      const kf_ull theirs = os * len, mine = sum * ol; // below 2^56: a count has 32 bits, a branch at most 4096 k-mers
      if (theirs > mine || (theirs == mine && (c ^ static_cast<uint32_t>(x)) < c)) beaten = true;
    }
  }
  // the fork and the merge are two k-mers, and the bubble is judged from the side whose fork is the smaller string
  const bool     judged = has && others && (merge >> 1) != (u >> 1) && su < ug_rc(ms, g.k);
  const bool     lose = judged && beaten;
  const uint64_t won = __ballot(judged && !beaten), lost = __ballot(lose);
  if ((threadIdx.x & 63) == 0) {
    if (won) atomicAdd(n_bubbles, static_cast<kf_ull>(__popcll(won)));
    if (lost) atomicAdd(n_branches, static_cast<kf_ull>(__popcll(lost)));
  }
  if (!lose) return;
  K        s = bs;
  uint32_t cur = first;
  for (uint32_t j = 0;; ++j) { // the same `len` nodes again
    mark[cur >> 1] = 1;
    if (j + 1 == len) break;
    s   = ug_succ(g, s, static_cast<uint32_t>(__ffs(ug_out(adj[cur >> 1], cur))) - 1);
    cur = ug_node(g, s);
    if (cur == UG_NONE) break;
  }
}

// an oriented node that exists: its k-mer is alive, and strand 1 only where the k-mer is not its own reverse complement
template <class K> __device__ inline bool ug_valid(const UgGraph<K> &g, const uint8_t *alive, uint32_t o, K s) {
  return alive[o >> 1] && !((o & 1) && s == g.keys[o >> 1]);
}

// rule 5's joins
template <class K>
__global__ __launch_bounds__(256) void k_ug_next(UgGraph<K> g, const uint8_t *alive, const uint8_t *adj, uint32_t *next) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 2ull * g.n) return;
  const uint32_t o = static_cast<uint32_t>(i);
  uint32_t       nx = UG_NONE;
  if (alive[o >> 1]) {
    const K        s = ug_seq(g, o);
    const uint32_t out = ug_out(adj[o >> 1], o);
    if (s != ug_rc(s, g.k) && __popc(out) == 1) {
      const K        ts = ug_succ(g, s, static_cast<uint32_t>(__ffs(out)) - 1);
      const uint32_t t = ug_node(g, ts);
      if (t != UG_NONE && (t >> 1) != (o >> 1) && ts != ug_rc(ts, g.k) && __popc(ug_in(adj[t >> 1], t)) == 1) nx = t;
    }
  }
  next[o] = nx;
}

// ptr = the previous node (a head points at itself, a node that does not exist at UG_NONE), dist = 1 (a head: 0)
template <class K>
__global__ __launch_bounds__(256) void k_ug_chain_init(UgGraph<K> g, const uint8_t *alive, const uint32_t *next, uint32_t *ptr,
                                                       uint32_t *dist) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 2ull * g.n) return;
  const uint32_t o = static_cast<uint32_t>(i);
  const bool     valid = alive[o >> 1] && ug_valid(g, alive, o, ug_seq(g, o));
  const uint32_t back = next[o ^ 1];
  ptr[o]  = !valid ? UG_NONE : (back == UG_NONE ? o : (back ^ 1));
  dist[o] = (valid && back != UG_NONE) ? 1u : 0u;
}

// one round of pointer doubling; *open counts the nodes that do not point at a head behind it
__global__ __launch_bounds__(256) void k_ug_double(uint64_t n2, const uint32_t *next, const uint32_t *ptr_in, const uint32_t *dist_in,
                                                   uint32_t *ptr_out, uint32_t *dist_out, kf_ull *open) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool           is_open = false;
  if (i < n2) {
    const uint32_t o = static_cast<uint32_t>(i);
    uint32_t       q = ptr_in[o], d = dist_in[o];
    if (q != UG_NONE && next[q ^ 1] != UG_NONE) { // q is no head
      d += dist_in[q];
      q = ptr_in[q];
      is_open = next[q ^ 1] != UG_NONE;
    }
    ptr_out[o]  = q;
    dist_out[o] = d;
  }
  wave_count(is_open, open);
}

// what still points at no head lies on a cycle: back = the previous node, low = the node itself
__global__ __launch_bounds__(256) void k_ug_cyc_init(uint64_t n2, const uint32_t *next, const uint32_t *ptr, uint8_t *cyc,
                                                     uint32_t *back, uint32_t *low) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n2) return;
  const uint32_t o = static_cast<uint32_t>(i), q = ptr[o];
  const bool     on = q != UG_NONE && next[q ^ 1] != UG_NONE;
  cyc[o]  = on;
  back[o] = on ? (next[o ^ 1] ^ 1) : UG_NONE;
  low[o]  = o;
}

// one round of the min-reduction: low = the smallest oriented node (as a 2k-bit number) of the 2^round nodes behind
template <class K>
__global__ __launch_bounds__(256) void k_ug_cyc_min(UgGraph<K> g, const uint8_t *cyc, const uint32_t *back_in, const uint32_t *low_in,
                                                    uint32_t *back_out, uint32_t *low_out) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 2ull * g.n) return;
  const uint32_t o = static_cast<uint32_t>(i);
  if (!cyc[o]) return;
  const uint32_t q = back_in[o], a = low_in[o], b = low_in[q];
  low_out[o]  = (a == b || ug_seq(g, a) < ug_seq(g, b)) ? a : b;
  back_out[o] = back_in[q];
}

// the cycle is cut in front of its smallest node, which becomes a head (low[head] then holds the node in front of it, the
// cut chain's last: the mirror cycle is cut at its own smallest node, not at the mirror of this one); its nodes start the
// doubling again
__global__ __launch_bounds__(256) void k_ug_cyc_cut(uint64_t n2, const uint8_t *cyc, uint32_t *low, uint32_t *next, uint32_t *ptr,
                                                    uint32_t *dist) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n2) return;
  const uint32_t o = static_cast<uint32_t>(i);
  if (!cyc[o]) return;
  const bool head = low[o] == o;
  ptr[o]  = head ? o : (next[o ^ 1] ^ 1);
  dist[o] = head ? 0u : 1u;
  if (head) { // (only this thread reads next[o ^ 1] and low[o])
    low[o]      = next[o ^ 1] ^ 1;
    next[o ^ 1] = UG_NONE;
  }
}

// the heads that are emitted.  WRITE = false counts them.
template <class K, bool WRITE>
__global__ __launch_bounds__(256) void k_ug_heads(UgGraph<K> g, const uint32_t *next, const uint32_t *ptr, K *first, uint32_t *head,
                                                  uint64_t cap, kf_ull *cursor) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool           take = false;
  K              s = 0;
  const uint32_t o = static_cast<uint32_t>(i);
  if (i < 2ull * g.n && ptr[o] == o && next[o ^ 1] == UG_NONE) {
    s = ug_seq(g, o);
    const uint32_t m = ptr[o ^ 1]; // the mirror chain's head (UG_NONE: a self-complementary k-mer, which exists once)
    take = m == UG_NONE || s < ug_seq(g, m);
  }
  const uint64_t slot = wave_append(take, cursor);
  if (WRITE && take && slot < cap) {
    first[slot] = s;
    head[slot]  = o;
  }
}

// per unitig in output order: its k-mers and whether it is a cycle; unit_of[head] = its id
__global__ __launch_bounds__(256) void k_ug_units(uint32_t n_units, const uint32_t *head, const uint32_t *ptr, const uint32_t *dist,
                                                  const uint8_t *cyc, const uint32_t *cyc_last, uint32_t *unit_of, uint32_t *n_kmers,
                                                  uint8_t *cyclic) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_units) return;
  const uint32_t h = head[u], m = ptr[h ^ 1];
  const bool     round = cyc && cyc[h];
  unit_of[h] = u;
  // a linear chain: the mirror head's mirror is its last node; a cut cycle: k_ug_cyc_cut kept it
  n_kmers[u] = round ? dist[cyc_last[h]] + 1 : (m == UG_NONE ? 1u : dist[m ^ 1] + 1);
  cyclic[u]  = round;
}

__global__ __launch_bounds__(256) void k_ug_cover(uint64_t n2, const uint32_t *ptr, const uint32_t *unit_of, const uint32_t *count,
                                                  kf_ull *cover) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n2) return;
  const uint32_t h = ptr[i];
  if (h == UG_NONE) return;
  const uint32_t u = unit_of[h];
  if (u != UG_NONE) atomicAdd(&cover[u], static_cast<kf_ull>(count[i >> 1]));
}

// `close` is the byte behind a sequence: the '\n' of a FASTA record, the '\t' of a GFA segment line
template <class K>
__global__ __launch_bounds__(256) void k_ug_write(UgGraph<K> g, const uint32_t *ptr, const uint32_t *dist, const uint32_t *unit_of,
                                                  const uint32_t *n_kmers, const uint64_t *seq_off, uint8_t *text, uint64_t cap,
                                                  uint8_t close) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 2ull * g.n) return;
  const uint32_t o = static_cast<uint32_t>(i), h = ptr[o];
  if (h == UG_NONE) return;
  const uint32_t u = unit_of[h];
  if (u == UG_NONE) return;
  const K        s = ug_seq(g, o);
  const uint64_t at = seq_off[u];
  const uint32_t d = dist[o];
  if (d) {
    const uint64_t w = at + d + g.k - 1;
    if (w < cap) text[w] = "ACGT"[kf_base(s, 0)];
    return;
  }
  if (at + n_kmers[u] + g.k > cap) return;
  for (int j = 0; j < g.k; ++j) text[at + j] = "ACGT"[kf_base(s, g.k - 1 - j)];
  text[at + n_kmers[u] + g.k - 1] = close;
}

// ---- rule 10: the links between the unitig ends

// a link as a 64-bit key in rule 10 (d)'s order: from id (31 bits), from orientation, to id (31 bits), to orientation
__device__ inline uint64_t ug_link_key(uint32_t from, uint32_t from_rev, uint32_t to, uint32_t to_rev) {
  return (static_cast<uint64_t>(from) << 33) | (static_cast<uint64_t>(from_rev) << 32) | (static_cast<uint64_t>(to) << 1) | to_rev;
}

// Rule 10 (b), (c): a quad of lanes per unitig end (end e = 2 id + orientation; the - end of a unitig that is one
// self-complementary k-mer does not exist), lane c asks for the successor by base c of the end's last node, resolves the
// unitig that starts there and keeps the link unless its mirror is the smaller tuple.  sc: links (the cursor), adjacencies,
// self-mirrored links, ends without a link, targets that are no unitig's first node -- five words side by side
template <class K>
__global__ __launch_bounds__(256) void k_ug_links(UgGraph<K> g, const uint8_t *adj, const uint32_t *ptr, const uint32_t *dist,
                                                  const uint32_t *unit_of, const uint32_t *head, const uint32_t *n_kmers,
                                                  const uint8_t *cyc, const uint32_t *cyc_last, uint32_t n_units, uint64_t *keys,
                                                  uint64_t cap, kf_ull *sc) {
  const uint64_t e = (static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x) >> 2;
  const uint32_t c = threadIdx.x & 3;
  bool           live = false, has = false, keep = false, own_mirror = false, lost = false;
  uint32_t       out = 0;
  uint64_t       own = 0;
  if (e < 2ull * n_units) {
    const uint32_t u = static_cast<uint32_t>(e >> 1), rev = static_cast<uint32_t>(e & 1), h = head[u], m = ptr[h ^ 1];
    const bool     single = m == UG_NONE; // one self-complementary k-mer: + only
    live = !(rev && single);
    if (live) {
      const uint32_t end = rev ? (h ^ 1) : ((cyc && cyc[h]) ? cyc_last[h] : (single ? h : (m ^ 1)));
      out = ug_out(adj[end >> 1], end);
      if (out & (1u << c)) {
        has = true;
        const uint32_t v = ug_node(g, ug_succ(g, ug_seq(g, end), c));
        uint32_t       to = UG_NONE, to_rev = 0;
        bool           to_single = false;
        if (v != UG_NONE) { // (the byte said it is there)
          const uint32_t p = ptr[v], q = ptr[v ^ 1];
          if (p == v && unit_of[v] != UG_NONE) { // the head of an emitted chain
            to        = unit_of[v];
            to_single = q == UG_NONE;
          } else if (q != UG_NONE && unit_of[q] != UG_NONE && dist[v ^ 1] + 1 == n_kmers[unit_of[q]]) { // the mirror of its last node
            to     = unit_of[q];
            to_rev = 1;
          }
        }
        lost = to == UG_NONE;
        if (!lost) {
          own = ug_link_key(u, rev, to, to_rev);
          const uint64_t mirror = ug_link_key(to, to_rev ^ 1, u, rev ^ 1);
          own_mirror = single || to_single || own == mirror; // a unitig without a - has no mirror link
          keep       = own_mirror || own < mirror;
        }
      }
    }
  }
  const uint64_t slot = wave_append(keep, sc);
  if (keep && slot < cap) keys[slot] = own;
  wave_count(has, sc + 1);
  wave_count(own_mirror, sc + 2);
  wave_count(live && c == 0 && !out, sc + 3);
  wave_count(lost, sc + 4);
}

__device__ inline uint32_t ug_digits(uint32_t x) { // decimal digits of x
  uint32_t d = 1;
  for (uint64_t p = 10; x >= p; p *= 10) ++d;
  return d;
}
// x in d decimal digits, the last at text[end - 1]
__device__ inline void ug_put_decimal(uint8_t *text, uint64_t end, uint32_t x, uint32_t d) {
  for (uint32_t j = 0; j < d; ++j, x /= 10) text[end - 1 - j] = static_cast<uint8_t>('0' + x % 10);
}

// Rule 10 (e): the sorted keys as the link table and as the byte length of each L line, "L\t<from>\t<o>\t<to>\t<o>\t<k-1>M\n";
// thread n writes the zero behind the lengths (stage_scan_total)
__global__ __launch_bounds__(256) void k_ug_link_lens(const uint64_t *keys, uint64_t n, uint32_t overlap_digits, msgpu_ug_link *links,
                                                      uint32_t *len) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    len[i] = 0;
    return;
  }
  const uint64_t key = keys[i];
  const uint32_t from = static_cast<uint32_t>(key >> 33), to = static_cast<uint32_t>(key >> 1) & 0x7fffffffu;
  links[i] = msgpu_ug_link{from, to, static_cast<uint8_t>((key >> 32) & 1), static_cast<uint8_t>(key & 1), 0};
  len[i]   = 10 + ug_digits(from) + ug_digits(to) + overlap_digits;
}

// a lane per link writes its line at base + off[i]
__global__ __launch_bounds__(256) void k_ug_link_write(const msgpu_ug_link *links, const uint64_t *off, uint64_t n, uint32_t overlap,
                                                       uint32_t overlap_digits, uint64_t base, uint8_t *text, uint64_t cap) {
  const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  const msgpu_ug_link l = links[i];
  const uint32_t      df = ug_digits(l.from), dt = ug_digits(l.to);
  uint64_t            at = base + off[i];
  if (at + 10 + df + dt + overlap_digits > cap) return;
  text[at]     = 'L';
  text[at + 1] = '\t';
  at += 2 + df;
  ug_put_decimal(text, at, l.from, df);
  text[at]     = '\t';
  text[at + 1] = l.from_rev ? '-' : '+';
  text[at + 2] = '\t';
  at += 3 + dt;
  ug_put_decimal(text, at, l.to, dt);
  text[at]     = '\t';
  text[at + 1] = l.to_rev ? '-' : '+';
  text[at + 2] = '\t';
  at += 3 + overlap_digits;
  ug_put_decimal(text, at, overlap, overlap_digits);
  text[at]     = 'M';
  text[at + 1] = '\n';
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_ugctx : msgpu::StageCtx {
  ScalarBlock sc;
  uint32_t    bubble = 0; // rule 9's parameter (msgpu_ug_set_bubbles)
  bool        graph = false; // rule 10 (msgpu_ug_set_graph)
  bool        wide = false; // k up to 128 (msgpu_ug_set_wide)
  int         open() { return sc.create(); }
};

struct msgpu_ug_result {
  msgpu_ug_stats               stats{};
  std::vector<msgpu_ug_round>  rounds;
  msgpu_ug_bubble_stats              bubble_stats{};
  std::vector<msgpu_ug_bubble_round> bubble_rounds;
  std::vector<msgpu_ug_unitig> units;
  std::vector<uint64_t>        first_words; // first_w words per unitig, least significant first (msgpu_ug_result_first_kmers)
  uint32_t                     first_w = 1;
  uint64_t                     bytes_peak = 0; // of the run's arena (msgpu_ug_result_peak_bytes)
  char                        *all = nullptr; // page-locked
  uint64_t                     all_len = 0;
  std::string                  cut;
  msgpu_ug_graph_stats         graph_stats{};
  std::vector<msgpu_ug_link>   links;
  char                        *gfa = nullptr; // page-locked; rule 10
  uint64_t                     gfa_len = 0;
  ~msgpu_ug_result() {
    if (all) (void)hipHostFree(all);
    if (gfa) (void)hipHostFree(gfa);
  }
};

namespace {

enum { UG_SC_REMOVED = SC_TOTAL_A, UG_SC_OPEN = SC_TOTAL_B, UG_SC_UNITS = SC_TOTAL_C,
       UG_SC_FORKS = SC_NBIG, UG_SC_BUBBLES = SC_NALIVE, UG_SC_BRANCHES = SC_IXFLAGS }; // (the last three lie side by side)
static_assert(UG_SC_BUBBLES == UG_SC_FORKS + 1 && UG_SC_BRANCHES == UG_SC_FORKS + 2, "one memset zeroes the bubble rounds' counters");
// rule 10: k_ug_links' five counters side by side; the bytes of the L lines come back in UG_SC_OPEN
enum { UG_SC_LINKS = SC_BIGSTATS, UG_SC_ADJACENCIES, UG_SC_SELF_MIRROR, UG_SC_DEAD_ENDS, UG_SC_LOST_LINKS };
static_assert(UG_SC_LOST_LINKS == SC_CLS && SC_CLS < SC_COUNT, "five free words of the scalar block");
constexpr char UG_GFA_HEADER[] = "H\tVN:Z:1.0\n";

inline hipError_t ug_zero_scalar(msgpu_ugctx *c, int slot) { return hipMemsetAsync(c->sc.d + slot, 0, 8, c->stream); }

// everything behind the format check, for one key width
template <class K>
int ug_stage(msgpu_ugctx *c, DevArena &D, const KfFile *F, const uint8_t *d_dropped, const msgpu_ug_params &prm, uint32_t bubble,
             bool graph, uint64_t budget, msgpu_ug_result *res) {
  msgpu_ug_stats &S = res->stats;
  hipStream_t     st = c->stream;
  StageClock      clock(st);
  const int      k = prm.k;
  const uint64_t n_first = F[0].n_lines >> 2, n_reads = n_first + (F[1].n_lines >> 2);
  const KfIn     in{{F[0].d, F[1].d}, {F[0].ls, F[1].ls}, n_first, n_reads, k, d_dropped};

  // ---- count: the k-mer filter's, least = min_count, no histogram
  kf_ull *d_cur;
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
             static_cast<kf_ull>(S.n_windows), sizeof(K), static_cast<kf_ull>(per_key), static_cast<kf_ull>(budget), KF_BINS,
             free_b);
    return MSGPU_E_NOMEM;
  }
  S.n_partitions      = parts.P;
  S.largest_partition = parts.largest;
  std::vector<KfChunk<K>> chunks;
  uint64_t                kept = 0;
  rc = kf_count<K>(c, D, clock, in, pre, parts, k, prm.min_count, KfCountMs{&S.extract_ms, &S.sort_ms, &S.runs_ms, &S.select_ms},
                   d_cur, [](const uint32_t *, uint32_t) { return MSGPU_OK; }, chunks, S.n_distinct, kept);
  if (rc != MSGPU_OK) return rc;
  if (kept >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "%llu solid k-mers; the limit is 2^31 - 1", static_cast<kf_ull>(kept));
    return MSGPU_E_ARG;
  }
  S.n_solid = kept;
  const uint32_t n = static_cast<uint32_t>(kept);
  const uint64_t n2 = 2ull * n;
  // what the rest keeps resident: keys, counts, the table, three bytes per k-mer, eight words per oriented node
  STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
  const uint64_t graph_bytes = n * (2 * (sizeof(K) + 4ull) + 8 + 3) + n2 * (8 * 4ull + 1);
  if (graph_bytes > free_b) {
    snprintf(c->err, sizeof(c->err), "%u solid k-mers of %zu-byte keys need about %llu bytes for the graph; %zu bytes of device "
             "memory are free", n, sizeof(K), static_cast<kf_ull>(graph_bytes), free_b);
    return MSGPU_E_NOMEM;
  }
  K        *d_keys = nullptr;
  uint32_t *d_cnt = nullptr, *d_slots = nullptr, slots_n = 0;
  STAGE_HIP(c, clock.begin(&S.select_ms));
  rc = kf_gather_sorted<K>(c, D, chunks, prm.min_count, n, k, d_cur, &d_keys, &d_cnt, &d_slots, &slots_n);
  if (rc != MSGPU_OK) return rc;
  STAGE_HIP(c, clock.end());
  UgGraph<K> g{d_keys, d_slots, slots_n - 1, n, k, 2 * (k - 1), kf_mask<K>(k)};

  // ---- neighbour bytes, tip rounds
  uint8_t *d_alive, *d_adj, *d_mark;
  STAGE_HIP(c, D.get(&d_alive, n));
  STAGE_HIP(c, D.get(&d_adj, n));
  STAGE_HIP(c, D.get(&d_mark, n));
  STAGE_HIP(c, hipMemsetAsync(d_alive, 1, n ? n : 1, st));
  STAGE_HIP(c, hipMemsetAsync(d_mark, 0, n ? n : 1, st));
  STAGE_HIP(c, clock.begin(&S.adjacency_ms));
  if (n) hipLaunchKernelGGL((k_ug_adj<K, true>), dim3(grid256(n)), dim3(256), 0, st, g, d_alive, d_adj);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  std::deque<msgpu_ug_round> rounds; // (the clock keeps pointers into it)
  uint64_t                   alive_n = n;
  const uint32_t             trim = static_cast<uint32_t>(prm.trim);
  auto refresh = [&](float *ms) -> int { // the neighbour bytes behind a round that removed something
    STAGE_HIP(c, clock.begin(ms));
    hipLaunchKernelGGL((k_ug_adj<K, false>), dim3(grid256(n)), dim3(256), 0, st, g, d_alive, d_adj);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    return MSGPU_OK;
  };
  auto tip_round = [&](uint32_t limit, uint64_t &removed) -> int { // rule 4, one round
    rounds.push_back(msgpu_ug_round{limit, 0, 0, 0.f, 0.f});
    msgpu_ug_round &R = rounds.back();
    STAGE_HIP(c, ug_zero_scalar(c, UG_SC_REMOVED));
    STAGE_HIP(c, clock.begin(&R.tips_ms));
    if (n) {
      hipLaunchKernelGGL(k_ug_tips<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_alive, d_adj, limit, d_mark);
      hipLaunchKernelGGL(k_ug_apply, dim3(grid256(n)), dim3(256), 0, st, n, d_alive, d_mark, reinterpret_cast<kf_ull *>(c->sc.d + UG_SC_REMOVED));
    }
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    const int r2 = c->sc.read(c);
    if (r2 != MSGPU_OK) return r2;
    removed = R.removed = c->sc.h[UG_SC_REMOVED];
    alive_n -= R.removed;
    return R.removed ? refresh(&R.adjacency_ms) : MSGPU_OK;
  };
  for (uint32_t limit = trim ? 1 : 0; limit;) {
    if (limit > trim) limit = trim;
    uint64_t removed = 0;
    rc = tip_round(limit, removed);
    if (rc != MSGPU_OK) return rc;
    if (limit < trim) limit = limit > trim / 2 ? trim : 2 * limit; // 1, 2, 4, ... below trim, then trim
    else if (!removed) limit = 0;                                  // the round at trim repeats until it removes nothing
  }
  // ---- rule 9 (on request): bubble phases, with a tip phase at trim behind each that removed something
  msgpu_ug_bubble_stats            &B = res->bubble_stats;
  std::deque<msgpu_ug_bubble_round> bubble_rounds; // (the clock keeps pointers into it)
  B.bubble = bubble;
  if (bubble) {
    uint32_t *d_forks; // lives during cleaning only
    STAGE_HIP(c, D.get(&d_forks, n2));
    kf_ull *sc_d = reinterpret_cast<kf_ull *>(c->sc.d);
    for (;;) {
      uint64_t phase_removed = 0;
      ++B.n_phases;
      for (;;) { // rounds until one removes nothing
        bubble_rounds.push_back(msgpu_ug_bubble_round{static_cast<uint32_t>(rounds.size()), 0, 0, 0, 0, 0, 0.f, 0.f});
        msgpu_ug_bubble_round &R = bubble_rounds.back();
        STAGE_HIP(c, hipMemsetAsync(c->sc.d + UG_SC_FORKS, 0, 3 * 8, st));
        STAGE_HIP(c, ug_zero_scalar(c, UG_SC_REMOVED));
        STAGE_HIP(c, clock.begin(&R.forks_ms));
        if (n) hipLaunchKernelGGL(k_ug_forks<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_alive, d_adj, d_forks, n2, sc_d + UG_SC_FORKS);
        STAGE_HIP(c, hipGetLastError());
        STAGE_HIP(c, clock.end());
        rc = c->sc.read(c);
        if (rc != MSGPU_OK) return rc;
        R.forks = c->sc.h[UG_SC_FORKS];
        if (R.forks > n2) {
          snprintf(c->err, sizeof(c->err), "%llu forks among %llu oriented nodes", static_cast<kf_ull>(R.forks), static_cast<kf_ull>(n2));
          return MSGPU_E_STATE;
        }
        if (R.forks) {
          STAGE_HIP(c, clock.begin(&R.walk_ms));
          hipLaunchKernelGGL(k_ug_bubbles<K>, dim3(grid256(4 * R.forks)), dim3(256), 0, st, g, d_adj, d_cnt, d_forks,
                             static_cast<uint32_t>(R.forks), bubble, d_mark, sc_d + UG_SC_BUBBLES, sc_d + UG_SC_BRANCHES);
          hipLaunchKernelGGL(k_ug_apply, dim3(grid256(n)), dim3(256), 0, st, n, d_alive, d_mark, sc_d + UG_SC_REMOVED);
          STAGE_HIP(c, hipGetLastError());
          STAGE_HIP(c, clock.end());
          rc = c->sc.read(c);
          if (rc != MSGPU_OK) return rc;
          R.bubbles          = c->sc.h[UG_SC_BUBBLES];
          R.branches_removed = c->sc.h[UG_SC_BRANCHES];
          R.removed          = c->sc.h[UG_SC_REMOVED];
        }
        B.n_bubbles += R.bubbles;
        B.n_branches_removed += R.branches_removed;
        B.max_forks = std::max<uint64_t>(B.max_forks, R.forks);
        if (!R.removed) break;
        alive_n -= R.removed;
        phase_removed += R.removed;
        rc = refresh(&B.adjacency_ms);
        if (rc != MSGPU_OK) return rc;
      }
      B.n_kmers_removed += phase_removed;
      if (!phase_removed || !trim) break;
      uint64_t tips_removed = 0;
      for (uint64_t removed = 1; removed;) { // the round at trim alone, until it removes nothing
        rc = tip_round(trim, removed);
        if (rc != MSGPU_OK) return rc;
        tips_removed += removed;
      }
      if (!tips_removed) break;
    }
    B.n_rounds = static_cast<uint32_t>(bubble_rounds.size());
    D.drop(d_forks);
  }
  S.n_solid_trimmed = alive_n;
  S.n_tip_rounds    = static_cast<uint32_t>(rounds.size());
  D.drop(d_mark);

  // ---- joins, pointer doubling
  uint32_t *d_next, *d_ptr[2], *d_dist[2];
  STAGE_HIP(c, D.get(&d_next, n2));
  for (int i = 0; i < 2; ++i) {
    STAGE_HIP(c, D.get(&d_ptr[i], n2));
    STAGE_HIP(c, D.get(&d_dist[i], n2));
  }
  STAGE_HIP(c, clock.begin(&S.next_ms));
  if (n) {
    hipLaunchKernelGGL(k_ug_next<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_alive, d_adj, d_next);
    hipLaunchKernelGGL(k_ug_chain_init<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_alive, d_next, d_ptr[0], d_dist[0]);
  }
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  int  cur = 0;
  auto doubling = [&](uint64_t &open) -> int { // rounds until the number of open nodes is 0 or stops falling
    uint64_t before = ~0ull;
    for (;;) {
      if (S.doubling_rounds >= 200) {
        snprintf(c->err, sizeof(c->err), "pointer doubling did not settle in %u rounds", S.doubling_rounds);
        return MSGPU_E_STATE;
      }
      STAGE_HIP(c, ug_zero_scalar(c, UG_SC_OPEN));
      STAGE_HIP(c, clock.begin(&S.doubling_ms));
      hipLaunchKernelGGL(k_ug_double, dim3(grid256(n2)), dim3(256), 0, st, n2, d_next, d_ptr[cur], d_dist[cur], d_ptr[cur ^ 1],
                         d_dist[cur ^ 1], reinterpret_cast<kf_ull *>(c->sc.d + UG_SC_OPEN));
      STAGE_HIP(c, hipGetLastError());
      STAGE_HIP(c, clock.end());
      cur ^= 1;
      ++S.doubling_rounds;
      const int r2 = c->sc.read(c);
      if (r2 != MSGPU_OK) return r2;
      open = c->sc.h[UG_SC_OPEN];
      if (!open || open == before) return MSGPU_OK;
      before = open;
    }
  };
  uint64_t  open = 0;
  uint8_t  *d_cyc = nullptr;
  uint32_t *d_cyc_last = nullptr;
  if (n) {
    rc = doubling(open);
    if (rc != MSGPU_OK) return rc;
  }
  if (open) { // cycles: their smallest node by a min-reduction, the cut, and the doubling again
    uint32_t *d_back[2], *d_low[2];
    STAGE_HIP(c, D.get(&d_cyc, n2));
    for (int i = 0; i < 2; ++i) {
      STAGE_HIP(c, D.get(&d_back[i], n2));
      STAGE_HIP(c, D.get(&d_low[i], n2));
    }
    STAGE_HIP(c, clock.begin(&S.doubling_ms));
    hipLaunchKernelGGL(k_ug_cyc_init, dim3(grid256(n2)), dim3(256), 0, st, n2, d_next, d_ptr[cur], d_cyc, d_back[0], d_low[0]);
    int at = 0;
    for (uint64_t span = 1; span < open; span *= 2, at ^= 1, ++S.doubling_rounds) // (a cycle has at most `open` nodes)
      hipLaunchKernelGGL(k_ug_cyc_min<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_cyc, d_back[at], d_low[at], d_back[at ^ 1],
                         d_low[at ^ 1]);
    hipLaunchKernelGGL(k_ug_cyc_cut, dim3(grid256(n2)), dim3(256), 0, st, n2, d_cyc, d_low[at], d_next, d_ptr[cur], d_dist[cur]);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    rc = doubling(open);
    if (rc != MSGPU_OK) return rc;
    if (open) {
      snprintf(c->err, sizeof(c->err), "%llu nodes reach no chain head after the cycles were cut", static_cast<kf_ull>(open));
      return MSGPU_E_STATE;
    }
    d_cyc_last = d_low[at];
    D.drop(d_low[at ^ 1]);
    for (int i = 0; i < 2; ++i) D.drop(d_back[i]);
  }
  uint32_t *d_p = d_ptr[cur], *d_d = d_dist[cur];
  D.drop(d_ptr[cur ^ 1]);
  D.drop(d_dist[cur ^ 1]);

  // ---- the emitted heads in output order, the unitig table, coverage
  STAGE_HIP(c, clock.begin(&S.order_ms));
  STAGE_HIP(c, ug_zero_scalar(c, UG_SC_UNITS));
  kf_ull *d_units_n = reinterpret_cast<kf_ull *>(c->sc.d + UG_SC_UNITS);
  if (n) hipLaunchKernelGGL((k_ug_heads<K, false>), dim3(grid256(n2)), dim3(256), 0, st, g, d_next, d_p, nullptr, nullptr, 0, d_units_n);
  STAGE_HIP(c, hipGetLastError());
  rc = c->sc.read(c);
  if (rc != MSGPU_OK) return rc;
  const uint32_t U = static_cast<uint32_t>(c->sc.h[UG_SC_UNITS]);
  S.n_unitigs = U;
  K        *d_first[2];
  uint32_t *d_head[2], *d_unit_of, *d_nk;
  uint8_t  *d_cyclic;
  kf_ull   *d_cover;
  uint64_t *d_seq_off;
  for (int i = 0; i < 2; ++i) {
    STAGE_HIP(c, D.get(&d_first[i], U));
    STAGE_HIP(c, D.get(&d_head[i], U));
  }
  STAGE_HIP(c, D.get(&d_unit_of, n2));
  STAGE_HIP(c, D.get(&d_nk, U));
  STAGE_HIP(c, D.get(&d_cyclic, U));
  STAGE_HIP(c, D.get(&d_cover, U));
  STAGE_HIP(c, D.get(&d_seq_off, U));
  STAGE_HIP(c, hipMemsetAsync(d_unit_of, 0xff, n2 ? n2 * 4 : 4, st));
  STAGE_HIP(c, hipMemsetAsync(d_cover, 0, U ? U * 8ull : 8, st));
  if (U) {
    STAGE_HIP(c, ug_zero_scalar(c, UG_SC_UNITS));
    hipLaunchKernelGGL((k_ug_heads<K, true>), dim3(grid256(n2)), dim3(256), 0, st, g, d_next, d_p, d_first[0], d_head[0], U, d_units_n);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_rocprim(D, [&](void *t, size_t &b) {
                return kf_sort_pairs(t, b, d_first[0], d_first[1], d_head[0], d_head[1], static_cast<unsigned int>(U), 2 * k, st);
              }));
    hipLaunchKernelGGL(k_ug_units, dim3(grid256(U)), dim3(256), 0, st, U, d_head[1], d_p, d_d, d_cyc, d_cyc_last, d_unit_of, d_nk,
                       d_cyclic);
    hipLaunchKernelGGL(k_ug_cover, dim3(grid256(n2)), dim3(256), 0, st, n2, d_p, d_unit_of, d_cnt, d_cover);
    STAGE_HIP(c, hipGetLastError());
  }
  STAGE_HIP(c, clock.end());
  std::vector<uint32_t> nk;
  std::vector<uint8_t>  cyclic;
  std::vector<kf_ull>   cover;
  std::vector<K>        first;
  std::vector<uint64_t> seq_off;
  try {
    nk.resize(U);
    cyclic.resize(U);
    cover.resize(U);
    first.resize(U);
    seq_off.resize(U);
    res->units.resize(U);
    res->first_w = sizeof(K) / 8;
    res->first_words.resize(U * (sizeof(K) / 8));
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, clock.begin(&S.copy_ms));
  if (U) {
    STAGE_HIP(c, hipMemcpyAsync(nk.data(), d_nk, U * 4ull, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(cyclic.data(), d_cyclic, U, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(cover.data(), d_cover, U * 8ull, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(first.data(), d_first[1], U * sizeof(K), hipMemcpyDeviceToHost, st));
  }
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));

  // ---- host: headers and offsets
  const StageTimer host0;
  std::string heads; // every header, one behind the other
  std::vector<uint32_t> head_len(U);
  uint64_t              total = 0, solid_sum = 0;
  char                  buf[96];
  try {
    for (uint32_t u = 0; u < U; ++u) {
      msgpu_ug_unitig &T = res->units[u];
      T.length   = static_cast<uint64_t>(nk[u]) + k - 1;
      T.coverage = cover[u];
      T.cyclic   = cyclic[u];
      T.reserved = 0;
      key_split(first[u], T.first_hi, T.first_lo);
      key_words(first[u], res->first_words.data() + u * (sizeof(K) / 8));
      head_len[u] = static_cast<uint32_t>(snprintf(buf, sizeof(buf), ">%u %llu %llu\n", u, static_cast<kf_ull>(T.length), cover[u]));
      heads.append(buf, head_len[u]);
      T.offset   = total + head_len[u];
      seq_off[u] = T.offset;
      total += head_len[u] + T.length + 1;
      solid_sum += nk[u];
      S.n_cycles += cyclic[u];
      S.longest_chain = std::max<uint64_t>(S.longest_chain, nk[u]);
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (solid_sum != alive_n) { // every k-mer lies in exactly one unitig: never seen otherwise
    snprintf(c->err, sizeof(c->err), "the unitigs hold %llu k-mers where %llu are solid", static_cast<kf_ull>(solid_sum),
             static_cast<kf_ull>(alive_n));
    return MSGPU_E_STATE;
  }
  S.host_ms += host0.ms();

  // ---- rule 10 (on request): the links of the unitig ends, their sort, the GFA text
  msgpu_ug_graph_stats &G = res->graph_stats;
  std::string           gfa_fix; // what the host writes of every S line: "S\t<id>\t" and "LN:i:<length>\tKC:i:<coverage>\n"
  std::vector<uint32_t> gfa_fix_len;
  std::vector<uint64_t> gfa_off; // of every sequence in the GFA text
  if (graph) {
    kf_ull        *sc_d = reinterpret_cast<kf_ull *>(c->sc.d);
    const uint64_t cap = 8ull * U; // 2 U ends, 4 successors each
    STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
    if (cap * 8 > free_b) {
      snprintf(c->err, sizeof(c->err), "%u unitigs need %llu bytes for the keys of their links; %zu bytes of device memory are free", U,
               static_cast<kf_ull>(cap * 8), free_b);
      return MSGPU_E_NOMEM;
    }
    uint64_t *d_key[2];
    STAGE_HIP(c, D.get(&d_key[0], cap));
    STAGE_HIP(c, hipMemsetAsync(c->sc.d + UG_SC_LINKS, 0, 5 * 8, st));
    STAGE_HIP(c, clock.begin(&G.links_ms));
    if (U)
      hipLaunchKernelGGL(k_ug_links<K>, dim3(grid256(cap)), dim3(256), 0, st, g, d_adj, d_p, d_d, d_unit_of, d_head[1], d_nk, d_cyc,
                         d_cyc_last, U, d_key[0], cap, sc_d + UG_SC_LINKS);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    rc = c->sc.read(c);
    if (rc != MSGPU_OK) return rc;
    const uint64_t L = c->sc.h[UG_SC_LINKS];
    G.n_links       = L;
    G.n_adjacencies = c->sc.h[UG_SC_ADJACENCIES];
    G.n_self_mirror = c->sc.h[UG_SC_SELF_MIRROR];
    G.n_dead_ends   = c->sc.h[UG_SC_DEAD_ENDS];
    if (c->sc.h[UG_SC_LOST_LINKS] || L > cap) { // rule 10 (b): never seen
      snprintf(c->err, sizeof(c->err), "%llu of %llu adjacencies end at no unitig's first node; %llu links of %u unitigs",
               static_cast<kf_ull>(c->sc.h[UG_SC_LOST_LINKS]), static_cast<kf_ull>(G.n_adjacencies), static_cast<kf_ull>(L), U);
      return MSGPU_E_STATE;
    }
    if (L >= (1ull << 32)) {
      snprintf(c->err, sizeof(c->err), "%llu links; the limit is 2^32 - 1", static_cast<kf_ull>(L));
      return MSGPU_E_ARG;
    }
    // the host's part of the S lines, and where the sequences go
    const StageTimer host_s;
    uint64_t         seg_bytes = 0;
    try {
      gfa_fix_len.resize(2ull * U);
      gfa_off.resize(U);
      res->links.resize(L);
      for (uint32_t u = 0; u < U; ++u) {
        const msgpu_ug_unitig &T = res->units[u];
        gfa_fix_len[2 * u] = static_cast<uint32_t>(snprintf(buf, sizeof(buf), "S\t%u\t", u));
        gfa_fix.append(buf, gfa_fix_len[2 * u]);
        gfa_fix_len[2 * u + 1] =
            static_cast<uint32_t>(snprintf(buf, sizeof(buf), "LN:i:%llu\tKC:i:%llu\n", static_cast<kf_ull>(T.length), static_cast<kf_ull>(T.coverage)));
        gfa_fix.append(buf, gfa_fix_len[2 * u + 1]);
        gfa_off[u] = sizeof(UG_GFA_HEADER) - 1 + seg_bytes + gfa_fix_len[2 * u];
        seg_bytes += gfa_fix_len[2 * u] + T.length + 1 + gfa_fix_len[2 * u + 1];
      }
    } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
    S.host_ms += host_s.ms();
    const uint64_t link_base = sizeof(UG_GFA_HEADER) - 1 + seg_bytes;
    uint32_t       overlap_digits = 1;
    for (int x = k - 1; x >= 10; x /= 10) ++overlap_digits;
    // the sorted keys, the table, a length and an offset per link, the segments; the L lines' bytes are not known yet
    STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const uint64_t link_bytes = L * (8 + sizeof(msgpu_ug_link) + 4 + 8) + 12 + U * 8ull + link_base;
    if (link_bytes + L * 10 > free_b) {
      snprintf(c->err, sizeof(c->err), "%llu links and %llu bytes of segment lines need more than %llu bytes for the graph's text; %zu "
               "bytes of device memory are free", static_cast<kf_ull>(L), static_cast<kf_ull>(link_base), static_cast<kf_ull>(link_bytes + L * 10), free_b);
      return MSGPU_E_NOMEM;
    }
    msgpu_ug_link *d_link;
    uint32_t      *d_len;
    uint64_t      *d_off, *d_gfa_off;
    uint8_t       *d_gfa;
    STAGE_HIP(c, D.get(&d_key[1], L));
    STAGE_HIP(c, D.get(&d_link, L));
    STAGE_HIP(c, D.get(&d_len, L + 1));
    STAGE_HIP(c, D.get(&d_off, L + 1));
    STAGE_HIP(c, D.get(&d_gfa_off, U));
    STAGE_HIP(c, clock.begin(&G.sort_ms));
    if (L)
      STAGE_HIP(c, stage_rocprim(D, [&](void *t, size_t &b) {
                  return rocprim::radix_sort_keys(t, b, d_key[0], d_key[1], static_cast<unsigned int>(L), 0, 64, st);
                }));
    STAGE_HIP(c, clock.end());
    STAGE_HIP(c, clock.begin(&G.text_ms));
    hipLaunchKernelGGL(k_ug_link_lens, dim3(grid256(L + 1)), dim3(256), 0, st, d_key[1], L, overlap_digits, d_link, d_len);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_scan_total(D, st, d_len, d_off, L, c->sc, UG_SC_OPEN));
    STAGE_HIP(c, clock.end());
    rc = c->sc.read(c);
    if (rc != MSGPU_OK) return rc;
    const uint64_t gfa_total = link_base + c->sc.h[UG_SC_OPEN];
    if (c->sc.h[UG_SC_OPEN] < L * 12 || c->sc.h[UG_SC_OPEN] > L * 32) {
      snprintf(c->err, sizeof(c->err), "%llu links in %llu bytes of L lines", static_cast<kf_ull>(L), static_cast<kf_ull>(c->sc.h[UG_SC_OPEN]));
      return MSGPU_E_STATE;
    }
    STAGE_HIP(c, D.get(&d_gfa, gfa_total));
    STAGE_HIP(c, clock.begin(&G.text_ms));
    if (U) {
      STAGE_HIP(c, hipMemcpyAsync(d_gfa_off, gfa_off.data(), U * 8ull, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_ug_write<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_p, d_d, d_unit_of, d_nk, d_gfa_off, d_gfa, gfa_total,
                         static_cast<uint8_t>('\t'));
    }
    if (L)
      hipLaunchKernelGGL(k_ug_link_write, dim3(grid256(L)), dim3(256), 0, st, d_link, d_off, L, static_cast<uint32_t>(k - 1),
                         overlap_digits, link_base, d_gfa, gfa_total);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    STAGE_HIP(c, clock.begin(&S.copy_ms));
    STAGE_HIP(c, hipHostMalloc(reinterpret_cast<void **>(&res->gfa), gfa_total, hipHostMallocDefault));
    STAGE_HIP(c, hipMemcpyAsync(res->gfa, d_gfa, gfa_total, hipMemcpyDeviceToHost, st));
    if (L) STAGE_HIP(c, hipMemcpyAsync(res->links.data(), d_link, L * sizeof(msgpu_ug_link), hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, clock.end());
    res->gfa_len = gfa_total;
    G.gfa_bytes  = gfa_total;
  }

  // ---- the bases
  uint8_t *d_text;
  STAGE_HIP(c, D.get(&d_text, total));
  STAGE_HIP(c, clock.begin(&S.write_ms));
  if (U) {
    STAGE_HIP(c, hipMemcpyAsync(d_seq_off, seq_off.data(), U * 8ull, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_ug_write<K>, dim3(grid256(n2)), dim3(256), 0, st, g, d_p, d_d, d_unit_of, d_nk, d_seq_off, d_text, total,
                       static_cast<uint8_t>('\n'));
    STAGE_HIP(c, hipGetLastError());
  }
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, clock.begin(&S.copy_ms));
  if (total) {
    STAGE_HIP(c, hipHostMalloc(reinterpret_cast<void **>(&res->all), total, hipHostMallocDefault));
    STAGE_HIP(c, hipMemcpyAsync(res->all, d_text, total, hipMemcpyDeviceToHost, st));
  }
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  clock.collect();
  res->all_len = total;

  // ---- host: the headers into the text, the cut text
  const StageTimer host1;
  try {
    uint64_t at = 0, cut_bytes = 0;
    for (uint32_t u = 0; u < U; ++u)
      if (res->units[u].length >= prm.min_length) cut_bytes += head_len[u] + res->units[u].length + 1;
    res->cut.reserve(cut_bytes);
    for (uint32_t u = 0; u < U; ++u) {
      const uint64_t rec = res->units[u].offset - head_len[u], bytes = head_len[u] + res->units[u].length + 1;
      memcpy(res->all + rec, heads.data() + at, head_len[u]);
      at += head_len[u];
      if (res->units[u].length >= prm.min_length) {
        res->cut.append(res->all + rec, bytes);
        ++S.n_unitigs_kept;
      }
    }
    res->rounds.assign(rounds.begin(), rounds.end());
    res->bubble_rounds.assign(bubble_rounds.begin(), bubble_rounds.end());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if (graph) { // the header and the host's part of the S lines into the GFA text
    memcpy(res->gfa, UG_GFA_HEADER, sizeof(UG_GFA_HEADER) - 1);
    uint64_t at = 0;
    for (uint32_t u = 0; u < U; ++u) {
      memcpy(res->gfa + gfa_off[u] - gfa_fix_len[2 * u], gfa_fix.data() + at, gfa_fix_len[2 * u]);
      at += gfa_fix_len[2 * u];
      memcpy(res->gfa + gfa_off[u] + res->units[u].length + 1, gfa_fix.data() + at, gfa_fix_len[2 * u + 1]);
      at += gfa_fix_len[2 * u + 1];
    }
  }
  for (const msgpu_ug_round &R : res->rounds) {
    S.tips_ms += R.tips_ms;
    S.adjacency_ms += R.adjacency_ms;
  }
  for (const msgpu_ug_bubble_round &R : res->bubble_rounds) {
    B.forks_ms += R.forks_ms;
    B.walk_ms += R.walk_ms;
  }
  S.host_ms += host1.ms();
  S.bytes_out[0] = res->all_len;
  S.bytes_out[1] = res->cut.size();
  return MSGPU_OK;
}

} // namespace

extern "C" {

int  msgpu_ug_create(int device, msgpu_ugctx **out) { return stage_create(device, out); }
void msgpu_ug_destroy(msgpu_ugctx *c) { stage_destroy(c); }

const char *msgpu_ug_last_error(const msgpu_ugctx *c) { return c ? c->err : "null context"; }
uint64_t    msgpu_ug_error_line(const msgpu_ugctx *c) { return c ? c->err_line : 0; }
int         msgpu_ug_error_file(const msgpu_ugctx *c) { return c ? c->err_file : 0; }

// the parameters as a run uses them; the context takes the error
static int ug_params(msgpu_ugctx *c, const msgpu_ug_params *params, msgpu_ug_params &prm) {
  prm = *params;
  if (prm.k < 2 || prm.k > (c->wide ? 128 : 64)) {
    snprintf(c->err, sizeof(c->err), "k = %d is outside 2..%d", prm.k, c->wide ? 128 : 64);
    return MSGPU_E_ARG;
  }
  if (prm.trim == -1) prm.trim = prm.k;
  if (prm.min_count < 1 || prm.trim < 0) {
    snprintf(c->err, sizeof(c->err), "min_count = %u must be at least 1, trim = %d at least 0 (or -1 for k)", prm.min_count, prm.trim);
    return MSGPU_E_ARG;
  }
  return MSGPU_OK;
}

int msgpu_ug_run_pair(msgpu_ugctx *c, const msgpu_ug_params *params, const msgpu_pair *pair, const uint8_t *dropped, uint64_t n_pairs,
                      uint32_t flags, uint64_t budget_bytes, msgpu_ug_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out        = nullptr;
  c->err[0]   = 0;
  c->err_line = 0;
  c->err_file = 0;
  if (!params || !pair || flags) return MSGPU_E_ARG;
  msgpu_ug_params prm;
  int             rc = ug_params(c, params, prm);
  if (rc != MSGPU_OK) return rc;
  if (pair->device != c->device) {
    snprintf(c->err, sizeof(c->err), "the pair is on device %d, the context on device %d", pair->device, c->device);
    return MSGPU_E_ARG;
  }
  const KfFile *F = pair->F;
  if (dropped && (pair->n_files != 2 || F[0].n_lines != F[1].n_lines || n_pairs != (F[0].n_lines >> 2))) {
    snprintf(c->err, sizeof(c->err), "a mask of %llu pairs on files of %llu and %llu records: with a mask both files hold n_pairs records",
             static_cast<kf_ull>(n_pairs), static_cast<kf_ull>(F[0].n_lines >> 2),
             static_cast<kf_ull>(pair->n_files == 2 ? F[1].n_lines >> 2 : 0));
    return MSGPU_E_ARG;
  }
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_ug_result> res;
  try {
    res.reset(new msgpu_ug_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  msgpu_ug_stats &S = res->stats;
  S.k          = static_cast<uint32_t>(prm.k);
  S.min_count  = prm.min_count;
  S.trim       = static_cast<uint32_t>(prm.trim);
  S.min_length = prm.min_length;
  const uint64_t lost0 = c->sc.lost;
  for (int f = 0; f < pair->n_files; ++f) {
    S.bytes_in[f]  = F[f].size;
    S.n_records[f] = F[f].n_lines >> 2;
  }
  DevArena D; // the run's own: the pair's bytes are read, never written
  uint8_t *d_dropped = nullptr;
  if (dropped) { // the mask goes to the device once
    STAGE_HIP(c, D.get(&d_dropped, n_pairs));
    if (n_pairs) STAGE_HIP(c, hipMemcpyAsync(d_dropped, dropped, n_pairs, hipMemcpyHostToDevice, c->stream));
    STAGE_HIP(c, hipStreamSynchronize(c->stream)); // (the caller's array may go when the call returns)
  }
  rc = prm.k <= 32   ? ug_stage<uint64_t>(c, D, F, d_dropped, prm, c->bubble, c->graph, budget_bytes, res.get())
       : prm.k <= 64 ? ug_stage<kf_u128>(c, D, F, d_dropped, prm, c->bubble, c->graph, budget_bytes, res.get())
       : prm.k <= 96 ? ug_stage<KfWide<3>>(c, D, F, d_dropped, prm, c->bubble, c->graph, budget_bytes, res.get())
                     : ug_stage<KfWide<4>>(c, D, F, d_dropped, prm, c->bubble, c->graph, budget_bytes, res.get());
  if (rc != MSGPU_OK) {
    (void)hipStreamSynchronize(c->stream); // (nothing of the run is still reading the pair when the arena goes)
    return rc;
  }
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;
  res->bytes_peak       = D.peak;
  S.n_lost_publications = c->sc.lost - lost0;
  S.wall_ms             = wall.ms();
  *out                  = res.release();
  return MSGPU_OK;
}

// open + run on the pair + close
int msgpu_ug_run(msgpu_ugctx *c, const msgpu_ug_params *params, const char *path_a, const char *path_b, uint32_t flags,
                 uint64_t budget_bytes, msgpu_ug_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out        = nullptr;
  c->err[0]   = 0;
  c->err_line = 0;
  c->err_file = 0;
  if (!params || !path_a || flags) return MSGPU_E_ARG;
  msgpu_ug_params prm;
  int             rc = ug_params(c, params, prm);
  if (rc != MSGPU_OK) return rc;
  const StageTimer wall;
  STAGE_HIP(c, hipSetDevice(c->device));
  msgpu_pair *pair = nullptr;
  rc = kf_pair_open(c, path_a, path_b, &pair);
  if (rc != MSGPU_OK) return rc;
  rc = msgpu_ug_run_pair(c, params, pair, nullptr, 0, 0, budget_bytes, out);
  if (rc == MSGPU_OK) {
    (*out)->stats.load_ms    = pair->load_ms;
    (*out)->stats.records_ms = pair->records_ms;
  }
  kf_pair_close(pair);
  if (rc == MSGPU_OK) (*out)->stats.wall_ms = wall.ms();
  return rc;
}

int msgpu_ug_set_bubbles(msgpu_ugctx *c, uint32_t bubble) {
  if (!c) return MSGPU_E_ARG;
  if (bubble > MSGPU_UG_BUBBLE_MAX) {
    snprintf(c->err, sizeof(c->err), "bubble = %u is above %u", bubble, MSGPU_UG_BUBBLE_MAX);
    return MSGPU_E_ARG;
  }
  c->bubble = bubble;
  return MSGPU_OK;
}

int msgpu_ug_set_graph(msgpu_ugctx *c, int on) {
  if (!c) return MSGPU_E_ARG;
  c->graph = on != 0;
  return MSGPU_OK;
}

int msgpu_ug_set_wide(msgpu_ugctx *c, int on) {
  if (!c) return MSGPU_E_ARG;
  c->wide = on != 0;
  return MSGPU_OK;
}

int msgpu_ug_result_first_kmers(const msgpu_ug_result *r, const uint64_t **words, uint32_t *words_per_kmer, uint64_t *n) {
  if (!r || !words || !words_per_kmer || !n) return MSGPU_E_ARG;
  *words          = r->first_words.data();
  *words_per_kmer = r->first_w;
  *n              = r->units.size();
  return MSGPU_OK;
}

uint64_t msgpu_ug_result_peak_bytes(const msgpu_ug_result *r) { return r ? r->bytes_peak : 0; }

int msgpu_ug_result_links(const msgpu_ug_result *r, msgpu_ug_graph_stats *out, const msgpu_ug_link **links, uint64_t *n) {
  if (!r || !out || !links || !n) return MSGPU_E_ARG;
  *out   = r->graph_stats;
  *links = r->links.data();
  *n     = r->links.size();
  return MSGPU_OK;
}

int msgpu_ug_result_stats(const msgpu_ug_result *r, msgpu_ug_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

int msgpu_ug_result_rounds(const msgpu_ug_result *r, const msgpu_ug_round **rounds, uint64_t *n) {
  if (!r || !rounds || !n) return MSGPU_E_ARG;
  *rounds = r->rounds.data();
  *n      = r->rounds.size();
  return MSGPU_OK;
}

int msgpu_ug_result_bubbles(const msgpu_ug_result *r, msgpu_ug_bubble_stats *out, const msgpu_ug_bubble_round **rounds, uint64_t *n) {
  if (!r || !out || !rounds || !n) return MSGPU_E_ARG;
  *out    = r->bubble_stats;
  *rounds = r->bubble_rounds.data();
  *n      = r->bubble_rounds.size();
  return MSGPU_OK;
}

int msgpu_ug_result_unitigs(const msgpu_ug_result *r, const msgpu_ug_unitig **unitigs, uint64_t *n) {
  if (!r || !unitigs || !n) return MSGPU_E_ARG;
  *unitigs = r->units.data();
  *n       = r->units.size();
  return MSGPU_OK;
}

const char *msgpu_ug_result_text(const msgpu_ug_result *r, int which, uint64_t *len) {
  if (len) *len = 0;
  if (!r) return "";
  if (which == MSGPU_UG_TEXT_ALL) {
    if (len) *len = r->all_len;
    return r->all ? r->all : "";
  }
  if (which == MSGPU_UG_TEXT_CUT) {
    if (len) *len = r->cut.size();
    return r->cut.data();
  }
  if (which == MSGPU_UG_TEXT_GFA && r->gfa) {
    if (len) *len = r->gfa_len;
    return r->gfa;
  }
  return "";
}

void msgpu_ug_result_free(msgpu_ug_result *r) {
  if (r) delete r;
}

} // extern "C"
