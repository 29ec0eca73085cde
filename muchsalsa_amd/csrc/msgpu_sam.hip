// msgpu_sam.hip -- the SAM stage: the mapper's tables as SAM 1.6 text, formatted on the device (include/msgpu.h, "SAM output";
// DESIGN.md section 16).  The chain table arrives with its runs (len << 4 | op), its rank rows (rule 12) and, for pairs, its
// mate rows (rule 13); the stage checks the tables on the device (S1), finds every query record's representative (S4),
// resolves every chain's FLAG and mate line (S8), and then, per batch of query records (S11), builds the line table (S3),
// gives every line its exact byte count, scans the counts and writes every line at its offset (S5 - S10).
//
// The shape of the device work is count, scan, write, and nothing in it walks a run list.  What a run contributes to its
// line depends on the run and on scans over the run table alone: the target bases consumed in front of it (T), the '='
// columns in front of it (E), the last run in front of it that resets MD's count (an exclusive maximum scan, pe) and the
// head of its stretch of = / X runs (an inclusive maximum scan, mhead: the M of eqx = 0).  So the width of every run in the
// CIGAR (cw) and in MD (mw) is a per-run kernel, their 64-bit scans (CW, MW) serve as the segmented scans of every line at
// once, a line's size is a thread's arithmetic, and in the write pass any lane can place any run, any MD column and any SEQ
// byte of a line without knowing what its neighbours do.  Two classes, listed with wave_append: a line of at most
// MSGPU_SAM_SHORT_BYTES is written by one wavefront (four lines per workgroup); a longer one by SAM_SLICES workgroups of 256
// lanes, slice s taking every SAM_SLICES-th stretch of 256 elements.  In both the lanes stride over the runs (one run's
// digits and letter per lane), over the target columns of MD (a lane finds its column's run by a binary search in T) and
// over SEQ (one aligned 32-bit store of four folded bytes per lane, single bytes in front of and behind the aligned part;
// consecutive lanes write consecutive words); the dozen numbers of a line are written by a lane each.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>
#include <unordered_set>

#include "msgpu_device.h"
#include "msgpu_internal.h"
#include "msgpu_kmer_shared.h"
#include "msgpu_stage.h"

namespace msgpu {

constexpr uint32_t SAM_I = 1, SAM_D = 2, SAM_EQ = 7, SAM_X = 8;
constexpr uint32_t SAM_NONE = MSGPU_SAM_UNMAPPED;
constexpr uint32_t SAM_SLICES = 8;          // workgroups per line of the long class
constexpr uint64_t SAM_BATCH_FIXED = 1ull << 20; // S11: alignment of the batch's blocks and rocPRIM's temporary buffer
constexpr uint64_t SAM_BATCH_LINE = 64;     // S11: line table 24, size 8, scan 8, two class lists 8, the scan's temporary share
// S1: what can be wrong with a chain, in the order in which one chain's violations are looked at
enum { SAM_BAD_OFF = 0, SAM_BAD_ORDER, SAM_BAD_STRAND, SAM_BAD_QREC, SAM_BAD_TREC, SAM_BAD_TRANGE, SAM_BAD_QRANGE, SAM_BAD_RUN, SAM_BAD_TCONS,
       SAM_BAD_QCONS, SAM_BAD_RANK, SAM_BAD_MATE };

struct SamTables { // the resident tables as the kernels see them
  const msgpu_map_chain *chains;
  const msgpu_map_rank  *ranks;
  const msgpu_map_mate  *mates; // null: single-end
  const uint64_t        *off;   // n_chains + 1
  const uint32_t        *ops;   // n_runs
  const uint64_t        *T, *Q, *E; // n_runs + 1: target bases, query bases and '=' columns in front of a run
  const uint32_t        *mhead;     // n_runs (eqx = 0): the head of the run's stretch of = / X runs
  const uint32_t        *pe;        // n_runs + 1 (md = 1): one behind the last X or D run in front of a run, 0 if none
  const uint64_t        *CW, *MW;   // n_runs + 1: the scans of the runs' widths in the CIGAR and (md = 1) in MD
  const kf_ull          *vkey;      // per query record: the representative's key, 0 without a primary
  const uint32_t        *cflag, *cmate; // per chain: FLAG; the mate line or SAM_NONE
  const uint8_t         *tn, *qn;       // the names, one behind the other (the queries' as S7 writes them)
  const uint64_t        *tn_off, *qn_off; // n + 1
  uint32_t               n_chains, n_runs, eqx, md, unmapped;
};

__device__ inline void sam_bad(kf_ull *bad, uint32_t chain, uint32_t what) { atomicMin(bad, (static_cast<kf_ull>(chain) << 4) | what); }
__device__ inline bool sam_is_m(uint32_t op) { return op == SAM_EQ || op == SAM_X; }
// (the decimal helpers dec_dig, dec_sdig, dec_put, dec_sput and S6's text_base: msgpu_device.h)
// S4: the representative of a query record, or SAM_NONE
__device__ inline uint32_t sam_rep(const kf_ull *vkey, uint32_t r) {
  const kf_ull k = vkey[r];
  return k ? 0xffffffffu - static_cast<uint32_t>(k) : SAM_NONE;
}

// S1 (a): nothing else of the tables can be read without the offsets
__global__ __launch_bounds__(256) void k_sam_check_off(const uint64_t *off, uint32_t n_chains, uint64_t n_runs, kf_ull *bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n_chains) return;
  if ((i == 0 && off[0] != 0) || off[i + 1] < off[i] || off[i + 1] > n_runs) sam_bad(bad, i, SAM_BAD_OFF);
}

// per run: its chain, what it consumes, its '=' columns, S1 (g); head[u] = u where the run opens a stretch of = / X runs
// (0 elsewhere: an inclusive maximum scan gives every run of the stretch its head), ev[u] = u + 1 for an X or D run
__global__ __launch_bounds__(256) void k_sam_runs(const uint64_t *off, uint32_t n_chains, const uint32_t *ops, uint32_t n_runs, uint32_t *run_chain,
                                                  uint32_t *tc, uint32_t *qc, uint32_t *ec, uint32_t *head, uint32_t *ev, kf_ull *bad) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_runs) return;
  const uint32_t i = last_le(off, 0, n_chains, u); // off[0] = 0 <= u, and off[i + 1] > u as off[n_chains] = n_runs
  const uint32_t len = ops[u] >> 4, op = ops[u] & 15;
  const bool     ok = len >= 1 && (op == SAM_I || op == SAM_D || op == SAM_EQ || op == SAM_X);
  if (!ok) sam_bad(bad, i, SAM_BAD_RUN);
  run_chain[u] = i;
  tc[u]        = ok && op != SAM_I ? len : 0;
  qc[u]        = ok && op != SAM_D ? len : 0;
  ec[u]        = ok && op == SAM_EQ ? len : 0;
  head[u]      = sam_is_m(op) && (u == off[i] || !sam_is_m(ops[u - 1] & 15)) ? u : 0;
  ev[u]        = op == SAM_X || op == SAM_D ? u + 1 : 0;
}

// S1 on the chain's fields, its rows and on what its runs consume, for the first n chains
__global__ __launch_bounds__(256) void k_sam_check_chain(SamTables X, uint32_t n, SeqRecs R, SeqRecs Q, kf_ull *bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return; // (the first n chains: the ones in front of the first chain with a bad offset)
  const msgpu_map_chain ch = X.chains[i];
  uint32_t              what = ~0u; // (none)
  auto                  found = [&](uint32_t w) { what = w < what ? w : what; };
  if (i && ch.query < X.chains[i - 1].query) found(SAM_BAD_ORDER);
  if (ch.strand > 1) found(SAM_BAD_STRAND);
  if (ch.query >= Q.n) found(SAM_BAD_QREC);
  if (ch.target >= R.n) found(SAM_BAD_TREC);
  if (ch.target < R.n && !(ch.t_start <= ch.t_end && ch.t_end <= R.len[ch.target])) found(SAM_BAD_TRANGE);
  if (ch.query < Q.n && !(ch.q_start <= ch.q_end && ch.q_end <= Q.len[ch.query])) found(SAM_BAD_QRANGE);
  const uint64_t a = X.off[i], b = X.off[i + 1];
  if (X.T[b] - X.T[a] != static_cast<uint64_t>(ch.t_end) - ch.t_start) found(SAM_BAD_TCONS);
  if (X.Q[b] - X.Q[a] != static_cast<uint64_t>(ch.q_end) - ch.q_start) found(SAM_BAD_QCONS);
  const uint32_t parent = X.ranks[i].parent;
  if (!(parent < X.n_chains && X.chains[parent].query == ch.query && X.ranks[parent].parent == parent)) found(SAM_BAD_RANK);
  if (X.mates && X.mates[i].cls == 1) {
    const uint32_t m = X.mates[i].mate;
    if (!(m < X.n_chains && X.chains[m].query == (ch.query ^ 1u) && X.mates[m].cls == 1 && X.mates[m].mate == i)) found(SAM_BAD_MATE);
  }
  if (what != ~0u) sam_bad(bad, i, what);
}

// S5, S10: what a run writes into its line's CIGAR (cw) and MD (mw), in bytes
__global__ __launch_bounds__(256) void k_sam_widths(SamTables X, const uint32_t *run_chain, uint32_t *cw, uint32_t *mw) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= X.n_runs) return;
  const uint32_t i = run_chain[u], len = X.ops[u] >> 4, op = X.ops[u] & 15;
  const uint32_t a = static_cast<uint32_t>(X.off[i]), b = static_cast<uint32_t>(X.off[i + 1]);
  uint32_t       w = dec_dig(len) + 1;
  if (!X.eqx && sam_is_m(op)) { // the stretch's last run writes the M
    const bool tail = u + 1 == b || !sam_is_m(X.ops[u + 1] & 15);
    w = tail ? dec_dig(X.T[u + 1] - X.T[X.mhead[u]]) + 1 : 0;
  }
  cw[u] = w;
  if (X.md) {
    const uint32_t p = X.pe[u] > a ? X.pe[u] : a;
    const uint32_t d = dec_dig(X.E[u] - X.E[p]); // the count in front of the run
    mw[u] = op == SAM_X ? d + 1 + 2 * (len - 1) : op == SAM_D ? d + 1 + len : 0;
  }
}

// S4: the greatest (score, smallest index) of a query record's primaries, one atomic per primary
__global__ __launch_bounds__(256) void k_sam_rep(const msgpu_map_chain *chains, const msgpu_map_rank *ranks, uint32_t n, kf_ull *vkey) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && ranks[i].parent == i)
    atomicMax(&vkey[chains[i].query], (static_cast<kf_ull>(static_cast<uint32_t>(chains[i].score) ^ 0x80000000u) << 32) | (0xffffffffu - i));
}

// S8: every chain's FLAG and mate line
__global__ __launch_bounds__(256) void k_sam_chain_rows(SamTables X, uint32_t *cflag, uint32_t *cmate) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n_chains) return;
  const msgpu_map_chain ch = X.chains[i];
  uint32_t              flag = ch.strand ? 0x10u : 0u, ml = SAM_NONE;
  if (X.ranks[i].parent != i) flag |= 0x100u;
  else if (sam_rep(X.vkey, ch.query) != i) flag |= 0x800u;
  if (X.mates) {
    flag |= 1u | (ch.query & 1u ? 0x80u : 0x40u);
    if (X.mates[i].cls == 1) {
      flag |= 2u;
      ml = X.mates[i].mate;
    } else ml = sam_rep(X.vkey, ch.query ^ 1u);
    flag |= ml == SAM_NONE ? 8u : X.chains[ml].strand ? 0x20u : 0u;
  }
  cflag[i] = flag;
  cmate[i] = ml;
}

// S3, S11: first[r] = the first chain of a query record >= r (n_q + 1 entries); the text bound of every chain's line
__global__ __launch_bounds__(256) void k_sam_first(const msgpu_map_chain *chains, uint32_t n_chains, uint32_t n_q, uint32_t *first) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r > n_q) return;
  uint32_t lo = 0, hi = n_chains;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (chains[mid].query < r) lo = mid + 1;
    else hi = mid;
  }
  first[r] = lo;
}
__global__ __launch_bounds__(256) void k_sam_chain_bound(SamTables X, SeqRecs Q, uint64_t *cb) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n_chains) return;
  const msgpu_map_chain ch = X.chains[i];
  const uint64_t        runs = X.off[i + 1] - X.off[i];
  cb[i] = MSGPU_SAM_LINE_FIXED + Q.len[ch.query] + 11 * (runs + 2) + (X.md ? 2ull * (ch.t_end - ch.t_start) + 11 * (runs + 1) : 0);
}
// per query record its lines and their text bound
__global__ __launch_bounds__(256) void k_sam_records(const uint32_t *first, const uint64_t *CB, SeqRecs Q, uint32_t unmapped, uint32_t *rl, uint64_t *rb) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= Q.n) return;
  const uint32_t nc = first[r + 1] - first[r];
  rl[r] = nc ? nc : unmapped;
  rb[r] = nc ? CB[first[r + 1]] - CB[first[r]] : unmapped ? MSGPU_SAM_LINE_FIXED + Q.len[r] : 0;
}

struct SamF { // the fields of one line: every lane of the line's group holds the same
  uint32_t  chain, query, flag;
  uint32_t  rname;          // the target record, SAM_NONE: '*'
  uint32_t  rnext_kind, rnext; // 0: '*', 1: '=', 2: the name of target rnext
  uint32_t  pos, mapq, pnext;
  long long tlen;
  uint32_t  lclip, rclip, clip; // clip: 'S' or 'H'
  uint32_t  a, b;               // the runs
  uint64_t  cig_len;            // 0: '*'
  uint32_t  seq_s, seq_n, seq_rc; // bytes [seq_s, seq_s + seq_n) of the record, reverse-complemented on request; 0 bytes: '*'
  uint32_t  nm, cm, nb, has_s2, has_nb, tp;
  int32_t   as, s2;
  uint64_t  md_len, md_final;
};

__device__ inline SamF sam_fields(const SamTables &X, const SeqRecs &Q, uint32_t chain, uint32_t query) {
  SamF       f{};
  const bool paired = X.mates != nullptr;
  f.chain = chain;
  f.query = query;
  f.rname = SAM_NONE;
  if (chain == SAM_NONE) { // S9
    const uint32_t ml = paired ? sam_rep(X.vkey, query ^ 1u) : SAM_NONE;
    f.flag = 4u | (paired ? 1u | (query & 1u ? 0x80u : 0x40u) : 0u);
    if (ml != SAM_NONE) {
      const msgpu_map_chain mc = X.chains[ml];
      f.flag |= mc.strand ? 0x20u : 0u;
      f.rname      = mc.target;
      f.pos        = mc.t_start + 1;
      f.rnext_kind = 1;
      f.pnext      = f.pos;
    } else if (paired) f.flag |= 8u;
    f.seq_n = Q.len[query];
    return f;
  }
  const msgpu_map_chain ch = X.chains[chain];
  const msgpu_map_rank  rk = X.ranks[chain];
  const uint32_t        qlen = Q.len[ch.query], ml = X.cmate[chain];
  f.flag  = X.cflag[chain];
  f.rname = ch.target;
  f.pos   = ch.t_start + 1;
  f.mapq  = rk.mapq;
  f.lclip = ch.strand ? qlen - ch.q_end : ch.q_start;
  f.rclip = ch.strand ? ch.q_start : qlen - ch.q_end;
  f.clip  = f.flag & 0x900u ? 'H' : 'S';
  f.a     = static_cast<uint32_t>(X.off[chain]);
  f.b     = static_cast<uint32_t>(X.off[chain + 1]);
  f.cig_len = X.CW[f.b] - X.CW[f.a] + (f.lclip ? dec_dig(f.lclip) + 1 : 0) + (f.rclip ? dec_dig(f.rclip) + 1 : 0);
  if (!(f.flag & 0x900u)) f.seq_n = qlen; // S6: the whole read; the aligned part; nothing
  else if (f.flag & 0x800u) {
    f.seq_s = ch.q_start;
    f.seq_n = ch.q_end - ch.q_start;
  }
  f.seq_rc = ch.strand;
  if (paired) { // S8
    if (ml != SAM_NONE) {
      const msgpu_map_chain mc = X.chains[ml];
      f.rnext_kind = mc.target == ch.target ? 1 : 2;
      f.rnext      = mc.target;
      f.pnext      = mc.t_start + 1;
      if (mc.target == ch.target) {
        const uint32_t  lo = ch.t_start < mc.t_start ? ch.t_start : mc.t_start, hi = ch.t_end > mc.t_end ? ch.t_end : mc.t_end;
        const long long mag = static_cast<long long>(hi) - lo;
        f.tlen = ch.t_start < mc.t_start || (ch.t_start == mc.t_start && !(ch.query & 1u)) ? mag : -mag;
      }
    } else {
      f.rnext_kind = 1;
      f.pnext      = f.pos;
    }
    f.has_nb = X.mates[chain].cls == 1;
    f.nb     = X.mates[chain].n_best;
  }
  f.nm     = ch.nm;
  f.as     = ch.score;
  f.cm     = ch.n_anchors;
  f.has_s2 = !(f.flag & 0x100u);
  f.s2     = rk.sub;
  f.tp     = f.flag & 0x100u ? 'S' : 'P';
  if (X.md) { // S10: the runs' tokens and the final count
    const uint32_t p = X.pe[f.b] > f.a ? X.pe[f.b] : f.a;
    f.md_final = X.E[f.b] - X.E[p];
    f.md_len   = X.MW[f.b] - X.MW[f.a] + dec_dig(f.md_final);
  }
  return f;
}

__device__ inline uint64_t sam_size(const SamTables &X, const SamF &f) {
  const uint64_t qn = X.qn_off[f.query + 1] - X.qn_off[f.query];
  const uint64_t rn = f.rname == SAM_NONE ? 1 : X.tn_off[f.rname + 1] - X.tn_off[f.rname];
  const uint64_t nx = f.rnext_kind == 2 ? X.tn_off[f.rnext + 1] - X.tn_off[f.rnext] : 1;
  uint64_t       n = qn + 1 + dec_dig(f.flag) + 1 + rn + 1 + dec_dig(f.pos) + 1 + dec_dig(f.mapq) + 1 + (f.cig_len ? f.cig_len : 1) + 1 + nx + 1 +
               dec_dig(f.pnext) + 1 + dec_sdig(f.tlen) + 1 + (f.seq_n ? f.seq_n : 1) + 2;
  if (f.chain != SAM_NONE) {
    n += 6 + dec_dig(f.nm) + 6 + dec_sdig(f.as) + 6 + dec_dig(f.cm) + (f.has_s2 ? 6 + dec_sdig(f.s2) : 0) + 7 + (f.has_nb ? 6 + dec_dig(f.nb) : 0);
    if (X.md) n += 6 + f.md_len;
  }
  return n + 1;
}

// S3: line j of the run is chain first[r] + (j - L[r]) of its record r, or the record's unmapped line; its size and its class
__global__ __launch_bounds__(256) void k_sam_lines(SamTables X, SeqRecs Q, const uint32_t *first, const uint64_t *L, uint32_t q0, uint32_t q1,
                                                   uint32_t n_lines, msgpu_sam_line *lines, uint64_t *size, uint32_t *list_short, uint32_t *list_long,
                                                   kf_ull *cur_short, kf_ull *cur_long) {
  const uint32_t jj = blockIdx.x * 256 + threadIdx.x;
  bool           is_short = false, is_long = false;
  if (jj < n_lines) {
    const uint64_t j = L[q0] + jj;
    const uint32_t r = last_le(L, q0, q1, j); // L[r] <= j < L[r + 1]: a record with lines
    const uint32_t nc = first[r + 1] - first[r];
    const uint32_t chain = nc ? first[r] + static_cast<uint32_t>(j - L[r]) : SAM_NONE;
    const SamF     f = sam_fields(X, Q, chain, r);
    const uint64_t n = sam_size(X, f);
    lines[jj] = msgpu_sam_line{chain, r, f.flag, 0, 0};
    size[jj]  = n;
    is_short  = n <= MSGPU_SAM_SHORT_BYTES;
    is_long   = !is_short;
  }
  const uint64_t s = wave_append(is_short, cur_short), l = wave_append(is_long, cur_long);
  if (is_short) list_short[s] = jj; // (at most n_lines takers in all: the slot lies inside the list)
  if (is_long) list_long[l] = jj;
}

// the write pass of one line by the lanes t, t + stride, ... of its group
__device__ inline void sam_write_line(const SamTables &X, const SeqRecs &R, const SeqRecs &Q, const SamF &f, uint8_t *p, uint32_t t, uint32_t stride) {
  uint64_t w = 0;
  uint32_t k = 0; // the small pieces are numbered: piece k is lane k's
  auto copy = [&](const uint8_t *src, uint64_t n, bool tab) {
    if (tab && t == 0) p[w] = '\t';
    w += tab;
    for (uint64_t j = t; j < n; j += stride) p[w + j] = src[j];
    w += n;
  };
  auto one = [&](uint8_t c, bool tab) {
    if (t == k) {
      if (tab) p[w] = '\t';
      p[w + tab] = c;
    }
    ++k;
    w += 1 + tab;
  };
  auto num = [&](long long v) { // '\t' and the number
    const uint32_t d = dec_sdig(v);
    if (t == k) {
      p[w] = '\t';
      dec_sput(p + w + 1, v, d);
    }
    ++k;
    w += 1 + d;
  };
  auto tag = [&](char c0, char c1, long long v) { // '\t' and XX:i:<v>
    const uint32_t d = dec_sdig(v);
    if (t == k) {
      p[w] = '\t', p[w + 1] = c0, p[w + 2] = c1, p[w + 3] = ':', p[w + 4] = 'i', p[w + 5] = ':';
      dec_sput(p + w + 6, v, d);
    }
    ++k;
    w += 6 + d;
  };
  copy(X.qn + X.qn_off[f.query], X.qn_off[f.query + 1] - X.qn_off[f.query], false);
  num(f.flag);
  if (f.rname == SAM_NONE) one('*', true);
  else copy(X.tn + X.tn_off[f.rname], X.tn_off[f.rname + 1] - X.tn_off[f.rname], true);
  num(f.pos);
  num(f.mapq);
  if (!f.cig_len) one('*', true);
  else { // S5
    if (t == 0) p[w] = '\t';
    uint64_t c = w + 1;
    if (f.lclip) {
      const uint32_t d = dec_dig(f.lclip);
      if (t == k) {
        dec_put(p + c, f.lclip, d);
        p[c + d] = static_cast<uint8_t>(f.clip);
      }
      ++k;
      c += d + 1;
    }
    for (uint32_t u = f.a + t; u < f.b; u += stride) {
      const uint32_t cw = static_cast<uint32_t>(X.CW[u + 1] - X.CW[u]);
      if (!cw) continue; // (an = or X run inside a stretch that its last run writes)
      const uint32_t op = X.ops[u] & 15;
      const bool     m = !X.eqx && sam_is_m(op);
      const uint64_t len = m ? X.T[u + 1] - X.T[X.mhead[u]] : X.ops[u] >> 4;
      uint8_t       *at = p + c + (X.CW[u] - X.CW[f.a]);
      dec_put(at, len, cw - 1);
      at[cw - 1] = m ? 'M' : op == SAM_I ? 'I' : op == SAM_D ? 'D' : op == SAM_EQ ? '=' : 'X';
    }
    c += X.CW[f.b] - X.CW[f.a];
    if (f.rclip) {
      const uint32_t d = dec_dig(f.rclip);
      if (t == k) {
        dec_put(p + c, f.rclip, d);
        p[c + d] = static_cast<uint8_t>(f.clip);
      }
      ++k;
    }
    w += 1 + f.cig_len;
  }
  if (f.rnext_kind == 2) copy(X.tn + X.tn_off[f.rnext], X.tn_off[f.rnext + 1] - X.tn_off[f.rnext], true);
  else one(f.rnext_kind ? '=' : '*', true);
  num(f.pnext);
  num(f.tlen);
  if (!f.seq_n) one('*', true);
  else { // S6: single bytes up to the first aligned word, words of four bytes, single bytes behind the last
    if (t == 0) p[w] = '\t';
    ++w;
    const uint8_t *src = Q.bases + Q.off[f.query] + f.seq_s;
    const uint32_t n = f.seq_n, rc = f.seq_rc;
    auto           at = [&](uint32_t j) { return text_base(rc ? src[n - 1 - j] : src[j], rc); };
    uint32_t       head = static_cast<uint32_t>((4 - (reinterpret_cast<uintptr_t>(p + w) & 3)) & 3);
    head = head < n ? head : n;
    const uint32_t words = (n - head) >> 2, tail = head + 4 * words;
    if (t < head) p[w + t] = at(t);
    for (uint32_t x = t; x < words; x += stride) {
      const uint32_t j = head + 4 * x;
      *reinterpret_cast<uint32_t *>(p + w + j) = at(j) | at(j + 1) << 8 | at(j + 2) << 16 | static_cast<uint32_t>(at(j + 3)) << 24;
    }
    if (tail + t < n && t < 3) p[w + tail + t] = at(tail + t);
    w += n;
  }
  one('*', true);
  if (f.chain != SAM_NONE) {
    tag('N', 'M', f.nm);
    tag('A', 'S', f.as);
    tag('c', 'm', f.cm);
    if (f.has_s2) tag('s', '2', f.s2);
    if (t == k) p[w] = '\t', p[w + 1] = 't', p[w + 2] = 'p', p[w + 3] = ':', p[w + 4] = 'A', p[w + 5] = ':', p[w + 6] = static_cast<uint8_t>(f.tp);
    ++k;
    w += 7;
    if (f.has_nb) tag('n', 'b', f.nb);
    if (X.md) { // S10: a lane per target column; the run's token lies at the scan of the widths, the final count behind them all
      if (t == k) p[w] = '\t', p[w + 1] = 'M', p[w + 2] = 'D', p[w + 3] = ':', p[w + 4] = 'Z', p[w + 5] = ':';
      ++k;
      w += 6;
      const uint32_t df = dec_dig(f.md_final);
      if (t == k) dec_put(p + w + f.md_len - df, f.md_final, df);
      ++k;
      const msgpu_map_chain ch = X.chains[f.chain];
      const uint8_t        *tb = R.bases + R.off[ch.target] + ch.t_start;
      const uint64_t        t0 = X.T[f.a];
      for (uint32_t x = t; x < ch.t_end - ch.t_start; x += stride) {
        const uint32_t u = last_le(X.T, f.a, f.b, t0 + x); // T[u] <= t0 + x < T[u + 1]: the run consumes target bases
        const uint32_t op = X.ops[u] & 15;
        if (op == SAM_EQ) continue;
        const uint32_t col = static_cast<uint32_t>(t0 + x - X.T[u]), pa = X.pe[u] > f.a ? X.pe[u] : f.a;
        const uint64_t count = X.E[u] - X.E[pa];
        const uint32_t d = dec_dig(count);
        uint8_t       *at = p + w + (X.MW[u] - X.MW[f.a]);
        const uint8_t  base = text_base(tb[x], 0);
        if (col == 0) {
          dec_put(at, count, d);
          at[d] = op == SAM_X ? base : '^';
        }
        if (op == SAM_D) at[d + 1 + col] = base;
        else if (col) at[d + 2 * col - 1] = '0', at[d + 2 * col] = base;
      }
      w += f.md_len;
    }
  }
  if (t == k) p[w] = '\n';
}

// the short class: a wavefront per line, four lines per workgroup
__global__ __launch_bounds__(256) void k_sam_write_short(SamTables X, SeqRecs R, SeqRecs Q, const uint32_t *list, uint32_t n_list, msgpu_sam_line *lines,
                                                         const uint64_t *O, uint64_t file_base, uint8_t *text) {
  const uint32_t li = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (li >= n_list) return;
  const uint32_t jj = list[li];
  const SamF     f = sam_fields(X, Q, lines[jj].chain, lines[jj].query);
  if (t == 0) lines[jj].offset = file_base + O[jj];
  sam_write_line(X, R, Q, f, text + O[jj], t, 64);
}
// the long class: SAM_SLICES workgroups per line
__global__ __launch_bounds__(256) void k_sam_write_long(SamTables X, SeqRecs R, SeqRecs Q, const uint32_t *list, msgpu_sam_line *lines, const uint64_t *O,
                                                        uint64_t file_base, uint8_t *text) {
  const uint32_t jj = list[blockIdx.x], t = blockIdx.y * 256 + threadIdx.x;
  const SamF     f = sam_fields(X, Q, lines[jj].chain, lines[jj].query);
  if (t == 0) lines[jj].offset = file_base + O[jj];
  sam_write_line(X, R, Q, f, text + O[jj], t, 256 * SAM_SLICES);
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_samctx : msgpu::StageCtx {
  SeqCtxHold  seq;
  ScalarBlock sc;
  int         open() {
    const int rc = msgpu_seq_create(device, &seq.p);
    return rc != MSGPU_OK ? rc : sc.create();
  }
};

struct msgpu_sam_result {
  msgpu_sam_stats              stats{};
  std::vector<msgpu_sam_line>  lines;
  std::vector<msgpu_sam_batch> batches;
  std::string                  text;
};

namespace {

enum { SAM_SC_BAD = 0, SAM_SC_TOTAL, SAM_SC_SHORT, SAM_SC_LONG };
static_assert(SAM_SC_LONG < SC_COUNT, "the scalar block");
static_assert(sizeof(msgpu_sam_stats) == 184 && sizeof(msgpu_sam_line) == 24 && sizeof(msgpu_sam_batch) == 64 && sizeof(msgpu_map_chain) == 48,
              "the C-ABI's sizes");

// (each begins with the words tests/sam_oracle.py uses for it)
const char *const SAM_WHAT[] = {"offsets (off[0] is not 0, or the run offsets decrease or exceed the run table)",
                                "query order (the chains are not ordered by query record)",
                                "strand (neither 0 nor 1)",
                                "query record (out of range)",
                                "target record (out of range)",
                                "target range (not t_start <= t_end <= tlen)",
                                "query range (not q_start <= q_end <= qlen)",
                                "run (a length of 0, or an op that is none of I, D, =, X)",
                                "target consumption (the runs do not consume t_end - t_start target bases)",
                                "query consumption (the runs do not consume q_end - q_start query bases)",
                                "rank (the parent is out of range, of another query record or no primary)",
                                "mates (the mate is out of range, not in the partner record or does not point back)"};

uint64_t sam_batch_bytes(uint64_t n_lines, uint64_t text_bound) { return SAM_BATCH_FIXED + SAM_BATCH_LINE * n_lines + text_bound; }

// S11: the mapper's greedy cut over the prefix sums of the records' lines and text bounds (n + 1 entries each); `unit` = 2 with
// mates (n is even then).  Returns the first record of the unit that fits no batch on its own, or n
uint32_t sam_cut(const uint64_t *lpre, const uint64_t *bpre, uint32_t n, uint32_t unit, uint64_t budget, std::vector<msgpu_sam_batch> &out) {
  out.clear();
  for (uint32_t first = 0; first < n;) {
    auto fits = [&](uint32_t end) {
      const uint64_t l = lpre[end] - lpre[first];
      return l < (1ull << 31) && sam_batch_bytes(l, bpre[end] - bpre[first]) <= budget;
    };
    if (!fits(first + unit)) return first;
    uint32_t lo = 1, hi = (n - first) / unit; // the last end that fits, in units behind `first`
    while (lo < hi) {
      const uint32_t mid = lo + ((hi - lo + 1) >> 1);
      if (fits(first + mid * unit)) lo = mid;
      else hi = mid - 1;
    }
    lo = first + lo * unit;
    msgpu_sam_batch b{};
    b.first_query = first;
    b.n_queries   = lo - first;
    b.n_lines     = lpre[lo] - lpre[first];
    b.text_bound  = bpre[lo] - bpre[first];
    b.bytes_bound = sam_batch_bytes(b.n_lines, b.text_bound);
    out.push_back(b);
    first = lo;
  }
  return n;
}

// S1's host checks and the names as the kernels read them: one behind the other with n + 1 offsets; `strip`: S7's "/1", "/2"
int sam_names(msgpu_samctx *c, const msgpu_seqfile *f, const char *what, bool unique, bool strip, std::string &bytes, std::vector<uint64_t> &off) {
  const uint32_t                  n = msgpu_seq_count(f);
  std::unordered_set<std::string> seen;
  off.assign(n + 1ull, 0);
  for (uint32_t r = 0; r < n; ++r) {
    std::string name = msgpu_seq_name(f, r);
    if (name.empty() || name.size() > 254) {
      snprintf(c->err, sizeof(c->err), "%s record %u: %s", what, r, name.empty() ? "an empty name" : "a name longer than 254 bytes");
      return MSGPU_E_ARG;
    }
    if (unique && !seen.insert(name).second) {
      snprintf(c->err, sizeof(c->err), "%s record %u: its name is that of an earlier record (%.200s)", what, r, name.c_str());
      return MSGPU_E_ARG;
    }
    if (strip && name.size() > 2 && name[name.size() - 2] == '/' && (name.back() == '1' || name.back() == '2')) name.resize(name.size() - 2);
    bytes += name;
    off[r + 1] = bytes.size();
  }
  return MSGPU_OK;
}

int sam_run(msgpu_samctx *c, const msgpu_sam_params &prm, const char *targets_path, const char *queries_path, const msgpu_map_chain *chains,
            uint64_t n_chains64, const uint32_t *ops, const uint64_t *off, const msgpu_map_rank *ranks, const msgpu_map_mate *mates,
            uint64_t budget_bytes, msgpu_sam_result *res) {
  msgpu_sam_stats &S = res->stats;
  hipStream_t      st = c->stream;
  DevArena         D, B; // the resident part; the batch
  StageClock       clock(st);
  int              rc;
  struct Drain { // on every way out the stream is idle before the copies' destinations and the arenas go
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{st};
  S.params = prm;

  const uint64_t n_runs64 = n_chains64 ? off[n_chains64] : 0;
  if (n_chains64 >= (1ull << 31) || n_runs64 >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "%llu chains with %llu runs; the limits are 2^31 - 1 of each", static_cast<kf_ull>(n_chains64),
             static_cast<kf_ull>(n_runs64));
    return MSGPU_E_ARG;
  }
  const uint32_t n_chains = static_cast<uint32_t>(n_chains64), n_runs = static_cast<uint32_t>(n_runs64);
  S.n_chains = n_chains;
  S.n_runs   = n_runs;

  const StageTimer loading;
  StageFile        FT, FQ;
  if ((rc = stage_load(c, D, targets_path, 1, "targets", FT)) != MSGPU_OK) return rc;
  if ((rc = stage_load(c, D, queries_path, 0, "queries", FQ)) != MSGPU_OK) return rc;
  S.load_ms = loading.ms();
  const SeqRecs &R = FT.recs, &Q = FQ.recs;
  S.n_targets = R.n;
  S.n_queries = Q.n;
  if (mates && (Q.n & 1u)) {
    snprintf(c->err, sizeof(c->err), "mates: %u query records; interleaved pairs have an even number", Q.n);
    return MSGPU_E_ARG;
  }

  // ---- S1's host checks, S2, the names
  std::string           tn, qn;
  std::vector<uint64_t> tn_off, qn_off;
  try {
    if ((rc = sam_names(c, FT.f, "target", true, false, tn, tn_off)) != MSGPU_OK) return rc;
    if ((rc = sam_names(c, FQ.f, "query", false, mates != nullptr, qn, qn_off)) != MSGPU_OK) return rc;
    res->text = "@HD\tVN:1.6\tSO:unsorted\tGO:query\n";
    for (uint32_t r = 0; r < R.n; ++r)
      res->text.append("@SQ\tSN:").append(tn, tn_off[r], tn_off[r + 1] - tn_off[r]).append("\tLN:").append(std::to_string(msgpu_seq_length(FT.f, r))).append("\n");
    res->text += "@PG\tID:muchsalsa_amd\tPN:muchsalsa_amd\n";
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  S.header_bytes = res->text.size();

  kf_ull *d_bad = reinterpret_cast<kf_ull *>(c->sc.d + SAM_SC_BAD);
  STAGE_HIP(c, hipMemsetAsync(d_bad, 0xff, 8, st));

  // ---- the resident tables
  msgpu_map_chain *d_chains;
  msgpu_map_rank  *d_ranks;
  msgpu_map_mate  *d_mates = nullptr;
  uint64_t        *d_off, *d_T, *d_Q, *d_E, *d_CW, *d_MW = nullptr, *d_tn_off, *d_qn_off;
  uint32_t        *d_ops, *d_run_chain, *d_tc, *d_qc, *d_ec, *d_head, *d_ev, *d_mhead = nullptr, *d_pe = nullptr, *d_cw, *d_mw = nullptr;
  uint8_t         *d_tn, *d_qn;
  STAGE_HIP(c, D.get(&d_chains, n_chains));
  STAGE_HIP(c, D.get(&d_ranks, n_chains));
  if (mates) STAGE_HIP(c, D.get(&d_mates, n_chains));
  STAGE_HIP(c, D.get_zeroed(&d_off, n_chains + 1ull, st));
  STAGE_HIP(c, D.get(&d_ops, n_runs));
  STAGE_HIP(c, D.get(&d_run_chain, n_runs));
  STAGE_HIP(c, D.get_zeroed(&d_tc, n_runs + 1ull, st)); // (a zero behind the last run: the scans give n_runs + 1 values)
  STAGE_HIP(c, D.get_zeroed(&d_qc, n_runs + 1ull, st));
  STAGE_HIP(c, D.get_zeroed(&d_ec, n_runs + 1ull, st));
  STAGE_HIP(c, D.get_zeroed(&d_head, n_runs + 1ull, st));
  STAGE_HIP(c, D.get_zeroed(&d_ev, n_runs + 1ull, st));
  STAGE_HIP(c, D.get(&d_T, n_runs + 1ull));
  STAGE_HIP(c, D.get(&d_Q, n_runs + 1ull));
  STAGE_HIP(c, D.get(&d_E, n_runs + 1ull));
  STAGE_HIP(c, D.get_zeroed(&d_cw, n_runs + 1ull, st));
  STAGE_HIP(c, D.get(&d_CW, n_runs + 1ull));
  if (!prm.eqx) STAGE_HIP(c, D.get(&d_mhead, n_runs + 1ull));
  if (prm.md) {
    STAGE_HIP(c, D.get(&d_pe, n_runs + 1ull));
    STAGE_HIP(c, D.get_zeroed(&d_mw, n_runs + 1ull, st));
    STAGE_HIP(c, D.get(&d_MW, n_runs + 1ull));
  }
  STAGE_HIP(c, D.get(&d_tn, tn.size()));
  STAGE_HIP(c, D.get(&d_qn, qn.size()));
  STAGE_HIP(c, D.get(&d_tn_off, R.n + 1ull));
  STAGE_HIP(c, D.get(&d_qn_off, Q.n + 1ull));
  if (n_chains) {
    STAGE_HIP(c, hipMemcpyAsync(d_chains, chains, n_chains * sizeof(msgpu_map_chain), hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_ranks, ranks, n_chains * sizeof(msgpu_map_rank), hipMemcpyHostToDevice, st));
    if (mates) STAGE_HIP(c, hipMemcpyAsync(d_mates, mates, n_chains * sizeof(msgpu_map_mate), hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_off, off, (n_chains + 1ull) * 8, hipMemcpyHostToDevice, st));
  }
  if (n_runs) STAGE_HIP(c, hipMemcpyAsync(d_ops, ops, n_runs * 4ull, hipMemcpyHostToDevice, st));
  if (!tn.empty()) STAGE_HIP(c, hipMemcpyAsync(d_tn, tn.data(), tn.size(), hipMemcpyHostToDevice, st));
  if (!qn.empty()) STAGE_HIP(c, hipMemcpyAsync(d_qn, qn.data(), qn.size(), hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_tn_off, tn_off.data(), (R.n + 1ull) * 8, hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_qn_off, qn_off.data(), (Q.n + 1ull) * 8, hipMemcpyHostToDevice, st));

  // ---- S1
  // The smallest bad chain is wanted, and of it the first violated check.  A bad offset is found first, as nothing else of
  // the run tables can be read without the offsets; the chains in front of it (n_ok of them, their runs in front of
  // off[n_ok]) still go through every other check, and only if they pass is the offset the answer.
  auto bad_chain = [&](uint64_t &bad) -> int { // through the scalar block; ~0: none
    const int r2 = c->sc.read(c);
    bad = c->sc.h[SAM_SC_BAD];
    return r2;
  };
  auto report = [&](uint64_t bad) -> int {
    snprintf(c->err, sizeof(c->err), "chain %llu: %s", static_cast<kf_ull>(bad >> 4), SAM_WHAT[bad & 15]);
    return MSGPU_E_ARG;
  };
  uint64_t bad_off = ~0ull, bad_any = ~0ull;
  STAGE_HIP(c, clock.begin(&S.validate_ms));
  if (n_chains) hipLaunchKernelGGL(k_sam_check_off, dim3(grid256(n_chains)), dim3(256), 0, st, d_off, n_chains, n_runs64, d_bad);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if ((rc = bad_chain(bad_off)) != MSGPU_OK) return rc;
  const uint32_t n_ok = bad_off == ~0ull ? n_chains : static_cast<uint32_t>(bad_off >> 4);
  const uint32_t runs_ok = n_ok ? static_cast<uint32_t>(off[n_ok]) : 0; // (<= n_runs: chain n_ok - 1 passed the check)
  STAGE_HIP(c, clock.begin(&S.scan_ms));
  if (runs_ok)
    hipLaunchKernelGGL(k_sam_runs, dim3(grid256(runs_ok)), dim3(256), 0, st, d_off, n_ok, d_ops, runs_ok, d_run_chain, d_tc, d_qc, d_ec, d_head, d_ev, d_bad);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_tc, d_T, n_runs + 1ull));
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_qc, d_Q, n_runs + 1ull));
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_ec, d_E, n_runs + 1ull));
  STAGE_HIP(c, clock.end());
  kf_ull   *d_vkey;
  uint32_t *d_cflag, *d_cmate;
  STAGE_HIP(c, D.get_zeroed(&d_vkey, Q.n, st));
  STAGE_HIP(c, D.get(&d_cflag, n_chains));
  STAGE_HIP(c, D.get(&d_cmate, n_chains));
  const SamTables X{d_chains, d_ranks, d_mates, d_off, d_ops, d_T, d_Q, d_E, d_mhead, d_pe, d_CW, d_MW, d_vkey, d_cflag, d_cmate, d_tn, d_qn,
                    d_tn_off, d_qn_off, n_chains, n_runs, static_cast<uint32_t>(prm.eqx), static_cast<uint32_t>(prm.md), static_cast<uint32_t>(prm.unmapped)};
  STAGE_HIP(c, clock.begin(&S.validate_ms));
  if (n_ok) hipLaunchKernelGGL(k_sam_check_chain, dim3(grid256(n_ok)), dim3(256), 0, st, X, n_ok, R, Q, d_bad);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if ((rc = bad_chain(bad_any)) != MSGPU_OK) return rc;
  if (bad_any != ~0ull) return report(bad_any); // no kernel below runs on a table that breaks S1

  // ---- S5, S10: the runs' widths and their scans
  STAGE_HIP(c, clock.begin(&S.scan_ms));
  if (!prm.eqx)
    STAGE_HIP(c, stage_rocprim(D, [&](void *t, size_t &b) {
      return rocprim::inclusive_scan(t, b, static_cast<const uint32_t *>(d_head), d_mhead, n_runs + 1ull, rocprim::maximum<uint32_t>(), st);
    }));
  if (prm.md)
    STAGE_HIP(c, stage_rocprim(D, [&](void *t, size_t &b) {
      return rocprim::exclusive_scan(t, b, static_cast<const uint32_t *>(d_ev), d_pe, 0u, n_runs + 1ull, rocprim::maximum<uint32_t>(), st);
    }));
  if (n_runs) hipLaunchKernelGGL(k_sam_widths, dim3(grid256(n_runs)), dim3(256), 0, st, X, d_run_chain, d_cw, d_mw);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_cw, d_CW, n_runs + 1ull));
  if (prm.md) STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_mw, d_MW, n_runs + 1ull));
  STAGE_HIP(c, clock.end());

  // ---- S4, S8: roles, FLAG and mate lines; S3, S11: the records' lines and text bounds
  uint32_t *d_first, *d_rl;
  uint64_t *d_cb, *d_CB, *d_rb, *d_L, *d_Bd;
  STAGE_HIP(c, D.get(&d_first, Q.n + 1ull));
  STAGE_HIP(c, D.get_zeroed(&d_cb, n_chains + 1ull, st));
  STAGE_HIP(c, D.get(&d_CB, n_chains + 1ull));
  STAGE_HIP(c, D.get_zeroed(&d_rl, Q.n + 1ull, st));
  STAGE_HIP(c, D.get_zeroed(&d_rb, Q.n + 1ull, st));
  STAGE_HIP(c, D.get(&d_L, Q.n + 1ull));
  STAGE_HIP(c, D.get(&d_Bd, Q.n + 1ull));
  STAGE_HIP(c, clock.begin(&S.roles_ms));
  if (n_chains) {
    hipLaunchKernelGGL(k_sam_rep, dim3(grid256(n_chains)), dim3(256), 0, st, d_chains, d_ranks, n_chains, d_vkey);
    hipLaunchKernelGGL(k_sam_chain_rows, dim3(grid256(n_chains)), dim3(256), 0, st, X, d_cflag, d_cmate);
    hipLaunchKernelGGL(k_sam_chain_bound, dim3(grid256(n_chains)), dim3(256), 0, st, X, Q, d_cb);
  }
  hipLaunchKernelGGL(k_sam_first, dim3(grid256(Q.n + 1ull)), dim3(256), 0, st, d_chains, n_chains, Q.n, d_first);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint64_t *>(D, st, d_cb, d_CB, n_chains + 1ull));
  if (Q.n) hipLaunchKernelGGL(k_sam_records, dim3(grid256(Q.n)), dim3(256), 0, st, d_first, d_CB, Q, X.unmapped, d_rl, d_rb);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_rl, d_L, Q.n + 1ull));
  STAGE_HIP(c, stage_scan<const uint64_t *>(D, st, d_rb, d_Bd, Q.n + 1ull));
  STAGE_HIP(c, clock.end());
  std::vector<uint64_t> lpre, bpre;
  try {
    lpre.resize(Q.n + 1ull);
    bpre.resize(Q.n + 1ull);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, hipMemcpyAsync(lpre.data(), d_L, (Q.n + 1ull) * 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(bpre.data(), d_Bd, (Q.n + 1ull) * 8, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipStreamSynchronize(st));
  const uint64_t n_lines = lpre[Q.n];
  if (n_lines >= (1ull << 32)) {
    snprintf(c->err, sizeof(c->err), "%llu lines; the limit is 2^32 - 1", static_cast<kf_ull>(n_lines));
    return MSGPU_E_ARG;
  }

  // ---- S11: the budget, the cut, one reservation for the largest batch
  uint64_t budget = budget_bytes;
  if (!budget) {
    size_t free_b = 0, total_b = 0;
    STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
    budget = free_b;
  }
  const uint32_t unit = mates ? 2 : 1;
  for (;;) {
    const uint32_t bad = sam_cut(lpre.data(), bpre.data(), Q.n, unit, budget, res->batches);
    if (bad != Q.n) {
      const uint64_t l = lpre[bad + unit] - lpre[bad], b = bpre[bad + unit] - bpre[bad];
      char           who[96];
      if (mates) snprintf(who, sizeof(who), "pair %u (query records %u and %u)", bad / 2, bad, bad + 1);
      else snprintf(who, sizeof(who), "query record %u", bad);
      if (l >= (1ull << 31)) {
        snprintf(c->err, sizeof(c->err), "%s has %llu lines; the limit of a batch is 2^31 - 1", who, static_cast<kf_ull>(l));
        return MSGPU_E_ARG;
      }
      snprintf(c->err, sizeof(c->err), "%s with %llu lines and a text bound of %llu bytes needs %llu bytes on its own; the budget of a batch is %llu "
               "bytes (S11: a record is not split)", who, static_cast<kf_ull>(l), static_cast<kf_ull>(b), static_cast<kf_ull>(sam_batch_bytes(l, b)),
               static_cast<kf_ull>(budget));
      return MSGPU_E_NOMEM;
    }
    uint64_t reserve = 0;
    for (const msgpu_sam_batch &b : res->batches)
      if (b.n_lines) reserve = std::max(reserve, b.bytes_bound);
    const hipError_t e = reserve ? B.reserve(reserve) : hipSuccess;
    if (e == hipErrorOutOfMemory && !budget_bytes && budget > SAM_BATCH_FIXED) {
      (void)hipGetLastError(); // the free memory is not one block's: the budget that 0 stands for shrinks by an eighth
      budget -= budget / 8;
      continue;
    }
    STAGE_HIP(c, e);
    break;
  }
  S.budget_bytes = budget;
  S.n_batches    = res->batches.size();

  // ---- per batch: the line table, the sizes, their scan, the text
  try {
    res->lines.resize(n_lines);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  kf_ull *d_cur_short = reinterpret_cast<kf_ull *>(c->sc.d + SAM_SC_SHORT), *d_cur_long = reinterpret_cast<kf_ull *>(c->sc.d + SAM_SC_LONG);
  uint64_t line0 = 0;
  for (msgpu_sam_batch &b : res->batches) {
    const uint32_t n = static_cast<uint32_t>(b.n_lines);
    if (!n) continue;
    STAGE_HIP(c, B.rewind());
    msgpu_sam_line *d_lines;
    uint64_t       *d_size, *d_O;
    uint32_t       *d_short, *d_long;
    STAGE_HIP(c, B.get(&d_lines, n));
    STAGE_HIP(c, B.get_zeroed(&d_size, n + 1ull, st));
    STAGE_HIP(c, B.get(&d_O, n + 1ull));
    STAGE_HIP(c, B.get(&d_short, n));
    STAGE_HIP(c, B.get(&d_long, n));
    STAGE_HIP(c, hipMemsetAsync(d_cur_short, 0, 16, st)); // (both cursors: neighbours in the scalar block)
    STAGE_HIP(c, clock.begin(&S.format_ms));
    hipLaunchKernelGGL(k_sam_lines, dim3(grid256(n)), dim3(256), 0, st, X, Q, d_first, d_L, b.first_query, b.first_query + b.n_queries, n, d_lines, d_size,
                       d_short, d_long, d_cur_short, d_cur_long);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_scan<const uint64_t *>(B, st, d_size, d_O, n + 1ull));
    hipLaunchKernelGGL(k_stage_put<uint64_t>, dim3(1), dim3(64), 0, st, c->sc.d, SAM_SC_TOTAL, d_O + n);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    if ((rc = c->sc.read(c)) != MSGPU_OK) return rc;
    const uint64_t bytes = c->sc.h[SAM_SC_TOTAL];
    b.n_short    = c->sc.h[SAM_SC_SHORT];
    b.n_long     = c->sc.h[SAM_SC_LONG];
    b.text_bytes = bytes;
    if (bytes > b.text_bound || b.n_short + b.n_long != n) { // (S11's bound holds for every line, or the kernels are wrong)
      snprintf(c->err, sizeof(c->err), "batch at query record %u: %llu bytes of text against a bound of %llu, %llu + %llu lines by class of %u",
               b.first_query, static_cast<kf_ull>(bytes), static_cast<kf_ull>(b.text_bound), static_cast<kf_ull>(b.n_short), static_cast<kf_ull>(b.n_long), n);
      return MSGPU_E_STATE;
    }
    uint8_t *d_text;
    STAGE_HIP(c, B.get(&d_text, bytes + 16));
    const uint64_t file_base = res->text.size();
    try {
      res->text.resize(file_base + bytes);
    } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
    STAGE_HIP(c, clock.begin(&S.format_ms));
    if (b.n_short)
      hipLaunchKernelGGL(k_sam_write_short, dim3(grid_of(b.n_short, 4)), dim3(256), 0, st, X, R, Q, d_short, static_cast<uint32_t>(b.n_short), d_lines, d_O,
                         file_base, d_text);
    for (uint64_t at = 0; at < b.n_long; at += 32768) // (the grid's x)
      hipLaunchKernelGGL(k_sam_write_long, dim3(static_cast<uint32_t>(std::min<uint64_t>(32768, b.n_long - at)), SAM_SLICES), dim3(256), 0, st, X, R, Q,
                         d_long + at, d_lines, d_O, file_base, d_text);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
    STAGE_HIP(c, clock.begin(&S.copy_ms));
    STAGE_HIP(c, hipMemcpyAsync(&res->text[file_base], d_text, bytes, hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, hipMemcpyAsync(res->lines.data() + line0, d_lines, n * sizeof(msgpu_sam_line), hipMemcpyDeviceToHost, st));
    STAGE_HIP(c, clock.end());
    STAGE_HIP(c, hipStreamSynchronize(st));
    if (stage_verify(c, B) != MSGPU_OK) return MSGPU_E_HIP;
    b.bytes_peak = B.peak;
    S.bytes_peak = std::max<uint64_t>(S.bytes_peak, B.peak);
    S.n_short += b.n_short;
    S.n_long += b.n_long;
    line0 += n;
  }
  STAGE_HIP(c, hipStreamSynchronize(st));
  clock.collect();
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;
  for (const msgpu_sam_line &l : res->lines) {
    if (l.chain == SAM_NONE) ++S.n_unmapped;
    else if (l.flag & 0x100u) ++S.n_secondary;
    else if (l.flag & 0x800u) ++S.n_supplementary;
    else ++S.n_representative;
  }
  S.n_lines    = n_lines;
  S.bytes_out  = res->text.size();
  S.bytes_peak += D.peak;
  return MSGPU_OK;
}

} // namespace

extern "C" {

void msgpu_sam_default_params(msgpu_sam_params *p) {
  if (p) *p = msgpu_sam_params{1, 0, 1, 0};
}

int  msgpu_sam_create(int device, msgpu_samctx **out) { return stage_create(device, out); }
void msgpu_sam_destroy(msgpu_samctx *c) { stage_destroy(c); }

const char *msgpu_sam_last_error(const msgpu_samctx *c) { return c ? c->err : "null context"; }

uint64_t msgpu_sam_batch_bytes(const msgpu_sam_params *, uint64_t n_lines, uint64_t text_bound) { return sam_batch_bytes(n_lines, text_bound); }

int msgpu_sam_run(msgpu_samctx *c, const msgpu_sam_params *params, const char *targets_path, const char *queries_path, const msgpu_map_chain *chains,
                  uint64_t n_chains, const uint32_t *ops, const uint64_t *off, const msgpu_map_rank *ranks, const msgpu_map_mate *mates, uint32_t flags,
                  uint64_t budget_bytes, msgpu_sam_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out      = nullptr;
  c->err[0] = 0;
  if (!params || !targets_path || !queries_path || flags || (n_chains && (!chains || !off)) || (n_chains && off[n_chains] && !ops)) return MSGPU_E_ARG;
  const msgpu_sam_params p = *params;
  if ((p.eqx | 1) != 1 || (p.md | 1) != 1 || (p.unmapped | 1) != 1 || p.reserved) {
    snprintf(c->err, sizeof(c->err), "eqx = %d, md = %d, unmapped = %d (each 0 or 1), reserved = %d (0)", p.eqx, p.md, p.unmapped, p.reserved);
    return MSGPU_E_ARG;
  }
  if (n_chains && !ranks) {
    snprintf(c->err, sizeof(c->err), "no rank rows for %llu chains", static_cast<unsigned long long>(n_chains));
    return MSGPU_E_ARG;
  }
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_sam_result> res;
  try {
    res.reset(new msgpu_sam_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  const StageTimer wall;
  const uint64_t   lost0 = c->sc.lost;
  const int        rc = sam_run(c, p, targets_path, queries_path, chains, n_chains, ops, off, ranks, mates, budget_bytes, res.get());
  if (rc != MSGPU_OK) return rc;
  res->stats.n_lost_publications = c->sc.lost - lost0;
  res->stats.wall_ms             = wall.ms();
  *out                           = res.release();
  return MSGPU_OK;
}

int msgpu_sam_result_stats(const msgpu_sam_result *r, msgpu_sam_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

int msgpu_sam_result_lines(const msgpu_sam_result *r, const msgpu_sam_line **lines, uint64_t *n) {
  if (!r || !lines || !n) return MSGPU_E_ARG;
  *lines = r->lines.data();
  *n     = r->lines.size();
  return MSGPU_OK;
}

int msgpu_sam_result_batches(const msgpu_sam_result *r, const msgpu_sam_batch **batches, uint64_t *n) {
  if (!r || !batches || !n) return MSGPU_E_ARG;
  *batches = r->batches.data();
  *n       = r->batches.size();
  return MSGPU_OK;
}

const char *msgpu_sam_result_text(const msgpu_sam_result *r, uint64_t *len) {
  if (len) *len = r ? r->text.size() : 0;
  return r ? r->text.data() : "";
}

void msgpu_sam_result_free(msgpu_sam_result *r) {
  if (r) delete r;
}

} // extern "C"
