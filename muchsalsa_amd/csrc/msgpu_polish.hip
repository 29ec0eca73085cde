// msgpu_polish.hip -- the polishing stage: a pile-up consensus of a draft from the mapper's run tables (include/msgpu.h,
// "pileup consensus").  Every chain of reads against the draft arrives as runs len << 4 | op; the stage
// checks the tables on the device (rule 1), picks one voter per read (rule 2; in ranked form every primary of sufficient
// mapping quality, by the mapper's rule 12 rows), walks every column of every voter into six
// integer counters per draft base (rules 3 and 4), collects, sorts and counts the insertion events (rules 4 and 6), calls
// every position (rule 5), and writes the polished records through msgpu_fasta_format (rule 7).
//
// The shape of the device work.  A run's start in the target and in the oriented query is the exclusive scan of what the runs
// consume minus the scan's value at the chain's first run: one global 64-bit scan per side serves as the segmented scan, and
// the consumption check of rule 1 reads the same sums.  The pile-up (k_pl_pileup) does not walk runs at all: the target span
// [t_start, t_end) of a voter holds exactly one '=', X or D column per position, so the columns of all voters are numbered by
// the scan of the voters' spans and every lane takes one column -- lanes of a wavefront lie on consecutive target positions
// whether the chain is one run of 5,000 columns or 200 runs of a few.  A lane finds its chain and its run by two binary
// searches over the scans.  The counters are planar by class (six rows of one 32-bit word per draft base): the 64 lanes of a
// wave instruction then add into stretches of 256 contiguous bytes of at most six rows, the shape global atomics run fastest
// at, where an interleaved layout (24 bytes per base) would spread the same adds over 1,536 bytes; and the call kernel reads
// every row coalesced.  Integer atomic adds are order-independent: the counters are exact and the same from run to run.
#include <hip/hip_runtime.h>

#include <memory>
#include <new>
#include <string>

#include "msgpu_polish.h"

namespace msgpu {

constexpr uint32_t PL_I = 1, PL_D = 2, PL_EQ = 7, PL_X = 8;
constexpr uint32_t PL_MAX_INS = 32;
// rule 1: what can be wrong with a chain, in the order in which one chain's violations are looked at
enum { PL_BAD_ORDER = 0, PL_BAD_STRAND, PL_BAD_QREC, PL_BAD_TREC, PL_BAD_TRANGE, PL_BAD_QRANGE, PL_BAD_RUN, PL_BAD_TCONS, PL_BAD_QCONS,
       PL_BAD_OFF, PL_BAD_RANK /* (j), ranked form only: behind every other violation of its chain */,
       PL_BAD_MATE /* (k), mates form only: likewise */ };
// (the classes of the counters, the counts PL_ST_* that the kernels add up, pl_class and pl_depth: msgpu_polish.h)

struct PlTables { // the chain table and the run tables with their scans
  const msgpu_map_chain *chains;
  const uint64_t        *off;  // n_chains + 1
  const uint32_t        *ops;  // n_runs
  const uint64_t        *T, *Q; // n_runs + 1: target / query bases that the runs in front of a run consume
  uint32_t               n_chains, n_runs;
};

__device__ inline void pl_bad(kf_ull *bad, uint32_t chain, uint32_t what) { atomicMin(bad, (static_cast<kf_ull>(chain) << 4) | what); }

// byte j of the chain's stretch of the oriented query, in the query store
__device__ inline uint8_t pl_query_byte(const SeqRecs &Q, const msgpu_map_chain &ch, uint64_t j) {
  const uint64_t qlen = Q.len[ch.query];
  const uint64_t fwd  = ch.strand ? qlen - 1 - (qlen - ch.q_end + j) : ch.q_start + j;
  return Q.bases[Q.off[ch.query] + fwd];
}

// rule 1, the offsets: nothing else of the tables can be read without them
__global__ __launch_bounds__(256) void k_pl_check_off(const uint64_t *off, uint32_t n_chains, uint64_t n_runs, kf_ull *bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_chains && (off[i + 1] < off[i] || off[i + 1] > n_runs)) pl_bad(bad, i, PL_BAD_OFF);
}

// the chain of every run; what the run consumes; rule 1 on the run itself
__global__ __launch_bounds__(256) void k_pl_runs(const uint64_t *off, uint32_t n_chains, const uint32_t *ops, uint32_t n_runs, uint32_t *run_chain,
                                                 uint32_t *tc, uint32_t *qc, kf_ull *bad) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  if (u >= n_runs) return;
  const uint32_t i = last_le(off, 0, n_chains, u); // off[0] = 0 <= u, and off[i + 1] > u as off[n_chains] = n_runs
  const uint32_t len = ops[u] >> 4, op = ops[u] & 15;
  const bool     ok = len >= 1 && (op == PL_I || op == PL_D || op == PL_EQ || op == PL_X);
  if (!ok) pl_bad(bad, i, PL_BAD_RUN);
  run_chain[u] = i;
  tc[u]        = ok && op != PL_I ? len : 0;
  qc[u]        = ok && op != PL_D ? len : 0;
}

// rule 1 on the chain's fields and on what its runs consume
__global__ __launch_bounds__(256) void k_pl_check_chain(PlTables X, SeqRecs R, SeqRecs Q, const msgpu_map_rank *ranks, const msgpu_map_mate *mates,
                                                        kf_ull *bad) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= X.n_chains) return;
  const msgpu_map_chain ch = X.chains[i];
  uint32_t              what = ~0u; // (none)
  auto                  found = [&](uint32_t w) { what = w < what ? w : what; };
  if (i && ch.query < X.chains[i - 1].query) found(PL_BAD_ORDER);
  if (ch.strand > 1) found(PL_BAD_STRAND);
  if (ch.query >= Q.n) found(PL_BAD_QREC);
  if (ch.target >= R.n) found(PL_BAD_TREC);
  if (ch.target < R.n && !(ch.t_start < ch.t_end && ch.t_end <= R.len[ch.target])) found(PL_BAD_TRANGE);
  if (ch.query < Q.n && !(ch.q_start <= ch.q_end && ch.q_end <= Q.len[ch.query])) found(PL_BAD_QRANGE);
  const uint64_t a = X.off[i], b = X.off[i + 1];
  if (X.T[b] - X.T[a] != static_cast<uint64_t>(ch.t_end) - ch.t_start) found(PL_BAD_TCONS);
  if (X.Q[b] - X.Q[a] != static_cast<uint64_t>(ch.q_end) - ch.q_start) found(PL_BAD_QCONS);
  if (ranks) { // (j): the parent is a chain of the table, of the same query record, and its own parent
    const msgpu_map_rank r = ranks[i];
    bool                 ok = r.parent < X.n_chains && r.mapq <= 60;
    if (ok) ok = X.chains[r.parent].query == ch.query && ranks[r.parent].parent == r.parent;
    if (!ok) found(PL_BAD_RANK);
  }
  if (mates) { // (k): cls is 0 or 1; a selected chain's mate is a chain of the table whose row names this one, of the pair's other record
    const msgpu_map_mate m = mates[i];
    bool                 ok = m.cls <= 1;
    if (ok && m.cls == 1) {
      ok = m.mate < X.n_chains && m.n_best >= 1;
      if (ok) ok = mates[m.mate].cls == 1 && mates[m.mate].mate == i && X.chains[m.mate].query == (ch.query ^ 1u);
    }
    if (!ok) found(PL_BAD_MATE);
  }
  if (what != ~0u) pl_bad(bad, i, what);
}

// rule 2 in two order-independent passes: the greatest (score, block) of a query's eligible chains, then the first chain that has it
__device__ inline bool pl_eligible(const msgpu_map_chain &ch, uint32_t min_identity) {
  return static_cast<uint64_t>(ch.matches) * 100 >= static_cast<uint64_t>(min_identity) * ch.block;
}
__device__ inline kf_ull pl_voter_key(const msgpu_map_chain &ch) {
  return (static_cast<kf_ull>(static_cast<uint32_t>(ch.score) ^ 0x80000000u) << 32) | ch.block;
}
__global__ __launch_bounds__(256) void k_pl_voter_key(const msgpu_map_chain *chains, uint32_t n, uint32_t min_identity, kf_ull *vkey) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && pl_eligible(chains[i], min_identity)) atomicMax(&vkey[chains[i].query], pl_voter_key(chains[i]));
}
__global__ __launch_bounds__(256) void k_pl_voter_idx(const msgpu_map_chain *chains, uint32_t n, uint32_t min_identity, const kf_ull *vkey,
                                                      uint32_t *vidx) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n && pl_eligible(chains[i], min_identity) && vkey[chains[i].query] == pl_voter_key(chains[i])) atomicMin(&vidx[chains[i].query], i);
}
// rule 2 in ranked form, one pass without an atomic: a chain votes iff it is eligible, primary and of sufficient mapping quality
__global__ __launch_bounds__(256) void k_pl_voter_ranked(const msgpu_map_chain *chains, const msgpu_map_rank *ranks, uint32_t n,
                                                         uint32_t min_identity, uint32_t min_mapq, uint32_t *vflag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) vflag[i] = pl_eligible(chains[i], min_identity) && ranks[i].parent == i && ranks[i].mapq >= min_mapq;
}
// rule 2 in mates form, likewise: a chain votes iff it is eligible, selected and its pair is placed best once
__global__ __launch_bounds__(256) void k_pl_voter_mates(const msgpu_map_chain *chains, const msgpu_map_mate *mates, uint32_t n, uint32_t min_identity,
                                                        uint32_t *vflag) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) vflag[i] = pl_eligible(chains[i], min_identity) && mates[i].cls == 1 && mates[i].n_best == 1;
}
// is chain i a voter: by its flag in ranked and in mates form, else as its query record's one voter
__device__ inline bool pl_votes(const msgpu_map_chain *chains, const uint32_t *vidx, const uint32_t *vflag, uint32_t i) {
  return vflag ? vflag[i] != 0 : vidx[chains[i].query] == i;
}
// the voters' spans (0 for every other chain), the counts, and the sum of the depths per draft record
__global__ __launch_bounds__(256) void k_pl_spans(const msgpu_map_chain *chains, uint32_t n, const uint32_t *vidx, const uint32_t *vflag,
                                                  uint32_t *span, kf_ull *rec_depth, kf_ull *st) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool     live = i < n, votes = live && pl_votes(chains, vidx, vflag, i);
  if (live) span[i] = votes ? chains[i].t_end - chains[i].t_start : 0;
  if (votes) atomicAdd(&rec_depth[chains[i].target], static_cast<kf_ull>(chains[i].t_end - chains[i].t_start));
  wave_count(votes, st + PL_ST_VOTERS);
  wave_count(live && !votes, st + PL_ST_IGNORED);
}

// rule 4, the columns: lane g takes column g of the voters' spans laid one behind the other (S = the scan of the spans)
__global__ __launch_bounds__(256) void k_pl_pileup(PlTables X, const uint64_t *S, uint64_t n_cols, SeqRecs R, SeqRecs Q, uint32_t *cnt, kf_ull *st) {
  const uint64_t g = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool     live = g < n_cols;
  uint32_t       op = 0;
  if (live) {
    const uint32_t        i = last_le(S, 0, X.n_chains, g); // S[i] <= g < S[i + 1]: a voter, the others have no columns
    const msgpu_map_chain ch = X.chains[i];
    const uint64_t        x = g - S[i]; // < t_end - t_start
    const uint32_t        a = static_cast<uint32_t>(X.off[i]), b = static_cast<uint32_t>(X.off[i + 1]);
    const uint64_t        t0 = X.T[a];
    const uint32_t        u = last_le(X.T, a, b, t0 + x); // T[u] <= t0 + x < T[u + 1]: the run consumes target bases
    op = X.ops[u] & 15;
    uint32_t cls = PL_DEL;
    if (op != PL_D) cls = pl_class(pl_query_byte(Q, ch, X.Q[u] - X.Q[a] + (t0 + x - X.T[u])), ch.strand);
    atomicAdd(&cnt[cls * R.n_bases + R.off[ch.target] + ch.t_start + x], 1u);
  }
  wave_count(op == PL_EQ, st + PL_ST_EQ);
  wave_count(op == PL_X, st + PL_ST_X);
  wave_count(op == PL_D, st + PL_ST_D);
}

// rule 4, the insertion events.  FILL = false: flag[u] = the run is a usable event at a slot 0 < p < tlen, and the counts;
// FILL = true: event E[u] = (slot in the store << 6 | L, the 2-bit packed letters, the first in the highest bits).
template <bool FILL>
__global__ __launch_bounds__(256) void k_pl_ins(PlTables X, const uint32_t *run_chain, const uint32_t *vidx, const uint32_t *vflag, SeqRecs R, SeqRecs Q, uint32_t *flag,
                                                const uint32_t *E, uint64_t *ev_key, uint64_t *ev_seq, kf_ull *st) {
  const uint32_t u = blockIdx.x * 256 + threadIdx.x;
  bool           ins = false, ends = false, usable = false;
  uint32_t       L = 0;
  if (u < X.n_runs && (X.ops[u] & 15) == PL_I && (!FILL || flag[u])) {
    const uint32_t        i = run_chain[u];
    const msgpu_map_chain ch = X.chains[i];
    if (pl_votes(X.chains, vidx, vflag, i)) {
      const uint32_t a = static_cast<uint32_t>(X.off[i]), b = static_cast<uint32_t>(X.off[i + 1]);
      ins  = true;
      L    = X.ops[u] >> 4;
      ends = u == a || u + 1 == b;
      if (!ends && L <= PL_MAX_INS) {
        const uint64_t j = X.Q[u] - X.Q[a];
        uint64_t       packed = 0;
        usable = true;
        for (uint32_t x = 0; x < L; ++x) {
          const uint32_t cls = pl_class(pl_query_byte(Q, ch, j + x), ch.strand);
          usable = usable && cls < PL_DEL;
          packed = packed << 2 | (cls & 3);
        }
        const uint64_t p = ch.t_start + (X.T[u] - X.T[a]);
        if (FILL) {
          ev_key[E[u]] = (R.off[ch.target] + p) << 6 | L;
          ev_seq[E[u]] = packed;
        } else {
          flag[u] = usable && p > 0 && p < R.len[ch.target];
        }
      }
    }
  }
  if (!FILL) {
    wave_add(L, st + PL_ST_I);
    wave_count(ends, st + PL_ST_ENDS);
    wave_count(usable, st + PL_ST_USABLE);
    wave_count(ins && !ends && !usable, st + PL_ST_UNUSABLE);
  }
}

// rule 6: the events sorted by (slot, L, letters).  head[e] = event e starts a group of equal events
__global__ __launch_bounds__(256) void k_pl_heads(const uint64_t *key, const uint64_t *seq, uint32_t n, uint32_t *head) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e < n) head[e] = e == 0 || key[e] != key[e - 1] || seq[e] != seq[e - 1];
}
// per slot the group with the greatest count; groups are numbered by (slot, L, letters), so the smaller number wins a tie
__global__ __launch_bounds__(256) void k_pl_best(const uint32_t *gstart, const uint32_t *n_groups, const uint64_t *key, kf_ull *best) {
  const uint32_t g = blockIdx.x * 256 + threadIdx.x;
  if (g >= *n_groups) return;
  const uint32_t e = gstart[g], count = gstart[g + 1] - e;
  atomicMax(&best[key[e] >> 6], (static_cast<kf_ull>(count) << 32) | (0xffffffffu - g));
}

struct PlCall { // rules 5 and 6 per byte of the draft's store
  const uint32_t *cnt;
  kf_ull         *best; // in: the slot's winner (0: none); out: 1 << 63 | its count << 32 | its first event when it is applied, else 0
  const uint32_t *gstart;
  const uint64_t *key;
  uint8_t        *call;   // 0: the draft's byte; 'A' 'C' 'G' 'T': that letter; 1: nothing
  uint32_t       *outlen; // bytes that the position emits
  kf_ull         *rec_sub, *rec_del, *rec_ins;
  uint32_t        min_depth;
};

__global__ __launch_bounds__(256) void k_pl_call(SeqRecs R, PlCall a, kf_ull *st) {
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  const uint32_t r = pos < R.n_bases ? seq_record(R, pos) : REC_NONE;
  int            kind = -1; // 0 verbatim, 1 unchanged, 2 substituted, 3 deleted
  uint32_t       depth = 0, ins_len = 0;
  if (r != REC_NONE) {
    uint32_t v[PL_CLASSES];
    for (int c = 0; c < PL_CLASSES; ++c) {
      v[c] = a.cnt[c * R.n_bases + pos];
      depth += v[c];
    }
    uint8_t out = 0;
    kind        = 0;
    if (depth >= a.min_depth && (v[PL_A] | v[PL_C] | v[PL_G] | v[PL_T] | v[PL_DEL])) {
      const uint32_t own = pl_class(R.bases[pos], 0); // PL_OTHER: a draft byte that is no base never wins a tie
      uint32_t       win = PL_A;
      for (uint32_t c = PL_C; c <= PL_DEL; ++c)
        if (v[c] > v[win]) win = c;
      if (own < PL_DEL && v[own] == v[win]) win = own;
      kind = win == own ? 1 : win == PL_DEL ? 3 : 2;
      out  = kind == 1 ? 0 : kind == 3 ? 1 : "ACGT"[win];
    }
    const kf_ull w = a.best[pos];
    kf_ull       keep = 0;
    if (w && pos > R.off[r]) { // (an event's slot is never a record's first position; the test keeps pos - 1 inside the record)
      const uint32_t count = static_cast<uint32_t>(w >> 32), e = a.gstart[0xffffffffu - static_cast<uint32_t>(w)];
      const uint32_t left = pl_depth(a.cnt, R.n_bases, pos - 1), m = left < depth ? left : depth;
      if (m >= a.min_depth && 2ull * count > m) {
        ins_len = static_cast<uint32_t>(a.key[e] & 63);
        keep    = PL_APPLIED | static_cast<kf_ull>(count) << 32 | e; // (count <= the events, below 2^31)
      }
    }
    a.best[pos]   = keep;
    a.call[pos]   = out;
    a.outlen[pos] = ins_len + (kind == 3 ? 0 : 1);
    if (kind == 2) atomicAdd(&a.rec_sub[r], 1ull);
    if (kind == 3) atomicAdd(&a.rec_del[r], 1ull);
    if (ins_len) atomicAdd(&a.rec_ins[r], 1ull);
  } else if (pos < R.n_bases) {
    a.outlen[pos] = 0;
    a.best[pos]   = 0;
  }
  wave_count(kind == 0, st + PL_ST_VERBATIM);
  wave_count(kind == 1, st + PL_ST_UNCHANGED);
  wave_count(kind == 2, st + PL_ST_SUBST);
  wave_count(kind == 3, st + PL_ST_DELETED);
  wave_count(ins_len != 0, st + PL_ST_APPLIED);
  wave_add(ins_len, st + PL_ST_INSERTED);
  wave_max(depth, st + PL_ST_MAXDEPTH);
}

// rule 7: every position's bytes at the scan of the lengths (O), the applied insertion in front of the call
__global__ __launch_bounds__(256) void k_pl_scatter(SeqRecs R, const uint8_t *call, const kf_ull *best, const uint64_t *key, const uint64_t *seq,
                                                    const uint32_t *outlen, const uint64_t *O, uint8_t *raw) {
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (pos >= R.n_bases || !outlen[pos]) return;
  uint64_t     w = O[pos];
  const kf_ull b = best[pos];
  if (b & PL_APPLIED) {
    const uint32_t e = static_cast<uint32_t>(b), L = static_cast<uint32_t>(key[e] & 63);
    const uint64_t s = seq[e];
    for (uint32_t x = 0; x < L; ++x) raw[w++] = "ACGT"[(s >> (2 * (L - 1 - x))) & 3];
  }
  if (call[pos] != 1) raw[w] = call[pos] ? call[pos] : R.bases[pos];
}
__global__ __launch_bounds__(256) void k_pl_reclen(SeqRecs R, const uint64_t *O, uint64_t *rec_start, uint64_t *rec_len) {
  const uint32_t r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R.n) return;
  rec_start[r] = O[R.off[r]];
  rec_len[r]   = O[R.off[r] + R.len[r]] - O[R.off[r]];
}

} // namespace msgpu

using namespace msgpu;

// ---- host side -----------------------------------------------------------------------------------------------------

struct msgpu_pl_result {
  msgpu_pl_stats               stats{};
  std::vector<msgpu_pl_record> records;
  std::string                  text;
  bool                         has_vcf = false; // MSGPU_PL_VCF
  VcfOut                       vcf;
};

// rule 8: `need` more bytes beside what the device holds already
int msgpu::pl_room(msgpu_plctx *c, uint64_t need, const char *what, uint64_t a, const char *a_name, uint64_t b, const char *b_name) {
  size_t free_b = 0, total_b = 0;
  STAGE_HIP(c, hipMemGetInfo(&free_b, &total_b));
  if (need <= free_b) return MSGPU_OK;
  snprintf(c->err, sizeof(c->err), "%s: %llu %s and %llu %s need %llu bytes of device memory beside the two stores; %zu are free", what,
           static_cast<kf_ull>(a), a_name, static_cast<kf_ull>(b), b_name, static_cast<kf_ull>(need), free_b);
  return MSGPU_E_NOMEM;
}

namespace {

static_assert(sizeof(msgpu_pl_variant) == 48 && sizeof(msgpu_pl_vcf_stats) == 120, "the C-ABI's sizes");
static_assert(sizeof(msgpu_pl_stats) == 256 && sizeof(msgpu_pl_record) == 48 && sizeof(msgpu_map_chain) == 48, "the C-ABI's sizes");

// (each begins with the words tests/pl_oracle.py uses for it)
const char *const PL_WHAT[] = {"query order (the chains are not ordered by query record)", "strand (neither 0 nor 1)",
                               "query record (out of range)", "target record (out of range)", "target range (not t_start < t_end <= tlen)",
                               "query range (not q_start <= q_end <= qlen)", "run (a length of 0, or an op that is none of I, D, =, X)",
                               "target consumption (the runs do not consume t_end - t_start target bases)",
                               "query consumption (the runs do not consume q_end - q_start query bases)",
                               "offsets (the run offsets decrease or exceed the run table)",
                               "rank (the parent is out of range, of another query record or no primary, or mapq exceeds 60)",
                               "mates (cls exceeds 1, or the mate is out of range, names another chain or is no mate of this read, or n_best is 0)"};

int pl_run(msgpu_plctx *c, const msgpu_pl_params &prm, const char *draft_path, const char *reads_path, const msgpu_map_chain *chains,
           uint64_t n_chains64, const uint32_t *ops, const uint64_t *off, const msgpu_map_rank *ranks, uint32_t min_mapq,
           const msgpu_map_mate *mates, bool vcf, msgpu_pl_result *res) {
  msgpu_pl_stats &S = res->stats;
  hipStream_t     st = c->stream;
  DevArena        D;
  StageClock      clock(st);
  int             rc;
  std::vector<uint64_t> h_rec[6]; // per draft record: start, length out, substitutions, deletions, insertions, sum of the depths
  uint64_t              h_st[PL_ST_COUNT];
  struct Drain { // on every way out the stream is idle before the copies' destinations and the arena go
    hipStream_t s;
    ~Drain() { (void)hipStreamSynchronize(s); }
  } drain{st};
  S.params = prm;

  const uint64_t n_runs64 = n_chains64 ? off[n_chains64] : 0;
  if (n_chains64 >= (1ull << 31) || n_runs64 >= (1ull << 31) || (n_chains64 && off[0] != 0)) {
    snprintf(c->err, sizeof(c->err), "%llu chains with %llu runs from offset %llu; the limits are 2^31 - 1 of each, from offset 0",
             static_cast<kf_ull>(n_chains64), static_cast<kf_ull>(n_runs64), static_cast<kf_ull>(n_chains64 ? off[0] : 0));
    return MSGPU_E_ARG;
  }
  const uint32_t n_chains = static_cast<uint32_t>(n_chains64), n_runs = static_cast<uint32_t>(n_runs64);
  S.n_chains = n_chains;
  S.n_runs   = n_runs;

  const StageTimer loading;
  StageFile        FT, FQ;
  if ((rc = stage_load(c, D, draft_path, 1, "draft", FT)) != MSGPU_OK) return rc;
  if ((rc = stage_load(c, D, reads_path, 0, "reads", FQ)) != MSGPU_OK) return rc;
  S.load_ms = loading.ms();
  const SeqRecs &R = FT.recs, &Q = FQ.recs;
  S.n_records    = R.n;
  S.n_bases      = R.n_bases;
  S.n_reads      = Q.n;
  S.n_read_bases = Q.n_bases;
  const uint64_t NB = R.n_bases;
  if (vcf && (rc = vcf_header(c, FT.f, res->vcf)) != MSGPU_OK) return rc; // V7, before any kernel

  // rule 8, what does not depend on the events: per draft byte the six counters, the slot's winner, the call, the output
  // length and its scan; per run the op, what it consumes on both sides with the two scans, its chain, the event flag and
  // its scan; per chain the entry, the offset, the span and its scan; per read the voter's key and index
  const uint64_t fixed_bytes = NB * (PL_CLASSES * 4ull + 8 + 1 + 4 + 8) + n_runs * (4ull + 4 + 4 + 8 + 8 + 4 + 4 + 4) +
                               n_chains * (sizeof(msgpu_map_chain) + 8ull + 4 + 8) + Q.n * 12ull + R.n * 48ull + (8ull << 20) +
                               (ranks || mates ? n_chains * (sizeof(msgpu_map_rank) + 4ull) : 0); // (ranked and mates form: the rows and the voters' flags)
  if ((rc = pl_room(c, fixed_bytes, "the pile-up", NB, "draft bases", n_runs, "runs")) != MSGPU_OK) return rc;

  kf_ull *d_st, *d_bad = reinterpret_cast<kf_ull *>(c->sc.d + PL_SC_BAD);
  STAGE_HIP(c, D.get_zeroed(&d_st, PL_ST_COUNT, st));
  STAGE_HIP(c, hipMemsetAsync(d_bad, 0xff, 8, st));

  // ---- rule 1
  msgpu_map_chain *d_chains;
  uint64_t        *d_off, *d_T, *d_Q;
  uint32_t        *d_ops, *d_run_chain, *d_tc, *d_qc;
  STAGE_HIP(c, D.get(&d_chains, n_chains));
  STAGE_HIP(c, D.get_zeroed(&d_off, n_chains + 1ull, st));
  STAGE_HIP(c, D.get(&d_ops, n_runs));
  STAGE_HIP(c, D.get(&d_run_chain, n_runs));
  STAGE_HIP(c, D.get_zeroed(&d_tc, n_runs + 1ull, st)); // (a zero behind the last run: the scans give n_runs + 1 sums)
  STAGE_HIP(c, D.get_zeroed(&d_qc, n_runs + 1ull, st));
  STAGE_HIP(c, D.get(&d_T, n_runs + 1ull));
  STAGE_HIP(c, D.get(&d_Q, n_runs + 1ull));
  if (n_chains) {
    STAGE_HIP(c, hipMemcpyAsync(d_chains, chains, n_chains * sizeof(msgpu_map_chain), hipMemcpyHostToDevice, st));
    STAGE_HIP(c, hipMemcpyAsync(d_off, off, (n_chains + 1ull) * 8, hipMemcpyHostToDevice, st));
  }
  if (n_runs) STAGE_HIP(c, hipMemcpyAsync(d_ops, ops, n_runs * 4ull, hipMemcpyHostToDevice, st));
  msgpu_map_rank *d_ranks = nullptr;
  uint32_t       *d_vflag = nullptr;
  if (ranks) {
    STAGE_HIP(c, D.get(&d_ranks, n_chains));
    STAGE_HIP(c, D.get(&d_vflag, n_chains));
    if (n_chains) STAGE_HIP(c, hipMemcpyAsync(d_ranks, ranks, n_chains * sizeof(msgpu_map_rank), hipMemcpyHostToDevice, st));
  }
  msgpu_map_mate *d_mates = nullptr;
  if (mates) {
    STAGE_HIP(c, D.get(&d_mates, n_chains));
    STAGE_HIP(c, D.get(&d_vflag, n_chains));
    if (n_chains) STAGE_HIP(c, hipMemcpyAsync(d_mates, mates, n_chains * sizeof(msgpu_map_mate), hipMemcpyHostToDevice, st));
  }
  auto bad_chain = [&]() -> int { // the smallest bad chain, through the scalar block
    const int r2 = c->sc.read(c);
    if (r2 != MSGPU_OK) return r2;
    const uint64_t bad = c->sc.h[PL_SC_BAD];
    if (bad == ~0ull) return MSGPU_OK;
    snprintf(c->err, sizeof(c->err), "chain %llu: %s", static_cast<kf_ull>(bad >> 4), PL_WHAT[bad & 15]);
    return MSGPU_E_ARG;
  };
  STAGE_HIP(c, clock.begin(&S.validate_ms));
  if (n_chains) hipLaunchKernelGGL(k_pl_check_off, dim3(grid256(n_chains)), dim3(256), 0, st, d_off, n_chains, n_runs64, d_bad);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if ((rc = bad_chain()) != MSGPU_OK) return rc;
  STAGE_HIP(c, clock.begin(&S.offsets_ms));
  if (n_runs) hipLaunchKernelGGL(k_pl_runs, dim3(grid256(n_runs)), dim3(256), 0, st, d_off, n_chains, d_ops, n_runs, d_run_chain, d_tc, d_qc, d_bad);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_tc, d_T, n_runs + 1ull));
  STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_qc, d_Q, n_runs + 1ull));
  STAGE_HIP(c, clock.end());
  const PlTables X{d_chains, d_off, d_ops, d_T, d_Q, n_chains, n_runs};
  STAGE_HIP(c, clock.begin(&S.validate_ms));
  if (n_chains) hipLaunchKernelGGL(k_pl_check_chain, dim3(grid256(n_chains)), dim3(256), 0, st, X, R, Q, d_ranks, d_mates, d_bad);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if ((rc = bad_chain()) != MSGPU_OK) return rc; // no kernel below runs on a table that breaks rule 1

  // ---- rule 2
  kf_ull   *d_vkey, *d_rec_depth, *d_rec_sub, *d_rec_del, *d_rec_ins;
  uint32_t *d_vidx, *d_span;
  uint64_t *d_S;
  STAGE_HIP(c, D.get_zeroed(&d_vkey, Q.n, st));
  STAGE_HIP(c, D.get(&d_vidx, Q.n));
  if (Q.n) STAGE_HIP(c, hipMemsetAsync(d_vidx, 0xff, Q.n * 4ull, st));
  STAGE_HIP(c, D.get_zeroed(&d_span, n_chains + 1ull, st));
  STAGE_HIP(c, D.get(&d_S, n_chains + 1ull));
  STAGE_HIP(c, D.get_zeroed(&d_rec_depth, R.n, st));
  STAGE_HIP(c, D.get_zeroed(&d_rec_sub, R.n, st));
  STAGE_HIP(c, D.get_zeroed(&d_rec_del, R.n, st));
  STAGE_HIP(c, D.get_zeroed(&d_rec_ins, R.n, st));
  STAGE_HIP(c, clock.begin(&S.voters_ms));
  if (n_chains) {
    const uint32_t mi = static_cast<uint32_t>(prm.min_identity);
    if (mates) {
      hipLaunchKernelGGL(k_pl_voter_mates, dim3(grid256(n_chains)), dim3(256), 0, st, d_chains, d_mates, n_chains, mi, d_vflag);
    } else if (ranks) {
      hipLaunchKernelGGL(k_pl_voter_ranked, dim3(grid256(n_chains)), dim3(256), 0, st, d_chains, d_ranks, n_chains, mi, min_mapq, d_vflag);
    } else {
      hipLaunchKernelGGL(k_pl_voter_key, dim3(grid256(n_chains)), dim3(256), 0, st, d_chains, n_chains, mi, d_vkey);
      hipLaunchKernelGGL(k_pl_voter_idx, dim3(grid256(n_chains)), dim3(256), 0, st, d_chains, n_chains, mi, d_vkey, d_vidx);
    }
    hipLaunchKernelGGL(k_pl_spans, dim3(grid256(n_chains)), dim3(256), 0, st, d_chains, n_chains, d_vidx, d_vflag, d_span, d_rec_depth, d_st);
  }
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(D, st, d_span, d_S, n_chains, c->sc, PL_SC_TOTAL));
  STAGE_HIP(c, clock.end());
  if ((rc = c->sc.read(c)) != MSGPU_OK) return rc;
  const uint64_t n_cols = c->sc.h[PL_SC_TOTAL];
  if (n_cols >= (1ull << 40)) {
    snprintf(c->err, sizeof(c->err), "the voters have %llu columns; the limit is 2^40 - 1", static_cast<kf_ull>(n_cols));
    return MSGPU_E_ARG;
  }

  // ---- rules 3 and 4: the counters
  uint32_t *d_cnt;
  STAGE_HIP(c, D.get_zeroed(&d_cnt, PL_CLASSES * NB, st));
  STAGE_HIP(c, clock.begin(&S.pileup_ms));
  if (n_cols) hipLaunchKernelGGL(k_pl_pileup, dim3(grid256(n_cols)), dim3(256), 0, st, X, d_S, n_cols, R, Q, d_cnt, d_st);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());

  // ---- rules 4 and 6: the insertion events
  uint32_t *d_flag, *d_E;
  kf_ull   *d_best;
  STAGE_HIP(c, D.get_zeroed(&d_flag, n_runs + 1ull, st));
  STAGE_HIP(c, D.get(&d_E, n_runs + 1ull));
  STAGE_HIP(c, D.get_zeroed(&d_best, NB, st));
  STAGE_HIP(c, clock.begin(&S.insertions_ms));
  if (n_runs) hipLaunchKernelGGL((k_pl_ins<false>), dim3(grid256(n_runs)), dim3(256), 0, st, X, d_run_chain, d_vidx, d_vflag, R, Q, d_flag, nullptr, nullptr, nullptr, d_st);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan_total(D, st, d_flag, d_E, n_runs, c->sc, PL_SC_TOTAL));
  STAGE_HIP(c, clock.end());
  if ((rc = c->sc.read(c)) != MSGPU_OK) return rc;
  const uint32_t n_ev = static_cast<uint32_t>(c->sc.h[PL_SC_TOTAL]); // <= n_runs < 2^31
  uint64_t      *d_key = nullptr, *d_seq = nullptr;
  uint32_t      *d_gstart = nullptr;
  if (n_ev) {
    // two buffers each of keys and letters, the heads, their scan and the groups' starts, and the sorts' temporary buffer
    if ((rc = pl_room(c, n_ev * (4 * 8ull + 3 * 4 + 16) + (8ull << 20), "the insertion events", n_ev, "events", NB, "draft bases")) != MSGPU_OK) return rc;
    uint64_t *d_key2, *d_seq2;
    uint32_t *d_head, *d_G;
    STAGE_HIP(c, D.get(&d_key, n_ev));
    STAGE_HIP(c, D.get(&d_seq, n_ev));
    STAGE_HIP(c, D.get(&d_key2, n_ev));
    STAGE_HIP(c, D.get(&d_seq2, n_ev));
    STAGE_HIP(c, D.get_zeroed(&d_head, n_ev + 1ull, st));
    STAGE_HIP(c, D.get(&d_G, n_ev + 1ull));
    STAGE_HIP(c, D.get(&d_gstart, n_ev + 1ull));
    STAGE_HIP(c, clock.begin(&S.insertions_ms));
    hipLaunchKernelGGL((k_pl_ins<true>), dim3(grid256(n_runs)), dim3(256), 0, st, X, d_run_chain, d_vidx, d_vflag, R, Q, d_flag, d_E, d_key, d_seq, d_st);
    STAGE_HIP(c, hipGetLastError());
    // two stable sorts: by the letters, then by (slot, L), whose 44 bits are the store's 38 and L's 6
    STAGE_HIP(c, stage_sort_pairs(D, st, d_seq, d_seq2, d_key, d_key2, n_ev));
    STAGE_HIP(c, stage_sort_pairs(D, st, d_key2, d_key, d_seq2, d_seq, n_ev, 44));
    hipLaunchKernelGGL(k_pl_heads, dim3(grid256(n_ev)), dim3(256), 0, st, d_key, d_seq, n_ev, d_head);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, stage_scan<const uint32_t *>(D, st, d_head, d_G, n_ev + 1ull));
    hipLaunchKernelGGL(k_stage_seg_starts<uint32_t>, dim3(grid256(n_ev + 1ull)), dim3(256), 0, st, d_head, d_G, n_ev, d_gstart);
    hipLaunchKernelGGL(k_pl_best, dim3(grid256(n_ev)), dim3(256), 0, st, d_gstart, d_G + n_ev, d_key, d_best);
    STAGE_HIP(c, hipGetLastError());
    STAGE_HIP(c, clock.end());
  }

  // ---- rules 5 and 6: the calls
  uint8_t  *d_call;
  uint32_t *d_outlen;
  uint64_t *d_O;
  STAGE_HIP(c, D.get(&d_call, NB));
  STAGE_HIP(c, D.get_zeroed(&d_outlen, NB + 1ull, st));
  STAGE_HIP(c, D.get(&d_O, NB + 1ull));
  STAGE_HIP(c, clock.begin(&S.call_ms));
  const PlCall ca{d_cnt, d_best, d_gstart, d_key, d_call, d_outlen, d_rec_sub, d_rec_del, d_rec_ins, static_cast<uint32_t>(prm.min_depth)};
  if (NB) hipLaunchKernelGGL(k_pl_call, dim3(grid256(NB)), dim3(256), 0, st, R, ca, d_st);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());

  // ---- rule 7
  STAGE_HIP(c, clock.begin(&S.output_ms));
  STAGE_HIP(c, stage_scan_total(D, st, d_outlen, d_O, NB, c->sc, PL_SC_TOTAL));
  STAGE_HIP(c, clock.end());
  if ((rc = c->sc.read(c)) != MSGPU_OK) return rc;
  const uint64_t raw_bytes = c->sc.h[PL_SC_TOTAL];
  uint64_t       text_bound = raw_bytes + raw_bytes / 60 + 2ull * R.n; // the text without its headers
  if ((rc = pl_room(c, raw_bytes + text_bound + R.n * 16ull + (1ull << 20), "the output", raw_bytes, "polished bases", R.n, "records")) != MSGPU_OK) return rc;
  uint8_t  *d_raw;
  uint64_t *d_rec_start, *d_rec_len;
  STAGE_HIP(c, D.get(&d_raw, raw_bytes + 16));
  STAGE_HIP(c, D.get(&d_rec_start, R.n));
  STAGE_HIP(c, D.get(&d_rec_len, R.n));
  STAGE_HIP(c, clock.begin(&S.output_ms));
  if (NB) hipLaunchKernelGGL(k_pl_scatter, dim3(grid256(NB)), dim3(256), 0, st, R, d_call, d_best, d_key, d_seq, d_outlen, d_O, d_raw);
  if (R.n) hipLaunchKernelGGL(k_pl_reclen, dim3(grid256(R.n)), dim3(256), 0, st, R, d_O, d_rec_start, d_rec_len);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if (vcf && (rc = vcf_run(c, D, clock, VcfIn{R, d_cnt, d_best, d_key, d_call, d_O, d_raw, d_st}, res->vcf)) != MSGPU_OK) return rc;

  try {
    for (auto &v : h_rec) v.resize(R.n);
    res->records.resize(R.n);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  const kf_ull *d_rec[6] = {reinterpret_cast<kf_ull *>(d_rec_start), reinterpret_cast<kf_ull *>(d_rec_len), d_rec_sub, d_rec_del, d_rec_ins, d_rec_depth};
  STAGE_HIP(c, clock.begin(&S.copy_ms));
  for (int k = 0; k < 6 && R.n; ++k) STAGE_HIP(c, hipMemcpyAsync(h_rec[k].data(), d_rec[k], R.n * 8ull, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(h_st, d_st, sizeof(h_st), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));

  FastaOut F; // (no pieces: k_pl_scatter wrote the bases; a record without bases keeps its header's '\n', rule 7)
  std::string h;
  try {
    for (uint32_t r = 0; r < R.n; ++r) {
      const uint64_t len_in = msgpu_seq_length(FT.f, r), len_out = h_rec[1][r];
      if (len_out > 0xffffffffull) {
        snprintf(c->err, sizeof(c->err), "draft record %u comes out with %llu bases; the limit is 2^32 - 1", r, static_cast<kf_ull>(len_out));
        return MSGPU_E_ARG;
      }
      res->records[r] = msgpu_pl_record{len_in, len_out, h_rec[2][r], h_rec[3][r], h_rec[4][r], len_in ? h_rec[5][r] * 100 / len_in : 0};
      h.assign(">").append(msgpu_seq_name(FT.f, r)).append("\n");
      F.recs.push_back(msgpu_fasta_record{h_rec[0][r], F.text, static_cast<uint32_t>(len_out), static_cast<uint32_t>(F.hdr.size()), static_cast<uint32_t>(h.size()), 0});
      F.hdr.append(h);
      F.text += msgpu_fasta_text_bytes(static_cast<uint32_t>(h.size()), len_out);
    }
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  if ((rc = F.emit(c, D, clock, d_raw, nullptr, nullptr, &S.format_ms, &S.copy_ms, res->text)) != MSGPU_OK) return rc;
  if (stage_verify(c, D) != MSGPU_OK) return MSGPU_E_HIP;

  S.n_voters        = h_st[PL_ST_VOTERS];
  S.n_ignored       = h_st[PL_ST_IGNORED];
  S.cols_eq         = h_st[PL_ST_EQ];
  S.cols_x          = h_st[PL_ST_X];
  S.cols_d          = h_st[PL_ST_D];
  S.cols_i          = h_st[PL_ST_I];
  S.pos_verbatim    = h_st[PL_ST_VERBATIM];
  S.pos_unchanged   = h_st[PL_ST_UNCHANGED];
  S.pos_substituted = h_st[PL_ST_SUBST];
  S.pos_deleted     = h_st[PL_ST_DELETED];
  S.ins_usable      = h_st[PL_ST_USABLE];
  S.ins_unusable    = h_st[PL_ST_UNUSABLE];
  S.ins_at_ends     = h_st[PL_ST_ENDS];
  S.ins_applied     = h_st[PL_ST_APPLIED];
  S.bases_inserted  = h_st[PL_ST_INSERTED];
  S.max_depth       = h_st[PL_ST_MAXDEPTH];
  S.bytes_out       = F.text;
  S.bytes_peak      = D.peak;
  res->has_vcf      = vcf;
  res->vcf.stats.bytes_peak = vcf ? D.peak : 0;
  return MSGPU_OK;
}

} // namespace

extern "C" {

void msgpu_pl_default_params(msgpu_pl_params *p) {
  if (p) *p = msgpu_pl_params{3, 0};
}

int  msgpu_pl_create(int device, msgpu_plctx **out) { return stage_create(device, out); }
void msgpu_pl_destroy(msgpu_plctx *c) { stage_destroy(c); }

const char *msgpu_pl_last_error(const msgpu_plctx *c) { return c ? c->err : "null context"; }

static int pl_entry(msgpu_plctx *c, const msgpu_pl_params *params, const char *draft_path, const char *reads_path, const msgpu_map_chain *chains,
                    uint64_t n_chains, const uint32_t *ops, const uint64_t *off, const msgpu_map_rank *ranks, uint32_t min_mapq, const msgpu_map_mate *mates,
                    uint32_t flags, msgpu_pl_result **out) {
  if (!c || !out) return MSGPU_E_ARG;
  *out      = nullptr;
  c->err[0] = 0;
  if (!params || !draft_path || !reads_path || (flags & ~MSGPU_PL_VCF) || (n_chains && (!chains || !off)) || (n_chains && off[n_chains] && !ops)) return MSGPU_E_ARG;
  const msgpu_pl_params p = *params;
  if (p.min_depth < 1 || p.min_identity < 0 || p.min_identity > 100) {
    snprintf(c->err, sizeof(c->err), "min_depth = %d (at least 1), min_identity = %d (0..100)", p.min_depth, p.min_identity);
    return MSGPU_E_ARG;
  }
  STAGE_HIP(c, hipSetDevice(c->device));
  std::unique_ptr<msgpu_pl_result> res;
  try {
    res.reset(new msgpu_pl_result());
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  const StageTimer wall;
  const uint64_t   lost0 = c->sc.lost;
  const int        rc = pl_run(c, p, draft_path, reads_path, chains, n_chains, ops, off, ranks, min_mapq, mates, (flags & MSGPU_PL_VCF) != 0, res.get());
  if (rc != MSGPU_OK) return rc;
  res->stats.n_lost_publications = c->sc.lost - lost0;
  res->stats.wall_ms             = wall.ms();
  *out                           = res.release();
  return MSGPU_OK;
}

int msgpu_pl_run(msgpu_plctx *c, const msgpu_pl_params *params, const char *draft_path, const char *reads_path, const msgpu_map_chain *chains,
                 uint64_t n_chains, const uint32_t *ops, const uint64_t *off, uint32_t flags, msgpu_pl_result **out) {
  return pl_entry(c, params, draft_path, reads_path, chains, n_chains, ops, off, nullptr, 0, nullptr, flags, out);
}

int msgpu_pl_run_ranked(msgpu_plctx *c, const msgpu_pl_params *params, const char *draft_path, const char *reads_path,
                        const msgpu_map_chain *chains, uint64_t n_chains, const uint32_t *ops, const uint64_t *off, const msgpu_map_rank *ranks,
                        uint32_t min_mapq, uint32_t flags, msgpu_pl_result **out) {
  static const msgpu_map_rank none{};
  if (c && out && !ranks && n_chains) {
    *out = nullptr;
    snprintf(c->err, sizeof(c->err), "no rank rows for %llu chains", static_cast<unsigned long long>(n_chains));
    return MSGPU_E_ARG;
  }
  return pl_entry(c, params, draft_path, reads_path, chains, n_chains, ops, off, ranks ? ranks : &none, min_mapq, nullptr, flags, out);
}

int msgpu_pl_run_mates(msgpu_plctx *c, const msgpu_pl_params *params, const char *draft_path, const char *reads_path,
                       const msgpu_map_chain *chains, uint64_t n_chains, const uint32_t *ops, const uint64_t *off, const msgpu_map_mate *mates,
                       uint32_t flags, msgpu_pl_result **out) {
  static const msgpu_map_mate none{};
  if (c && out && !mates && n_chains) {
    *out = nullptr;
    snprintf(c->err, sizeof(c->err), "no mate rows for %llu chains", static_cast<unsigned long long>(n_chains));
    return MSGPU_E_ARG;
  }
  return pl_entry(c, params, draft_path, reads_path, chains, n_chains, ops, off, nullptr, 0, mates ? mates : &none, flags, out);
}

int msgpu_pl_result_stats(const msgpu_pl_result *r, msgpu_pl_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->stats;
  return MSGPU_OK;
}

int msgpu_pl_result_records(const msgpu_pl_result *r, const msgpu_pl_record **records, uint64_t *n) {
  if (!r || !records || !n) return MSGPU_E_ARG;
  *records = r->records.data();
  *n       = r->records.size();
  return MSGPU_OK;
}

const char *msgpu_pl_result_text(const msgpu_pl_result *r, uint64_t *len) {
  if (len) *len = r ? r->text.size() : 0;
  return r ? r->text.data() : "";
}

const char *msgpu_pl_result_vcf(const msgpu_pl_result *r, uint64_t *len) {
  const bool has = r && r->has_vcf;
  if (len) *len = has ? r->vcf.text.size() : 0;
  return has ? r->vcf.text.data() : nullptr;
}

int msgpu_pl_result_variants(const msgpu_pl_result *r, const msgpu_pl_variant **rows, uint64_t *n) {
  if (!r || !rows || !n) return MSGPU_E_ARG;
  *rows = r->vcf.rows.data();
  *n    = r->vcf.rows.size();
  return MSGPU_OK;
}

int msgpu_pl_result_vcf_stats(const msgpu_pl_result *r, msgpu_pl_vcf_stats *out) {
  if (!r || !out) return MSGPU_E_ARG;
  *out = r->vcf.stats;
  return MSGPU_OK;
}

void msgpu_pl_result_free(msgpu_pl_result *r) {
  if (r) delete r;
}

} // extern "C"
