// msgpu_polish.h -- what the polishing stage (msgpu_polish.hip) and its VCF output (msgpu_vcf.hip) share: the classes of the
// six counters, the words of the call kernel that the VCF kernels read, the context, the memory check of rule 8, and the VCF's
// two entry points, which the polisher's run calls behind k_pl_call and k_pl_scatter while their arrays are resident.
#ifndef MSGPU_POLISH_H
#define MSGPU_POLISH_H

#include <string>
#include <vector>

#include "msgpu_device.h"
#include "msgpu_internal.h"
#include "msgpu_kmer_shared.h"
#include "msgpu_stage.h"

namespace msgpu {

enum { PL_A = 0, PL_C, PL_G, PL_T, PL_DEL, PL_OTHER, PL_CLASSES };
// the counts of msgpu_pl_stats that the kernels add up, one 64-bit word each
enum { PL_ST_VOTERS = 0, PL_ST_IGNORED, PL_ST_EQ, PL_ST_X, PL_ST_D, PL_ST_I, PL_ST_VERBATIM, PL_ST_UNCHANGED, PL_ST_SUBST, PL_ST_DELETED,
       PL_ST_USABLE, PL_ST_UNUSABLE, PL_ST_ENDS, PL_ST_APPLIED, PL_ST_INSERTED, PL_ST_MAXDEPTH, PL_ST_COUNT };
// the scalar block's slots of the stage
enum { PL_SC_BAD = 0, PL_SC_TOTAL, PL_SC_VCF_SHORT, PL_SC_VCF_LONG, PL_SC_VCF_SUBST, PL_SC_VCF_DELETED, PL_SC_VCF_INSERTED };
static_assert(PL_SC_VCF_INSERTED < SC_COUNT, "the scalar block");

// best[pos] behind k_pl_call: 0, or for an applied insertion 1 << 63 | its group's count << 32 | its first event
constexpr kf_ull PL_APPLIED = 1ull << 63;
__device__ inline uint32_t pl_applied_count(kf_ull b) { return static_cast<uint32_t>(b >> 32) & 0x7fffffffu; }

// rule 3: the class of the oriented query's byte; s = 1 reads the complement (upper case only, as MSGPU_COPY_REVCOMP), then folds
__device__ inline uint32_t pl_class(uint8_t b, uint32_t s) {
  if (s) b = b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
  if (b >= 'a' && b <= 'z') b -= 32;
  return b == 'A' ? PL_A : b == 'C' ? PL_C : b == 'G' ? PL_G : b == 'T' ? PL_T : PL_OTHER;
}
__device__ inline uint32_t pl_depth(const uint32_t *cnt, uint64_t plane, uint64_t pos) {
  uint32_t d = 0;
  for (int c = 0; c < PL_CLASSES; ++c) d += cnt[c * plane + pos];
  return d;
}

} // namespace msgpu

struct msgpu_plctx : msgpu::StageCtx {
  msgpu::SeqCtxHold  seq;
  msgpu::ScalarBlock sc;
  int                open() {
    const int rc = msgpu_seq_create(device, &seq.p);
    return rc != MSGPU_OK ? rc : sc.create();
  }
};

namespace msgpu {

// rule 8: `need` more bytes beside what the device holds already
int pl_room(msgpu_plctx *c, uint64_t need, const char *what, uint64_t a, const char *a_name, uint64_t b, const char *b_name);

struct VcfIn { // the polisher's arrays as they stand behind k_pl_call and k_pl_scatter
  SeqRecs         R;
  const uint32_t *cnt;  // six planes of R.n_bases counters
  const kf_ull   *best; // (PL_APPLIED)
  const uint64_t *key;  // the sorted events' (slot << 6 | L); null without events
  const uint8_t  *call; // 0: the draft's byte; 'A' 'C' 'G' 'T': that letter; 1: nothing
  const uint64_t *O;    // R.n_bases + 1: where a position's bytes lie in raw
  const uint8_t  *raw;
  const kf_ull   *st;   // PL_ST_COUNT words
};
struct VcfOut {
  std::string                   text, names; // names: the records' names one behind the other
  std::vector<uint64_t>         name_off;    // n + 1
  std::vector<msgpu_pl_variant> rows;
  msgpu_pl_vcf_stats            stats{};
};

// V7 and V6: the names' check and the header -> out.text; MSGPU_E_ARG naming the record
int vcf_header(msgpu_plctx *c, const msgpu_seqfile *draft, VcfOut &out);
// V1 - V5: the lines behind the header, the rows and the counts; returns behind a synchronisation of the stream
int vcf_run(msgpu_plctx *c, DevArena &D, StageClock &clock, const VcfIn &in, VcfOut &out);

} // namespace msgpu

#endif
