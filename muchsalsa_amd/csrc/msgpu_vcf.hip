// msgpu_vcf.hip -- what the polishing stage changed, as VCF 4.2 text formatted on the device (include/msgpu.h, rules V1 - V9
// behind "pileup consensus").  On request only (MSGPU_PL_VCF); it starts behind k_pl_call and
// k_pl_scatter of msgpu_polish.hip, whatever form rule 2 took, and reads what they left resident: the call and the slot's
// applied insertion per draft base, the six counters, the scan of the output lengths (O) and the polished bases (raw).
//
// The shape of the device work is flag, scan, compact, reduce, count, scan, write.  One pass per base of the store marks the
// positions that head a block and those that end one (V1; a byte of `call`, its two neighbours, and `best` where no edit
// decides); the scan of the heads numbers the blocks, and a second pass over the flag word writes a block's a at its head
// and its b at its end -- the end belongs to the last head at or in front of it.  Nothing else scales with the draft.  A block
// can be one base or a deleted stretch of 100 kb, so no lane walks one alone: a wavefront owns a block of up to VCF_ROW_WAVE
// positions, its lanes stride over it and reduce DP, AO and the two "holds" bits by shuffles; a longer block goes to
// VCF_SLICES workgroups whose partial results lie side by side, without an atomic, for the thread that sizes the line.  ALT0
// needs no gathering: the polisher emits ins(a) call(a) ... call(b - 1) one behind the other at O[a], and ins(b) lies at
// O[b], so ALT0 is |ALT0| consecutive bytes of raw.  A line's exact size is a thread's arithmetic; a 64-bit scan places the
// lines; a line of at most MSGPU_VCF_SHORT_BYTES is written by one wavefront (four lines per workgroup), a longer one by
// VCF_SLICES workgroups, as in the SAM stage: REF in aligned 32-bit stores of four folded bytes, the numbers by a lane each.
#include <hip/hip_runtime.h>
#include <rocprim/iterator/transform_iterator.hpp>

#include <new>
#include <string>
#include <unordered_set>

#include "msgpu_polish.h"

namespace msgpu {

constexpr uint32_t VCF_SLICES = 8;      // workgroups per block, and per line, of the long classes
constexpr uint32_t VCF_ROW_WAVE = 4096; // a block of at most this many positions is reduced by one wavefront
constexpr uint32_t VCF_HEAD = 1, VCF_END = 2, VCF_PURE = 4; // the flag word: heads a block; ends one; the head is an insertion alone
// a row's `type` until k_vcf_sizes writes the TYPE: the block holds a deletion, an insertion; its partial results lie at slot alt_len
constexpr uint32_t VCF_HAS_DEL = 1u << 8, VCF_HAS_INS = 1u << 9, VCF_SLICED = 1u << 10;
enum { VCF_ST_SNP = 0, VCF_ST_MNP, VCF_ST_INS, VCF_ST_DEL, VCF_ST_COMPLEX, VCF_ST_WHOLE, VCF_ST_REF, VCF_ST_ALT, VCF_ST_SLICED, VCF_ST_COUNT };

struct VcfPart { // what the lanes of a unit found in their share of a block
  uint32_t dp, ao, bits;
};
struct VcfTables {
  VcfIn           in;
  const uint8_t  *tn;     // the records' names, one behind the other
  const uint64_t *tn_off; // n + 1
};
struct VcfHeadBit { // the scan's input: the flag word's head bit
  __host__ __device__ uint64_t operator()(uint32_t f) const { return f & VCF_HEAD; }
};

// V1 per byte of the store: does the position head a block, does it end one
__global__ __launch_bounds__(256) void k_vcf_flags(SeqRecs R, const uint8_t *call, const kf_ull *best, uint32_t *flag) {
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (pos >= R.n_bases) return;
  const uint32_t r = seq_record(R, pos);
  uint32_t       f = 0;
  if (r != REC_NONE) { // (a gap of the store belongs to no block)
    const bool e = call[pos] != 0;
    const bool eprev = pos > R.off[r] && call[pos - 1] != 0, enext = pos + 1 < R.off[r] + R.len[r] && call[pos + 1] != 0;
    if (e) f = (eprev ? 0 : VCF_HEAD) | (enext ? 0 : VCF_END);
    else if (!eprev && (best[pos] & PL_APPLIED)) f = VCF_HEAD | VCF_PURE; // (an applied slot is never a record's first position)
  }
  flag[pos] = f;
}

// the blocks' a and b: H = the exclusive scan of the heads, so the block of an end is the heads up to it, less one.  `ref_len`
// holds b until k_vcf_sizes has both
__global__ __launch_bounds__(256) void k_vcf_compact(SeqRecs R, const uint32_t *flag, const uint64_t *H, msgpu_pl_variant *rows) {
  const uint64_t pos = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (pos >= R.n_bases) return;
  const uint32_t f = flag[pos];
  if (!f) return;
  const uint32_t r = seq_record(R, pos), p = static_cast<uint32_t>(pos - R.off[r]);
  const uint64_t k = H[pos]; // (a head: its own number; an end that is no head: one more than its block's)
  if (f & VCF_HEAD) {
    msgpu_pl_variant &v = rows[k];
    v.record = r;
    v.a      = p;
    v.dp = v.ao = 0xffffffffu;
    v.alt_len = v.type = v.anchor = 0;
    v.offset = v.length = 0;
    if (f & VCF_PURE) v.ref_len = p;
  }
  if (f & VCF_END) rows[f & VCF_HEAD ? k : k - 1].ref_len = p + 1;
}

// V4 over the positions a + t, a + t + stride, ... of a block and over its slots likewise
__device__ inline VcfPart vcf_reduce(const VcfIn &in, uint32_t rec, uint32_t a, uint32_t b, uint32_t t, uint32_t stride) {
  const uint64_t base = in.R.off[rec], NB = in.R.n_bases;
  const uint32_t tlen = in.R.len[rec];
  VcfPart        x{0xffffffffu, 0xffffffffu, 0};
  for (uint64_t p = static_cast<uint64_t>(a) + t; p < b; p += stride) {
    const uint8_t  c = in.call[base + p];
    const uint32_t d = pl_depth(in.cnt, NB, base + p), s = in.cnt[(c == 1 ? PL_DEL : pl_class(c, 0)) * NB + base + p];
    x.dp = d < x.dp ? d : x.dp;
    x.ao = s < x.ao ? s : x.ao;
    if (c == 1) x.bits |= VCF_HAS_DEL;
  }
  for (uint64_t p = static_cast<uint64_t>(a) + t; p <= b && p < tlen; p += stride) { // (slot tlen holds no insertion, and no word)
    const kf_ull w = in.best[base + p];
    if (w & PL_APPLIED) {
      const uint32_t s = pl_applied_count(w);
      x.ao = s < x.ao ? s : x.ao;
      x.bits |= VCF_HAS_INS;
    }
  }
  if (a == b && t == 0) { // an insertion alone: 0 < a < tlen
    const uint32_t l = pl_depth(in.cnt, NB, base + a - 1), h = pl_depth(in.cnt, NB, base + a);
    x.dp = l < h ? l : h;
  }
  return x;
}
__device__ inline VcfPart vcf_wave(VcfPart x) { // over the wavefront, in every lane
  for (int o = 32; o; o >>= 1) {
    const uint32_t d = __shfl_xor(x.dp, o), s = __shfl_xor(x.ao, o);
    x.dp = d < x.dp ? d : x.dp;
    x.ao = s < x.ao ? s : x.ao;
    x.bits |= __shfl_xor(x.bits, o);
  }
  return x;
}

// a wavefront per block, four blocks per workgroup; a block beyond VCF_ROW_WAVE is listed for k_vcf_rows_sliced
__global__ __launch_bounds__(256) void k_vcf_rows(VcfIn in, msgpu_pl_variant *rows, uint32_t n_blocks, uint32_t *sliced, uint32_t cap, kf_ull *n_sliced) {
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (k >= n_blocks) return;
  const uint32_t a = rows[k].a, b = rows[k].ref_len;
  if (b - a > VCF_ROW_WAVE) {
    if (t == 0) {
      const kf_ull slot = atomicAdd(n_sliced, 1ull);
      if (slot < cap) { // (blocks do not overlap: at most n_bases / VCF_ROW_WAVE are this long)
        sliced[slot]    = k;
        rows[k].alt_len = static_cast<uint32_t>(slot);
        rows[k].type    = VCF_SLICED;
      }
    }
    return;
  }
  const VcfPart x = vcf_wave(vcf_reduce(in, rows[k].record, a, b, t, 64));
  if (t == 0) {
    rows[k].dp   = x.dp;
    rows[k].ao   = x.ao;
    rows[k].type = x.bits;
  }
}
// VCF_SLICES workgroups per listed block; part[slot * VCF_SLICES + slice] = the workgroup's result, no atomic.  The grid's x
// is the list's bound: a workgroup beyond the count leaves
__global__ __launch_bounds__(256) void k_vcf_rows_sliced(VcfIn in, const msgpu_pl_variant *rows, const uint32_t *sliced, const kf_ull *n_sliced, VcfPart *part) {
  __shared__ VcfPart s[4];
  if (blockIdx.x >= *n_sliced) return;
  const uint32_t k = sliced[blockIdx.x];
  const VcfPart  x = vcf_wave(vcf_reduce(in, rows[k].record, rows[k].a, rows[k].ref_len, blockIdx.y * 256 + threadIdx.x, 256 * VCF_SLICES));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = x;
  __syncthreads();
  if (threadIdx.x == 0) {
    VcfPart y = s[0];
    for (int w = 1; w < 4; ++w) {
      y.dp = s[w].dp < y.dp ? s[w].dp : y.dp;
      y.ao = s[w].ao < y.ao ? s[w].ao : y.ao;
      y.bits |= s[w].bits;
    }
    part[blockIdx.x * VCF_SLICES + blockIdx.y] = y;
  }
}

__device__ inline uint32_t vcf_type_len(uint32_t type) { return type == MSGPU_VCF_COMPLEX ? 7 : 3; }
__device__ inline uint32_t vcf_pos(const msgpu_pl_variant &v) {
  return v.anchor == MSGPU_VCF_ANCHOR_NONE ? v.a + 1 : v.anchor == MSGPU_VCF_ANCHOR_LEFT ? v.a : 1;
}
// V5: the line's bytes
__device__ inline uint64_t vcf_size(const VcfTables &X, const msgpu_pl_variant &v) {
  const uint32_t whole = v.anchor == MSGPU_VCF_ANCHOR_WHOLE, anchored = v.anchor == MSGPU_VCF_ANCHOR_LEFT || v.anchor == MSGPU_VCF_ANCHOR_RIGHT;
  const uint64_t ref = whole ? 1 : static_cast<uint64_t>(v.ref_len) + anchored, alt = whole ? 5 : static_cast<uint64_t>(v.alt_len) + anchored;
  return (X.tn_off[v.record + 1] - X.tn_off[v.record]) + 1 + dec_dig(vcf_pos(v)) + 3 + ref + 1 + alt + 8 +
         (whole ? 4 + dec_dig(X.in.R.len[v.record]) + 1 : 0) + 3 + dec_dig(v.dp) + 1 + 3 + dec_dig(v.ao) + 1 + 5 + vcf_type_len(v.type) + 1;
}

// V2 - V4 per block: |REF0|, |ALT0|, TYPE, the anchoring, the line's size and class, the counts
__global__ __launch_bounds__(256) void k_vcf_sizes(VcfTables X, msgpu_pl_variant *rows, uint32_t n_blocks, const VcfPart *part, uint64_t *size,
                                                   uint32_t *list_short, uint32_t *list_long, kf_ull *cur_short, kf_ull *cur_long, kf_ull *vst) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  const bool     live = k < n_blocks;
  bool           is_short = false, is_long = false;
  uint32_t       type = 0xffffffffu, ref_len = 0, alt_len = 0, whole = 0;
  if (live) {
    msgpu_pl_variant v = rows[k];
    const VcfIn     &in = X.in;
    const uint32_t   a = v.a, b = v.ref_len, tlen = in.R.len[v.record];
    const uint64_t   base = in.R.off[v.record];
    uint32_t         bits = v.type;
    if (bits & VCF_SLICED) {
      bits = 0;
      for (uint32_t s = 0; s < VCF_SLICES; ++s) {
        const VcfPart y = part[v.alt_len * VCF_SLICES + s];
        v.dp = y.dp < v.dp ? y.dp : v.dp;
        v.ao = y.ao < v.ao ? y.ao : v.ao;
        bits |= y.bits;
      }
    }
    uint32_t trailing = 0; // ins(b)
    if (b < tlen) {
      const kf_ull w = in.best[base + b];
      if (w & PL_APPLIED) trailing = static_cast<uint32_t>(in.key[static_cast<uint32_t>(w)] & 63);
    }
    ref_len = b - a;
    alt_len = static_cast<uint32_t>(in.O[base + b] - in.O[base + a]) + trailing;
    type    = !ref_len ? MSGPU_VCF_INS : !alt_len ? MSGPU_VCF_DEL : ref_len == alt_len && !(bits & (VCF_HAS_DEL | VCF_HAS_INS)) ? (ref_len == 1 ? MSGPU_VCF_SNP : MSGPU_VCF_MNP) : MSGPU_VCF_COMPLEX;
    v.anchor  = ref_len && alt_len ? MSGPU_VCF_ANCHOR_NONE : a > 0 ? MSGPU_VCF_ANCHOR_LEFT : b < tlen ? MSGPU_VCF_ANCHOR_RIGHT : MSGPU_VCF_ANCHOR_WHOLE;
    v.ref_len = ref_len;
    v.alt_len = alt_len;
    v.type    = type;
    v.length  = vcf_size(X, v);
    rows[k]   = v;
    size[k]   = v.length;
    whole     = v.anchor == MSGPU_VCF_ANCHOR_WHOLE;
    is_short  = v.length <= MSGPU_VCF_SHORT_BYTES;
    is_long   = !is_short;
  }
  const uint64_t s = wave_append(is_short, cur_short), l = wave_append(is_long, cur_long);
  if (is_short) list_short[s] = k; // (at most n_blocks takers in all: the slot lies inside the list)
  if (is_long) list_long[l] = k;
  wave_count(type == MSGPU_VCF_SNP, vst + VCF_ST_SNP);
  wave_count(type == MSGPU_VCF_MNP, vst + VCF_ST_MNP);
  wave_count(type == MSGPU_VCF_INS, vst + VCF_ST_INS);
  wave_count(type == MSGPU_VCF_DEL, vst + VCF_ST_DEL);
  wave_count(type == MSGPU_VCF_COMPLEX, vst + VCF_ST_COMPLEX);
  wave_count(whole != 0, vst + VCF_ST_WHOLE);
  wave_add(ref_len, vst + VCF_ST_REF);
  wave_add(alt_len, vst + VCF_ST_ALT);
}

// n bytes at p, byte j = at(j), by the lanes t, t + stride, ...: single bytes up to the first aligned word, words of four
// bytes (consecutive lanes write consecutive words), single bytes behind the last
template <class At> __device__ inline void vcf_put(uint8_t *p, uint64_t n, At at, uint32_t t, uint32_t stride) {
  uint64_t head = (4 - (reinterpret_cast<uintptr_t>(p) & 3)) & 3;
  head = head < n ? head : n;
  const uint64_t words = (n - head) >> 2, tail = head + 4 * words;
  if (t < head) p[t] = at(t);
  for (uint64_t x = t; x < words; x += stride) {
    const uint64_t j = head + 4 * x;
    *reinterpret_cast<uint32_t *>(p + j) = at(j) | at(j + 1) << 8 | at(j + 2) << 16 | static_cast<uint32_t>(at(j + 3)) << 24;
  }
  if (tail + t < n && t < 3) p[tail + t] = at(tail + t);
}

// the write pass of one line by the lanes t, t + stride, ... of its group (at least 16 of them: the small pieces are a lane's each)
__device__ inline void vcf_write_line(const VcfTables &X, const msgpu_pl_variant &v, uint8_t *p, uint32_t t, uint32_t stride) {
  const VcfIn   &in = X.in;
  const uint64_t base = in.R.off[v.record];
  const uint8_t *draft = in.R.bases + base, *alt0 = in.raw + in.O[base + v.a];
  const uint32_t b = v.a + v.ref_len;
  uint64_t       w = 0;
  uint32_t       k = 0; // the small pieces are numbered: piece k is lane k's
  auto text = [&](const char *s, uint32_t n) {
    if (t == k)
      for (uint32_t j = 0; j < n; ++j) p[w + j] = static_cast<uint8_t>(s[j]);
    ++k;
    w += n;
  };
  auto tagged = [&](const char *s, uint32_t n, uint32_t value, char end) { // s, the number, end
    const uint32_t d = dec_dig(value);
    if (t == k) {
      for (uint32_t j = 0; j < n; ++j) p[w + j] = static_cast<uint8_t>(s[j]);
      dec_put(p + w + n, value, d);
      p[w + n + d] = static_cast<uint8_t>(end);
    }
    ++k;
    w += n + d + 1;
  };
  auto one = [&](uint8_t c) {
    if (t == k) p[w] = c;
    ++k;
    ++w;
  };
  const uint64_t nl = X.tn_off[v.record + 1] - X.tn_off[v.record];
  const uint8_t *name = X.tn + X.tn_off[v.record];
  for (uint64_t j = t; j < nl; j += stride) p[j] = name[j];
  w = nl;
  tagged("\t", 1, vcf_pos(v), '\t');
  text(".\t", 2);
  if (v.anchor == MSGPU_VCF_ANCHOR_WHOLE) { // V3
    one(text_base(draft[0], 0));
    text("\t<DEL>", 6);
  } else {
    const uint32_t left = v.anchor == MSGPU_VCF_ANCHOR_LEFT, right = v.anchor == MSGPU_VCF_ANCHOR_RIGHT;
    const uint8_t *ref = draft + v.a - left; // REF is one stretch of the draft, the anchor included
    const uint64_t rn = static_cast<uint64_t>(v.ref_len) + left + right;
    vcf_put(p + w, rn, [&](uint64_t j) { return text_base(ref[j], 0); }, t, stride);
    w += rn;
    one('\t');
    if (left) one(text_base(draft[v.a - 1], 0));
    vcf_put(p + w, v.alt_len, [&](uint64_t j) { return alt0[j]; }, t, stride);
    w += v.alt_len;
    if (right) one(text_base(draft[b], 0));
  }
  text("\t.\tPASS\t", 8);
  if (v.anchor == MSGPU_VCF_ANCHOR_WHOLE) tagged("END=", 4, in.R.len[v.record], ';');
  tagged("DP=", 3, v.dp, ';');
  tagged("AO=", 3, v.ao, ';');
  text("TYPE=", 5);
  const char *const names[] = {"snp\n", "mnp\n", "ins\n", "del\n", "complex\n"};
  text(names[v.type], vcf_type_len(v.type) + 1);
}

// the short class: a wavefront per line, four lines per workgroup
__global__ __launch_bounds__(256) void k_vcf_write_short(VcfTables X, const uint32_t *list, uint32_t n_list, msgpu_pl_variant *rows, const uint64_t *L,
                                                         uint64_t file_base, uint8_t *text) {
  const uint32_t li = blockIdx.x * 4 + (threadIdx.x >> 6), t = threadIdx.x & 63;
  if (li >= n_list) return;
  const uint32_t k = list[li];
  if (t == 0) rows[k].offset = file_base + L[k];
  vcf_write_line(X, rows[k], text + L[k], t, 64);
}
// the long class: VCF_SLICES workgroups per line
__global__ __launch_bounds__(256) void k_vcf_write_long(VcfTables X, const uint32_t *list, msgpu_pl_variant *rows, const uint64_t *L, uint64_t file_base,
                                                        uint8_t *text) {
  const uint32_t k = list[blockIdx.x], t = blockIdx.y * 256 + threadIdx.x;
  msgpu_pl_variant v = rows[k]; // (before the offset is written: every lane reads the same row)
  if (t == 0) rows[k].offset = file_base + L[k];
  v.offset = 0;
  vcf_write_line(X, v, text + L[k], t, 256 * VCF_SLICES);
}

// ---- host side -----------------------------------------------------------------------------------------------------

int vcf_header(msgpu_plctx *c, const msgpu_seqfile *draft, VcfOut &out) {
  const uint32_t n = msgpu_seq_count(draft);
  try {
    std::unordered_set<std::string> seen;
    std::string                     contigs;
    out.names.clear();
    out.name_off.assign(n + 1ull, 0);
    for (uint32_t r = 0; r < n; ++r) { // V7
      const std::string name = msgpu_seq_name(draft, r);
      const char       *why = nullptr;
      if (name.empty()) why = "an empty name";
      else if (name.size() > 254) why = "a name longer than 254 bytes";
      else if (name[0] == '*' || name[0] == '=') why = "a name that begins with * or =";
      for (size_t j = 0; j < name.size() && !why; ++j) {
        const unsigned char b = static_cast<unsigned char>(name[j]);
        if (b < 0x21 || b > 0x7e || b == ',' || b == '<' || b == '>') why = "a name with a byte outside 0x21..0x7e or one of , < >";
      }
      if (!why && !seen.insert(name).second) why = "its name is that of an earlier record";
      if (why) {
        snprintf(c->err, sizeof(c->err), "VCF: draft record %u: %s", r, why);
        return MSGPU_E_ARG;
      }
      out.names += name;
      out.name_off[r + 1] = out.names.size();
      contigs.append("##contig=<ID=").append(name).append(",length=").append(std::to_string(msgpu_seq_length(draft, r))).append(">\n");
    }
    out.text = "##fileformat=VCFv4.2\n##source=muchsalsa_amd.polish\n" + contigs +
               "##INFO=<ID=DP,Number=1,Type=Integer,Description=\"Least depth over the block's positions\">\n"
               "##INFO=<ID=AO,Number=1,Type=Integer,Description=\"Least support among the block's edits\">\n"
               "##INFO=<ID=TYPE,Number=1,Type=String,Description=\"snp, mnp, ins, del or complex\">\n"
               "##INFO=<ID=END,Number=1,Type=Integer,Description=\"Last position of a deleted record\">\n"
               "##ALT=<ID=DEL,Description=\"Deletion of the whole record\">\n"
               "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n";
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  out.stats.header_bytes = out.text.size();
  return MSGPU_OK;
}

int vcf_run(msgpu_plctx *c, DevArena &D, StageClock &clock, const VcfIn &in, VcfOut &out) {
  hipStream_t         st = c->stream;
  const SeqRecs      &R = in.R;
  const uint64_t      NB = R.n_bases;
  msgpu_pl_vcf_stats &S = out.stats;
  int                 rc;
  S.text_bytes = S.header_bytes;

  // ---- V1: per base the flag word and its scan
  if ((rc = pl_room(c, (NB + 1) * 12 + (2ull << 20), "the VCF's flags", NB, "draft bases", R.n, "records")) != MSGPU_OK) return rc;
  uint32_t *d_flag;
  uint64_t *d_H;
  STAGE_HIP(c, D.get(&d_flag, NB + 1));
  STAGE_HIP(c, D.get(&d_H, NB + 1));
  STAGE_HIP(c, hipMemsetAsync(d_flag + NB, 0, 4, st)); // (a zero behind the flags: the scan's last sum is the blocks)
  STAGE_HIP(c, clock.begin(&S.vcf_ms));
  if (NB) hipLaunchKernelGGL(k_vcf_flags, dim3(grid256(NB)), dim3(256), 0, st, R, in.call, in.best, d_flag);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan(D, st, rocprim::make_transform_iterator(static_cast<const uint32_t *>(d_flag), VcfHeadBit{}), d_H, NB + 1));
  hipLaunchKernelGGL(k_stage_put<uint64_t>, dim3(1), dim3(64), 0, st, c->sc.d, PL_SC_TOTAL, d_H + NB);
  hipLaunchKernelGGL(k_stage_put<kf_ull>, dim3(1), dim3(64), 0, st, c->sc.d, PL_SC_VCF_SUBST, in.st + PL_ST_SUBST);
  hipLaunchKernelGGL(k_stage_put<kf_ull>, dim3(1), dim3(64), 0, st, c->sc.d, PL_SC_VCF_DELETED, in.st + PL_ST_DELETED);
  hipLaunchKernelGGL(k_stage_put<kf_ull>, dim3(1), dim3(64), 0, st, c->sc.d, PL_SC_VCF_INSERTED, in.st + PL_ST_INSERTED);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if ((rc = c->sc.read(c)) != MSGPU_OK) return rc;
  const uint64_t n_blocks64 = c->sc.h[PL_SC_TOTAL];
  const uint64_t edits_ref = c->sc.h[PL_SC_VCF_SUBST] + c->sc.h[PL_SC_VCF_DELETED], edits_alt = c->sc.h[PL_SC_VCF_SUBST] + c->sc.h[PL_SC_VCF_INSERTED];
  if (n_blocks64 >= (1ull << 31)) {
    snprintf(c->err, sizeof(c->err), "VCF: %llu blocks; the limit is 2^31 - 1", static_cast<kf_ull>(n_blocks64));
    return MSGPU_E_ARG;
  }
  const uint32_t n_blocks = static_cast<uint32_t>(n_blocks64);
  if (!n_blocks) { // V6: the header alone
    STAGE_HIP(c, hipStreamSynchronize(st));
    return MSGPU_OK;
  }

  // ---- the rows: a and b, then DP, AO and the bits
  const uint32_t cap = static_cast<uint32_t>(std::min<uint64_t>(n_blocks, NB / VCF_ROW_WAVE + 1));
  size_t         longest = 0;
  for (uint32_t r = 0; r < R.n; ++r) longest = std::max<size_t>(longest, out.name_off[r + 1] - out.name_off[r]);
  if ((rc = pl_room(c, n_blocks * (sizeof(msgpu_pl_variant) + 8ull + 8 + 4 + 4) + cap * (4ull + VCF_SLICES * sizeof(VcfPart)) + out.names.size() + R.n * 8ull + (2ull << 20),
                    "the VCF's blocks", n_blocks, "blocks", NB, "draft bases")) != MSGPU_OK)
    return rc;
  msgpu_pl_variant *d_rows;
  uint64_t         *d_size, *d_L, *d_tn_off;
  uint32_t         *d_short, *d_long, *d_sliced;
  VcfPart          *d_part;
  kf_ull           *d_vst;
  uint8_t          *d_tn;
  STAGE_HIP(c, D.get(&d_rows, n_blocks));
  STAGE_HIP(c, D.get_zeroed(&d_size, n_blocks + 1ull, st));
  STAGE_HIP(c, D.get(&d_L, n_blocks + 1ull));
  STAGE_HIP(c, D.get(&d_short, n_blocks));
  STAGE_HIP(c, D.get(&d_long, n_blocks));
  STAGE_HIP(c, D.get(&d_sliced, cap));
  STAGE_HIP(c, D.get(&d_part, static_cast<size_t>(cap) * VCF_SLICES));
  STAGE_HIP(c, D.get_zeroed(&d_vst, VCF_ST_COUNT, st));
  STAGE_HIP(c, D.get(&d_tn, out.names.size()));
  STAGE_HIP(c, D.get(&d_tn_off, R.n + 1ull));
  if (!out.names.empty()) STAGE_HIP(c, hipMemcpyAsync(d_tn, out.names.data(), out.names.size(), hipMemcpyHostToDevice, st));
  STAGE_HIP(c, hipMemcpyAsync(d_tn_off, out.name_off.data(), (R.n + 1ull) * 8, hipMemcpyHostToDevice, st));
  kf_ull *d_cur_short = reinterpret_cast<kf_ull *>(c->sc.d + PL_SC_VCF_SHORT), *d_cur_long = reinterpret_cast<kf_ull *>(c->sc.d + PL_SC_VCF_LONG);
  STAGE_HIP(c, hipMemsetAsync(d_cur_short, 0, 16, st)); // (both cursors: neighbours in the scalar block)
  const VcfTables X{in, d_tn, d_tn_off};
  STAGE_HIP(c, clock.begin(&S.vcf_ms));
  hipLaunchKernelGGL(k_vcf_compact, dim3(grid256(NB)), dim3(256), 0, st, R, d_flag, d_H, d_rows);
  hipLaunchKernelGGL(k_vcf_rows, dim3(grid_of(n_blocks, 4)), dim3(256), 0, st, in, d_rows, n_blocks, d_sliced, cap, d_vst + VCF_ST_SLICED);
  hipLaunchKernelGGL(k_vcf_rows_sliced, dim3(cap, VCF_SLICES), dim3(256), 0, st, in, d_rows, d_sliced, d_vst + VCF_ST_SLICED, d_part);
  hipLaunchKernelGGL(k_vcf_sizes, dim3(grid256(n_blocks)), dim3(256), 0, st, X, d_rows, n_blocks, d_part, d_size, d_short, d_long, d_cur_short, d_cur_long, d_vst);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, stage_scan<const uint64_t *>(D, st, d_size, d_L, n_blocks + 1ull));
  hipLaunchKernelGGL(k_stage_put<uint64_t>, dim3(1), dim3(64), 0, st, c->sc.d, PL_SC_TOTAL, d_L + n_blocks);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, clock.end());
  if ((rc = c->sc.read(c)) != MSGPU_OK) return rc;
  const uint64_t bytes = c->sc.h[PL_SC_TOTAL], n_short = c->sc.h[PL_SC_VCF_SHORT], n_long = c->sc.h[PL_SC_VCF_LONG];
  // every line is its name, at most MSGPU_VCF_LINE_FIXED bytes and its alleles, and the alleles are the stage's own edits
  const uint64_t bound = n_blocks * (MSGPU_VCF_LINE_FIXED + static_cast<uint64_t>(longest)) + edits_ref + edits_alt;
  if (bytes > bound || n_short + n_long != n_blocks) {
    snprintf(c->err, sizeof(c->err), "VCF: %llu bytes of text against a bound of %llu, %llu + %llu lines by class of %u", static_cast<kf_ull>(bytes),
             static_cast<kf_ull>(bound), static_cast<kf_ull>(n_short), static_cast<kf_ull>(n_long), n_blocks);
    return MSGPU_E_STATE;
  }

  // ---- the text
  if ((rc = pl_room(c, bytes + (1ull << 20), "the VCF's text", bytes, "bytes of text", n_blocks, "blocks")) != MSGPU_OK) return rc;
  uint8_t *d_text;
  kf_ull   h_vst[VCF_ST_COUNT];
  STAGE_HIP(c, D.get(&d_text, bytes + 16));
  const uint64_t file_base = out.text.size();
  try {
    out.text.resize(file_base + bytes);
    out.rows.resize(n_blocks);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  STAGE_HIP(c, clock.begin(&S.vcf_ms));
  if (n_short)
    hipLaunchKernelGGL(k_vcf_write_short, dim3(grid_of(n_short, 4)), dim3(256), 0, st, X, d_short, static_cast<uint32_t>(n_short), d_rows, d_L, file_base, d_text);
  for (uint64_t at = 0; at < n_long; at += 32768) // (the grid's x)
    hipLaunchKernelGGL(k_vcf_write_long, dim3(static_cast<uint32_t>(std::min<uint64_t>(32768, n_long - at)), VCF_SLICES), dim3(256), 0, st, X, d_long + at,
                       d_rows, d_L, file_base, d_text);
  STAGE_HIP(c, hipGetLastError());
  STAGE_HIP(c, hipMemcpyAsync(&out.text[file_base], d_text, bytes, hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(out.rows.data(), d_rows, n_blocks * sizeof(msgpu_pl_variant), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, hipMemcpyAsync(h_vst, d_vst, sizeof(h_vst), hipMemcpyDeviceToHost, st));
  STAGE_HIP(c, clock.end());
  STAGE_HIP(c, hipStreamSynchronize(st));
  S.n_variants      = n_blocks;
  S.n_snp           = h_vst[VCF_ST_SNP];
  S.n_mnp           = h_vst[VCF_ST_MNP];
  S.n_ins           = h_vst[VCF_ST_INS];
  S.n_del           = h_vst[VCF_ST_DEL];
  S.n_complex       = h_vst[VCF_ST_COMPLEX];
  S.n_whole_deleted = h_vst[VCF_ST_WHOLE];
  S.n_short         = n_short;
  S.n_long          = n_long;
  S.ref_bases       = h_vst[VCF_ST_REF];
  S.alt_bases       = h_vst[VCF_ST_ALT];
  S.text_bytes      = out.text.size();
  return MSGPU_OK;
}

} // namespace msgpu
