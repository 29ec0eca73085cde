// msgpu_kmer_wide.h -- the k-mer key of W 64-bit words, for the k a built-in integer does not hold: W = 3 for k = 65..96,
// W = 4 for k = 97..128 (a key of W words serves 32 (W - 1) < k <= 32 W, so its two top bits, at 2 (k - 1), always lie in its
// top word).  It is what the templates of msgpu_kmer_shared.h and msgpu_unitig.hip ask of a key: construction from a small
// integer, | & ~ == != < >, shifts, the mask of 2k bits, and beside them the pieces those templates reach through an
// overload: the rolling window (KfRoll), the step to a successor / predecessor string, the base at a position, the reverse
// complement and the split into words.  No shift in this file is by 64 or more: a shift across words is a carried shift by
// less than 64, and the all-ones mask at 2k = 64 W never comes from 1 << 2k.  The file needs neither the HIP runtime nor
// rocPRIM, so a host program can include it alone (tests/cpp/test_kmer_wide.cpp does, under the undefined-behaviour sanitizer).
#ifndef MSGPU_KMER_WIDE_H
#define MSGPU_KMER_WIDE_H

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MSGPU_HD __host__ __device__
#else
#define MSGPU_HD
#endif

namespace msgpu {

typedef unsigned __int128 kf_u128;

// the 2-bit groups of a word in reverse order
MSGPU_HD inline uint64_t ug_rev2(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
  x = __brevll(x);
  return ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
#else
  x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
  x = ((x >> 4) & 0x0f0f0f0f0f0f0f0full) | ((x & 0x0f0f0f0f0f0f0f0full) << 4);
  return __builtin_bswap64(x);
#endif
}

template <int W> struct KfWide {
  static_assert(W >= 2 && W <= 4, "a key of two to four words");
  uint64_t w[W]; // w[0] holds the last bases

  KfWide() = default;
  MSGPU_HD KfWide(uint64_t x) {
    w[0] = x;
    for (int i = 1; i < W; ++i) w[i] = 0;
  }
  MSGPU_HD explicit operator uint32_t() const { return static_cast<uint32_t>(w[0]); }

  // by less than 64, carried from word to word
  MSGPU_HD void shl_small(int n) {
    if (!n) return;
    for (int i = W - 1; i > 0; --i) w[i] = (w[i] << n) | (w[i - 1] >> (64 - n));
    w[0] <<= n;
  }
  MSGPU_HD void shr_small(int n) {
    if (!n) return;
    for (int i = 0; i < W - 1; ++i) w[i] = (w[i] >> n) | (w[i + 1] << (64 - n));
    w[W - 1] >>= n;
  }
  // by any n in [0, 64 W): whole words one at a time, then the rest.  The kernels' steps do not come here (push_low,
  // push_high, kf_base and ug_rc below shift by a known 2 or by less than 64).
  MSGPU_HD KfWide operator<<(int n) const {
    KfWide r = *this;
    for (int q = n >> 6; q > 0; --q) {
      for (int i = W - 1; i > 0; --i) r.w[i] = r.w[i - 1];
      r.w[0] = 0;
    }
    r.shl_small(n & 63);
    return r;
  }
  MSGPU_HD KfWide operator>>(int n) const {
    KfWide r = *this;
    for (int q = n >> 6; q > 0; --q) {
      for (int i = 0; i < W - 1; ++i) r.w[i] = r.w[i + 1];
      r.w[W - 1] = 0;
    }
    r.shr_small(n & 63);
    return r;
  }
  MSGPU_HD KfWide operator|(const KfWide &o) const {
    KfWide r;
    for (int i = 0; i < W; ++i) r.w[i] = w[i] | o.w[i];
    return r;
  }
  MSGPU_HD KfWide operator&(const KfWide &o) const {
    KfWide r;
    for (int i = 0; i < W; ++i) r.w[i] = w[i] & o.w[i];
    return r;
  }
  MSGPU_HD KfWide operator~() const {
    KfWide r;
    for (int i = 0; i < W; ++i) r.w[i] = ~w[i];
    return r;
  }
  MSGPU_HD bool operator==(const KfWide &o) const {
    bool e = true;
    for (int i = 0; i < W; ++i) e = e && w[i] == o.w[i];
    return e;
  }
  MSGPU_HD bool operator!=(const KfWide &o) const { return !(*this == o); }
  MSGPU_HD bool operator<(const KfWide &o) const { // from the top word down
    bool less = false, same = true;
    for (int i = W - 1; i >= 0; --i) {
      less = less || (same && w[i] < o.w[i]);
      same = same && w[i] == o.w[i];
    }
    return less;
  }
  MSGPU_HD bool operator>(const KfWide &o) const { return o < *this; }

  // the bits of the 2k-bit mask in the top word (every word below it is whole), and where the first base lies in that word
  MSGPU_HD static uint64_t top_word_mask(int k) {
    const int bits = 2 * k - 64 * (W - 1); // 2..64
    return bits == 64 ? ~0ull : ((1ull << bits) - 1);
  }
  MSGPU_HD static int top_word_shift(int k) { return 2 * (k - 1) - 64 * (W - 1); } // 0..62
  MSGPU_HD static KfWide mask(int k) {
    KfWide r;
    for (int i = 0; i < W - 1; ++i) r.w[i] = ~0ull;
    r.w[W - 1] = top_word_mask(k);
    return r;
  }
  // ((s << 2) | c) & mask and (s >> 2) | (c << top) as carried word shifts by 2
  MSGPU_HD void push_low(uint32_t c, uint64_t top_mask) {
    for (int i = W - 1; i > 0; --i) w[i] = (w[i] << 2) | (w[i - 1] >> 62);
    w[0] = (w[0] << 2) | c;
    w[W - 1] &= top_mask;
  }
  MSGPU_HD void push_high(uint32_t c, int top_shift) {
    for (int i = 0; i < W - 1; ++i) w[i] = (w[i] >> 2) | (w[i + 1] << 62);
    w[W - 1] = (w[W - 1] >> 2) | (static_cast<uint64_t>(c) << top_shift);
  }
};

// the mask of 2k bits of any key type
template <class K> MSGPU_HD inline K kf_mask_of(int k, const K *) {
  return (2 * k == static_cast<int>(sizeof(K) * 8)) ? ~static_cast<K>(0) : ((static_cast<K>(1) << (2 * k)) - 1);
}
template <int W> MSGPU_HD inline KfWide<W> kf_mask_of(int k, const KfWide<W> *) { return KfWide<W>::mask(k); }
template <class K> MSGPU_HD inline K kf_mask(int k) { return kf_mask_of(k, static_cast<const K *>(nullptr)); }

// the base (0..3) whose two bits start at bit 2 pos
template <class K> MSGPU_HD inline uint32_t kf_base(K s, int pos) { return static_cast<uint32_t>(s >> (2 * pos)) & 3u; }
template <int W> MSGPU_HD inline uint32_t kf_base(const KfWide<W> &s, int pos) {
  uint64_t word = 0;
  for (int i = 0; i < W; ++i)
    if (i == (pos >> 5)) word = s.w[i]; // (a select per word: no indexing by a variable)
  return static_cast<uint32_t>(word >> (2 * (pos & 31))) & 3u;
}

// the reverse complement: ug_rev2 per word, the word order reversed, complemented, shifted down by 64 W - 2k (below 64)
template <int W> MSGPU_HD inline KfWide<W> ug_rc(const KfWide<W> &x, int k) {
  KfWide<W> f;
  for (int i = 0; i < W; ++i) f.w[i] = ~ug_rev2(x.w[W - 1 - i]);
  f.shr_small(64 * W - 2 * k);
  return f;
}

// (hi, lo) = the low 128 bits
template <int W> inline void key_split(const KfWide<W> &key, uint64_t &hi, uint64_t &lo) {
  lo = key.w[0];
  hi = key.w[1];
}
// a key as words, least significant first
template <class K> inline void key_words(const K &key, uint64_t *out) {
  out[0] = static_cast<uint64_t>(key);
  if constexpr (sizeof(K) > 8) out[1] = static_cast<uint64_t>(key >> 64);
}
template <int W> inline void key_words(const KfWide<W> &key, uint64_t *out) {
  for (int i = 0; i < W; ++i) out[i] = key.w[i];
}

// the rolling window (msgpu_kmer_shared.h) over a key of W words: fw and rc, one word of mask and a shift
template <class K> struct KfRoll;
template <int W> struct KfRoll<KfWide<W>> {
  KfWide<W> fw = 0, rc = 0;
  uint64_t  top_mask;
  uint32_t  run = 0, k;
  int       top_shift;
  MSGPU_HD explicit KfRoll(int k_)
      : top_mask(KfWide<W>::top_word_mask(k_)), k(static_cast<uint32_t>(k_)), top_shift(KfWide<W>::top_word_shift(k_)) {}
  MSGPU_HD bool step(uint8_t b, KfWide<W> &key) {
    const uint32_t u = b & 0xdfu; // case folded
    if (!(u == 'A' || u == 'C' || u == 'G' || u == 'T')) {
      run = 0;
      return false;
    }
    const uint32_t c = ((u >> 1) & 3u) ^ ((u >> 2) & 1u); // A 0, C 1, G 2, T 3
    fw.push_low(c, top_mask);
    rc.push_high(3u - c, top_shift);
    if (++run < k) return false;
    key = fw < rc ? fw : rc;
    return true;
  }
};

} // namespace msgpu

#endif
