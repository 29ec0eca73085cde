// test_arena.hip -- the stages' device arena (csrc/msgpu_stage.h, DevArena) on its own, in the mode its environment asks for:
// with MSGPU_POISON every block reads back as 0xA5 and lies between guards that verify() and drop() check, without it
// nothing of that exists; addresses, offsets inside a reservation, live and peak are the same either way.  The writes that
// the guard checks catch go one byte behind and one byte in front of a block: into the guards, which belong to the
// arena's own allocation.  Exit status 0 and "ok ..." on stdout, or 1 and one line on stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msgpu_stage.h"

using msgpu::DevArena;

#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      fprintf(stderr, "test_arena, line %d: ", __LINE__);                                                              \
      fprintf(stderr, __VA_ARGS__);                                                                                    \
      fprintf(stderr, "\n");                                                                                           \
      return 1;                                                                                                        \
    }                                                                                                                  \
  } while (0)
#define HIP(expr)                                                                                                      \
  do {                                                                                                                 \
    const hipError_t e_ = (expr);                                                                                      \
    CHECK(e_ == hipSuccess, "%s: %s", #expr, hipGetErrorString(e_));                                                   \
  } while (0)

__global__ void k_fill(uint8_t *p, size_t n, uint8_t v) {
  const size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x;
  if (i < n) p[i] = v;
}
__global__ void k_poke(uint8_t *p, long at, uint8_t v) { // one byte at p[at]
  if (blockIdx.x == 0 && threadIdx.x == 0) p[at] = v;
}

static hipStream_t g_st;

// the first of the n bytes at p that is not v, or n
static int first_other(const void *p, size_t n, uint8_t v, size_t *at) {
  std::vector<uint8_t> h(n);
  HIP(hipStreamSynchronize(g_st));
  HIP(hipMemcpy(h.data(), p, n, hipMemcpyDeviceToHost));
  size_t i = 0;
  while (i < n && h[i] == v) ++i;
  *at = i;
  return 0;
}
#define ALL(p, n, v, what)                                                                                             \
  do {                                                                                                                 \
    size_t at_ = 0;                                                                                                    \
    if (first_other((p), (n), (v), &at_)) return 1;                                                                    \
    CHECK(at_ == (n), "%s: byte %zu of %zu is not 0x%02x", (what), at_, static_cast<size_t>(n), (v));                  \
  } while (0)

static int poke(void *p, long at) {
  hipLaunchKernelGGL(k_poke, dim3(1), dim3(64), 0, g_st, static_cast<uint8_t *>(p), at, uint8_t(0x11));
  HIP(hipGetLastError());
  HIP(hipStreamSynchronize(g_st));
  return 0;
}

static const size_t COUNTS[] = {0, 1, 255, 256, 257, 1u << 20};

// blocks from get() and get_zeroed() of every count, of type T, in one arena
template <class T> static int blocks(bool poison) {
  DevArena D;
  size_t   sum = 0;
  for (size_t count : COUNTS) {
    T           *p = nullptr, *z = nullptr;
    const size_t n = (count ? count : 1) * sizeof(T);
    HIP(D.get(&p, count));
    CHECK(p && reinterpret_cast<uintptr_t>(p) % DevArena::ALIGN == 0, "get(%zu) of %zu-byte words: %p is not 256-byte aligned", count, sizeof(T), static_cast<void *>(p));
    if (poison) ALL(p, n, uint8_t(0xA5), "a block of get()");
    HIP(D.get_zeroed(&z, count, g_st));
    CHECK(z && reinterpret_cast<uintptr_t>(z) % DevArena::ALIGN == 0, "get_zeroed(%zu): %p is not 256-byte aligned", count, static_cast<void *>(z));
    if (count) ALL(z, count * sizeof(T), uint8_t(0), "a block of get_zeroed()");
    sum += 2 * n;
    CHECK(D.live == sum && D.peak == sum, "live %zu, peak %zu after blocks of %zu bytes", D.live, D.peak, sum);
    // used inside its bounds, last byte included
    hipLaunchKernelGGL(k_fill, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0, g_st, reinterpret_cast<uint8_t *>(p), n, uint8_t(0x11));
    HIP(hipGetLastError());
    ALL(p, n, uint8_t(0x11), "a block that a kernel filled");
  }
  HIP(D.room(1000)); // rocPRIM's temporary: a block like the others
  CHECK(D.tmp && D.tmp_bytes == 1000 && D.live == sum + 1000, "room(1000): %zu bytes, live %zu", D.tmp_bytes, D.live);
  if (poison) ALL(D.tmp, 1000, uint8_t(0xA5), "the temporary buffer");
  char err[256] = "";
  CHECK(D.verify(g_st, err, sizeof(err)) == hipSuccess && !err[0], "an arena used inside its blocks does not verify: %s", err);
  return 0;
}

// one sequence of calls on a reserved arena and on one that calls hipMalloc: the offsets, live and peak after every step
static int trace(bool poison, std::vector<size_t> &t) {
  if (poison) setenv("MSGPU_POISON", "1", 1);
  else unsetenv("MSGPU_POISON");
  auto step = [&t](const DevArena &A, const void *p) {
    t.push_back(p ? static_cast<size_t>(static_cast<const uint8_t *>(p) - A.pool) : 0);
    t.push_back(A.live);
    t.push_back(A.peak);
    t.push_back(A.tmp_bytes);
    t.push_back(A.pool_used);
  };
  {
    DevArena  A;
    uint8_t  *a, *e;
    uint64_t *b;
    uint32_t *c;
    HIP(A.reserve((1u << 20) + 5));
    CHECK(reinterpret_cast<uintptr_t>(A.pool) % DevArena::ALIGN == 0, "the reservation is not 256-byte aligned");
    t.push_back(A.pool_bytes);
    for (int round = 0; round < 2; ++round) {
      HIP(A.get(&a, 100));
      step(A, a);
      HIP(A.get(&b, 1000));
      step(A, b);
      HIP(A.room(5000));
      step(A, A.tmp);
      HIP(A.get(&c, 77));
      step(A, c);
      HIP(A.room(70000));
      step(A, A.tmp);
      HIP(A.room(100)); // (fits: nothing moves)
      step(A, A.tmp);
      A.drop_tmp();
      step(A, nullptr);
      HIP(A.get(&e, 0));
      step(A, e);
      CHECK(A.get(&e, 2u << 20) == hipErrorOutOfMemory && !e, "a block larger than the reservation was handed out");
      step(A, nullptr);
      HIP(A.rewind());
      step(A, nullptr);
    }
  }
  {
    DevArena  A;
    uint8_t  *a;
    uint64_t *b;
    uint32_t *c;
    HIP(A.get(&a, 100));
    HIP(A.get(&b, 1000));
    step(A, nullptr);
    HIP(A.room(5000));
    step(A, nullptr);
    HIP(A.get(&c, 0));
    A.drop(b);
    step(A, nullptr);
    A.drop_tmp();
    step(A, nullptr);
    HIP(A.room(64));
    step(A, nullptr);
  }
  return 0;
}

// the text of a failed verify(): the block, its size, the side ("front" or "back")
static int names(DevArena &D, const char *block, const char *bytes, const char *side) {
  char              err[384] = "";
  const hipError_t  e = D.verify(g_st, err, sizeof(err));
  const std::string hit = std::string("the ") + side + " guard", other = std::string("the ") + (strcmp(side, "back") ? "back" : "front") + " guard";
  CHECK(e != hipSuccess, "a written %s guard of %s went unnoticed", side, block);
  CHECK(!strncmp(err, "arena guard:", 12) && strstr(err, block) && strstr(err, bytes) && strstr(err, hit.c_str()) && !strstr(err, other.c_str()),
        "the text does not name %s, %s, %s alone: %s", block, bytes, hit.c_str(), err);
  return 0;
}

// (a poke goes into a guard only where the arena says that there is one)
#define FENCED(D, n) CHECK((D).fenced.size() == (n), "%zu blocks between guards, not %d", (D).fenced.size(), int(n))

static int guards() {
  uint8_t  *a;
  uint32_t *b;
  uint64_t *c;
  char      err[384] = "";
  { // one byte behind block 1
    DevArena D;
    HIP(D.get(&a, 100));
    HIP(D.get(&b, 257));
    HIP(D.get(&c, 3));
    FENCED(D, 3u);
    if (poke(b, 257 * 4)) return 1;
    if (names(D, "block 1 ", " 1028 bytes", "back")) return 1;
    CHECK(D.verify(g_st, err, sizeof(err)) != hipSuccess, "a second verify() forgot the guard");
  }
  { // one byte in front of block 2
    DevArena D;
    HIP(D.get(&a, 100));
    HIP(D.get(&b, 257));
    HIP(D.get(&c, 3));
    FENCED(D, 3u);
    if (poke(c, -1)) return 1;
    if (names(D, "block 2 ", " 24 bytes", "front")) return 1;
  }
  { // the block goes before anybody verifies: drop() remembers
    DevArena D;
    HIP(D.get(&a, 100));
    HIP(D.get(&b, 257));
    FENCED(D, 2u);
    if (poke(a, 100)) return 1;
    D.drop(a);
    CHECK(D.live == 1028, "live %zu after the drop", D.live);
    if (names(D, "block 0 ", " 100 bytes", "back")) return 1;
  }
  { // a dropped block that was used inside its bounds, and the temporary buffer: clean
    DevArena D;
    HIP(D.get(&a, 100));
    HIP(D.room(1000));
    if (poke(a, 99) || poke(a, 0) || poke(D.tmp, 999)) return 1;
    D.drop(a);
    D.drop_tmp();
    CHECK(D.verify(g_st, err, sizeof(err)) == hipSuccess, "a clean arena does not verify: %s", err);
  }
  { // a reservation: the guards lie around the whole of it
    DevArena D;
    HIP(D.reserve(4096));
    HIP(D.get(&a, 100));
    HIP(D.room(512));
    if (poke(a, 100)) return 1; // (the padding behind a block of a reservation: not fenced)
    if (poke(D.tmp, 511)) return 1; // the reservation's last byte
    CHECK(D.verify(g_st, err, sizeof(err)) == hipSuccess, "a reservation used inside its bytes does not verify: %s", err);
    CHECK(D.pool_fenced, "a reservation without guards");
    if (poke(D.pool, 4096)) return 1;
    if (names(D, "block 0 (the reservation)", " 4096 bytes", "back")) return 1;
  }
  {
    DevArena D;
    HIP(D.reserve(4096));
    CHECK(D.pool_fenced, "a reservation without guards");
    if (poke(D.pool, -1)) return 1;
    if (names(D, "block 0 (the reservation)", " 4096 bytes", "front")) return 1;
  }
  return 0;
}

// what a kernel left in a reservation is gone after rewind(); the temporary buffer comes poisoned as well
static int rewound(bool poison) {
  DevArena D;
  uint8_t *a, *b;
  HIP(D.reserve(1u << 16));
  if (poison) ALL(D.pool, D.pool_bytes, uint8_t(0xA5), "a fresh reservation");
  HIP(D.get(&a, 1000));
  hipLaunchKernelGGL(k_fill, dim3(4), dim3(256), 0, g_st, a, size_t(1000), uint8_t(0x11));
  HIP(hipGetLastError());
  ALL(a, 1000, uint8_t(0x11), "a block that a kernel filled");
  HIP(D.room(3000));
  hipLaunchKernelGGL(k_fill, dim3(12), dim3(256), 0, g_st, static_cast<uint8_t *>(D.tmp), size_t(3000), uint8_t(0x11));
  HIP(hipGetLastError());
  HIP(hipStreamSynchronize(g_st));
  HIP(D.rewind());
  CHECK(!D.live && !D.peak && !D.tmp && !D.pool_used, "rewind() left something held");
  HIP(D.get(&b, 1000));
  CHECK(b == a, "the first block after rewind() is not the first block of the reservation");
  HIP(D.room(3000));
  if (poison) {
    ALL(b, 1024, uint8_t(0xA5), "the first block after rewind()");
    ALL(D.tmp, 3072, uint8_t(0xA5), "the temporary buffer after rewind()");
  }
  // the temporary buffer grows over bytes that the smaller one held, and a block takes bytes that it gave back
  hipLaunchKernelGGL(k_fill, dim3(12), dim3(256), 0, g_st, static_cast<uint8_t *>(D.tmp), size_t(3072), uint8_t(0x11));
  HIP(hipGetLastError());
  HIP(D.room(6000));
  if (poison) ALL(D.tmp, 6144, uint8_t(0xA5), "a temporary buffer that grew");
  hipLaunchKernelGGL(k_fill, dim3(24), dim3(256), 0, g_st, static_cast<uint8_t *>(D.tmp), size_t(6144), uint8_t(0x11));
  HIP(hipGetLastError());
  HIP(hipStreamSynchronize(g_st));
  D.drop_tmp();
  HIP(D.get(&a, (1u << 16) - 1024));
  if (poison) ALL(a, (1u << 16) - 1024, uint8_t(0xA5), "a block over bytes of an earlier temporary buffer");
  char err[256] = "";
  CHECK(D.verify(g_st, err, sizeof(err)) == hipSuccess, "a reservation used inside its bytes does not verify: %s", err);
  return 0;
}

int main() {
  const bool poison = getenv("MSGPU_POISON") != nullptr;
  HIP(hipSetDevice(0));
  HIP(hipStreamCreateWithFlags(&g_st, hipStreamNonBlocking)); // as the stages' streams are
  if (blocks<uint8_t>(poison) || blocks<uint32_t>(poison) || blocks<uint64_t>(poison)) return 1;
  if (rewound(poison)) return 1;
  std::vector<size_t> with, without;
  if (trace(true, with) || trace(false, without)) return 1;
  if (poison) setenv("MSGPU_POISON", "1", 1); // (the variable is asked per call: back to what the process was given)
  else unsetenv("MSGPU_POISON");
  CHECK(with.size() == without.size(), "%zu figures with the switch, %zu without", with.size(), without.size());
  for (size_t i = 0; i < with.size(); ++i)
    CHECK(with[i] == without[i], "figure %zu (offset, live, peak, tmp_bytes, pool_used per step) is %zu with the switch and %zu without", i, with[i], without[i]);
  if (poison) {
    if (guards()) return 1;
  } else { // no guards, nothing to verify: an arena says so at once
    DevArena D;
    uint8_t *a;
    char     err[64] = "";
    HIP(D.get(&a, 100));
    CHECK(D.fenced.empty() && D.verify(g_st, err, sizeof(err)) == hipSuccess && !err[0], "verify() without the switch: %s", err);
  }
  HIP(hipStreamSynchronize(g_st));
  HIP(hipStreamDestroy(g_st));
  printf("ok %s\n", poison ? "poisoned" : "plain");
  return 0;
}
