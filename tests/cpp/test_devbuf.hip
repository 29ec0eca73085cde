// test_devbuf.hip -- the overlap context's device buffer (csrc/msgpu_devbuf.h, DevBuf) on its own, in the mode its environment
// asks for.  With MSGPU_POISON a block is exactly as large as the request, reads back as 0xA5 and lies between guards that
// check() compares: one byte written at `size` names the back guard, one byte written at -1 the front guard (both lie in the
// guards, which belong to the buffer's own allocation: nothing out of bounds is touched); a view that outgrows its allocation
// keeps its first `off` bytes and gets fresh guards; every larger request reallocates.  Without the variable the sizes are
// need + need/8 + 256, `hint` and `grow_by` as ever, there are no guards, and a larger request inside the slack does not
// allocate.  Exit status 0 and "ok ..." on stdout, or 1 and one line on stderr.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msgpu_devbuf.h"

using msgpu::DevArena;
using msgpu::DevBuf;

#define CHECK(cond, ...)                                                                                               \
  do {                                                                                                                 \
    if (!(cond)) {                                                                                                     \
      fprintf(stderr, "test_devbuf, line %d: ", __LINE__);                                                             \
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

// the first of the n bytes at p that is not v, or n
static int first_other(const void *p, size_t n, uint8_t v, size_t *at) {
  std::vector<uint8_t> h(n);
  HIP(hipDeviceSynchronize());
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

static bool aligned(const void *p) { return reinterpret_cast<uintptr_t>(p) % DevArena::ALIGN == 0; }

// the text of a failed check(): the buffer, its size, the side ("front" or "back")
static int names(DevBuf &b, const char *bytes, const char *side) {
  char              err[384] = "";
  const hipError_t  e = b.check(err, sizeof(err));
  const std::string hit = std::string("the ") + side + " guard", other = std::string("the ") + (strcmp(side, "back") ? "back" : "front") + " guard";
  const std::string who = std::string("buffer ") + b.name + " ";
  CHECK(e != hipSuccess, "a written %s guard of %s went unnoticed", side, b.name);
  CHECK(!strncmp(err, "arena guard:", 12) && strstr(err, who.c_str()) && strstr(err, bytes) && strstr(err, hit.c_str()) && !strstr(err, other.c_str()),
        "the text does not name %s, %s, %s alone: %s", b.name, bytes, hit.c_str(), err);
  return 0;
}

static const size_t SIZES[] = {1, 255, 256, 257, 1000, (1u << 20) + 3};

static int poisoned() {
  char err[384] = "";
  for (size_t n : SIZES) { // a fresh block: exact, aligned, 0xA5, verifies; used up to its last byte it still verifies
    DevBuf b;
    HIP(b.ensure(n));
    CHECK(b.p && aligned(b.p) && b.guarded && b.gen == 1, "ensure(%zu): %p, guarded %d, generation %llu", n, b.p, int(b.guarded), (unsigned long long)b.gen);
    CHECK(b.cap == n && b.room() == n, "ensure(%zu) under the switch: cap %zu", n, b.cap);
    ALL(b.p, n, DevArena::POISON_BYTE, "a fresh block");
    ALL(static_cast<uint8_t *>(b.p) - DevArena::GUARD, DevArena::GUARD, DevArena::GUARD_BYTE, "the front guard");
    ALL(static_cast<uint8_t *>(b.p) + n, DevArena::GUARD, DevArena::GUARD_BYTE, "the back guard");
    HIP(hipMemset(b.p, 0x11, n));
    CHECK(b.check(err, sizeof(err)) == hipSuccess && !err[0], "a block used inside its bounds does not verify: %s", err);
    // the same request again, and a smaller one: the block stands
    const void *was = b.p;
    HIP(b.ensure(n));
    HIP(b.ensure(n / 2));
    CHECK(b.p == was && b.gen == 1 && b.cap == n, "a request that fits reallocated");
    // one byte more: a new block, exact again, poisoned again
    HIP(b.ensure(n + 1));
    CHECK(b.gen == 2 && b.cap == n + 1 && b.guarded && aligned(b.p), "ensure(%zu + 1): generation %llu, cap %zu", n, (unsigned long long)b.gen, b.cap);
    ALL(b.p, n + 1, DevArena::POISON_BYTE, "a block that replaced a smaller one");
    CHECK(b.check(err, sizeof(err)) == hipSuccess, "a fresh block does not verify: %s", err);
  }
  { // hint and grow_by do not count under the switch
    DevBuf b;
    b.hint            = 1u << 20;
    b.own_grow_by     = 4.0;
    DevBuf::grow_by   = 3.0;
    const hipError_t e = b.ensure(1000);
    DevBuf::grow_by   = 1.0;
    HIP(e);
    CHECK(b.cap == 1000, "hint / grow_by under the switch: cap %zu", b.cap);
  }
  { // one byte at `size`: the back guard
    DevBuf b;
    b.name = "back_case";
    HIP(b.ensure(1000));
    HIP(hipMemset(static_cast<uint8_t *>(b.p) + 1000, 0x11, 1));
    if (names(b, " 1000 bytes", "back")) return 1;
    CHECK(b.check(err, sizeof(err)) != hipSuccess, "a second check() forgot the guard");
  }
  { // one byte at -1: the front guard
    DevBuf b;
    b.name = "front_case";
    HIP(b.ensure(257));
    HIP(hipMemset(static_cast<uint8_t *>(b.p) - 1, 0x11, 1));
    if (names(b, " 257 bytes", "front")) return 1;
  }
  { // the block goes before anybody checks: the reallocation remembers, and so does release()
    DevBuf b;
    b.name = "gone_case";
    HIP(b.ensure(100));
    HIP(hipMemset(static_cast<uint8_t *>(b.p) + 100, 0x11, 1));
    HIP(b.ensure(200));
    CHECK(b.cap == 200 && b.gen == 2, "cap %zu after the second request", b.cap);
    if (names(b, " 100 bytes", "back")) return 1;
    DevBuf d;
    d.name = "released_case";
    HIP(d.ensure(64));
    HIP(hipMemset(static_cast<uint8_t *>(d.p) - 1, 0x11, 1));
    HIP(d.release());
    CHECK(!d.p && !d.cap && !d.guarded, "release() left a block");
    if (names(d, " 64 bytes", "front")) return 1;
  }
  { // a view that outgrows its allocation: the kept part moves, the rest is poison, the guards are fresh and at the new end
    DevBuf b;
    b.name = "view_case";
    HIP(b.ensure(500));
    HIP(hipMemset(b.p, 0x22, 500));
    b.off = 500;
    HIP(b.ensure(300));
    CHECK(b.cap == 800 && b.gen == 2 && b.guarded && aligned(b.p) && b.room() == 300, "a view of 300 bytes behind 500: cap %zu, generation %llu", b.cap, (unsigned long long)b.gen);
    CHECK(b.at() == static_cast<char *>(b.p) + 500, "at() is not p + off");
    ALL(b.p, 500, uint8_t(0x22), "the kept part");
    ALL(b.at(), 300, DevArena::POISON_BYTE, "the bytes behind the kept part");
    ALL(static_cast<uint8_t *>(b.p) - DevArena::GUARD, DevArena::GUARD, DevArena::GUARD_BYTE, "the front guard of the moved view");
    ALL(static_cast<uint8_t *>(b.p) + 800, DevArena::GUARD, DevArena::GUARD_BYTE, "the back guard of the moved view");
    CHECK(b.check(err, sizeof(err)) == hipSuccess, "a moved view does not verify: %s", err);
    // a guard of the old block, written before the move, is remembered
    b.off = 800;
    HIP(hipMemset(static_cast<uint8_t *>(b.p) + 800, 0x11, 1));
    HIP(b.ensure(10));
    CHECK(b.cap == 810 && b.gen == 3, "cap %zu after the second move", b.cap);
    if (names(b, " 800 bytes", "back")) return 1;
  }
  { // mixed: a block from a time without the variable has no guards and stays until a request outgrows it
    DevBuf b;
    unsetenv("MSGPU_POISON");
    HIP(b.ensure(1000));
    setenv("MSGPU_POISON", "1", 1);
    const void *was = b.p;
    CHECK(!b.guarded && b.cap == 1000 + 125 + 256, "a plain block: guarded %d, cap %zu", int(b.guarded), b.cap);
    HIP(b.ensure(1100));
    CHECK(b.p == was && !b.guarded && b.gen == 1, "a plain block that holds the request was replaced");
    CHECK(b.check(err, sizeof(err)) == hipSuccess, "a plain block does not verify: %s", err);
    HIP(b.ensure(5000));
    CHECK(b.guarded && b.cap == 5000 && b.gen == 2, "the block that replaced a plain one: guarded %d, cap %zu", int(b.guarded), b.cap);
    // ... and the other way round: a guarded block is given back whole
    unsetenv("MSGPU_POISON");
    HIP(b.ensure(6000));
    setenv("MSGPU_POISON", "1", 1);
    CHECK(!b.guarded && b.cap == 6000 + 750 + 256 && b.gen == 3, "a plain block behind a guarded one: guarded %d, cap %zu", int(b.guarded), b.cap);
  }
  { // moving: the guards go with the block, the name stays with the member
    DevBuf a, b;
    a.name = "a";
    b.name = "b";
    HIP(a.ensure(100));
    std::swap(a, b);
    CHECK(!a.p && !a.guarded && b.p && b.guarded && b.cap == 100 && !strcmp(a.name, "a") && !strcmp(b.name, "b"), "a swap of two buffers");
    CHECK(b.check(err, sizeof(err)) == hipSuccess, "a moved block does not verify: %s", err);
  }
  return 0;
}

static int plain() {
  char err[64] = "";
  for (size_t n : SIZES) {
    DevBuf b;
    HIP(b.ensure(n));
    CHECK(b.p && !b.guarded && b.gen == 1 && b.cap == n + n / 8 + 256, "ensure(%zu): cap %zu, guarded %d", n, b.cap, int(b.guarded));
    CHECK(b.check(err, sizeof(err)) == hipSuccess && !err[0], "check() without the switch: %s", err);
    // a second, larger request inside the slack does not allocate
    const void *was = b.p;
    HIP(b.ensure(n + n / 8 + 256));
    CHECK(b.p == was && b.gen == 1, "a request inside the slack allocated");
    // one beyond it does, by the same formula
    const size_t m = n + n / 8 + 257;
    HIP(b.ensure(m));
    CHECK(b.gen == 2 && b.cap == m + m / 8 + 256, "ensure(%zu): cap %zu", m, b.cap);
  }
  { // hint: at least that much
    DevBuf b;
    b.hint = 100000;
    HIP(b.ensure(1000));
    CHECK(b.cap == 100000, "a request with hint 100000: cap %zu", b.cap);
    b.hint = 10;
    HIP(b.ensure(200000));
    CHECK(b.cap == 200000 + 25000 + 256, "a request beyond its hint: cap %zu", b.cap);
  }
  { // grow_by, the thread's and the buffer's own: the larger of the two, on what lies behind `off`
    DevBuf b;
    DevBuf::grow_by = 3.0;
    hipError_t e    = b.ensure(1000);
    DevBuf::grow_by = 1.0;
    HIP(e);
    CHECK(b.cap == static_cast<size_t>(double(1000 + 125 + 256) * 3.0), "a request with grow_by 3: cap %zu", b.cap);
    DevBuf d;
    d.own_grow_by   = 4.0;
    DevBuf::grow_by = 2.0;
    e               = d.ensure(1000);
    DevBuf::grow_by = 1.0;
    HIP(e);
    CHECK(d.cap == static_cast<size_t>(double(1381) * 4.0), "a request with own_grow_by 4: cap %zu", d.cap);
    // a view: the kept part is not multiplied, and moves
    HIP(hipMemset(d.p, 0x22, 5524));
    d.off         = 5524;
    d.own_grow_by = 2.0;
    HIP(d.ensure(100));
    const size_t need = 5624, want = need + need / 8 + 256;
    CHECK(d.cap == 5524 + static_cast<size_t>(double(want - 5524) * 2.0) && d.gen == 2, "a view with own_grow_by 2: cap %zu", d.cap);
    ALL(d.p, 5524, uint8_t(0x22), "the kept part");
  }
  return 0;
}

int main() {
  const bool poison = getenv("MSGPU_POISON") != nullptr;
  HIP(hipSetDevice(0));
  if (poison ? poisoned() : plain()) return 1;
  HIP(hipDeviceSynchronize());
  printf("ok %s\n", poison ? "poisoned" : "plain");
  return 0;
}
