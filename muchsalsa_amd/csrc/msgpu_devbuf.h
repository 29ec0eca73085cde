// msgpu_devbuf.h -- DevBuf, the device memory of the overlap context (msgpu_api.hip): a block that grows and is kept from job
// to job.  A header of its own so that tests/cpp/test_devbuf.hip can test it alone.  No kernels.
#ifndef MSGPU_DEVBUF_H
#define MSGPU_DEVBUF_H

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>

#include "msgpu_stage.h"

namespace msgpu {

struct DevBuf { // device memory that grows and is kept from job to job; gives itself back, moves, does not copy
  void  *p   = nullptr; // the block (behind its front guard, if it has one)
  size_t cap = 0;       // its size in bytes
  // A buffer can be used as a VIEW that starts `off` bytes into the allocation: the job-wide result tables of a
  // resident batched run (msgpu_overlap_batched_ex) -- window k writes behind what the windows before it left, and a
  // reallocation keeps those first `off` bytes.  off = 0 everywhere else.
  size_t off  = 0;
  size_t hint = 0; // expected final size of the allocation (bytes): a reallocation asks for at least this much
  // While a batched job runs its first windows, every (re)allocation on this thread asks for the size the job's LARGEST
  // window will need, not the current one's (msgpu_overlap_batched_ex sets this: windows grow, and a scratch table that
  // grows with them is freed and allocated again -- a device-wide synchronisation -- in every window of a first call)
  static inline thread_local double grow_by = 1.0;
  double own_grow_by = 0.0; // the same for this buffer alone (a job-wide result table while the job's FIRST window fills it)
  // MSGPU_POISON (debugging), asked where an allocation is about to happen, as DevArena::poisoned() asks it: the request is
  // exact (no slack, no hint, no grow_by: cap is what was asked for, every larger request reallocates), the block is filled
  // with DevArena's 0xA5 before ensure() returns and lies between two guards of DevArena::GUARD bytes of 0xC3 inside the same
  // allocation, the back one from the first byte past the request.  check() compares them; a block that is given back is
  // checked first, and what was found is kept in `broken` for the next check().  A block allocated without the variable has
  // no guards and stays as it is until a request outgrows it.  Without the variable none of this exists: the same calls,
  // sizes and addresses as ever.
  bool        guarded = false;  // this block lies between guards (moves with the block)
  const char *name    = "buffer"; // for the texts (stays with the member)
  uint64_t    gen     = 0;        // the allocations made through this member so far
  std::string broken;             // the first guard found overwritten, kept for check()
  DevBuf() = default;
  DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
  DevBuf &operator=(DevBuf &&o) noexcept {
    std::swap(p, o.p);
    std::swap(cap, o.cap);
    std::swap(off, o.off);
    std::swap(hint, o.hint);
    std::swap(own_grow_by, o.own_grow_by);
    std::swap(guarded, o.guarded);
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(base());
  }
  void *base() const { return guarded ? static_cast<uint8_t *>(p) - DevArena::GUARD : p; } // what hipMalloc returned
  // the two guards of a guarded block (behind a synchronisation); the first byte that is not a guard's goes into `broken`
  hipError_t look() {
    if (!p || !guarded) return hipSuccess;
    uint8_t        h[2 * DevArena::GUARD];
    const uint8_t *b = static_cast<const uint8_t *>(p);
    hipError_t     e = hipMemcpy(h, b - DevArena::GUARD, DevArena::GUARD, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h + DevArena::GUARD, b + cap, DevArena::GUARD, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < 2 * DevArena::GUARD && broken.empty(); ++i)
      if (h[i] != DevArena::GUARD_BYTE) {
        char t[224];
        snprintf(t, sizeof(t), "arena guard: buffer %s of %zu bytes: the %s guard was written (0x%02x at byte %zu of its %zu)", name, cap,
                 i < DevArena::GUARD ? "front" : "back", h[i], i % DevArena::GUARD, DevArena::GUARD);
        broken = t;
      }
    return hipSuccess;
  }
  // The guards of the block, behind everything the device has in flight.  Anything but hipSuccess: a guard was written (in
  // this block, or in one that this member gave back), or the check itself failed; `err` says which
  hipError_t check(char *err, size_t err_bytes) {
    hipError_t e = guarded ? hipDeviceSynchronize() : hipSuccess;
    if (e == hipSuccess) e = look();
    if (e != hipSuccess) snprintf(err, err_bytes, "arena guard: buffer %s: %s", name, hipGetErrorString(e));
    else if (!broken.empty()) snprintf(err, err_bytes, "%s", broken.c_str());
    else return hipSuccess;
    return e != hipSuccess ? e : hipErrorIllegalState;
  }
  // the block goes back (its guards are looked at first: the caller has synchronised, or `wait` says to); off, hint and
  // `broken` stay
  hipError_t release(bool wait = true) {
    if (!p) return hipSuccess;
    if (guarded) {
      hipError_t e = wait ? hipDeviceSynchronize() : hipSuccess;
      if (e == hipSuccess) e = look();
      if (e != hipSuccess && broken.empty()) broken = std::string("arena guard: buffer ") + name + ": " + hipGetErrorString(e);
    }
    const hipError_t e = hipFree(base());
    p       = nullptr;
    cap     = 0;
    guarded = false;
    return e;
  }
  hipError_t ensure(size_t bytes) { // room for `bytes` behind `off`
    if (off + bytes <= cap) return hipSuccess;
    const bool   poison = DevArena::poisoned();
    const size_t need   = off + bytes;
    size_t       want   = need + need / 8 + 256; // slack so slowly growing inputs do not reallocate each run
    const double by = own_grow_by > grow_by ? own_grow_by : grow_by;
    if (by > 1.0) want = off + static_cast<size_t>(double(want - off) * by);
    if (hint > want) want = hint;
    if (poison) want = need; // (exact: a request one byte larger meets the guard, not the slack)
    static const bool dbg_alloc = std::getenv("MSGPU_ALLOC_DEBUG") != nullptr;
    if (dbg_alloc) fprintf(stderr, "[alloc] %zu -> %zu bytes (need %zu, kept %zu, hint %zu, grow_by %.2f)\n", cap, want, need, off, hint, grow_by);
    void      *np = nullptr;
    hipError_t e;
    if (p && !off) { // nothing to keep: give the old block back first
      e = release();
      if (e != hipSuccess) return e;
    }
    e = hipMalloc(&np, poison ? want + 2 * DevArena::GUARD : want);
    if (e != hipSuccess) return e;
    if (poison) { // guard, 0xA5, guard; complete when fence() returns (the context's streams do not wait for the null stream)
      e = DevArena::fence(static_cast<uint8_t *>(np), want);
      if (e != hipSuccess) {
        (void)hipFree(np);
        return e;
      }
      np = static_cast<uint8_t *>(np) + DevArena::GUARD;
    }
    if (p) { // a view that outgrew its allocation: everything in flight on the old block first, then its kept part moves
      e = hipDeviceSynchronize();
      if (e == hipSuccess) e = hipMemcpy(np, p, off, hipMemcpyDeviceToDevice);
      if (e == hipSuccess) e = hipDeviceSynchronize();
      if (e != hipSuccess) {
        (void)hipFree(poison ? static_cast<uint8_t *>(np) - DevArena::GUARD : np);
        return e;
      }
      (void)release(false);
    }
    p       = np;
    cap     = want;
    guarded = poison;
    ++gen;
    return hipSuccess;
  }
  template <class T> T *as() const { return reinterpret_cast<T *>(static_cast<char *>(p) + off); }
  void  *at() const { return static_cast<char *>(p) + off; }
  size_t room() const { return cap > off ? cap - off : 0; } // bytes behind `off`
};

} // namespace msgpu

#endif
