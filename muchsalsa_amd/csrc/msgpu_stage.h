// msgpu_stage.h -- the host-side scaffolding of the six contexts, defined once: the overlap context (msgpu_api.hip) and the
// pipeline stages (msgpu_filter.hip, msgpu_scrub.hip, msgpu_kmer.hip, msgpu_unitig.hip, msgpu_map.hip).  The context with
// its create / destroy, the HIP-error macro, the holders of an event and of a stream, the device arena with its temporary
// buffer for rocPRIM, the event clock, the wall-clock timer, the scalar block and its read-back, the record lookup of
// the stages that name sequences, and the loader of the stages that read a store's bases.  msgpu_seq.hip takes the holders.
// And the host-side idioms of the stage files, one copy of each: the arena block that comes zeroed (DevArena::get_zeroed), the
// scan whose total goes into the scalar block (stage_scan_total), a 64- or 128-bit key as two words (key_split), and the
// records of a FASTA text with their way through gather, format and copy (FastaOut).  No kernels.
#ifndef MSGPU_STAGE_H
#define MSGPU_STAGE_H

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "msgpu.h"
#include "msgpu_device.h"
#include "msgpu_internal.h"

namespace msgpu {

// ---- errors: anything with an `err` array takes a failed HIP call's text

template <class C> int stage_fail(C *c, int code, const char *what, hipError_t e) {
  snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
  return code;
}
#define STAGE_HIP(c, expr)                                                                                             \
  do {                                                                                                                 \
    hipError_t _e = (expr);                                                                                            \
    if (_e != hipSuccess) return msgpu::stage_fail((c), _e == hipErrorOutOfMemory ? MSGPU_E_NOMEM : MSGPU_E_HIP, #expr, _e); \
  } while (0)

// ---- the context

struct StageCtx { // what every stage context is made of
  int         device = 0;
  hipStream_t stream = nullptr;
  char        err[384] = {0};
  uint64_t    err_line = 0;
  int         err_file = 0;
  // What a context owns beyond its stream: a context that does shadows open() (called by stage_create on the context's
  // device, behind the stream) and holds it in members whose destructors release it (run by stage_destroy on that device).
  int open() { return MSGPU_OK; }
};

template <class Ctx> void stage_destroy(Ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamDestroy(c->stream);
  }
  delete c;
}

template <class Ctx> int stage_create(int device, Ctx **out) {
  if (!out) return MSGPU_E_ARG;
  *out     = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return MSGPU_E_NODEVICE;
  if (device < 0 || device >= ndev) return MSGPU_E_ARG;
  auto *c = new (std::nothrow) Ctx();
  if (!c) return MSGPU_E_NOMEM;
  c->device = device;
  int rc    = MSGPU_OK;
  if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess)
    rc = MSGPU_E_HIP;
  if (rc == MSGPU_OK) rc = c->open();
  if (rc != MSGPU_OK) {
    stage_destroy(c);
    return rc;
  }
  *out = c;
  return MSGPU_OK;
}

// ---- handles that give themselves back: movable, not copyable, and usable wherever the raw handle is

struct EventHold {
  hipEvent_t e = nullptr;
  EventHold() = default;
  EventHold(EventHold &&o) noexcept : e(o.e) { o.e = nullptr; }
  EventHold &operator=(EventHold &&o) noexcept {
    std::swap(e, o.e);
    return *this;
  }
  ~EventHold() { reset(); }
  hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(&e, flags); }
  void       reset() { // (an event that was never created: nothing)
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  operator hipEvent_t() const { return e; }
};

struct StreamHold { // waits for what the stream holds before it destroys it
  hipStream_t s = nullptr;
  StreamHold() = default;
  StreamHold(StreamHold &&o) noexcept : s(o.s) { o.s = nullptr; }
  StreamHold &operator=(StreamHold &&o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~StreamHold() { reset(); }
  hipError_t create(unsigned flags = hipStreamNonBlocking) { return hipStreamCreateWithFlags(&s, flags); }
  hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(&s, flags, priority); }
  void       reset() {
    if (s) {
      (void)hipStreamSynchronize(s);
      (void)hipStreamDestroy(s);
    }
    s = nullptr;
  }
  operator hipStream_t() const { return s; }
};

struct SeqCtxHold { // the sequence store of a stage that gathers its output from one
  msgpu_seqctx *p = nullptr;
  ~SeqCtxHold() { msgpu_seq_destroy(p); }
  operator msgpu_seqctx *() const { return p; }
};

struct SeqFileHold { // a parsed sequence file, freed on every way out
  msgpu_seqfile *f = nullptr;
  ~SeqFileHold() { msgpu_seq_free(f); }
  operator const msgpu_seqfile *() const { return f; }
};

// ---- device memory

struct DevArena { // device memory freed on every way out of a run
  std::vector<void *> p;
  std::vector<size_t> p_bytes;       // the size of every block of p
  void               *tmp = nullptr; // one temporary buffer for every rocPRIM call of the run, grown when a call needs more
  size_t              tmp_bytes = 0;
  size_t              live = 0, peak = 0; // the bytes held now, and the most that were held at once (since the last rewind())
  // A reserved arena (reserve()) holds one block and hands out its bytes instead of calling hipMalloc: get() takes them from
  // the front, 256-byte aligned, the temporary buffer lies at the back and grows towards the front, and rewind() gives
  // everything back at once.  A stage that runs in batches reserves the largest batch's bytes once: no hipMalloc and no
  // hipFree (which synchronises the device) per batch, and `peak` is what a batch really touched.
  uint8_t *pool = nullptr;
  size_t   pool_bytes = 0, pool_used = 0;
  static constexpr size_t ALIGN = 256;
  static size_t           aligned(size_t n) { return (n + ALIGN - 1) / ALIGN * ALIGN; }
  // MSGPU_POISON (debugging, asked per call; see DevBuf::ensure in msgpu_devbuf.h): whatever get(), room(), reserve() and
  // rewind() hand out is filled with 0xA5, and the fill is complete when they return (the stage streams do not wait for the
  // null stream).  A block from hipMalloc, and a reservation as a whole, then lies between two guards of GUARD bytes of
  // 0xC3 that belong to the same allocation and to nobody: drop() checks those of its block, verify() those of every block
  // still held.  The blocks inside a reservation stay adjacent and are not fenced from one another.  The guards are not
  // counted in live / peak.  Without the variable none of this exists: the same calls, sizes and addresses as ever.
  static constexpr size_t  GUARD = 256;
  static constexpr uint8_t POISON_BYTE = 0xA5, GUARD_BYTE = 0xC3;
  struct Fenced { // a block between guards: its address as handed out, its bytes, its number among the arena's allocations
    void  *x;
    size_t bytes, index;
  };
  std::vector<Fenced> fenced;
  bool                pool_fenced = false;
  size_t              n_blocks = 0; // the blocks from hipMalloc so far (a reservation is the one block of its arena)
  std::string         broken;       // the first guard found overwritten, kept for verify()
  static bool poisoned() { return getenv("MSGPU_POISON") != nullptr; }
  static hipError_t fill(void *x, size_t n, bool wait_first) { // 0xA5 over n bytes that work in flight may still use, or nobody
    hipError_t e = wait_first ? hipDeviceSynchronize() : hipSuccess;
    if (e == hipSuccess) e = hipMemset(x, POISON_BYTE, n);
    return e == hipSuccess ? hipDeviceSynchronize() : e;
  }
  static hipError_t fence(uint8_t *base, size_t n) { // guard, n bytes of poison, guard
    hipError_t e = hipMemset(base, GUARD_BYTE, GUARD);
    if (e == hipSuccess) e = hipMemset(base + GUARD + n, GUARD_BYTE, GUARD);
    return e == hipSuccess ? fill(base + GUARD, n, false) : e;
  }
  void *base_of(void *x) const { // what hipMalloc returned for block x
    for (const Fenced &f : fenced)
      if (f.x == x) return static_cast<uint8_t *>(x) - GUARD;
    return x;
  }
  ~DevArena() {
    for (void *x : p) (void)hipFree(base_of(x));
    if (pool) (void)hipFree(pool_fenced ? pool - GUARD : pool);
  }
  void hold(size_t n) {
    live += n;
    peak = std::max(peak, live);
  }
  hipError_t reserve(size_t n) { // once, on an arena that holds nothing
    pool_bytes = aligned(n ? n : 1);
    if (!poisoned()) return hipMalloc(reinterpret_cast<void **>(&pool), pool_bytes);
    uint8_t   *m = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&m), pool_bytes + 2 * GUARD);
    if (e != hipSuccess) return e;
    e = fence(m, pool_bytes);
    if (e != hipSuccess) {
      (void)hipFree(m);
      return e;
    }
    pool        = m + GUARD;
    pool_fenced = true;
    return hipSuccess;
  }
  hipError_t rewind() { // (after a synchronisation) a reserved arena as it was after reserve()
    pool_used = tmp_bytes = live = peak = 0;
    tmp = nullptr;
    return pool && poisoned() ? fill(pool, pool_bytes, false) : hipSuccess;
  }
  template <class T> hipError_t get(T **out, size_t count) {
    const size_t n = (count ? count : 1) * sizeof(T);
    if (pool) {
      *out = nullptr;
      if (aligned(n) > pool_bytes - pool_used - tmp_bytes) return hipErrorOutOfMemory;
      if (poisoned()) { // (bytes that an earlier temporary buffer of the batch may have held)
        const hipError_t e = fill(pool + pool_used, aligned(n), true);
        if (e != hipSuccess) return e;
      }
      *out = reinterpret_cast<T *>(pool + pool_used);
      pool_used += aligned(n);
      hold(aligned(n));
      return hipSuccess;
    }
    const bool fenced_block = poisoned();
    void      *m = nullptr;
    hipError_t e = hipMalloc(&m, fenced_block ? n + 2 * GUARD : n);
    if (e == hipSuccess && fenced_block) {
      e = fence(static_cast<uint8_t *>(m), n);
      if (e == hipSuccess) {
        m = static_cast<uint8_t *>(m) + GUARD;
        fenced.push_back(Fenced{m, n, n_blocks});
      } else {
        (void)hipFree(m);
        m = nullptr;
      }
    }
    if (e == hipSuccess) {
      p.push_back(m);
      p_bytes.push_back(n);
      hold(n);
      ++n_blocks;
    }
    *out = static_cast<T *>(m);
    return e;
  }
  template <class T> hipError_t get_zeroed(T **out, size_t count, hipStream_t st) { // the block, zeroed in st
    hipError_t e = get(out, count);
    return e == hipSuccess && count ? hipMemsetAsync(*out, 0, count * sizeof(T), st) : e;
  }
  void drop(void *x) { // (not for the blocks of a reserved arena: rewind() returns those)
    auto it = std::find(p.begin(), p.end(), x);
    if (it != p.end()) {
      live -= p_bytes[it - p.begin()];
      p_bytes.erase(p_bytes.begin() + (it - p.begin()));
      p.erase(it);
    }
    for (size_t i = 0; i < fenced.size(); ++i)
      if (fenced[i].x == x) { // its guards, behind everything that may still write: hipFree would wait for that as well
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = check(x, fenced[i].bytes, fenced[i].index, false);
        if (e != hipSuccess && broken.empty()) broken = std::string("arena guard: ") + hipGetErrorString(e);
        x = static_cast<uint8_t *>(x) - GUARD;
        fenced.erase(fenced.begin() + i);
        break;
      }
    (void)hipFree(x);
  }
  hipError_t room(size_t need) {
    if (tmp && need <= tmp_bytes) return hipSuccess;
    if (pool) {
      const size_t n = aligned(need ? need : 1);
      if (n > pool_bytes - pool_used) return hipErrorOutOfMemory;
      if (poisoned()) { // (the smaller buffer it grows over may be in use)
        const hipError_t e = fill(pool + pool_bytes - n, n, true);
        if (e != hipSuccess) return e;
      }
      hold(n - tmp_bytes);
      tmp       = pool + pool_bytes - n;
      tmp_bytes = n;
      return hipSuccess;
    }
    uint8_t   *t = nullptr;
    hipError_t e = get(&t, need);
    if (e == hipSuccess) {
      tmp       = t;
      tmp_bytes = need;
    }
    return e;
  }
  void drop_tmp() { // (after a synchronisation) a large temporary buffer that the rest of the run should not carry
    if (pool) live -= tmp_bytes;
    else drop(tmp);
    tmp       = nullptr;
    tmp_bytes = 0;
  }
  // the two guards around the n bytes at x (behind a synchronisation); the first byte that is not a guard's goes into `broken`
  hipError_t check(const void *x, size_t n, size_t index, bool reservation) {
    uint8_t        h[2 * GUARD];
    const uint8_t *b = static_cast<const uint8_t *>(x);
    hipError_t     e = hipMemcpy(h, b - GUARD, GUARD, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h + GUARD, b + n, GUARD, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return e;
    for (size_t i = 0; i < 2 * GUARD && broken.empty(); ++i)
      if (h[i] != GUARD_BYTE) {
        char t[192];
        snprintf(t, sizeof(t), "arena guard: block %zu%s of %zu bytes: the %s guard was written (0x%02x at byte %zu of its %zu)", index,
                 reservation ? " (the reservation)" : "", n, i < GUARD ? "front" : "back", h[i], i % GUARD, GUARD);
        broken = t;
      }
    return hipSuccess;
  }
  // The guards of every block still held, behind a synchronisation of st; nothing without MSGPU_POISON.  Anything but
  // hipSuccess: a guard was written (here, or in a block that drop() gave back), or the check itself failed; `err` says which
  hipError_t verify(hipStream_t st, char *err, size_t err_bytes) {
    if (!poisoned()) return hipSuccess;
    hipError_t e = hipStreamSynchronize(st);
    for (size_t i = 0; i < fenced.size() && e == hipSuccess; ++i) e = check(fenced[i].x, fenced[i].bytes, fenced[i].index, false);
    if (e == hipSuccess && pool_fenced) e = check(pool, pool_bytes, 0, true);
    if (e != hipSuccess) snprintf(err, err_bytes, "arena guard: %s", hipGetErrorString(e));
    else if (!broken.empty()) snprintf(err, err_bytes, "%s", broken.c_str());
    else return hipSuccess;
    return e != hipSuccess ? e : hipErrorIllegalState;
  }
};

// the arena's guards before a run returns MSGPU_OK (DevArena::verify): a written guard is an error of the run
template <class C> int stage_verify(C *c, DevArena &D) {
  return D.verify(c->stream, c->err, sizeof(c->err)) == hipSuccess ? MSGPU_OK : MSGPU_E_HIP;
}

// rocPRIM's two calls on the arena's temporary buffer: call(null, bytes) answers the size, call(tmp, bytes) runs
template <class Call> hipError_t stage_rocprim(DevArena &D, Call &&call) {
  size_t     need = 0;
  hipError_t e    = call(static_cast<void *>(nullptr), need);
  if (e == hipSuccess) e = D.room(need);
  if (e == hipSuccess) e = call(D.tmp, need);
  return e;
}
// exclusive sums from zero of n values, in the type of `out`
template <class In, class Out> hipError_t stage_scan(DevArena &D, hipStream_t st, In in, Out *out, size_t n) {
  return stage_rocprim(D, [&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, Out(0), n, rocprim::plus<Out>(), st); });
}
// stable sort of n (key, value) pairs by the key's bits [0, end_bit)
template <class K, class V>
hipError_t stage_sort_pairs(DevArena &D, hipStream_t st, K *kin, K *kout, V *vin, V *vout, size_t n, unsigned end_bit = 8 * sizeof(K)) {
  return stage_rocprim(D, [&](void *t, size_t &b) {
    return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, static_cast<unsigned int>(n), 0, end_bit, st);
  });
}

inline uint32_t grid_of(uint64_t n, uint32_t per) { return static_cast<uint32_t>((n + per - 1) / per); }
inline uint32_t grid256(uint64_t n) { return grid_of(n, 256); }

// ---- time

struct StageClock { // device steps by event pairs, summed per step after the run's last synchronisation
  struct Span {
    EventHold a, b;
    float    *acc = nullptr;
  };
  std::vector<Span> spans;
  hipStream_t       st;
  explicit StageClock(hipStream_t s) : st(s) {}
  hipError_t begin(float *acc) {
    Span s;
    s.acc        = acc;
    hipError_t e = s.a.create();
    if (e == hipSuccess) e = s.b.create();
    if (e == hipSuccess) e = hipEventRecord(s.a, st);
    spans.push_back(std::move(s));
    return e;
  }
  hipError_t end() { return hipEventRecord(spans.back().b, st); }
  void       collect() { // (after a synchronisation)
    for (auto &s : spans) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) *s.acc += ms;
    }
    spans.clear();
  }
};

struct StageTimer { // wall-clock milliseconds since it was made
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
  float ms() const { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

// ---- the scalar block

// SC_COUNT words on the device, read through the project's read-back protocol (msgpu_device.h, publish_to_host), in one of
// two modes decided when the block is created:
// - mapped (default): no copy and no stream synchronisation.  The launch that closes a step carries arm()'s HostPublish, one
//   wavefront of it writes the block into the mapped mirror and publishes a sequence number, the host polls for it in wait()
//   (about half the latency of copy + synchronise).  A stream that ends or breaks without the number arriving is answered by
//   a copy, and counted.
// - copy (MSGPU_SYNC_READBACK, or no mapped pointer): arm() gives a launch nothing to publish; wait() enqueues one copy of
//   the block into the mirror and waits for it.
// Work that does not depend on the values can be enqueued between the armed launch and wait(): it keeps the GPU busy while
// the host turns around.  read() is the two halves around a one-wavefront launch of its own.
struct ScalarBlock {
  uint64_t *d = nullptr;     // the block on the device
  uint64_t *h = nullptr;     // its page-locked, device-mapped mirror and the sequence number behind it
  uint64_t *h_dev = nullptr; // the device's address of the mirror; null: every read-back is a copy
  uint64_t  seq = 0, lost = 0;
  EventHold copied; // recorded behind the copy mode's copy: a caller can wait for that alone
  ~ScalarBlock() {
    if (d) (void)hipFree(d);
    if (h) (void)hipHostFree(h);
  }
  int create() { // on the current device; zeroed.  The mirror is coherent: the host polls it while a kernel writes it
    if (hipHostMalloc(reinterpret_cast<void **>(&h), (SC_COUNT + 1) * sizeof(uint64_t), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
      h = nullptr;
      return MSGPU_E_NOMEM;
    }
    memset(h, 0, (SC_COUNT + 1) * sizeof(uint64_t));
    void *dev = nullptr;
    if (!getenv("MSGPU_SYNC_READBACK") && hipHostGetDevicePointer(&dev, h, 0) == hipSuccess) h_dev = static_cast<uint64_t *>(dev);
    const bool ok = hipMalloc(reinterpret_cast<void **>(&d), SC_COUNT * sizeof(uint64_t)) == hipSuccess &&
                    hipMemset(d, 0, SC_COUNT * sizeof(uint64_t)) == hipSuccess && hipStreamSynchronize(nullptr) == hipSuccess &&
                    copied.create(hipEventDisableTiming) == hipSuccess;
    return ok ? MSGPU_OK : MSGPU_E_HIP;
  }
  HostPublish arm() { return h_dev ? HostPublish{h_dev, ++seq} : HostPublish{nullptr, 0}; }
  // The block as the launch that took arm() left it -> h.  `late()` is asked about once a millisecond, while c's stream is
  // still busy, whether the caller has waited long enough: not MSGPU_OK ends the wait with that code.  `sync(event)` is the
  // caller's wait for a copy: for the event behind it, or (null) for c's stream.
  template <class Late, class Sync> int wait(StageCtx *c, Late late, Sync sync) {
    if (h_dev) {
      const uint64_t     s    = seq;
      volatile uint64_t *flag = h + SC_COUNT;
      for (uint64_t spins = 1;; ++spins) {
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == s) return MSGPU_OK;
        __builtin_ia32_pause();
        if ((spins & 0xffff) == 0) { // every ~1 ms: is the stream still alive?
          const hipError_t q = hipStreamQuery(c->stream);
          if (q == hipSuccess) { // everything ran: the number is there, or something is badly wrong
            if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == s) return MSGPU_OK;
            break;
          }
          if (q != hipErrorNotReady) break;
          if (int rc = late()) return rc;
        }
      }
      // The stream stopped making progress, or finished without the publication arriving in mapped memory.  Take the values
      // the slow way, surface a stream error if there is one, and count it either way.  The error text is NOT touched on a
      // call that goes on to succeed: the text belongs to a non-zero return code.
      ++lost;
    }
    STAGE_HIP(c, hipMemcpyAsync(h, d, SC_COUNT * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (h_dev) return sync(nullptr);
    STAGE_HIP(c, hipEventRecord(copied, c->stream));
    return sync(copied);
  }
  int wait(StageCtx *c) { // no deadline, and a copy is waited for with the stream
    return wait(c, [] { return MSGPU_OK; }, [c](hipEvent_t) -> int {
      STAGE_HIP(c, hipStreamSynchronize(c->stream));
      return MSGPU_OK;
    });
  }
  int read(StageCtx *c) { // the block as it stands at this point of c's stream -> h
    const HostPublish p = arm();
    if (p.seq) {
      launch_publish_scalars(c->stream, d, p);
      STAGE_HIP(c, hipGetLastError());
    }
    return wait(c);
  }
};

// Exclusive sums of n + 1 words of which the last is zero, so that out[n] is the total, and the total into `slot` of the
// scalar block.  Nothing is read back: the caller's sc.read(c) does that, behind whatever else it enqueues first.
template <class Out> hipError_t stage_scan_total(DevArena &D, hipStream_t st, const uint32_t *in, Out *out, size_t n, ScalarBlock &sc, int slot) {
  const hipError_t e = stage_scan(D, st, in, out, n + 1);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_stage_put<Out>, dim3(1), dim3(64), 0, st, sc.d, slot, out + n);
  return hipGetLastError();
}

// a key of 64 or of 128 bits as (hi, lo)
template <class K> void key_split(K key, uint64_t &hi, uint64_t &lo) {
  lo = static_cast<uint64_t>(key);
  if constexpr (sizeof(K) > 8) hi = static_cast<uint64_t>(key >> 64);
  else hi = 0;
}

// ---- the records a stage's ids name

constexpr uint32_t STAGE_NONE = 0xffffffffu;

// rec_ids[i] = id_of_name(name of record i) (STAGE_NONE: no id of the stage's), rec_of[id] = the first record of that id.
// Returns the first k < n_want whose id want[k] (k itself where want is null) has no record, or STAGE_NONE: the caller says
// which line asked for it.
template <class IdOfName>
uint32_t stage_first_records(const msgpu_seqfile *f, IdOfName id_of_name, uint32_t n_ids, const uint32_t *want, uint32_t n_want,
                             std::vector<uint32_t> &rec_ids, std::vector<uint32_t> &rec_of) {
  const uint32_t nr = msgpu_seq_count(f);
  rec_ids.resize(nr);
  rec_of.assign(n_ids, STAGE_NONE);
  for (uint32_t i = 0; i < nr; ++i) {
    rec_ids[i] = id_of_name(msgpu_seq_name(f, i));
    if (rec_ids[i] != STAGE_NONE && rec_of[rec_ids[i]] == STAGE_NONE) rec_of[rec_ids[i]] = i;
  }
  for (uint32_t k = 0; k < n_want; ++k)
    if (rec_of[want ? want[k] : k] == STAGE_NONE) return k;
  return STAGE_NONE;
}

struct StageFile { // a parsed file in its store, and its records as the kernels see them
  SeqFileHold f;
  SeqRecs     recs{};
};

// `path` into store `kind` of the context's sequence store, and the records' offsets and lengths into the arena (a zero behind
// the lengths: their scan gives n + 1 sums).  `what` names the file in the error texts
template <class Ctx> int stage_load(Ctx *c, DevArena &D, const char *path, int kind, const char *what, StageFile &F) {
  int rc = msgpu_seq_parse_upload(c->seq, kind, path, -1, &F.f.f);
  if (rc != MSGPU_OK) {
    snprintf(c->err, sizeof(c->err), "%s %s: %s", what, path, msgpu_seq_last_error(c->seq));
    return rc;
  }
  const uint32_t        n = msgpu_seq_count(F.f);
  std::vector<uint64_t> off;
  std::vector<uint32_t> len;
  try {
    off.resize(n);
    len.resize(n);
  } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
  uint64_t n_bases = 0;
  F.recs.bases = seq_store_bases(c->seq, kind, &n_bases);
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t L = msgpu_seq_length(F.f, i);
    off[i] = msgpu_seq_offset(F.f, i);
    if (L >= (1ull << 31)) {
      snprintf(c->err, sizeof(c->err), "%s record %u has %llu bases; the limit is 2^31 - 1", what, i, static_cast<unsigned long long>(L));
      return MSGPU_E_ARG;
    }
    if ((i && off[i] < off[i - 1] + len[i - 1]) || off[i] + L > n_bases) {
      snprintf(c->err, sizeof(c->err), "%s record %u does not lie behind record %u in the store", what, i, i ? i - 1 : 0);
      return MSGPU_E_STATE;
    }
    len[i] = static_cast<uint32_t>(L);
  }
  if (n_bases >= (1ull << 38)) {
    snprintf(c->err, sizeof(c->err), "%s: %llu bases; the limit is 2^38 - 1", what, static_cast<unsigned long long>(n_bases));
    return MSGPU_E_ARG;
  }
  uint64_t *d_off;
  uint32_t *d_len;
  STAGE_HIP(c, D.get(&d_off, n));
  STAGE_HIP(c, D.get(&d_len, n + 1ull));
  STAGE_HIP(c, hipMemsetAsync(d_len + n, 0, 4, c->stream));
  if (n) {
    STAGE_HIP(c, hipMemcpyAsync(d_off, off.data(), n * 8ull, hipMemcpyHostToDevice, c->stream));
    STAGE_HIP(c, hipMemcpyAsync(d_len, len.data(), n * 4ull, hipMemcpyHostToDevice, c->stream));
    STAGE_HIP(c, hipStreamSynchronize(c->stream));
  }
  F.recs.off     = d_off;
  F.recs.len     = d_len;
  F.recs.n       = n;
  F.recs.n_bases = n_bases;
  return MSGPU_OK;
}

// ---- a stage's FASTA text

// The records of the text, collected one by one, and their way to the host: the bases gathered from the context's sequence
// store piece by piece (or written by the stage's own kernels), wrapped by msgpu_fasta_format, copied.
struct FastaOut {
  StageTimer                      planning; // from the first record to the gather plan
  std::vector<msgpu_copy>         pieces;
  std::vector<msgpu_fasta_record> recs;
  std::string                     hdr;      // every header, one behind the other
  uint64_t                        raw = 0, text = 0; // the bases and the bytes of text so far
  // a record of the n bases at `src` of the store (`from`: the MSGPU_COPY_* flags of its pieces), under header h of hn bytes
  void add(uint64_t src, uint64_t n, uint32_t from, const char *h, size_t hn) {
    // a record without bases: the header without its '\n' (msgpu_fasta_format closes every record with one)
    const uint32_t hl = static_cast<uint32_t>(n ? hn : hn - 1);
    if (n) pieces.push_back(msgpu_copy{src, raw, static_cast<uint32_t>(n), from});
    recs.push_back(msgpu_fasta_record{raw, text, static_cast<uint32_t>(n), static_cast<uint32_t>(hdr.size()), hl, 0});
    hdr.append(h, hl);
    raw += n;
    text += msgpu_fasta_text_bytes(hl, n);
  }
  // The text -> dest, through the arena; returns behind the stream's synchronisation with the clock collected.  d_raw: the
  // records' bases where the stage wrote them itself; null: the pieces are gathered from the store.  The four accumulators
  // take the planning time and the spans of gather, format and copy (null: no span)
  template <class Ctx, class Text /* of chars: a string or a vector */>
  int emit(Ctx *c, DevArena &D, StageClock &clock, const uint8_t *d_raw, float *plan_ms, float *gather_ms, float *format_ms, float *copy_ms,
           Text &dest) {
    hipStream_t st = c->stream;
    if (hdr.size() >= 0xffffffffull) return MSGPU_E_ARG;
    const bool gathers = !d_raw;
    struct FreePlan {
      msgpu_gather_plan *p = nullptr;
      ~FreePlan() { msgpu_gather_plan_free(p); }
    } plan;
    int rc = MSGPU_OK;
    if (gathers) {
      rc = msgpu_gather_plan_create(c->seq, pieces.data(), pieces.size(), &plan.p);
      if (rc != MSGPU_OK) {
        snprintf(c->err, sizeof(c->err), "gather plan: %s", msgpu_seq_last_error(c->seq));
        return rc;
      }
    }
    if (plan_ms) *plan_ms = planning.ms();
    uint8_t *d_gathered = nullptr, *d_text;
    if (gathers) STAGE_HIP(c, D.get(&d_gathered, raw + 16));
    STAGE_HIP(c, D.get(&d_text, text + 16));
    if (gathers) {
      d_raw = d_gathered;
      if (gather_ms) STAGE_HIP(c, clock.begin(gather_ms));
      rc = msgpu_gather_run(c->seq, plan.p, d_gathered, raw + 16, st);
      if (rc == MSGPU_OK && gather_ms) STAGE_HIP(c, clock.end());
    }
    if (rc == MSGPU_OK) {
      if (format_ms) STAGE_HIP(c, clock.begin(format_ms)); // (from the same point of the stream)
      rc = msgpu_fasta_format(c->seq, d_raw, recs.data(), recs.size(), hdr.data(), hdr.size(), d_text, text + 16, st);
    }
    if (rc != MSGPU_OK) {
      snprintf(c->err, sizeof(c->err), "%s: %s", gathers ? "gather / format" : "format", msgpu_seq_last_error(c->seq));
      return rc;
    }
    if (format_ms) STAGE_HIP(c, clock.end());
    if (copy_ms) STAGE_HIP(c, clock.begin(copy_ms)); // (from the same point of the stream)
    try {
      dest.resize(text);
    } catch (std::bad_alloc const &) { return MSGPU_E_NOMEM; }
    if (text) STAGE_HIP(c, hipMemcpyAsync(&dest[0], d_text, text, hipMemcpyDeviceToHost, st));
    if (copy_ms) STAGE_HIP(c, clock.end());
    STAGE_HIP(c, hipStreamSynchronize(st));
    clock.collect();
    return MSGPU_OK;
  }
};

} // namespace msgpu

#endif
