// dp_hip.h -- the HIP side of the device resources (DESIGN.md "Device resources"): one mapping of a HIP error to a PAGAN_* code,
// the scope that puts a thread on a device and back, the owners of a stream, an event and an allocation, and the two calls that
// turn dp_pool.h's bookkeeping into hipMalloc and hipFree.
#ifndef PAGAN_DP_HIP_H
#define PAGAN_DP_HIP_H

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "../../include/pagan_dp.h"
#include "dp_pool.h"

namespace pgdev {

// A failed HIP call as a PAGAN_* code: out of memory is PAGAN_E_NOMEM, anything else `other`; PAGAN_DP_VERBOSE=1 names the call.
inline int hip_code(hipError_t e, const char *tag, const char *expr, int other) {
    if (std::getenv("PAGAN_DP_VERBOSE")) std::fprintf(stderr, "%s: %s failed: %s\n", tag, expr, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PAGAN_E_NOMEM : other;
}
// Return the code / clear the sticky error and return false.  A translation unit names one once, with its tag and its `other`.
#define PG_HIP_CODE(expr, tag, other) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) return pgdev::hip_code(e_, tag, #expr, other); } while (0)
#define PG_HIP_BOOL(expr, tag) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) { (void)pgdev::hip_code(e_, tag, #expr, 0); (void)hipGetLastError(); return false; } } while (0)

// The calling thread on `device` (negative: the one it is on) for the length of a call, back on the device it came with afterwards.
struct DeviceScope {
    int back = -1, device; bool ok;
    explicit DeviceScope(int want) : device(want) {
        ok = hipGetDevice(&back) == hipSuccess;
        if (ok && device < 0) device = back;
        ok = ok && hipSetDevice(device) == hipSuccess;
    }
    ~DeviceScope() { if (back >= 0) (void)hipSetDevice(back); }
};

// Owners of what a call makes on the device: a stream, an event, an allocation.  Move-only; each frees in its destructor, on the
// device it was made on, so a return from the middle of a function leaks nothing.  A stream is SYNCHRONISED before it is
// destroyed: on a failure path its kernels may still be writing memory, and that memory must not reach a pool (whose next take
// would hand it out) or hipFree before they are done -- so whatever gives the memory back does so after the streams' owners are
// gone: a struct declares its DevBuf BEFORE its Stream.  On a success path the code has synchronised already and the
// destructor's wait is a no-op.
template <class T>
struct Owned {
    T h = nullptr; int device = 0;
    Owned() = default;
    Owned(Owned &&o) noexcept : h(o.h), device(o.device) { o.h = nullptr; }
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() { if (h) { DeviceScope on(device); drop(h); } }
    operator T() const { return h; }
    static void drop(hipStream_t s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    static void drop(hipEvent_t e) { (void)hipEventDestroy(e); }
    static void drop(char *p) { (void)hipFree(p); }
};
struct Stream : Owned<hipStream_t> {
    hipError_t create(unsigned flags = hipStreamDefault) { const hipError_t e = hipGetDevice(&device); return e != hipSuccess ? e : hipStreamCreateWithFlags(&h, flags); }
};
struct Event : Owned<hipEvent_t> {
    hipError_t create(bool timing = true) { const hipError_t e = hipGetDevice(&device); return e != hipSuccess ? e : hipEventCreateWithFlags(&h, timing ? hipEventDefault : hipEventDisableTiming); }
};
struct DevBuf : Owned<char *> {
    hipError_t alloc(size_t bytes) { const hipError_t e = hipGetDevice(&device); return e != hipSuccess ? e : hipMalloc((void **)&h, bytes); }
};

// Frees what a pool handed back, each slab on its own device; the caller holds no pool's mutex and stays on its device.
inline void free_slabs(const std::vector<Slab> &drop) {
    for (const Slab &s : drop) { DeviceScope on(s.device); (void)hipFree(s.p); }
}
inline void drain_slabs(SlabPool &pool, int device) {
    std::vector<Slab> drop;
    pool.drain(device, &drop);
    free_slabs(drop);
}
inline void give_slab(SlabPool &pool, int device, char *p, size_t cap) {
    std::vector<Slab> drop;
    pool.give(device, p, cap, &drop);
    free_slabs(drop);
}
// `need` bytes on `device`, which the thread is on: an idle slab of the pool, else a new one of the policy's size for a miss;
// where that fails and the policy says so, once more with the pool's idle slabs freed.  nullptr: no memory (no sticky error left).
inline char *slab_alloc(SlabPool &pool, int device, size_t need, size_t *cap) {
    char *p = pool.take(device, need, cap);
    if (p) return p;
    *cap = pool.pol.miss_bytes(need);
    for (int attempt = 0; attempt < 2; ++attempt) {
        if (hipMalloc((void **)&p, *cap) == hipSuccess) return p;
        (void)hipGetLastError();
        if (!pool.pol.retry_drained) break;
        if (attempt == 0) drain_slabs(pool, -1);               // (idle slabs may be what is in the way)
    }
    return nullptr;
}

} // namespace pgdev

#endif
