// dp_pool.h -- the bookkeeping of device resources that outlive a call (DESIGN.md "Device resources"): the 256-byte rounding,
// the bump carver, the pool of idle device slabs and the pool of idle per-device objects.  Plain C++: nothing here includes HIP,
// allocates device memory or frees it (dp_hip.h does, with what these hand back), so tests/native/slab_pool_main.cpp drives all of
// it on the CPU.
#ifndef PAGAN_DP_POOL_H
#define PAGAN_DP_POOL_H

#include <cstddef>
#include <mutex>
#include <utility>
#include <vector>

namespace pgdev {

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// Bump carver over one allocation, every piece rounded up to 256 bytes.  A null `base` only sizes: the same calls, `cur` the
// total, no pointer handed out.  take<T>(0) takes one element, so that two arrays never share an address.
struct Carve {
    char *base; size_t cur = 0;
    size_t skip(size_t bytes) { const size_t at = cur; cur += up256(bytes); return at; }           // the piece's offset
    template <class T> T *take(size_t n) { const size_t at = skip(sizeof(T) * (n ? n : 1)); return base ? (T *)(base + at) : nullptr; }
};

struct Slab { int device; char *p; size_t cap; };

// What one pool of idle slabs does; 0 switches a rule off.  (the rule on a failed allocation is dp_hip.h's slab_alloc)
struct SlabPolicy {
    size_t slack_mul, slack_add;     // an idle slab is taken for `need` bytes only if cap <= slack_mul * need + slack_add
    size_t grow_div;                 // a miss allocates need + need / grow_div
    size_t max_idle;                 // idle slabs in all ...
    size_t max_idle_per_device;      // ... and on the device a slab is given back to
    size_t max_idle_bytes;           // idle bytes in all, while more than one slab is idle
    bool evict_smallest;             // over a bound: the smallest idle slab of that device goes (false: the oldest of all)
    bool retry_drained;              // a failed allocation: the pool's idle slabs are freed and the allocation is tried once more
    size_t miss_bytes(size_t need) const { return grow_div ? need + need / grow_div : need; }
};

// Idle slabs of all devices.  Bookkeeping only: what leaves the pool for good is handed to the caller in `drop`, who frees it
// after the call -- nothing is freed while the mutex is held (a hipFree of a few GB takes 10-30 ms and synchronises the device).
struct SlabPool {
    explicit SlabPool(const SlabPolicy &policy) : pol(policy) {}
    // the smallest idle slab of `device` with cap >= need (the oldest of equals) unless the policy finds it too large; nullptr: a miss
    char *take(int device, size_t need, size_t *cap) {
        std::lock_guard<std::mutex> g(m);
        int best = -1;
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].device == device && idle[k].cap >= need && (best < 0 || idle[k].cap < idle[best].cap)) best = (int)k;
        if (best < 0 || (pol.slack_mul && idle[best].cap > pol.slack_mul * need + pol.slack_add)) return nullptr;
        char *p = idle[best].p;
        *cap = idle[best].cap;
        idle.erase(idle.begin() + best);
        return p;
    }
    // the slab is idle from here on (a null one is ignored); what the policy evicts for it is appended to `drop`, in eviction order
    void give(int device, char *p, size_t cap, std::vector<Slab> *drop) {
        if (!p) return;
        std::lock_guard<std::mutex> g(m);
        idle.push_back({device, p, cap});
        for (;;) {
            size_t bytes = 0, here = 0;
            int smallest = -1;
            for (size_t k = 0; k < idle.size(); ++k) {
                bytes += idle[k].cap;
                if (idle[k].device != device) continue;
                ++here;
                if (smallest < 0 || idle[k].cap < idle[smallest].cap) smallest = (int)k;
            }
            const bool over = (pol.max_idle && idle.size() > pol.max_idle) || (pol.max_idle_per_device && here > pol.max_idle_per_device) ||
                              (pol.max_idle_bytes && bytes > pol.max_idle_bytes && idle.size() > 1);
            if (!over) break;
            const int victim = pol.evict_smallest ? smallest : 0;
            drop->push_back(idle[victim]);
            idle.erase(idle.begin() + victim);
        }
    }
    // the idle slabs of one device (-1: of all) leave the pool, oldest first
    void drain(int device, std::vector<Slab> *drop) {
        std::lock_guard<std::mutex> g(m);
        for (size_t k = 0; k < idle.size();)
            if (device < 0 || idle[k].device == device) { drop->push_back(idle[k]); idle.erase(idle.begin() + k); } else ++k;
    }
    size_t idle_bytes(int device) {
        std::lock_guard<std::mutex> g(m);
        size_t n = 0;
        for (const Slab &s : idle) if (s.device == device) n += s.cap;
        return n;
    }
    const SlabPolicy pol;
    std::mutex m;
    std::vector<Slab> idle;
};

// Idle objects that belong to a device (a batch's streams and events, a builder's stream, a finder's scratch): the first idle
// one on the device, else the caller makes one.  What the pool does not keep goes to the caller, who destroys it after the call.
template <class T>
struct IdlePerDevice {
    bool take(int device, T *out) {
        std::lock_guard<std::mutex> g(m);
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].first == device) { *out = idle[k].second; idle.erase(idle.begin() + k); return true; }
        return false;
    }
    // max_per_device idle ones already on `device` (0: no bound): `o` is not kept but appended to `dropped`
    void give(int device, const T &o, size_t max_per_device, std::vector<std::pair<int, T>> *dropped) {
        std::lock_guard<std::mutex> g(m);
        size_t have = 0;
        for (const auto &e : idle) have += e.first == device;
        if (max_per_device && have >= max_per_device) dropped->emplace_back(device, o);
        else idle.emplace_back(device, o);
    }
    void drain(std::vector<std::pair<int, T>> *all) {
        std::lock_guard<std::mutex> g(m);
        all->insert(all->end(), idle.begin(), idle.end()), idle.clear();
    }
    std::mutex m;
    std::vector<std::pair<int, T>> idle;
};

} // namespace pgdev

#endif
