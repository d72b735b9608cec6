// slab_pool_main.cpp -- pagan2-msa_amd/csrc/dp_pool.h on its own, for a host compiler's sanitizers: tests/test_pool_cpu.py compiles
// this file under -fsanitize=address,undefined and runs it as a child process.
//
// The three pools of idle device memory the library had before dp_pool.h -- the batch arenas of dp_abi.hip, the forward/backward
// arenas of dp_fb.hip, the builder slabs of dp_parent.hip -- are restated here as they were written, each on its own, with the
// device calls replaced by a counter that hands out addresses nobody reads through.  The program drives each of them and a
// SlabPool under that pool's policy with the same seeded sequence of take, allocate on a miss, give, drain of one device and
// drain of all over three devices, sizes from bytes to several GiB, and requires after every step the same address and capacity,
// the same evicted slabs in the same order and the same idle bytes on every device.  A run counts only if the old pool itself went
// through every rule it has (the counts are printed; a zero fails the run).  The same for IdlePerDevice with caps 0 and 4 against
// the old per-device object pool, and a check of Carve: sizing and carving give the same offsets, all multiples of 256, and
// no elements take one.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../pagan2-msa_amd/csrc/dp_pool.h"

namespace {

using pgdev::Slab;
using pgdev::SlabPolicy;

struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    uint64_t below(uint64_t n) { return next() % n; }
};

struct Fake {                                    // "hipMalloc": addresses 256 apart, never dereferenced
    uintptr_t at = 0x10000;
    char *alloc() { char *p = reinterpret_cast<char *>(at); at += 256; return p; }
};

struct Counts { long reuse = 0, refusal = 0, by_count = 0, by_bytes = 0, smallest_others_stay = 0; };

// ---- the old pools, as they were ----
struct Model {
    std::vector<Slab> idle;
    Fake mem;
    Counts n;
    virtual ~Model() {}
    virtual char *take(int device, size_t need, size_t *cap) = 0;            // an idle slab, else a new one
    virtual void give(int device, char *p, size_t cap, std::vector<Slab> *drop) = 0;
    int best_fit(int device, size_t need) const {
        int best = -1;
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].device == device && idle[k].cap >= need && (best < 0 || idle[k].cap < idle[best].cap)) best = (int)k;
        return best;
    }
    void clear(int device, std::vector<Slab> *drop) {
        for (size_t k = 0; k < idle.size();)
            if (device < 0 || idle[k].device == device) { drop->push_back(idle[k]); idle.erase(idle.begin() + k); } else ++k;
    }
    size_t idle_bytes(int device) const {
        size_t b = 0;
        for (const Slab &s : idle) if (s.device == device) b += s.cap;
        return b;
    }
};

struct BatchArenas : Model {                     // ArenaPool and take_arena
    char *take(int device, size_t n_, size_t *cap) override {
        const int best = best_fit(device, n_);
        if (best < 0) { *cap = n_; return mem.alloc(); }
        char *p = idle[best].p;
        *cap = idle[best].cap;
        idle.erase(idle.begin() + best);
        ++n.reuse;
        return p;
    }
    void give(int device, char *p, size_t cap, std::vector<Slab> *drop) override {
        idle.push_back({device, p, cap});
        for (;;) {
            int count = 0, smallest = -1;
            for (size_t k = 0; k < idle.size(); ++k)
                if (idle[k].device == device) { ++count; if (smallest < 0 || idle[k].cap < idle[smallest].cap) smallest = (int)k; }
            if (count <= 2) break;
            drop->push_back(idle[smallest]);
            idle.erase(idle.begin() + smallest);
            ++n.by_count;
            if ((int)idle.size() > count - 1) ++n.smallest_others_stay;
        }
    }
};

struct FbArenas : Model {                        // FbArenaPool
    char *take(int device, size_t need, size_t *cap) override {
        const int best = best_fit(device, need);
        if (best >= 0 && idle[best].cap <= 2 * need + (64u << 20)) {
            Slab s_ = idle[best]; idle.erase(idle.begin() + best); *cap = s_.cap; ++n.reuse; return s_.p;
        }
        if (best >= 0) ++n.refusal;
        *cap = need + need / 16;
        return mem.alloc();
    }
    void give(int device, char *p, size_t cap, std::vector<Slab> *drop) override {
        const size_t kMaxIdleBytes = (size_t)8 << 30;
        idle.push_back({device, p, cap});
        size_t total = 0;
        for (auto &s_ : idle) total += s_.cap;
        while (idle.size() > 32 || (total > kMaxIdleBytes && idle.size() > 1)) {
            if (idle.size() > 32) ++n.by_count; else ++n.by_bytes;
            total -= idle.front().cap;
            drop->push_back(idle.front());
            idle.erase(idle.begin());
        }
    }
};

struct BuilderSlabs : Model {                    // MemPool
    char *take(int device, size_t need, size_t *cap) override {
        const int best = best_fit(device, need);
        if (best >= 0 && idle[best].cap <= 4 * need + (1u << 20)) {
            Slab s = idle[best]; idle.erase(idle.begin() + best); *cap = s.cap; ++n.reuse; return s.p;
        }
        if (best >= 0) ++n.refusal;
        *cap = need + need / 8;
        return mem.alloc();
    }
    void give(int device, char *p, size_t cap, std::vector<Slab> *drop) override {
        if (!p) return;
        if (idle.size() >= 48) { drop->push_back(idle.front()); idle.erase(idle.begin()); ++n.by_count; }
        idle.push_back({device, p, cap});
    }
};

// the policies as the library's translation units write them out (tests/test_pool_cpu.py compares these lines with theirs)
const SlabPolicy kArenaPolicy = {0, 0, 0, 0, 2, 0, true, false};
const SlabPolicy kFbArenaPolicy = {2, (size_t)64 << 20, 16, 32, 0, (size_t)8 << 30, false, true};
const SlabPolicy kParentPolicy = {4, (size_t)1 << 20, 8, 48, 0, 0, false, false};

bool same(const std::vector<Slab> &a, const std::vector<Slab> &b) {
    if (a.size() != b.size()) return false;
    for (size_t k = 0; k < a.size(); ++k) if (a[k].device != b[k].device || a[k].p != b[k].p || a[k].cap != b[k].cap) return false;
    return true;
}

int fail(const char *pool, uint64_t seed, int step, const char *what) {
    std::fprintf(stderr, "%s, seed %llu, step %d: %s differs\n", pool, (unsigned long long)seed, step, what);
    return 1;
}

// one seeded sequence on both; 0: they agreed at every step
int drive(const char *name, Model &model, const SlabPolicy &policy, uint64_t seed, int steps) {
    pgdev::SlabPool pool(policy);
    Fake mem;
    Rng rng{seed * 0x9E3779B97F4A7C15ull + 1};
    std::vector<Slab> live;                      // taken and not given back
    std::vector<size_t> seen;                    // capacities that went idle: a later request is cut to fit one of them
    for (int step = 0; step < steps; ++step) {
        const int device = (int)rng.below(3);
        const bool large = (step / 256) & 1;     // by turns: many small slabs (the bounds by count), slabs of GiB (the bound by bytes)
        const uint64_t op = rng.below(100);
        const uint64_t takes = (step / 128) % 4 == 0 ? 90 : 30;      // by turns: slabs pile up in use, then come back (the idle bounds)
        std::vector<Slab> drop_m, drop_p;
        if (op < takes || live.empty()) {
            size_t need = ((size_t)1 << rng.below(large ? 33 : 21)) + (size_t)rng.below(4096);
            if (!seen.empty() && rng.below(3) == 0) { const size_t c = seen[rng.below(seen.size())]; need = c - (size_t)rng.below(c / 2 + 1); }
            if (rng.below(16) == 0) need = 1 + (size_t)rng.below(64);
            size_t cap_m = 0, cap_p = 0;
            char *pm = model.take(device, need, &cap_m);
            char *pp = pool.take(device, need, &cap_p);
            if (!pp) { cap_p = policy.miss_bytes(need); pp = mem.alloc(); }
            if (pm != pp || cap_m != cap_p) return fail(name, seed, step, "take");
            live.push_back({device, pp, cap_p});
        } else if (op < 97) {
            const size_t k = (size_t)rng.below(live.size());
            const Slab s = live[k];
            live.erase(live.begin() + k);
            model.give(s.device, s.p, s.cap, &drop_m);
            pool.give(s.device, s.p, s.cap, &drop_p);
            seen.push_back(s.cap);
            if (seen.size() > 64) seen.erase(seen.begin());
        } else if (op == 97 && &policy == &kParentPolicy) {
            model.give(device, nullptr, 123, &drop_m);        // (the builder's pool is handed null slabs: ignored)
            pool.give(device, nullptr, 123, &drop_p);
        } else {
            const int which = op == 99 ? -1 : device;
            model.clear(which, &drop_m);
            pool.drain(which, &drop_p);
        }
        if (!same(drop_m, drop_p)) return fail(name, seed, step, "what was evicted");
        for (int d = 0; d < 3; ++d) if (model.idle_bytes(d) != pool.idle_bytes(d)) return fail(name, seed, step, "idle bytes");
    }
    return 0;
}

// ---- the old per-device object pool (GpuObjPool; StreamPool and ScratchPool are its unbounded case) ----
struct ObjModel {
    std::vector<std::pair<int, int>> idle;
    bool take(int device, int *o) {
        for (size_t k = 0; k < idle.size(); ++k)
            if (idle[k].first == device) { *o = idle[k].second; idle.erase(idle.begin() + k); return true; }
        return false;
    }
    void give(int device, int o, int bound, std::vector<std::pair<int, int>> *dropped) {
        int have = 0;
        for (auto &e : idle) have += e.first == device;
        if (bound && have >= bound) dropped->emplace_back(device, o);
        else idle.emplace_back(device, o);
    }
};

int drive_objects(size_t bound, uint64_t seed, int steps, long *reused, long *dropped_n) {
    ObjModel model;
    pgdev::IdlePerDevice<int> pool;
    Rng rng{seed * 0xD1B54A32D192ED03ull + 1};
    std::vector<std::pair<int, int>> live;
    int next_m = 0, next_p = 0;
    for (int step = 0; step < steps; ++step) {
        const int device = (int)rng.below(3);
        const uint64_t op = rng.below(100);
        std::vector<std::pair<int, int>> drop_m, drop_p;
        if (op < 40 || live.empty()) {
            int om = -1, op_ = -1;
            const bool hm = model.take(device, &om), hp = pool.take(device, &op_);
            if (!hm) om = next_m++; else ++*reused;
            if (!hp) op_ = next_p++;
            if (hm != hp || om != op_) { std::fprintf(stderr, "objects, cap %zu, seed %llu, step %d: take differs\n", bound, (unsigned long long)seed, step); return 1; }
            live.emplace_back(device, om);
        } else if (op < 97) {
            const size_t k = (size_t)rng.below(live.size());
            const std::pair<int, int> o = live[k];
            live.erase(live.begin() + k);
            model.give(o.first, o.second, (int)bound, &drop_m);
            pool.give(o.first, o.second, bound, &drop_p);
            *dropped_n += (long)drop_m.size();
        } else {
            drop_m = model.idle; model.idle.clear();
            pool.drain(&drop_p);
        }
        if (drop_m != drop_p) { std::fprintf(stderr, "objects, cap %zu, seed %llu, step %d: what left the pool differs\n", bound, (unsigned long long)seed, step); return 1; }
    }
    return 0;
}

struct Wide { char bytes[24]; };

int check_carve(uint64_t seed) {
    Rng rng{seed + 77};
    std::vector<std::pair<int, size_t>> calls;
    for (int k = 0; k < 200; ++k) calls.emplace_back((int)rng.below(4), rng.below(5) == 0 ? 0 : (size_t)rng.below(3000));
    std::vector<size_t> at_size, at_real;
    auto run = [&](pgdev::Carve &c, std::vector<size_t> *at) {
        for (auto &call : calls) {
            const size_t before = c.cur;
            char *p = nullptr;
            size_t elem = 0;
            switch (call.first) {
                case 0: p = (char *)c.take<char>(call.second); elem = 1; break;
                case 1: p = (char *)c.take<int32_t>(call.second); elem = 4; break;
                case 2: p = (char *)c.take<double>(call.second); elem = 8; break;
                default: p = (char *)c.take<Wide>(call.second); elem = sizeof(Wide); break;
            }
            if (c.base ? p != c.base + before : p != nullptr) return 1;
            if (before % 256 || c.cur % 256) return 1;
            const size_t n = call.second ? call.second : 1;                   // no elements take one
            if (c.cur - before != (elem * n + 255) / 256 * 256) return 1;
            at->push_back(before);
        }
        return 0;
    };
    pgdev::Carve sizing{nullptr};
    if (run(sizing, &at_size)) return 1;
    std::vector<char> buffer(sizing.cur);
    pgdev::Carve real{buffer.data()};
    if (run(real, &at_real)) return 1;
    if (at_size != at_real || sizing.cur != real.cur) return 1;
    pgdev::Carve offsets{nullptr};                                            // skip(): the offset; no bytes take none
    if (offsets.skip(0) != 0 || offsets.cur != 0 || offsets.skip(1) != 0 || offsets.skip(256) != 256 || offsets.skip(257) != 512 || offsets.cur != 1024) return 1;
    for (size_t x : {(size_t)0, (size_t)1, (size_t)255, (size_t)256, (size_t)257, ((size_t)6 << 30) + 1})
        if (pgdev::up256(x) != (x + 255) / 256 * 256) return 1;
    return 0;
}

} // namespace

int main(int argc, char **argv) {
    const int seeds = argc > 1 ? std::atoi(argv[1]) : 8, steps = argc > 2 ? std::atoi(argv[2]) : 4096;
    int bad = 0;
    {
        Counts n;
        for (int s = 1; s <= seeds && !(bad & 1); ++s) {
            BatchArenas m;
            bad |= drive("batch arenas", m, kArenaPolicy, s, steps);
            n.reuse += m.n.reuse; n.by_count += m.n.by_count; n.smallest_others_stay += m.n.smallest_others_stay;
        }
        std::printf("batch arenas: reuse %ld evicted_by_count %ld smallest_while_others_stay %ld\n", n.reuse, n.by_count, n.smallest_others_stay);
        if (!n.reuse || !n.by_count || !n.smallest_others_stay) bad |= 2;
    }
    {
        Counts n;
        for (int s = 1; s <= seeds && !(bad & 1); ++s) {
            FbArenas m;
            bad |= drive("fb arenas", m, kFbArenaPolicy, s, steps);
            n.reuse += m.n.reuse; n.refusal += m.n.refusal; n.by_count += m.n.by_count; n.by_bytes += m.n.by_bytes;
        }
        std::printf("fb arenas: reuse %ld refused_for_slack %ld evicted_by_count %ld evicted_by_bytes %ld\n", n.reuse, n.refusal, n.by_count, n.by_bytes);
        if (!n.reuse || !n.refusal || !n.by_count || !n.by_bytes) bad |= 2;
    }
    {
        Counts n;
        for (int s = 1; s <= seeds && !(bad & 1); ++s) {
            BuilderSlabs m;
            bad |= drive("builder slabs", m, kParentPolicy, s, steps);
            n.reuse += m.n.reuse; n.refusal += m.n.refusal; n.by_count += m.n.by_count;
        }
        std::printf("builder slabs: reuse %ld refused_for_slack %ld evicted_by_count %ld\n", n.reuse, n.refusal, n.by_count);
        if (!n.reuse || !n.refusal || !n.by_count) bad |= 2;
    }
    for (size_t bound : {(size_t)0, (size_t)4}) {
        long reused = 0, dropped = 0;
        for (int s = 1; s <= seeds && !(bad & 1); ++s) bad |= drive_objects(bound, s, steps, &reused, &dropped);
        std::printf("objects cap %zu: reuse %ld not_kept %ld\n", bound, reused, dropped);
        if (!reused || (bound ? !dropped : dropped != 0)) bad |= 2;
    }
    for (int s = 1; s <= seeds; ++s) if (check_carve(s)) { std::fprintf(stderr, "Carve: seed %d\n", s); bad |= 4; }
    std::printf("carve: %s\n", (bad & 4) ? "differs" : "ok");
    return bad;
}
