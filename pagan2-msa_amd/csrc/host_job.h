// host_job.h -- one alignment job of the host side (a node of the tree walk, a step of the pileup chain) and the owner of its
// result.  Plain C++17, no HIP: tests/native/host_job_main.cpp drives it under sanitizers with a pagan_result_free of its own.
#pragma once
#include <utility>
#include <vector>

#include "../../include/pagan_host.h"

namespace pagan {

// A pagan_result whose three arrays are released exactly once.  Move-only; empty reads as a zeroed struct.
class OwnedResult {
    pagan_result r_{};
    bool held_ = false;
    void take(OwnedResult &o) { r_ = o.r_; held_ = o.held_; o.r_ = pagan_result{}; o.held_ = false; }
public:
    OwnedResult() = default;
    OwnedResult(OwnedResult &&o) noexcept { take(o); }
    OwnedResult &operator=(OwnedResult &&o) noexcept { if (this != &o) { reset(); take(o); } return *this; }
    ~OwnedResult() { reset(); }
    void reset() { if (held_) pagan_result_free(&r_); r_ = pagan_result{}; held_ = false; }
    // takes over a struct the library (or the importer) just filled: only after PAGAN_OK -- after an error return nothing in
    // it is valid, the library released it
    void adopt(const pagan_result &raw) { reset(); r_ = raw; held_ = true; }
    bool held() const { return held_; }
    const pagan_result &get() const { return r_; }
};

// What one call of the aligner consumes and leaves: the two child graphs' views, the tunnel, the result.  pb points into
// upper / lower: a move re-seats it.
struct NodeJob {
    pagan_graph gl{}, gr{};
    std::vector<int32_t> upper, lower;
    pagan_band pb{};
    bool banded = false;
    OwnedResult res;
    NodeJob() = default;
    NodeJob(NodeJob &&o) noexcept { *this = std::move(o); }
    NodeJob &operator=(NodeJob &&o) noexcept {
        if (this == &o) return *this;
        gl = o.gl; gr = o.gr; upper = std::move(o.upper); lower = std::move(o.lower); banded = o.banded; res = std::move(o.res);
        o.banded = false;
        seat(); o.seat();
        return *this;
    }
    void seat() { pb.n = (int32_t)upper.size(); pb.upper = upper.data(); pb.lower = lower.data(); }
    void set_band() { seat(); banded = true; }                      // upper / lower are filled: the job runs inside them
    const pagan_band *band() const { return banded ? &pb : nullptr; }
    pagan_job job(const pagan_model *pm) const { return pagan_job{&gl, &gr, pm, band()}; }
};

// The aligner behind the test seam (pagan_msa_set_batch_backend, pagan_pileup_set_batch_backend) or the library's own
inline int call_aligner(pagan_batch_fn backend, void *user, int32_t n, const pagan_job *jobs, const pagan_opts *po, pagan_result *res) {
    return backend ? backend(n, jobs, po, res, user) : pagan_dp_align_batch(n, jobs, po, res);
}

} // namespace pagan
