// host_job_main.cpp -- pagan2-msa_amd/csrc/host_job.h on its own, for a host compiler's sanitizers: tests/test_host_job_cpu.py
// compiles this file under -fsanitize=address,undefined and runs it as a child process.
//
// pagan_result_free is this program's: it frees the three arrays as the library's does, counts its calls and keeps the set of
// live results, so an array released twice or never is seen here as well as by the sanitizer.  The cases are the ones the walk
// (host_tree.cpp) and the pileup chain (host_pileup.cpp) go through: a result adopted and destroyed; adopted over a held one (the
// sampler or the decoder replacing a node's result in fb_node); reset, then adopted (the retry of an unreachable corner); moved
// while a vector reallocates (steps.emplace_back, work.resize); move-assigned onto a held one (pagan_msa_import_result); an
// empty result (n_cols == 0, null arrays); a NodeJob moved while its band points into its own vectors.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <utility>
#include <vector>

#include "../../pagan2-msa_amd/csrc/host_job.h"

namespace {

long frees = 0, bad = 0;
std::set<const void *> live;                     // the cols arrays of the results made and not yet released

pagan_result make(int n_cols, int tag) {
    pagan_result r{};
    r.status = PAGAN_DP_REACHED; r.score = tag; r.n_cols = n_cols; r.n_left_used = 2; r.n_right_used = 3;
    r.cols = (pagan_col *)std::malloc(sizeof(pagan_col) * (size_t)(n_cols > 0 ? n_cols : 1));
    r.left_used = (int32_t *)std::malloc(4 * 2);
    r.right_used = (int32_t *)std::malloc(4 * 3);
    for (int k = 0; k < n_cols; ++k) r.cols[k] = pagan_col{k + 1, k + 1, tag};
    live.insert(r.cols);
    return r;
}

bool readable(const pagan_result &r, int n_cols, int tag) {       // (the sanitizer sees a read of released memory)
    if (r.n_cols != n_cols || r.score != tag) return false;
    for (int k = 0; k < n_cols; ++k) if (r.cols[k].left != k + 1 || r.cols[k].path_state != tag) return false;
    return true;
}

int failures = 0;
void check(const char *name, bool ok, long want_frees) {
    const bool good = ok && frees == want_frees && bad == 0 && live.empty();
    std::printf("%s: %s frees %ld\n", name, good ? "ok" : "FAILED", frees);
    if (!good) ++failures;
    frees = 0; bad = 0; live.clear();
}

} // namespace

extern "C" void pagan_result_free(pagan_result *r) {
    ++frees;
    if (r->cols && live.erase(r->cols) != 1) ++bad;               // released twice, or never made here
    std::free(r->cols); std::free(r->left_used); std::free(r->right_used);
    r->cols = nullptr; r->left_used = nullptr; r->right_used = nullptr;
    r->n_cols = r->n_left_used = r->n_right_used = 0;
}

int main() {
    using pagan::NodeJob;
    using pagan::OwnedResult;
    bool ok = true;
    {
        OwnedResult o;
        ok = !o.held() && o.get().n_cols == 0 && o.get().cols == nullptr;
        o.adopt(make(5, 1));
        ok = ok && o.held() && readable(o.get(), 5, 1);
    }
    check("adopt, destroy", ok, 1);
    {
        OwnedResult o;
        o.adopt(make(5, 1));
        o.adopt(make(7, 2));
        ok = frees == 1 && o.held() && readable(o.get(), 7, 2);
    }
    check("adopt over a held result", ok, 2);
    {
        OwnedResult o;
        o.adopt(make(5, 1));
        o.reset();
        ok = frees == 1 && !o.held() && o.get().cols == nullptr && o.get().n_cols == 0;
        o.reset();                                                // (nothing held: no call)
        ok = ok && frees == 1;
        o.adopt(make(6, 3));
        ok = ok && readable(o.get(), 6, 3);
    }
    check("reset, adopt", ok, 2);
    {
        std::vector<OwnedResult> v;
        for (int k = 0; k < 40; ++k) { v.emplace_back(); v.back().adopt(make(k + 1, k)); }      // (reallocates several times)
        ok = frees == 0;
        for (int k = 0; k < 40; ++k) ok = ok && v[k].held() && readable(v[k].get(), k + 1, k);
        v.resize(64);                                             // (and once more, with empty ones behind)
        for (int k = 0; k < 40; ++k) ok = ok && readable(v[k].get(), k + 1, k);
        ok = ok && frees == 0 && !v[63].held();
    }
    check("moved by a vector that reallocates", ok, 40);
    {
        OwnedResult a, b;
        a.adopt(make(4, 1));
        b.adopt(make(9, 2));
        a = std::move(b);
        ok = frees == 1 && a.held() && readable(a.get(), 9, 2) && !b.held() && b.get().cols == nullptr;
        OwnedResult &same = a;
        a = std::move(same);                                      // (onto itself: kept)
        ok = ok && frees == 1 && readable(a.get(), 9, 2);
        OwnedResult c(std::move(a));
        ok = ok && frees == 1 && !a.held() && readable(c.get(), 9, 2);
    }
    check("move-assign onto a held result", ok, 2);
    {
        pagan_result e{};                                         // n_cols == 0, null arrays: held all the same, released by one call
        OwnedResult o;
        o.adopt(e);
        ok = o.held() && o.get().n_cols == 0;
        OwnedResult p(std::move(o));
        ok = ok && p.held() && !o.held();
    }
    check("an empty result", ok, 1);
    {
        std::vector<NodeJob> jobs;
        for (int k = 0; k < 40; ++k) {
            jobs.emplace_back();
            NodeJob &j = jobs.back();
            j.upper.assign((size_t)k + 3, k); j.lower.assign((size_t)k + 3, k + 10);
            j.set_band();
            j.res.adopt(make(k + 1, k));
        }
        for (int k = 0; k < 40; ++k) {
            const NodeJob &j = jobs[k];
            const pagan_job jb = j.job(nullptr);
            ok = ok && jb.band == &j.pb && jb.left == &j.gl && jb.right == &j.gr && j.pb.n == k + 3 && j.pb.upper == j.upper.data() &&
                 j.pb.lower == j.lower.data() && j.pb.upper[k + 2] == k && j.pb.lower[0] == k + 10 && readable(j.res.get(), k + 1, k);
        }
        NodeJob moved(std::move(jobs[7]));
        ok = ok && moved.pb.upper == moved.upper.data() && moved.pb.n == 10 && moved.pb.lower[9] == 17 && readable(moved.res.get(), 8, 7);
        ok = ok && jobs[7].band() == nullptr && jobs[7].pb.n == 0 && !jobs[7].res.held();          // (the source: no band, nothing held)
        jobs[3] = std::move(moved);                                // (onto a job that holds a band and a result)
        ok = ok && frees == 1 && jobs[3].pb.upper == jobs[3].upper.data() && jobs[3].pb.n == 10 && readable(jobs[3].res.get(), 8, 7);
        jobs[3].banded = false;                                    // (the retry without the band)
        ok = ok && jobs[3].job(nullptr).band == nullptr;
    }
    check("a NodeJob moved with its band", ok, 40);
    return failures == 0 ? 0 : 1;
}
