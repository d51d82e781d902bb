// What the host sides of the batched RANSAC solvers (sim3_ransac.hip, pnp_ransac.hip, initializer_ransac.hip) share: the checks a
// batch starts with, the flat list that spreads its hypotheses over one grid, its records on their way through the arena.  Host only.
#pragma once
#include <vector>

#include "matcher_handle.h"

namespace aos2 {

constexpr int kSolverMaxProblems = 64;

inline int solver_check_batch(const void *problems, const void *results, int n_problems)
{
    if (n_problems < 0 || n_problems > kSolverMaxProblems || (n_problems > 0 && (!problems || !results))) {
        set_error("bad argument (0..64 problems and their results)");
        return AOS2_ERR_ARG;
    }
    return AOS2_OK;
}

// iterations [first, last) of problem p, `width` draws each: draw i of a set picks among the n - i correspondences that are left
inline int solver_check_draws(int p, const int32_t *draws, int n, int width, int first, int last)
{
    for (int k = first; k < last; ++k)
        for (int i = 0; i < width; ++i) {
            const int32_t r = draws[(size_t)width * k + i];
            if (r < 0 || r > n - 1 - i) {
                set_error("problem %d: draw %d of iteration %d is %d, outside [0, %d]", p, i, k, r, n - 1 - i);
                return AOS2_ERR_ARG;
            }
        }
    return AOS2_OK;
}

// a double on its way into an int the way the x86 conversion does it for the reference: INT_MIN where it does not fit
inline int32_t x86_int(double v) { return (v > -2147483649.0 && v < 2147483648.0) ? (int32_t)v : INT32_MIN; }

// `count` more entries that name `owner` in a flat list of work items -> off, where they start; a list beyond `limit` entries (what
// the kernels' 32-bit offsets into the per-entry scratch allow) is AOS2_ERR_CAPACITY with the message `what`
inline int flat_list_append(std::vector<int32_t> &list, size_t count, int32_t owner, size_t limit, const char *what, int32_t &off)
{
    if (list.size() + count > limit) {
        set_error("%s", what);
        return AOS2_ERR_CAPACITY;
    }
    off = (int32_t)list.size();
    list.insert(list.end(), count, owner);
    return AOS2_OK;
}

// The problems of a batch that have something to run.  The arena registers the pointer fields of a ProbDev by address, so the
// records stand in a fixed array (a batch has at most kSolverMaxProblems) and the batch is not copied.
template <class ProbDev, class ResDev>
struct SolverBatch {
    ProbDev dev[kSolverMaxProblems];
    ResDev res[kSolverMaxProblems];   // after end(): what the kernels left for dev[d]
    int src[kSolverMaxProblems];      // dev[d] is problems[src[d]]
    int n = 0;
    const int32_t *d_hyp;             // on the device: the flat list, dev[0 .. n), res[0 .. n)
    const ProbDev *d_probs;
    ResDev *d_res;
    SolverBatch() = default;
    SolverBatch(const SolverBatch &) = delete;
    ProbDev &add(int source)
    {
        src[n] = source;
        return dev[n++] = ProbDev{};
    }
    // behind the caller's own arrays: the list, the records and the results; the upload; the start of the call's timed bracket
    int begin(Arena &A, const std::vector<int32_t> &hyp)
    {
        A.in(d_hyp, hyp.data(), 4 * hyp.size());
        A.hole(d_probs, sizeof(ProbDev) * (size_t)n);
        A.out(d_res, sizeof(ResDev) * (size_t)n);
        if (int st = A.alloc()) return st;
        A.fill_hole(d_probs, dev, sizeof(ProbDev) * (size_t)n);
        if (int st = A.upload()) return st;
        return A.begin();
    }
    // behind the launches and the caller's own fetches: res and everything fetched arrive
    int end(Arena &A)
    {
        A.fetch(res, d_res, sizeof(ResDev) * (size_t)n);
        return A.end();
    }
};

}  // namespace aos2
