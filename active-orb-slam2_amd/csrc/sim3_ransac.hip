// The RANSAC of Sim3Solver (src/Sim3Solver.cc) for a batch of loop candidates on the device (include/aos2.h: aos2_sim3_ransac): the
// call sits between SearchByBoW(KF, KF) and SearchBySim3 of LoopClosing::ComputeSim3 and uses the matcher's handle.  The arithmetic
// is csrc/sim3.h, shared with the host tap.  The random triples are an input, so every hypothesis of every problem is independent: a
// hypothesis is one entry of a flat list (problem, iteration), three kernels follow each other on the handle's stream with one upload
// in front and one fetch behind.
#include <algorithm>
#include <cmath>

#include "matcher_handle.h"
#include "sim3.h"
#include "solver_batch.h"
#include "wave_ops.h"

namespace aos2 {

// mRansacMaxIts (SetRansacParameters, src/Sim3Solver.cc:125-135).  A quotient that is no int (NaN when epsilon > 1, infinite when
// probability is 1 or epsilon^3 vanishes against 1) converts the way the x86 instruction does it for the reference: INT_MIN.
static int32_t sim3_ransac_its(int n, double probability, int min_inliers, int max_iterations)
{
    const float epsilon = (float)min_inliers / n;
    const int nIterations = min_inliers == n ? 1 : x86_int(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3))));
    return std::max(1, std::min(nIterations, max_iterations));
}

int sim3_check(const aos2_sim3_problem_t *problems, const aos2_sim3_result_t *results, int n_problems, int32_t *its, uint8_t *run)
{
    if (int st = solver_check_batch(problems, results, n_problems)) return st;
    for (int p = 0; p < n_problems; ++p) {
        const aos2_sim3_problem_t &P = problems[p];
        if (P.n < 0 || P.max_iterations < 1 || (P.n > 0 && (!P.X3Dc1 || !P.X3Dc2 || !P.max_err1 || !P.max_err2 || !results[p].inliers))) {
            set_error("problem %d: bad argument (n >= 0, max_iterations >= 1, the per-correspondence arrays)", p);
            return AOS2_ERR_ARG;
        }
        its[p] = sim3_ransac_its(P.n, P.probability, P.min_inliers, P.max_iterations);
        run[p] = P.n >= P.min_inliers;
        if (!run[p]) continue;
        if (P.n < 3 || !P.draws) {
            set_error("problem %d: %d correspondences to draw triples from, or no draws", p, P.n);
            return AOS2_ERR_ARG;
        }
        if (int st = solver_check_draws(p, P.draws, P.n, 3, 0, P.max_iterations)) return st;
    }
    return AOS2_OK;
}

void sim3_result_clear(const aos2_sim3_problem_t &P, int32_t its, aos2_sim3_result_t &R)
{
    uint8_t *inl = R.inliers;
    int32_t *counts = R.counts;
    R = aos2_sim3_result_t{};
    R.inliers = inl;
    R.counts = counts;
    R.ransac_max_its = its;
    R.first_success = R.best_iteration = -1;
    if (P.n > 0) memset(inl, 0, (size_t)P.n);
    if (counts) std::fill(counts, counts + P.max_iterations, -1);
}

// one problem with something to run; the pointers are regions of the handle's arena
struct Sim3ProbDev {
    const float *X1, *X2, *e1, *e2;   // [n][3], [n][3], [n], [n]
    const int32_t *draws;             // [its][3]
    int32_t *counts;                  // [its]
    uint8_t *inliers;                 // [n]
    int32_t n, its, hyp_off, fix_scale, min_inliers, pad;
    Sim3Cam K1, K2;
};

struct Sim3ResDev {
    int32_t first_success, best_iteration, best_inliers, pad;
    float T12[16], R12[9], t12[3], s12;
};

// one thread per hypothesis: the triple, Horn's closed form, the first three rows of T12 and T21 (24 floats; the fourth rows are
// constant and the scale is not read by the inlier test)
__global__ __launch_bounds__(64) void sim3_models_kernel(const Sim3ProbDev *__restrict__ probs, const int32_t *__restrict__ hyp_prob, int total,
                                                        float *__restrict__ models)
{
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= total) return;
    const Sim3ProbDev &P = probs[hyp_prob[h]];
    Sim3Model m;
    sim3_model_of(P.n, P.X1, P.X2, P.draws, h - P.hyp_off, P.fix_scale != 0, m);
    float *o = models + 24 * (size_t)h;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        o[k] = m.T12[k];
        o[12 + k] = m.T21[k];
    }
}

// one wave per hypothesis, four per workgroup: the model and the cameras are uniform, the lanes stride over the correspondences 64 at
// a time.  mvP1im1 / mvP2im2 are formed inline from the coordinates the projections read anyway (two divisions per point instead of
// 16 more bytes per point and a kernel of their own).  No atomics: one store per hypothesis, independent of scheduling.
__global__ __launch_bounds__(256) void sim3_inliers_kernel(const Sim3ProbDev *__restrict__ probs, const int32_t *__restrict__ hyp_prob, int total,
                                                          const float *__restrict__ models)
{
    const int h = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (h >= total) return;
    const Sim3ProbDev &P = probs[hyp_prob[h]];
    const float *mp = models + 24 * (size_t)h;
    float T12[12], T21[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        T12[k] = mp[k];
        T21[k] = mp[12 + k];
    }
    const Sim3Cam K1 = P.K1, K2 = P.K2;
    const int n = P.n;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const float X1[3] = {P.X1[3 * (size_t)i], P.X1[3 * (size_t)i + 1], P.X1[3 * (size_t)i + 2]};
            const float X2[3] = {P.X2[3 * (size_t)i], P.X2[3 * (size_t)i + 1], P.X2[3 * (size_t)i + 2]};
            in = sim3_inlier(T12, T21, K1, K2, X1, X2, P.e1[i], P.e2[i]);
        }
        count += __popcll(__ballot(in));
    }
    if (lane == 0) P.counts[h - P.hyp_off] = count;
}

// one workgroup per problem: the literal loop of :183-199 over the counts (one thread; a few hundred integers), then the selected
// hypothesis once more with the same routine -- the same bits, so no [iterations][n] mask is ever stored -- for mvbBestInliers and
// the mBest* members.  Iterations behind the stop are reported as not run.
__global__ __launch_bounds__(256) void sim3_resolve_kernel(const Sim3ProbDev *__restrict__ probs, Sim3ResDev *__restrict__ res)
{
    __shared__ int s_best, s_stop;
    const Sim3ProbDev &P = probs[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) {
        Sim3Scan scan;
        int stop = P.its - 1;
        for (int it = 0; it < P.its; ++it)
            if (scan.step(it, P.counts[it], P.min_inliers)) {
                stop = it;
                break;
            }
        s_best = scan.best_iteration;
        s_stop = stop;
        Sim3ResDev &R = res[blockIdx.x];
        R.first_success = scan.first_success;
        R.best_iteration = scan.best_iteration;
        R.best_inliers = scan.best_inliers;
    }
    __syncthreads();
    const int best = s_best;
    for (int it = s_stop + 1 + tid; it < P.its; it += 256) P.counts[it] = -1;
    if (best < 0) return;   // (its >= 1 and counts >= 0: does not happen)
    Sim3Model m;
    sim3_model_of(P.n, P.X1, P.X2, P.draws, best, P.fix_scale != 0, m);
    const Sim3Cam K1 = P.K1, K2 = P.K2;
    for (int i = tid; i < P.n; i += 256)
        P.inliers[i] = sim3_inlier(m.T12, m.T21, K1, K2, P.X1 + 3 * (size_t)i, P.X2 + 3 * (size_t)i, P.e1[i], P.e2[i]);
    if (tid == 0) {
        Sim3ResDev &R = res[blockIdx.x];
#pragma unroll
        for (int k = 0; k < 12; ++k) R.T12[k] = m.T12[k];
        R.T12[12] = R.T12[13] = R.T12[14] = 0.0f;
        R.T12[15] = 1.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) R.R12[k] = m.R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) R.t12[k] = m.t[k];
        R.s12 = m.s;
    }
}

}  // namespace aos2

extern "C" {

int aos2_sim3_ransac(aos2_matcher_t *m, const aos2_sim3_problem_t *problems, aos2_sim3_result_t *results, int n_problems)
{
    using namespace aos2;
    if (!m) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int32_t its[64];
    uint8_t run[64];
    int st = sim3_check(problems, results, n_problems, its, run);
    if (st || n_problems == 0) return st;
    if ((st = matcher_init(m))) return st;
    // the problems with something to run, and the flat list of their hypotheses
    SolverBatch<Sim3ProbDev, Sim3ResDev> B;
    std::vector<int32_t> hyp_prob;
    for (int p = 0; p < n_problems; ++p) {
        sim3_result_clear(problems[p], its[p], results[p]);
        if (!run[p]) continue;
        const aos2_sim3_problem_t &P = problems[p];
        int32_t hyp_off;
        if ((st = flat_list_append(hyp_prob, (size_t)its[p], B.n, INT32_MAX, "more than 2^31 hypotheses in one call", hyp_off))) return st;
        Sim3ProbDev &D = B.add(p);
        D.n = P.n;
        D.its = its[p];
        D.hyp_off = hyp_off;
        D.fix_scale = P.fix_scale;
        D.min_inliers = P.min_inliers;
        D.K1 = Sim3Cam{P.fx1, P.fy1, P.cx1, P.cy1};
        D.K2 = Sim3Cam{P.fx2, P.fy2, P.cx2, P.cy2};
    }
    const int n_dev = B.n, total = (int)hyp_prob.size();
    if (n_dev == 0) return AOS2_OK;
    Arena A{m};
    for (int d = 0; d < n_dev; ++d) {
        const aos2_sim3_problem_t &P = problems[B.src[d]];
        Sim3ProbDev &D = B.dev[d];
        const size_t n = (size_t)P.n;
        A.in(D.X1, P.X3Dc1, 12 * n);
        A.in(D.X2, P.X3Dc2, 12 * n);
        A.in(D.e1, P.max_err1, 4 * n);
        A.in(D.e2, P.max_err2, 4 * n);
        A.in(D.draws, P.draws, 12 * (size_t)D.its);
        A.out(D.counts, 4 * (size_t)D.its);
        A.out(D.inliers, n);
    }
    float *d_models;
    A.scratch(d_models, 96 * (size_t)total);
    if ((st = B.begin(A, hyp_prob))) return st;
    hipLaunchKernelGGL(sim3_models_kernel, dim3((total + 63) / 64), dim3(64), 0, m->stream, B.d_probs, B.d_hyp, total, d_models);
    hipLaunchKernelGGL(sim3_inliers_kernel, dim3((total + 3) / 4), dim3(256), 0, m->stream, B.d_probs, B.d_hyp, total, d_models);
    hipLaunchKernelGGL(sim3_resolve_kernel, dim3(n_dev), dim3(256), 0, m->stream, B.d_probs, B.d_res);
    for (int d = 0; d < n_dev; ++d) {
        aos2_sim3_result_t &R = results[B.src[d]];
        if (R.counts) A.fetch(R.counts, B.dev[d].counts, 4 * (size_t)B.dev[d].its);
        A.fetch(R.inliers, B.dev[d].inliers, (size_t)B.dev[d].n);
    }
    if ((st = B.end(A))) return st;
    for (int d = 0; d < n_dev; ++d) {
        aos2_sim3_result_t &R = results[B.src[d]];
        const Sim3ResDev &S = B.res[d];
        R.first_success = S.first_success;
        R.best_iteration = S.best_iteration;
        R.best_inliers = S.best_inliers;
        memcpy(R.T12, S.T12, sizeof R.T12);
        memcpy(R.R12, S.R12, sizeof R.R12);
        memcpy(R.t12, S.t12, sizeof R.t12);
        R.s12 = S.s12;
    }
    return AOS2_OK;
}

}  // extern "C"
