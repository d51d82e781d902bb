// The RANSAC of PnPsolver (src/PnPsolver.cc) for a batch of relocalisation candidates on the device (include/aos2.h:
// aos2_pnp_ransac): the call sits between SearchByBoW(KF, F) and PoseOptimization of Tracking::Relocalization and uses the matcher's
// handle.  The arithmetic is csrc/pnp.h, shared with the host tap.  The minimal sets are an input, so every hypothesis of every
// problem is independent, and Refine() is a function of the best set alone: a hypothesis is one entry of a flat list (problem,
// iteration), every iteration (and the carried-in best) owns a Refine() slot that works only when the loop would reach it with a new
// best.  Five kernels follow each other on the handle's stream with one upload in front and one fetch behind; none needs an atomic, a
// spin or another workgroup's result of the same launch.
#include <algorithm>
#include <cmath>

#include "matcher_handle.h"
#include "pnp.h"
#include "solver_batch.h"
#include "wave_ops.h"

namespace aos2 {

int pnp_check(const aos2_pnp_problem_t *problems, const aos2_pnp_result_t *results, int n_problems, uint8_t *run)
{
    if (int st = solver_check_batch(problems, results, n_problems)) return st;
    for (int p = 0; p < n_problems; ++p) {
        const aos2_pnp_problem_t &P = problems[p];
        if (P.n < 0 || P.min_set < 4 || P.min_set > 16 || P.first_iteration < 0 || P.first_iteration > P.n_iterations || P.best_inliers_in < 0 ||
            (P.n > 0 && (!P.P3Dw || !P.P2D || !P.max_err || !results[p].inliers || !results[p].best)) ||
            (P.best_inliers_in > 0 && (!P.best_in || P.n == 0))) {
            set_error("problem %d: bad argument (n >= 0, 4 <= min_set <= 16, 0 <= first_iteration <= n_iterations, the per-correspondence "
                      "arrays, best_in with best_inliers_in > 0)", p);
            return AOS2_ERR_ARG;
        }
        run[p] = P.n >= P.min_inliers && P.first_iteration < P.n_iterations;
        if (!run[p]) continue;
        if (P.n < P.min_set || !P.draws) {
            set_error("problem %d: %d correspondences to draw sets of %d from, or no draws", p, P.n, P.min_set);
            return AOS2_ERR_ARG;
        }
        if (int st = solver_check_draws(p, P.draws, P.n, P.min_set, P.first_iteration, P.n_iterations)) return st;
    }
    return AOS2_OK;
}

void pnp_result_clear(const aos2_pnp_problem_t &P, aos2_pnp_result_t &R)
{
    uint8_t *inl = R.inliers, *best = R.best;
    int32_t *counts = R.counts;
    R = aos2_pnp_result_t{};
    R.inliers = inl;
    R.best = best;
    R.counts = counts;
    R.returned_at = R.best_iteration = -1;
    R.best_inliers = P.best_inliers_in;
    if (P.n > 0) {
        memset(inl, 0, (size_t)P.n);
        if (P.best_inliers_in > 0) memmove(best, P.best_in, (size_t)P.n);
        else memset(best, 0, (size_t)P.n);
    }
    if (counts) std::fill(counts, counts + P.n_iterations, -1);
}

// one problem with something to run; the pointers are regions of the handle's arena.  Iterations are local here: 0 .. its-1 stand for
// first .. n_iterations-1 of the solver; slot k < its is the Refine() of the set of local iteration k, slot its that of the carried set
struct PnpProbDev {
    const float *P3D, *P2D, *max_err;   // [n][3], [n][2], [n]
    const int32_t *draws;               // [its][min_set]
    const uint8_t *best_in;             // [n] (zeros when nothing is carried in)
    int32_t *counts;                    // [its]
    uint8_t *inliers, *best;            // [n], [n]
    uint8_t *slot_flags;                // [its][n]: the set a working slot refines
    int32_t n, its, hyp_off, slot_off, min_inliers, min_set, best_inliers_in, first;
    PnpCam K;
};

struct PnpResDev {
    int32_t returned_at, best_iteration, best_inliers, n_inliers;
    float Tcw[16], best_Tcw[16];
};

// the 12x12 workspace of one lane in LDS, [element][lane]: lane l reads doubles 64 apart, the 64 lanes of an access read 512
// contiguous bytes, so run-time (i, k) indexing costs no bank conflict and no scratch
struct PnpLds {
    double *b;
    __device__ double &At(int i, int k) { return b[(i * 12 + k) * 64]; }
    __device__ double &V(int i, int k) { return b[(144 + i * 12 + k) * 64]; }
    __device__ double &W(int i) { return b[(288 + i) * 64]; }
};

// EPnP of the minimal set, one lane per hypothesis, one wave per workgroup: 300 doubles of LDS per lane are 150 KiB of the CU's 160
__global__ __launch_bounds__(64) void pnp_models_kernel(const PnpProbDev *__restrict__ probs, const int32_t *__restrict__ hyp_prob, int total,
                                                       double *__restrict__ models)
{
    __shared__ double lds[300 * 64];
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= total) return;
    const PnpProbDev &P = probs[hyp_prob[h]];
    PnpLds ws{lds + threadIdx.x};
    const PnpPts pts = {P.P3D, P.P2D, P.max_err};
    double Rt[12];
    pnp_compute_pose(PnpSetDraws{P.n, P.min_set, P.draws + (size_t)P.min_set * (h - P.hyp_off)}, pts, P.K, ws, Rt, Rt + 9);
    double *o = models + 12 * (size_t)h;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = Rt[k];
}

// one wave per hypothesis, four per workgroup: the model is uniform, the lanes stride over the correspondences 64 at a time.  No
// atomics: one store per hypothesis, independent of scheduling.
__global__ __launch_bounds__(256) void pnp_counts_kernel(const PnpProbDev *__restrict__ probs, const int32_t *__restrict__ hyp_prob, int total,
                                                        const double *__restrict__ models)
{
    const int h = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (h >= total) return;
    const PnpProbDev &P = probs[hyp_prob[h]];
    double Rt[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) Rt[k] = models[12 * (size_t)h + k];
    const PnpPts pts = {P.P3D, P.P2D, P.max_err};
    const PnpCam K = P.K;
    const int n = P.n;
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n && pnp_inlier(Rt, K, pts, i);
        count += __popcll(__ballot(in));
    }
    if (lane == 0) P.counts[h - P.hyp_off] = count;
}

// one thread per problem: the slots whose Refine() the loop can reach -- an iteration with count >= min_inliers that beats every
// earlier one and the carried count, and the carried set when such an iteration arrives before any of those
__global__ void pnp_mark_kernel(const PnpProbDev *__restrict__ probs, int n_dev, uint8_t *__restrict__ work)
{
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d >= n_dev) return;
    const PnpProbDev &P = probs[d];
    PnpScan scan(P.best_inliers_in);
    for (int it = 0; it < P.its; ++it) {
        const int before = scan.best_iteration;
        if (!scan.step(it, P.counts[it], P.min_inliers)) continue;
        if (scan.best_iteration != before) work[P.slot_off + it] = 1;
        else if (scan.best_iteration < 0) work[P.slot_off + P.its] = 1;
    }
}

// inliers of a model over all correspondences by the 256 threads of a workgroup (flags, when given, receive them) -> every thread
__device__ inline int pnp_block_count(const double *Rt, const PnpCam &K, const PnpPts &pts, int n, uint8_t *flags, int32_t *s_wave)
{
    const int tid = threadIdx.x;
    int count = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const bool in = i < n && pnp_inlier(Rt, K, pts, i);
        if (flags && i < n) flags[i] = in;
        count += __popcll(__ballot(in));
    }
    return block_sum_waves_i32<256>(count, s_wave);
}

// Refine() (:260-305), one workgroup per slot; it leaves at once unless the slot is marked.  The set is the hypothesis' flags,
// recomputed from its stored model (the same bits as the count came from), or the carried flags.  Thread 0 runs the serial parts of
// the same pnp_compute_pose; the 144 entries of M'M, each a sum over the set in index order, get a thread each.
__global__ __launch_bounds__(256) void pnp_refine_kernel(const PnpProbDev *__restrict__ probs, const int32_t *__restrict__ slot_prob,
                                                        const uint8_t *__restrict__ work, const double *__restrict__ models,
                                                        double *__restrict__ ref_models, int32_t *__restrict__ ref_counts)
{
    __shared__ PnpLocal<12, 12> ws;
    __shared__ PnpGeo G;
    __shared__ double Rr[12];
    __shared__ int32_t s_wave[4];
    const int slot = blockIdx.x, tid = threadIdx.x;
    if (!work[slot]) return;
    const PnpProbDev &P = probs[slot_prob[slot]];
    const int k = slot - P.slot_off;
    const PnpPts pts = {P.P3D, P.P2D, P.max_err};
    const PnpCam K = P.K;
    const uint8_t *flags = P.best_in;
    if (k < P.its) {
        uint8_t *mine = P.slot_flags + (size_t)k * P.n;
        pnp_block_count(models + 12 * (size_t)(P.hyp_off + k), K, pts, P.n, mine, s_wave);
        flags = mine;
    }
    const PnpSetFlags S{P.n, flags};
    if (tid == 0) pnp_geometry(S, pts, G);
    __syncthreads();
    if (tid < 144) ws.at[tid / 12][tid % 12] = pnp_mtm_entry(S, pts, K, G, tid / 12, tid % 12);
    __syncthreads();
    if (tid == 0) pnp_solve(S, pts, K, G, ws, Rr, Rr + 9);
    __syncthreads();
    const int count = pnp_block_count(Rr, K, pts, P.n, nullptr, s_wave);
    if (tid < 12) ref_models[12 * (size_t)slot + tid] = Rr[tid];
    if (tid == 0) ref_counts[slot] = count;
}

// one workgroup per problem: the literal loop of :182-239 over the counts and the slots' results (one thread), then the flags of the
// refined pose and of the best hypothesis once more through pnp_inlier, the float poses, and -1 for the iterations behind the stop
__global__ __launch_bounds__(256) void pnp_resolve_kernel(const PnpProbDev *__restrict__ probs, const double *__restrict__ models,
                                                         const double *__restrict__ ref_models, const int32_t *__restrict__ ref_counts,
                                                         PnpResDev *__restrict__ res)
{
    __shared__ int s_best, s_stop, s_slot;
    const PnpProbDev &P = probs[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) {
        PnpScan scan(P.best_inliers_in);
        int stop = P.its - 1, ret_slot = -1;
        for (int it = 0; it < P.its; ++it) {
            if (!scan.step(it, P.counts[it], P.min_inliers)) continue;
            const int slot = P.slot_off + (scan.best_iteration < 0 ? P.its : scan.best_iteration);
            if (scan.refined(it, ref_counts[slot], P.min_inliers)) {
                stop = it;
                ret_slot = slot;
                break;
            }
        }
        s_best = scan.best_iteration;
        s_stop = stop;
        s_slot = ret_slot;
        PnpResDev &R = res[blockIdx.x];
        R.returned_at = scan.returned_at < 0 ? -1 : P.first + scan.returned_at;
        R.best_iteration = scan.best_iteration < 0 ? -1 : P.first + scan.best_iteration;
        R.best_inliers = scan.best_inliers;
        if (ret_slot >= 0) {
            R.n_inliers = ref_counts[ret_slot];
            pnp_Tcw(ref_models + 12 * (size_t)ret_slot, R.Tcw);
        }
        if (scan.best_iteration >= 0) pnp_Tcw(models + 12 * (size_t)(P.hyp_off + scan.best_iteration), R.best_Tcw);
    }
    __syncthreads();
    const int best = s_best, slot = s_slot;
    for (int it = s_stop + 1 + tid; it < P.its; it += 256) P.counts[it] = -1;
    const PnpPts pts = {P.P3D, P.P2D, P.max_err};
    const PnpCam K = P.K;
    for (int i = tid; i < P.n; i += 256) {
        P.best[i] = best >= 0 ? pnp_inlier(models + 12 * (size_t)(P.hyp_off + best), K, pts, i) : P.best_in[i];
        if (slot >= 0) P.inliers[i] = pnp_inlier(ref_models + 12 * (size_t)slot, K, pts, i);
    }
}

}  // namespace aos2

extern "C" {

int aos2_pnp_ransac_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                               int32_t *ransac_min_inliers, float *ransac_epsilon, int32_t *ransac_max_its)
{
    using namespace aos2;
    if (n < 0 || !ransac_min_inliers || !ransac_epsilon || !ransac_max_its) {
        set_error("bad argument (n >= 0, the three outputs)");
        return AOS2_ERR_ARG;
    }
    int nMinInliers = x86_int((double)((float)n * epsilon));   // int = N * mRansacEpsilon, a float product (:134)
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    if (epsilon < (float)nMinInliers / n) epsilon = (float)nMinInliers / n;
    int nIterations;
    if (nMinInliers == n) nIterations = 1;
    else nIterations = x86_int(ceil(log(1 - probability) / log(1 - pow((double)epsilon, 3))));
    *ransac_min_inliers = nMinInliers;
    *ransac_epsilon = epsilon;
    *ransac_max_its = std::max(1, std::min(nIterations, max_iterations));
    return AOS2_OK;
}

int aos2_pnp_ransac(aos2_matcher_t *m, const aos2_pnp_problem_t *problems, aos2_pnp_result_t *results, int n_problems)
{
    using namespace aos2;
    if (!m) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    uint8_t run[64];
    int st = pnp_check(problems, results, n_problems, run);
    if (st || n_problems == 0) return st;
    if ((st = matcher_init(m))) return st;
    // the problems with something to run, the flat list of their hypotheses and that of their Refine() slots
    SolverBatch<PnpProbDev, PnpResDev> B;
    std::vector<int32_t> hyp_prob, slot_prob;
    for (int p = 0; p < n_problems; ++p) {
        pnp_result_clear(problems[p], results[p]);
        if (!run[p]) continue;
        const aos2_pnp_problem_t &P = problems[p];
        const size_t its = (size_t)(P.n_iterations - P.first_iteration), limit = (size_t)INT32_MAX / 16;
        const char *what = "more than 2^27 hypotheses in one call";
        int32_t hyp_off, slot_off;
        if ((st = flat_list_append(slot_prob, its + 1, B.n, limit, what, slot_off))) return st;
        if ((st = flat_list_append(hyp_prob, its, B.n, limit, what, hyp_off))) return st;
        PnpProbDev &D = B.add(p);
        D.n = P.n;
        D.its = (int32_t)its;
        D.first = P.first_iteration;
        D.hyp_off = hyp_off;
        D.slot_off = slot_off;
        D.min_inliers = P.min_inliers;
        D.min_set = P.min_set;
        D.best_inliers_in = P.best_inliers_in;
        D.K = PnpCam{P.fx, P.fy, P.cx, P.cy};
    }
    const int n_dev = B.n, total = (int)hyp_prob.size(), slots = (int)slot_prob.size();
    if (n_dev == 0) return AOS2_OK;
    Arena A{m};
    for (int d = 0; d < n_dev; ++d) {
        const aos2_pnp_problem_t &P = problems[B.src[d]];
        PnpProbDev &D = B.dev[d];
        const size_t n = (size_t)P.n, its = (size_t)D.its;
        A.in(D.P3D, P.P3Dw, 12 * n);
        A.in(D.P2D, P.P2D, 8 * n);
        A.in(D.max_err, P.max_err, 4 * n);
        A.in(D.draws, P.draws + (size_t)P.min_set * P.first_iteration, 4 * (size_t)P.min_set * its);
        A.in(D.best_in, P.best_inliers_in > 0 ? P.best_in : (const uint8_t *)nullptr, n);   // (no source: zeros)
        A.scratch(D.slot_flags, its * n);
        A.out(D.counts, 4 * its);
        A.out(D.inliers, n);
        A.out(D.best, n);
    }
    const int32_t *d_slot;
    double *d_models, *d_ref_models;
    int32_t *d_ref_counts;
    uint8_t *d_work;
    A.in(d_slot, slot_prob.data(), 4 * (size_t)slots);
    A.scratch(d_models, 96 * (size_t)total);
    A.scratch(d_ref_models, 96 * (size_t)slots);
    A.scratch(d_ref_counts, 4 * (size_t)slots);
    A.scratch(d_work, (size_t)slots);
    if ((st = B.begin(A, hyp_prob))) return st;
    hipLaunchKernelGGL(pnp_models_kernel, dim3((total + 63) / 64), dim3(64), 0, m->stream, B.d_probs, B.d_hyp, total, d_models);
    hipLaunchKernelGGL(pnp_counts_kernel, dim3((total + 3) / 4), dim3(256), 0, m->stream, B.d_probs, B.d_hyp, total, d_models);
    hipLaunchKernelGGL(pnp_mark_kernel, dim3(1), dim3(64), 0, m->stream, B.d_probs, n_dev, d_work);
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(slots), dim3(256), 0, m->stream, B.d_probs, d_slot, d_work, d_models, d_ref_models, d_ref_counts);
    hipLaunchKernelGGL(pnp_resolve_kernel, dim3(n_dev), dim3(256), 0, m->stream, B.d_probs, d_models, d_ref_models, d_ref_counts, B.d_res);
    for (int d = 0; d < n_dev; ++d) {
        const aos2_pnp_problem_t &P = problems[B.src[d]];
        aos2_pnp_result_t &R = results[B.src[d]];
        if (R.counts) A.fetch(R.counts + P.first_iteration, B.dev[d].counts, 4 * (size_t)B.dev[d].its);
        A.fetch(R.inliers, B.dev[d].inliers, (size_t)B.dev[d].n);
        A.fetch(R.best, B.dev[d].best, (size_t)B.dev[d].n);
    }
    if ((st = B.end(A))) return st;
    for (int d = 0; d < n_dev; ++d) {
        aos2_pnp_result_t &R = results[B.src[d]];
        const PnpResDev &S = B.res[d];
        R.returned_at = S.returned_at;
        R.best_iteration = S.best_iteration;
        R.best_inliers = S.best_inliers;
        R.n_inliers = S.n_inliers;
        memcpy(R.Tcw, S.Tcw, sizeof R.Tcw);
        memcpy(R.best_Tcw, S.best_Tcw, sizeof R.best_Tcw);
    }
    return AOS2_OK;
}

}  // extern "C"
