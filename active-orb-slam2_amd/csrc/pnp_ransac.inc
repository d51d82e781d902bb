// The RANSAC of PnPsolver (src/PnPsolver.cc) for a batch of relocalisation candidates on the device (include/aos2.h:
// aos2_pnp_ransac), part of matcher.hip's translation unit: the call sits between SearchByBoW(KF, F) and PoseOptimization of
// Tracking::Relocalization and uses the same handle.  The arithmetic is csrc/pnp.h, shared with the host tap.  The minimal sets are
// an input, so every hypothesis of every problem is independent, and Refine() is a function of the best set alone: a hypothesis is
// one entry of a flat list (problem, iteration), every iteration (and the carried-in best) owns a Refine() slot that works only when
// the loop would reach it with a new best.  Five kernels follow each other on the handle's stream with one upload in front and one
// fetch behind; none needs an atomic, a spin or another workgroup's result of the same launch.
#include "pnp.h"

namespace aos2 {

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
    __syncthreads();
    if ((tid & 63) == 0) s_wave[tid >> 6] = count;
    __syncthreads();
    return s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
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
    std::vector<PnpProbDev> dev;
    std::vector<int> src;
    std::vector<int32_t> hyp_prob, slot_prob;
    dev.reserve((size_t)n_problems);
    for (int p = 0; p < n_problems; ++p) {
        pnp_result_clear(problems[p], results[p]);
        if (!run[p]) continue;
        const aos2_pnp_problem_t &P = problems[p];
        PnpProbDev D = {};
        D.n = P.n;
        D.its = P.n_iterations - P.first_iteration;
        D.first = P.first_iteration;
        D.hyp_off = (int32_t)hyp_prob.size();
        D.slot_off = (int32_t)slot_prob.size();
        D.min_inliers = P.min_inliers;
        D.min_set = P.min_set;
        D.best_inliers_in = P.best_inliers_in;
        D.K = PnpCam{P.fx, P.fy, P.cx, P.cy};
        if (slot_prob.size() + (size_t)D.its + 1 > (size_t)INT32_MAX / 16) {
            set_error("more than 2^27 hypotheses in one call");
            return AOS2_ERR_CAPACITY;
        }
        hyp_prob.insert(hyp_prob.end(), (size_t)D.its, (int32_t)dev.size());
        slot_prob.insert(slot_prob.end(), (size_t)D.its + 1, (int32_t)dev.size());
        dev.push_back(D);
        src.push_back(p);
    }
    const int n_dev = (int)dev.size(), total = (int)hyp_prob.size(), slots = (int)slot_prob.size();
    if (n_dev == 0) return AOS2_OK;
    Arena A{m};
    for (int d = 0; d < n_dev; ++d) {   // (dev is sized: its fields stay where they are)
        const aos2_pnp_problem_t &P = problems[src[d]];
        const size_t n = (size_t)P.n, its = (size_t)dev[d].its;
        A.in(dev[d].P3D, P.P3Dw, 12 * n);
        A.in(dev[d].P2D, P.P2D, 8 * n);
        A.in(dev[d].max_err, P.max_err, 4 * n);
        A.in(dev[d].draws, P.draws + (size_t)P.min_set * P.first_iteration, 4 * (size_t)P.min_set * its);
        A.in(dev[d].best_in, P.best_inliers_in > 0 ? P.best_in : (const uint8_t *)nullptr, n);   // (no source: zeros)
        A.scratch(dev[d].slot_flags, its * n);
        A.out(dev[d].counts, 4 * its);
        A.out(dev[d].inliers, n);
        A.out(dev[d].best, n);
    }
    const int32_t *d_hyp, *d_slot;
    const PnpProbDev *d_probs;
    double *d_models, *d_ref_models;
    int32_t *d_ref_counts;
    uint8_t *d_work;
    PnpResDev *d_res;
    A.in(d_hyp, hyp_prob.data(), 4 * (size_t)total);
    A.in(d_slot, slot_prob.data(), 4 * (size_t)slots);
    A.hole(d_probs, sizeof(PnpProbDev) * (size_t)n_dev);
    A.scratch(d_models, 96 * (size_t)total);
    A.scratch(d_ref_models, 96 * (size_t)slots);
    A.scratch(d_ref_counts, 4 * (size_t)slots);
    A.scratch(d_work, (size_t)slots);
    A.out(d_res, sizeof(PnpResDev) * (size_t)n_dev);
    if ((st = A.alloc())) return st;
    A.fill_hole(d_probs, dev.data(), sizeof(PnpProbDev) * (size_t)n_dev);
    if ((st = A.upload())) return st;
    if ((st = A.begin())) return st;
    hipLaunchKernelGGL(pnp_models_kernel, dim3((total + 63) / 64), dim3(64), 0, m->stream, d_probs, d_hyp, total, d_models);
    hipLaunchKernelGGL(pnp_counts_kernel, dim3((total + 3) / 4), dim3(256), 0, m->stream, d_probs, d_hyp, total, d_models);
    hipLaunchKernelGGL(pnp_mark_kernel, dim3(1), dim3(64), 0, m->stream, d_probs, n_dev, d_work);
    hipLaunchKernelGGL(pnp_refine_kernel, dim3(slots), dim3(256), 0, m->stream, d_probs, d_slot, d_work, d_models, d_ref_models, d_ref_counts);
    hipLaunchKernelGGL(pnp_resolve_kernel, dim3(n_dev), dim3(256), 0, m->stream, d_probs, d_models, d_ref_models, d_ref_counts, d_res);
    std::vector<PnpResDev> res((size_t)n_dev);
    A.fetch(res.data(), d_res, sizeof(PnpResDev) * (size_t)n_dev);
    for (int d = 0; d < n_dev; ++d) {
        const aos2_pnp_problem_t &P = problems[src[d]];
        aos2_pnp_result_t &R = results[src[d]];
        if (R.counts) A.fetch(R.counts + P.first_iteration, dev[d].counts, 4 * (size_t)dev[d].its);
        A.fetch(R.inliers, dev[d].inliers, (size_t)dev[d].n);
        A.fetch(R.best, dev[d].best, (size_t)dev[d].n);
    }
    if ((st = A.end())) return st;
    for (int d = 0; d < n_dev; ++d) {
        aos2_pnp_result_t &R = results[src[d]];
        const PnpResDev &S = res[d];
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
