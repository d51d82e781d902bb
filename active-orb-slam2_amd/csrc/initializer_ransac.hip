// Initializer::Initialize (src/Initializer.cc) for a batch of monocular sequences on the device (include/aos2.h:
// aos2_initializer_initialize): the call sits behind SearchForInitialization of Tracking::MonocularInitialization and uses the
// matcher's handle.  The arithmetic is csrc/initializer.h, shared with the host tap.  The minimal sets are an input, so every
// (problem, iteration, H or F) is one entry of a flat list.  Seven kernels follow each other on the handle's stream with one upload
// in front and one fetch behind: prepare (Normalize), models, scores, pick (+ the winner's flags), hypotheses, CheckRT, decide (+ the
// scatter of the chosen reconstruction).  None needs an atomic, a spin or another workgroup's result of the same launch, and the
// host does not wait between them.
#include "matcher_handle.h"
#include "initializer.h"
#include "solver_batch.h"
#include "wave_ops.h"

namespace aos2 {

int initializer_check(const aos2_initializer_problem_t *problems, const aos2_initializer_result_t *results, int n_problems)
{
    if (int st = solver_check_batch(problems, results, n_problems)) return st;
    for (int p = 0; p < n_problems; ++p) {
        const aos2_initializer_problem_t &P = problems[p];
        const aos2_initializer_result_t &R = results[p];
        if (P.n_keys1 < 1 || P.n_keys2 < 1 || !P.keys1 || !P.keys2 || P.n_matches < 8 || !P.matches || P.iterations < 1 || !P.sets ||
            !(P.sigma > 0) || !R.inliers_h || !R.inliers_f || !R.P3D || !R.triangulated) {
            set_error("problem %d: bad argument (the keys of both frames, n_matches >= 8, iterations >= 1 with their sets, sigma > 0, the four "
                      "result arrays)", p);
            return AOS2_ERR_ARG;
        }
        for (int i = 0; i < P.n_matches; ++i) {
            const int32_t a = P.matches[2 * i], b = P.matches[2 * i + 1];
            if (a < 0 || a >= P.n_keys1 || b < 0 || b >= P.n_keys2) {
                set_error("problem %d: match %d is (%d, %d), outside the frames' %d and %d keys", p, i, a, b, P.n_keys1, P.n_keys2);
                return AOS2_ERR_ARG;
            }
        }
        for (size_t k = 0; k < (size_t)P.iterations * 8; ++k)
            if (P.sets[k] < 0 || P.sets[k] >= P.n_matches) {
                set_error("problem %d: entry %d of set %d is %d, outside [0, %d)", p, (int)(k % 8), (int)(k / 8), P.sets[k], P.n_matches);
                return AOS2_ERR_ARG;
            }
    }
    return AOS2_OK;
}

void initializer_result_clear(const aos2_initializer_problem_t &P, aos2_initializer_result_t &R)
{
    uint8_t *ih = R.inliers_h, *jf = R.inliers_f, *tri = R.triangulated;
    float *p3d = R.P3D;
    R = aos2_initializer_result_t{};
    R.inliers_h = ih;
    R.inliers_f = jf;
    R.P3D = p3d;
    R.triangulated = tri;
    R.best_iteration_h = R.best_iteration_f = -1;
    memset(ih, 0, (size_t)P.n_matches);
    memset(jf, 0, (size_t)P.n_matches);
    memset(p3d, 0, 12 * (size_t)P.n_keys1);
    memset(tri, 0, (size_t)P.n_keys1);
}

// one problem; the pointers are regions of the handle's arena.  Entry k of the flat list of a problem: k < its is the homography of
// iteration k, k >= its the fundamental matrix of iteration k - its.
struct InitProbDev {
    const float *keys1, *keys2;      // [n_keys][2]
    const int32_t *matches, *sets;   // [n_matches][2], [its][8]
    const int32_t *next_same;        // [n_matches]: the next match with the same first key, -1 without one
    float *nrm;                      // [8]: (meanX, sX, meanY, sY) of frame 1 | frame 2
    float *models, *scores;          // [2 its][18], [2 its]
    uint8_t *inl;                    // [2][n_matches]: inliers_h | inliers_f
    float *hyp;                      // [72 + 24]: R of the 8 hypotheses | t
    float *cosv, *p3d;               // [8][n_matches], [8][n_matches][3]: CheckRT per hypothesis and match
    uint8_t *code;                   // [8][n_matches]: INIT_RT_* (0 for a match that is no inlier)
    float *P3D;                      // [n_keys1][3]
    uint8_t *tri;                    // [n_keys1]
    int32_t n_keys1, n_keys2, n_matches, its, hyp_off, min_triangulated;
    float sigma, min_parallax;
    InitCam cam;
};

struct InitResDev {
    int32_t status, initialized, used_homography, best_h, best_f, n_hypotheses, n_inl[2], n_good[8];
    float SH, SF, H21[9], F21[9], R21[9], t21[3], parallax[8];
};

// a lane's Jacobi workspace in LDS, [element][lane]: run-time (i, k) indexing costs no bank conflict and no scratch
template <int RS, int VO, int VS>
struct InitLdsT {
    float *f;
    double *w;
    __device__ float &A(int i, int k) { return f[(i * RS + k) * 64]; }
    __device__ float &V(int i, int k) { return f[(VO + i * VS + k) * 64]; }
    __device__ double &W(int i) { return w[i * 64]; }
};

// Normalize: the two dependent float chains of one axis of one frame (mean, then mean deviation) per lane, four lanes per problem
__global__ __launch_bounds__(64) void init_prepare_kernel(const InitProbDev *__restrict__ probs, int n_dev)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= 4 * n_dev) return;
    const InitProbDev &P = probs[g >> 2];
    const int frame = (g >> 1) & 1, axis = g & 1;
    float *o = P.nrm + 4 * frame + 2 * axis;
    init_normalize_axis(frame ? P.keys2 : P.keys1, frame ? P.n_keys2 : P.n_keys1, axis, o, o + 1);
}

// ComputeH21 / ComputeF21 and the denormalisation, one lane per entry, one wave per workgroup: 225 floats and 9 doubles per lane
__global__ __launch_bounds__(64) void init_models_kernel(const InitProbDev *__restrict__ probs, const int32_t *__restrict__ hyp_prob, int total)
{
    __shared__ float ldsf[225 * 64];
    __shared__ double ldsw[9 * 64];
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= total) return;
    const InitProbDev &P = probs[hyp_prob[h]];
    const int k = h - P.hyp_off;
    InitLdsT<16, 144, 9> ws{ldsf + threadIdx.x, ldsw + threadIdx.x};
    const InitPts pts = {P.keys1, P.keys2, P.matches, P.nrm, P.nrm + 4};
    float M[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) M[j] = 0.0f;
    if (k < P.its) init_model_h(pts, P.sets + 8 * (size_t)k, ws, M, M + 9);
    else init_model_f(pts, P.sets + 8 * (size_t)(k - P.its), ws, M);
    float *o = P.models + 18 * (size_t)k;
#pragma unroll
    for (int j = 0; j < 18; ++j) o[j] = M[j];
}

// CheckHomography / CheckFundamental: one wave per entry, four per workgroup.  The lanes evaluate the two addends of 64 matches,
// then the ONE float chain of the entry takes them in match order (lane 0's two, lane 1's two, ...): the sequential sum, bit for bit
__global__ __launch_bounds__(256) void init_scores_kernel(const InitProbDev *__restrict__ probs, const int32_t *__restrict__ hyp_prob, int total)
{
    const int h = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
    if (h >= total) return;
    const InitProbDev &P = probs[hyp_prob[h]];
    const int k = h - P.hyp_off;
    const bool is_h = k < P.its;
    float M[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) M[j] = P.models[18 * (size_t)k + j];
    const InitPts pts = {P.keys1, P.keys2, P.matches, P.nrm, P.nrm + 4};
    const float invS = init_inv_sigma2(P.sigma);
    const int n = P.n_matches;
    float s = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        float a = 0.0f, b = 0.0f;
        if (i < n) init_terms(is_h, M, invS, pts, i, a, b);
#pragma unroll
        for (int l = 0; l < 64; ++l) {
            s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(a), l));
            s += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b), l));
        }
    }
    if (lane == 0) P.scores[k] = s;
}

// one workgroup per (problem, model): the pick over the scores (one thread), then the winner's inlier flags and their count
__global__ __launch_bounds__(256) void init_pick_kernel(const InitProbDev *__restrict__ probs, InitResDev *__restrict__ res)
{
    __shared__ int s_best;
    __shared__ int32_t s_wave[4];
    const InitProbDev &P = probs[blockIdx.x];
    InitResDev &R = res[blockIdx.x];
    const int model = blockIdx.y, tid = threadIdx.x;
    const bool is_h = model == 0;
    if (tid == 0) {
        float score;
        const int best = init_pick(P.scores + (size_t)model * P.its, P.its, &score);
        s_best = best;
        (is_h ? R.SH : R.SF) = score;
        (is_h ? R.best_h : R.best_f) = best;
        if (best >= 0) {
            const float *M = P.models + 18 * ((size_t)model * P.its + best);
            float *o = is_h ? R.H21 : R.F21;
            for (int j = 0; j < 9; ++j) o[j] = M[j];
        }
    }
    __syncthreads();
    const int best = s_best;
    if (best < 0) return;
    float M[18];
#pragma unroll
    for (int j = 0; j < 18; ++j) M[j] = P.models[18 * ((size_t)model * P.its + best) + j];
    const InitPts pts = {P.keys1, P.keys2, P.matches, P.nrm, P.nrm + 4};
    const float invS = init_inv_sigma2(P.sigma);
    int count = 0;
    for (int base = 0; base < P.n_matches; base += 256) {
        const int i = base + tid;
        float a, b;
        const bool in = i < P.n_matches && init_terms(is_h, M, invS, pts, i, a, b);
        if (i < P.n_matches) P.inl[(size_t)model * P.n_matches + i] = in;
        count += __popcll(__ballot(in));
    }
    const int n_inl = block_sum_waves_i32<256>(count, s_wave);
    if (tid == 0) R.n_inl[model] = n_inl;
}

// one lane per problem: RH and the branch of :112-118, the 3x3 decompositions, the 4 or 8 (R, t)
__global__ __launch_bounds__(64) void init_hyps_kernel(const InitProbDev *__restrict__ probs, InitResDev *__restrict__ res, int n_dev)
{
    __shared__ float ldsf[18 * 64];
    __shared__ double ldsw[3 * 64];
    const int d = blockIdx.x * 64 + threadIdx.x;
    if (d >= n_dev) return;
    const InitProbDev &P = probs[d];
    InitResDev &R = res[d];
    InitLdsT<3, 9, 3> ws{ldsf + threadIdx.x, ldsw + threadIdx.x};
    const float RH = R.SH / (R.SH + R.SF);
    const bool use_h = (double)RH > 0.40;
    R.used_homography = use_h;
    if ((use_h ? R.best_h : R.best_f) < 0) {
        R.status = AOS2_INIT_NO_MODEL;
        return;
    }
    if (use_h) R.n_hypotheses = init_hyps_h(R.H21, P.cam, ws, P.hyp, P.hyp + 72) ? 8 : 0;
    else {
        init_hyps_f(R.F21, P.cam, ws, P.hyp, P.hyp + 72);
        R.n_hypotheses = 4;
    }
}

// CheckRT, one workgroup per (problem, hypothesis): every inlier match in parallel, nGood an integer sum, the parallax the order
// statistic min(50, nGood - 1) of the cosines, found bit by bit on their keys (no sort order to reproduce)
__global__ __launch_bounds__(256) void init_checkrt_kernel(const InitProbDev *__restrict__ probs, InitResDev *__restrict__ res)
{
    __shared__ int32_t s_wave[4];
    const InitProbDev &P = probs[blockIdx.x];
    InitResDev &R = res[blockIdx.x];
    const int h = blockIdx.y, tid = threadIdx.x, n = P.n_matches;
    if (h >= R.n_hypotheses) return;
    const uint8_t *inl = P.inl + (R.used_homography ? 0 : (size_t)n);
    InitRT S;
    init_rt_setup(P.hyp + 9 * h, P.hyp + 72 + 3 * h, P.cam, S);
    const float th2 = init_th2(P.sigma);
    float *cosv = P.cosv + (size_t)h * n, *p3d = P.p3d + 3 * (size_t)h * n;
    uint8_t *code = P.code + (size_t)h * n;
    int good = 0;
    for (int i = tid; i < n; i += 256) {
        if (!inl[i]) continue;
        const int k1 = P.matches[2 * i], k2 = P.matches[2 * i + 1];
        float x[3], c = 0;
        const int cd = init_rt_point(S, P.cam, th2, P.keys1[2 * k1], P.keys1[2 * k1 + 1], P.keys2[2 * k2], P.keys2[2 * k2 + 1], x, &c);
        code[i] = (uint8_t)cd;
        if (cd & INIT_RT_GOOD) {
            cosv[i] = c;
            p3d[3 * i] = x[0];
            p3d[3 * i + 1] = x[1];
            p3d[3 * i + 2] = x[2];
            ++good;
        }
    }
    const int nGood = block_sum_i32<256>(good, s_wave);   // (its barriers also publish code / cosv to the workgroup)
    float parallax = 0;
    if (nGood > 0) {
        const int want = (nGood - 1 < 50 ? nGood - 1 : 50) + 1;   // the smallest key with at least `want` keys <= it
        uint32_t prefix = 0;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t cand = prefix | ((1u << bit) - 1u);
            int c = 0;
            for (int i = tid; i < n; i += 256)
                if ((code[i] & INIT_RT_GOOD) && init_float_key(cosv[i]) <= cand) ++c;
            if (block_sum_i32<256>(c, s_wave) < want) prefix |= 1u << bit;
        }
        parallax = init_parallax_deg(init_key_float(prefix));
    }
    if (tid == 0) {
        R.n_good[h] = nGood;
        R.parallax[h] = parallax;
    }
}

// one workgroup per problem: the decision (one thread), then the chosen hypothesis' points and flags go to the first frame's keys.
// Matches that share a first key write in match order in the reference: a match writes only when no later one of its chain does.
__global__ __launch_bounds__(256) void init_decide_kernel(const InitProbDev *__restrict__ probs, InitResDev *__restrict__ res)
{
    __shared__ int s_pick;
    const InitProbDev &P = probs[blockIdx.x];
    InitResDev &R = res[blockIdx.x];
    const int tid = threadIdx.x, n = P.n_matches;
    if (R.n_hypotheses == 0) return;
    if (tid == 0) {
        const int N = R.n_inl[R.used_homography ? 0 : 1];
        const int pick = R.used_homography ? init_decide_h(R.n_good, R.parallax, N, P.min_parallax, P.min_triangulated)
                                           : init_decide_f(R.n_good, R.parallax, N, P.min_parallax, P.min_triangulated);
        s_pick = pick;
        if (pick >= 0) {
            R.initialized = 1;
            for (int j = 0; j < 9; ++j) R.R21[j] = P.hyp[9 * pick + j];
            for (int j = 0; j < 3; ++j) R.t21[j] = P.hyp[72 + 3 * pick + j];
        }
    }
    __syncthreads();
    const int pick = s_pick;
    if (pick < 0) return;
    const uint8_t *code = P.code + (size_t)pick * n;
    const float *p3d = P.p3d + 3 * (size_t)pick * n;
    for (int i = tid; i < n; i += 256) {
        const int cd = code[i];
        if (!cd) continue;
        bool later_point = false, later_flag = false;
        for (int j = P.next_same[i]; j >= 0; j = P.next_same[j]) {
            later_point |= (code[j] & INIT_RT_GOOD) != 0;
            later_flag |= (code[j] & (INIT_RT_CLEARS | INIT_RT_SETS)) != 0;
        }
        const int k1 = P.matches[2 * i];
        if ((cd & INIT_RT_GOOD) && !later_point) {
            P.P3D[3 * k1] = p3d[3 * i];
            P.P3D[3 * k1 + 1] = p3d[3 * i + 1];
            P.P3D[3 * k1 + 2] = p3d[3 * i + 2];
        }
        if ((cd & (INIT_RT_CLEARS | INIT_RT_SETS)) && !later_flag) P.tri[k1] = (cd & INIT_RT_SETS) != 0;
    }
}

}  // namespace aos2

extern "C" {

int aos2_initializer_initialize(aos2_matcher_t *m, const aos2_initializer_problem_t *problems, aos2_initializer_result_t *results,
                                int n_problems)
{
    using namespace aos2;
    if (!m) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = initializer_check(problems, results, n_problems);
    if (st || n_problems == 0) return st;
    if ((st = matcher_init(m))) return st;
    const int n_dev = n_problems;
    SolverBatch<InitProbDev, InitResDev> B;
    std::vector<int32_t> hyp_prob, next_same, last;
    Arena A{m};
    for (int d = 0; d < n_dev; ++d) {
        const aos2_initializer_problem_t &P = problems[d];
        initializer_result_clear(P, results[d]);
        InitProbDev &D = B.add(d);
        D.n_keys1 = P.n_keys1;
        D.n_keys2 = P.n_keys2;
        D.n_matches = P.n_matches;
        D.its = P.iterations;
        D.min_triangulated = P.min_triangulated;
        D.sigma = P.sigma;
        D.min_parallax = P.min_parallax;
        D.cam = InitCam{P.fx, P.fy, P.cx, P.cy};
        if ((st = flat_list_append(hyp_prob, 2 * (size_t)P.iterations, d, (size_t)INT32_MAX / 32, "more than 2^26 hypotheses in one call",
                                   D.hyp_off)))
            return st;
        const size_t n = (size_t)P.n_matches, its = (size_t)P.iterations;
        next_same.assign(n, -1);
        last.assign((size_t)P.n_keys1, -1);
        for (size_t i = n; i-- > 0;) {
            next_same[i] = last[(size_t)P.matches[2 * i]];
            last[(size_t)P.matches[2 * i]] = (int32_t)i;
        }
        A.in(D.keys1, P.keys1, 8 * (size_t)P.n_keys1);
        A.in(D.keys2, P.keys2, 8 * (size_t)P.n_keys2);
        A.in(D.matches, P.matches, 8 * n);
        A.in(D.sets, P.sets, 32 * its);
        A.in(D.next_same, next_same.data(), 4 * n);
        A.scratch(D.nrm, 32);
        A.scratch(D.models, 72 * 2 * its);
        A.scratch(D.scores, 4 * 2 * its);
        A.scratch(D.hyp, 4 * 96);
        A.scratch(D.cosv, 4 * 8 * n);
        A.scratch(D.p3d, 12 * 8 * n);
        A.scratch(D.code, 8 * n);
        A.out(D.inl, 2 * n);
        A.out(D.P3D, 12 * (size_t)P.n_keys1);
        A.out(D.tri, (size_t)P.n_keys1);
    }
    const int total = (int)hyp_prob.size();
    if ((st = B.begin(A, hyp_prob))) return st;
    hipLaunchKernelGGL(init_prepare_kernel, dim3((4 * n_dev + 63) / 64), dim3(64), 0, m->stream, B.d_probs, n_dev);
    hipLaunchKernelGGL(init_models_kernel, dim3((total + 63) / 64), dim3(64), 0, m->stream, B.d_probs, B.d_hyp, total);
    hipLaunchKernelGGL(init_scores_kernel, dim3((total + 3) / 4), dim3(256), 0, m->stream, B.d_probs, B.d_hyp, total);
    hipLaunchKernelGGL(init_pick_kernel, dim3(n_dev, 2), dim3(256), 0, m->stream, B.d_probs, B.d_res);
    hipLaunchKernelGGL(init_hyps_kernel, dim3((n_dev + 63) / 64), dim3(64), 0, m->stream, B.d_probs, B.d_res, n_dev);
    hipLaunchKernelGGL(init_checkrt_kernel, dim3(n_dev, 8), dim3(256), 0, m->stream, B.d_probs, B.d_res);
    hipLaunchKernelGGL(init_decide_kernel, dim3(n_dev), dim3(256), 0, m->stream, B.d_probs, B.d_res);
    for (int d = 0; d < n_dev; ++d) {
        const aos2_initializer_problem_t &P = problems[d];
        aos2_initializer_result_t &R = results[d];
        A.fetch(R.inliers_h, B.dev[d].inl, (size_t)P.n_matches);
        A.fetch(R.inliers_f, B.dev[d].inl + P.n_matches, (size_t)P.n_matches);
        A.fetch(R.P3D, B.dev[d].P3D, 12 * (size_t)P.n_keys1);
        A.fetch(R.triangulated, B.dev[d].tri, (size_t)P.n_keys1);
    }
    if ((st = B.end(A))) return st;
    for (int d = 0; d < n_dev; ++d) {
        aos2_initializer_result_t &R = results[d];
        const InitResDev &S = B.res[d];
        R.status = S.status;
        R.initialized = S.initialized;
        R.used_homography = S.used_homography;
        R.SH = S.SH;
        R.SF = S.SF;
        memcpy(R.H21, S.H21, sizeof R.H21);
        memcpy(R.F21, S.F21, sizeof R.F21);
        R.best_iteration_h = S.best_h;
        R.best_iteration_f = S.best_f;
        memcpy(R.R21, S.R21, sizeof R.R21);
        memcpy(R.t21, S.t21, sizeof R.t21);
        memcpy(R.n_good, S.n_good, sizeof R.n_good);
        memcpy(R.parallax, S.parallax, sizeof R.parallax);
        R.n_hypotheses = S.n_hypotheses;
    }
    return AOS2_OK;
}

}  // extern "C"
