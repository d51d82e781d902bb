// Optimizer::OptimizeSim3 on gfx950 for a batch of loop candidates (include/aos2.h: aos2_optimize_sim3; reference
// src/Optimizer.cc:1047-1242).  The arithmetic is csrc/sim3_opt.h, shared with the host tap at the end of this file.
#include <vector>

#include "sim3_opt.h"
#include "wave_ops.h"

namespace aos2 {

// one problem with something to run; the pointers are regions of the handle's arena
struct SoResDev {
    Sim3d S;
    int32_t n_bad, n_inliers, wrote, pad;
    int32_t iterations[2], trials[2];
};

struct SoProbDev {
    SoArrays A;
    double *chi;        // [2n] scratch: chi2 of the edge's stored residual (e->chi2())
    uint8_t *act;       // [2n] scratch: the edge is still in the graph
    uint8_t *outlier;   // [n] out
    SoResDev *res;
    Sim3d S_in;
    double th2, delta;
    int32_t fix_scale, pad;
};

constexpr int kSoThreads = 256, kSoRows = kSoThreads / 16;
constexpr int kSoMaxN = (1 << 30) - 1024;   // edge numbers (2 n, plus one stride of the workgroup) stay below 2^31

// The edges of one problem as the workgroup holds them: edge e belongs to thread e % 256 (so an even thread has e12 edges only and
// its neighbour tid ^ 1 the e21 of the same correspondences), the per-edge state lives in global scratch that only the owner touches,
// sums are reduced in an order that is a function of the thread number alone.
struct SoDevEdges {
    const SoProbDev &P;
    double *part;   // [kSoRows][kSoSum]: one partial per row of 16 lanes
    double *fin;    // [kSoSum]
    Sim3d *pert;    // [14][2]: perturbed transform k, forward and inverse
    int *cnt;

    // Workgroup sum of N doubles per thread, the result in every thread.  Row sums by DPP (lane 16 r of a row is the one that is
    // kept), then the 16 row partials of each value are added in row order by one thread: the order depends on nothing but the
    // thread number.  Two barriers: `part` is rewritten only after every reader of the previous call passed its second barrier, `fin`
    // only after the next call's first barrier, which a thread reaches after copying the values out.
    template <int N>
    __device__ __forceinline__ void block_sum(double (&v)[N])
    {
        const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = row_sum_f64(v[i]);
        if ((lane & 15) == 0) {
            double *dst = part + (tid >> 4) * N;
#pragma unroll
            for (int i = 0; i < N; ++i) dst[i] = v[i];
        }
        __syncthreads();
        if (tid < N) {
            double s = part[tid];
#pragma unroll
            for (int r = 1; r < kSoRows; ++r) s += part[r * N + tid];
            fin[tid] = s;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = fin[i];
    }

    // the unperturbed transform of this thread's kind of edge
    __device__ __forceinline__ void own_transform(const Sim3d &S, Sim3d &T0) const
    {
        Sim3d inv;
        so_inverse(S, inv);
        T0 = (threadIdx.x & 1) ? inv : S;
    }

    __device__ __forceinline__ void linearise(const Sim3d &S, bool fix_scale, double delta, double (&Hb)[kSoSum])
    {
        const int tid = threadIdx.x, n2 = 2 * P.A.n;
        if (tid < 14) so_perturbed(S, tid, fix_scale, pert[2 * tid], pert[2 * tid + 1]);   // once per linearisation, for all edges
        Sim3d T0;
        own_transform(S, T0);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kSoSum; ++k) Hb[k] = 0;
        for (int e = tid; e < n2; e += kSoThreads) {
            if (!P.act[e]) continue;
            SoEdge E;
            so_load_edge(P.A, e, E);
            double c;
            so_edge_linearise(T0, pert + (tid & 1), 2, E, delta, Hb, c);
            P.chi[e] = c;
        }
        block_sum(Hb);
    }

    __device__ __forceinline__ double trial(const Sim3d &S, double delta)
    {
        const int tid = threadIdx.x, n2 = 2 * P.A.n;
        Sim3d T0;
        own_transform(S, T0);
        double sum[1] = {0};
        for (int e = tid; e < n2; e += kSoThreads) {
            if (!P.act[e]) continue;
            SoEdge E;
            so_load_edge(P.A, e, E);
            double c;
            sum[0] += so_edge_trial(T0, E, delta, c);
            P.chi[e] = c;
        }
        block_sum(sum);
        return sum[0];
    }

    // :1187-1204 (remove) and :1221-1235: a correspondence with either chi2 above th2 loses its match, and in the first pass both
    // edges.  The other edge's chi2 is in the neighbouring lane.  Returns the number of correspondences flagged by this call.
    __device__ __forceinline__ int reject(double th2, bool remove)
    {
        const int tid = threadIdx.x, lane = tid & 63, n2 = 2 * P.A.n;
        if (tid == 0) *cnt = 0;
        __syncthreads();
        int bad = 0;
        for (int base = tid - lane; base < n2; base += kSoThreads) {   // a wave-uniform trip count: the DPP move needs all 64 lanes
            const int e = base + lane;
            const bool a = e < n2 && P.act[e];
            const double c = a ? P.chi[e] : 0.0;
            const double other = dpp_f64<0xB1>(c);   // lane ^ 1
            if (a && (c > th2 || other > th2)) {
                if (remove) P.act[e] = 0;
                if (!(e & 1)) {
                    P.outlier[e >> 1] = 1;
                    bad++;
                }
            }
        }
        if (bad) atomicAdd(cnt, bad);
        __syncthreads();
        const int total = *cnt;
        __syncthreads();
        return total;
    }
};

// One workgroup of 256 per problem, the whole of :1181-1241 in one launch.  Every thread carries S12, the solver's x and the LM state
// and takes every decision redundantly from the broadcast sums (no thread-0 sections); a trial costs one projection per edge and a
// sum of one, a linearisation 15 projections per edge and a sum of 36.  One wave per SIMD of f64 work: the 36 sums, the 7x7 system
// and the transforms stay in registers.
__global__ __launch_bounds__(kSoThreads) void sim3_opt_kernel(const SoProbDev *__restrict__ probs)
{
    __shared__ double part[kSoRows * kSoSum];
    __shared__ double fin[kSoSum];
    __shared__ Sim3d pert[28];
    __shared__ int cnt;
    const SoProbDev P = probs[blockIdx.x];
    const int tid = threadIdx.x, n2 = 2 * P.A.n;
    for (int e = tid; e < n2; e += kSoThreads) {
        P.act[e] = 1;
        P.chi[e] = 0;
        if (!(e & 1)) P.outlier[e >> 1] = 0;
    }
    SoDevEdges edges{P, part, fin, pert, &cnt};
    SoOutcome o;
    so_procedure(edges, P.S_in, P.A.n, P.th2, P.delta, P.fix_scale != 0, o);
    if (tid == 0) {
        SoResDev &R = *P.res;
        R.S = o.S;
        R.n_bad = o.n_bad;
        R.n_inliers = o.n_inliers;
        R.wrote = o.wrote;
        R.pad = 0;
        for (int k = 0; k < 2; ++k) {
            R.iterations[k] = o.iterations[k];
            R.trials[k] = o.trials[k];
        }
    }
}

// The three members of SoDevEdges alone, on per-edge state the caller planted (aos2_debug_sim3_opt_steps_device): sim3_opt_kernel's
// launch shape and LDS objects, no fill of act / chi / outlier, the steps of `mask` in the order linearise, trial, reject.  What a
// step leaves is copied out by the threads that hold it: the sums by thread 0, pert by threads 0..27, chi by each edge's owner.
struct SoStepDev {
    SoProbDev P;   // chi / act / outlier: planted; res and S_in are not used
    Sim3d S_lin, S_trial;
    double *Hb, *pert, *chi_lin, *trial_sum, *chi_trial;
    int32_t *flagged;
    int32_t mask, remove;
};

__global__ __launch_bounds__(kSoThreads) void sim3_opt_steps_kernel(const SoStepDev *__restrict__ items)
{
    __shared__ double part[kSoRows * kSoSum];
    __shared__ double fin[kSoSum];
    __shared__ Sim3d pert[28];
    __shared__ int cnt;
    const SoStepDev I = items[blockIdx.x];
    const int tid = threadIdx.x, n2 = 2 * I.P.A.n;
    SoDevEdges edges{I.P, part, fin, pert, &cnt};
    if (I.mask & AOS2_SIM3_OPT_STEP_LINEARISE) {
        double Hb[kSoSum];
        edges.linearise(I.S_lin, I.P.fix_scale != 0, I.P.delta, Hb);
        if (tid == 0) {
#pragma unroll
            for (int k = 0; k < kSoSum; ++k) I.Hb[k] = Hb[k];
        }
        if (tid < 28) {
            const Sim3d T = pert[tid];
            double *dst = I.pert + 8 * tid;
            for (int k = 0; k < 4; ++k) dst[k] = T.q[k];
            for (int k = 0; k < 3; ++k) dst[4 + k] = T.t[k];
            dst[7] = T.s;
        }
        for (int e = tid; e < n2; e += kSoThreads) I.chi_lin[e] = I.P.chi[e];
    }
    if (I.mask & AOS2_SIM3_OPT_STEP_TRIAL) {
        const double sum = edges.trial(I.S_trial, I.P.delta);
        if (tid == 0) *I.trial_sum = sum;
        for (int e = tid; e < n2; e += kSoThreads) I.chi_trial[e] = I.P.chi[e];
    }
    if (I.mask & AOS2_SIM3_OPT_STEP_REJECT) {
        const int flagged = edges.reject(I.P.th2, I.remove != 0);
        if (tid == 0) *I.flagged = flagged;
    }
}

// the same edges on the host, one after the other in index order
struct SoHostEdges {
    SoArrays A;
    std::vector<double> chi;
    std::vector<uint8_t> act;
    uint8_t *outlier;
    Sim3d pert[28];   // of the last linearisation

    void linearise(const Sim3d &S, bool fix_scale, double delta, double (&Hb)[kSoSum])
    {
        Sim3d T0[2];
        for (int k = 0; k < 14; ++k) so_perturbed(S, k, fix_scale, pert[2 * k], pert[2 * k + 1]);
        T0[0] = S;
        so_inverse(S, T0[1]);
        for (int k = 0; k < kSoSum; ++k) Hb[k] = 0;
        for (int e = 0; e < 2 * A.n; ++e) {
            if (!act[e]) continue;
            SoEdge E;
            so_load_edge(A, e, E);
            so_edge_linearise(T0[e & 1], pert + (e & 1), 2, E, delta, Hb, chi[e]);
        }
    }
    double trial(const Sim3d &S, double delta)
    {
        Sim3d T0[2];
        T0[0] = S;
        so_inverse(S, T0[1]);
        double sum = 0;
        for (int e = 0; e < 2 * A.n; ++e) {
            if (!act[e]) continue;
            SoEdge E;
            so_load_edge(A, e, E);
            sum += so_edge_trial(T0[e & 1], E, delta, chi[e]);
        }
        return sum;
    }
    int reject(double th2, bool remove)
    {
        int bad = 0;
        for (int c = 0; c < A.n; ++c) {
            if (!act[2 * c] || !(chi[2 * c] > th2 || chi[2 * c + 1] > th2)) continue;
            if (remove) act[2 * c] = act[2 * c + 1] = 0;
            outlier[c] = 1;
            bad++;
        }
        return bad;
    }
};

static int so_check_problem(const aos2_sim3_opt_problem_t &P, const uint8_t *outlier, int i)
{
    if (P.n < 0 || !(P.th2 > 0) || (P.n > 0 && (!P.X1c || !P.X2c || !P.obs1 || !P.obs2 || !P.inv_sigma2_1 || !P.inv_sigma2_2 || !outlier))) {
        set_error("problem %d: bad argument (n >= 0, th2 > 0, the per-correspondence arrays)", i);
        return AOS2_ERR_ARG;
    }
    if (P.n > kSoMaxN) {
        set_error("problem %d: more than %d correspondences", i, kSoMaxN);
        return AOS2_ERR_CAPACITY;
    }
    return AOS2_OK;
}

static int so_check(const aos2_sim3_opt_problem_t *p, const aos2_sim3_opt_result_t *r, int n_problems)
{
    if (n_problems < 0 || n_problems > 64 || (n_problems > 0 && (!p || !r))) {
        set_error("bad argument (0..64 problems and their results)");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n_problems; ++i)
        if (int st = so_check_problem(p[i], r[i].outlier, i)) return st;
    return AOS2_OK;
}

static void so_input(const aos2_sim3_opt_problem_t &P, SoArrays &A, Sim3d &S)
{
    A.n = P.n;
    A.X1c = P.X1c; A.X2c = P.X2c; A.obs1 = P.obs1; A.obs2 = P.obs2; A.w1 = P.inv_sigma2_1; A.w2 = P.inv_sigma2_2;
    A.cam1[0] = (double)P.fx1; A.cam1[1] = (double)P.fy1; A.cam1[2] = (double)P.cx1; A.cam1[3] = (double)P.cy1;
    A.cam2[0] = (double)P.fx2; A.cam2[1] = (double)P.fy2; A.cam2[2] = (double)P.cx2; A.cam2[3] = (double)P.cy2;
    memcpy(S.q, P.q12, sizeof S.q);
    memcpy(S.t, P.t12, sizeof S.t);
    S.s = P.s12;
}

// the result of a problem in which nothing ran (n == 0), or the frame every other result is written into
static void so_result_clear(const aos2_sim3_opt_problem_t &P, aos2_sim3_opt_result_t &R)
{
    uint8_t *out = R.outlier;
    R = aos2_sim3_opt_result_t{};
    R.outlier = out;
    memcpy(R.q12, P.q12, sizeof R.q12);
    memcpy(R.t12, P.t12, sizeof R.t12);
    R.s12 = P.s12;
    if (P.n > 0) memset(out, 0, (size_t)P.n);
}

static void so_result_set(const aos2_sim3_opt_problem_t &P, const Sim3d &S, int wrote, int n_bad, int n_inliers, const int32_t *iterations,
                          const int32_t *trials, aos2_sim3_opt_result_t &R)
{
    if (wrote) {   // (otherwise the caller's g2oS12 stays: so_result_clear copied it)
        memcpy(R.q12, S.q, sizeof R.q12);
        memcpy(R.t12, S.t, sizeof R.t12);
        R.s12 = S.s;
    }
    R.n_bad = n_bad;
    R.n_inliers = n_inliers;
    for (int k = 0; k < 2; ++k) {
        R.iterations[k] = iterations[k];
        R.trials[k] = trials[k];
    }
}

// deltaHuber (:1096): a float
static double so_delta(float th2) { return (double)sqrtf(th2); }

static int so_steps_check(const aos2_sim3_opt_steps_t *it, int n_items)
{
    if (n_items < 0 || n_items > 64 || (n_items > 0 && !it)) {
        set_error("bad argument (0..64 items)");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < n_items; ++i) {
        const aos2_sim3_opt_steps_t &I = it[i];
        if (int st = so_check_problem(I.problem, I.outlier, i)) return st;
        if (I.problem.n < 1 || I.tail < 0 || I.tail > 4096 || (I.mask & ~7) || !I.act_in || !I.chi_in || !I.outlier_in || !I.Hb || !I.pert || !I.chi_lin ||
            !I.trial_sum || !I.chi_trial || !I.flagged || !I.chi || !I.act) {
            set_error("item %d: bad argument (n >= 1, 0 <= tail <= 4096, mask of 3 bits, every buffer)", i);
            return AOS2_ERR_ARG;
        }
    }
    return AOS2_OK;
}

static void so_sim3_of(const double *v, Sim3d &S)
{
    memcpy(S.q, v, sizeof S.q);
    memcpy(S.t, v + 4, sizeof S.t);
    S.s = v[7];
}

// A problem's six input arrays staged, with the pointers of D.A registered for them (D stays where it is until the arena is bound),
// and everything of D that is no pointer into the arena.
static void so_stage(HostArena &H, const aos2_sim3_opt_problem_t &P, SoProbDev &D)
{
    const size_t n = (size_t)P.n;
    so_input(P, D.A, D.S_in);
    H.in(D.A.X1c, P.X1c, 3 * n);
    H.in(D.A.X2c, P.X2c, 3 * n);
    H.in(D.A.obs1, P.obs1, 2 * n);
    H.in(D.A.obs2, P.obs2, 2 * n);
    H.in(D.A.w1, P.inv_sigma2_1, n);
    H.in(D.A.w2, P.inv_sigma2_2, n);
    D.th2 = (double)P.th2;
    D.delta = so_delta(P.th2);
    D.fix_scale = P.fix_scale != 0;
    D.pad = 0;
}

}  // namespace aos2

using namespace aos2;

extern "C" {

int aos2_optimize_sim3(aos2_lba_t *s, const aos2_sim3_opt_problem_t *p, aos2_sim3_opt_result_t *r, int n_problems)
{
    if (!s) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = so_check(p, r, n_problems);
    if (st || n_problems == 0) return st;
    if ((st = lba_handle_init(s))) return st;
    std::vector<int> src;   // the problems with something to run
    for (int i = 0; i < n_problems; ++i)
        if (p[i].n > 0) src.push_back(i);
    const int n_dev = (int)src.size();
    s->last_sim3_opt_ms = 0;
    if (n_dev == 0) {
        for (int i = 0; i < n_problems; ++i) so_result_clear(p[i], r[i]);
        return AOS2_OK;
    }
    // inputs and the problem descriptors go up as one copy from the handle's page-locked staging buffer, the results of all problems
    // -- outcome and outlier flags -- are neighbours in the arena and come back as one copy (as aos2_pose_optimization does it)
    HostArena H;
    H.fields.swap(s->so_fields);   // (the handle keeps the list's memory between calls)
    H.fields.clear();
    std::vector<SoProbDev> dev((size_t)n_dev);   // the table: its pointer fields are registered with the arena, by address
    size_t in_cap = sizeof(SoProbDev) * (size_t)n_dev + 512;
    for (int d = 0; d < n_dev; ++d) in_cap += (size_t)p[src[d]].n * (12 + 12 + 8 + 8 + 4 + 4) + 6 * 256;
    if ((st = s->h_in.alloc(in_cap))) return st;
    H.host = s->h_in.p;
    H.host_cap = in_cap;
    for (int d = 0; d < n_dev; ++d) so_stage(H, p[src[d]], dev[d]);
    size_t o_probs;
    SoProbDev *table = H.push_fill<SoProbDev>((size_t)n_dev, o_probs);   // filled below (needs the device base)
    if (!table || H.host_size > in_cap) {
        set_error("internal: OptimizeSim3 input staging");
        return AOS2_ERR_ARG;
    }
    const size_t in_bytes = H.host_size;
    for (int d = 0; d < n_dev; ++d) {
        const size_t n = (size_t)p[src[d]].n;
        H.room(dev[d].chi, 2 * n);
        H.room(dev[d].act, 2 * n);
    }
    const size_t o_res = up256(H.size);   // results of all problems from here on
    for (int d = 0; d < n_dev; ++d) {
        H.room(dev[d].res, 1);
        H.room(dev[d].outlier, (size_t)p[src[d]].n);
    }
    const size_t res_bytes = H.size - o_res;
    if ((st = s->arena.alloc(H.size + 256))) return st;
    if ((st = s->h_stage.alloc(res_bytes + 64))) return st;
    uint8_t *base = s->arena.p;
    H.bind(base);
    memcpy(table, dev.data(), sizeof(SoProbDev) * (size_t)n_dev);
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(base, H.data(), in_bytes, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipEventRecord(s->ev[0], q));
    hipLaunchKernelGGL(sim3_opt_kernel, dim3(n_dev), dim3(kSoThreads), 0, q, (const SoProbDev *)(base + o_probs));
    AOS2_HIP_CHECK(hipEventRecord(s->ev[1], q));
    const uint8_t *res = s->h_stage.p;
    AOS2_HIP_CHECK(hipMemcpyAsync(s->h_stage.p, base + o_res, res_bytes, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    (void)hipEventElapsedTime(&s->last_sim3_opt_ms, s->ev[0], s->ev[1]);
    for (int i = 0; i < n_problems; ++i) so_result_clear(p[i], r[i]);
    for (int d = 0; d < n_dev; ++d) {
        const aos2_sim3_opt_problem_t &P = p[src[d]];
        SoResDev R;
        memcpy(&R, span_copy(res, base + o_res, dev[d].res), sizeof R);
        memcpy(r[src[d]].outlier, span_copy(res, base + o_res, dev[d].outlier), (size_t)P.n);
        so_result_set(P, R.S, R.wrote, R.n_bad, R.n_inliers, R.iterations, R.trials, r[src[d]]);
    }
    s->so_fields.swap(H.fields);
    return AOS2_OK;
}

float aos2_optimize_sim3_last_device_ms(const aos2_lba_t *s) { return s ? s->last_sim3_opt_ms : 0.f; }

int aos2_debug_sim3_opt_host(const aos2_sim3_opt_problem_t *p, aos2_sim3_opt_result_t *r, int n_problems)
{
    if (int st = so_check(p, r, n_problems)) return st;
    for (int i = 0; i < n_problems; ++i) {
        const aos2_sim3_opt_problem_t &P = p[i];
        so_result_clear(P, r[i]);
        if (P.n == 0) continue;
        SoHostEdges E;
        Sim3d S_in;
        so_input(P, E.A, S_in);
        E.chi.assign(2 * (size_t)P.n, 0.0);
        E.act.assign(2 * (size_t)P.n, 1);
        E.outlier = r[i].outlier;
        SoOutcome o;
        so_procedure(E, S_in, P.n, (double)P.th2, so_delta(P.th2), P.fix_scale != 0, o);
        so_result_set(P, o.S, o.wrote, o.n_bad, o.n_inliers, o.iterations, o.trials, r[i]);
    }
    return AOS2_OK;
}

int aos2_debug_sim3_opt_steps_host(const aos2_sim3_opt_steps_t *items, int n_items)
{
    if (int st = so_steps_check(items, n_items)) return st;
    for (int i = 0; i < n_items; ++i) {
        const aos2_sim3_opt_steps_t &I = items[i];
        const aos2_sim3_opt_problem_t &P = I.problem;
        const size_t n2 = 2 * (size_t)P.n, tail = (size_t)I.tail;
        SoHostEdges E;
        Sim3d S_lin, S_trial;
        so_input(P, E.A, S_lin);
        so_sim3_of(I.S_lin, S_lin);
        so_sim3_of(I.S_trial, S_trial);
        E.chi.assign(I.chi_in, I.chi_in + n2 + tail);
        E.act.assign(I.act_in, I.act_in + n2 + tail);
        memmove(I.outlier, I.outlier_in, (size_t)P.n + tail);
        E.outlier = I.outlier;
        const double delta = so_delta(P.th2);
        if (I.mask & AOS2_SIM3_OPT_STEP_LINEARISE) {
            double Hb[kSoSum];
            E.linearise(S_lin, P.fix_scale != 0, delta, Hb);
            memcpy(I.Hb, Hb, sizeof Hb);
            for (int k = 0; k < 28; ++k) {
                memcpy(I.pert + 8 * k, E.pert[k].q, 4 * sizeof(double));
                memcpy(I.pert + 8 * k + 4, E.pert[k].t, 3 * sizeof(double));
                I.pert[8 * k + 7] = E.pert[k].s;
            }
            memcpy(I.chi_lin, E.chi.data(), n2 * sizeof(double));
        }
        if (I.mask & AOS2_SIM3_OPT_STEP_TRIAL) {
            *I.trial_sum = E.trial(S_trial, delta);
            memcpy(I.chi_trial, E.chi.data(), n2 * sizeof(double));
        }
        if (I.mask & AOS2_SIM3_OPT_STEP_REJECT) *I.flagged = E.reject((double)P.th2, I.remove != 0);
        memcpy(I.chi, E.chi.data(), (n2 + tail) * sizeof(double));
        memcpy(I.act, E.act.data(), n2 + tail);
    }
    return AOS2_OK;
}

int aos2_debug_sim3_opt_steps_device(aos2_lba_t *s, const aos2_sim3_opt_steps_t *items, int n_items)
{
    if (!s) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = so_steps_check(items, n_items);
    if (st || n_items == 0) return st;
    if ((st = lba_handle_init(s))) return st;
    // One image of the arena goes up and the whole of it comes back: the outputs start as what the caller's buffers hold, so what no
    // thread writes returns as it was passed in.
    HostArena H;
    std::vector<SoStepDev> dev((size_t)n_items);   // the table: its pointer fields are registered with the arena, by address
    for (int i = 0; i < n_items; ++i) {
        const aos2_sim3_opt_steps_t &I = items[i];
        const size_t n = (size_t)I.problem.n, tail = (size_t)I.tail;
        SoStepDev &D = dev[i];
        so_stage(H, I.problem, D.P);
        H.in(D.P.chi, I.chi_in, 2 * n + tail);
        H.in(D.P.act, I.act_in, 2 * n + tail);
        H.in(D.P.outlier, I.outlier_in, n + tail);
        H.in(D.Hb, I.Hb, kSoSum);
        H.in(D.pert, I.pert, 8 * 28);
        H.in(D.chi_lin, I.chi_lin, 2 * n);
        H.in(D.trial_sum, I.trial_sum, 1);
        H.in(D.chi_trial, I.chi_trial, 2 * n);
        H.in(D.flagged, I.flagged, 1);
        so_sim3_of(I.S_lin, D.S_lin);
        so_sim3_of(I.S_trial, D.S_trial);
        D.mask = I.mask;
        D.remove = I.remove != 0;
    }
    const size_t o_items = H.push(nullptr, sizeof(SoStepDev) * (size_t)n_items);
    H.own.resize(H.size);
    if ((st = s->arena.alloc(H.size + 256))) return st;
    uint8_t *base = s->arena.p;
    H.bind(base);
    memcpy(H.own.data() + o_items, dev.data(), sizeof(SoStepDev) * (size_t)n_items);
    hipStream_t q = s->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(base, H.own.data(), H.size, hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(sim3_opt_steps_kernel, dim3(n_items), dim3(kSoThreads), 0, q, (const SoStepDev *)(base + o_items));
    AOS2_HIP_CHECK(hipMemcpyAsync(H.own.data(), base, H.size, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    for (int i = 0; i < n_items; ++i) {
        const aos2_sim3_opt_steps_t &I = items[i];
        const size_t n = (size_t)I.problem.n, tail = (size_t)I.tail;
        const SoStepDev &D = dev[i];
        const uint8_t *back = H.own.data();
        memcpy(I.chi, span_copy(back, base, D.P.chi), bytes_of(D.P.chi, 2 * n + tail));
        memcpy(I.act, span_copy(back, base, D.P.act), 2 * n + tail);
        memcpy(I.outlier, span_copy(back, base, D.P.outlier), n + tail);
        memcpy(I.Hb, span_copy(back, base, D.Hb), bytes_of(D.Hb, kSoSum));
        memcpy(I.pert, span_copy(back, base, D.pert), bytes_of(D.pert, 8 * 28));
        memcpy(I.chi_lin, span_copy(back, base, D.chi_lin), bytes_of(D.chi_lin, 2 * n));
        memcpy(I.trial_sum, span_copy(back, base, D.trial_sum), bytes_of(D.trial_sum, 1));
        memcpy(I.chi_trial, span_copy(back, base, D.chi_trial), bytes_of(D.chi_trial, 2 * n));
        memcpy(I.flagged, span_copy(back, base, D.flagged), bytes_of(D.flagged, 1));
    }
    return AOS2_OK;
}

}  // extern "C"
