// Optimizer::LocalBundleAdjustment numerical core on gfx950 (reference src/Optimizer.cc:507-744 and
// the vendored g2o it drives: optimization_algorithm_levenberg.cpp:61-164, block_solver.hpp:367-604,
// base_binary_edge.hpp:55-120, robust_kernel_impl.cpp:78-91, types_six_dof_expmap.{h,cpp},
// se3quat.h).  All arithmetic is IEEE double like g2o (one float reciprocal in the stereo
// projection, types_six_dof_expmap.cpp:151).
//
// One call solves a BATCH of independent windows (aos2_lba_solve_batch; aos2_lba_solve is a batch of one).
// Every kernel takes the array of window descriptors and uses blockIdx.y as the window, so the latency-bound
// Levenberg-Marquardt chains of all windows advance side by side on different compute units.
//
// The whole procedure of a window -- optimize(5), the outlier pass, optimize(10), the final inlier check -- is
// enqueued as ONE program; the Levenberg-Marquardt control flow (rho, lambda, accept / restore, the three
// termination rules, the iteration counters, the polls of pbStopFlag) lives in a small per-window state block on the
// device (LmState), updated after every trial by the landmark kernel's last workgroup (lm_decide); every kernel is gated by that state.  The host only
// looks at the states when the program has run: a window that needed more trials than were enqueued (steps rejected
// by the gain ratio) gets another short program.  No host round trip per trial.
//
// Device layout: SoA doubles for poses (qx qy qz qw tx ty tz), points, edges.  The edge set of a window has three CSR
// views (by point, by free pose, by point restricted to free poses sorted by pose = the Hpl column of
// block_solver.hpp:398) built once per call.  The second optimisation (level-0 edges only, Optimizer.cc:672-708)
// reuses them: an excluded edge is MASKED -- its Jacobians, weights and Hpl block are written as zeros, its residual
// is left alone like g2o leaves the _error of an inactive edge -- so every sum it took part in receives +0.0, which
// is the same as leaving it out; vertices that lose all their edges keep a lambda-only diagonal block, decoupled from
// the rest, and receive a zero update (g2o drops them from the index mapping instead: same result for the others).
//
// This unit holds every kernel and the helpers that launch them (lba_launch.h).  What host and device share -- the window
// descriptor LbaWin, LmState, EdgeRec, SchurTask and the constants the layout depends on -- is lba_window.h; the host plan that
// fills them is lba_plan.h; the handle, the steps of a solve and the C API are lba_solve.hip; the test taps are lba_taps.hip.
#include "lba_launch.h"
#include "ldlt_reg.h"
#include "wave_ops.h"

namespace aos2 {

// an edge record as its two 16-byte halves: {obs[3], w} and {pose, pl_pos, flags, -}
typedef float flt4_t __attribute__((ext_vector_type(4)));
typedef int int4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void erec_load(const LbaWin &W, int a, flt4_t &lo, int4_t &hi)
{
    const EdgeRec *r = W.erec + a;
    lo = *reinterpret_cast<const flt4_t *>(r);
    hi = *(reinterpret_cast<const int4_t *>(r) + 1);
}
__device__ __forceinline__ void erec_store(const LbaWin &W, int a, flt4_t lo, int4_t hi)
{
    EdgeRec *r = W.erec + a;
    *reinterpret_cast<flt4_t *>(r) = lo;
    *(reinterpret_cast<int4_t *>(r) + 1) = hi;
}

// bool SparseOptimizer::terminate(): counts the evaluation, latches the flag
// `seen` >= 0: the value of the flag read by the caller shortly before (the word lives in host memory: a read is a PCIe
// round trip, which the decision starts ahead of its other loads)
__device__ inline bool lm_poll(LmState *st, const int32_t *abort_word, int seen = -1)
{
    st->polls++;
    if (st->stop_poll > 0) return true;
    const int a = seen >= 0 ? seen : abort_word ? __hip_atomic_load(abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
    if (a || (st->stop_at_poll > 0 && st->polls >= st->stop_at_poll)) {
        st->stop_poll = st->polls;
        return true;
    }
    return false;
}

// Optimizer.cc:663-666 right after optimizer.optimize(5) returned: bDoMore = !*pbStopFlag.  Called where the first
// optimisation ends (the LM decision of its last trial, or k_prepare when it does not run at all); xmark = 1 lets the
// transition kernel run the outlier pass.
__device__ inline void lm_first_done(LmState *st, const int32_t *abort_word, int seen = -1)
{
    st->phase = 1;
    st->xmark = 0;
    if (lm_poll(st, abort_word, seen)) {
        st->phase = 3;
        return;
    }
    st->xmark = 1;
    st->n_active = 0;
}

// Sums of two values per thread of an N-thread workgroup (binary trees in LDS, fixed order) -> out0[blockIdx.x], out1[blockIdx.x]
template <int N>
__device__ __forceinline__ void workgroup_sum2(double v0, double v1, double *out0, double *out1)
{
    __shared__ double sh[2][N];
    sh[0][threadIdx.x] = v0;
    sh[1][threadIdx.x] = v1;
    __syncthreads();
#pragma unroll
    for (int s = N / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sh[0][threadIdx.x] = sh[0][threadIdx.x] + sh[0][threadIdx.x + s];
            sh[1][threadIdx.x] = sh[1][threadIdx.x] + sh[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out0[blockIdx.x] = sh[0][0];
        out1[blockIdx.x] = sh[1][0];
    }
}

// Converter::toSE3Quat / toVector3d and the float -> double copies of Optimizer.cc:523-525, 552-553, 597-606
__global__ __launch_bounds__(256) void k_prepare(const LbaWin *__restrict__ wins, int stop_at_poll)
{
    const LbaWin &W = wins[blockIdx.y];
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < W.n_poses) pose_from_Tcw(W.in_Tcw + 16 * (size_t)i, W.pose + 7 * (size_t)i);
    if (i < W.n_points)
        for (int d = 0; d < 3; ++d) W.point[3 * (size_t)i + d] = (double)W.in_xyz[3 * (size_t)i + d];
    if (i < W.n_edges) {
        for (int d = 0; d < 3; ++d) W.err[3 * (size_t)i + d] = 0.0;
        W.e_robust[i] = 1;
        W.e_level1[i] = 0;
        // the record of position i of the landmarks' edge lists (every edge is in the list once)
        const int k = W.pt_k[i];
        const flt4_t lo = {W.in_obs[3 * (size_t)k], W.in_obs[3 * (size_t)k + 1], W.in_obs[3 * (size_t)k + 2], W.in_w[k]};
        const int4_t hi = {W.e_pose[k], W.pl_pos[k], (int)((W.e_stereo[k] ? kEdgeStereo : 0) | kEdgeRobust), 0};
        erec_store(W, i, lo, hi);
    }
    if (blockIdx.x == 0 && W.hs_ld == W.npad) {   // reduced system stored padded (k_ldlt_reg, k_ldlt_dev): the identity tail of the matrix, once
        const int n = 6 * W.np, npad = W.npad;
        for (int q = threadIdx.x; q < (npad - n) * npad; q += 256) {
            const int r = n + q / npad, c = q % npad;
            W.Hs[(size_t)r * npad + c] = r == c ? 1.0 : 0.0;
        }
        // ... and the columns beyond n of the rows above it (k_ldlt_reg loads its tiles from the upper block triangle)
        for (int q = threadIdx.x; q < n * (npad - n); q += 256) {
            const int r = q / (npad - n), c = n + q % (npad - n);
            W.Hs[(size_t)r * npad + c] = 0.0;
        }
    }
    if (blockIdx.x == 0) {   // the state record (1.8 KB): zeroed by the workgroup, not by one thread
        LmState *st = W.st;
        static_assert(sizeof(LmState) % 8 == 0, "LmState is cleared as 64-bit words");
        for (int k = threadIdx.x; k < (int)(sizeof(LmState) / 8); k += 256) reinterpret_cast<long long *>(st)[k] = 0;
        __syncthreads();
        if (threadIdx.x == 0) {
            st->iters_max[0] = W.iters1;
            st->iters_max[1] = W.iters2;
            st->polls = 1;   // the entry check of Optimizer.cc:656-658 was made on the host
            st->stop_at_poll = stop_at_poll;
            st->n_active = W.n_edges;
            // SparseOptimizer::optimize(iterations) entry, first call (sparse_optimizer.cpp:354-372): `i < iterations &&
            // !terminate() && ok` before the first iteration
            st->phase = 0;
            st->it = 0;
            if (st->iters_max[0] <= 0 || lm_poll(st, W.abort_word)) {
                st->iters_done[0] = 0;
                lm_first_done(st, W.abort_word);
            } else
                st->initp = 1;
        }
    }
}

// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::computeError (types_six_dof_expmap.h:80-141) with the camera point given
__device__ __forceinline__ void edge_error(const Cam &cam, const double p[3], const double *obs, int stereo, double er[3])
{
    if (!stereo) {
        const double u = p[0] / p[2], v = p[1] / p[2];
        er[0] = obs[0] - (u * cam.fx + cam.cx);
        er[1] = obs[1] - (v * cam.fy + cam.cy);
        er[2] = 0;
    } else {
        const float invz = (float)(1.0 / p[2]);
        const double r0 = p[0] * invz * cam.fx + cam.cx;
        const double r1 = p[1] * invz * cam.fy + cam.cy;
        const double r2 = r0 - (double)__fmul_rn(cam.bf_f, invz);
        er[0] = obs[0] - r0;
        er[1] = obs[1] - r1;
        er[2] = obs[2] - r2;
    }
}

// The decision of one Levenberg-Marquardt trial and everything that hangs on it (levenberg.cpp:99-164,
// sparse_optimizer.cpp:372-414): gain ratio, lambda update or pop(), the `while (rho < 0 && qmax < maxTrials &&
// !terminate())` condition, the three ways an iteration can end the optimisation, and the `for (i < iterations &&
// !terminate() && ok)` condition of the next iteration.  Thread 0 decides, all threads
// restore the estimates after a rejected step.  Runs at the end of k_points(solve = 1) in the workgroup that finished
// LAST (no launch of its own): what the other workgroups of this launch wrote -- the per-landmark sums, and on the restore
// path their backups -- is read with device-scope loads.
__device__ __forceinline__ double load_dev(const double *p)
{
    return __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
}
// ... and the matching store: write-through at device scope (what a workgroup hands to the deciding one)
__device__ __forceinline__ void store_dev(double *p, double v)
{
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(p), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
// chi2 (and the scale terms x_j (lambda x_j + b_j)) of a trial from the per-landmark sums k_points left: value i goes to
// virtual lane i % 128, a lane adds its values in ascending order, a tree adds the 128 lanes -- an order that depends on
// the problem only, not on how the landmark kernels were launched (both landmark-kernel layouts and every batch size give
// the same bits).  Called by all threads of a workgroup of >= 128 threads.
__device__ __forceinline__ void canonical_sums(const LbaWin &W, bool with_scale, double &chi_out, double &scale_out)
{
    __shared__ double s_red[2][128];
    const int tid = threadIdx.x;
    if (tid < 128) {
        double c = 0, s2 = 0;
        for (int i0 = tid; i0 < W.nl; i0 += 128 * 16) {   // 16 values of the lane in flight, added in ascending order
            double v[16], w[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                const int i = i0 + 128 * u;
                v[u] = i < W.nl ? load_dev(W.part + i) : 0.0;
                w[u] = with_scale && i < W.nl ? load_dev(W.part + W.nl + i) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) {
                c += v[u];     // (x + 0.0 == x past the end)
                s2 += w[u];
            }
        }
        if (with_scale)
            for (int i = tid; i < 6 * W.np; i += 128) s2 += W.tmp[i];
        s_red[0][tid] = c;
        s_red[1][tid] = s2;
    }
    __syncthreads();
    for (int h = 64; h > 0; h >>= 1) {
        if (tid < h) {
            s_red[0][tid] += s_red[0][tid + h];
            s_red[1][tid] += s_red[1][tid + h];
        }
        __syncthreads();
    }
    chi_out = s_red[0][0];
    scale_out = s_red[1][0];
}
template <int NT>
__device__ __forceinline__ void lm_decide(const LbaWin &W)
{
    __shared__ int s_restore;
    LmState *st = W.st;
    // pbStopFlag lives in host memory: its read (a PCIe round trip) travels together with the loads of the sums
    const int flag_seen = threadIdx.x == 0 && W.abort_word ? __hip_atomic_load(W.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
    double tempChi, scale;
    canonical_sums(W, true, tempChi, scale);
    if (threadIdx.x == 0) {
        const int pass = st->phase == 0 ? 0 : 1;
        const bool ok2 = W.np == 0 || W.scal[3] != 0.0;
        if (!ok2) {
            tempChi = 1.7976931348623157e308;
            st->solver_failed++;
        }
        double rho = st->currentChi - tempChi;
        scale += 1e-3;
        rho /= scale;
        if (!ok2) rho = -1.0;   // (currentChi - DBL_MAX) / scale: negative for the positive scale of an LM step
        const bool accepted = rho > 0 && isfinite(tempChi);
        if (st->ntr < 48) {
            st->tr_rho[st->ntr] = rho; st->tr_temp[st->ntr] = tempChi; st->tr_cur[st->ntr] = st->currentChi;
            st->tr_lambda[st->ntr] = st->lambda;
            st->ntr++;
        }
        if (accepted) {
            const double t3 = 2 * rho - 1;
            double alpha = 1. - t3 * t3 * t3;
            alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
            const double scaleFactor = 1. / 3. > alpha ? 1. / 3. : alpha;
            st->lambda *= scaleFactor;
            st->ni = 2;
            st->currentChi = tempChi;
            st->err_at = 1;
        } else {
            st->lambda *= st->ni;
            st->ni *= 2;
            st->err_at = 2;
        }
        s_restore = accepted ? 0 : 1;
        st->qmax++;
        st->trials[pass]++;
        int lin = 0;
        const bool again = rho < 0 && st->qmax < 10 && !lm_poll(st, W.abort_word, flag_seen);
        if (!again) {
            bool term = st->qmax == 10 || rho == 0;
            if (!term) {
                if ((st->iniChi - st->currentChi) * 1e3 < st->iniChi)
                    st->nBad++;
                else
                    st->nBad = 0;
                term = st->nBad >= 3;
            }
            st->it++;
            bool more = st->it < st->iters_max[pass];
            if (more) more = !lm_poll(st, W.abort_word, flag_seen);   // evaluated before `ok`
            if (more) more = !term;
            if (more) {
                st->qmax = 0;
                st->iniChi = st->currentChi;
                lin = accepted ? 1 : 0;   // (a step that was neither accepted nor repeated leaves the system as it is)
            } else {
                st->run = 0;
                st->iters_done[pass] = st->it;
                st->final_chi2 = st->currentChi;
                st->final_lambda = st->lambda;
                if (pass == 0)
                    lm_first_done(st, W.abort_word, flag_seen);
                else
                    st->phase = 3;
            }
        }
        st->lin = lin;
    }
    __syncthreads();
    // pop() after a rejected step (SparseOptimizer::push / pop, sparse_optimizer.cpp:600-610).  The backup holds the
    // estimates a trial starts from: the kernels that move an estimate (the pose update of the reduced-system kernel, the
    // landmark update of k_points) save the old value first -- push() costs no pass of its own.
    // The trial's estimates are kept in the backup's place (a swap): the edges' _error after a rejected trial is the
    // one computed AT the trial (computeActiveErrors ran before pop()), and the passes that read it re-form it from there.
    if (s_restore)
        for (int i = threadIdx.x; i < W.est_n; i += NT) {
            const double trial = load_dev(W.pose + i);
            W.pose[i] = load_dev(W.bk + i);
            W.bk[i] = trial;
        }
}

// end of a k_points launch (solve = 1): the workgroup that finishes last takes the LM decision
template <int NT>
__device__ __forceinline__ void points_tail(const LbaWin &W)
{
    __shared__ int s_last;
    // What this workgroup leaves for the deciding one -- the per-landmark sums and the landmark backups -- was stored
    // write-through at device scope (store_dev), so its visibility needs the stores' completion only (every thread waits
    // for its own, then the barrier), not a write-back of the whole L2: __threadfence() here (buffer_wbl2 by each of the
    // ~1000 workgroups of a 32-window launch) cost 38 of the kernel's 79 us.
    // (Round 4: the workgroup-scope release fence alone does NOT wait for them -- outside tgsplit mode the compiler emits only
    // `s_waitcnt lgkmcnt(0)` for it, and the counter's atomic could reach its L2 channel before a sum's store reached its own:
    // a deciding workgroup then read a stale sum.  Two window groups running side by side made it show -- 4 wrong windows in
    // ~250 batches of 17 on two of three boxes, none in 3.6 M hand-overs of the round-2 stress on a quiet device.  Every thread
    // now waits for the completion of its own write-through stores explicitly.)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(&W.st->blocks_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == W.n_part - 1;
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   // (the reads below are device-scope loads: load_dev)
    if (threadIdx.x == 0) W.st->blocks_done = 0;
    lm_decide<NT>(W);
}

// J_pose of an edge (linearizeOplus, types_six_dof_expmap.cpp:103-157, 188-234): rows 0-1 (and 2 for stereo) x 6.
// One division per edge: with iz = 1 / z, a = x iz, b = y iz the entries x y / z^2 fx, (1 + x^2 / z^2) fx, y / z fx, ... are
// products (the reference divides ~13 times per edge here and ~9 more in the landmark Jacobian; an f64 division is ~10
// dependent instructions on this part).  Same quantities, equal to rounding (1e-16 relative) -- like the pose-only kernel.
__device__ __forceinline__ void jac_pose(const Cam &cam, const double p[3], int stereo, double Jb[18])
{
    const double fx = cam.fx, fy = cam.fy, bf = cam.bf;
    const double iz = 1.0 / p[2], a = p[0] * iz, b = p[1] * iz, ab = a * b;
    Jb[0] = ab * fx;
    Jb[1] = -(1 + a * a) * fx;
    Jb[2] = b * fx;
    Jb[3] = -(iz * fx);
    Jb[4] = 0;
    Jb[5] = a * iz * fx;
    Jb[6] = (1 + b * b) * fy;
    Jb[7] = -(ab * fy);
    Jb[8] = -(a * fy);
    Jb[9] = 0;
    Jb[10] = -(iz * fy);
    Jb[11] = b * iz * fy;
#pragma unroll
    for (int i = 12; i < 18; ++i) Jb[i] = 0;
    if (stereo) {
        const double bfz2 = bf * (iz * iz);
        Jb[12] = Jb[0] - bfz2 * p[1];
        Jb[13] = Jb[1] + bfz2 * p[0];
        Jb[14] = Jb[2];
        Jb[15] = Jb[3];
        Jb[16] = 0;
        Jb[17] = Jb[5] - bfz2;
    }
}

// J_point of an edge (the same linearizeOplus): -1 / z [fx 0 -x / z fx; 0 fy -y / z fy] R for the two pixel rows (mono and
// stereo edges alike), the stereo row = row 0 - bf / z^2 R_2.  R = the keyframe's rotation (row-major), one division.
__device__ __forceinline__ void jac_point(const Cam &cam, const double R[9], const double p[3], int stereo, double Ja[9])
{
    const double iz = 1.0 / p[2], a = p[0] * iz, b = p[1] * iz;
    const double fxz = cam.fx * iz, fyz = cam.fy * iz, afxz = a * fxz, bfyz = b * fyz;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Ja[c] = afxz * R[6 + c] - fxz * R[c];
        Ja[3 + c] = bfyz * R[6 + c] - fyz * R[3 + c];
        Ja[6 + c] = 0;
    }
    if (stereo) {
        const double bfz2 = cam.bf * (iz * iz);
#pragma unroll
        for (int c = 0; c < 3; ++c) Ja[6 + c] = Ja[c] - bfz2 * R[6 + c];
    }
}

// ---- linearisation records (LbaWin::lrec).  With a = x / z, b = y / z, iz = 1 / z the Jacobians of an edge
// (linearizeOplus, jac_pose / jac_point above) are  J_pose = Pt E,  J_point = -iz Pt R  with
//     Pt = [fx 0 -a fx; 0 fy -b fy; (stereo) fx 0 bf iz - a fx],   E = [ [a b 1]x | -iz I ]  (3 x 6),
// so the edge's Hpl block is  J_pose^T w J_point = -E^T C R,  C = w iz Pt^T Pt  (symmetric 3 x 3, C01 = 0): six numbers
// formed from the record in ~20 operations, and the products with E are cross products with (a, b, 1).
typedef double dbl4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void lrec_store(const LbaWin &W, int pos, const double p[3], double wo, int stereo, const double omr[3])
{
    const double iz = 1.0 / p[2];
    const dbl4_t v = {p[0] * iz, p[1] * iz, iz, stereo ? -wo : wo};
    *reinterpret_cast<dbl4_t *>(W.lrec + 4 * (size_t)pos) = v;
#pragma unroll
    for (int i = 0; i < 3; ++i) W.lomr[3 * (size_t)pos + i] = omr[i];
}
__device__ __forceinline__ void lrec_mask(const LbaWin &W, int pos)
{
    const dbl4_t v = {0.0, 0.0, 0.0, 0.0};
    *reinterpret_cast<dbl4_t *>(W.lrec + 4 * (size_t)pos) = v;
#pragma unroll
    for (int i = 0; i < 3; ++i) W.lomr[3 * (size_t)pos + i] = 0.0;
}
__device__ __forceinline__ dbl4_t lrec_load(const LbaWin &W, int pos) { return *reinterpret_cast<const dbl4_t *>(W.lrec + 4 * (size_t)pos); }
struct EdgeLin {
    double a, b, iz;
    double C00, C02, C11, C12, C22;
};
__device__ __forceinline__ EdgeLin lrec_form(const Cam &cam, const dbl4_t rec)
{
    EdgeLin L;
    L.a = rec.x; L.b = rec.y; L.iz = rec.z;
    const bool stereo = rec.w < 0.0;
    const double s = fabs(rec.w) * L.iz;
    const double fx2 = cam.fx * cam.fx, fy2 = cam.fy * cam.fy;
    // (a mono edge adds exact zeros for the third row)
    const double fs = stereo ? cam.fx : 0.0, c = stereo ? cam.bf * L.iz - L.a * cam.fx : 0.0;
    L.C00 = (fx2 + fs * fs) * s;
    L.C02 = (fs * c - L.a * fx2) * s;
    L.C11 = fy2 * s;
    L.C12 = -(L.b * fy2) * s;
    L.C22 = (L.a * L.a * fx2 + L.b * L.b * fy2 + c * c) * s;
    return L;
}
// C t
__device__ __forceinline__ void lrec_C(const EdgeLin &L, const double t[3], double h[3])
{
    h[0] = L.C00 * t[0] + L.C02 * t[2];
    h[1] = L.C11 * t[1] + L.C12 * t[2];
    h[2] = L.C02 * t[0] + L.C12 * t[1] + L.C22 * t[2];
}
// J_pose^T omr = E^T (Pt^T omr) of a free-keyframe edge: its share of b_p (constructQuadraticForm, base_binary_edge.hpp:95-110), from the record
// and the omr the landmark side left (lomr): E^T g = (-(a, b, 1) x g, -iz g)
__device__ __forceinline__ void lrec_bp(const Cam &cam, const dbl4_t rec, const double o[3], double (&acc)[6])
{
    const double a = rec.x, b = rec.y, iz = rec.z;
    const bool stereo = rec.w < 0.0;
    const double fs = stereo ? cam.fx : 0.0, c = stereo ? cam.bf * iz - a * cam.fx : 0.0;
    const double g0 = cam.fx * o[0] + fs * o[2], g1 = cam.fy * o[1], g2 = c * o[2] - a * cam.fx * o[0] - b * cam.fy * o[1];
    acc[0] += g1 - b * g2;
    acc[1] += a * g2 - g0;
    acc[2] += b * g0 - a * g1;
    acc[3] += -(iz * g0);
    acc[4] += -(iz * g1);
    acc[5] += -(iz * g2);
}
// B^T xp of a free-keyframe edge (block_solver.hpp:455-480 multiplies by the stored Hpl block B):
// B^T xp = -R^T C E xp,  E xp = (a, b, 1) x omega - iz upsilon  for xp = (omega, upsilon)
__device__ __forceinline__ void lrec_backsub(const Cam &cam, const dbl4_t rec, const double R[9], const double xp[6], double v[3])
{
    const EdgeLin L = lrec_form(cam, rec);
    const double t[3] = {L.b * xp[2] - xp[1] - L.iz * xp[3], xp[0] - L.a * xp[2] - L.iz * xp[4], L.a * xp[1] - L.b * xp[0] - L.iz * xp[5]};
    double h[3];
    lrec_C(L, t, h);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = -(R[c] * h[0] + R[3 + c] * h[1] + R[6 + c] * h[2]);
}

// Landmark kernels: a 256-thread workgroup takes kLmBlock landmarks, kLmSlots threads each -- thread (landmark, slot j)
// works on the landmark's edges j, j + kLmSlots, ... (one edge for the usual <= 8 observations) and the landmark's first
// thread adds the per-edge terms in edge order, so the sums are the ones a thread walking the edges one after the other
// would form (the order g2o adds them in), while the chain of dependent gathers per thread is one edge long instead of
// the whole observation list (a single window has only ~2000 landmarks: the walk was pure latency).
// (kLmBlock = 32, kLmSlots = 8: lba_window.h)
// edges of a landmark fetched together by the one-thread-per-landmark kernels (measured on 32 windows of 24 k edges, 6
// observations per landmark: k_points_walk 43.4 us with 4 / 4, 38.6 with 6 / 6; the linearisation spills beyond 4)
constexpr int kWalkChunk = 4;     // free-keyframe edges (back-substitution)
constexpr int kWalkChunkE = 6;     // all edges (residuals)
constexpr int kWalkChunkLin = 4;   // all edges (linearisation)

// solve = 1 (a Levenberg-Marquardt trial): the landmark's part of
// BlockSolver::solve -- xl = (Hll + lambda I)^-1 (bl - B^T xp), block_solver.hpp:455-480 -- and of
// SparseOptimizer::update (X += xl), its scale terms x_j (lambda x_j + b_j), then computeActiveErrors +
// activeRobustChi2 (sparse_optimizer.cpp:61-114) of the landmark's edges at the new estimates (the poses were
// updated by the kernel before), and -- in the workgroup that finishes last -- the LM decision (lm_decide).
// solve = 0 (top of solve() in iteration 0): the residuals only.
// Landmark l leaves its chi2 terms in part[l] and its scale terms in part[nl + l] (canonical_sums adds them).
__global__ __launch_bounds__(256) void k_points(const LbaWin *__restrict__ wins, const SchurTask *__restrict__ tasks, int solve)
{
    __shared__ double s_v[kLmBlock][kLmSlots][3];
    __shared__ double s_X[kLmBlock][3];
    const SchurTask tk = tasks[blockIdx.x];
    const LbaWin &W = wins[tk.w];
    if (!(solve ? W.st->run : W.st->initp)) return;
    const int tid = threadIdx.x, ll = tid / kLmSlots, j = tid % kLmSlots;
    const int l = tk.code * kLmBlock + ll;
    const bool has = l < W.nl, leader = j == 0;
    const int n6 = 6 * W.np;
    double sc = 0, chi = 0;
    double *X = has ? W.point + 3 * (size_t)W.hpoint[l] : nullptr;
    double Xv[3] = {0, 0, 0};
    if (has)
        for (int r = 0; r < 3; ++r) Xv[r] = X[r];
    if (solve) {
        const double lambda = W.st->lambda;
        const int a0 = has ? W.pl_off[l] : 0, a1 = has ? W.pl_off[l + 1] : 0;
        double cl[3] = {0, 0, 0};
        if (has && leader)
            for (int r = 0; r < 3; ++r) cl[r] = W.b[n6 + 3 * l + r];
        for (int rd = 0; __syncthreads_or(a0 + kLmSlots * rd < a1); ++rd) {
            const int a = a0 + kLmSlots * rd + j;
            double v[3] = {0, 0, 0};
            if (a < a1) {   // B_i^T (-x_p) of one free-keyframe edge
                const int i1 = W.pl_ph[a];
                const dbl4_t rec = lrec_load(W, a);
                double xp[6], R[9];
#pragma unroll
                for (int r = 0; r < 6; ++r) xp[r] = -W.x[6 * i1 + r];
#pragma unroll
                for (int i = 0; i < 9; ++i) R[i] = W.Rl[9 * (size_t)i1 + i];
                lrec_backsub(W.cam, rec, R, xp, v);
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) s_v[ll][j][c] = v[c];
            __syncthreads();
            if (leader) {
                const int m = min(kLmSlots, a1 - (a0 + kLmSlots * rd));
                for (int jj = 0; jj < m; ++jj)
                    for (int c = 0; c < 3; ++c) cl[c] += s_v[ll][jj][c];
            }
        }
        if (has && leader) {
            // (Hll + lambda I)^-1: the same operations as in the Schur kernel, so the same bits
            double Dm[9], Dinv[9];
            for (int i = 0; i < 9; ++i) Dm[i] = W.Hll[9 * (size_t)l + i];
            Dm[0] += lambda; Dm[4] += lambda; Dm[8] += lambda;
            mat3_inverse(Dm, Dinv);
            double *Xb = W.bk + 7 * (size_t)W.n_poses + 3 * (size_t)W.hpoint[l];
            for (int r = 0; r < 3; ++r) {
                const double xl = Dinv[r * 3] * cl[0] + Dinv[r * 3 + 1] * cl[1] + Dinv[r * 3 + 2] * cl[2];
                W.x[n6 + 3 * l + r] = xl;
                store_dev(Xb + r, Xv[r]);   // push() (read back by the deciding workgroup when the step is rejected)
                Xv[r] += xl;
                store_dev(X + r, Xv[r]);   // (read back by the deciding workgroup when the step is rejected: the swap)
                s_X[ll][r] = Xv[r];
                sc += xl * (lambda * xl + W.b[n6 + 3 * l + r]);
            }
        }
        __syncthreads();
        if (has)
            for (int r = 0; r < 3; ++r) Xv[r] = s_X[ll][r];
    }
    {
        const int e0 = has ? W.pt_off[l] : 0, e1 = has ? W.pt_off[l + 1] : 0;
        for (int rd = 0; __syncthreads_or(e0 + kLmSlots * rd < e1); ++rd) {
            const int a = e0 + kLmSlots * rd + j;
            double c = 0;
            if (a < e1) {
                const int e = W.pt_k[a];
                if (!W.e_level1[e]) {   // an inactive edge keeps its _error (and adds nothing: chi2 >= 0, so + 0.0 is exact)
                    double p[3], er[3];
                    se3_map(W.pose + 7 * (size_t)W.e_pose[e], Xv, p);
                    const int stereo = W.e_stereo[e];
                    const double ob[3] = {(double)W.in_obs[3 * (size_t)e], (double)W.in_obs[3 * (size_t)e + 1], (double)W.in_obs[3 * (size_t)e + 2]};
                    edge_error(W.cam, p, ob, stereo, er);   // (_error is not stored: LmState::err_at)
                    c = edge_chi2(er, (double)W.in_w[e], stereo ? 3 : 2);
                    if (W.e_robust[e]) {
                        double rho[2];
                        robustify(c, stereo ? W.cam.delta_stereo : W.cam.delta_mono, rho);
                        c = rho[0];
                    }
                }
            }
            s_v[ll][j][0] = c;
            __syncthreads();
            if (leader) {
                const int m = min(kLmSlots, e1 - (e0 + kLmSlots * rd));
                for (int jj = 0; jj < m; ++jj) chi += s_v[ll][jj][0];
            }
        }
    }
    if (has && leader) {
        store_dev(W.part + l, chi);
        store_dev(W.part + W.nl + l, sc);
    }
    if (solve) points_tail<256>(W);
}

// The keyframe state of the window a landmark workgroup of the walks belongs to, staged in LDS: the poses (7 doubles each) and, for a
// trial's back-substitution, the update x (6) and the linearisation's rotation Rl (9) of every free keyframe -- at most ~80 keyframes
// that every edge of the workgroup's landmarks gathers from.  The last level of the walks' dependent gathers then reads LDS.
// A window whose state is larger than kWalkLdsBytes reads device memory as before (a choice per workgroup; both from one body).
// 16 KB per workgroup: with 12 waves per compute unit (three per SIMD) that is 3 workgroups of k_lin / 6 of k_points_walk, 48 / 96 of
// the unit's 160 KB -- the registers bound the residency, not the LDS.  (kWalkLdsBytes, walk_lds_bytes: lba_window.h)
extern __shared__ double walk_sm[];   // the dynamic LDS of k_points_walk and k_lin<true>
__device__ __forceinline__ void walk_stage(const LbaWin &W, double *sm, bool with_x)
{
    const int n7 = 7 * W.n_poses, n6 = 6 * W.np, n9 = 9 * W.np;
    for (int i = threadIdx.x; i < n7; i += blockDim.x) sm[i] = W.pose[i];
    if (with_x) {
        for (int i = threadIdx.x; i < n6; i += blockDim.x) sm[n7 + i] = W.x[i];
        for (int i = threadIdx.x; i < n9; i += blockDim.x) sm[n7 + n6 + i] = W.Rl[i];
    }
    __syncthreads();
}

// The same work with one thread per landmark walking its edges (128-thread workgroups): the layout for many windows per
// launch, where the landmarks alone fill the device and idle slots, barriers and LDS round trips only cost (32 windows of
// 24 k edges: 4.4 ms against 6.4 ms).  Per landmark the operations and their order are those of k_points, so both layouts
// leave the same bits.
template <bool kLds>
__device__ __forceinline__ void points_walk_body(const LbaWin &W, int l, int solve, int hp, int a0, int a1, int e0, int e1)
{
    const int n6 = 6 * W.np;
    const double *s_pose = walk_sm, *s_x = walk_sm + 7 * W.n_poses, *s_Rl = s_x + n6;
    double sc = 0, chi = 0;
    double *X = W.point + 3 * (size_t)hp;
    double Xv[3] = {X[0], X[1], X[2]};
    if (solve) {
        const double lambda = W.st->lambda;
        double cl[3] = {W.b[n6 + 3 * l], W.b[n6 + 3 * l + 1], W.b[n6 + 3 * l + 2]};
        // The walk is a chain of dependent gathers (edge list -> edge -> keyframe); kWalkChunk edges are fetched level by
        // level together, then their terms are added in edge order (the same sums, a quarter of the round trips).
        for (int a = a0; a < a1; a += kWalkChunk) {
            int ka[kWalkChunk], i1[kWalkChunk];   // (positions in the list = the indices of the dense Hpl array)
#pragma unroll
            for (int u = 0; u < kWalkChunk; ++u) ka[u] = min(a + u, a1 - 1);
#pragma unroll
            for (int u = 0; u < kWalkChunk; ++u) i1[u] = W.pl_ph[ka[u]];
            dbl4_t rec[kWalkChunk];
            double xp[kWalkChunk][6], Rr[kWalkChunk][9];
#pragma unroll
            for (int u = 0; u < kWalkChunk; ++u) rec[u] = lrec_load(W, ka[u]);
#pragma unroll
            for (int u = 0; u < kWalkChunk; ++u) {
#pragma unroll
                for (int r = 0; r < 6; ++r) xp[u][r] = -(kLds ? s_x[6 * i1[u] + r] : W.x[6 * i1[u] + r]);
#pragma unroll
                for (int i = 0; i < 9; ++i) Rr[u][i] = kLds ? s_Rl[9 * i1[u] + i] : W.Rl[9 * (size_t)i1[u] + i];
            }
#pragma unroll
            for (int u = 0; u < kWalkChunk; ++u) {
                if (a + u >= a1) break;
                double v[3];
                lrec_backsub(W.cam, rec[u], Rr[u], xp[u], v);
                for (int c = 0; c < 3; ++c) cl[c] += v[c];
            }
        }
        double Dm[9], Dinv[9];
        for (int i = 0; i < 9; ++i) Dm[i] = W.Hll[9 * (size_t)l + i];
        Dm[0] += lambda; Dm[4] += lambda; Dm[8] += lambda;
        mat3_inverse(Dm, Dinv);
        double *Xb = W.bk + 7 * (size_t)W.n_poses + 3 * (size_t)hp;
        for (int r = 0; r < 3; ++r) {
            const double xl = Dinv[r * 3] * cl[0] + Dinv[r * 3 + 1] * cl[1] + Dinv[r * 3 + 2] * cl[2];
            W.x[n6 + 3 * l + r] = xl;
            store_dev(Xb + r, Xv[r]);   // push()
            Xv[r] += xl;
            store_dev(X + r, Xv[r]);
            sc += xl * (lambda * xl + W.b[n6 + 3 * l + r]);
        }
    }
    for (int a = e0; a < e1; a += kWalkChunkE) {
        // the edges' records lie at their positions in the list (EdgeRec): one level of loads, then the keyframes
        flt4_t lo[kWalkChunkE];
        int4_t hi[kWalkChunkE];
        double T[kWalkChunkE][7];
#pragma unroll
        for (int u = 0; u < kWalkChunkE; ++u) erec_load(W, min(a + u, e1 - 1), lo[u], hi[u]);
#pragma unroll
        for (int u = 0; u < kWalkChunkE; ++u)
#pragma unroll
            for (int i = 0; i < 7; ++i) T[u][i] = kLds ? s_pose[7 * hi[u].x + i] : W.pose[7 * (size_t)hi[u].x + i];
#pragma unroll
        for (int u = 0; u < kWalkChunkE; ++u) {
            if (a + u >= e1) break;
            const uint32_t fl = (uint32_t)hi[u].z;
            if (fl & kEdgeLevel1) continue;   // an inactive edge keeps its _error
            double p[3], er[3];
            se3_map(T[u], Xv, p);
            const int stereo = fl & kEdgeStereo;
            const double ob[3] = {(double)lo[u].x, (double)lo[u].y, (double)lo[u].z};
            edge_error(W.cam, p, ob, stereo, er);   // (_error is not stored: LmState::err_at)
            double c = edge_chi2(er, (double)lo[u].w, stereo ? 3 : 2);
            if (fl & kEdgeRobust) {
                double rho[2];
                robustify(c, stereo ? W.cam.delta_stereo : W.cam.delta_mono, rho);
                c = rho[0];
            }
            chi += c;
        }
    }
    store_dev(W.part + l, chi);
    store_dev(W.part + W.nl + l, sc);
}

__global__ __launch_bounds__(128) void k_points_walk(const LbaWin *__restrict__ wins, const SchurTask *__restrict__ tasks, int solve)
{
    const SchurTask tk = tasks[blockIdx.x];
    const LbaWin &W = wins[tk.w];
    if (!(solve ? W.st->run : W.st->initp)) return;
    const int l = tk.code * blockDim.x + threadIdx.x;
    const bool has = l < W.nl;
    // the landmark's first-level loads are requested before the keyframe state is staged: they travel together
    int hp = 0, a0 = 0, a1 = 0, e0 = 0, e1 = 0;
    if (has) {
        hp = W.hpoint[l];
        e0 = W.pt_off[l];
        e1 = W.pt_off[l + 1];
        if (solve) {
            a0 = W.pl_off[l];
            a1 = W.pl_off[l + 1];
        }
    }
    const bool lds = walk_lds_bytes(W.n_poses, W.np) <= kWalkLdsBytes;   // (the same for every thread of the workgroup)
    if (lds) {
        walk_stage(W, walk_sm, solve != 0);
        if (has) points_walk_body<true>(W, l, solve, hp, a0, a1, e0, e1);
    } else if (has)
        points_walk_body<false>(W, l, solve, hp, a0, a1, e0, e1);
    if (solve) points_tail<128>(W);
}

// robustified information of an edge (BaseBinaryEdge::constructQuadraticForm, base_binary_edge.hpp:55-120):
// omr = -rho' Omega e, wo = rho' * w
__device__ __forceinline__ void edge_weights_of(const Cam &cam, const double er[3], double w, int robust, int stereo, double omr[3], double &wo)
{
    // static indices only (a runtime-length loop over D would put the arrays in scratch memory)
    omr[0] = -(w * er[0]);
    omr[1] = -(w * er[1]);
    omr[2] = stereo ? -(w * er[2]) : 0.0;
    wo = w;
    if (robust) {
        double rho[2];
        robustify(edge_chi2(er, w, stereo ? 3 : 2), stereo ? cam.delta_stereo : cam.delta_mono, rho);
        wo = rho[1] * w;
        omr[0] *= rho[1];
        omr[1] *= rho[1];
        if (stereo) omr[2] *= rho[1];
    }
}
// ... of edge k whose landmark maps to p in its keyframe: the residual is re-formed from p and the observation (the same
// operations on the same values as the residual pass that stored _error: the same bits, for 12 bytes of observation instead
// of 24 of stored residual)
__device__ __forceinline__ void edge_weights(const LbaWin &W, int k, const double p[3], int stereo, double omr[3], double &wo)
{
    const double ob[3] = {(double)W.in_obs[3 * (size_t)k], (double)W.in_obs[3 * (size_t)k + 1], (double)W.in_obs[3 * (size_t)k + 2]};
    double er[3];
    edge_error(W.cam, p, ob, stereo, er);
    edge_weights_of(W.cam, er, (double)W.in_w[k], W.e_robust[k], stereo, omr, wo);
}

// buildSystem, the landmarks' side (block_solver.hpp:502-560), kLmBlock landmarks per workgroup (see k_points): thread
// (landmark, slot) linearises one edge at a time -- linearizeOplus, Ji^T Omega Ji, Ji^T omr, and the edge's Hpl block
// Jj^T Omega Ji -- and the landmark's first thread adds the terms in insertion order like g2o: Hll, b_l.
// A masked edge adds nothing (its Hpl block was zeroed when it was masked).
__device__ __forceinline__ void lin_points_body(const LbaWin &W, int blk)
{
    __shared__ double s_c[kLmBlock][kLmSlots][12 + 1];
    const int tid = threadIdx.x, ll = tid / kLmSlots, j = tid % kLmSlots;
    const int l = blk * kLmBlock + ll;
    const bool has = l < W.nl, leader = j == 0;
    double Xv[3] = {0, 0, 0};
    if (has) {
        const double *X = W.point + 3 * (size_t)W.hpoint[l];
        for (int r = 0; r < 3; ++r) Xv[r] = X[r];
    }
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
    const int a0 = has ? W.pt_off[l] : 0, a1 = has ? W.pt_off[l + 1] : 0;
    for (int rd = 0; __syncthreads_or(a0 + kLmSlots * rd < a1); ++rd) {
        const int a = a0 + kLmSlots * rd + j;
        double cH[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, cb[3] = {0, 0, 0};
        const int k = a < a1 ? W.pt_k[a] : -1;
        if (k >= 0 && !W.e_level1[k]) {
            const double *T = W.pose + 7 * (size_t)W.e_pose[k];
            const int stereo = W.e_stereo[k];
            double p[3], R[9];
            se3_map(T, Xv, p);
            rot_from_quat(T, R);
            double Ja[9];
            jac_point(W.cam, R, p, stereo, Ja);
            double omr[3], wo;
            edge_weights(W, k, p, stereo, omr, wo);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                cb[r] = Ja[r] * omr[0] + Ja[3 + r] * omr[1] + Ja[6 + r] * omr[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) cH[r * 3 + c] = Ja[r] * wo * Ja[c] + Ja[3 + r] * wo * Ja[3 + c] + Ja[6 + r] * wo * Ja[6 + c];
            }
            const int pp = W.pl_pos[k];
            if (pp >= 0) lrec_store(W, pp, p, wo, stereo, omr);
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) s_c[ll][j][i] = cH[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) s_c[ll][j][9 + i] = cb[i];
        __syncthreads();
        if (leader) {
            const int m = min(kLmSlots, a1 - (a0 + kLmSlots * rd));
            for (int jj = 0; jj < m; ++jj) {
#pragma unroll
                for (int i = 0; i < 9; ++i) H[i] += s_c[ll][jj][i];
#pragma unroll
                for (int i = 0; i < 3; ++i) bl[i] += s_c[ll][jj][9 + i];
            }
        }
    }
    if (has && leader) {
        for (int i = 0; i < 9; ++i) W.Hll[9 * (size_t)l + i] = H[i];
        for (int i = 0; i < 3; ++i) W.b[6 * (size_t)W.np + 3 * (size_t)l + i] = bl[i];
    }
}

// the same with one thread per landmark walking its edges (see k_points_walk); the per-edge terms are formed and added in
// the same order, so Hll, b_l and Hpl carry the same bits
template <bool kLds>
__device__ __forceinline__ void lin_points_walk(const LbaWin &W, int l)
{
    const double *s_pose = walk_sm;
    const int e0 = W.pt_off[l], e1 = W.pt_off[l + 1];
    const double *X = W.point + 3 * (size_t)W.hpoint[l];
    const double Xv[3] = {X[0], X[1], X[2]};
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, bl[3] = {0, 0, 0};
    for (int a = e0; a < e1; a += kWalkChunkLin) {
        // kWalkChunkLin edges fetched level by level together (see k_points_walk), linearised and added in edge order
        flt4_t lo[kWalkChunkLin];
        int4_t hi[kWalkChunkLin];
        double T[kWalkChunkLin][7];
#pragma unroll
        for (int u = 0; u < kWalkChunkLin; ++u) erec_load(W, min(a + u, e1 - 1), lo[u], hi[u]);
#pragma unroll
        for (int u = 0; u < kWalkChunkLin; ++u)
#pragma unroll
            for (int i = 0; i < 7; ++i) T[u][i] = kLds ? s_pose[7 * hi[u].x + i] : W.pose[7 * (size_t)hi[u].x + i];
#pragma unroll
        for (int u = 0; u < kWalkChunkLin; ++u) {
            if (a + u >= e1) break;
            const uint32_t fl = (uint32_t)hi[u].z;
            if (fl & kEdgeLevel1) continue;
            const int stereo = fl & kEdgeStereo;
            const double ob[3] = {(double)lo[u].x, (double)lo[u].y, (double)lo[u].z};   // (the observation; the residual is re-formed below)
            double p[3], R[9];
            se3_map(T[u], Xv, p);
            rot_from_quat(T[u], R);
            double Ja[9];
            jac_point(W.cam, R, p, stereo, Ja);
            double omr[3], wo;
            double res[3];
            edge_error(W.cam, p, ob, stereo, res);
            edge_weights_of(W.cam, res, (double)lo[u].w, (fl & kEdgeRobust) != 0, stereo, omr, wo);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                bl[r] += Ja[r] * omr[0] + Ja[3 + r] * omr[1] + Ja[6 + r] * omr[2];
#pragma unroll
                for (int c = 0; c < 3; ++c) H[r * 3 + c] += Ja[r] * wo * Ja[c] + Ja[3 + r] * wo * Ja[3 + c] + Ja[6 + r] * wo * Ja[6 + c];
            }
            if (hi[u].y >= 0) lrec_store(W, hi[u].y, p, wo, stereo, omr);
        }
    }
    // (the addresses below are formed here, from the index alone: formed ahead of the loop -- for both forms of the body at once -- they
    // hold two registers across it, which at this kernel's 168 registers for three waves per SIMD is 12 bytes of scratch: tools/lba_kernel_resources.py)
    asm volatile("" : "+v"(l));
    for (int i = 0; i < 9; ++i) W.Hll[9 * (size_t)l + i] = H[i];
    for (int i = 0; i < 3; ++i) W.b[6 * (size_t)W.np + 3 * (size_t)l + i] = bl[i];
}

// acc[K] of every thread of an NT-thread workgroup -> their sums (returned in threads e < K).  16-lane DPP row sums (as a
// reduce-scatter: the lanes of a row share the K totals and each writes its own), then
// the row totals of each value through LDS in row order: a fixed order (bit-reproducible), NT / 16 x K doubles of LDS.
// n_items = work items of the workgroup (thread t had one iff t < n_items): waves without any skip their share, and rows
// without any are left out of the final sums (they would add +0.0).
template <int K, int NT = 256>
__device__ __forceinline__ double workgroup_sum_k256(double (&acc)[K], double *red /* (NT / 16) x (K + 1) */, int n_items)
{
    const int row = threadIdx.x >> 4, wave = threadIdx.x >> 6;
    const int rows_used = min(NT / 16, (n_items + 15) >> 4);
    if (wave * 64 < n_items) {   // wave-uniform
        row_sums_scatter_f64<K>(acc);
        row_scatter_store<K>(acc, red + row * (K + 1));
    }
    __syncthreads();
    double sum = 0;
    if ((int)threadIdx.x < K)
        for (int r = 0; r < rows_used; ++r) sum += red[r * (K + 1) + threadIdx.x];
    return sum;
}

// buildSystem, the keyframes' side: Hpp += Jj^T Omega Jj, b_p += Jj^T omr.  One 256-thread workgroup per free pose:
// thread j takes the pose's edges j, j + 256, ... (the Jacobian is recomputed from the estimates: no per-edge arrays;
// few edges per thread keep the chain of dependent gathers short), then workgroup_sum_k256 (fixed order).
// (The former 256 x 43 tree in LDS held 88 KB per pose -- one workgroup per compute unit.)
__device__ __forceinline__ void lin_poses_body(const LbaWin &W, int ph, int init)
{
    __shared__ double red[16 * 43];
    if (ph >= W.np) return;
    double T[7];
    {
        const double *Tp = W.pose + 7 * (size_t)W.hpose[ph];
#pragma unroll
        for (int i = 0; i < 7; ++i) T[i] = Tp[i];
    }
    if (threadIdx.x == 0) {   // the rotation the landmark side linearises at (the same function of the same values)
        double R[9];
        rot_from_quat(T, R);
#pragma unroll
        for (int i = 0; i < 9; ++i) W.Rl[9 * (size_t)ph + i] = R[i];
    }
    // Hpp and b_p themselves are formed by k_schur's diagonal units from the landmark side's records (schur_item<true>, lrec_bp); only the
    // first linearisation of an optimisation needs them here: k_lm_init takes lambda from the diagonal of Hpp before any Schur launch
    if (!init) return;
    double acc[42];
#pragma unroll
    for (int i = 0; i < 42; ++i) acc[i] = 0;
    for (int a = W.ps_off[ph] + threadIdx.x; a < W.ps_off[ph + 1]; a += 256) {
        const int k = W.ps_k[a];
        if (W.e_level1[k]) continue;
        const int stereo = W.e_stereo[k];
        double p[3], Jb[18], omr[3], wo;
        se3_map(T, W.point + 3 * (size_t)W.e_point[k], p);
        jac_pose(W.cam, p, stereo, Jb);
        edge_weights(W, k, p, stereo, omr, wo);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            acc[36 + r] += Jb[r] * omr[0] + Jb[6 + r] * omr[1] + Jb[12 + r] * omr[2];
#pragma unroll
            for (int c = 0; c < 6; ++c) acc[r * 6 + c] += Jb[r] * wo * Jb[c] + Jb[6 + r] * wo * Jb[6 + c] + Jb[12 + r] * wo * Jb[12 + c];
        }
    }
    const double sum = workgroup_sum_k256<42>(acc, red, W.ps_off[ph + 1] - W.ps_off[ph]);
    if (threadIdx.x < 36)
        W.Hpp[36 * (size_t)ph + threadIdx.x] = sum;
    else if (threadIdx.x < 42)
        W.b[6 * (size_t)ph + (threadIdx.x - 36)] = sum;
}

// buildSystem as ONE launch: the landmark side and the keyframe side are independent of each other.  The task list holds the
// landmark blocks of all windows (block by block across the windows), then one task per free keyframe, so the landmark
// workgroups of ALL windows start before any keyframe workgroup: their walks are the long
// dependent chains of the launch (33 of its 54 us on 32 windows when they queued behind the keyframe workgroups of the
// windows before them), the keyframe workgroups fill in behind.
// (three waves per SIMD, asked for: the walk gained from the third wave, 36.2 -> 34.4 us on 32 windows.  168 registers, no scratch; k_points_walk
// reaches three waves unasked, at 166.  What keeps both at that limit depends on the register allocator: tools/lba_kernel_resources.py checks it.)
template <bool kWalk>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_lin(const LbaWin *__restrict__ wins, const SchurTask *__restrict__ tasks, int init)
{
    const SchurTask tk = tasks[blockIdx.x];
    const LbaWin &W = wins[tk.w];
    if (!(init ? W.st->initp : W.st->lin)) return;
    const int blk = tk.code & 0x0fffffff;
    const bool keyframe = (tk.code >> 28) != 0;
    if (keyframe)
        lin_poses_body(W, blk, init);
    else if (kWalk) {
        const int l = blk * 256 + threadIdx.x;
        const bool has = l < W.nl;
        // (the landmark's own first loads are not requested ahead of the staging as in k_points_walk: the three registers they hold across
        // it cost this kernel 20 bytes of scratch)
        if (walk_lds_bytes(W.n_poses, W.np) <= kWalkLdsBytes) {
            walk_stage(W, walk_sm, false);
            if (has) lin_points_walk<true>(W, l);
        } else if (has)
            lin_points_walk<false>(W, l);
    } else
        lin_points_body(W, blk);
}

// top of solve() in iteration 0 (levenberg.cpp:75-97): currentChi, lambda = 1e-5 * max |H_jj| over all free vertices
// (computeLambdaInit :166-180), ni = 2; the first trial's push() (the backup of the estimates)
__global__ __launch_bounds__(1024) void k_lm_init(const LbaWin *__restrict__ wins)
{
    __shared__ double sh[1024];
    const LbaWin &W = wins[blockIdx.x];
    LmState *st = W.st;
    if (!st->initp) return;
    const int n6 = 6 * W.np, n = n6 + 3 * W.nl;
    double acc = 0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        double v;
        if (i < n6)
            v = W.Hpp[36 * (size_t)(i / 6) + (i % 6) * 7];
        else {
            const int j = i - n6;
            v = W.Hll[9 * (size_t)(j / 3) + (j % 3) * 4];
        }
        acc = fmax(acc, fabs(v));
    }
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
        __syncthreads();
    }
    for (int i = threadIdx.x; i < W.est_n; i += 1024) W.bk[i] = W.pose[i];
    double chi, unused;
    canonical_sums(W, false, chi, unused);
    if (threadIdx.x == 0) {
        st->currentChi = st->iniChi = chi;
        st->lambda = 1e-5 * sh[0];
        st->ni = 2;
        st->nBad = 0;
        st->it = 0;
        st->qmax = 0;
        st->initp = 0;
        st->lin = 0;
        st->run = 1;
        st->err_at = 1;   // (the residual pass before this launch)
    }
}

// ---- Schur complement (block_solver.hpp:379-432), one 256-thread workgroup per (pose, pose) block of the upper block
// triangle.  The host ranks the items -- (landmark, free-pose edges ka <= kb of it) -- by their block, landmark order
// inside a block (build_schur_items).  Thread j of the block takes the items j, j + 256, ...: (Hll + lambda I)^-1 of the
// landmark, B_a Dinv B_b^T (and, on the diagonal blocks, the coefficient term B_a Dinv b_l), accumulated in registers;
// the partial 6x6 sums are added by workgroup_sum_k256: no atomics, a fixed order (bit-reproducible), and no per-item
// array in memory (a materialised item list cost 288 B written + read per
// item: 0.31 ms per trial for 32 windows of 24 k edges).  Hschur = Hpp + lambda I - sum, bschur = b_p - sum.
// threads per block: measured (one 12 k-edge window / one 24 k-edge window / 32 windows of 24 k edges, whole solve):
// 64: 1.88 / 2.27 / 4.42 ms, 128: 1.74 / 1.92 / 4.35 ms, 256: 1.71 / 1.87 / 4.78 ms (most off-diagonal blocks hold < 128 items)
constexpr int kSchurThreads = 256;
// Work units of k_schur, one 256-thread workgroup each (build_schur_units ranks them, the host lays the units of all windows of
// the call out as ONE task list -- no grid padded to the largest window, no workgroup that only finds out it has nothing to do):
//   DIAG  a diagonal (pose, pose) block: every observation of a keyframe, hundreds to thousands of items, strided over the
//         256 threads, sums through workgroup_sum_k256;
//   BIG   an off-diagonal block of more than 256 items, the same way;
//   PACK  16 ROWS of 16 lanes; a row holds up to 16 consecutive items of ONE off-diagonal block (a block of n items takes
//         ceil(n / 16) consecutive rows of one unit), one item per thread: the covisible landmarks of most keyframe pairs are a
//         few dozen, often fewer than 16 -- one wave per block left 40-85 % of the lanes idle and a window of 40 free keyframes
//         cost 235 workgroups.  Row sums by DPP, then a block's rows are added in row order: for a block of up to 64 items
//         exactly the sums (and bits) of the one-wave-per-block form.
// (kSchurDiag = 0, kSchurBig = 1, kSchurPack = 2: lba_window.h;
// SchurTask.code = kind << 28 | argument -- DIAG: i; BIG: block rank; PACK: first row; w = -1: padding of the XCD interleave)
// one item: (Hll + lambda I)^-1 of the landmark, and B_a D^-1 B_b^T in factored form.  With B = -E^T C R (lrec_form)
//     B_a D^-1 B_b^T = E_a^T Q E_b,   Q = C_a (R_a D^-1 R_b^T) C_b   (3 x 3),
// and the products with E = [ [a b 1]x | -iz I ] are cross products: the two 144-byte blocks are neither stored nor fetched --
// each side is its 32-byte record (LbaWin::lrec) and the keyframe's rotation (uniform over the block: a broadcast load) --
// and an item takes ~360 operations instead of the ~350 of the stored-block form plus 23 divergent 16-byte requests (9 now).
__device__ __forceinline__ double sf(double a, double b, double c) { return a * b + c; }
template <bool kDiag>
__device__ __forceinline__ void schur_item(const LbaWin &W, int j, double lambda, int n6, const double *__restrict__ Ra_g,
                                           const double *__restrict__ Rb_g, double (&acc)[42])
{
    const int ka = W.it_ka[j], kb = W.it_kb[j], l = W.it_l[j];   // three independent loads, then one level of gathers
    const dbl4_t rb = lrec_load(W, kb);
    const dbl4_t ra = kDiag ? rb : lrec_load(W, ka);             // (diagonal block: the two edges of an item are one)
    double D[9], Dinv[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) D[i] = W.Hll[9 * (size_t)l + i];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    mat3_inverse(D, Dinv);
    double Ra[9], G[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) Ra[i] = Ra_g[i];
    {
        double G0[9];   // R_a D^-1
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G0[r * 3 + c] = sf(Ra[r * 3 + 2], Dinv[6 + c], sf(Ra[r * 3 + 1], Dinv[3 + c], Ra[r * 3] * Dinv[c]));
        if (kDiag) {   // the coefficient term B_a D^-1 b_l = -E_a^T C_a (R_a D^-1 b_l)
            const double *bl = W.b + n6 + 3 * (size_t)l;
            const double b0 = bl[0], b1 = bl[1], b2 = bl[2];
            const EdgeLin La = lrec_form(W.cam, ra);
            const double t[3] = {G0[0] * b0 + G0[1] * b1 + G0[2] * b2, G0[3] * b0 + G0[4] * b1 + G0[5] * b2, G0[6] * b0 + G0[7] * b1 + G0[8] * b2};
            double h[3];
            lrec_C(La, t, h);
            acc[36] += La.b * h[2] - h[1];
            acc[37] += h[0] - La.a * h[2];
            acc[38] += La.a * h[1] - La.b * h[0];
            acc[39] += La.iz * h[0];
            acc[40] += La.iz * h[1];
            acc[41] += La.iz * h[2];
        }
        double Rb[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) Rb[i] = kDiag ? Ra[i] : Rb_g[i];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) G[r * 3 + c] = sf(G0[r * 3 + 2], Rb[c * 3 + 2], sf(G0[r * 3 + 1], Rb[c * 3 + 1], G0[r * 3] * Rb[c * 3]));
    }
    const EdgeLin La = lrec_form(W.cam, ra), Lb = kDiag ? La : lrec_form(W.cam, rb);
    double Q[9];
    {
        double CG[9];   // C_a G
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            CG[c] = sf(La.C02, G[6 + c], La.C00 * G[c]);
            CG[3 + c] = sf(La.C12, G[6 + c], La.C11 * G[3 + c]);
            CG[6 + c] = sf(La.C22, G[6 + c], sf(La.C12, G[3 + c], La.C02 * G[c]));
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            Q[r * 3] = sf(CG[r * 3 + 2], Lb.C02, CG[r * 3] * Lb.C00);
            Q[r * 3 + 1] = sf(CG[r * 3 + 2], Lb.C12, CG[r * 3 + 1] * Lb.C11);
            Q[r * 3 + 2] = sf(CG[r * 3 + 2], Lb.C22, sf(CG[r * 3 + 1], Lb.C12, CG[r * 3] * Lb.C02));
        }
    }
    if (kDiag) {   // the edge's own Hpp term J_pose^T w J_pose = E^T (w Pt^T Pt) E = E^T (C / iz) E enters with the other sign: the
                   // diagonal block is Hpp - sum B D^-1 B^T = -sum E^T (Q - w Pt^T Pt) E, so the keyframe side of the linearisation
                   // (a second pass over every free-keyframe edge: map, Jacobian, 126 products) is not needed after the first one
        const double w = fabs(ra.w), fx2 = W.cam.fx * W.cam.fx, fy2 = W.cam.fy * W.cam.fy;
        const bool st = ra.w < 0.0;
        const double fs = st ? W.cam.fx : 0.0, c = st ? W.cam.bf * La.iz - La.a * W.cam.fx : 0.0;
        const double P00 = (fx2 + fs * fs) * w, P02 = (fs * c - La.a * fx2) * w, P11 = fy2 * w, P12 = -(La.b * fy2) * w;
        const double P22 = (La.a * La.a * fx2 + La.b * La.b * fy2 + c * c) * w;
        Q[0] -= P00; Q[2] -= P02; Q[4] -= P11; Q[5] -= P12; Q[6] -= P02; Q[7] -= P12; Q[8] -= P22;
    }
    // U = Q E_b (3 x 6), then E_a^T U: rows 0-2 = [a b 1]x^T U, rows 3-5 = -iz_a U
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        double u[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double q0 = Q[r * 3], q1 = Q[r * 3 + 1], q2 = Q[r * 3 + 2];
            u[r] = c == 0 ? q1 - Lb.b * q2 : c == 1 ? Lb.a * q2 - q0 : c == 2 ? Lb.b * q0 - Lb.a * q1 : -(Lb.iz * Q[r * 3 + (c - 3)]);
        }
        // (a diagonal block is symmetric -- E^T (Q - w Pt^T Pt) E with a symmetric middle --: its unit forms the upper triangle only and
        // stores both; the six slots that frees, (1,0) (2,0) (2,1) (3,0) (3,1) (3,2), carry b_p below)
        acc[c] += u[1] - La.b * u[2];
        if (!kDiag || c >= 1) acc[6 + c] += La.a * u[2] - u[0];
        if (!kDiag || c >= 2) acc[12 + c] += La.b * u[0] - La.a * u[1];
        if (!kDiag || c >= 3) acc[18 + c] += -(La.iz * u[0]);
        if (!kDiag || c >= 4) acc[24 + c] += -(La.iz * u[1]);
        if (!kDiag || c >= 5) acc[30 + c] += -(La.iz * u[2]);
    }
    if (kDiag) {   // b_p += J_pose^T omr = E^T (Pt^T omr) (lrec_bp), omr as the landmark side left it
        const double o[3] = {W.lomr[3 * (size_t)kb], W.lomr[3 * (size_t)kb + 1], W.lomr[3 * (size_t)kb + 2]};
        double bp[6] = {0, 0, 0, 0, 0, 0};
        lrec_bp(W.cam, ra, o, bp);
        acc[6] += bp[0]; acc[12] += bp[1]; acc[13] += bp[2]; acc[18] += bp[3]; acc[19] += bp[4]; acc[20] += bp[5];
    }
}

// Hschur = Hpp + lambda I - sum (diagonal), -sum (off-diagonal, both triangles); bschur = b_p - sum
__device__ __forceinline__ void schur_store(const LbaWin &W, int i1, int i2, int e, double sum, double lambda)
{
    const bool diag = i1 == i2;
    if (e < 36) {
        double v = -sum;
        const int r = e / 6, c = e - 6 * r;
        if (diag && r == c) v += lambda;   // (Hpp is inside the diagonal unit's sum: schur_item<true>)
        W.Hs[(size_t)(6 * i1 + r) * W.hs_ld + 6 * i2 + c] = v;
        if (!diag) W.Hs[(size_t)(6 * i2 + c) * W.hs_ld + 6 * i1 + r] = v;
    }
    // (bschur of a diagonal unit: k_schur, after its b_p pass)
}

// three workgroups per compute unit (one wave of a workgroup per SIMD)
__global__ __launch_bounds__(kSchurThreads) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_schur(const LbaWin *__restrict__ wins, const SchurTask *__restrict__ tasks)
{
    constexpr int NT = kSchurThreads;
    __shared__ double red[(NT / 16) * 43];
    __shared__ int32_t s_info[16], s_ij[16];
    const SchurTask tk = tasks[blockIdx.x];
    if (tk.w < 0) return;
    const LbaWin &W = wins[tk.w];
    // (every dependent load is a round trip of its own on the workgroup's critical path: the state words and the unit's
    // item range are requested together, before the branch on the first of them)
    const int run = W.st->run;
    const double lambda = W.st->lambda;
    const int np = W.np, n6 = 6 * np;
    const int kind = tk.code >> 28, arg = tk.code & 0x0fffffff;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double acc[42];
#pragma unroll
    for (int i = 0; i < 42; ++i) acc[i] = 0;
    if (kind == kSchurPack) {
        const int row = tid >> 4, li = tid & 15, r = arg + row;
        int o0 = 0, info = 0, ij = 0;
        if (r < W.n_srows) {
            o0 = W.sr_o0[r];
            info = W.sr_info[r];
            ij = W.sr_ij[r];
        }
        if (!run) return;
        if (li == 0) {
            s_info[row] = info;
            s_ij[row] = ij;
        }
        if (li < (info & 255)) schur_item<false>(W, o0 + li, lambda, n6, W.Rl + 9 * (size_t)(ij & 0xffff), W.Rl + 9 * (size_t)(ij >> 16), acc);
        row_sums_scatter_f64<36>(acc);
        row_scatter_store<36>(acc, red + row * 43);
        __syncthreads();
        // a block's rows are neighbours inside the unit: its first row's slot adds them in row order
        for (int rr = wave; rr < 16; rr += NT / 64) {
            const int inf = s_info[rr], nrb = (inf >> 16) & 255;
            if (((inf >> 8) & 255) != 0 || nrb == 0 || lane >= 36) continue;
            double sum = 0;
            for (int k = 0; k < nrb; ++k) sum += red[(rr + k) * 43 + lane];
            schur_store(W, s_ij[rr] & 0xffff, s_ij[rr] >> 16, lane, sum, lambda);
        }
        return;
    }
    // DIAG / BIG: one block, items strided over the workgroup
    int i1, i2;
    if (kind == kSchurDiag)
        i1 = i2 = arg;
    else {   // block rank -> (i1 < i2), row-major upper triangle (the order of blk_off)
        int rem = arg;
        i1 = 0;
        while (rem >= np - i1) {
            rem -= np - i1;
            ++i1;
        }
        i2 = i1 + rem;
    }
    const int blk = i1 * np - i1 * (i1 - 1) / 2 + (i2 - i1);
    const int o0 = W.blk_off[blk], n = W.blk_off[blk + 1] - o0;
    if (!run) return;
    if (kind == kSchurDiag)
        for (int j = tid; j < n; j += NT) schur_item<true>(W, o0 + j, lambda, n6, W.Rl + 9 * (size_t)i1, W.Rl + 9 * (size_t)i1, acc);
    else
        for (int j = tid; j < n; j += NT) schur_item<false>(W, o0 + j, lambda, n6, W.Rl + 9 * (size_t)i1, W.Rl + 9 * (size_t)i2, acc);
    const double sum = workgroup_sum_k256<42, NT>(acc, red, n);
    if (kind != kSchurDiag) {
        schur_store(W, i1, i2, tid, sum, lambda);
        return;
    }
    // diagonal unit: Hschur_ii = lambda I - (upper-triangle sums, mirrored); b_p from its six slots; bschur = b_p - sum B D^-1 b_l
    __shared__ double s_bsum[6];
    if (tid >= 36 && tid < 42) s_bsum[tid - 36] = sum;
    __syncthreads();
    if (tid < 36) {
        const int r = tid / 6, c = tid - 6 * r;
        if (r <= c) {
            double v = -sum;
            if (r == c) v += lambda;
            W.Hs[(size_t)(6 * i1 + r) * W.hs_ld + 6 * i1 + c] = v;
            if (r != c) W.Hs[(size_t)(6 * i1 + c) * W.hs_ld + 6 * i1 + r] = v;
        } else {
            const int j = tid == 6 ? 0 : tid == 12 ? 1 : tid == 13 ? 2 : tid == 18 ? 3 : tid == 19 ? 4 : tid == 20 ? 5 : -1;
            if (j >= 0) {
                W.b[6 * i1 + j] = sum;
                W.bs[6 * i1 + j] = sum - s_bsum[j];
            }
        }
    }
}

// Dense LDL^T (no pivoting; fails on a zero pivot like Eigen::SimplicialLDLT) + solve of the reduced camera system of a window
// of more than 40 free keyframes (up to 40: k_ldlt_reg), one workgroup of 8 waves per window.  The matrix is padded to a multiple
// of 16 with an identity tail and lives in device memory: in place in Wn.Hs, which k_schur wrote with leading dimension npad
// (L2-resident; the identity tail is set once by k_prepare and stays an identity under the factorisation).  Everything else --
// the panel's L D, the vectors, T -- stays in LDS.  Blocked right-looking factorisation, block 16; per 16-column panel k
//   D_k  the 16x16 diagonal block by wave 0: unblocked LDL^T with row i of the block in the registers of lane i (pivot
//        and column entries travel through v_readlane; no predication: the upper halves of the rows are scratch), the
//        reciprocal pivots, then T_k = L_kk^-1 (lane c owns column c) and the block's part of the forward substitution
//        y_k = T_k r_k
//   P_k  panel below the block as a GEMM: W_I = A_Ik T_k^T on 16x16 tiles with v_mfma_f64_16x16x4_f64, L_Ik = W_I D^-1;
//        the rows' share of the forward substitution r_i -= L_ik y_k (so L y = b is solved while the matrix is
//        factorised)
//   U_k  trailing update A[I][J] -= W[I] L[J]^T on 16x16 tiles (MFMA); wave 0 takes the tile (k+1, k+1) and goes
//        straight on to D_{k+1} (look-ahead) while the other seven waves update the rest
// Two workgroup barriers per panel.  The backward substitution x = L^-T D^-1 y walks the panels the other way round
// with the same look-ahead (x_k = T_k^T s_k, one barrier per panel); finally the first np threads apply the update to
// the poses.  What one wave stores to the matrix and another wave of the workgroup loads afterwards is ordered by
// __syncthreads() (the compute unit's vector cache is write-through and shared by the workgroup's waves); inside wave 0 by
// wave_sync() = completion of the wave's outstanding stores.  The pivot chain of the diagonal blocks never touches memory, so
// what the matrix in device memory costs is one round trip per phase (measured: DESIGN.md 5.3).
typedef double double4_t __attribute__((ext_vector_type(4)));
typedef double __attribute__((address_space(1))) gdouble_t;
constexpr int kTileBatch = 4;
// doubles of dynamic LDS ldlt_body needs (W, the four vectors, T_k^T of two panels, the staged diagonal block, 16 of slack) ...
__host__ __device__ constexpr size_t ldlt_dev_lds_doubles(int npad) { return (size_t)npad * 17 + 4 * (size_t)npad + 3 * 16 * 17 + 16; }
// ... and the largest window that fits a CU's 160 KB with the kernel's static LDS: npad = 928, 154 free keyframes.  A larger window is
// refused on the host (build_structures) before anything is enqueued.  (kLdMaxNpad, kLdMaxNp: lba_window.h)
constexpr size_t kLdMaxDynLds = ldlt_dev_lds_doubles(kLdMaxNpad) * sizeof(double);   // 162 560 B
static_assert(kLdMaxDynLds + 64 <= 160 * 1024 && ldlt_dev_lds_doubles(kLdMaxNpad + 16) * sizeof(double) + 64 > 160 * 1024,
              "k_ldlt_dev: kLdMaxNpad is the largest padded size whose dynamic + static LDS fits a CU's 160 KB");
__device__ __forceinline__ void ldlt_body(const LbaWin &Wn, double *sm)
{
    constexpr int NT = 512, NW = 8;
    __shared__ int s_fail, s_tile;
    const int n = 6 * Wn.np, npad = Wn.npad;
    const double lambda = Wn.st->lambda;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // the matrix's rows lie on 128-byte boundaries; the LDS arrays have odd leading dimensions: column-direction accesses (MFMA
    // operands, substitution) fall on distinct banks
    const int ld = npad, lw = 17;
    gdouble_t *M = (gdouble_t *)Wn.Hs;           // npad x ld: lower triangle = the matrix, then L (factorised in place)
    double *W = sm;                              // npad x lw: L * D of the current panel
    double *dvec = W + (size_t)npad * lw;        // npad: D
    double *rdv = dvec + npad;                   // npad: 1 / D
    double *rv = rdv + npad;                     // npad: residual of the forward substitution, then y, then D^-1 y, then s
    double *xs = rv + npad;                      // npad: solution
    double *Tb = xs + npad;                      // 2 x 16 x 17: T_k^T of the current / next panel
    double *Dst = Tb + 2 * 16 * 17;              // 16 x 17: the next diagonal block on its way from the trailing update to wave 0's rows
    if (tid == 0) s_fail = 0;
    for (int i = tid; i < npad; i += NT) rv[i] = i < n ? Wn.bs[i] : 0.0;
    __syncthreads();
    // LDS writes of this wave visible to its other lanes (one wave: LDS operations execute in order), and its stores to the
    // matrix complete before its other lanes load them
    auto wave_sync = [] {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    };
    // D_k (wave 0 only; lanes >= 16 mirror lanes 0..15, their results are not stored).  Measured single-wave latencies
    // (tools/microbench/f64_latency.hip): dependent f64 FMA 9 cycles, IEEE division 67, v_rcp_f64 + 2 Newton steps 34,
    // a v_readlane pair 13, LDS write -> broadcast read 77.  So per pivot: the pivot itself comes by v_readlane and its
    // reciprocal by rcp + Newton (within 1 ulp), the column's other entries by ONE LDS write + broadcast reads that fly
    // while the reciprocal is refined (30 v_readlane would cost 200 cycles of issue), and nothing is predicated: the
    // upper halves of the rows are scratch.  T = L_kk^-1 is built on the way -- lane c owns column c,
    // T <- (I - l_j e_j^T) T needs only column j of L, which every lane has just read -- and so is y_k = L_kk^-1 r_k.
    auto rcp_newton = [](double d) {   // 1 / d within 1 ulp: v_rcp_f64 + two Newton steps (34 cycles; the IEEE division takes 67)
        double rd = __builtin_amdgcn_rcp(d);
        double e = __builtin_fma(-d, rd, 1.0);
        rd = __builtin_fma(rd, e, rd);
        e = __builtin_fma(-d, rd, 1.0);
        return __builtin_fma(rd, e, rd);
    };
    auto diag_block = [&](int k0, bool staged) {
        const int li = lane & 15;
        double *colbuf = xs;   // 16 doubles of scratch (xs is unused until the backward pass)
        double *Tk = Tb + ((k0 >> 4) & 1) * (16 * 17);
        double row[16];
        if (staged) {
#pragma unroll
            for (int c = 0; c < 16; ++c) row[c] = Dst[li * 17 + c];
        } else {
#pragma unroll
            for (int c = 0; c < 16; ++c) row[c] = M[(size_t)(k0 + li) * ld + k0 + c];
        }
        double dsave = 1.0;
        double cur = rv[k0 + li];
        bool bad = false;
        // T = L_kk^-1 (unit lower triangular), lane c owns column c, built alongside the factorisation: eliminating column j
        // gives every lane the whole column (ck[k] = a_kj, the broadcast it needs for its own row anyway) and the reciprocal
        // pivot, i.e. L[k][j] = ck[k] rd for all k -- so t[k] -= L[k][j] t[j] costs one product and 15 - j fused
        // multiply-adds here, instead of a second pass that re-read L through 120 LDS broadcasts per lane (1840 cycles per
        // block).  (Rows in lanes 0..15 and T in lanes 16..31 as ONE instruction stream -- both updates are
        // x[k] -= (x[j] rd) ck[k] -- was measured slower: 36.5 k against 34.7 k cycles for the 8 blocks, the lane-group
        // selects and predicated stores cost more than the 7.5 multiply-adds per pivot they save.)
        double t[16];
#pragma unroll
        for (int c = 0; c < 16; ++c) t[c] = c == li ? 1.0 : 0.0;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const double ci = row[j];
            dsave = li == j ? ci : dsave;   // the pivot of this lane's row (what is stored at M[k0 + li][k0 + li] below)
            if (j < 15) colbuf[li] = ci;
            const double dj = readlane_f64(ci, j);
            if (dj == 0.0 || dj != dj) bad = true;
            double ck[16];
#pragma unroll
            for (int k = j + 1; k < 16; ++k) ck[k] = colbuf[k];
            const double rd = rcp_newton(dj);
            const double lij = ci * rd;
            const double yj = readlane_f64(cur, j);
            const double st = rd * t[j];
#pragma unroll
            for (int k = j + 1; k < 16; ++k) {
                row[k] = __builtin_fma(-lij, ck[k], row[k]);
                t[k] = __builtin_fma(-ck[k], st, t[k]);
            }
            // row i > j: its entry of column j becomes L[i][j]; row j keeps the pivot; rows above hold scratch there.  Both
            // finished values leave for LDS at once (the rows of the block without predication: the entries right of the
            // diagonal are scratch that nothing reads; lanes >= 16 store the same values to the same places; column c of T
            // = row c of the panel's T^T buffer, dense: zeros above the diagonal, ones on it), so the live registers shrink
            // with j instead of holding 16 finished entries of each array to the end
            M[(size_t)(k0 + li) * ld + k0 + j] = li == j ? ci : lij;   // (lanes >= 16 repeat the stores of lanes 0..15: a predicate here costs 85 registers and spills)
            Tk[li * 17 + j] = t[j];
            cur = li > j ? __builtin_fma(-lij, yj, cur) : cur;   // forward substitution inside the block
            __builtin_amdgcn_sched_barrier(0);   // keep the pivots apart (hoisting the later pivots' reads only costs spills)
        }
        if (bad) {
            if (lane == 0) s_fail = 1;
            return;
        }
        rv[k0 + li] = cur;   // y of this block
        wave_sync();
        dvec[k0 + li] = dsave;
        rdv[k0 + li] = rcp_newton(dsave);   // (the same operations as in the loop: the same bits)
    };
    if (wave == 0) diag_block(0, false);
    __syncthreads();
    const int nb = npad >> 4;
    const int col = lane & 15, rq = lane >> 4;
    for (int kb = 0; kb < nb && !s_fail; ++kb) {
        const int k0 = kb << 4;
        const int m = nb - kb - 1;
        // ---- P_k: W_I = A_Ik T^T (one 16-row tile per wave turn), L_Ik = W_I D^-1
        // (wave 0 requests the entries of the NEXT diagonal block -- tile 0 of the trailing update, final since the last
        // panel's update -- before the panel: its round trip to device memory is off the critical path of the look-ahead)
        double4_t acc0 = {0, 0, 0, 0};
        if (wave == 0 && m > 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) acc0[r] = M[(size_t)(k0 + 16 + rq + 4 * r) * ld + k0 + 16 + col];
        }
        for (int ti = wave; ti < m; ti += NW) {
            const int I0 = (kb + 1 + ti) << 4;
            double4_t acc = {0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const int c = 4 * kk + rq;
                const double av = M[(size_t)(I0 + col) * ld + k0 + c];                                  // A[i = col][c]
                const double tv = Tb[(kb & 1) * (16 * 17) + c * 17 + col];                                // B[c][j = col] = T[j][c]
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, tv, acc, 0, 0, 0);
            }
            const double rd = rdv[k0 + col];
            // the tile's A entries were all read by the MFMAs above (this wave only): overwrite them with L
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                W[(size_t)(I0 + rq + 4 * r) * lw + col] = acc[r];
                M[(size_t)(I0 + rq + 4 * r) * ld + k0 + col] = acc[r] * rd;
            }
        }
        if (tid == 0) s_tile = 1;   // (tile 0 is wave 0's)
        __syncthreads();
        // forward substitution of the rows below: r_i -= sum_c L[i][k0 + c] y_c (c ascending)
        for (int i = k0 + 16 + tid; i < npad; i += NT) {
            double l[16];
#pragma unroll
            for (int c = 0; c < 16; ++c) l[c] = W[(size_t)i * lw + c] * rdv[k0 + c];   // (L = W D^-1: the product the panel stored, the same bits)
            double ri = rv[i];
#pragma unroll
            for (int c = 0; c < 16; ++c) ri -= l[c] * rv[k0 + c];
            rv[i] = ri;
        }
        // ---- U_k: trailing update with f64 MFMA on the lower-triangle tiles (I >= J > kb); tile 0 = (kb+1, kb+1) goes
        // to wave 0, which then factorises that block while the other waves finish the update
        const int ntiles = m * (m + 1) / 2;
        auto tile_at = [&](int t, int &I0, int &J0) {
            int ii = 0, rem = t;
            while (rem > ii) {  // row-major lower triangle: row ii holds ii+1 tiles
                rem -= ii + 1;
                ++ii;
            }
            I0 = (kb + 1 + ii) << 4;
            J0 = (kb + 1 + rem) << 4;
        };
        // B[k][j] = L[J0 + j][k0 + k]: as the product W D^-1 the panel stored in the matrix -- the same bits, from LDS
        auto lval = [&](int J0, int kk) -> double { return W[(size_t)(J0 + col) * lw + 4 * kk + rq] * rdv[k0 + 4 * kk + rq]; };
        // tile 0, started from the entries wave 0 requested before the panel; the result is the next diagonal block and goes to
        // wave 0's rows through LDS, not through the matrix
        auto tile0 = [&]() {
            const int I0 = (kb + 1) << 4;
            double4_t acc = acc0;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const double av = -W[(size_t)(I0 + col) * lw + 4 * kk + rq];          // A[i = lane&15][k = lane>>4]
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lval(I0, kk), acc, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) Dst[(rq + 4 * r) * 17 + col] = acc[r];
        };
        // The tiles are handed out kTileBatch at a time from a counter in LDS (a tile's result does not depend on the wave
        // that forms it), the next batch's entries are requested before the current batch's products are formed (a batch is a
        // round trip to device memory), and wave 0 joins when its diagonal block is done: at 30-40 free keyframes the trailing
        // update, not the pivot chain, was the longer side of the look-ahead (measured: DESIGN.md 5.3)
        auto run_tiles = [&]() {
            auto grab = [&]() {
                int t = 0;
                if (lane == 0) t = atomicAdd(&s_tile, kTileBatch);
                return __builtin_amdgcn_readfirstlane(t);
            };
            int I0[kTileBatch], J0[kTileBatch];
            double4_t acc[kTileBatch];
            auto fetch = [&](int t, int (&I)[kTileBatch], int (&J)[kTileBatch], double4_t (&a)[kTileBatch]) {
#pragma unroll
                for (int u = 0; u < kTileBatch; ++u) tile_at(min(t + u, ntiles - 1), I[u], J[u]);
#pragma unroll
                for (int u = 0; u < kTileBatch; ++u)
#pragma unroll
                    for (int r = 0; r < 4; ++r) a[u][r] = M[(size_t)(I[u] + rq + 4 * r) * ld + J[u] + col];
            };
            int t = grab();
            if (t < ntiles) fetch(t, I0, J0, acc);
            while (t < ntiles) {
                const int tn = grab();
                int In[kTileBatch], Jn[kTileBatch];
                double4_t an[kTileBatch];
                if (tn < ntiles) fetch(tn, In, Jn, an);
#pragma unroll
                for (int u = 0; u < kTileBatch; ++u)
#pragma unroll
                    for (int kk = 0; kk < 4; ++kk) {
                        const double av = -W[(size_t)(I0[u] + col) * lw + 4 * kk + rq];
                        acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lval(J0[u], kk), acc[u], 0, 0, 0);
                    }
#pragma unroll
                for (int u = 0; u < kTileBatch; ++u)
                    if (t + u < ntiles)
#pragma unroll
                        for (int r = 0; r < 4; ++r) M[(size_t)(I0[u] + rq + 4 * r) * ld + J0[u] + col] = acc[u][r];
                t = tn;
#pragma unroll
                for (int u = 0; u < kTileBatch; ++u) {
                    I0[u] = In[u]; J0[u] = Jn[u]; acc[u] = an[u];
                }
            }
        };
        if (wave == 0) {
            if (ntiles > 0) {
                // (the rows k0+16 .. k0+31 of the forward substitution above belong to threads 0..15 = this wave)
                wave_sync();
                tile0();
                wave_sync();
                diag_block(k0 + 16, true);
                run_tiles();
            }
        } else {
            run_tiles();
        }
        __syncthreads();
    }
    if (s_fail) {
        if (tid == 0) Wn.scal[3] = 0.0;
        if (tid < Wn.np) {   // the trial is rejected (lm_decide): its pop() must find the estimates it started from
            const double *Tp = Wn.pose + 7 * (size_t)Wn.hpose[tid];
            double *Tbk = Wn.bk + 7 * (size_t)Wn.hpose[tid];
            for (int i = 0; i < 7; ++i) Tbk[i] = Tp[i];
        }
        return;
    }
    // ---- backward substitution: x = L^-T D^-1 y; per block x_k = T_k^T s_k, then the rows above take L_k^T x_k
    for (int i = tid; i < npad; i += NT) rv[i] = rv[i] * rdv[i];
    __syncthreads();
    auto back_load = [&](int k0, double (&lcol)[16]) {   // L[j][i] for j > i of the diagonal block (the rest is unused)
        const int li = lane & 15;
#pragma unroll
        for (int j = 0; j < 16; ++j) lcol[j] = M[(size_t)(k0 + j) * ld + k0 + li];
    };
    auto back_block = [&](int k0, const double (&lcol)[16]) {   // wave 0: L_kk^T x_k = s_k, k descending inside the block
        const int li = lane & 15;
        double cur = rv[k0 + li];
#pragma unroll
        for (int j = 15; j >= 1; --j) {
            const double xj = readlane_f64(cur, j);
            cur = li < j ? __builtin_fma(-lcol[j], xj, cur) : cur;
        }
        xs[k0 + li] = cur;
    };
    if (wave == 0) {
        double lc[16];
        back_load((nb - 1) << 4, lc);
        back_block((nb - 1) << 4, lc);
    }
    __syncthreads();
    for (int kb = nb - 1; kb > 0; --kb) {
        const int k0 = kb << 4;
        // rows above the block take its contribution; wave 0 does the rows of the next block first and solves it
        auto update_row = [&](int i) {
            double l[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) l[j] = M[(size_t)(k0 + j) * ld + i];
            double acc = rv[i];
#pragma unroll
            for (int j = 15; j >= 0; --j) acc -= l[j] * xs[k0 + j];
            rv[i] = acc;
        };
        if (wave == 0) {
            double lc[16];
            back_load(k0 - 16, lc);   // (independent of x: requested together with the rows' entries -- one round trip, not two, when the matrix is in device memory)
            if (lane < 16) update_row(k0 - 16 + lane);
            wave_sync();
            back_block(k0 - 16, lc);
        } else {
            for (int i = tid - 64; i < k0 - 16; i += NT - 64) update_row(i);
        }
        __syncthreads();
    }
    for (int i = tid; i < n; i += NT) Wn.x[i] = xs[i];
    if (tid == 0) Wn.scal[3] = 1.0;
    if (tid < Wn.np) {   // VertexSE3Expmap::oplusImpl + the poses' scale terms
        double upd[6];
        for (int i = 0; i < 6; ++i) {
            upd[i] = xs[6 * tid + i];
            Wn.tmp[6 * tid + i] = upd[i] * (lambda * upd[i] + Wn.b[6 * tid + i]);
        }
        double *Tp = Wn.pose + 7 * (size_t)Wn.hpose[tid], *Tbk = Wn.bk + 7 * (size_t)Wn.hpose[tid];
        for (int i = 0; i < 7; ++i) Tbk[i] = Tp[i];   // push()
        se3_oplus_fast(upd, Tp);   // (polynomial small-angle form, lba_math.h; agrees with se3_oplus to a few ulp)
    }
}

__global__ __launch_bounds__(512) void k_ldlt_dev(const LbaWin *__restrict__ wins)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const LbaWin &Wn = wins[blockIdx.x];
    if (!Wn.st->run || Wn.np == 0 || Wn.ldlt_form != kLdltDev) return;
    ldlt_body(Wn, sm);
}

// The form every window of <= 40 free keyframes takes (ldlt_reg.h): the trailing matrix as MFMA accumulator tiles in the registers of
// seven waves, the diagonal tiles / panel / T_k / vectors in LDS, no device-memory traffic between the load and the solution; the
// epilogue is ldlt_body's (solution, pose update with the push() backup, the poses' scale terms).
__global__ __launch_bounds__(kLrThreads) void k_ldlt_reg(const LbaWin *__restrict__ wins)
{
    extern __shared__ __attribute__((aligned(16))) double sm[];
    const LbaWin &Wn = wins[blockIdx.x];
    if (!Wn.st->run || Wn.np == 0 || Wn.ldlt_form != kLdltReg) return;
    const int tid = threadIdx.x, n = 6 * Wn.np;
    const double lambda = Wn.st->lambda;
    double *xs = nullptr;
    const bool ok = ldlt_reg_solve<false>(Wn.Hs, n, Wn.npad, Wn.bs, sm, xs, nullptr);
    if (!ok) {
        if (tid == 0) Wn.scal[3] = 0.0;
        if (tid < Wn.np) {   // the trial is rejected (lm_decide): its pop() must find the estimates it started from
            const double *Tp = Wn.pose + 7 * (size_t)Wn.hpose[tid];
            double *Tbk = Wn.bk + 7 * (size_t)Wn.hpose[tid];
            for (int i = 0; i < 7; ++i) Tbk[i] = Tp[i];
        }
        return;
    }
    for (int i = tid; i < n; i += kLrThreads) Wn.x[i] = xs[i];
    if (tid == 0) Wn.scal[3] = 1.0;
    if (tid < Wn.np) {   // VertexSE3Expmap::oplusImpl + the poses' scale terms
        double upd[6];
        for (int i = 0; i < 6; ++i) {
            upd[i] = xs[6 * tid + i];
            Wn.tmp[6 * tid + i] = upd[i] * (lambda * upd[i] + Wn.b[6 * tid + i]);
        }
        double *Tp = Wn.pose + 7 * (size_t)Wn.hpose[tid], *Tbk = Wn.bk + 7 * (size_t)Wn.hpose[tid];
        for (int i = 0; i < 7; ++i) Tbk[i] = Tp[i];   // push()
        se3_oplus_fast(upd, Tp);
    }
}

// Between the two optimisations (Optimizer.cc:667-710), one launch (the bDoMore check of :663-666 was made where the first
// optimisation ended: lm_first_done).  Edges with chi2 above the threshold or non-positive depth leave the optimisation
// (setLevel(1)), all edges drop their robust kernel (:672-703); the workgroup that finishes last does
// initializeOptimization(0) (fails without level-0 edges) and the entry of optimize(10).
// _error of edge e as the last residual evaluation left it (LmState::err_at): re-formed with the operations of the residual pass
// from the estimates it ran on (p_cur = the edge's camera point at the CURRENT estimates, which the caller needs anyway), and stored
// when `keep` -- the values an edge keeps while it is inactive
__device__ __forceinline__ void edge_last_error(const LbaWin &W, int e, int at, const double p_cur[3], int stereo, bool keep, double er[3])
{
    double *dst = W.err + 3 * (size_t)e;
    if (at == 0) {
        er[0] = dst[0]; er[1] = dst[1]; er[2] = dst[2];
        return;
    }
    double p[3] = {p_cur[0], p_cur[1], p_cur[2]};
    if (at == 2) se3_map(W.bk + 7 * (size_t)W.e_pose[e], W.bk + 7 * (size_t)W.n_poses + 3 * (size_t)W.e_point[e], p);
    const double ob[3] = {(double)W.in_obs[3 * (size_t)e], (double)W.in_obs[3 * (size_t)e + 1], (double)W.in_obs[3 * (size_t)e + 2]};
    edge_error(W.cam, p, ob, stereo, er);
    if (keep) {
        dst[0] = er[0]; dst[1] = er[1]; dst[2] = er[2];
    }
}

__global__ __launch_bounds__(256) void k_transition(const LbaWin *__restrict__ wins)
{
    __shared__ int s_last;
    const LbaWin &W = wins[blockIdx.y];
    LmState *st = W.st;
    if (!st->xmark) return;
    const int err_at = st->err_at;   // (reset by the workgroup that finishes last: after every workgroup's read)
    // (a thread takes the edge at its position of the landmarks' edge lists -- every edge is there once --, so that it can keep the
    // position's record in step)
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    int keep = 0;
    if (a < W.n_edges) {
        const int e = W.pt_k[a];
        const int stereo = W.e_stereo[e];
        double p[3], er[3];
        se3_map(W.pose + 7 * (size_t)W.e_pose[e], W.point + 3 * (size_t)W.e_point[e], p);
        edge_last_error(W, e, err_at, p, stereo, true, er);
        const double c = edge_chi2(er, (double)W.in_w[e], stereo ? 3 : 2);
        const bool bad = c > (stereo ? 7.815 : 5.991) || !(p[2] > 0.0);
        if (bad) {
            W.e_level1[e] = 1;
            const int pp = W.pl_pos[e];
            if (pp >= 0) lrec_mask(W, pp);
        }
        W.e_robust[e] = 0;
        W.erec[a].flags = (W.erec[a].flags & ~kEdgeRobust) | (bad ? kEdgeLevel1 : 0);
        keep = bad ? 0 : 1;
    }
    const unsigned long long m = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&st->n_active, __popcll(m));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the waves' additions are performed before the workgroup reports itself done: see points_tail)
    __syncthreads();
    // (the last workgroup reads nothing of the others but n_active, an atomic: no device-scope fence)
    if (threadIdx.x == 0) s_last = __hip_atomic_fetch_add(&st->blocks_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (int)gridDim.x - 1;
    __syncthreads();
    if (!s_last || threadIdx.x != 0) return;
    st->blocks_done = 0;
    st->xmark = 0;
    st->it = 0;
    st->err_at = 0;   // (the stored values stand until the second optimisation evaluates)
    const int n_active = __hip_atomic_load(&st->n_active, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n_active == 0 || st->iters_max[1] <= 0 || lm_poll(st, W.abort_word)) {
        st->phase = 3;
        st->iters_done[1] = 0;
    } else {
        st->phase = 2;
        st->initp = 1;
    }
}

// final inlier check (:712-744) and the write-back conversions (:763-778)
__global__ __launch_bounds__(256) void k_final(const LbaWin *__restrict__ wins)
{
    const LbaWin &W = wins[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W.n_edges) {
        const int stereo = W.e_stereo[i];
        double p[3], er[3];
        se3_map(W.pose + 7 * (size_t)W.e_pose[i], W.point + 3 * (size_t)W.e_point[i], p);
        edge_last_error(W, i, W.e_level1[i] ? 0 : W.st->err_at, p, stereo, false, er);   // (an inactive edge kept its _error)
        const double c = edge_chi2(er, (double)W.in_w[i], stereo ? 3 : 2);
        const bool bad = c > (stereo ? 7.815 : 5.991) || !(p[2] > 0.0);
        if (W.out_chi2) W.out_chi2[i] = c;
        W.out_outlier[i] = bad ? 1 : 0;
    }
    if (i < W.n_poses) pose_to_Tcw(W.pose + 7 * (size_t)i, W.out_Tcw + 16 * (size_t)i);
    if (i < W.n_points)
        for (int d = 0; d < 3; ++d) W.out_xyz[3 * (size_t)i + d] = (float)W.point[3 * (size_t)i + d];
}

// ---------------------------------------------------------------------------------------------------------- host
static_assert(kLrMaxNpad == 16 * kLrMaxNb, "lba_window.h restates the register form's size limit (ldlt_reg.h)");

// The reduced-system kernels take their LDS dynamically (the panel and the vectors of the largest window of a launch): each
// kernel's cap is declared once per device binding, and every launch goes through enqueue_ldlt, which sizes it
int ldlt_declare_lds()
{
    AOS2_HIP_CHECK(hipFuncSetAttribute((const void *)k_ldlt_dev, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdMaxDynLds));
    AOS2_HIP_CHECK(hipFuncSetAttribute((const void *)k_ldlt_reg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLrMaxDynLds));
    return AOS2_OK;
}
// Both forms over the descriptors blk[0 .. nw): a window returns early from the kernel that is not its form.  mx_npad_reg /
// mx_npad_dev: the largest padded size among the windows of that form, 0 = none (the kernel is not launched)
void enqueue_ldlt(const LbaWin *blk, int nw, int mx_npad_reg, int mx_npad_dev, hipStream_t q_reg, hipStream_t q_dev)
{
    if (mx_npad_reg > 0)
        hipLaunchKernelGGL(k_ldlt_reg, dim3(nw), dim3(kLrThreads), ldlt_reg_lds_doubles(mx_npad_reg) * sizeof(double), q_reg, blk);
    if (mx_npad_dev > 0) hipLaunchKernelGGL(k_ldlt_dev, dim3(nw), dim3(512), ldlt_dev_lds_doubles(mx_npad_dev) * sizeof(double), q_dev, blk);
}

// ---- enqueueing (csrc/lba_launch.h declares these: the solve and the taps call them, no kernel is launched from another unit)
static unsigned blocks(size_t n, int t) { return (unsigned)((n + t - 1) / t); }

void enqueue_prepare(const LaunchCtx &C, const Prog &P)
{
    hipLaunchKernelGGL(k_prepare, dim3(blocks(std::max(P.D.mx_E, P.D.mx_pts), 256), P.nw), dim3(256), 0, P.q, P.blk, C.s->debug_stop_at_poll);
}
void enqueue_points(const LaunchCtx &C, const Prog &P, int solve)
{
    if (C.walk)
        hipLaunchKernelGGL(k_points_walk, dim3((unsigned)P.n_pts), dim3(128), (size_t)P.D.walk_lds, P.q, P.wins, P.pts, solve);
    else
        hipLaunchKernelGGL(k_points, dim3((unsigned)P.n_pts), dim3(256), 0, P.q, P.wins, P.pts, solve);
}
void enqueue_lin(const LaunchCtx &C, const Prog &P, int init)
{
    if (!P.n_lin) return;
    if (C.walk)
        hipLaunchKernelGGL(k_lin<true>, dim3((unsigned)P.n_lin), dim3(256), (size_t)P.D.walk_lds, P.q, P.wins, P.lin, init);
    else
        hipLaunchKernelGGL(k_lin<false>, dim3((unsigned)P.n_lin), dim3(256), 0, P.q, P.wins, P.lin, init);
}
void enqueue_init(const LaunchCtx &C, const Prog &P)
{
    enqueue_points(C, P, 0);
    enqueue_lin(C, P, 1);
    hipLaunchKernelGGL(k_lm_init, dim3(P.nw), dim3(1024), 0, P.q, P.blk);
}
void enqueue_schur(const Prog &P)
{
    if (P.n_schur) hipLaunchKernelGGL(k_schur, dim3((unsigned)P.n_schur), dim3(kSchurThreads), 0, P.q, P.wins, P.schur);
}
// the pose half of a Levenberg-Marquardt trial: the Schur complement and the reduced system's solve with the pose update
void enqueue_reduced(LaunchCtx &C, const Prog &P, bool first_group)
{
    const GroupDims &D = P.D;
    enqueue_schur(P);
    if (first_group && C.stagger_pending) {   // the other group starts here: half a trial behind
        (void)hipEventRecord(C.s->ev_stag, C.s->stream);
        (void)hipStreamWaitEvent(C.s->stream_b, C.s->ev_stag, 0);
        C.stagger_pending = false;
    }
    // the two forms of the reduced-system kernel work on different windows: side by side (the register form on a stream of its own)
    const bool both = D.any_glob && D.any_reg;
    if (both) {
        (void)hipEventRecord(P.fork, P.q);
        (void)hipStreamWaitEvent(P.q2, P.fork, 0);
    }
    enqueue_ldlt(P.blk, P.nw, D.any_reg ? D.mx_npad_reg : 0, D.any_glob ? D.mx_npad_glob : 0, both ? P.q2 : P.q, P.q);
    if (both) {
        (void)hipEventRecord(P.join, P.q2);
        (void)hipStreamWaitEvent(P.q, P.join, 0);
    }
}
// one Levenberg-Marquardt trial: 4 launches (5 with reduced systems of both kinds)
void enqueue_trial(LaunchCtx &C, const Prog &P, bool first_group)
{
    enqueue_reduced(C, P, first_group);
    enqueue_points(C, P, 1);   // + the LM decision in its last workgroup
    enqueue_lin(C, P, 0);
}
void enqueue_transition(const Prog &P)
{
    hipLaunchKernelGGL(k_transition, dim3(blocks(P.D.mx_E, 256), P.nw), dim3(256), 0, P.q, P.blk);
}
void enqueue_final(const Prog &P)
{
    hipLaunchKernelGGL(k_final, dim3(blocks(std::max(P.D.mx_E, P.D.mx_pts), 256), P.nw), dim3(256), 0, P.q, P.blk);
}

// The whole procedure of a group's windows: optimisation k gets slots[k] trials and runs if any window of the call asks for
// iterations (iters[k] > 0)
void enqueue_program(LaunchCtx &C, const Prog &P, bool first_group, const int (&iters)[2], const int (&slots)[2])
{
    enqueue_prepare(C, P);
    for (int k = 0; k < 2; ++k) {
        if (k == 1) enqueue_transition(P);
        if (iters[k] > 0) {
            enqueue_init(C, P);
            for (int t = 0; t < slots[k]; ++t) enqueue_trial(C, P, first_group);
        }
    }
}

}  // namespace aos2
