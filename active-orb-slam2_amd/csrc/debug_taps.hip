// Test taps: host/device execution of shared primitives so parity tests can pin them in isolation.
#include <algorithm>
#include <cmath>
#include <map>
#include <set>
#include <vector>

#include "aos2_common.h"
#include "initializer.h"
#include "octree.h"
#include "pnp.h"
#include "sincos_exact.h"
#include "sim3.h"
#include "triangulate.h"
#include "visibility.h"
#include "connections.h"
#include "local_map.h"
#include "motion_tw.h"
#include "normal_depth.h"
#include "wave_ops.h"

namespace aos2 {
__global__ void sincos_kernel(const float *a, int n, float *s, float *c)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sincos_exact(a[i], &s[i], &c[i]);
}

// Every primitive of wave_ops.h on one int and one double per thread: a workgroup of NT threads per case, kWaveOpsI ints and
// kWaveOpsD doubles per thread (the order below is the layout capi.py names).
constexpr int kWaveOpsI = 17, kWaveOpsD = 7;
template <int NT>
__global__ __launch_bounds__(NT) void wave_ops_kernel(const int32_t *vi, const double *vd, int32_t *out_i, double *out_d)
{
    __shared__ int32_t wsum[NT / 64];
    const size_t t = (size_t)blockIdx.x * NT + threadIdx.x;
    const int v = vi[t];
    const double d = vd[t];
    int32_t *oi = out_i + kWaveOpsI * t;
    double *od = out_d + kWaveOpsD * t;
    oi[0] = (int32_t)dpp_u32<0xB1>((uint32_t)v);
    oi[1] = (int32_t)dpp_u32<0x4E>((uint32_t)v);
    oi[2] = (int32_t)dpp_u32<0x141>((uint32_t)v);
    oi[3] = (int32_t)dpp_u32<0x140>((uint32_t)v);
    oi[4] = dpp_i32<0xB1>(v);
    oi[5] = dpp_i32<0x4E>(v);
    oi[6] = dpp_i32<0x141>(v);
    oi[7] = dpp_i32<0x140>(v);
    oi[8] = wave_row_sum_i32(v);
    oi[9] = wave_sum_i32(v);
    oi[10] = wave_max_i32(v);
    oi[11] = (int32_t)wave_row_min_u32((uint32_t)v);
    oi[12] = (int32_t)wave_min_u32((uint32_t)v);
    oi[13] = wave_incl_scan_i32(v);
    int total;
    oi[14] = block_excl_scan_i32<NT>(v, wsum, total);
    oi[15] = total;
    // block_sum_i32 twice on the same LDS words (which the scan has just read): the sum of v, then that of 2 v; their difference is
    // the sum of v only if no wave of the second call stored before every wave of the first had read
    const uint32_t once = (uint32_t)block_sum_i32<NT>(v, wsum), twice = (uint32_t)block_sum_i32<NT>((int)(2u * (uint32_t)v), wsum);
    oi[16] = (int32_t)(twice - once);
    od[0] = dpp_f64<0xB1>(d);
    od[1] = dpp_f64<0x4E>(d);
    od[2] = dpp_f64<0x141>(d);
    od[3] = dpp_f64<0x140>(d);
    od[4] = row_sum_f64(d);
    od[5] = readlane_f64(d, 0);
    od[6] = readlane_f64(d, 63);
}

// row_sums_scatter_f64<K> by one wave: every lane's K values in, every lane's slots out
template <int K>
__global__ __launch_bounds__(64) void row_sums_scatter_kernel(const double *v, double *out)
{
    double a[K];
#pragma unroll
    for (int i = 0; i < K; ++i) a[i] = v[K * threadIdx.x + i];
    row_sums_scatter_f64<K>(a);
#pragma unroll
    for (int s = 0; s < row_scatter_slots(K); ++s) out[row_scatter_slots(K) * threadIdx.x + s] = a[s];
}

template <int K>
int row_sums_scatter_run(const double *v, double *out, int32_t *owner)
{
    constexpr int S = row_scatter_slots(K);
    int st;
    DevBuf<double> dv, dout;
    if ((st = dv.alloc(64 * K)) || (st = dout.alloc(64 * S))) return st;
    AOS2_HIP_CHECK(hipMemcpy(dv.p, v, sizeof(double) * 64 * K, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(row_sums_scatter_kernel<K>, dim3(1), dim3(64), 0, 0, dv.p, dout.p);
    AOS2_HIP_CHECK(hipDeviceSynchronize());
    AOS2_HIP_CHECK(hipMemcpy(out, dout.p, sizeof(double) * 64 * S, hipMemcpyDeviceToHost));
    dv.release(); dout.release();
    for (int i = 0; i < K; ++i) {
        int li = 0, s = 0;
        row_scatter_owner<K>(i, li, s);
        owner[2 * i] = li;
        owner[2 * i + 1] = s;
    }
    return AOS2_OK;
}

// FindHomography / FindFundamental (:124-223) of one problem, serially: score, matrix (18 floats for H: H21 | H12), flags -> iteration
static int initializer_find_host(bool is_h, const aos2_initializer_problem_t &P, const InitPts &pts, float *score, float *model, uint8_t *flags)
{
    InitLocal ws;
    const float invS = init_inv_sigma2(P.sigma);
    std::vector<float> scores((size_t)P.iterations), models((size_t)P.iterations * 18);
    for (int it = 0; it < P.iterations; ++it) {
        float *M = models.data() + 18 * (size_t)it;
        if (is_h) init_model_h(pts, P.sets + 8 * (size_t)it, ws, M, M + 9);
        else init_model_f(pts, P.sets + 8 * (size_t)it, ws, M);
        float s = 0;
        for (int i = 0; i < P.n_matches; ++i) {
            float a, b;
            init_terms(is_h, M, invS, pts, i, a, b);
            s += a;
            s += b;
        }
        scores[(size_t)it] = s;
    }
    const int best = init_pick(scores.data(), P.iterations, score);
    if (best >= 0) {
        memcpy(model, models.data() + 18 * (size_t)best, 18 * sizeof(float));
        for (int i = 0; i < P.n_matches; ++i) {
            float a, b;
            flags[i] = init_terms(is_h, model, invS, pts, i, a, b);
        }
    }
    return best;
}
}  // namespace aos2

extern "C" {

int aos2_debug_pnp_set(int n, const int32_t *row, int min_set, int32_t *indices)
{
    using namespace aos2;
    if (!row || !indices || min_set < 0 || n < min_set) {
        set_error("bad argument (the two arrays, 0 <= min_set <= n)");
        return AOS2_ERR_ARG;
    }
    for (int i = 0; i < min_set; ++i)
        if (row[i] < 0 || row[i] > n - 1 - i) {
            set_error("draw %d is %d, outside [0, %d]", i, row[i], n - 1 - i);
            return AOS2_ERR_ARG;
        }
    int k = 0;
    PnpSetDraws{n, min_set, row}.each([&](int i) { indices[k++] = i; });
    return AOS2_OK;
}

int aos2_debug_pnp_scan(int first_iteration, int n_iterations, const int32_t *counts, const int32_t *refined, int32_t refined_carried,
                        int min_inliers, int best_inliers_in, int32_t *returned_at, int32_t *best_iteration, int32_t *best_inliers)
{
    using namespace aos2;
    if (first_iteration < 0 || first_iteration > n_iterations || (n_iterations > 0 && (!counts || !refined)) || !returned_at || !best_iteration ||
        !best_inliers) {
        set_error("bad argument (0 <= first_iteration <= n_iterations, the two tables, the three outputs)");
        return AOS2_ERR_ARG;
    }
    PnpScan scan(best_inliers_in);
    for (int it = first_iteration; it < n_iterations; ++it)
        if (scan.step(it, counts[it], min_inliers) &&
            scan.refined(it, scan.best_iteration < 0 ? refined_carried : refined[scan.best_iteration], min_inliers))
            break;
    *returned_at = scan.returned_at;
    *best_iteration = scan.best_iteration;
    *best_inliers = scan.best_inliers;
    return AOS2_OK;
}

int aos2_debug_pnp_host(const aos2_pnp_problem_t *problems, aos2_pnp_result_t *results, int n_problems)
{
    using namespace aos2;
    uint8_t run[64];
    if (int st = pnp_check(problems, results, n_problems, run)) return st;
    for (int p = 0; p < n_problems; ++p) {
        const aos2_pnp_problem_t &P = problems[p];
        aos2_pnp_result_t &R = results[p];
        pnp_result_clear(P, R);
        if (!run[p]) continue;
        const PnpCam K = {P.fx, P.fy, P.cx, P.cy};
        const PnpPts pts = {P.P3Dw, P.P2D, P.max_err};
        PnpLocal<12, 12> ws;
        std::vector<uint8_t> flags((size_t)P.n), rflags((size_t)P.n);
        PnpScan scan(P.best_inliers_in);
        bool refined_is_current = false;   // Refine() of the set R.best holds: Rr, rcount, rflags
        double Rr[12];
        int32_t rcount = 0;
        for (int it = P.first_iteration; it < P.n_iterations; ++it) {
            double Rt[12];
            pnp_compute_pose(PnpSetDraws{P.n, P.min_set, P.draws + (size_t)P.min_set * it}, pts, K, ws, Rt, Rt + 9);
            int32_t count = 0;
            for (int i = 0; i < P.n; ++i) count += flags[i] = pnp_inlier(Rt, K, pts, i);
            if (R.counts) R.counts[it] = count;
            const int32_t before = scan.best_iteration;
            if (!scan.step(it, count, P.min_inliers)) continue;
            if (scan.best_iteration != before) {   // :212-224
                memcpy(R.best, flags.data(), flags.size());
                pnp_Tcw(Rt, R.best_Tcw);
                refined_is_current = false;
            }
            if (!refined_is_current) {   // Refine() (:260-305)
                pnp_compute_pose(PnpSetFlags{P.n, R.best}, pts, K, ws, Rr, Rr + 9);
                rcount = 0;
                for (int i = 0; i < P.n; ++i) rcount += rflags[i] = pnp_inlier(Rr, K, pts, i);
                refined_is_current = true;
            }
            if (scan.refined(it, rcount, P.min_inliers)) {
                pnp_Tcw(Rr, R.Tcw);
                R.n_inliers = rcount;
                memcpy(R.inliers, rflags.data(), rflags.size());
                break;
            }
        }
        R.returned_at = scan.returned_at;
        R.best_iteration = scan.best_iteration;
        R.best_inliers = scan.best_inliers;
    }
    return AOS2_OK;
}

int aos2_debug_initializer_host(const aos2_initializer_problem_t *problems, aos2_initializer_result_t *results, int n_problems)
{
    using namespace aos2;
    if (int st = initializer_check(problems, results, n_problems)) return st;
    for (int p = 0; p < n_problems; ++p) {
        const aos2_initializer_problem_t &P = problems[p];
        aos2_initializer_result_t &R = results[p];
        initializer_result_clear(P, R);
        float nrm1[4], nrm2[4];
        for (int axis = 0; axis < 2; ++axis) {
            init_normalize_axis(P.keys1, P.n_keys1, axis, nrm1 + 2 * axis, nrm1 + 2 * axis + 1);
            init_normalize_axis(P.keys2, P.n_keys2, axis, nrm2 + 2 * axis, nrm2 + 2 * axis + 1);
        }
        const InitPts pts = {P.keys1, P.keys2, P.matches, nrm1, nrm2};
        float H[18] = {}, F[18] = {};
        R.best_iteration_h = initializer_find_host(true, P, pts, &R.SH, H, R.inliers_h);
        R.best_iteration_f = initializer_find_host(false, P, pts, &R.SF, F, R.inliers_f);
        memcpy(R.H21, H, sizeof R.H21);
        memcpy(R.F21, F, sizeof R.F21);
        const float RH = R.SH / (R.SH + R.SF);
        R.used_homography = (double)RH > 0.40;   // (a float against the double 0.40)
        if ((R.used_homography ? R.best_iteration_h : R.best_iteration_f) < 0) {
            R.status = AOS2_INIT_NO_MODEL;
            continue;
        }
        const uint8_t *inl = R.used_homography ? R.inliers_h : R.inliers_f;
        int N = 0;
        for (int i = 0; i < P.n_matches; ++i) N += inl[i] != 0;
        const InitCam cam = {P.fx, P.fy, P.cx, P.cy};
        InitLocal ws;
        float Rs[72], ts[24];
        if (R.used_homography) R.n_hypotheses = init_hyps_h(R.H21, cam, ws, Rs, ts) ? 8 : 0;
        else {
            init_hyps_f(R.F21, cam, ws, Rs, ts);
            R.n_hypotheses = 4;
        }
        if (R.n_hypotheses == 0) continue;
        const float th2 = init_th2(P.sigma);
        std::vector<std::vector<float>> P3D((size_t)R.n_hypotheses, std::vector<float>(3 * (size_t)P.n_keys1, 0.0f));
        std::vector<std::vector<uint8_t>> good((size_t)R.n_hypotheses, std::vector<uint8_t>((size_t)P.n_keys1, 0));
        for (int h = 0; h < R.n_hypotheses; ++h) {
            InitRT S;
            init_rt_setup(Rs + 9 * h, ts + 3 * h, cam, S);
            std::vector<float> cosines;
            for (int i = 0; i < P.n_matches; ++i) {
                if (!inl[i]) continue;
                const int k1 = P.matches[2 * i], k2 = P.matches[2 * i + 1];
                float x[3], c = 0;
                const int code = init_rt_point(S, cam, th2, P.keys1[2 * k1], P.keys1[2 * k1 + 1], P.keys2[2 * k2], P.keys2[2 * k2 + 1], x, &c);
                if (code & INIT_RT_CLEARS) good[h][k1] = 0;
                if (code & INIT_RT_GOOD) {
                    cosines.push_back(c);
                    memcpy(&P3D[h][3 * (size_t)k1], x, 12);
                }
                if (code & INIT_RT_SETS) good[h][k1] = 1;
            }
            R.n_good[h] = (int32_t)cosines.size();
            if (!cosines.empty()) {
                const size_t idx = std::min<size_t>(50, cosines.size() - 1);
                std::vector<uint32_t> keys(cosines.size());
                for (size_t k = 0; k < keys.size(); ++k) keys[k] = init_float_key(cosines[k]);
                std::nth_element(keys.begin(), keys.begin() + idx, keys.end());
                R.parallax[h] = init_parallax_deg(init_key_float(keys[idx]));
            }
        }
        const int pick = R.used_homography ? init_decide_h(R.n_good, R.parallax, N, P.min_parallax, P.min_triangulated)
                                           : init_decide_f(R.n_good, R.parallax, N, P.min_parallax, P.min_triangulated);
        if (pick < 0) continue;
        R.initialized = 1;
        memcpy(R.R21, Rs + 9 * pick, sizeof R.R21);
        memcpy(R.t21, ts + 3 * pick, sizeof R.t21);
        memcpy(R.P3D, P3D[pick].data(), 12 * (size_t)P.n_keys1);
        memcpy(R.triangulated, good[pick].data(), (size_t)P.n_keys1);
    }
    return AOS2_OK;
}

int aos2_debug_initializer_svd(const float *A, int rows, int cols, float *left, float *w, float *right)
{
    using namespace aos2;
    if (!A || !left || !w || !right || rows < 1 || rows > 16 || cols < 1 || cols > 9 || !(rows >= cols || rows + 1 == cols)) {
        set_error("bad argument (the four arrays, rows <= 16, cols <= 9, rows >= cols or rows + 1 == cols)");
        return AOS2_ERR_ARG;
    }
    InitLocal ws;
    const bool wide = rows < cols;
    const int n = wide ? rows : cols, m = wide ? cols : rows, n1 = wide ? cols : n;
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < m; ++k) ws.A(i, k) = wide ? A[i * cols + k] : A[k * cols + i];
    init_jacobi(ws, m, n);
    init_svd_tail(ws, m, n, n1);
    for (int i = 0; i < n1; ++i)
        for (int k = 0; k < m; ++k) left[i * m + k] = ws.A(i, k);
    for (int i = 0; i < n; ++i) {
        w[i] = (float)ws.W(i);
        for (int k = 0; k < n; ++k) right[i * n + k] = ws.V(i, k);
    }
    return AOS2_OK;
}

int aos2_debug_initializer_rng(int n, uint32_t *out)
{
    using namespace aos2;
    if (n < 0 || (n > 0 && !out)) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    InitRng rng{0x12345678};
    for (int i = 0; i < n; ++i) out[i] = rng.next();
    return AOS2_OK;
}

int aos2_debug_initializer_inv33(const float *S, float *inv, double *det)
{
    using namespace aos2;
    if (!S || !inv || !det) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    init_inv33(S, inv);
    *det = init_det33(S);
    return AOS2_OK;
}

int aos2_debug_triangulate_host(const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1, const aos2_triang_obs_t *obs2, float *x3D,
                                uint8_t *status)
{
    using namespace aos2;
    if (int st = triang_check(g, n, obs1, obs2, x3D, status)) return st;
    const TriKf K1 = {g->Tcw1, g->fx1, g->fy1, g->cx1, g->cy1, g->mb1, g->mbf1, g->scale_factors1};
    const TriKf K2 = {g->Tcw2, g->fx2, g->fy2, g->cx2, g->cy2, g->mb2, g->mbf2, g->scale_factors2};
    for (int k = 0; k < n; ++k) {
        const aos2_triang_obs_t &a = obs1[k], &b = obs2[k];
        status[k] = (uint8_t)triangulate_pair(K1, K2, TriObs{a.ux, a.uy, a.kx, a.ky, a.u_right, a.depth, a.octave},
                                              TriObs{b.ux, b.uy, b.kx, b.ky, b.u_right, b.depth, b.octave}, x3D + 3 * (size_t)k);
    }
    return AOS2_OK;
}

int aos2_debug_sim3_host(const aos2_sim3_problem_t *problems, aos2_sim3_result_t *results, int n_problems)
{
    using namespace aos2;
    int32_t its[64];
    uint8_t run[64];
    if (int st = sim3_check(problems, results, n_problems, its, run)) return st;
    for (int p = 0; p < n_problems; ++p) {
        const aos2_sim3_problem_t &P = problems[p];
        aos2_sim3_result_t &R = results[p];
        sim3_result_clear(P, its[p], R);
        if (!run[p]) continue;
        const Sim3Cam K1 = {P.fx1, P.fy1, P.cx1, P.cy1}, K2 = {P.fx2, P.fy2, P.cx2, P.cy2};
        Sim3Scan scan;
        for (int it = 0; it < its[p]; ++it) {
            Sim3Model m;
            sim3_model_of(P.n, P.X3Dc1, P.X3Dc2, P.draws, it, P.fix_scale != 0, m);
            std::vector<uint8_t> flags((size_t)P.n);
            int32_t count = 0;
            for (int i = 0; i < P.n; ++i)
                count += flags[i] = sim3_inlier(m.T12, m.T21, K1, K2, P.X3Dc1 + 3 * (size_t)i, P.X3Dc2 + 3 * (size_t)i, P.max_err1[i], P.max_err2[i]);
            if (R.counts) R.counts[it] = count;
            const bool done = scan.step(it, count, P.min_inliers);
            if (scan.best_iteration == it) {   // :185-190
                memcpy(R.inliers, flags.data(), flags.size());
                for (int r = 0; r < 3; ++r) {
                    memcpy(R.T12 + 4 * r, m.T12 + 4 * r, 16);
                    R.T12[12 + r] = 0.0f;
                }
                R.T12[15] = 1.0f;
                memcpy(R.R12, m.R, sizeof m.R);
                memcpy(R.t12, m.t, sizeof m.t);
                R.s12 = m.s;
            }
            if (done) break;
        }
        R.first_success = scan.first_success;
        R.best_iteration = scan.best_iteration;
        R.best_inliers = scan.best_inliers;
    }
    return AOS2_OK;
}

int aos2_debug_octree_host(const int16_t *xs, const int16_t *ys, const uint8_t *score, int n, int minX, int maxX,
                           int minY, int maxY, int N, int32_t *out_idx, int cap)
{
    using namespace aos2;
    if (n <= 0) return 0;
    const int mn = oct_max_nodes(n, N);
    std::vector<OctNode> nodes(mn);
    std::vector<int32_t> perm(n), tmp(n), pairs((size_t)4 * mn);
    OctScratch S{nodes.data(), perm.data(), tmp.data(), pairs.data(), pairs.data() + 2 * mn, mn, mn};
    return distribute_octree(xs, ys, score, n, minX, maxX, minY, maxY, N, S, out_idx, cap);
}

// countVisible (src/camera.cc:135-198) for every state in turn, one point at a time: the loop the planner runs
static void vis_count_host(const aos2_vis_t *h, int ns, const float *in, bool poses, int32_t *count, float *sum, uint64_t *mask)
{
    using namespace aos2;
    aos2_vis_camera_t cam;
    VisMapView M;
    vis_view(h, &cam, &M);
    const VisGates g = vis_gates(cam);
    const size_t words = (size_t)(M.n + 63) / 64;
    for (int s = 0; s < ns; ++s) {
        const VisState S = poses ? vis_state_from_pose(in + 16 * (size_t)s, cam)
                                 : vis_state_from_xyt(in[3 * (size_t)s], in[3 * (size_t)s + 1], in[3 * (size_t)s + 2], cam);
        if (mask) std::fill(mask + s * words, mask + (s + 1) * words, (uint64_t)0);
        float num_visible = 0;
        for (int i = 0; i < M.n; ++i)
            if (vis_point(g, S, M.x[i], M.y[i], M.z[i], M.upper[i], M.lower[i], M.max_range[i], M.min_range[i])) {
                num_visible += M.ratio[i];
                if (mask) mask[s * words + i / 64] |= (uint64_t)1 << (i % 64);
            }
        if (sum) sum[s] = num_visible;
        count[s] = vis_round(num_visible);
    }
}

int aos2_debug_visibility_host(aos2_vis_t *h, int ns, const float *states, int32_t *count, float *sum, uint64_t *mask)
{
    if (int st = aos2::vis_check_count(h, ns, states, count)) return st;
    vis_count_host(h, ns, states, false, count, sum, mask);
    return AOS2_OK;
}

int aos2_debug_visibility_poses_host(aos2_vis_t *h, int ns, const float *T_wb, int32_t *count, float *sum, uint64_t *mask)
{
    if (int st = aos2::vis_check_count(h, ns, T_wb, count)) return st;
    vis_count_host(h, ns, T_wb, true, count, sum, mask);
    return AOS2_OK;
}

int aos2_debug_visibility_motion_costs_host(aos2_vis_t *h, int nm, const int32_t *offsets, const float *states, int thres, double *cost)
{
    using namespace aos2;
    if (int st = vis_check_motions(h, nm, offsets, states, cost)) return st;
    aos2_vis_camera_t cam;
    VisMapView M;
    vis_view(h, &cam, &M);
    const int thr = thres < 0 ? cam.feature_threshold : thres;
    for (int m = 0; m < nm; ++m) {   // src/StateValidChecker.cc:531-541
        double C = 0;
        for (int i = offsets[m] + 1; i < offsets[m + 1] - 1; ++i) {
            int32_t c;
            vis_count_host(h, 1, states + 3 * (size_t)i, false, &c, nullptr, nullptr);
            C += vis_motion_cost_term(c, thr);
        }
        cost[m] = C;
    }
    return AOS2_OK;
}

int aos2_debug_visibility_advance_host(aos2_vis_t *h, int ns, const float *states, int thres, int32_t *index)
{
    using namespace aos2;
    if (int st = vis_check_advance(h, ns, states, index)) return st;
    aos2_vis_camera_t cam;
    VisMapView M;
    vis_view(h, &cam, &M);
    const int thr = thres == -1 ? cam.feature_threshold : thres;
    int i = 0;   // src/plan.cc:145-148
    for (; i < ns; ++i) {
        int32_t c;
        vis_count_host(h, 1, states + 3 * (size_t)i, false, &c, nullptr, nullptr);
        if (!(c > thr)) break;
    }
    *index = i - 1;
    return AOS2_OK;
}

// Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) of one frame, written the way the reference is: a std::map of votes, a
// std::set of children, the list a std::vector that grows while it is walked, marks per keyframe and per point
// (mnTrackReferenceForFrame).  A keyframe row stands for the KeyFrame*, so the containers iterate in ascending row.
// Returns whether there were votes (:1433).
static bool local_map_frame_host(const aos2_local_map_graph_t &g, int N, int32_t *mp, std::vector<int32_t> &vpLocalKeyFrames,
                                 std::vector<int32_t> &vpLocalMapPoints, int32_t &refKF)
{
    // UpdateLocalKeyFrames :1411-1519
    std::map<int32_t, int> keyframeCounter;
    for (int i = 0; i < N; i++) {
        if (mp[i] >= 0 && mp[i] < g.n_points) {
            const int32_t pMP = mp[i];
            if (!g.point_bad[pMP]) {
                for (int e = g.obs_off[pMP]; e < g.obs_off[pMP + 1]; e++) keyframeCounter[g.obs_kf[e]]++;
            } else {
                mp[i] = -1;
            }
        }
    }
    if (!keyframeCounter.empty()) {
        int max = 0;
        int32_t pKFmax = -1;
        vpLocalKeyFrames.clear();
        vpLocalKeyFrames.reserve(3 * keyframeCounter.size());
        std::vector<uint8_t> inList(g.n_keyframes, 0);
        for (std::map<int32_t, int>::const_iterator it = keyframeCounter.begin(), itEnd = keyframeCounter.end(); it != itEnd; it++) {
            const int32_t pKF = it->first;
            if (g.kf_bad[pKF]) continue;
            if (it->second > max) {
                max = it->second;
                pKFmax = pKF;
            }
            vpLocalKeyFrames.push_back(pKF);
            inList[pKF] = 1;
        }
        const size_t nFirst = vpLocalKeyFrames.size();
        for (size_t itKF = 0; itKF < nFirst; itKF++) {
            if (vpLocalKeyFrames.size() > AOS2_LOCAL_MAP_MAX_KFS) break;
            const int32_t pKF = vpLocalKeyFrames[itKF];
            for (int k = 0; k < AOS2_LOCAL_MAP_NEIGHBOURS; k++) {
                const int32_t pNeighKF = g.kf_best[(size_t)pKF * AOS2_LOCAL_MAP_NEIGHBOURS + k];
                if (pNeighKF < 0) continue;   // (the padding of a shorter list)
                if (!g.kf_bad[pNeighKF]) {
                    if (!inList[pNeighKF]) {
                        vpLocalKeyFrames.push_back(pNeighKF);
                        inList[pNeighKF] = 1;
                        break;
                    }
                }
            }
            const std::set<int32_t> spChilds(g.kf_child + g.kf_child_off[pKF], g.kf_child + g.kf_child_off[pKF + 1]);
            for (std::set<int32_t>::const_iterator sit = spChilds.begin(), send = spChilds.end(); sit != send; sit++) {
                const int32_t pChildKF = *sit;
                if (!g.kf_bad[pChildKF]) {
                    if (!inList[pChildKF]) {
                        vpLocalKeyFrames.push_back(pChildKF);
                        inList[pChildKF] = 1;
                        break;
                    }
                }
            }
            const int32_t pParent = g.kf_parent[pKF];
            if (pParent >= 0) {
                if (!inList[pParent]) {
                    vpLocalKeyFrames.push_back(pParent);
                    inList[pParent] = 1;
                    break;
                }
            }
        }
        if (pKFmax >= 0) refKF = pKFmax;
    }
    // UpdateLocalPoints :1385-1408
    vpLocalMapPoints.clear();
    std::vector<uint8_t> listed(g.n_points, 0);
    for (size_t itKF = 0; itKF < vpLocalKeyFrames.size(); itKF++) {
        const int32_t pKF = vpLocalKeyFrames[itKF];
        if (pKF < 0 || pKF >= g.n_keyframes) continue;   // (a caller's previous list, no votes)
        for (int e = g.kf_mp_off[pKF]; e < g.kf_mp_off[pKF + 1]; e++) {
            const int32_t pMP = g.kf_mp[e];
            if (pMP < 0) continue;
            if (listed[pMP]) continue;
            if (!g.point_bad[pMP]) {
                vpLocalMapPoints.push_back(pMP);
                listed[pMP] = 1;
            }
        }
    }
    return !keyframeCounter.empty();
}

int aos2_debug_local_map_host(const aos2_local_map_graph_t *g, int batch, int cap, const int32_t *n, int32_t *mp, int32_t *local,
                              int local_cap, int32_t *n_local, int32_t *local_kfs, int kf_cap, int32_t *n_local_kfs, int32_t *ref_kf)
{
    if (int st = aos2::local_map_check(g, nullptr)) return st;
    if (batch < 0 || cap <= 0 || local_cap <= 0 || kf_cap <= 0 ||
        (batch > 0 && (!n || !mp || !local || !n_local || !local_kfs || !n_local_kfs || !ref_kf))) {
        aos2::set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    std::vector<int32_t> kfs, pts;
    for (int b = 0; b < batch; ++b) {
        int32_t *lk = local_kfs + (size_t)b * kf_cap, *lp = local + (size_t)b * local_cap;
        const int n_in = std::max(0, std::min(n_local_kfs[b], kf_cap));
        kfs.assign(lk, lk + n_in);
        const int N = std::max(0, std::min(n[b], cap));
        const bool voted = local_map_frame_host(*g, N, mp + (size_t)b * cap, kfs, pts, ref_kf[b]);
        if (voted) {   // (no votes: the caller's rows stand as they are, whatever lies behind its count)
            for (int j = 0; j < kf_cap; ++j) lk[j] = j < (int)kfs.size() ? kfs[j] : -1;
            n_local_kfs[b] = (int32_t)kfs.size();
        }
        for (int j = 0; j < local_cap; ++j) lp[j] = j < (int)pts.size() ? pts[j] : -1;
        n_local[b] = (int32_t)pts.size();
    }
    return AOS2_OK;
}

int aos2_debug_local_map_stats_host(const aos2_local_map_graph_t *g, int batch, int cap, const int32_t *n, int32_t *mp,
                                    const uint8_t *outlier, int stereo, int only_tracking, int32_t *stats, int32_t *found_inc)
{
    if (int st = aos2::local_map_check(g, nullptr)) return st;
    if (batch < 0 || cap <= 0 || (batch > 0 && (!n || !mp || !outlier || !stats))) {
        aos2::set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (int b = 0; b < batch; ++b) {   // src/Tracking.cc:1040-1071
        int mnMatchesInliers = 0, nObsvMappoints = 0, totalObservation = 0;
        const int N = std::max(0, std::min(n[b], cap));
        for (int i = 0; i < N; i++) {
            int32_t &pMP = mp[(size_t)b * cap + i];
            if (pMP >= 0 && pMP < g->n_points) {
                nObsvMappoints++;
                if (!outlier[(size_t)b * cap + i]) {
                    if (found_inc) found_inc[pMP]++;
                    if (!only_tracking) {
                        if (g->point_nobs[pMP] > 0) mnMatchesInliers++;
                        totalObservation += g->point_nobs[pMP];
                    } else
                        mnMatchesInliers++;
                } else if (stereo)
                    pMP = -1;
            }
        }
        stats[3 * (size_t)b] = nObsvMappoints;
        stats[3 * (size_t)b + 1] = mnMatchesInliers;
        stats[3 * (size_t)b + 2] = totalObservation;
    }
    return AOS2_OK;
}

// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:636-700): the loop as the reference runs it, one candidate, one feature and
// one observation at a time, through the per-item functions of csrc/kf_culling.h; SetBadFlag's erasure takes effect at once
int aos2_debug_keyframe_culling_host(const aos2_local_map_graph_t *g, const aos2_kf_culling_view_t *view, int monocular, int n_cand,
                                     const int32_t *cand, uint8_t *status, int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points,
                                     int bad_cap, int32_t *n_bad_points)
{
    using namespace aos2;
    if (int st = local_map_check(g, nullptr)) return st;
    if (int st = kf_culling_check_view(g, view)) return st;
    if (int st = kf_culling_check_call(g->n_keyframes, n_cand, cand, status, n_mps, n_redundant, bad_points, bad_cap, n_bad_points))
        return st;
    const int np = g->n_points;
    const LmGraph G = {{np, g->n_keyframes}, lm_from_public(*g, view)};
    std::vector<int32_t> nobs(g->point_nobs, g->point_nobs + np), stamp(np, -1);
    std::vector<uint8_t> bad(g->point_bad, g->point_bad + np), erased(g->obs_off[np], 0);
    const KfcOverlay X = {nobs.data(), stamp.data(), bad.data(), erased.data()};
    std::vector<int32_t> went_bad;
    for (int ci = 0; ci < n_cand; ci++) {
        const int pKF = cand[ci];
        int nMPs = 0, nRedundantObservations = 0;
        if (!(G.kf_flags[pKF] & 1))
            for (int f = G.kf_mp_off[pKF]; f < G.kf_mp_off[pKF + 1]; f++) {
                const int r = kfc_feature(G, X, monocular ? 1 : 0, pKF, f);
                nMPs += r & 1;
                nRedundantObservations += r >> 1;
            }
        status[ci] = (uint8_t)kfc_status(G.kf_flags[pKF], nMPs, nRedundantObservations);
        n_mps[ci] = nMPs;
        n_redundant[ci] = nRedundantObservations;
        if (status[ci] == AOS2_KFC_CULLED)
            for (int f = G.kf_mp_off[pKF]; f < G.kf_mp_off[pKF + 1]; f++)
                if (kfc_erase(G, X, pKF, ci, f)) went_bad.push_back(G.kf_mp[f]);
    }
    std::sort(went_bad.begin(), went_bad.end());
    *n_bad_points = (int32_t)went_bad.size();
    for (int j = 0; j < std::min<int>((int)went_bad.size(), bad_cap); ++j) bad_points[j] = went_bad[j];
    return AOS2_OK;
}

// KeyFrame::UpdateConnections (src/KeyFrame.cc:350-440): the serial loop of csrc/connections.h over a host graph, with the checks
// of the device call
int aos2_debug_update_connections_host(const aos2_local_map_graph_t *g, int th, int n, const int32_t *kf, const int32_t *n_mp,
                                       const int32_t *mp, int mp_cap, int32_t *n_conn, int32_t *conn_kf, int32_t *conn_w, int conn_cap,
                                       int32_t *n_ordered, int32_t *ordered_kf, int32_t *ordered_w, int ordered_cap)
{
    using namespace aos2;
    if (int st = local_map_check(g, nullptr)) return st;
    const ConnArgs A = {th, n, kf, n_mp, mp, mp_cap, n_conn, conn_kf, conn_w, conn_cap, n_ordered, ordered_kf, ordered_w, ordered_cap};
    char why[200];
    if (conn_check(A, g->n_keyframes, why, sizeof why)) return lm_fail("update connections", "%s", why);
    const LmGraph G = {{g->n_points, g->n_keyframes}, lm_from_public(*g, nullptr)};
    conn_host_run(G, A);
    return AOS2_OK;
}

// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:363-413): the serial loop of csrc/normal_depth.h over a host graph and view, with
// the checks of the device call
int aos2_debug_update_normal_depth_host(const aos2_local_map_graph_t *g, const aos2_kf_culling_view_t *view,
                                        const aos2_normal_depth_t *a)
{
    using namespace aos2;
    if (int st = local_map_check(g, nullptr)) return st;
    if (int st = kf_culling_check_view(g, view)) return st;
    if (!a) return lm_fail("update normal and depth", "the arguments are NULL");
    char why[200];
    if (nd_check(*a, g->n_keyframes, why, sizeof why)) return lm_fail("update normal and depth", "%s", why);
    const LmGraph G = {{g->n_points, g->n_keyframes}, lm_from_public(*g, view)};
    nd_host_run(G, *a);
    return AOS2_OK;
}

// check_collisions (src/collisions.cc:70-94) and countVisible of one state, then isValid (src/StateValidChecker.cc:97-119)
static bool svc_valid_host(const aos2::SvcView &V, const double *q, uint8_t *cfree_out, int32_t *count_out)
{
    using namespace aos2;
    int gate = tw_collision_gate(q, V.n_obs, V.params);
    if (gate < 0) {
        double best = INFINITY;
        for (int i = 0; i < V.n_obs; ++i) {
            const double d2 = tw_obstacle_d2(q, V.obs[2 * (size_t)i], V.obs[2 * (size_t)i + 1]);
            best = d2 < best ? d2 : best;
        }
        gate = tw_collision_free(best, V.params.robot_r, V.obs_r) ? 1 : 0;
    }
    const float f[3] = {(float)q[0], (float)q[1], (float)q[2]};   // the narrowing of countVisible(float, float, float)
    int32_t c;
    vis_count_host(V.vis, 1, f, false, &c, nullptr, nullptr);
    if (cfree_out) *cfree_out = (uint8_t)gate;
    if (count_out) *count_out = c;
    return tw_is_valid(q, gate != 0, c, V.thr, V.params);
}

int aos2_debug_svc_valid_host(aos2_svc_t *h, int ns, const double *states, uint8_t *valid, uint8_t *collision_free, int32_t *count)
{
    using namespace aos2;
    if (int st = svc_check_valid(h, ns, states, valid)) return st;
    SvcView V;
    svc_view(h, &V);
    for (int i = 0; i < ns; ++i)
        valid[i] = svc_valid_host(V, states + 3 * (size_t)i, collision_free ? collision_free + i : nullptr, count ? count + i : nullptr) ? 1 : 0;
    return AOS2_OK;
}

int aos2_debug_svc_motions_host(aos2_svc_t *h, int nm, const double *q1, const double *q2, aos2_svc_motions_out_t *out)
{
    using namespace aos2;
    if (int st = svc_check_motions(h, nm, q1, q2, out)) return st;
    SvcView V;
    svc_view(h, &V);
    out->states_needed = 0;
    std::vector<TwPlan> plans(nm);
    long long total = 0;
    for (int m = 0; m < nm; ++m) {
        tw_shortest_path(q1 + 3 * (size_t)m, q2 + 3 * (size_t)m, V.params.turn_radius, V.params.dt, plans[m]);
        if (plans[m].too_long) {
            set_error("motion checks: a segment of motion %d has more than %d states", m, AOS2_SVC_MAX_SEGMENT_STATES);
            return AOS2_ERR_ARG;
        }
        total += plans[m].n_states;
    }
    out->states_needed = total;
    if (total > 0x7fffffffll / 3) {
        set_error("motion checks: the motions have %lld states together, more than a call takes", total);
        return AOS2_ERR_ARG;
    }
    if (out->states && out->states_capacity < total) {
        set_error("motion checks: the states need %lld rows, the buffer has %lld", total, (long long)out->states_capacity);
        return AOS2_ERR_CAPACITY;
    }
    int32_t off = 0;
    std::vector<double> Q;
    for (int m = 0; m < nm; ++m) {
        const TwPlan &P = plans[m];
        const int n = P.n_states;
        Q.resize(3 * (size_t)n);
        for (int i = 0; i < n; ++i) tw_plan_state(q1 + 3 * (size_t)m, P, i, &Q[3 * (size_t)i]);
        int first = -1;
        double len = 0, camc = 0;
        for (int i = 1; i < n; ++i) {
            int32_t c;
            const bool ok = svc_valid_host(V, &Q[3 * (size_t)i], nullptr, &c);
            if (first < 0 && !ok) first = i;
            len += tw_length_term(&Q[3 * (size_t)(i - 1)], &Q[3 * (size_t)i]);
            if (i < n - 1) camc += vis_motion_cost_term(c, V.thr);
        }
        if (out->path_valid) out->path_valid[m] = (uint8_t)P.valid;
        if (out->type) out->type[m] = P.type;
        for (int k = 0; k < 3; ++k) {
            if (out->t) out->t[3 * (size_t)m + k] = P.t[k];
            if (out->m) out->m[3 * (size_t)m + k] = P.m[k];
        }
        if (out->n_states) out->n_states[m] = n;
        if (out->valid) out->valid[m] = P.valid && first < 0 ? 1 : 0;
        if (out->first_invalid) out->first_invalid[m] = first;
        if (out->cost_length) out->cost_length[m] = len;
        if (out->cost_camera) out->cost_camera[m] = camc;
        if (out->offsets) out->offsets[m] = off;
        if (out->states) std::copy(Q.begin(), Q.end(), out->states + 3 * (size_t)off);
        off += n;
    }
    if (out->offsets) out->offsets[nm] = off;
    return AOS2_OK;
}

void aos2_debug_sincos_host(float angle_rad, float *s, float *c) { aos2::sincos_exact(angle_rad, s, c); }

int aos2_debug_sincos_device(const float *angles, int n, float *s, float *c, int device)
{
    using namespace aos2;
    int st;
    if ((st = bind_device(device))) return st;
    DevBuf<float> da, ds, dc;
    if ((st = da.alloc(n)) || (st = ds.alloc(n)) || (st = dc.alloc(n))) return st;
    AOS2_HIP_CHECK(hipMemcpy(da.p, angles, sizeof(float) * n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(sincos_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, da.p, n, ds.p, dc.p);
    AOS2_HIP_CHECK(hipDeviceSynchronize());
    AOS2_HIP_CHECK(hipMemcpy(s, ds.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    AOS2_HIP_CHECK(hipMemcpy(c, dc.p, sizeof(float) * n, hipMemcpyDeviceToHost));
    da.release(); ds.release(); dc.release();
    return AOS2_OK;
}

int aos2_debug_wave_ops_device(const int32_t *vi, const double *vd, int n_cases, int nt, int32_t *out_i, double *out_d, int device)
{
    using namespace aos2;
    if (!vi || !vd || !out_i || !out_d || n_cases < 1 || (nt != 128 && nt != 256)) {
        set_error("bad argument (the four arrays, >= 1 cases, 128 or 256 threads: the sizes the library scans with)");
        return AOS2_ERR_ARG;
    }
    int st;
    if ((st = bind_device(device))) return st;
    const size_t n = (size_t)n_cases * nt;
    DevBuf<int32_t> di, doi;
    DevBuf<double> dd, dod;
    if ((st = di.alloc(n)) || (st = dd.alloc(n)) || (st = doi.alloc(kWaveOpsI * n)) || (st = dod.alloc(kWaveOpsD * n))) return st;
    AOS2_HIP_CHECK(hipMemcpy(di.p, vi, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    AOS2_HIP_CHECK(hipMemcpy(dd.p, vd, sizeof(double) * n, hipMemcpyHostToDevice));
    if (nt == 128) hipLaunchKernelGGL(wave_ops_kernel<128>, dim3(n_cases), dim3(128), 0, 0, di.p, dd.p, doi.p, dod.p);
    else hipLaunchKernelGGL(wave_ops_kernel<256>, dim3(n_cases), dim3(256), 0, 0, di.p, dd.p, doi.p, dod.p);
    AOS2_HIP_CHECK(hipDeviceSynchronize());
    AOS2_HIP_CHECK(hipMemcpy(out_i, doi.p, sizeof(int32_t) * kWaveOpsI * n, hipMemcpyDeviceToHost));
    AOS2_HIP_CHECK(hipMemcpy(out_d, dod.p, sizeof(double) * kWaveOpsD * n, hipMemcpyDeviceToHost));
    di.release(); dd.release(); doi.release(); dod.release();
    return AOS2_OK;
}

int aos2_debug_row_sums_scatter_device(const double *v, int K, double *out, int32_t *owner, int device)
{
    using namespace aos2;
    if (!v || !out || !owner || (K != 7 && K != 36 && K != 42)) {
        set_error("bad argument (the three arrays, K = 7, 36 or 42)");
        return AOS2_ERR_ARG;
    }
    if (int st = bind_device(device)) return st;
    return K == 7 ? row_sums_scatter_run<7>(v, out, owner) : K == 36 ? row_sums_scatter_run<36>(v, out, owner) : row_sums_scatter_run<42>(v, out, owner);
}

// PNG scanline filters undone in place (PNG specification, section 9: None / Sub / Up / Average / Paeth): `rows` = h rows of
// 1 filter byte + stride data bytes as they come out of zlib; bpp = bytes per complete pixel.  Host code for the optional
// real-data loaders (active-orb-slam2_amd/datasets.py): the Average / Paeth recurrences run byte by byte along a row.
int aos2_png_unfilter(uint8_t *rows, int h, int stride, int bpp)
{
    if (!rows || h < 0 || stride <= 0 || bpp <= 0) return AOS2_ERR_ARG;
    const size_t pitch = (size_t)stride + 1;
    for (int y = 0; y < h; ++y) {
        uint8_t *cur = rows + (size_t)y * pitch + 1;
        const uint8_t *up = y ? rows + (size_t)(y - 1) * pitch + 1 : nullptr;
        const int ft = rows[(size_t)y * pitch];
        for (int x = 0; x < stride; ++x) {
            const int a = x >= bpp ? cur[x - bpp] : 0, b = up ? up[x] : 0, c = (up && x >= bpp) ? up[x - bpp] : 0;
            int pred = 0;
            switch (ft) {
            case 0: break;
            case 1: pred = a; break;
            case 2: pred = b; break;
            case 3: pred = (a + b) >> 1; break;
            case 4: {
                const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
                pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                break;
            }
            default: return AOS2_ERR_ARG;
            }
            cur[x] = (uint8_t)(cur[x] + pred);
        }
    }
    return AOS2_OK;
}

}  // extern "C"
