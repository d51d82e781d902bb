// Optimizer::BundleAdjustment / GlobalBundleAdjustemnt on gfx950 for one map (include/aos2.h: aos2_global_bundle_adjustment; reference
// src/Optimizer.cc:41-237).  The arithmetic is csrc/global_ba.h, shared with the host tap.
//
// The structure does not change over the iterations, so the host works it out once per call (gba_symbolic): the hessian indices, the
// edge lists of every pose and landmark, the 6x6 block pattern of the reduced camera system (pairs of free poses that share a
// landmark) and of its factor (block_ldlt.h), and for every block the list of edge pairs whose product the Schur complement
// subtracts from it, in the oracle's loop order (landmark, then position in the landmark's list).  The values never leave the device.
// An LM iteration is k_gba_linearise, k_gba_sums, k_gba_begin and up to ten trials of (k_gba_landmarks, k_gba_assemble,
// k_gba_factor_solve, k_gba_update, k_gba_trial_edges, k_gba_decide), each of which returns at once when the iteration's trials are
// over.  Every sum is taken by one thread over a host-built list, or by a workgroup in an order that depends on the thread number
// alone: no floating-point atomics.  The host reads the control words once per iteration to stop enqueueing and forwards
// *stop_flag into the mapped word the kernels poll.
//
// The kernels and the host tap run the same per-item functions (gba_item_*) on the same layout: the tap walks the items serially on
// host memory and solves the reduced system with the skyline LDL^T of block_ldlt.h.
#include <algorithm>
#include <vector>

#include "block_ldlt.h"
#include "global_ba.h"

namespace aos2 {

constexpr int kGbaThreads = 256, kGbaRows = kGbaThreads / 16;
constexpr size_t kGbaArenaMax = (size_t)2 << 30;
constexpr int kGbaHostMaxPoses = 2048, kGbaDenseMaxPoses = 512, kGbaFamilies = 6;
static_assert(kGbaThreads == kBlockLdltThreads, "k_gba_factor_solve is one workgroup of block_factor_solve");

struct GbaDev {
    int32_t n_poses, n_points, n_edges, np, nl, robust, n_eblk, pad;
    GbaCam cam;
    double delta_mono, delta_stereo;
    const int32_t *e_pose, *e_point;
    const float *e_obs, *e_w;
    const uint8_t *e_stereo;
    const float *in_Tcw, *in_xyz;
    double *pose[2], *point[2];                 // [n_poses][7], [n_points][3]: the estimates, ctl->cur holds the accepted ones
    double *lin;                                // [n_edges][kGbaLin]
    const int32_t *hpose, *hpoint;              // [np], [nl]: the vertex of a hessian index
    const int32_t *pose_hidx, *point_hidx;      // [n_poses], [n_points]: hessian index or -1
    const int32_t *pe_ptr, *pe_list;            // free pose -> its edges in edge order
    const int32_t *le_ptr, *le_list;            // landmark -> its edges in edge order
    const int32_t *pl_ptr, *pl_list;            // landmark -> its edges with a free pose, by (pose index, edge)
    const int32_t *term_ptr, *term_a, *term_b;  // slot of the reduced system -> the edge pairs it loses, by (landmark, a, b)
    const int32_t *co_ptr, *co_list;            // free pose -> the edges of b_s' Schur part, by (landmark, edge)
    double *Hpp, *bp, *Hll, *bl, *Dinv, *db, *xl;   // [np][36], [6 np], [nl][9], [3 nl], [nl][9], [3 nl], [3 nl]
    double *part_chi;                           // [n_eblk] chi2 of the edges of a workgroup
    BlockSystem sys;                            // H = the reduced system with lambda on its diagonal, b = b_s, x = the poses' step
    GbaControl *ctl;
    const int32_t *abort_word;                  // mapped host memory (the device path), NULL on the host
    float *out_Tcw, *out_xyz;
};

// ---------------------------------------------------------------------------------------------- the items (device and host)
__host__ __device__ inline void gba_item_prepare(const GbaDev &P, int i)
{
    if (i < P.n_poses) {
        double qt[7];
        pose_from_Tcw(P.in_Tcw + 16 * (size_t)i, qt);
        for (int d = 0; d < 7; ++d) P.pose[0][7 * (size_t)i + d] = P.pose[1][7 * (size_t)i + d] = qt[d];
    }
    if (i < P.n_points)
        for (int d = 0; d < 3; ++d) P.point[0][3 * (size_t)i + d] = P.point[1][3 * (size_t)i + d] = (double)P.in_xyz[3 * (size_t)i + d];
    if (i < 3 * P.nl) P.xl[i] = 0;
    if (i < 6 * P.np) P.sys.x[i] = 0;   // a first solve that fails applies the solver's vector as it stands
}

__host__ __device__ inline double gba_delta(const GbaDev &P, int stereo) { return stereo ? P.delta_stereo : P.delta_mono; }

// an edge's linearisation at the accepted estimates -> its robust chi2
__host__ __device__ inline double gba_item_linearise(const GbaDev &P, int e, int cur)
{
    double l[kGbaLin];
    const int st = P.e_stereo[e];
    gba_linearise_edge(P.cam, P.pose[cur] + 7 * (size_t)P.e_pose[e], P.point[cur] + 3 * (size_t)P.e_point[e], P.e_obs + 3 * (size_t)e, st,
                       (double)P.e_w[e], P.robust != 0, gba_delta(P, st), l);
    double *out = P.lin + (size_t)e * kGbaLin;
    for (int i = 0; i < kGbaLin; ++i) out[i] = l[i];
    return l[kGbaChi];
}

// item < 42 np: an entry of Hpp or b of a free pose; then 12 nl: of Hll or b of a landmark.  Each sums its edges in edge order.
__host__ __device__ inline void gba_item_sums(const GbaDev &P, long long item)
{
    const long long nP = 42LL * P.np;
    if (item < nP) {
        const int h = (int)(item / 42), ent = (int)(item % 42);
        double s = 0;
        for (int q = P.pe_ptr[h]; q < P.pe_ptr[h + 1]; ++q) {
            const int e = P.pe_list[q];
            s += gba_pose_term(P.lin + (size_t)e * kGbaLin, P.e_stereo[e] ? 3 : 2, ent);
        }
        if (ent < 36) P.Hpp[(size_t)h * 36 + ent] = s;
        else P.bp[(size_t)h * 6 + ent - 36] = s;
    } else if (item < nP + 12LL * P.nl) {
        const int h = (int)((item - nP) / 12), ent = (int)((item - nP) % 12);
        double s = 0;
        for (int q = P.le_ptr[h]; q < P.le_ptr[h + 1]; ++q) {
            const int e = P.le_list[q];
            s += gba_point_term(P.lin + (size_t)e * kGbaLin, P.e_stereo[e] ? 3 : 2, ent);
        }
        if (ent < 9) P.Hll[(size_t)h * 9 + ent] = s;
        else P.bl[(size_t)h * 3 + ent - 9] = s;
    }
}

// |diagonal entry| i of Hpp (i < 6 np) or Hll
__host__ __device__ inline double gba_diag_abs(const GbaDev &P, int i)
{
    if (i < 6 * P.np) return fabs(P.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]);
    const int j = i - 6 * P.np;
    return fabs(P.Hll[(size_t)(j / 3) * 9 + (j % 3) * 4]);
}

__host__ __device__ inline void gba_item_landmark(const GbaDev &P, int h, double lambda)
{
    double Dinv[9], db[3];
    gba_landmark(P.Hll + (size_t)h * 9, P.bl + (size_t)h * 3, lambda, Dinv, db);
    for (int i = 0; i < 9; ++i) P.Dinv[(size_t)h * 9 + i] = Dinv[i];
    for (int i = 0; i < 3; ++i) P.db[(size_t)h * 3 + i] = db[i];
}

// item < 36 n_slots: an entry of a block of the reduced system; then 6 np: a component of b_s
__host__ __device__ inline void gba_item_assemble(const GbaDev &P, long long item, double lambda)
{
    const long long nH = 36LL * P.sys.n_slots;
    if (item < nH) {
        const int slot = (int)(item / 36), ent = (int)(item % 36), a = ent / 6, b = ent % 6;
        const bool diag = slot < P.np;
        double s = 0;
        if (diag) {
            s = P.Hpp[(size_t)slot * 36 + (a <= b ? a * 6 + b : b * 6 + a)];
            if (a == b) s += lambda;
        }
        for (int q = P.term_ptr[slot]; q < P.term_ptr[slot + 1]; ++q) {
            const int ea = P.term_a[q], eb = P.term_b[q];
            const double *Dinv = P.Dinv + (size_t)P.point_hidx[P.e_point[ea]] * 9;
            s -= gba_block_term(P.lin + (size_t)ea * kGbaLin + kGbaHpl, Dinv, P.lin + (size_t)eb * kGbaLin + kGbaHpl, diag, a, b);
        }
        const_cast<double *>(P.sys.H)[item] = s;
    } else if (item < nH + 6LL * P.np) {
        const int i = (int)(item - nH), h = i / 6, r = i % 6;
        double c = 0;
        for (int q = P.co_ptr[h]; q < P.co_ptr[h + 1]; ++q) {
            const int e = P.co_list[q];
            c += gba_coeff_term(P.lin + (size_t)e * kGbaLin + kGbaHpl, P.db + (size_t)P.point_hidx[P.e_point[e]] * 3, r);
        }
        const_cast<double *>(P.sys.b)[i] = P.bp[i] - c;
    }
}

// item < nl: the step of a landmark (xl = Dinv (b_l - B^T xp), when the reduced system was solved) and its trial estimate;
// item < np: the trial estimate of a free pose
__host__ __device__ inline void gba_item_update(const GbaDev &P, int item, int cur, bool solved)
{
    if (item < P.nl) {
        if (solved) {
            double cl[3] = {P.bl[3 * (size_t)item], P.bl[3 * (size_t)item + 1], P.bl[3 * (size_t)item + 2]};
            for (int q = P.pl_ptr[item]; q < P.pl_ptr[item + 1]; ++q) {
                const int e = P.pl_list[q];
                const double *Bi = P.lin + (size_t)e * kGbaLin + kGbaHpl, *xp = P.sys.x + 6 * (size_t)P.pose_hidx[P.e_pose[e]];
                for (int c = 0; c < 3; ++c)
                    for (int r = 0; r < 6; ++r) cl[c] += Bi[r * 3 + c] * (-xp[r]);
            }
            const double *Dinv = P.Dinv + (size_t)item * 9;
            for (int r = 0; r < 3; ++r) P.xl[3 * (size_t)item + r] = Dinv[r * 3] * cl[0] + Dinv[r * 3 + 1] * cl[1] + Dinv[r * 3 + 2] * cl[2];
        }
        const size_t v = (size_t)P.hpoint[item];
        for (int d = 0; d < 3; ++d) P.point[cur ^ 1][3 * v + d] = P.point[cur][3 * v + d] + P.xl[3 * (size_t)item + d];
    }
    if (item < P.np) {
        const size_t v = (size_t)P.hpose[item];
        double T[7];
        for (int d = 0; d < 7; ++d) T[d] = P.pose[cur][7 * v + d];
        se3_oplus(P.sys.x + 6 * (size_t)item, T);
        for (int d = 0; d < 7; ++d) P.pose[cur ^ 1][7 * v + d] = T[d];
    }
}

// robust chi2 of an edge at the trial estimates
__host__ __device__ inline double gba_item_trial_edge(const GbaDev &P, int e, int cur)
{
    const int st = P.e_stereo[e];
    double er[3];
    gba_edge_error(P.cam, P.pose[cur ^ 1] + 7 * (size_t)P.e_pose[e], P.point[cur ^ 1] + 3 * (size_t)P.e_point[e], P.e_obs + 3 * (size_t)e, st, er);
    return gba_edge_robust_chi2(er, (double)P.e_w[e], st, P.robust != 0, gba_delta(P, st));
}

// term i of the scale of a trial: x_j (lambda x_j + b_j), the poses first
__host__ __device__ inline double gba_scale_term(const GbaDev &P, int i, double lambda)
{
    const int n6 = 6 * P.np;
    const double x = i < n6 ? P.sys.x[i] : P.xl[i - n6], b = i < n6 ? P.bp[i] : P.bl[i - n6];
    return x * (lambda * x + b);
}

// :193-235 as the float32 the reference writes back; a point without an edge keeps its input bit for bit
__host__ __device__ inline void gba_item_finish(const GbaDev &P, int i, int cur)
{
    if (i < P.n_poses) pose_to_Tcw(P.pose[cur] + 7 * (size_t)i, P.out_Tcw + 16 * (size_t)i);
    if (i < P.n_points)
        for (int d = 0; d < 3; ++d)
            P.out_xyz[3 * (size_t)i + d] = P.point_hidx[i] >= 0 ? (float)P.point[cur][3 * (size_t)i + d] : P.in_xyz[3 * (size_t)i + d];
}

// ---------------------------------------------------------------------------------------------- the kernels
// Workgroup maximum of one double per thread, the result in every thread: the shape of block_sum_f64 (wave_ops.h), which takes
// the sums.  Row results by DPP, then every thread combines the 16 row partials in row order.
__device__ __forceinline__ double gba_block_max(double v, double *part)
{
    const int tid = threadIdx.x;
    v = fmax(v, dpp_f64<0xB1>(v));
    v = fmax(v, dpp_f64<0x4E>(v));
    v = fmax(v, dpp_f64<0x141>(v));
    v = fmax(v, dpp_f64<0x140>(v));
    if ((tid & 15) == 0) part[tid >> 4] = v;
    __syncthreads();
    double s = part[0];
    for (int r = 1; r < kGbaRows; ++r) s = fmax(s, part[r]);
    __syncthreads();
    return s;
}

__device__ __forceinline__ bool gba_flag(const GbaDev &P)
{
    return P.abort_word && __hip_atomic_load(P.abort_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_prepare(const GbaDev *__restrict__ Pp)
{
    gba_item_prepare(*Pp, blockIdx.x * kGbaThreads + threadIdx.x);
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_linearise(const GbaDev *__restrict__ Pp)
{
    __shared__ double part[kGbaRows];
    const GbaDev &P = *Pp;
    if (!P.ctl->running) return;
    const int e = blockIdx.x * kGbaThreads + threadIdx.x;
    const double chi = e < P.n_edges ? gba_item_linearise(P, e, P.ctl->cur) : 0.0;
    const double s = block_sum_f64(chi, part);
    if (threadIdx.x == 0) P.part_chi[blockIdx.x] = s;
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_sums(const GbaDev *__restrict__ Pp)
{
    const GbaDev &P = *Pp;
    if (!P.ctl->running) return;
    gba_item_sums(P, (long long)blockIdx.x * kGbaThreads + threadIdx.x);
}

// chi2 of the linearisation (workgroup w's partial in thread w % 256), lambda's start from the largest diagonal entry, the start of
// the iteration; one workgroup
__global__ __launch_bounds__(kGbaThreads) void k_gba_begin(const GbaDev *__restrict__ Pp)
{
    __shared__ double part[kGbaRows];
    const GbaDev &P = *Pp;
    GbaControl *ctl = P.ctl;
    if (!ctl->running) return;
    double chi = 0, mx = 0;
    for (int i = threadIdx.x; i < P.n_eblk; i += kGbaThreads) chi += P.part_chi[i];
    chi = block_sum_f64(chi, part);
    if (ctl->iterations == 0) {
        for (int i = threadIdx.x; i < 6 * P.np + 3 * P.nl; i += kGbaThreads) mx = fmax(gba_diag_abs(P, i), mx);
        mx = gba_block_max(mx, part);
    }
    if (threadIdx.x == 0) gba_iteration_begin(*ctl, chi, mx, gba_flag(P));
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_landmarks(const GbaDev *__restrict__ Pp)
{
    const GbaDev &P = *Pp;
    if (!P.ctl->running || !P.ctl->open) return;
    const int h = blockIdx.x * kGbaThreads + threadIdx.x;
    if (h < P.nl) gba_item_landmark(P, h, P.ctl->lm.lambda);
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_assemble(const GbaDev *__restrict__ Pp)
{
    const GbaDev &P = *Pp;
    if (!P.ctl->running || !P.ctl->open) return;
    gba_item_assemble(P, (long long)blockIdx.x * kGbaThreads + threadIdx.x, P.ctl->lm.lambda);
}

// lambda is on the diagonal already (the Schur complement is taken of H + lambda I)
__global__ __launch_bounds__(kGbaThreads) void k_gba_factor_solve(const GbaDev *__restrict__ Pp)
{
    const GbaDev &P = *Pp;
    if (!P.ctl->running || !P.ctl->open) return;
    block_factor_solve<6>(P.sys, 0.0, &P.ctl->solved);
}

// the same on a system alone (aos2_debug_global_ba_solve_device)
__global__ __launch_bounds__(kGbaThreads) void k_gba_factor_solve_tap(BlockSystem S, double lambda, int32_t *solved) { block_factor_solve<6>(S, lambda, solved); }

__global__ __launch_bounds__(kGbaThreads) void k_gba_update(const GbaDev *__restrict__ Pp)
{
    const GbaDev &P = *Pp;
    if (!P.ctl->running || !P.ctl->open) return;
    gba_item_update(P, blockIdx.x * kGbaThreads + threadIdx.x, P.ctl->cur, P.ctl->solved != 0);
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_trial_edges(const GbaDev *__restrict__ Pp)
{
    __shared__ double part[kGbaRows];
    const GbaDev &P = *Pp;
    if (!P.ctl->running || !P.ctl->open) return;
    const int e = blockIdx.x * kGbaThreads + threadIdx.x;
    const double chi = e < P.n_edges ? gba_item_trial_edge(P, e, P.ctl->cur) : 0.0;
    const double s = block_sum_f64(chi, part);
    if (threadIdx.x == 0) P.part_chi[blockIdx.x] = s;
}

// chi2 and scale of the trial, the decision; one workgroup.  An accepted trial flips ctl->cur: its estimates become the accepted ones.
__global__ __launch_bounds__(kGbaThreads) void k_gba_decide(const GbaDev *__restrict__ Pp)
{
    __shared__ double part[kGbaRows];
    const GbaDev &P = *Pp;
    GbaControl *ctl = P.ctl;
    if (!ctl->running || !ctl->open) return;
    const double lambda = ctl->lm.lambda;
    double chi = 0, scale = 0;
    for (int i = threadIdx.x; i < P.n_eblk; i += kGbaThreads) chi += P.part_chi[i];
    for (int i = threadIdx.x; i < 6 * P.np + 3 * P.nl; i += kGbaThreads) scale += gba_scale_term(P, i, lambda);
    chi = block_sum_f64(chi, part);
    scale = block_sum_f64(scale, part);
    if (threadIdx.x == 0) gba_trial_decide(*ctl, chi, scale, gba_flag(P));
}

__global__ __launch_bounds__(kGbaThreads) void k_gba_finish(const GbaDev *__restrict__ Pp)
{
    gba_item_finish(*Pp, blockIdx.x * kGbaThreads + threadIdx.x, Pp->ctl->cur);
}

// ---------------------------------------------------------------------------------------------- the symbolic phase (host)
struct GbaHost {
    int np = 0, nl = 0, h_blocks = 0;
    bool runs = false;   // initializeOptimization found an edge
    std::vector<int32_t> hpose, hpoint, pose_hidx, point_hidx;
    std::vector<int32_t> pe_ptr, pe_list, le_ptr, le_list, pl_ptr, pl_list, term_ptr, term_a, term_b, co_ptr, co_list;
    std::vector<int32_t> hi, lo;
    BlockSymbolic Y;
};

// a counting sort by `where` that keeps the order of the entries
static void gba_bucket(const std::vector<int32_t> &where, size_t n, std::vector<int32_t> &ptr, std::vector<int32_t> &at)
{
    ptr.assign(n + 1, 0);
    for (int32_t w : where) ptr[(size_t)w + 1]++;
    for (size_t i = 0; i < n; ++i) ptr[i + 1] += ptr[i];
    std::vector<int32_t> next(ptr.begin(), ptr.end() - 1);
    at.resize(where.size());
    for (size_t i = 0; i < where.size(); ++i) at[i] = next[(size_t)where[i]]++;
}

static int gba_check(const aos2_lba_problem_t *p, const aos2_gba_options_t *o, const aos2_gba_result_t *r)
{
    bool ok = p && o && r && p->n_poses >= 0 && p->n_points >= 0 && p->n_edges >= 0 && o->iterations > 0 && o->huber_mono > 0 && o->huber_stereo > 0 &&
              (p->n_poses == 0 || (p->pose_Tcw && p->pose_fixed && p->pose_id && r->pose_Tcw)) &&
              (p->n_points == 0 || (p->point_xyz && p->point_id && r->point_xyz && r->point_included)) &&
              (p->n_edges == 0 || (p->edge_pose && p->edge_point && p->edge_obs && p->edge_stereo && p->edge_inv_sigma2));
    if (!ok) {
        set_error("bad argument (the problem, the options with iterations >= 1 and positive deltas, the result; counts >= 0 and their arrays)");
        return AOS2_ERR_ARG;
    }
    for (int e = 0; e < p->n_edges; ++e)
        if (p->edge_pose[e] < 0 || p->edge_pose[e] >= p->n_poses || p->edge_point[e] < 0 || p->edge_point[e] >= p->n_points) {
            set_error("edge %d references a vertex out of range", e);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

// initializeOptimization's index mapping (free poses with an edge by pose_id, then points with an edge by point_id) and the lists.
// false: the factor does not fit max_bytes.
static bool gba_symbolic(const aos2_lba_problem_t &P, size_t max_bytes, GbaHost &G)
{
    const int ne = P.n_edges;
    std::vector<uint8_t> pose_act((size_t)P.n_poses, 0), point_act((size_t)P.n_points, 0);
    for (int e = 0; e < ne; ++e) pose_act[(size_t)P.edge_pose[e]] = point_act[(size_t)P.edge_point[e]] = 1;
    G.runs = ne > 0;
    G.hpose.clear();
    G.hpoint.clear();
    for (int i = 0; i < P.n_poses; ++i)
        if (pose_act[(size_t)i] && !P.pose_fixed[i]) G.hpose.push_back(i);
    for (int i = 0; i < P.n_points; ++i)
        if (point_act[(size_t)i]) G.hpoint.push_back(i);
    std::stable_sort(G.hpose.begin(), G.hpose.end(), [&](int32_t a, int32_t b) { return P.pose_id[a] < P.pose_id[b]; });
    std::stable_sort(G.hpoint.begin(), G.hpoint.end(), [&](int32_t a, int32_t b) { return P.point_id[a] < P.point_id[b]; });
    G.np = (int)G.hpose.size();
    G.nl = (int)G.hpoint.size();
    G.pose_hidx.assign((size_t)P.n_poses, -1);
    G.point_hidx.assign((size_t)P.n_points, -1);
    for (int h = 0; h < G.np; ++h) G.pose_hidx[(size_t)G.hpose[(size_t)h]] = h;
    for (int h = 0; h < G.nl; ++h) G.point_hidx[(size_t)G.hpoint[(size_t)h]] = h;
    // the edge lists of the poses and of the landmarks, in edge order
    std::vector<int32_t> where, what, at;
    for (int e = 0; e < ne; ++e)
        if (G.pose_hidx[(size_t)P.edge_pose[e]] >= 0) {
            where.push_back(G.pose_hidx[(size_t)P.edge_pose[e]]);
            what.push_back(e);
        }
    gba_bucket(where, (size_t)G.np, G.pe_ptr, at);
    G.pe_list.resize(what.size());
    for (size_t i = 0; i < what.size(); ++i) G.pe_list[(size_t)at[i]] = what[i];
    where.clear();
    for (int e = 0; e < ne; ++e) where.push_back(G.point_hidx[(size_t)P.edge_point[e]]);
    gba_bucket(where, (size_t)G.nl, G.le_ptr, at);
    G.le_list.resize((size_t)ne);
    for (int e = 0; e < ne; ++e) G.le_list[(size_t)at[(size_t)e]] = e;
    // a landmark's column of Hpl: its edges with a free pose, ascending pose index, then edge
    G.pl_ptr.assign((size_t)G.nl + 1, 0);
    G.pl_list.clear();
    for (int l = 0; l < G.nl; ++l) {
        const size_t b = G.pl_list.size();
        for (int q = G.le_ptr[(size_t)l]; q < G.le_ptr[(size_t)l + 1]; ++q)
            if (G.pose_hidx[(size_t)P.edge_pose[G.le_list[(size_t)q]]] >= 0) G.pl_list.push_back(G.le_list[(size_t)q]);
        std::stable_sort(G.pl_list.begin() + (long)b, G.pl_list.end(),
                         [&](int32_t x, int32_t y) { return G.pose_hidx[(size_t)P.edge_pose[x]] < G.pose_hidx[(size_t)P.edge_pose[y]]; });
        G.pl_ptr[(size_t)l + 1] = (int32_t)G.pl_list.size();
    }
    auto hp = [&](int32_t e) { return G.pose_hidx[(size_t)P.edge_pose[e]]; };
    // the pattern: pairs of free poses that share a landmark
    G.hi.clear();
    G.lo.clear();
    for (int l = 0; l < G.nl; ++l)
        for (int a = G.pl_ptr[(size_t)l]; a < G.pl_ptr[(size_t)l + 1]; ++a)
            for (int b = a + 1; b < G.pl_ptr[(size_t)l + 1]; ++b) {
                const int i1 = hp(G.pl_list[(size_t)a]), i2 = hp(G.pl_list[(size_t)b]);
                if (i1 != i2 && (G.hi.empty() || G.hi.back() != i2 || G.lo.back() != i1)) {
                    G.hi.push_back(i2);
                    G.lo.push_back(i1);
                }
            }
    if (!block_symbolic(G.np, G.hi, G.lo, 36, max_bytes, G.Y)) return false;
    // the terms of every block, by (landmark, a, b): solve_schur's loop order
    const size_t n_slots = (size_t)G.np + G.Y.l_blocks();
    std::vector<int32_t> ta, tb, cw, ce;
    where.clear();
    for (int l = 0; l < G.nl; ++l)
        for (int a = G.pl_ptr[(size_t)l]; a < G.pl_ptr[(size_t)l + 1]; ++a) {
            const int32_t ea = G.pl_list[(size_t)a];
            const int i1 = hp(ea);
            cw.push_back(i1);
            ce.push_back(ea);
            for (int b = a; b < G.pl_ptr[(size_t)l + 1]; ++b) {
                const int32_t eb = G.pl_list[(size_t)b];
                const int i2 = hp(eb);
                where.push_back(i1 == i2 ? i1 : G.Y.slot(i2, i1));
                ta.push_back(ea);
                tb.push_back(eb);
            }
        }
    gba_bucket(where, n_slots, G.term_ptr, at);
    G.term_a.resize(ta.size());
    G.term_b.resize(ta.size());
    for (size_t i = 0; i < ta.size(); ++i) {
        G.term_a[(size_t)at[i]] = ta[i];
        G.term_b[(size_t)at[i]] = tb[i];
    }
    gba_bucket(cw, (size_t)G.np, G.co_ptr, at);
    G.co_list.resize(ce.size());
    for (size_t i = 0; i < ce.size(); ++i) G.co_list[(size_t)at[i]] = ce[i];
    G.h_blocks = 0;
    for (size_t s = (size_t)G.np; s < n_slots; ++s) G.h_blocks += G.term_ptr[s + 1] > G.term_ptr[s];
    return true;
}

static inline int gba_blocks(long long items) { return (int)std::max<long long>(1, (items + kGbaThreads - 1) / kGbaThreads); }

// The layout of a call: what the host stages (a prefix), the control words and the results (neighbours, read back together), the
// scratch, and the grids of the launches.  Every array is registered with the field of D that points at it (regions.h), so the
// object stays where it is between plan() and bind().  `base` is device memory for the kernels and host memory for the tap.
struct GbaLayout {
    HostArena H;
    GbaDev D;                    // as bind() completes it
    const GbaDev *dP = nullptr;  // ... and where the kernels find it
    size_t o_dev = 0, o_ctl = 0, in_bytes = 0, res_bytes = 0;
    int g_prep = 1, g_sums = 1, g_land = 1, g_asm = 1, g_upd = 1, g_fin = 1, n_eblk = 1;   // workgroups of the launches

    void plan(const aos2_lba_problem_t &P, const aos2_gba_options_t &O, const GbaHost &G, int stop_at_poll)
    {
        const size_t ne = (size_t)P.n_edges, npo = (size_t)P.n_poses, npt = (size_t)P.n_points, np = (size_t)G.np, nl = (size_t)G.nl;
        const size_t n_slots = np + G.Y.l_blocks();
        n_eblk = gba_blocks((long long)ne);
        g_prep = gba_blocks(std::max<long long>(std::max(P.n_poses, P.n_points), std::max(6LL * G.np, 3LL * G.nl)));
        g_sums = gba_blocks(42LL * G.np + 12LL * G.nl);
        g_land = gba_blocks(G.nl);
        g_asm = gba_blocks(36LL * (long long)n_slots + 6LL * G.np);
        g_upd = gba_blocks(std::max(G.np, G.nl));
        g_fin = gba_blocks(std::max(P.n_poses, P.n_points));
        memset((void *)&D, 0, sizeof D);
        D.n_poses = P.n_poses; D.n_points = P.n_points; D.n_edges = P.n_edges; D.np = G.np; D.nl = G.nl; D.robust = O.robust != 0;
        D.n_eblk = n_eblk;
        // KeyFrame::fx .. mbf are float members copied into the edges' double fields (:113-116, :142-146)
        D.cam.fx = (double)P.fx; D.cam.fy = (double)P.fy; D.cam.cx = (double)P.cx; D.cam.cy = (double)P.cy; D.cam.bf = (double)P.bf; D.cam.bf_f = P.bf;
        D.delta_mono = (double)O.huber_mono; D.delta_stereo = (double)O.huber_stereo;
        D.sys.nf = G.np; D.sys.n_slots = (int32_t)n_slots;
        H.in(D.e_pose, P.edge_pose, ne);
        H.in(D.e_point, P.edge_point, ne);
        H.in(D.e_obs, P.edge_obs, 3 * ne);
        H.in(D.e_w, P.edge_inv_sigma2, ne);
        H.in(D.e_stereo, P.edge_stereo, ne);
        H.in(D.in_Tcw, P.pose_Tcw, 16 * npo);
        H.in(D.in_xyz, P.point_xyz, 3 * npt);
        H.in(D.hpose, G.hpose); H.in(D.hpoint, G.hpoint); H.in(D.pose_hidx, G.pose_hidx); H.in(D.point_hidx, G.point_hidx);
        H.in(D.pe_ptr, G.pe_ptr); H.in(D.pe_list, G.pe_list); H.in(D.le_ptr, G.le_ptr); H.in(D.le_list, G.le_list);
        H.in(D.pl_ptr, G.pl_ptr); H.in(D.pl_list, G.pl_list);
        H.in(D.term_ptr, G.term_ptr); H.in(D.term_a, G.term_a); H.in(D.term_b, G.term_b);
        H.in(D.co_ptr, G.co_ptr); H.in(D.co_list, G.co_list);
        H.in(D.sys.colptr, G.Y.colptr); H.in(D.sys.rowidx, G.Y.rowidx); H.in(D.sys.upd_ptr, G.Y.upd_ptr); H.in(D.sys.upd_dst, G.Y.upd_dst);
        o_dev = H.in(dP, &D, 1);   // (bind() writes D there)
        GbaControl c;
        gba_control_init(c, O.iterations, G.runs, stop_at_poll);
        o_ctl = H.in(D.ctl, &c, 1);
        in_bytes = H.host_size;
        H.room(D.out_Tcw, 16 * npo);
        H.room(D.out_xyz, 3 * npt);
        res_bytes = H.size - o_ctl;
        for (int k = 0; k < 2; ++k) {
            H.room(D.pose[k], 7 * npo);
            H.room(D.point[k], 3 * npt);
        }
        H.room(D.lin, kGbaLin * ne);
        H.room(D.Hpp, 36 * np); H.room(D.bp, 6 * np);
        H.room(D.Hll, 9 * nl); H.room(D.bl, 3 * nl);
        H.room(D.Dinv, 9 * nl); H.room(D.db, 3 * nl); H.room(D.xl, 3 * nl);
        H.room(D.part_chi, (size_t)n_eblk);
        H.room(D.sys.H, 36 * n_slots); H.room(D.sys.L, 36 * n_slots);
        H.room(D.sys.b, 6 * np); H.room(D.sys.y, 6 * np); H.room(D.sys.x, 6 * np);
    }

    // points D at the arena at `base` and writes it into the staged prefix
    void bind(uint8_t *base, const int32_t *abort_word)
    {
        H.bind(base);
        D.abort_word = abort_word;
        memcpy(H.own.data() + o_dev, &D, sizeof D);
    }
};

// what a call takes beside the factor, per edge / pose / point / pair of a landmark's edges (an upper bound of the lists)
static size_t gba_fixed_bytes(const aos2_lba_problem_t &P)
{
    return (size_t)P.n_edges * (8 * kGbaLin + 4 * 12 + 32) + (size_t)P.n_poses * (64 * 2 + 56 * 2 + 288 + 48 * 4 + 64) +
           (size_t)P.n_points * (12 * 2 + 24 * 2 + 72 * 2 + 24 * 3 + 32) + ((size_t)64 << 10);
}

static void gba_result(const GbaControl &c, const GbaHost &G, const aos2_lba_problem_t &P, const uint8_t *res, const GbaLayout &Lay, float ms,
                       aos2_gba_result_t &R)
{
    R.iterations = c.iterations;
    R.trials = c.trials;
    R.chi2_initial = G.runs ? c.chi2_initial : 0;
    R.chi2_final = G.runs ? c.lm.currentChi : 0;
    R.final_lambda = c.lm.lambda;
    R.polls = c.polls;
    R.stop_poll = c.stop_poll;
    R.h_blocks = G.h_blocks;
    R.l_blocks = (int32_t)G.Y.l_blocks();
    R.ms_device = ms;
    R.status = AOS2_OK;
    const GbaDev &D = Lay.D;
    if (P.n_poses > 0) memcpy(R.pose_Tcw, span_copy(res, D.ctl, D.out_Tcw), bytes_of(D.out_Tcw, 16 * (size_t)P.n_poses));
    if (P.n_points > 0) memcpy(R.point_xyz, span_copy(res, D.ctl, D.out_xyz), bytes_of(D.out_xyz, 3 * (size_t)P.n_points));
    for (int i = 0; i < P.n_points; ++i) R.point_included[i] = G.point_hidx[(size_t)i] >= 0;
}

// the symbolic phase of a call with its memory check
static int gba_host_phase(const aos2_lba_problem_t &P, GbaHost &G)
{
    const size_t fixed = gba_fixed_bytes(P);
    // (the term lists: 12 bytes per pair of a landmark's edges; counted with the factor's budget)
    size_t pairs = 0;
    {
        std::vector<int32_t> deg((size_t)P.n_points, 0);
        for (int e = 0; e < P.n_edges; ++e) deg[(size_t)P.edge_point[e]]++;
        for (int32_t d : deg) pairs += (size_t)d * ((size_t)d + 1) / 2;
    }
    const size_t lists = pairs * 12;
    if (fixed + lists > kGbaArenaMax || !gba_symbolic(P, kGbaArenaMax - fixed - lists, G)) {
        set_error("the map and the factor of its reduced camera system do not fit the %zu MiB a call may take", kGbaArenaMax >> 20);
        return AOS2_ERR_GBA_MEMORY;
    }
    return AOS2_OK;
}

static bool gba_stop_requested(const aos2_lba_problem_t &P) { return P.stop_flag && *P.stop_flag != 0; }

// ---------------------------------------------------------------------------------------------- the host tap
static void gba_host_linearise(const GbaDev &D, double &chi)
{
    chi = 0;
    for (int e = 0; e < D.n_edges; ++e) chi += gba_item_linearise(D, e, D.ctl->cur);
    for (long long it = 0; it < 42LL * D.np + 12LL * D.nl; ++it) gba_item_sums(D, it);
}

static void gba_host_reduce(const GbaDev &D, double lambda)
{
    for (int h = 0; h < D.nl; ++h) gba_item_landmark(D, h, lambda);
    for (long long it = 0; it < 36LL * D.sys.n_slots + 6LL * D.np; ++it) gba_item_assemble(D, it, lambda);
}

static void gba_host_run(const aos2_lba_problem_t &P, const GbaHost &G, const GbaDev &D)
{
    GbaControl &ctl = *D.ctl;
    for (int i = 0; i < std::max(std::max(P.n_poses, P.n_points), std::max(6 * G.np, 3 * G.nl)); ++i) gba_item_prepare(D, i);
    if (G.runs) {
        SkylineLdlt K;
        K.shape(G.np, G.hi, G.lo, 6);
        std::vector<double> b((size_t)K.n), x((size_t)K.n, 0.0);
        while (ctl.running) {
            double chi, mx = 0;
            gba_host_linearise(D, chi);
            if (ctl.iterations == 0)
                for (int i = 0; i < 6 * D.np + 3 * D.nl; ++i) mx = fmax(gba_diag_abs(D, i), mx);
            gba_iteration_begin(ctl, chi, mx, gba_stop_requested(P));
            while (ctl.running && ctl.open) {
                const double lambda = ctl.lm.lambda;
                gba_host_reduce(D, lambda);
                // the lower triangle of the reduced system into the envelope
                std::fill(K.A.begin(), K.A.end(), 0.0);
                for (int s = 0; s < D.sys.n_slots; ++s) {
                    int row = s, col = s;
                    if (s >= G.np) {
                        const int p = s - G.np;
                        row = G.Y.rowidx[(size_t)p];
                        col = (int)(std::upper_bound(G.Y.colptr.begin(), G.Y.colptr.end(), p) - G.Y.colptr.begin()) - 1;
                        if (G.term_ptr[(size_t)s + 1] == G.term_ptr[(size_t)s]) continue;   // fill only: outside the envelope of A it may be
                    }
                    for (int a = 0; a < 6; ++a)
                        for (int c = 0; c < (s < G.np ? a + 1 : 6); ++c) K.a(K.A, 6 * row + a, 6 * col + c) = D.sys.H[(size_t)s * 36 + a * 6 + c];
                }
                for (int i = 0; i < K.n; ++i) b[(size_t)i] = D.sys.b[i];
                ctl.solved = K.solve(0.0, b, x);
                for (int i = 0; i < K.n; ++i) D.sys.x[i] = x[(size_t)i];
                for (int i = 0; i < std::max(D.np, D.nl); ++i) gba_item_update(D, i, ctl.cur, ctl.solved != 0);
                double temp = 0, scale = 0;
                for (int e = 0; e < D.n_edges; ++e) temp += gba_item_trial_edge(D, e, ctl.cur);
                for (int i = 0; i < 6 * D.np + 3 * D.nl; ++i) scale += gba_scale_term(D, i, lambda);
                gba_trial_decide(ctl, temp, scale, gba_stop_requested(P));
            }
        }
    }
    for (int i = 0; i < std::max(P.n_poses, P.n_points); ++i) gba_item_finish(D, i, ctl.cur);
}

}  // namespace aos2

using namespace aos2;

extern "C" {

int aos2_global_bundle_adjustment(aos2_lba_t *s, const aos2_lba_problem_t *p, const aos2_gba_options_t *o, aos2_gba_result_t *r)
{
    if (!s) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int st = gba_check(p, o, r);
    if (st) return st;
    GbaHost G;
    if ((st = gba_host_phase(*p, G))) return st;
    GbaLayout Lay;
    Lay.plan(*p, *o, G, s->debug_stop_at_poll);
    if (Lay.H.size + 256 > kGbaArenaMax + ((size_t)64 << 20)) {
        set_error("the map does not fit the %zu MiB a call may take", kGbaArenaMax >> 20);
        return AOS2_ERR_GBA_MEMORY;
    }
    if ((st = lba_handle_init(s))) return st;
    s->last_gba_ms = 0;
    if ((st = s->arena.alloc(Lay.H.size + 256))) return st;
    if ((st = s->h_stage.alloc(Lay.res_bytes + 64))) return st;
    if ((st = s->h_abort.alloc(2))) return st;
    int32_t *d_abort = nullptr;
    AOS2_HIP_CHECK(hipHostGetDevicePointer((void **)&d_abort, s->h_abort.p, 0));
    __atomic_store_n(&s->h_abort.p[0], gba_stop_requested(*p) ? 1 : 0, __ATOMIC_RELAXED);
    Lay.bind(s->arena.p, d_abort);
    hipStream_t q = s->stream;
    const GbaDev *dP = Lay.dP;
    AOS2_HIP_CHECK(hipMemcpyAsync(s->arena.p, Lay.H.data(), Lay.in_bytes, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipEventRecord(s->ev[0], q));
    // profiling (aos2_debug_global_ba_profile): an event pair around every family of launches, summed after the call
    LaunchProfiler prof{s->gba_profile, q};
    const dim3 T(kGbaThreads);
    prof.mark(5, true);
    hipLaunchKernelGGL(k_gba_prepare, dim3(Lay.g_prep), T, 0, q, dP);
    prof.mark(5, false);
    GbaControl *hctl = (GbaControl *)s->h_stage.p;
    bool any = G.runs;
    for (int it = 0; any && it < o->iterations; ++it) {
        prof.mark(0, true);
        hipLaunchKernelGGL(k_gba_linearise, dim3(Lay.n_eblk), T, 0, q, dP);
        hipLaunchKernelGGL(k_gba_sums, dim3(Lay.g_sums), T, 0, q, dP);
        prof.mark(0, false);
        prof.mark(4, true);
        hipLaunchKernelGGL(k_gba_begin, dim3(1), T, 0, q, dP);
        prof.mark(4, false);
        for (int t = 0; t < 10; ++t) {
            prof.mark(1, true);
            hipLaunchKernelGGL(k_gba_landmarks, dim3(Lay.g_land), T, 0, q, dP);
            prof.mark(1, false);
            prof.mark(2, true);
            hipLaunchKernelGGL(k_gba_assemble, dim3(Lay.g_asm), T, 0, q, dP);
            prof.mark(2, false);
            prof.mark(3, true);
            hipLaunchKernelGGL(k_gba_factor_solve, dim3(1), T, 0, q, dP);
            prof.mark(3, false);
            prof.mark(1, true);
            hipLaunchKernelGGL(k_gba_update, dim3(Lay.g_upd), T, 0, q, dP);
            prof.mark(1, false);
            prof.mark(4, true);
            hipLaunchKernelGGL(k_gba_trial_edges, dim3(Lay.n_eblk), T, 0, q, dP);
            hipLaunchKernelGGL(k_gba_decide, dim3(1), T, 0, q, dP);
            prof.mark(4, false);
        }
        AOS2_HIP_CHECK(hipMemcpyAsync(hctl, Lay.D.ctl, sizeof(GbaControl), hipMemcpyDeviceToHost, q));
        AOS2_HIP_CHECK(hipStreamSynchronize(q));
        AOS2_HIP_CHECK(hipGetLastError());
        any = hctl->running != 0;
        if (gba_stop_requested(*p)) __atomic_store_n(&s->h_abort.p[0], 1, __ATOMIC_RELAXED);
    }
    prof.mark(5, true);
    hipLaunchKernelGGL(k_gba_finish, dim3(Lay.g_fin), T, 0, q, dP);
    prof.mark(5, false);
    AOS2_HIP_CHECK(hipEventRecord(s->ev[1], q));
    AOS2_HIP_CHECK(hipMemcpyAsync(s->h_stage.p, Lay.D.ctl, Lay.res_bytes, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    (void)hipEventElapsedTime(&s->last_gba_ms, s->ev[0], s->ev[1]);
    prof.sum(s->gba_family_ms, kGbaFamilies);
    GbaControl c;
    memcpy(&c, s->h_stage.p, sizeof c);
    gba_result(c, G, *p, s->h_stage.p, Lay, s->last_gba_ms, *r);
    return AOS2_OK;
}

int aos2_debug_global_ba_profile(aos2_lba_t *s, int on, float *family_ms)
{
    static_assert(sizeof(aos2_lba::gba_family_ms) == sizeof(float) * kGbaFamilies, "the families of include/aos2.h");
    return LaunchProfiler::entry(s, &aos2_lba::gba_profile, &aos2_lba::gba_family_ms, on, family_ms);
}

int aos2_debug_global_ba_host(const aos2_lba_problem_t *p, const aos2_gba_options_t *o, aos2_gba_result_t *r, int stop_at_poll)
{
    int st = gba_check(p, o, r);
    if (st) return st;
    if (p->n_poses > kGbaHostMaxPoses) {
        set_error("more than %d keyframes", kGbaHostMaxPoses);
        return AOS2_ERR_CAPACITY;
    }
    GbaHost G;
    if ((st = gba_host_phase(*p, G))) return st;
    GbaLayout Lay;
    Lay.plan(*p, *o, G, stop_at_poll);
    std::vector<uint8_t> mem(Lay.H.size + 256, 0);
    memcpy(mem.data(), Lay.H.data(), Lay.in_bytes);
    Lay.bind(mem.data(), nullptr);
    gba_host_run(*p, G, Lay.D);
    gba_result(*Lay.D.ctl, G, *p, (const uint8_t *)Lay.D.ctl, Lay, 0.f, *r);
    return AOS2_OK;
}

int aos2_debug_global_ba_reduced_device(aos2_lba_t *s, const aos2_lba_problem_t *p, const aos2_gba_options_t *o, double lambda, int32_t n_free,
                                        double *S, double *bs, int32_t *h_blocks)
{
    aos2_gba_result_t none;
    memset(&none, 0, sizeof none);
    float dummy_f = 0;
    uint8_t dummy_b = 0;
    none.pose_Tcw = none.point_xyz = &dummy_f;   // (gba_check wants a result; this call writes none)
    none.point_included = &dummy_b;
    if (!s || !S || !bs || !h_blocks || n_free < 1 || n_free > kGbaDenseMaxPoses) {
        set_error("bad argument (the handle, the outputs, 1 <= n_free <= %d)", kGbaDenseMaxPoses);
        return AOS2_ERR_ARG;
    }
    int st = gba_check(p, o, &none);
    if (st) return st;
    GbaHost G;
    if ((st = gba_host_phase(*p, G))) return st;
    if (G.np != n_free) {
        set_error("the problem has %d free keyframes with an edge, not %d", G.np, n_free);
        return AOS2_ERR_ARG;
    }
    GbaLayout Lay;
    Lay.plan(*p, *o, G, 0);
    if ((st = lba_handle_init(s))) return st;
    if ((st = s->arena.alloc(Lay.H.size + 256))) return st;
    Lay.bind(s->arena.p, nullptr);
    // the control words of an open first trial at the given lambda
    GbaControl c;
    gba_control_init(c, 1, true, 0);
    c.open = 1;
    c.lm.lambda = lambda;
    memcpy(Lay.H.own.data() + Lay.o_ctl, &c, sizeof c);
    hipStream_t q = s->stream;
    const GbaDev &D = Lay.D;
    const dim3 T(kGbaThreads);
    const size_t n6 = 6 * (size_t)G.np;
    std::vector<double> Hs((size_t)D.sys.n_slots * 36);
    AOS2_HIP_CHECK(hipMemcpyAsync(s->arena.p, Lay.H.data(), Lay.in_bytes, hipMemcpyHostToDevice, q));
    hipLaunchKernelGGL(k_gba_prepare, dim3(Lay.g_prep), T, 0, q, Lay.dP);
    hipLaunchKernelGGL(k_gba_linearise, dim3(Lay.n_eblk), T, 0, q, Lay.dP);
    hipLaunchKernelGGL(k_gba_sums, dim3(Lay.g_sums), T, 0, q, Lay.dP);
    hipLaunchKernelGGL(k_gba_landmarks, dim3(Lay.g_land), T, 0, q, Lay.dP);
    hipLaunchKernelGGL(k_gba_assemble, dim3(Lay.g_asm), T, 0, q, Lay.dP);
    AOS2_HIP_CHECK(hipMemcpyAsync(Hs.data(), D.sys.H, bytes_of(D.sys.H, Hs.size()), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(bs, D.sys.b, bytes_of(D.sys.b, n6), hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    AOS2_HIP_CHECK(hipGetLastError());
    block_dense<6>(G.Y, Hs.data(), true, S);   // a diagonal block is given by its lower triangle
    *h_blocks = G.h_blocks;
    return AOS2_OK;
}

int aos2_debug_global_ba_solve_device(aos2_lba_t *s, int n_blocks, int n_off, const int32_t *rows, const int32_t *cols, const double *val,
                                      const double *diag, const double *b, double lambda, double *x, int32_t *ok, int32_t *l_blocks)
{
    return block_solve_tap<6, k_gba_factor_solve_tap>(s, 8192, AOS2_ERR_GBA_MEMORY, kGbaArenaMax, n_blocks, n_off, rows, cols, val, diag, b, lambda, x, ok,
                                                      l_blocks);
}

}  // extern "C"
