// Optimizer::BundleAdjustment (reference src/Optimizer.cc:41-237) as arithmetic: the one definition that the device kernels
// (global_ba.hip) and the host tap (aos2_debug_global_ba_host) both run.  SE3 / quaternion arithmetic, the Huber kernel and the 3x3
// inverse are lba_math.h's, the Levenberg-Marquardt decisions sim3_opt.h's SoLm; new here, restated from g2o in the order
// oracle/lba_oracle.c executes them:
//   Edge{,Stereo}SE3ProjectXYZ::computeError / linearizeOplus   types/types_six_dof_expmap.{h,cpp} (the float invz of the stereo projection)
//   BaseBinaryEdge::constructQuadraticForm                       core/base_binary_edge.hpp:55-120
//   BlockSolver<6,3>::solve (Schur complement)                   core/block_solver.hpp:367-486
//   SparseOptimizer::optimize, terminate()                       core/sparse_optimizer.cpp:354-419
// The conventions are DESIGN.md section 2 item 15.
#pragma once
#include "sim3_opt.h"

namespace aos2 {

struct GbaCam {
    double fx, fy, cx, cy, bf;
    float bf_f;   // cam_project takes bf as `const float &` (.cpp:150)
};

// what an edge keeps of one linearisation, kGbaLin doubles:
//   [0, 9) A = d e / d point (3x3, row d)   [9, 27) B = d e / d pose (3x6)   [27, 30) -rho' Omega e   [30] rho' w   [31] rho(chi2)
//   [32, 50) the 6x3 block B^T (rho' Omega) A of Hpl
constexpr int kGbaLin = 50, kGbaA = 0, kGbaB = 9, kGbaOr = 27, kGbaWo = 30, kGbaChi = 31, kGbaHpl = 32;

__host__ __device__ inline void gba_edge_error(const GbaCam &cam, const double qt[7], const double X[3], const float *obs, int stereo, double er[3])
{
    double p[3];
    se3_map(qt, X, p);
    if (!stereo) {
        const double u = p[0] / p[2], v = p[1] / p[2];
        er[0] = (double)obs[0] - (u * cam.fx + cam.cx);
        er[1] = (double)obs[1] - (v * cam.fy + cam.cy);
        er[2] = 0;
    } else {
        const float invz = (float)(1.0 / p[2]);
        const double r0 = p[0] * invz * cam.fx + cam.cx;
        const double r1 = p[1] * invz * cam.fy + cam.cy;
        const double r2 = r0 - (double)(cam.bf_f * invz);
        er[0] = (double)obs[0] - r0;
        er[1] = (double)obs[1] - r1;
        er[2] = (double)obs[2] - r2;
    }
}

// chi2 of an edge as activeRobustChi2 counts it
__host__ __device__ inline double gba_edge_robust_chi2(const double er[3], double w, int stereo, bool robust, double delta)
{
    const double c = edge_chi2(er, w, stereo ? 3 : 2);
    if (!robust) return c;
    double rho[2];
    robustify(c, delta, rho);
    return rho[0];
}

// linearizeOplus (.cpp:103-139 mono, :188-234 stereo): Ji = d e / d point, Jj = d e / d pose
__host__ __device__ inline void gba_edge_jacobians(const GbaCam &cam, const double qt[7], const double X[3], int stereo, double Ji[9], double Jj[18])
{
    double p[3], R[9];
    se3_map(qt, X, p);
    rot_from_quat(qt, R);
    const double x = p[0], y = p[1], z = p[2], z_2 = z * z, fx = cam.fx, fy = cam.fy, bf = cam.bf;
    for (int i = 0; i < 9; ++i) Ji[i] = 0;
    for (int i = 0; i < 18; ++i) Jj[i] = 0;
    if (!stereo) {
        const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
        const double s = -1. / z;
        for (int r = 0; r < 2; ++r)
            for (int c = 0; c < 3; ++c) {
                const double a0 = s * tmp[r * 3], a1 = s * tmp[r * 3 + 1], a2 = s * tmp[r * 3 + 2];
                Ji[r * 3 + c] = a0 * R[c] + a1 * R[3 + c] + a2 * R[6 + c];
            }
    } else {
        for (int c = 0; c < 3; ++c) {
            Ji[0 * 3 + c] = -fx * R[0 * 3 + c] / z + fx * x * R[2 * 3 + c] / z_2;
            Ji[1 * 3 + c] = -fy * R[1 * 3 + c] / z + fy * y * R[2 * 3 + c] / z_2;
            Ji[2 * 3 + c] = Ji[0 * 3 + c] - bf * R[2 * 3 + c] / z_2;
        }
    }
    Jj[0] = x * y / z_2 * fx;
    Jj[1] = -(1 + (x * x / z_2)) * fx;
    Jj[2] = y / z * fx;
    Jj[3] = -1. / z * fx;
    Jj[4] = 0;
    Jj[5] = x / z_2 * fx;
    Jj[6] = (1 + y * y / z_2) * fy;
    Jj[7] = -x * y / z_2 * fy;
    Jj[8] = -x / z * fy;
    Jj[9] = 0;
    Jj[10] = -1. / z * fy;
    Jj[11] = y / z_2 * fy;
    if (stereo) {
        Jj[12] = Jj[0] - bf * y / z_2;
        Jj[13] = Jj[1] + bf * x / z_2;
        Jj[14] = Jj[2];
        Jj[15] = Jj[3];
        Jj[16] = 0;
        Jj[17] = Jj[5] - bf / z_2;
    }
}

// computeActiveErrors + the edge's part of buildSystem: everything the sums over edges read
__host__ __device__ inline void gba_linearise_edge(const GbaCam &cam, const double qt[7], const double X[3], const float *obs, int stereo, double w,
                                                   bool robust, double delta, double *lin)
{
    const int D = stereo ? 3 : 2;
    double er[3];
    gba_edge_error(cam, qt, X, obs, stereo, er);
    gba_edge_jacobians(cam, qt, X, stereo, lin + kGbaA, lin + kGbaB);
    const double *A = lin + kGbaA, *B = lin + kGbaB;
    double om[3] = {0, 0, 0}, wo = w, chi = edge_chi2(er, w, D);
    for (int i = 0; i < D; ++i) om[i] = -(w * er[i]);
    if (robust) {
        double rho[2];
        robustify(chi, delta, rho);
        wo = rho[1] * w;
        for (int i = 0; i < D; ++i) om[i] *= rho[1];
        chi = rho[0];
    }
    for (int i = 0; i < 3; ++i) lin[kGbaOr + i] = om[i];
    lin[kGbaWo] = wo;
    lin[kGbaChi] = chi;
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 3; ++c) {
            double t = 0;
            for (int d = 0; d < D; ++d) t += B[d * 6 + r] * wo * A[d * 3 + c];
            lin[kGbaHpl + r * 3 + c] = t;
        }
}

// what an edge adds to its pose: entry ent < 36 of Hpp (row-major 6x6), ent - 36 of b
__host__ __device__ inline double gba_pose_term(const double *lin, int D, int ent)
{
    const double *B = lin + kGbaB;
    double t = 0;
    if (ent < 36) {
        const int r = ent / 6, c = ent % 6;
        for (int d = 0; d < D; ++d) t += B[d * 6 + r] * lin[kGbaWo] * B[d * 6 + c];
    } else {
        const int r = ent - 36;
        for (int d = 0; d < D; ++d) t += B[d * 6 + r] * lin[kGbaOr + d];
    }
    return t;
}
// ... and to its landmark: entry ent < 9 of Hll, ent - 9 of b
__host__ __device__ inline double gba_point_term(const double *lin, int D, int ent)
{
    const double *A = lin + kGbaA;
    double t = 0;
    if (ent < 9) {
        const int r = ent / 3, c = ent % 3;
        for (int d = 0; d < D; ++d) t += A[d * 3 + r] * lin[kGbaWo] * A[d * 3 + c];
    } else {
        const int r = ent - 9;
        for (int d = 0; d < D; ++d) t += A[d * 3 + r] * lin[kGbaOr + d];
    }
    return t;
}

// a landmark of the Schur complement at lambda: Dinv = (Hll + lambda I)^-1 (Eigen's 3x3 inverse by cofactors), db = Dinv b_l
__host__ __device__ inline void gba_landmark(const double Hll[9], const double bl[3], double lambda, double Dinv[9], double db[3])
{
    double m[9];
    for (int i = 0; i < 9; ++i) m[i] = Hll[i];
    m[0] += lambda;
    m[4] += lambda;
    m[8] += lambda;
    mat3_inverse(m, Dinv);
    for (int r = 0; r < 3; ++r) db[r] = Dinv[r * 3] * bl[0] + Dinv[r * 3 + 1] * bl[1] + Dinv[r * 3 + 2] * bl[2];
}

// entry (r, c) of (Bi Dinv) Bj^T: what a pair of edges of one landmark (Hpl blocks Bi, Bj) subtracts from the block (pose of i, pose of j)
__host__ __device__ inline double gba_schur_term(const double *Bi, const double *Dinv, const double *Bj, int r, int c)
{
    const double q0 = Bi[r * 3] * Dinv[0] + Bi[r * 3 + 1] * Dinv[3] + Bi[r * 3 + 2] * Dinv[6];
    const double q1 = Bi[r * 3] * Dinv[1] + Bi[r * 3 + 1] * Dinv[4] + Bi[r * 3 + 2] * Dinv[7];
    const double q2 = Bi[r * 3] * Dinv[2] + Bi[r * 3 + 1] * Dinv[5] + Bi[r * 3 + 2] * Dinv[8];
    return q0 * Bj[c * 3] + q1 * Bj[c * 3 + 1] + q2 * Bj[c * 3 + 2];
}
// The lower-triangle blocks are kept, the solver reads the upper block triangle: entry (a, b) of the block (hi, lo) is entry (b, a) of
// the oracle's block (lo, hi), and a diagonal block is read through its upper triangle.  ea = the edge that comes first in its
// landmark's list (the lower pose index), diag = both edges belong to one pose.
__host__ __device__ inline double gba_block_term(const double *Ba, const double *Dinv, const double *Bb, bool diag, int a, int b)
{
    if (diag) return a <= b ? gba_schur_term(Ba, Dinv, Bb, a, b) : gba_schur_term(Ba, Dinv, Bb, b, a);
    return gba_schur_term(Ba, Dinv, Bb, b, a);
}
__host__ __device__ inline double gba_coeff_term(const double *Bi, const double *db, int r)
{
    return Bi[r * 3] * db[0] + Bi[r * 3 + 1] * db[1] + Bi[r * 3 + 2] * db[2];
}

// the control state of one optimize(iterations) call, kept on the device between the kernels
struct GbaControl {
    SoLm lm;
    double rho, chi2_initial;
    int32_t qmax;             // trials of the current iteration
    int32_t open;             // the current iteration still has a trial to run
    int32_t running;          // optimize() has not returned
    int32_t solved;           // the last factorisation had no zero or NaN pivot
    int32_t max_iterations, iterations, trials;
    int32_t polls, stop_poll, stop_at_poll;   // evaluations of terminate(), the one that first saw the flag, the test hook
    int32_t cur;              // which of the two sets of estimates holds the last accepted step
    int32_t pad;
};

__host__ __device__ inline void gba_control_init(GbaControl &c, int max_iterations, bool runs, int stop_at_poll)
{
    c.lm = SoLm();
    c.rho = c.chi2_initial = 0;
    c.qmax = c.open = c.solved = c.iterations = c.trials = c.polls = c.stop_poll = c.cur = c.pad = 0;
    c.running = runs;
    c.max_iterations = max_iterations;
    c.stop_at_poll = stop_at_poll;
}

// bool SparseOptimizer::terminate(): flag = what *pbStopFlag holds now
__host__ __device__ inline bool gba_poll(GbaControl &c, bool flag)
{
    c.polls++;
    if (c.stop_poll > 0) return true;
    if (flag || (c.stop_at_poll > 0 && c.polls >= c.stop_at_poll)) {
        c.stop_poll = c.polls;
        return true;
    }
    return false;
}

// the start of an LM iteration (levenberg.cpp:77-97): chi = activeRobustChi2 of the linearisation, max_diag over Hpp and Hll.  The
// head of optimize()'s loop before iteration 0 is evaluated here, the later ones where the iteration before ends.
__host__ __device__ inline void gba_iteration_begin(GbaControl &c, double chi, double max_diag, bool flag)
{
    if (c.iterations == 0) {
        if (gba_poll(c, flag)) {
            c.running = 0;
            return;
        }
        c.lm.lambda = 1e-5 * max_diag;
        c.lm.ni = 2;
        c.lm.nBad = 0;
        c.chi2_initial = chi;
    }
    c.lm.currentChi = c.lm.iniChi = chi;
    c.rho = 0;
    c.qmax = 0;
    c.open = 1;
}

// one trial (:107-161): true = accepted.  scale = sum of x_j (lambda x_j + b_j) over poses and landmarks, lambda as it was during
// the solve.  Closes the iteration (`while (rho < 0 && qmax < maxTrials && !terminate())`) and the call (:163-166 and
// `i < iterations && !terminate() && ok` of the next iteration).
__host__ __device__ inline bool gba_trial_decide(GbaControl &c, double tempChi, double scale, bool flag)
{
    const bool accepted = c.lm.decide_scaled(tempChi, c.solved != 0, scale, c.rho);
    c.qmax++;
    c.trials++;
    if (accepted) c.cur ^= 1;
    if (!(c.rho < 0 && c.qmax < 10 && !gba_poll(c, flag))) {
        c.open = 0;
        c.iterations++;
        const bool ok = c.lm.end(c.qmax, c.rho);
        if (c.iterations >= c.max_iterations || gba_poll(c, flag) || !ok) c.running = 0;
    }
    return accepted;
}

}  // namespace aos2
