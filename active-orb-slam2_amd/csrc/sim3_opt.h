// Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1047-1242) as arithmetic: the one definition that the device kernel
// (sim3_opt.hip) and the host tap (aos2_debug_sim3_opt_host) both run.  g2o pieces restated here:
//   Sim3(Vector7d), map, inverse, operator*        Thirdparty/g2o/g2o/types/sim3.h:70-146, 233-272
//   EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ types_seven_dof_expmap.h:130-171 (linearizeOplus is commented out there, so
//   the Jacobians are g2o's central differences, core/base_binary_edge.hpp:130-205, delta = 1e-9)
//   constructQuadraticForm + Huber                 core/base_binary_edge.hpp:55-120, robust_kernel_impl.cpp:78-91
//   the dense 7x7 solve                            solvers/linear_solver_dense.h:64-110 (Cholesky of H + lambda I)
//   Levenberg-Marquardt                            core/optimization_algorithm_levenberg.cpp:61-189
// The edges themselves (where they live, who sums) are the caller's: so_procedure / so_optimize take a backend B with
//   void   linearise(const Sim3d &S, bool fix_scale, double delta, double (&Hb)[kSoSum])   sums of so_edge_linearise over the active edges
//   double trial(const Sim3d &S, double delta)                                             sum of so_edge_trial over the active edges
//   int    reject(double th2, bool remove)                                                 the loops of :1187-1204 / :1221-1235
// quat_from_rot / quat_rotate are lba_math.h's; its robustify / edge_chi2 are __device__ only, so the two-row forms the host tap also
// runs (so_huber, so_chi2) are here.
// Edge 2c is e12 of correspondence c, edge 2c + 1 its e21 (insertion order, :1156, :1174).
#pragma once
#include "lba_math.h"

namespace aos2 {

constexpr int kSoSum = 36;   // 28 (H, upper triangle row by row) + 7 (b) + 1 (robust chi2)

struct Sim3d {   // g2o::Sim3: r (x, y, z, w), t, s
    double q[4], t[3], s;
};

// the arrays of aos2_sim3_opt_problem_t, wherever they live
struct SoArrays {
    int32_t n;
    const float *X1c, *X2c, *obs1, *obs2, *w1, *w2;
    double cam1[4], cam2[4];   // fx, fy, cx, cy
};

// one edge as the residual needs it: the fixed point, the measurement, the information and the camera of the image it projects into
struct SoEdge {
    double X[3], obs[2], w, fx, fy, cx, cy;
};

__host__ __device__ inline void so_load_edge(const SoArrays &A, int e, SoEdge &E)
{
    const size_t c = (size_t)(e >> 1);
    const bool inv = e & 1;   // e21: P3D1c through S12^-1 into image 2
    const float *X = (inv ? A.X1c : A.X2c) + 3 * c, *ob = (inv ? A.obs2 : A.obs1) + 2 * c;
    const double *cam = inv ? A.cam2 : A.cam1;
    for (int k = 0; k < 3; ++k) E.X[k] = (double)X[k];
    E.obs[0] = (double)ob[0];
    E.obs[1] = (double)ob[1];
    E.w = (double)(inv ? A.w2 : A.w1)[c];
    E.fx = cam[0]; E.fy = cam[1]; E.cx = cam[2]; E.cy = cam[3];
}

// Sim3(const Vector7d &update), sim3.h:70-142: the four (sigma, theta) branches at eps = 1e-5, r = Quaterniond(R) (not normalised)
__host__ __device__ inline void so_exp(const double u[7], Sim3d &S)
{
    const double *omega = u, *ups = u + 3, sigma = u[6];
    const double theta = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
    const double Om[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
    double Om2[9], R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Om2[i * 3 + j] = Om[i * 3] * Om[j] + Om[i * 3 + 1] * Om[3 + j] + Om[i * 3 + 2] * Om[6 + j];
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    const double eps = 0.00001;
    S.s = exp(sigma);
    double A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
            for (int i = 0; i < 9; ++i) R[i] = I[i] + Om[i] + Om2[i];
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
            const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
            for (int i = 0; i < 9; ++i) R[i] = I[i] + a * Om[i] + b * Om2[i];
        }
    } else {
        C = (S.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
            for (int i = 0; i < 9; ++i) R[i] = I[i] + Om[i] + Om2[i];
        } else {
            const double ra = sin(theta) / theta, rb = (1 - cos(theta)) / (theta * theta);
            for (int i = 0; i < 9; ++i) R[i] = I[i] + ra * Om[i] + rb * Om2[i];
            const double a = S.s * sin(theta), b = S.s * cos(theta);
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    quat_from_rot(R, S.q);
    for (int i = 0; i < 3; ++i) {
        double acc = 0;
        for (int j = 0; j < 3; ++j) acc += (A * Om[i * 3 + j] + B * Om2[i * 3 + j] + C * I[i * 3 + j]) * ups[j];
        S.t[i] = acc;
    }
}

// Sim3::map (sim3.h:144-146): s * (r * xyz) + t
__host__ __device__ inline void so_map(const Sim3d &S, const double X[3], double out[3])
{
    double r[3];
    quat_rotate(S.q, X, r);
    for (int i = 0; i < 3; ++i) out[i] = S.s * r[i] + S.t[i];
}

// Sim3::operator* (sim3.h:266-272): the quaternion product is not renormalised
__host__ __device__ inline void so_mul(const Sim3d &a, const Sim3d &b, Sim3d &o)
{
    const double *p = a.q, *q = b.q;
    double r[4], rt[3];
    r[3] = p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2];
    r[0] = p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1];
    r[1] = p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2];
    r[2] = p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0];
    quat_rotate(a.q, b.t, rt);
    for (int i = 0; i < 3; ++i) o.t[i] = a.s * rt[i] + a.t[i];
    for (int i = 0; i < 4; ++i) o.q[i] = r[i];
    o.s = a.s * b.s;
}

// Sim3::inverse (sim3.h:233-236)
__host__ __device__ inline void so_inverse(const Sim3d &S, Sim3d &o)
{
    const double c[4] = {-S.q[0], -S.q[1], -S.q[2], S.q[3]}, f = -1. / S.s;
    const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    double r[3];
    quat_rotate(c, v, r);
    for (int i = 0; i < 4; ++i) o.q[i] = c[i];
    for (int i = 0; i < 3; ++i) o.t[i] = r[i];
    o.s = 1. / S.s;
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): zeroes update[6] IN the caller's vector when the scale is fixed
__host__ __device__ inline void so_oplus(double u[7], bool fix_scale, const Sim3d &S, Sim3d &o)
{
    if (fix_scale) u[6] = 0;
    Sim3d E;
    so_exp(u, E);
    so_mul(E, S, o);
}

// The transforms of one linearisation, the same for every edge (base_binary_edge.hpp:181-197): k = 2 d (+delta e_d) and 2 d + 1
// (-delta e_d), d = 0..6; fwd = exp(+-delta e_d) S is what e12 maps with, inv = fwd^-1 what e21 maps with.
constexpr double kSoDelta = 1e-9;
__host__ __device__ inline void so_perturbed(const Sim3d &S, int k, bool fix_scale, Sim3d &fwd, Sim3d &inv)
{
    double add[7];
    for (int d = 0; d < 7; ++d) add[d] = d != (k >> 1) ? 0.0 : (k & 1) ? -kSoDelta : kSoDelta;
    so_oplus(add, fix_scale, S, fwd);
    so_inverse(fwd, inv);
}

// obs - cam_map(project(T.map(X))) (types_seven_dof_expmap.h:138-145, :160-167)
__host__ __device__ inline void so_residual(const Sim3d &T, const SoEdge &E, double er[2])
{
    double p[3];
    so_map(T, E.X, p);
    er[0] = E.obs[0] - (p[0] / p[2] * E.fx + E.cx);
    er[1] = E.obs[1] - (p[1] / p[2] * E.fy + E.cy);
}

__host__ __device__ inline double so_chi2(const double er[2], double w) { return er[0] * (w * er[0]) + er[1] * (w * er[1]); }

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho[0], rho[1]
__host__ __device__ inline void so_huber(double e, double delta, double &rho0, double &rho1)
{
    const double dsqr = delta * delta;
    if (e <= dsqr) {
        rho0 = e;
        rho1 = 1.;
    } else {
        const double sqrte = sqrt(e);
        rho0 = 2 * sqrte * delta - dsqr;
        rho1 = delta / sqrte;
    }
}

// computeError + the edge's term of activeRobustChi2 at the transform T (S12 for an e12, its inverse for an e21): one projection.
// chi2 = what e->chi2() returns until the next computeError.
__host__ __device__ inline double so_edge_trial(const Sim3d &T, const SoEdge &E, double delta, double &chi2)
{
    double er[2], rho0, rho1;
    so_residual(T, E, er);
    chi2 = so_chi2(er, E.w);
    so_huber(chi2, delta, rho0, rho1);
    return rho0;
}

// computeError, linearizeOplus and constructQuadraticForm of one edge: 15 projections.  T0 = the unperturbed transform of the edge's
// kind, pert[stride * k] = the perturbed one for k = 0..13.  J.col(d) = scalar * (e(+) - e(-)), scalar = 1 / (2 delta), as g2o forms
// it; the stored residual is the unperturbed one (:200).  acc += (H, b, rho[0]).
__host__ __device__ inline void so_edge_linearise(const Sim3d &T0, const Sim3d *pert, int stride, const SoEdge &E, double delta, double (&acc)[kSoSum],
                                                  double &chi2)
{
    const double scalar = 1.0 / (2 * kSoDelta);
    double er[2], J[2][7], rho0, rho1;
    so_residual(T0, E, er);
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        so_residual(pert[stride * (2 * d)], E, ep);
        so_residual(pert[stride * (2 * d + 1)], E, em);
        J[0][d] = scalar * (ep[0] - em[0]);
        J[1][d] = scalar * (ep[1] - em[1]);
    }
    chi2 = so_chi2(er, E.w);
    so_huber(chi2, delta, rho0, rho1);
    acc[35] += rho0;
    const double wo = rho1 * E.w;                                   // robustInformation: rho[1] * Omega
    const double r0 = -(E.w * er[0]) * rho1, r1 = -(E.w * er[1]) * rho1;   // omega_r = -Omega e, *= rho[1]
    int m = 0;
    for (int r = 0; r < 7; ++r) {
        acc[28 + r] += J[0][r] * r0 + J[1][r] * r1;
        const double a0 = J[0][r] * wo, a1 = J[1][r] * wo;
        for (int c = r; c < 7; ++c, ++m) acc[m] += a0 * J[0][c] + a1 * J[1][c];
    }
}

// (H + lambda I) x = b for the 7x7 system, Hb = 28 (upper triangle row by row) + 7 (b): LinearSolverDense's Cholesky in the
// square-root-free form L D L^T (the pivots are the squares of Cholesky's diagonal: the same positivity test), right-looking,
// in registers, shaped like solve6 of pose_opt.h.  false = "not positive definite"; x keeps its values then.
__host__ __device__ inline bool so_solve7(const double *Hb, double lambda, double (&x)[7])
{
    double a[7][7], rd[7];
    {
        int k = 0;
        for (int r = 0; r < 7; ++r)
            for (int c = r; c < 7; ++c, ++k) a[c][r] = Hb[k];
    }
    for (int d = 0; d < 7; ++d) a[d][d] += lambda;
    bool pos = true;
    for (int j = 0; j < 7; ++j) {
        const double d = a[j][j];
        if (!(d > 0)) pos = false;
        rd[j] = 1.0 / d;
        double l[7];
        for (int r = j + 1; r < 7; ++r) l[r] = a[r][j] * rd[j];
        for (int r = j + 1; r < 7; ++r)
            for (int c = j + 1; c <= r; ++c) a[r][c] -= l[r] * a[c][j];
        for (int r = j + 1; r < 7; ++r) a[r][j] = l[r];
    }
    double y[7], xv[7];
    for (int r = 0; r < 7; ++r) {
        double s = Hb[28 + r];
        for (int m = 0; m < r; ++m) s -= a[r][m] * y[m];
        y[r] = s;
    }
    for (int r = 6; r >= 0; --r) {
        double s = y[r] * rd[r];
        for (int m = r + 1; m < 7; ++m) s -= a[m][r] * xv[m];
        xv[r] = s;
    }
    if (pos)
        for (int r = 0; r < 7; ++r) x[r] = xv[r];
    return pos;
}

// the Levenberg-Marquardt state of one optimize() call and its two decisions (levenberg.cpp:93-97, :129-161)
struct SoLm {
    double lambda = 0, ni = 2, currentChi = 0, iniChi = 0;
    int nBad = 0;

    __host__ __device__ void begin(int iteration, const double *Hb)
    {
        currentChi = iniChi = Hb[35];
        if (iteration == 0) {   // computeLambdaInit: tau * max |H_jj|
            double maxDiagonal = 0.;
            for (int j = 0, k = 0; j < 7; k += 7 - j, ++j) maxDiagonal = fmax(fabs(Hb[k]), maxDiagonal);
            lambda = 1e-5 * maxDiagonal;
            ni = 2;
            nBad = 0;
        }
    }
    // one trial: true = accepted (the estimate stays), false = pop.  rho is the caller's loop condition.
    __host__ __device__ bool decide(double tempChi, bool solved, const double *x, const double *Hb, double &rho)
    {
        double scale = 0.;
        for (int j = 0; j < 7; ++j) scale += x[j] * (lambda * x[j] + Hb[28 + j]);
        return decide_scaled(tempChi, solved, scale, rho);
    }
    // the same decision for a system of any size: scale = the sum of x_j (lambda x_j + b_j) over all of it (essential_graph.h)
    __host__ __device__ bool decide_scaled(double tempChi, bool solved, double scale, double &rho)
    {
        if (!solved) tempChi = 1.7976931348623157e308;
        rho = currentChi - tempChi;
        scale += 1e-3;
        rho /= scale;
        if (rho > 0 && fabs(tempChi) <= 1.7976931348623157e308) {   // g2o_isfinite (false for NaN too)
            const double t = 2 * rho - 1;
            double alpha = 1. - t * t * t;
            alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
            const double scaleFactor = 1. / 3. > alpha ? 1. / 3. : alpha;
            lambda *= scaleFactor;
            ni = 2;
            currentChi = tempChi;
            return true;
        }
        lambda *= ni;
        ni *= 2;
        return false;
    }
    // after the trials of an iteration: true = OK, false = Terminate
    __host__ __device__ bool end(int qmax, double rho)
    {
        if (qmax == 10 || rho == 0) return false;
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++;
        else nBad = 0;
        return nBad < 3;
    }
};

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg on the one free vertex.  x is the solver's vector: it
// outlives a failed solve (the update then applies the previous one, and the trial is rejected).
template <class B>
__host__ __device__ inline void so_optimize(B &edges, Sim3d &S, int iterations, bool fix_scale, double delta, double (&x)[7], int32_t &n_iterations,
                                            int32_t &n_trials)
{
    SoLm lm;
    bool ok = true;
    for (int i = 0; i < iterations && ok; ++i) {
        double Hb[kSoSum];
        edges.linearise(S, fix_scale, delta, Hb);   // computeActiveErrors, activeRobustChi2, buildSystem
        lm.begin(i, Hb);
        double rho = 0;
        int qmax = 0;
        do {
            const Sim3d backup = S;                   // push
            const bool solved = so_solve7(Hb, lm.lambda, x);
            so_oplus(x, fix_scale, backup, S);
            const double tempChi = edges.trial(S, delta);
            if (!lm.decide(tempChi, solved, x, Hb, rho)) S = backup;   // pop
            qmax++;
            n_trials++;
        } while (rho < 0 && qmax < 10);
        n_iterations++;
        ok = lm.end(qmax, rho);
    }
}

struct SoOutcome {
    Sim3d S;                 // g2oS12 as the caller has to leave it
    int32_t n_bad, n_inliers, wrote;   // wrote = 0: the return through :1212, S is the input
    int32_t iterations[2], trials[2];
};

// src/Optimizer.cc:1181-1241 for n >= 1 correspondences
template <class B>
__host__ __device__ inline void so_procedure(B &edges, const Sim3d &S_in, int n, double th2, double delta, bool fix_scale, SoOutcome &o)
{
    Sim3d S = S_in;
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    o.iterations[0] = o.iterations[1] = o.trials[0] = o.trials[1] = 0;
    int nBad = 0;
    // (one call site of so_optimize: the two optimisations are two turns of a loop that is kept a loop, which halves the kernel's code)
#pragma nounroll
    for (int pass = 0; pass < 2; ++pass) {
        int32_t iterations = 0, trials = 0;
        so_optimize(edges, S, pass == 0 ? 5 : nBad > 0 ? 10 : 5, fix_scale, delta, x, iterations, trials);
        const int flagged = edges.reject(th2, pass == 0);
        if (pass == 0) {
            o.iterations[0] = iterations;
            o.trials[0] = trials;
            o.n_bad = nBad = flagged;
            if (n - nBad < 10) {   // :1212: before g2oS12 is written; the matches erased above stay erased
                o.S = S_in;
                o.n_inliers = 0;
                o.wrote = 0;
                return;
            }
        } else {
            o.iterations[1] = iterations;
            o.trials[1] = trials;
            o.S = S;
            o.n_inliers = n - nBad - flagged;
            o.wrote = 1;
        }
    }
}

}  // namespace aos2
