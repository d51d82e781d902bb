// Optimizer::OptimizeEssentialGraph (reference src/Optimizer.cc:782-1045) as arithmetic: the one definition that the device kernels
// (essential_graph.hip) and the host tap (aos2_debug_essential_graph_host) both run.  Sim3(Vector7d), operator*, inverse, map, oplus and
// the Levenberg-Marquardt decisions are sim3_opt.h's; new here, restated from g2o:
//   Sim3::log                                      Thirdparty/g2o/g2o/types/sim3.h:148-230 (W.lu().solve(t): PartialPivLU of a 3x3)
//   EdgeSim3::computeError                         types_seven_dof_expmap.h:106-114: log(C * S_v0 * S_v1^-1), information = I, no kernel
//   the Jacobians                                  linearizeOplus is not overridden: central differences, core/base_binary_edge.hpp:130-205
//   constructQuadraticForm                         core/base_binary_edge.hpp:55-120
//   Levenberg-Marquardt with setUserLambdaInit     core/optimization_algorithm_levenberg.cpp:61-189
// The conventions are DESIGN.md section 2 item 14.
#pragma once
#include "sim3_opt.h"

namespace aos2 {

// x of A x = t for a 3x3 (row-major) by Eigen's PartialPivLU: the pivot of column k is the entry of largest magnitude in rows k..2,
// the first one on ties; a zero pivot column is left as it is (the division then gives what Eigen's gives)
__host__ __device__ inline void eg_lu3_solve(const double A[9], const double t[3], double x[3])
{
    double a[3][3], b[3] = {t[0], t[1], t[2]};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) a[i][j] = A[i * 3 + j];
    for (int k = 0; k < 3; ++k) {
        int p = k;
        double best = fabs(a[k][k]);
        for (int i = k + 1; i < 3; ++i)
            if (fabs(a[i][k]) > best) {
                best = fabs(a[i][k]);
                p = i;
            }
        if (p != k) {
            for (int j = 0; j < 3; ++j) {
                const double s = a[k][j];
                a[k][j] = a[p][j];
                a[p][j] = s;
            }
            const double s = b[k];
            b[k] = b[p];
            b[p] = s;
        }
        if (best != 0)
            for (int i = k + 1; i < 3; ++i) a[i][k] /= a[k][k];
        for (int i = k + 1; i < 3; ++i)
            for (int j = k + 1; j < 3; ++j) a[i][j] -= a[i][k] * a[k][j];
    }
    b[1] -= a[1][0] * b[0];
    b[2] -= a[2][0] * b[0];
    b[2] -= a[2][1] * b[1];
    x[2] = b[2] / a[2][2];
    x[1] = (b[1] - a[1][2] * x[2]) / a[1][1];
    x[0] = (b[0] - a[0][1] * x[1] - a[0][2] * x[2]) / a[0][0];
}

// Sim3::log (sim3.h:148-230): the four (sigma, d) branches at eps = 1e-5, d = 0.5 (tr R - 1) of r.toRotationMatrix()
__host__ __device__ inline void eg_log(const Sim3d &S, double res[7])
{
    const double sigma = log(S.s);
    double R[9];
    rot_from_quat(S.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR
    const double eps = 0.00001;
    double omega[3], A, B, C;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            for (int i = 0; i < 3; ++i) omega[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta, f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; ++i) omega[i] = f * dR[i];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            for (int i = 0; i < 3; ++i) omega[i] = 0.5 * dR[i];
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d), f = theta / (2 * sqrt(1 - d * d));
            for (int i = 0; i < 3; ++i) omega[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const double Om[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
    double W[9];   // A * Omega + B * Omega * Omega + C * I, the product taken as (B * Omega) * Omega
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double bo2 = (B * Om[i * 3]) * Om[j] + (B * Om[i * 3 + 1]) * Om[3 + j] + (B * Om[i * 3 + 2]) * Om[6 + j];
            W[i * 3 + j] = A * Om[i * 3 + j] + bo2 + (i == j ? C : 0.0);
        }
    eg_lu3_solve(W, S.t, res + 3);
    for (int i = 0; i < 3; ++i) res[i] = omega[i];
    res[6] = sigma;
}

// EdgeSim3::computeError: A = the estimate of vertex 0, Binv = the inverse of the estimate of vertex 1
__host__ __device__ inline void eg_residual(const Sim3d &C, const Sim3d &A, const Sim3d &Binv, double e[7])
{
    Sim3d CA, T;
    so_mul(C, A, CA);
    so_mul(CA, Binv, T);
    eg_log(T, e);
}

__host__ __device__ inline double eg_chi2(const double e[7])   // information = identity
{
    double c = e[0] * e[0];
    for (int r = 1; r < 7; ++r) c += e[r] * e[r];
    return c;
}

// The transforms of one linearisation that belong to a vertex, not to an edge: kEgPert Sim3 per vertex,
//   [0] the inverse of the estimate, [1 + 2 k] the estimate after oplus(+-delta e_d) (k = 2 d, 2 d + 1 as so_perturbed), [2 + 2 k] its inverse
constexpr int kEgPert = 29;

// column d of the Jacobian of side `side` (0: vertex 0 is perturbed, 1: vertex 1) into J[r * 7 + d]: scalar * (e(+) - e(-))
__host__ __device__ inline void eg_jacobian_column(const Sim3d &C, const Sim3d &S0, const Sim3d *pert0, const Sim3d *pert1, int side, int d, double *J)
{
    const double scalar = 1.0 / (2 * kSoDelta);
    double ep[7], em[7];
    if (side == 0) {
        eg_residual(C, pert0[1 + 4 * d], pert1[0], ep);
        eg_residual(C, pert0[3 + 4 * d], pert1[0], em);
    } else {
        eg_residual(C, S0, pert1[2 + 4 * d], ep);
        eg_residual(C, S0, pert1[4 + 4 * d], em);
    }
    for (int r = 0; r < 7; ++r) J[r * 7 + d] = scalar * (ep[r] - em[r]);
}

// entry (a, b) of JA^T JB, the rows taken in order
__host__ __device__ inline double eg_jtj(const double *JA, const double *JB, int a, int b)
{
    double s = JA[a] * JB[b];
    for (int r = 1; r < 7; ++r) s += JA[r * 7 + a] * JB[r * 7 + b];
    return s;
}
// component a of J^T e
__host__ __device__ inline double eg_jte(const double *J, const double *e, int a)
{
    double s = J[a] * e[0];
    for (int r = 1; r < 7; ++r) s += J[r * 7 + a] * e[r];
    return s;
}
// What an edge adds to a block of H (the blocks of the lower triangle are kept: block (hi, lo) = J_hi^T J_lo, the transpose of g2o's
// J_low^T J_high).  kind 0: J0^T J0, 1: J1^T J1, 2: J0^T J1 (vertex 0 has the higher index), 3: J1^T J0.  J = the edge's two Jacobians.
__host__ __device__ inline double eg_block_term(const double *J, int kind, int a, int b)
{
    const double *J0 = J, *J1 = J + 49;
    return kind == 0 ? eg_jtj(J0, J0, a, b) : kind == 1 ? eg_jtj(J1, J1, a, b) : kind == 2 ? eg_jtj(J0, J1, a, b) : eg_jtj(J1, J0, a, b);
}

// the control state of one optimize(iterations) call: where the decisions of sim3_opt.h's SoLm are kept between the kernels
struct EgControl {
    SoLm lm;
    double rho, chi2_initial;
    int32_t qmax;             // trials of the current iteration
    int32_t open;             // the current iteration still has a trial to run
    int32_t running;          // optimize() has not returned
    int32_t solved;           // the last factorisation had no zero or NaN pivot
    int32_t max_iterations, iterations, trials, rejected, accepted_first, pad;
};

__host__ __device__ inline void eg_control_init(EgControl &c, int max_iterations, bool runs)
{
    c.lm = SoLm();
    c.rho = c.chi2_initial = 0;
    c.qmax = c.open = c.solved = c.iterations = c.trials = c.rejected = c.accepted_first = c.pad = 0;
    c.running = runs;
    c.max_iterations = max_iterations;
}

// the start of an LM iteration (levenberg.cpp:77-97 with _userLambdaInit = 1e-16): chi = activeRobustChi2 of the linearisation
__host__ __device__ inline void eg_iteration_begin(EgControl &c, double chi)
{
    c.lm.currentChi = c.lm.iniChi = chi;
    if (c.iterations == 0) {
        c.lm.lambda = 1e-16;
        c.lm.ni = 2;
        c.lm.nBad = 0;
        c.chi2_initial = chi;
    }
    c.rho = 0;
    c.qmax = 0;
    c.open = 1;
}

// one trial (:107-161): true = accepted, false = the estimates go back.  scale = sum of x_j (lambda x_j + b_j), lambda as it was
// during the solve.  Closes the iteration (the do-while's condition) and the call (:163-166, optimize()'s loop).
__host__ __device__ inline bool eg_trial_decide(EgControl &c, double tempChi, double scale)
{
    const bool accepted = c.lm.decide_scaled(tempChi, c.solved != 0, scale, c.rho);
    c.qmax++;
    c.trials++;
    if (!accepted) c.rejected++;
    else if (c.iterations == 0) c.accepted_first++;
    if (!(c.rho < 0 && c.qmax < 10)) {
        c.open = 0;
        c.iterations++;
        if (!c.lm.end(c.qmax, c.rho) || c.iterations >= c.max_iterations) c.running = 0;
    }
    return accepted;
}

// :1002-1008: R(q), t * (1. / s) as the float 4x4
__host__ __device__ inline void eg_pose(const Sim3d &S, float *T)
{
    double R[9];
    rot_from_quat(S.q, R);
    const double f = 1. / S.s;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) T[i * 4 + j] = (float)R[i * 3 + j];
        T[i * 4 + 3] = (float)(S.t[i] * f);
    }
    T[12] = T[13] = T[14] = 0.f;
    T[15] = 1.f;
}

// :1033-1040: correctedSwr.map(Srw.map(P)) in double, rounded to float once
__host__ __device__ inline void eg_point(const Sim3d &Srw, const Sim3d &corrected_Srw, const float *P, float *out)
{
    Sim3d Swr;
    so_inverse(corrected_Srw, Swr);
    const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
    double c[3], w[3];
    so_map(Srw, X, c);
    so_map(Swr, c, w);
    for (int i = 0; i < 3; ++i) out[i] = (float)w[i];
}

}  // namespace aos2
