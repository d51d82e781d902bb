// The arithmetic of PnPsolver (src/PnPsolver.cc): the index removal of iterate (:188-201), compute_pose (:477-525, EPnP: control
// points, barycentric coordinates, M'M, the null space, three beta approximations, Gauss-Newton, R and t), CheckInliers (:308-339)
// and the loop of iterate (:182-239) over inlier counts and memoised Refine() results.  ONE routine set for the device kernels
// (csrc/pnp_ransac.hip) and the host tap (aos2_debug_pnp_host): the translation units are built with -ffp-contract=off, so both run
// the same operation sequence.  Everything is double in index order; there is no libm call but sqrt.  The OpenCV routines the
// reference calls (cvSVD, cvSolve / cvInvert with CV_SVD, cvMulTransposed) are restated as DESIGN.md section 2 item 11.
//
// A correspondence set is never copied: a set is something with each(f) that calls f(i) for its members in order -- the minimal set
// through pnp_set_index, the set Refine() works on through a flag array -- and every per-point quantity (alphas, the rows of M, pcs)
// is a pure function of the point and a few doubles, recomputed where it is read.  The 12x12 work (M'M, the rotations, W) lives in a
// workspace type: plain arrays on the host, LDS laid out [element][lane] on the device.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/aos2.h"

namespace aos2 {

struct PnpCam {
    double fu, fv, uc, vc;   // (float F.fx ... widened, :104-107)
};

struct PnpPts {
    const float *P3D, *P2D, *max_err;   // mvP3Dw [n][3], mvP2D [n][2], mvMaxError [n]
};

// the index that draw k of an iteration selects (:193-200): vAvailableIndices starts as 0..n-1, a drawn position takes the value of
// the back, which is popped.  The value at position p after the removals of draws 0..k-1, followed backwards: the removal of draw t
// wrote the then-back n-1-t to position row[t].  No list is kept.
__host__ __device__ inline int pnp_set_index(int n, const int32_t *row, int k)
{
    int p = row[k];
    for (int t = k - 1; t >= 0; --t)
        if (p == row[t]) p = n - 1 - t;
    return p;
}

struct PnpSetDraws {   // the minimal set of an iteration
    int n, cnt;
    const int32_t *row;
    template <class F>
    __host__ __device__ void each(F &&f) const
    {
        for (int k = 0; k < cnt; ++k) f(pnp_set_index(n, row, k));
    }
};

struct PnpSetFlags {   // the set Refine() works on (:262-281)
    int n;
    const uint8_t *flags;
    template <class F>
    __host__ __device__ void each(F &&f) const
    {
        for (int i = 0; i < n; ++i)
            if (flags[i]) f(i);
    }
};

// ---- the one-sided Jacobi SVD on a workspace: At (N rows of M), V (N x N), W (N)
template <int N, int M>
struct PnpLocal {
    double at[N][M], v[N][N], w[N];
    __host__ __device__ double &At(int i, int k) { return at[i][k]; }
    __host__ __device__ double &V(int i, int k) { return v[i][k]; }
    __host__ __device__ double &W(int i) { return w[i]; }
};

// SMALL: every loop unrolled, so that a PnpLocal is indexed with constants only and stays in registers on the device
template <int N, int M, bool SMALL, class Ws>
__host__ __device__ inline void pnp_jacobi(Ws &ws)
{
    constexpr int UN = SMALL ? 64 : 1;
    const double eps = 10 * DBL_EPSILON;
#pragma unroll UN
    for (int i = 0; i < N; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const double t = ws.At(i, k);
            sd += t * t;
        }
        ws.W(i) = sd;
#pragma unroll
        for (int k = 0; k < N; ++k) ws.V(i, k) = i == k ? 1.0 : 0.0;
    }
    for (int sweep = 0; sweep < 30; ++sweep) {
        bool changed = false;
#pragma unroll UN
        for (int i = 0; i < N - 1; ++i)
#pragma unroll UN
            for (int j = i + 1; j < N; ++j) {
                double a = ws.W(i), b = ws.W(j), p = 0;
#pragma unroll
                for (int k = 0; k < M; ++k) p += ws.At(i, k) * ws.At(j, k);
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
#pragma unroll
                for (int k = 0; k < M; ++k) {
                    const double x = ws.At(i, k), y = ws.At(j, k);
                    const double t0 = c * x + s * y, t1 = -s * x + c * y;
                    ws.At(i, k) = t0;
                    ws.At(j, k) = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                ws.W(i) = a;
                ws.W(j) = b;
                changed = true;
#pragma unroll
                for (int k = 0; k < N; ++k) {
                    const double x = ws.V(i, k), y = ws.V(j, k);
                    ws.V(i, k) = c * x + s * y;
                    ws.V(j, k) = -s * x + c * y;
                }
            }
        if (!changed) break;
    }
#pragma unroll UN
    for (int i = 0; i < N; ++i) {
        double sd = 0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const double t = ws.At(i, k);
            sd += t * t;
        }
        ws.W(i) = sqrt(sd);
    }
    // selection sort into descending W, strict test; the swap partner is matched by comparison, never used as an index
#pragma unroll UN
    for (int i = 0; i < N - 1; ++i) {
        int j = i;
        double wj = ws.W(i);
#pragma unroll UN
        for (int k = i + 1; k < N; ++k) {
            const double wk = ws.W(k);
            if (wj < wk) wj = wk, j = k;
        }
#pragma unroll UN
        for (int k = i + 1; k < N; ++k)
            if (k == j) {
                const double w0 = ws.W(i);
                ws.W(i) = ws.W(k);
                ws.W(k) = w0;
#pragma unroll
                for (int q = 0; q < M; ++q) {
                    const double t = ws.At(i, q);
                    ws.At(i, q) = ws.At(k, q);
                    ws.At(k, q) = t;
                }
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    const double t = ws.V(i, q);
                    ws.V(i, q) = ws.V(k, q);
                    ws.V(k, q) = t;
                }
            }
    }
}

// the rows of At scaled to the left singular vectors: u_i = At[i] * (1 / W[i]) (a vanished W gives infinities and NaNs that flow on)
template <int N, int M, class Ws>
__host__ __device__ inline void pnp_svd_normalise(Ws &ws)
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double s = 1 / ws.W(i);
#pragma unroll
        for (int k = 0; k < M; ++k) ws.At(i, k) *= s;
    }
}

// cvSolve(A, b, x, CV_SVD) for the M x N matrix A (M >= N) whose transpose is ws.At: x = sum_i v_i * ((u_i . b) * (1 / w_i)) over the
// singular values above 2 * DBL_EPSILON * sum(w), i and every inner sum in index order
template <int N, int M>
__host__ __device__ inline void pnp_svd_solve(PnpLocal<N, M> &ws, const double b[M], double x[N], bool decompose = true)
{
    if (decompose) {
        pnp_jacobi<N, M, true>(ws);
        pnp_svd_normalise<N, M>(ws);
    }
    double thr = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) thr += ws.W(i);
    thr *= 2 * DBL_EPSILON;
#pragma unroll
    for (int j = 0; j < N; ++j) x[j] = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double wi = ws.W(i);
        if (fabs(wi) <= thr) continue;
        wi = 1 / wi;
        double s = 0;
#pragma unroll
        for (int k = 0; k < M; ++k) s += ws.At(i, k) * b[k];
        s *= wi;
#pragma unroll
        for (int j = 0; j < N; ++j) x[j] += s * ws.V(i, j);
    }
}

// ---- EPnP
struct PnpGeo {
    double cws[4][3];   // the control points (choose_control_points, :375-409)
    double ci[9];       // cc_inv (compute_barycentric_coordinates, :413-421)
};

// the alphas of one point (:423-433)
__host__ __device__ inline void pnp_alphas(const PnpGeo &G, const float *pw, double a[4])
{
    const double d0 = (double)pw[0] - G.cws[0][0], d1 = (double)pw[1] - G.cws[0][1], d2 = (double)pw[2] - G.cws[0][2];
#pragma unroll
    for (int j = 0; j < 3; ++j) a[1 + j] = G.ci[3 * j] * d0 + G.ci[3 * j + 1] * d1 + G.ci[3 * j + 2] * d2;
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// one element of M (fill_M, :436-451): row 2*point + par, column col
__host__ __device__ inline double pnp_M_elem(int par, int col, const double a[4], double u, double v, const PnpCam &K)
{
    const int j = col / 3, k = col - 3 * j;
    const double aj = j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
    if (k == 0) return par == 0 ? aj * K.fu : 0.0;
    if (k == 1) return par == 0 ? 0.0 : aj * K.fv;
    return par == 0 ? aj * (K.uc - u) : aj * (K.vc - v);
}

// choose_control_points and cc_inv
template <class Set>
__host__ __device__ inline void pnp_geometry(const Set &S, const PnpPts &pts, PnpGeo &G)
{
    int cnt = 0;
    double c0[3] = {0, 0, 0};
    S.each([&](int i) {
        const float *pw = pts.P3D + 3 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 3; ++j) c0[j] += (double)pw[j];
        ++cnt;
    });
#pragma unroll
    for (int j = 0; j < 3; ++j) G.cws[0][j] = c0[j] / cnt;
    // PW0' PW0 (cvMulTransposed, order 1): every entry a sum over the points in order
    PnpLocal<3, 3> ws;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) ws.at[r][c] = 0;
    S.each([&](int i) {
        const float *pw = pts.P3D + 3 * (size_t)i;
        const double d[3] = {(double)pw[0] - G.cws[0][0], (double)pw[1] - G.cws[0][1], (double)pw[2] - G.cws[0][2]};
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) ws.at[r][c] += d[r] * d[c];
    });
    pnp_jacobi<3, 3, true>(ws);   // dc = W, the rows of UCt = the accumulated rotations
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const double k = sqrt(ws.w[i - 1] / cnt);
#pragma unroll
        for (int j = 0; j < 3; ++j) G.cws[i][j] = G.cws[0][j] + k * ws.v[i - 1][j];
    }
    // cvInvert(CC, CC_inv, CV_SVD): the pseudo-inverse applied to the columns of the identity
    PnpLocal<3, 3> cc;   // At = CC': At[j-1][i] = cc[3*i + j-1]
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 1; j < 4; ++j) cc.at[j - 1][i] = G.cws[j][i] - G.cws[0][i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double e[3] = {c == 0 ? 1.0 : 0.0, c == 1 ? 1.0 : 0.0, c == 2 ? 1.0 : 0.0};
        double x[3];
        pnp_svd_solve<3, 3>(cc, e, x, c == 0);
#pragma unroll
        for (int r = 0; r < 3; ++r) G.ci[3 * r + c] = x[r];
    }
}

// M'M (cvMulTransposed of the 2n x 12 M) into ws.At: every entry a sum over the rows of M in order
template <class Set, class Ws>
__host__ __device__ inline void pnp_mtm(const Set &S, const PnpPts &pts, const PnpCam &K, const PnpGeo &G, Ws &ws)
{
    for (int r = 0; r < 12; ++r)
#pragma unroll
        for (int c = 0; c < 12; ++c) ws.At(r, c) = 0;
    S.each([&](int i) {
        double a[4];
        pnp_alphas(G, pts.P3D + 3 * (size_t)i, a);
        const double u = pts.P2D[2 * (size_t)i], v = pts.P2D[2 * (size_t)i + 1];
#pragma unroll
        for (int par = 0; par < 2; ++par) {
            double m[12];
#pragma unroll
            for (int c = 0; c < 12; ++c) m[c] = pnp_M_elem(par, c, a, u, v, K);
#pragma unroll
            for (int r = 0; r < 12; ++r)
#pragma unroll
                for (int c = 0; c < 12; ++c) ws.At(r, c) += m[r] * m[c];
        }
    });
}

// the same sum for ONE entry (the refine kernel gives every entry a thread of its own)
template <class Set>
__host__ __device__ inline double pnp_mtm_entry(const Set &S, const PnpPts &pts, const PnpCam &K, const PnpGeo &G, int r, int c)
{
    double acc = 0;
    S.each([&](int i) {
        double a[4];
        pnp_alphas(G, pts.P3D + 3 * (size_t)i, a);
        const double u = pts.P2D[2 * (size_t)i], v = pts.P2D[2 * (size_t)i + 1];
        acc += pnp_M_elem(0, r, a, u, v, K) * pnp_M_elem(0, c, a, u, v, K);
        acc += pnp_M_elem(1, r, a, u, v, K) * pnp_M_elem(1, c, a, u, v, K);
    });
    return acc;
}

__host__ __device__ inline double pnp_dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__host__ __device__ inline double pnp_dist2(const double *p, const double *q)
{
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2]);
}

// qr_solve (:860-950) of the 6x4 system; false: a singular column, x is left as it was
__host__ __device__ inline bool pnp_qr_solve(double A[6][4], double b[6], double x[4])
{
    double A1[4], A2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double eta = fabs(A[k][k]);
#pragma unroll
        for (int i = k + 1; i < 6; ++i) {
            const double elt = fabs(A[i - 1][k]);   // (the reference's walk starts at row k again: it reads rows k .. 4)
            if (eta < elt) eta = elt;
        }
        if (eta == 0) return false;
        const double inv_eta = 1. / eta;
        double sum = 0;
#pragma unroll
        for (int i = k; i < 6; ++i) {
            A[i][k] *= inv_eta;
            sum += A[i][k] * A[i][k];
        }
        double sigma = sqrt(sum);
        if (A[k][k] < 0) sigma = -sigma;
        A[k][k] += sigma;
        A1[k] = sigma * A[k][k];
        A2[k] = -eta * sigma;
#pragma unroll
        for (int j = k + 1; j < 4; ++j) {
            double s = 0;
#pragma unroll
            for (int i = k; i < 6; ++i) s += A[i][k] * A[i][j];
            const double tau = s / A1[k];
#pragma unroll
            for (int i = k; i < 6; ++i) A[i][j] -= tau * A[i][k];
        }
    }
    // b <- Q' b
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        double tau = 0;
#pragma unroll
        for (int i = j; i < 6; ++i) tau += A[i][j] * b[i];
        tau /= A1[j];
#pragma unroll
        for (int i = j; i < 6; ++i) b[i] -= tau * A[i][j];
    }
    // x = R^-1 b
    x[3] = b[3] / A2[3];
#pragma unroll
    for (int i = 2; i >= 0; --i) {
        double sum = 0;
#pragma unroll
        for (int j = i + 1; j < 4; ++j) sum += A[i][j] * x[j];
        x[i] = (b[i] - sum) / A2[i];
    }
    return true;
}

// gauss_newton (:812-858): five steps; L is read through the workspace (rows 0..5, columns 0..9 of At)
template <class Ws>
__host__ __device__ inline void pnp_gauss_newton(Ws &ws, const double rho[6], double betas[4])
{
    double x[4] = {0, 0, 0, 0};
    for (int step = 0; step < 5; ++step) {
        double A[6][4], b[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double L[10];
#pragma unroll
            for (int c = 0; c < 10; ++c) L[c] = ws.At(i, c);
            A[i][0] = 2 * L[0] * betas[0] + L[1] * betas[1] + L[3] * betas[2] + L[6] * betas[3];
            A[i][1] = L[1] * betas[0] + 2 * L[2] * betas[1] + L[4] * betas[2] + L[7] * betas[3];
            A[i][2] = L[3] * betas[0] + L[4] * betas[1] + 2 * L[5] * betas[2] + L[8] * betas[3];
            A[i][3] = L[6] * betas[0] + L[7] * betas[1] + L[8] * betas[2] + 2 * L[9] * betas[3];
            b[i] = rho[i] - (L[0] * betas[0] * betas[0] + L[1] * betas[0] * betas[1] + L[2] * betas[1] * betas[1] + L[3] * betas[0] * betas[2] +
                             L[4] * betas[1] * betas[2] + L[5] * betas[2] * betas[2] + L[6] * betas[0] * betas[3] + L[7] * betas[1] * betas[3] +
                             L[8] * betas[2] * betas[3] + L[9] * betas[3] * betas[3]);
        }
        pnp_qr_solve(A, b, x);
#pragma unroll
        for (int i = 0; i < 4; ++i) betas[i] += x[i];
    }
}

// compute_R_and_t (:651-662) for one beta vector: ccs from the four null-space rows, pcs per point, the sign, Horn-free
// estimate_R_and_t (:569-627) through the 3x3 SVD, and the mean reprojection error (:550-567)
template <class Set, class Ws>
__host__ __device__ inline double pnp_R_and_t(const Set &S, const PnpPts &pts, const PnpCam &K, const PnpGeo &G, Ws &ws, const double betas[4],
                                              double R[9], double t[3])
{
    double ccs[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) ccs[j][0] = ccs[j][1] = ccs[j][2] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) ccs[j][k] += betas[i] * ws.V(11 - i, 3 * j + k);
    auto pc_of = [&](int i, double pc[3]) {
        double a[4];
        pnp_alphas(G, pts.P3D + 3 * (size_t)i, a);
#pragma unroll
        for (int j = 0; j < 3; ++j) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
    };
    // solve_for_sign (:636-649): the depth of the first point decides
    bool first = true, flip = false;
    S.each([&](int i) {
        if (!first) return;
        first = false;
        double pc[3];
        pc_of(i, pc);
        flip = pc[2] < 0.0;
    });
    if (flip)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < 3; ++k) ccs[j][k] = -ccs[j][k];
    int cnt = 0;
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    S.each([&](int i) {
        double pc[3];
        pc_of(i, pc);
        const float *pw = pts.P3D + 3 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            pc0[j] += pc[j];
            pw0[j] += (double)pw[j];
        }
        ++cnt;
    });
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        pc0[j] /= cnt;
        pw0[j] /= cnt;
    }
    PnpLocal<3, 3> ab;   // At = ABt': at[c][j] = abt[3*j + c]
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 3; ++j) ab.at[c][j] = 0;
    S.each([&](int i) {
        double pc[3];
        pc_of(i, pc);
        const float *pw = pts.P3D + 3 * (size_t)i;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) ab.at[c][j] += (pc[j] - pc0[j]) * ((double)pw[c] - pw0[c]);
    });
    // cvSVD(ABt, D, U, V): U[i][k] = the normalised row k of At at i, V[j][k] = the accumulated rotation row k at j
    pnp_jacobi<3, 3, true>(ab);
    pnp_svd_normalise<3, 3>(ab);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = ab.at[0][i] * ab.v[0][j] + ab.at[1][i] * ab.v[1][j] + ab.at[2][i] * ab.v[2][j];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
    if (det < 0) {
        R[6] = -R[6];
        R[7] = -R[7];
        R[8] = -R[8];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = pc0[i] - pnp_dot3(R + 3 * i, pw0);
    double sum2 = 0.0;
    S.each([&](int i) {
        const float *pf = pts.P3D + 3 * (size_t)i;
        const double pw[3] = {(double)pf[0], (double)pf[1], (double)pf[2]};
        const double Xc = pnp_dot3(R, pw) + t[0], Yc = pnp_dot3(R + 3, pw) + t[1], inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
        const double ue = K.uc + K.fu * Xc * inv_Zc, ve = K.vc + K.fv * Yc * inv_Zc;
        const double u = pts.P2D[2 * (size_t)i], v = pts.P2D[2 * (size_t)i + 1];
        sum2 += sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
    });
    return sum2 / cnt;
}

// compute_pose after M'M is in ws.At (:493-524): the SVD, L_6x10 and rho, the three candidates; the smallest error wins, strict `<`
// in the order 1, 2, 3.  rep_errors[3] (optional) receives the three errors.
template <class Set, class Ws>
__host__ __device__ inline double pnp_solve(const Set &S, const PnpPts &pts, const PnpCam &K, const PnpGeo &G, Ws &ws, double R[9], double t[3],
                                            double *rep_errors = nullptr)
{
    pnp_jacobi<12, 12, false>(ws);   // rows 11 .. 8 of the sorted rotations: the null space
    // compute_L_6x10 (:760-800) into rows 0..5 of At, which nothing reads any more
    {
        int a = 0, b = 1;
        for (int i = 0; i < 6; ++i) {
            double dv[4][3];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int c = 0; c < 3; ++c) dv[q][c] = ws.V(11 - q, 3 * a + c) - ws.V(11 - q, 3 * b + c);
            ws.At(i, 0) = pnp_dot3(dv[0], dv[0]);
            ws.At(i, 1) = 2.0 * pnp_dot3(dv[0], dv[1]);
            ws.At(i, 2) = pnp_dot3(dv[1], dv[1]);
            ws.At(i, 3) = 2.0 * pnp_dot3(dv[0], dv[2]);
            ws.At(i, 4) = 2.0 * pnp_dot3(dv[1], dv[2]);
            ws.At(i, 5) = pnp_dot3(dv[2], dv[2]);
            ws.At(i, 6) = 2.0 * pnp_dot3(dv[0], dv[3]);
            ws.At(i, 7) = 2.0 * pnp_dot3(dv[1], dv[3]);
            ws.At(i, 8) = 2.0 * pnp_dot3(dv[2], dv[3]);
            ws.At(i, 9) = pnp_dot3(dv[3], dv[3]);
            if (++b > 3) b = ++a + 1;
        }
    }
    const double rho[6] = {pnp_dist2(G.cws[0], G.cws[1]), pnp_dist2(G.cws[0], G.cws[2]), pnp_dist2(G.cws[0], G.cws[3]),
                           pnp_dist2(G.cws[1], G.cws[2]), pnp_dist2(G.cws[1], G.cws[3]), pnp_dist2(G.cws[2], G.cws[3])};
    double best = 0, Rc[9], tc[3];
    for (int cand = 1; cand <= 3; ++cand) {
        double betas[4];
        if (cand == 1) {   // find_betas_approx_1 (:667-694): columns 0 1 3 6
            PnpLocal<4, 6> s;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                s.at[0][i] = ws.At(i, 0);
                s.at[1][i] = ws.At(i, 1);
                s.at[2][i] = ws.At(i, 3);
                s.at[3][i] = ws.At(i, 6);
            }
            double b4[4];
            pnp_svd_solve<4, 6>(s, rho, b4);
            if (b4[0] < 0) {
                betas[0] = sqrt(-b4[0]);
                betas[1] = -b4[1] / betas[0];
                betas[2] = -b4[2] / betas[0];
                betas[3] = -b4[3] / betas[0];
            } else {
                betas[0] = sqrt(b4[0]);
                betas[1] = b4[1] / betas[0];
                betas[2] = b4[2] / betas[0];
                betas[3] = b4[3] / betas[0];
            }
        } else if (cand == 2) {   // find_betas_approx_2 (:699-726): columns 0 1 2
            PnpLocal<3, 6> s;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int c = 0; c < 3; ++c) s.at[c][i] = ws.At(i, c);
            double b3[3];
            pnp_svd_solve<3, 6>(s, rho, b3);
            if (b3[0] < 0) {
                betas[0] = sqrt(-b3[0]);
                betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
            } else {
                betas[0] = sqrt(b3[0]);
                betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
            }
            if (b3[1] < 0) betas[0] = -betas[0];
            betas[2] = 0.0;
            betas[3] = 0.0;
        } else {   // find_betas_approx_3 (:731-758): columns 0 .. 4
            PnpLocal<5, 6> s;
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int c = 0; c < 5; ++c) s.at[c][i] = ws.At(i, c);
            double b5[5];
            pnp_svd_solve<5, 6>(s, rho, b5);
            if (b5[0] < 0) {
                betas[0] = sqrt(-b5[0]);
                betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
            } else {
                betas[0] = sqrt(b5[0]);
                betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
            }
            if (b5[1] < 0) betas[0] = -betas[0];
            betas[2] = b5[3] / betas[0];
            betas[3] = 0.0;
        }
        pnp_gauss_newton(ws, rho, betas);
        const double err = pnp_R_and_t(S, pts, K, G, ws, betas, Rc, tc);
        if (rep_errors) rep_errors[cand - 1] = err;
        if (cand == 1 || err < best) {
            best = err;
#pragma unroll
            for (int k = 0; k < 9; ++k) R[k] = Rc[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t[k] = tc[k];
        }
    }
    return best;
}

// compute_pose (:477-525) of a set of any size >= 4 -> R (row-major), t; the mean reprojection error of the winner
template <class Set, class Ws>
__host__ __device__ inline double pnp_compute_pose(const Set &S, const PnpPts &pts, const PnpCam &K, Ws &ws, double R[9], double t[3],
                                                   double *rep_errors = nullptr)
{
    PnpGeo G;
    pnp_geometry(S, pts, G);
    pnp_mtm(S, pts, K, G, ws);
    return pnp_solve(S, pts, K, G, ws, R, t, rep_errors);
}

// CheckInliers for one correspondence (:314-329), widths as written: Xc, Yc, invZc are floats of double expressions, ue / ve double,
// distX / distY floats of a double difference, error2 a float expression compared with the float mvMaxError.  Rt = R | t, 12 doubles.
__host__ __device__ inline bool pnp_inlier(const double Rt[12], const PnpCam &K, const PnpPts &pts, int i)
{
    const float *pw = pts.P3D + 3 * (size_t)i;
    const float Xc = (float)(Rt[0] * pw[0] + Rt[1] * pw[1] + Rt[2] * pw[2] + Rt[9]);
    const float Yc = (float)(Rt[3] * pw[0] + Rt[4] * pw[1] + Rt[5] * pw[2] + Rt[10]);
    const float invZc = (float)(1 / (Rt[6] * pw[0] + Rt[7] * pw[1] + Rt[8] * pw[2] + Rt[11]));
    const double ue = K.uc + K.fu * Xc * invZc;
    const double ve = K.vc + K.fv * Yc * invZc;
    const float distX = (float)(pts.P2D[2 * (size_t)i] - ue);
    const float distY = (float)(pts.P2D[2 * (size_t)i + 1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < pts.max_err[i];
}

// mBestTcw / mRefinedTcw (:217-223, :294-300): eye(4, 4, CV_32F) with the doubles converted
__host__ __device__ inline void pnp_Tcw(const double Rt[12], float T[16])
{
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) T[4 * i + j] = (float)Rt[3 * i + j];
        T[4 * i + 3] = (float)Rt[9 + i];
    }
    T[12] = T[13] = T[14] = 0.0f;
    T[15] = 1.0f;
}

// The loop of iterate (:182-239) over the inlier counts of the iterations and the memoised results of Refine(): literal, one
// iteration at a time.  Refine() is a function of the best set alone, so its count is looked up by the iteration that set the best
// (-1: the set carried in from an earlier call).
struct PnpScan {
    int32_t best_inliers, best_iteration = -1, returned_at = -1;
    __host__ __device__ explicit PnpScan(int32_t best_inliers_in) : best_inliers(best_inliers_in) {}
    // the first half of an iteration (:209-224); true: Refine() runs, on the set of best_iteration
    __host__ __device__ bool step(int it, int32_t count, int32_t min_inliers)
    {
        if (count < min_inliers) return false;
        if (count > best_inliers) {
            best_inliers = count;
            best_iteration = it;
        }
        return true;
    }
    // the second half (:226-236) with Refine()'s inlier count; true: iterate() returns here
    __host__ __device__ bool refined(int it, int32_t refined_inliers, int32_t min_inliers)
    {
        if (refined_inliers > min_inliers) {
            returned_at = it;
            return true;
        }
        return false;
    }
};

// validates a batch; run[p] = 0 where nothing is launched (n < min_inliers, :173-177, or no iteration asked for).  csrc/pnp_ransac.hip.
int pnp_check(const aos2_pnp_problem_t *problems, const aos2_pnp_result_t *results, int n_problems, uint8_t *run);
// the results of a problem before anything ran: nothing returned, the carried-in best stands
void pnp_result_clear(const aos2_pnp_problem_t &P, aos2_pnp_result_t &R);

}  // namespace aos2
