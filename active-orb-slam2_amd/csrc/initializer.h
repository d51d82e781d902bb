// Initializer (src/Initializer.cc): Normalize, ComputeH21 / ComputeF21, CheckHomography / CheckFundamental, the model pick,
// ReconstructF + DecomposeE, ReconstructH and CheckRT, ONE routine each for the device kernels (csrc/initializer_ransac.hip) and the
// host tap (aos2_debug_initializer_host).  The translation units are built with -ffp-contract=off, so both run the same operation
// sequence.  The OpenCV routines it stands for are DESIGN.md section 2 item 12 (parity unpinned): the float one-sided Jacobi of item
// 8 at 16x9, 8x9 and 3x3 with the left factor's tail loop (normalisation, and the completion row of the wide case), the 3x3
// inverse / determinant in double, and item 9's gemm / norm rules.  The 4x4 of Initializer::Triangulate is csrc/triangulate.h's.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "../../include/aos2.h"
#include "triangulate.h"

namespace aos2 {

// cv::RNG: the multiply-with-carry generator behind JacobiSVDImpl_'s completion vectors
struct InitRng {
    uint64_t state;
    __host__ __device__ uint32_t next()
    {
        state = (uint64_t)(uint32_t)state * 4164903690U + (uint32_t)(state >> 32);
        return (uint32_t)state;
    }
};

// the workspace of one solver on the host: At up to 9 rows of 16, V up to 9x9, W.  The device's is InitLds (same accessors).
struct InitLocal {
    float a[9 * 16], v[9 * 9];
    double w[9];
    __host__ __device__ float &A(int i, int k) { return a[i * 16 + k]; }
    __host__ __device__ float &V(int i, int k) { return v[i * 9 + k]; }
    __host__ __device__ double &W(int i) { return w[i]; }
};

// JacobiSVDImpl_<float> up to the sort: n rows of length m in A, V = I (n x n) rotated along, rows sorted into descending W
template <class WS>
__host__ __device__ inline void init_jacobi(WS &ws, int m, int n)
{
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) {
            const float t = ws.A(i, k);
            sd += (double)t * (double)t;
        }
        ws.W(i) = sd;
        for (int k = 0; k < n; ++k) ws.V(i, k) = k == i ? 1.0f : 0.0f;
    }
    const double eps = (double)(FLT_EPSILON * 2);
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                double a = ws.W(i), b = ws.W(j), p = 0;
                for (int k = 0; k < m; ++k) p += (double)ws.A(i, k) * (double)ws.A(j, k);
                if (fabs(p) <= eps * sqrt(a * b)) continue;
                p *= 2;
                const double beta = a - b, gamma = sqrt(p * p + beta * beta);
                float c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = (float)sqrt(delta / gamma);
                    c = (float)(p / (gamma * (double)s * 2));
                } else {
                    c = (float)sqrt((gamma + beta) / (gamma * 2));
                    s = (float)(p / (gamma * (double)c * 2));
                }
                a = b = 0;
                for (int k = 0; k < m; ++k) {
                    const float x = ws.A(i, k), y = ws.A(j, k);
                    const float t0 = c * x + s * y;
                    const float t1 = -s * x + c * y;
                    ws.A(i, k) = t0;
                    ws.A(j, k) = t1;
                    a += (double)t0 * (double)t0;
                    b += (double)t1 * (double)t1;
                }
                ws.W(i) = a;
                ws.W(j) = b;
                changed = true;
                for (int k = 0; k < n; ++k) {
                    const float x = ws.V(i, k), y = ws.V(j, k);
                    const float t0 = c * x + s * y;
                    const float t1 = -s * x + c * y;
                    ws.V(i, k) = t0;
                    ws.V(j, k) = t1;
                }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) {
            const float t = ws.A(i, k);
            sd += (double)t * (double)t;
        }
        ws.W(i) = sqrt(sd);
    }
    for (int i = 0; i < n - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < n; ++k)
            if (ws.W(j) < ws.W(k)) j = k;
        if (i != j) {
            const double t = ws.W(i);
            ws.W(i) = ws.W(j);
            ws.W(j) = t;
            for (int k = 0; k < m; ++k) {
                const float f = ws.A(i, k);
                ws.A(i, k) = ws.A(j, k);
                ws.A(j, k) = f;
            }
            for (int k = 0; k < n; ++k) {
                const float f = ws.V(i, k);
                ws.V(i, k) = ws.V(j, k);
                ws.V(j, k) = f;
            }
        }
    }
}

// the tail loop of JacobiSVDImpl_: rows 0 .. n1-1 of A become the left factor.  A row with W > FLT_MIN is scaled by (float)(1/W);
// a row without one (every row i >= n) is the completion vector: +-1/m by the generator's bit 8, two passes of subtraction against
// the rows before it, each followed by a scale by 1/sum|.| (0 when that sum is at most 100 eps), then the 2-norm in double
template <class WS>
__host__ __device__ inline void init_svd_tail(WS &ws, int m, int n, int n1)
{
    const double minval = (double)FLT_MIN;
    const float eps = FLT_EPSILON * 2;
    InitRng rng{0x12345678};
    for (int i = 0; i < n1; ++i) {
        double sd = i < n ? ws.W(i) : 0;
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            const float val0 = (float)(1. / m);
            for (int k = 0; k < m; ++k) ws.A(i, k) = (rng.next() & 256) != 0 ? val0 : -val0;
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    sd = 0;
                    for (int k = 0; k < m; ++k) sd += (double)(ws.A(i, k) * ws.A(j, k));
                    float asum = 0;
                    for (int k = 0; k < m; ++k) {
                        const float t = (float)((double)ws.A(i, k) - sd * (double)ws.A(j, k));
                        ws.A(i, k) = t;
                        asum += fabsf(t);
                    }
                    asum = asum > eps * 100 ? 1 / asum : 0;
                    for (int k = 0; k < m; ++k) ws.A(i, k) *= asum;
                }
            sd = 0;
            for (int k = 0; k < m; ++k) {
                const float t = ws.A(i, k);
                sd += (double)t * (double)t;
            }
            sd = sqrt(sd);
        }
        const float s = (float)(sd > minval ? 1 / sd : 0.);
        for (int k = 0; k < m; ++k) ws.A(i, k) *= s;
    }
}

// ---- float 3x3 helpers (row-major) ----------------------------------------------------------------------------------------------
// cv::gemm: C = alpha * A * B, products and sums in double in index order, one rounding
__host__ __device__ inline void init_mul33(const float *A, const float *B, float *C, double alpha = 1.0)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            C[3 * i + j] = (float)(alpha * (((double)A[3 * i] * (double)B[j] + (double)A[3 * i + 1] * (double)B[3 + j]) + (double)A[3 * i + 2] * (double)B[6 + j]));
}
__host__ __device__ inline void init_transpose33(const float *A, float *At)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) At[3 * j + i] = A[3 * i + j];
}
// A * v (+ add), the same rule
__host__ __device__ inline void init_mulv3(const float *A, const float *v, float *o, double a0 = 0, double a1 = 0, double a2 = 0, bool add = false)
{
    const double ad[3] = {a0, a1, a2};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double s = ((double)A[3 * i] * (double)v[0] + (double)A[3 * i + 1] * (double)v[1]) + (double)A[3 * i + 2] * (double)v[2];
        o[i] = add ? (float)(s + ad[i]) : (float)s;
    }
}
// cv::determinant of a float 3x3: in double, returned as the double
__host__ __device__ inline double init_det33(const float *m)
{
    return (double)m[0] * ((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) -
           (double)m[1] * ((double)m[3] * (double)m[8] - (double)m[5] * (double)m[6]) +
           (double)m[2] * ((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]);
}
// cv::Mat::inv() of a float 3x3: adjugate terms as double products times 1/det, rounded once; det == 0 gives zeros
__host__ __device__ inline void init_inv33(const float *S, float *D)
{
    double d = init_det33(S);
    if (d == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) D[k] = 0.0f;
        return;
    }
    d = 1. / d;
    D[0] = (float)(((double)S[4] * (double)S[8] - (double)S[5] * (double)S[7]) * d);
    D[1] = (float)(((double)S[2] * (double)S[7] - (double)S[1] * (double)S[8]) * d);
    D[2] = (float)(((double)S[1] * (double)S[5] - (double)S[2] * (double)S[4]) * d);
    D[3] = (float)(((double)S[5] * (double)S[6] - (double)S[3] * (double)S[8]) * d);
    D[4] = (float)(((double)S[0] * (double)S[8] - (double)S[2] * (double)S[6]) * d);
    D[5] = (float)(((double)S[2] * (double)S[3] - (double)S[0] * (double)S[5]) * d);
    D[6] = (float)(((double)S[3] * (double)S[7] - (double)S[4] * (double)S[6]) * d);
    D[7] = (float)(((double)S[1] * (double)S[6] - (double)S[0] * (double)S[7]) * d);
    D[8] = (float)(((double)S[0] * (double)S[4] - (double)S[1] * (double)S[3]) * d);
}
// t / cv::norm(t): a scale by the double reciprocal of the double norm, one rounding
__host__ __device__ inline void init_unit3(float *t)
{
    const double r = 1.0 / sqrt(((double)t[0] * (double)t[0] + (double)t[1] * (double)t[1]) + (double)t[2] * (double)t[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = (float)((double)t[k] * r);
}

// cv::SVD::compute of a general float 3x3: U[i][k] = row k of At scaled by (float)(1/W[k]), w, vt = the rotations
template <class WS>
__host__ __device__ inline void init_svd33(WS &ws, const float *M, float *U, float *w, float *Vt)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int k = 0; k < 3; ++k) ws.A(i, k) = M[3 * k + i];
    init_jacobi(ws, 3, 3);
    init_svd_tail(ws, 3, 3, 3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        w[i] = (float)ws.W(i);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            U[3 * i + k] = ws.A(k, i);
            Vt[3 * i + k] = ws.V(i, k);
        }
    }
}

// ---- Normalize (:749-795) -------------------------------------------------------------------------------------------------------
// one axis of one frame: mean and 1/meanDev, both float sums in index order over ALL keys (pts: float pairs, axis 0 / 1)
__host__ __device__ inline void init_normalize_axis(const float *pts, int n, int axis, float *mean_out, float *s_out)
{
    float mean = 0;
    for (int i = 0; i < n; ++i) mean += pts[2 * i + axis];
    mean = mean / n;
    float dev = 0;
    for (int i = 0; i < n; ++i) dev += fabsf(pts[2 * i + axis] - mean);
    dev = dev / n;
    *mean_out = mean;
    *s_out = (float)(1.0 / (double)dev);
}
// nrm = (meanX, sX, meanY, sY) -> T
__host__ __device__ inline void init_T(const float *nrm, float *T)
{
    T[0] = nrm[1]; T[1] = 0; T[2] = -nrm[0] * nrm[1];
    T[3] = 0; T[4] = nrm[3]; T[5] = -nrm[2] * nrm[3];
    T[6] = 0; T[7] = 0; T[8] = 1;
}

// what a solver reads of one problem
struct InitPts {
    const float *keys1, *keys2;      // [n_keys][2]
    const int32_t *matches;          // [n_matches][2]
    const float *nrm1, *nrm2;        // (meanX, sX, meanY, sY) of each frame
};

// the normalised points of match idx (:155-156)
__host__ __device__ inline void init_norm_pair(const InitPts &P, int idx, float &u1, float &v1, float &u2, float &v2)
{
    const int a = P.matches[2 * idx], b = P.matches[2 * idx + 1];
    u1 = (P.keys1[2 * a] - P.nrm1[0]) * P.nrm1[1];
    v1 = (P.keys1[2 * a + 1] - P.nrm1[2]) * P.nrm1[3];
    u2 = (P.keys2[2 * b] - P.nrm2[0]) * P.nrm2[1];
    v2 = (P.keys2[2 * b + 1] - P.nrm2[2]) * P.nrm2[3];
}

// ComputeH21 (:226-266) of one set + the denormalisation (:160-161) -> H21i, H12i
template <class WS>
__host__ __device__ inline void init_model_h(const InitPts &P, const int32_t *set, WS &ws, float *H21, float *H12)
{
    for (int i = 0; i < 8; ++i) {
        float u1, v1, u2, v2;
        init_norm_pair(P, set[i], u1, v1, u2, v2);
        const int r = 2 * i;
        ws.A(0, r) = 0.0f; ws.A(1, r) = 0.0f; ws.A(2, r) = 0.0f;
        ws.A(3, r) = -u1; ws.A(4, r) = -v1; ws.A(5, r) = -1.0f;
        ws.A(6, r) = v2 * u1; ws.A(7, r) = v2 * v1; ws.A(8, r) = v2;
        ws.A(0, r + 1) = u1; ws.A(1, r + 1) = v1; ws.A(2, r + 1) = 1.0f;
        ws.A(3, r + 1) = 0.0f; ws.A(4, r + 1) = 0.0f; ws.A(5, r + 1) = 0.0f;
        ws.A(6, r + 1) = -u2 * u1; ws.A(7, r + 1) = -u2 * v1; ws.A(8, r + 1) = -u2;
    }
    init_jacobi(ws, 16, 9);
    float Hn[9], T1[9], T2[9], T2inv[9], tmp[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Hn[k] = ws.V(8, k);
    init_T(P.nrm1, T1);
    init_T(P.nrm2, T2);
    init_inv33(T2, T2inv);
    init_mul33(T2inv, Hn, tmp);
    init_mul33(tmp, T1, H21);
    init_inv33(H21, H12);
}

// ComputeF21 (:268-303) of one set + the denormalisation (:212) -> F21i
template <class WS>
__host__ __device__ inline void init_model_f(const InitPts &P, const int32_t *set, WS &ws, float *F21)
{
    for (int i = 0; i < 8; ++i) {
        float u1, v1, u2, v2;
        init_norm_pair(P, set[i], u1, v1, u2, v2);
        ws.A(i, 0) = u2 * u1; ws.A(i, 1) = u2 * v1; ws.A(i, 2) = u2;
        ws.A(i, 3) = v2 * u1; ws.A(i, 4) = v2 * v1; ws.A(i, 5) = v2;
        ws.A(i, 6) = u1; ws.A(i, 7) = v1; ws.A(i, 8) = 1.0f;
    }
    init_jacobi(ws, 9, 8);
    init_svd_tail(ws, 9, 8, 9);
    float Fpre[9], U[9], w[3], Vt[9], D[9], tmp[9], Fn[9], T1[9], T2[9], T2t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) Fpre[k] = ws.A(8, k);
    init_svd33(ws, Fpre, U, w, Vt);
    w[2] = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) D[k] = 0.0f;
    D[0] = w[0]; D[4] = w[1]; D[8] = w[2];
    init_mul33(U, D, tmp);
    init_mul33(tmp, Vt, Fn);
    init_T(P.nrm1, T1);
    init_T(P.nrm2, T2);
    init_transpose33(T2, T2t);
    init_mul33(T2t, Fn, tmp);
    init_mul33(tmp, T1, F21);
}

// ---- CheckHomography / CheckFundamental (:305-468): the two addends of one match (+0 where the reference adds nothing: the score
// is never negative, so s + 0 is s) and its inlier flag --------------------------------------------------------------------------
__host__ __device__ inline float init_inv_sigma2(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }

__host__ __device__ inline bool init_terms_h(const float *h, const float *hi, float invSigmaSquare, float u1, float v1, float u2, float v2,
                                             float &a, float &b)
{
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(hi[6] * u2 + hi[7] * v2 + hi[8]));
    const float u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
    const float v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; a = 0.0f; }
    else a = th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
    const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; b = 0.0f; }
    else b = th - chiSquare2;
    return bIn;
}

__host__ __device__ inline bool init_terms_f(const float *f, float invSigmaSquare, float u1, float v1, float u2, float v2, float &a, float &b)
{
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2 = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) { bIn = false; a = 0.0f; }
    else a = thScore - chiSquare1;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1 = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) { bIn = false; b = 0.0f; }
    else b = thScore - chiSquare2;
    return bIn;
}

// model: 18 floats (H21 | H12) or 9 (F21); is_h selects the check
__host__ __device__ inline bool init_terms(bool is_h, const float *model, float invSigmaSquare, const InitPts &P, int i, float &a, float &b)
{
    const int k1 = P.matches[2 * i], k2 = P.matches[2 * i + 1];
    const float u1 = P.keys1[2 * k1], v1 = P.keys1[2 * k1 + 1], u2 = P.keys2[2 * k2], v2 = P.keys2[2 * k2 + 1];
    return is_h ? init_terms_h(model, model + 9, invSigmaSquare, u1, v1, u2, v2, a, b) : init_terms_f(model, invSigmaSquare, u1, v1, u2, v2, a, b);
}

// the model pick (:165, :216): the first iteration whose score is strictly greater than every earlier one, from 0.0; NaN never wins
__host__ __device__ inline int init_pick(const float *scores, int its, float *best_score)
{
    float score = 0.0f;
    int best = -1;
    for (int it = 0; it < its; ++it)
        if (scores[it] > score) {
            score = scores[it];
            best = it;
        }
    *best_score = score;
    return best;
}

// ---- the motion hypotheses -------------------------------------------------------------------------------------------------------
struct InitCam { float fx, fy, cx, cy; };
__host__ __device__ inline void init_K(const InitCam &c, float *K)
{
    K[0] = c.fx; K[1] = 0; K[2] = c.cx;
    K[3] = 0; K[4] = c.fy; K[5] = c.cy;
    K[6] = 0; K[7] = 0; K[8] = 1;
}

// ReconstructF :479-487 + DecomposeE (:909-929): hypothesis k of R[4][9], t[4][3] = (R1,t1) (R2,t1) (R1,t2) (R2,t2)
template <class WS>
__host__ __device__ inline void init_hyps_f(const float *F21, const InitCam &cam, WS &ws, float *R, float *t)
{
    float K[9], Kt[9], tmp[9], E[9], U[9], w[3], Vt[9];
    init_K(cam, K);
    init_transpose33(K, Kt);
    init_mul33(Kt, F21, tmp);
    init_mul33(tmp, K, E);
    init_svd33(ws, E, U, w, Vt);
    float tt[3] = {U[2], U[5], U[8]};
    init_unit3(tt);
    const float W[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
    float Wt[9], R1[9], R2[9];
    init_transpose33(W, Wt);
    init_mul33(U, W, tmp);
    init_mul33(tmp, Vt, R1);
    if (init_det33(R1) < 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
    init_mul33(U, Wt, tmp);
    init_mul33(tmp, Vt, R2);
    if (init_det33(R2) < 0)
#pragma unroll
        for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        R[k] = R1[k];
        R[9 + k] = R2[k];
        R[18 + k] = R1[k];
        R[27 + k] = R2[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t[k] = tt[k];
        t[3 + k] = tt[k];
        t[6 + k] = -tt[k];
        t[9 + k] = -tt[k];
    }
}

// ReconstructH :584-686: the eight (R, t) of Faugeras; false: the d1/d2 < 1.00001 || d2/d3 < 1.00001 exit
template <class WS>
__host__ __device__ inline bool init_hyps_h(const float *H21, const InitCam &cam, WS &ws, float *R, float *t)
{
    float K[9], invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    init_K(cam, K);
    init_inv33(K, invK);
    init_mul33(invK, H21, tmp);
    init_mul33(tmp, K, A);
    init_svd33(ws, A, U, w, Vt);
    const float s = (float)(init_det33(U) * init_det33(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    for (int i = 0; i < 8; ++i) {
        const int q = i & 3;
        const float x1 = q < 2 ? aux1 : -aux1, x3 = (q & 1) ? -aux3 : aux3;
        const bool pos = q == 0 || q == 3;
        float Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, tp[3];
        if (i < 4) {
            const float st = pos ? aux_stheta : -aux_stheta;
            Rp[0] = ctheta; Rp[2] = -st; Rp[6] = st; Rp[8] = ctheta;
            tp[0] = x1; tp[1] = 0; tp[2] = -x3;
#pragma unroll
            for (int k = 0; k < 3; ++k) tp[k] *= d1 - d3;
        } else {
            const float sp = pos ? aux_sphi : -aux_sphi;
            Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1; Rp[6] = sp; Rp[8] = -cphi;
            tp[0] = x1; tp[1] = 0; tp[2] = x3;
#pragma unroll
            for (int k = 0; k < 3; ++k) tp[k] *= d1 + d3;
        }
        float Ri[9], ti[3];
        init_mul33(U, Rp, tmp, (double)s);
        init_mul33(tmp, Vt, Ri);
        init_mulv3(U, tp, ti);
        init_unit3(ti);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[9 * i + k] = Ri[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) t[3 * i + k] = ti[k];
    }
    return true;
}

// ---- CheckRT (:798-907) ----------------------------------------------------------------------------------------------------------
struct InitRT {
    float R[9], t[3], P1[12], P2[12], O2[3];
};
__host__ __device__ inline void init_rt_setup(const float *R, const float *t, const InitCam &cam, InitRT &S)
{
    float K[9];
    init_K(cam, K);
#pragma unroll
    for (int k = 0; k < 9; ++k) S.R[k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) S.t[k] = t[k];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            S.P1[4 * i + j] = j < 3 ? K[3 * i + j] : 0.0f;
            const float c0 = j < 3 ? R[j] : t[0], c1 = j < 3 ? R[3 + j] : t[1], c2 = j < 3 ? R[6 + j] : t[2];
            S.P2[4 * i + j] = (float)(((double)K[3 * i] * (double)c0 + (double)K[3 * i + 1] * (double)c1) + (double)K[3 * i + 2] * (double)c2);
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)   // O2 = -R.t() * t
        S.O2[i] = (float)(-1.0 * (((double)R[i] * (double)t[0] + (double)R[3 + i] * (double)t[1]) + (double)R[6 + i] * (double)t[2]));
}

// isfinite(float): the exponent is not all ones
__host__ __device__ inline bool init_finite(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return (b & 0x7f800000u) != 0x7f800000u;
}

enum { INIT_RT_GOOD = 1, INIT_RT_CLEARS = 2, INIT_RT_SETS = 4 };   // counted (P3D, cosine); vbGood[first] = false; vbGood[first] = true

// one inlier match: what the loop body does with it.  p, cosp are valid with INIT_RT_GOOD.
__host__ __device__ inline int init_rt_point(const InitRT &S, const InitCam &cam, float th2, float u1, float v1, float u2, float v2, float *p,
                                             float *cosp)
{
    const TriKf K1 = {S.P1, 0, 0, 0, 0, 0, 0, nullptr}, K2 = {S.P2, 0, 0, 0, 0, 0, 0, nullptr};
    const float xn[4] = {u1, v1, u2, v2};
    float v[4];
    tri_svd_null(K1, K2, xn, v);
    if (!tri_dehomogenize(v, p)) return INIT_RT_CLEARS;   // x / 0: not finite
    if (!init_finite(p[0]) || !init_finite(p[1]) || !init_finite(p[2])) return INIT_RT_CLEARS;
    const float dist1 = (float)sqrt(tri_dot3(p, p));
    const float n2[3] = {p[0] - S.O2[0], p[1] - S.O2[1], p[2] - S.O2[2]};
    const float dist2 = (float)sqrt(tri_dot3(n2, n2));
    const float cosParallax = (float)(tri_dot3(p, n2) / (double)(dist1 * dist2));
    if (p[2] <= 0 && (double)cosParallax < 0.99998) return 0;
    float p2[3];
    init_mulv3(S.R, p, p2, (double)S.t[0], (double)S.t[1], (double)S.t[2], true);
    if (p2[2] <= 0 && (double)cosParallax < 0.99998) return 0;
    const float invZ1 = (float)(1.0 / (double)p[2]);
    const float im1x = cam.fx * p[0] * invZ1 + cam.cx, im1y = cam.fy * p[1] * invZ1 + cam.cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 0;
    const float invZ2 = (float)(1.0 / (double)p2[2]);
    const float im2x = cam.fx * p2[0] * invZ2 + cam.cx, im2y = cam.fy * p2[1] * invZ2 + cam.cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 0;
    *cosp = cosParallax;
    return INIT_RT_GOOD | ((double)cosParallax < 0.99998 ? INIT_RT_SETS : 0);
}

// acos(c) * 180 / CV_PI (:901): the float overload as the double function rounded (item 5's rule), a float product, a double quotient
__host__ __device__ inline float init_parallax_deg(float c)
{
    const float a = (float)acos((double)c);
    return (float)((double)(a * 180) / 3.1415926535897932384626433832795);
}
// a float as a key whose unsigned order is the float order (the order statistic of the cosines is found on keys)
__host__ __device__ inline uint32_t init_float_key(float f)
{
    uint32_t b;
    memcpy(&b, &f, 4);
    return (b & 0x80000000u) ? ~b : b | 0x80000000u;
}
__host__ __device__ inline float init_key_float(uint32_t k)
{
    const uint32_t b = (k & 0x80000000u) ? k & 0x7fffffffu : ~k;
    float f;
    memcpy(&f, &b, 4);
    return f;
}
__host__ __device__ inline float init_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

// the decisions: the hypothesis that initialises, or -1
__host__ __device__ inline int init_decide_f(const int32_t *nGood, const float *parallax, int N, float minParallax, int minTriangulated)
{
    int maxGood = nGood[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) maxGood = nGood[k] > maxGood ? nGood[k] : maxGood;
    const int n09 = (int)(0.9 * N);
    const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
    int nsimilar = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if ((double)nGood[k] > 0.7 * maxGood) nsimilar++;
    if (maxGood < nMinGood || nsimilar > 1) return -1;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (maxGood == nGood[k]) return parallax[k] > minParallax ? k : -1;
    return -1;
}
__host__ __device__ inline int init_decide_h(const int32_t *nGood, const float *parallax, int N, float minParallax, int minTriangulated)
{
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    float bestParallax = -1;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        if (nGood[i] > bestGood) {
            secondBestGood = bestGood;
            bestGood = nGood[i];
            bestSolutionIdx = i;
            bestParallax = parallax[i];
        } else if (nGood[i] > secondBestGood) {
            secondBestGood = nGood[i];
        }
    }
    if ((double)secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && (double)bestGood > 0.9 * N)
        return bestSolutionIdx;
    return -1;
}

// the argument checks of both entry points (csrc/initializer_ransac.hip) and the cleared result
int initializer_check(const aos2_initializer_problem_t *problems, const aos2_initializer_result_t *results, int n_problems);
void initializer_result_clear(const aos2_initializer_problem_t &P, aos2_initializer_result_t &R);

}  // namespace aos2
