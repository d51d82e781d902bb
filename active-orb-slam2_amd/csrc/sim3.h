// The arithmetic of Sim3Solver (src/Sim3Solver.cc): ComputeCentroid (:215-224), ComputeSim3 (:226-337, Horn's closed form with
// cv::eigen of the 4x4 and cv::Rodrigues), Project (:382-403), FromCameraToImage (:405-423) and the inlier test of :350-356.  ONE
// routine for the device kernels (csrc/sim3_ransac.hip) and the host tap (aos2_debug_sim3_host): the translation units are built
// with -ffp-contract=off, so both run the same operation sequence.  The OpenCV conventions it restates are DESIGN.md section 2
// item 9:
//   cv::reduce(SUM): float sums in column order; C / P.cols, vec = 2*ang*vec/norm(vec), (1.0/s)*R.t(): a scale by the double factor
//   rounded to float; matrix products (gemm): products and sums in double in index order, alpha and an addend applied in double, one
//   rounding; Mat::dot, cv::norm: double accumulation; cv::Rodrigues in double, rounded to float at the end;
//   cv::eigen on a symmetric float 4x4: the classical Jacobi of OpenCV 3.2 core/src/lapack.cpp (JacobiImpl_<float>).
// Nothing is indexed at run time: the pivot (k, l) of a Jacobi rotation selects one of six instantiations, reads go through select
// chains, so the 4x4, the eigenvectors and indR / indC stay in registers on the device.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/aos2.h"

namespace aos2 {

// validates a batch and computes mRansacMaxIts of each problem (SetRansacParameters, :125-135) -> its[n_problems]; run[p] = 0 where
// n < min_inliers (:146-150).  csrc/sim3_ransac.hip.
int sim3_check(const aos2_sim3_problem_t *problems, const aos2_sim3_result_t *results, int n_problems, int32_t *its, uint8_t *run);
// the results of a problem nothing ran for
void sim3_result_clear(const aos2_sim3_problem_t &P, int32_t its, aos2_sim3_result_t &R);

struct Sim3Cam {
    float fx, fy, cx, cy;
};

// one hypothesis: mR12i, mt12i, ms12i and the first three rows of mT12i / mT21i (the fourth is 0 0 0 1)
struct Sim3Model {
    float R[9], t[3], s;
    float T12[12], T21[12];
};

// the three indices of an iteration from its draws (:163-177): vAvailableIndices starts as 0..n-1, a drawn position takes the
// value of the back, which is popped
__host__ __device__ inline void sim3_triple(int n, int r0, int r1, int r2, int &i0, int &i1, int &i2)
{
    i0 = r0;
    i1 = r1 == r0 ? n - 1 : r1;
    const int back2 = r0 == n - 2 ? n - 1 : n - 2;   // the back after the first removal
    i2 = r2 == r1 ? back2 : r2 == r0 ? n - 1 : r2;
}

__host__ __device__ inline float sim3_sqrtf(float x) { return (float)sqrt((double)x); }   // the correctly rounded float sqrt

// OpenCV's own hypot helper (lapack.cpp), scaled by the larger argument
__host__ __device__ inline float sim3_hypot(float a, float b)
{
    a = fabsf(a);
    b = fabsf(b);
    if (a > b) {
        b /= a;
        return a * sim3_sqrtf(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * sim3_sqrtf(1 + a * a);
    }
    return 0;
}

__host__ __device__ inline float sim3_pick4(const float v[4], int i) { return i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3]; }

// the state of JacobiImpl_<float> for n = 4: the upper triangle of A, W, V (eigenvectors in rows), and per row / column the
// position of the largest off-diagonal element (indR[k] > k, indC[k] < k)
struct Sim3Jacobi {
    float A[4][4], W[4], V[4][4];
    int indR[4], indC[4];
};

template <int IDX>
__host__ __device__ inline void sim3_jacobi_track(Sim3Jacobi &J)
{
    if (IDX < 3) {
        int m = IDX + 1;
        float mv = fabsf(J.A[IDX][IDX + 1 < 4 ? IDX + 1 : 3]);
#pragma unroll
        for (int i = IDX + 2; i < 4; ++i) {
            const float val = fabsf(J.A[IDX][i]);
            if (mv < val) mv = val, m = i;
        }
        J.indR[IDX] = m;
    }
    if (IDX > 0) {
        int m = 0;
        float mv = fabsf(J.A[0][IDX]);
#pragma unroll
        for (int i = 1; i < IDX; ++i) {
            const float val = fabsf(J.A[i][IDX]);
            if (mv < val) mv = val, m = i;
        }
        J.indC[IDX] = m;
    }
}

__host__ __device__ inline void sim3_rot(float &v0, float &v1, float c, float s)
{
    const float a0 = v0, b0 = v1;
    v0 = a0 * c - b0 * s;
    v1 = a0 * s + b0 * c;
}

// one rotation about the pivot (K, L), K < L
template <int K, int L>
__host__ __device__ inline void sim3_jacobi_rotate(Sim3Jacobi &J, float c, float s, float t)
{
    J.A[K][L] = 0;
    J.W[K] -= t;
    J.W[L] += t;
#pragma unroll
    for (int i = 0; i < K; ++i) sim3_rot(J.A[i][K], J.A[i][L], c, s);
#pragma unroll
    for (int i = K + 1; i < L; ++i) sim3_rot(J.A[K][i], J.A[i][L], c, s);
#pragma unroll
    for (int i = L + 1; i < 4; ++i) sim3_rot(J.A[K][i], J.A[L][i], c, s);
#pragma unroll
    for (int i = 0; i < 4; ++i) sim3_rot(J.V[K][i], J.V[L][i], c, s);
    sim3_jacobi_track<K>(J);
    sim3_jacobi_track<L>(J);
}

// cv::eigen(N, eval, evec) on the symmetric float 4x4 whose upper triangle is N: evec.row(0) -> q.  Only the first pass of the
// final selection sort is made (strict `W[m] < W[i]`): the later passes do not touch row 0.
__host__ __device__ inline void sim3_eigen_top(const float N[4][4], float q[4])
{
    Sim3Jacobi J;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            J.A[i][j] = N[i][j];
            J.V[i][j] = i == j ? 1.0f : 0.0f;
        }
        J.W[i] = N[i][i];
        J.indR[i] = J.indC[i] = 0;
    }
    sim3_jacobi_track<0>(J);
    sim3_jacobi_track<1>(J);
    sim3_jacobi_track<2>(J);
    sim3_jacobi_track<3>(J);
    for (int iters = 0; iters < 4 * 4 * 30; ++iters) {
        // the pivot: the largest of the row maxima, then of the column maxima
        int k = 0;
        float mv = fabsf(sim3_pick4(J.A[0], J.indR[0]));
#pragma unroll
        for (int i = 1; i < 3; ++i) {
            const float val = fabsf(sim3_pick4(J.A[i], J.indR[i]));
            if (mv < val) mv = val, k = i;
        }
        int l = k == 0 ? J.indR[0] : k == 1 ? J.indR[1] : J.indR[2];
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            const float col[4] = {J.A[0][i], J.A[1][i], J.A[2][i], 0.0f};   // (indC[i] < i <= 3)
            const float val = fabsf(sim3_pick4(col, J.indC[i]));
            if (mv < val) mv = val, k = J.indC[i], l = i;
        }
        const int pair = k == 0 ? l - 1 : k == 1 ? l + 1 : 5;   // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const float p = pair == 0 ? J.A[0][1] : pair == 1 ? J.A[0][2] : pair == 2 ? J.A[0][3] : pair == 3 ? J.A[1][2] : pair == 4 ? J.A[1][3] : J.A[2][3];
        if (fabsf(p) <= FLT_EPSILON) break;
        const float y = (sim3_pick4(J.W, l) - sim3_pick4(J.W, k)) * 0.5f;
        float t = fabsf(y) + sim3_hypot(p, y);
        float s = sim3_hypot(p, t);
        const float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        switch (pair) {
        case 0: sim3_jacobi_rotate<0, 1>(J, c, s, t); break;
        case 1: sim3_jacobi_rotate<0, 2>(J, c, s, t); break;
        case 2: sim3_jacobi_rotate<0, 3>(J, c, s, t); break;
        case 3: sim3_jacobi_rotate<1, 2>(J, c, s, t); break;
        case 4: sim3_jacobi_rotate<1, 3>(J, c, s, t); break;
        default: sim3_jacobi_rotate<2, 3>(J, c, s, t); break;
        }
    }
    int m = 0;
    float wm = J.W[0];
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (wm < J.W[i]) wm = J.W[i], m = i;
#pragma unroll
    for (int j = 0; j < 4; ++j) q[j] = m == 0 ? J.V[0][j] : m == 1 ? J.V[1][j] : m == 2 ? J.V[2][j] : J.V[3][j];
}

// ComputeCentroid on a 3x3 whose column i is point i: P[r][i] -> Pr, C
__host__ __device__ inline void sim3_centroid(const float P[3][3], float Pr[3][3], float C[3])
{
    const float third = (float)(1.0 / 3);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        C[r] = ((P[r][0] + P[r][1]) + P[r][2]) * third;
#pragma unroll
        for (int i = 0; i < 3; ++i) Pr[r][i] = P[r][i] - C[r];
    }
}

// cv::Rodrigues on a float 1x3, in double, rounded to float at the end
__host__ __device__ inline void sim3_rodrigues(const float vec[3], float R[9])
{
    double rx = vec[0], ry = vec[1], rz = vec[2];
    const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
    if (theta < DBL_EPSILON) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = (k % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, itheta = theta ? 1.0 / theta : 0.0;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double r_x[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (float)((c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k]) + s * r_x[k]);
}

// ComputeSim3(P1, P2) (:226-337); a, b, c: the three sampled points of each set
__host__ __device__ inline void sim3_horn(const float a1[3], const float b1[3], const float c1[3], const float a2[3], const float b2[3],
                                          const float c2[3], bool fix_scale, Sim3Model &m)
{
    float P1[3][3], P2[3][3], Pr1[3][3], Pr2[3][3], O1[3], O2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        P1[r][0] = a1[r]; P1[r][1] = b1[r]; P1[r][2] = c1[r];
        P2[r][0] = a2[r]; P2[r][1] = b2[r]; P2[r][2] = c2[r];
    }
    sim3_centroid(P1, Pr1, O1);
    sim3_centroid(P2, Pr2, O2);
    // M = Pr2 * Pr1.t()
    float M[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            M[i][j] = (float)(((double)Pr2[i][0] * (double)Pr1[j][0] + (double)Pr2[i][1] * (double)Pr1[j][1]) + (double)Pr2[i][2] * (double)Pr1[j][2]);
    // N11 .. N44 (:251-260): float expressions, left to right
    float N[4][4];
    N[0][0] = M[0][0] + M[1][1] + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = M[0][0] - M[1][1] - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = -M[0][0] + M[1][1] - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = -M[0][0] - M[1][1] + M[2][2];
    N[1][0] = N[0][1]; N[2][0] = N[0][2]; N[3][0] = N[0][3]; N[2][1] = N[1][2]; N[3][1] = N[1][3]; N[3][2] = N[2][3];
    float q[4];
    sim3_eigen_top(N, q);
    // angle-axis (:274-280) and cv::Rodrigues (:284)
    const double nrm = sqrt(((double)q[1] * (double)q[1] + (double)q[2] * (double)q[2]) + (double)q[3] * (double)q[3]);
    const double ang = atan2(nrm, (double)q[0]);
    const float f = (float)((2 * ang) * (1.0 / nrm));
    const float vec[3] = {q[1] * f, q[2] * f, q[3] * f};
    sim3_rodrigues(vec, m.R);
    // P3 = mR12i * Pr2; scale (:292-311)
    if (!fix_scale) {
        double nom = 0, den = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const float P3 = (float)(((double)m.R[3 * i] * (double)Pr2[0][j] + (double)m.R[3 * i + 1] * (double)Pr2[1][j]) + (double)m.R[3 * i + 2] * (double)Pr2[2][j]);
                nom += (double)Pr1[i][j] * (double)P3;
                den += (double)(P3 * P3);
            }
        m.s = (float)(nom / den);
    } else
        m.s = 1.0f;
    // mt12i = O1 - ms12i * mR12i * O2; T12 = [s R | t]; T21 = [(1/s) R.t() | -sRinv * t]
    const float sinv = (float)(1.0 / (double)m.s);
    float sRinv[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double acc = ((double)m.R[3 * i] * (double)O2[0] + (double)m.R[3 * i + 1] * (double)O2[1]) + (double)m.R[3 * i + 2] * (double)O2[2];
        m.t[i] = (float)((double)O1[i] - (double)m.s * acc);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            m.T12[4 * i + j] = m.R[3 * i + j] * m.s;
            sRinv[3 * i + j] = m.R[3 * j + i] * sinv;
            m.T21[4 * i + j] = sRinv[3 * i + j];
        }
        m.T12[4 * i + 3] = m.t[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        m.T21[4 * i + 3] = (float)-(((double)sRinv[3 * i] * (double)m.t[0] + (double)sRinv[3 * i + 1] * (double)m.t[1]) + (double)sRinv[3 * i + 2] * (double)m.t[2]);
}

// FromCameraToImage of one point (:415-421)
__host__ __device__ inline void sim3_to_image(const Sim3Cam &K, float X, float Y, float Z, float &u, float &v)
{
    const float invz = 1 / Z;
    const float x = X * invz, y = Y * invz;
    u = K.fx * x + K.cx;
    v = K.fy * y + K.cy;
}

// Project of one point (:394-401): T = the first three rows of Tcw
__host__ __device__ inline void sim3_project(const float T[12], const Sim3Cam &K, const float P[3], float &u, float &v)
{
    float c[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
        c[i] = (float)((((double)T[4 * i] * (double)P[0] + (double)T[4 * i + 1] * (double)P[1]) + (double)T[4 * i + 2] * (double)P[2]) + (double)T[4 * i + 3]);
    sim3_to_image(K, c[0], c[1], c[2], u, v);
}

// the two errors of :350-354 for one correspondence
__host__ __device__ inline void sim3_errors(const float T12[12], const float T21[12], const Sim3Cam &K1, const Sim3Cam &K2, const float X1[3],
                                            const float X2[3], float &err1, float &err2)
{
    float p1u, p1v, p2u, p2v, q1u, q1v, q2u, q2v;
    sim3_to_image(K1, X1[0], X1[1], X1[2], p1u, p1v);   // mvP1im1
    sim3_to_image(K2, X2[0], X2[1], X2[2], p2u, p2v);   // mvP2im2
    sim3_project(T12, K1, X2, q1u, q1v);                // vP2im1
    sim3_project(T21, K2, X1, q2u, q2v);                // vP1im2
    const float d1x = p1u - q1u, d1y = p1v - q1v, d2x = q2u - p2u, d2y = q2v - p2v;
    err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
    err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
}

// :356
__host__ __device__ inline bool sim3_inlier(const float T12[12], const float T21[12], const Sim3Cam &K1, const Sim3Cam &K2, const float X1[3],
                                            const float X2[3], float max_err1, float max_err2)
{
    float err1, err2;
    sim3_errors(T12, T21, K1, K2, X1, X2, err1, err2);
    return err1 < max_err1 && err2 < max_err2;
}

// the model of iteration `it` of a problem from its draws
__host__ __device__ inline void sim3_model_of(int n, const float *X1, const float *X2, const int32_t *draws, int it, bool fix_scale, Sim3Model &m)
{
    int i0, i1, i2;
    sim3_triple(n, draws[3 * it], draws[3 * it + 1], draws[3 * it + 2], i0, i1, i2);
    sim3_horn(X1 + 3 * (size_t)i0, X1 + 3 * (size_t)i1, X1 + 3 * (size_t)i2, X2 + 3 * (size_t)i0, X2 + 3 * (size_t)i1, X2 + 3 * (size_t)i2, fix_scale, m);
}

// the state of the loop of :158-201 over the counts of the iterations: literal, one iteration at a time
struct Sim3Scan {
    int32_t best_inliers = 0, best_iteration = -1, first_success = -1;
    // true: iterate() returns here
    __host__ __device__ bool step(int it, int32_t count, int32_t min_inliers)
    {
        if (count >= best_inliers) {
            best_inliers = count;
            best_iteration = it;
            if (count > min_inliers) {
                first_success = it;
                return true;
            }
        }
        return false;
    }
};

}  // namespace aos2
