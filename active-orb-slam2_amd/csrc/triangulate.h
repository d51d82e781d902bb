// The per-match body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:295-436): parallax test, linear triangulation
// (cv::SVD of a 4x4), the KeyFrame::UnprojectStereo fallbacks (src/KeyFrame.cc:676-692) and the depth / reprojection / scale
// gates that decide whether a MapPoint is born.  ONE routine for the device kernels (csrc/frames_keyframe.hip on resident keyframe
// batches, csrc/triangulate.hip on the matcher's handle; tri_block below is the workgroup form both run) and the host tap
// (aos2_debug_triangulate_host): the translation units are built with -ffp-contract=off, so all run the same operation
// sequence.  The OpenCV conventions it restates are DESIGN.md section 2.7:
//   cv::Mat products, Mat::dot, cv::norm: products and sums in double in index order, an addend widened to double, one rounding;
//   A.row(k) = xn * Tcw.row(2) - Tcw.row(r): float multiply, float subtract;
//   x3D.rowRange(0,3) / w: a scale by the float reciprocal (float)(1.0 / (double)w);
//   cos(2 * atan2(mb / 2, depth)): the float overloads = the double functions rounded to float;
//   cv::SVD::compute on a float 4x4: the one-sided Jacobi of OpenCV 3.2 core/src/lapack.cpp (JacobiSVDImpl_<float>).
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/aos2.h"

namespace aos2 {

// the members of one keyframe the loop reads: mTcw (row-major 4x4), fx fy cx cy mb mbf, mvScaleFactors
struct TriKf {
    const float *T;
    float fx, fy, cx, cy, mb, mbf;
    const float *sf;
};

// one feature of a keyframe: mvKeysUn[i].pt, mvKeys[i].pt (UnprojectStereo reads the distorted key), mvuRight[i], mvDepth[i],
// mvKeysUn[i].octave
struct TriObs {
    float ux, uy, kx, ky, ur, depth;
    int32_t octave;
};

// the argument checks of the host-pointer form and the host tap (csrc/triangulate.hip): everything the routine indexes with
int triang_check(const aos2_triang_geom_t *g, int n, const aos2_triang_obs_t *obs1, const aos2_triang_obs_t *obs2, const float *x3D,
                 const uint8_t *status);

enum { TRI_BRANCH_NONE = 0, TRI_BRANCH_SVD = 1, TRI_BRANCH_STEREO1 = 2, TRI_BRANCH_STEREO2 = 3 };

// Ow = -Rcw.t() * tcw (KeyFrame::SetPose, src/KeyFrame.cc:64-82; cv::gemm: double accumulation, one rounding)
__host__ __device__ inline void tri_center(const float *T, float Ow[3])
{
    for (int k = 0; k < 3; ++k) {
        const double sacc = ((double)T[k] * (double)T[3] + (double)T[4 + k] * (double)T[7]) + (double)T[8 + k] * (double)T[11];
        Ow[k] = (float)(sacc * -1.0);
    }
}

// Rwc * v: row i of Rwc is column i of Rcw
__host__ __device__ inline void tri_rot_wc(const float *T, const float v[3], double addend0, double addend1, double addend2, float out[3])
{
    const double add[3] = {addend0, addend1, addend2};
    for (int i = 0; i < 3; ++i)
        out[i] = (float)((((double)T[i] * (double)v[0] + (double)T[4 + i] * (double)v[1]) + (double)T[8 + i] * (double)v[2]) + add[i]);
}

__host__ __device__ inline double tri_dot3(const float a[3], const float b[3])
{
    return ((double)a[0] * (double)b[0] + (double)a[1] * (double)b[1]) + (double)a[2] * (double)b[2];
}

// cos(2 * atan2(mb / 2, depth)) through the float overloads (:316, :318)
__host__ __device__ inline float tri_cos_stereo(float mb, float depth)
{
    const float a = (float)atan2((double)(mb / 2), (double)depth);
    return (float)cos((double)(2 * a));
}

// :295-353 up to the choice of how x3D is obtained.  xn = (xn1.x, xn1.y, xn2.x, xn2.y).
__host__ __device__ inline int tri_front(const TriKf &K1, const TriKf &K2, const TriObs &o1, const TriObs &o2, float xn[4])
{
    const bool bStereo1 = o1.ur >= 0, bStereo2 = o2.ur >= 0;
    const float invfx1 = 1.0f / K1.fx, invfy1 = 1.0f / K1.fy, invfx2 = 1.0f / K2.fx, invfy2 = 1.0f / K2.fy;
    xn[0] = (o1.ux - K1.cx) * invfx1;
    xn[1] = (o1.uy - K1.cy) * invfy1;
    xn[2] = (o2.ux - K2.cx) * invfx2;
    xn[3] = (o2.uy - K2.cy) * invfy2;
    const float x1[3] = {xn[0], xn[1], 1.0f}, x2[3] = {xn[2], xn[3], 1.0f};
    float ray1[3], ray2[3];
    tri_rot_wc(K1.T, x1, 0.0, 0.0, 0.0, ray1);
    tri_rot_wc(K2.T, x2, 0.0, 0.0, 0.0, ray2);
    const double n1 = sqrt(tri_dot3(ray1, ray1)), n2 = sqrt(tri_dot3(ray2, ray2));
    const float cosParallaxRays = (float)(tri_dot3(ray1, ray2) / (n1 * n2));
    const float cosParallaxStereo0 = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo0, cosParallaxStereo2 = cosParallaxStereo0;
    if (bStereo1) cosParallaxStereo1 = tri_cos_stereo(K1.mb, o1.depth);
    else if (bStereo2) cosParallaxStereo2 = tri_cos_stereo(K2.mb, o2.depth);
    const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998))
        return TRI_BRANCH_SVD;
    // (UnprojectStereo with mvDepth <= 0 returns an empty Mat: no point)
    if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) return o1.depth > 0 ? TRI_BRANCH_STEREO1 : TRI_BRANCH_NONE;
    if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) return o2.depth > 0 ? TRI_BRANCH_STEREO2 : TRI_BRANCH_NONE;
    return TRI_BRANCH_NONE;
}

// one Jacobi rotation of the rows (x, y) of At and (vx, vy) of V, W re-accumulated from the new rows
__host__ __device__ inline bool tri_jacobi_pair(float x[4], float y[4], float vx[4], float vy[4], double &Wi, double &Wj)
{
    double a = Wi, b = Wj, p = 0;
    for (int k = 0; k < 4; ++k) p += (double)x[k] * (double)y[k];
    const double eps = (double)(FLT_EPSILON * 2);
    if (fabs(p) <= eps * sqrt(a * b)) return false;
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
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * x[k] + s * y[k];
        const float t1 = -s * x[k] + c * y[k];
        x[k] = t0;
        y[k] = t1;
        a += (double)t0 * (double)t0;
        b += (double)t1 * (double)t1;
    }
    Wi = a;
    Wj = b;
    for (int k = 0; k < 4; ++k) {
        const float t0 = c * vx[k] + s * vy[k];
        const float t1 = -s * vx[k] + c * vy[k];
        vx[k] = t0;
        vy[k] = t1;
    }
    return true;
}

// the selection sort's step for position i: the row j > i with the first largest W (strict `W[j] < W[k]`) changes places with row i
__host__ __device__ inline void tri_swap_if(bool take, double &wa, double &wb, float va[4], float vb[4])
{
    if (take) {
        const double t = wa;
        wa = wb;
        wb = t;
        for (int k = 0; k < 4; ++k) {
            const float f = va[k];
            va[k] = vb[k];
            vb[k] = f;
        }
    }
}

// column k of A (:327-330): A.row(0) = xn1.x * Tcw1.row(2) - Tcw1.row(0), ...
__host__ __device__ inline void tri_column_of_A(const float *T1, const float *T2, const float xn[4], int k, float col[4])
{
    col[0] = xn[0] * T1[8 + k] - T1[k];
    col[1] = xn[1] * T1[8 + k] - T1[4 + k];
    col[2] = xn[2] * T2[8 + k] - T2[k];
    col[3] = xn[3] * T2[8 + k] - T2[4 + k];
}

// :326-335: A from the two projection rows of each keyframe, cv::SVD::compute(A, w, u, vt, MODIFY_A | FULL_UV), v = vt.row(3).
// Every row is a named array and every pair a call with fixed operands, so that nothing is indexed at run time.
__host__ __device__ inline void tri_svd_null(const TriKf &K1, const TriKf &K2, const float xn[4], float v[4])
{
    // At = A^T: row i of At is column i of A
    float a0[4], a1[4], a2[4], a3[4];
    tri_column_of_A(K1.T, K2.T, xn, 0, a0);
    tri_column_of_A(K1.T, K2.T, xn, 1, a1);
    tri_column_of_A(K1.T, K2.T, xn, 2, a2);
    tri_column_of_A(K1.T, K2.T, xn, 3, a3);
    float v0[4] = {1, 0, 0, 0}, v1[4] = {0, 1, 0, 0}, v2[4] = {0, 0, 1, 0}, v3[4] = {0, 0, 0, 1};
    double W0 = 0, W1 = 0, W2 = 0, W3 = 0;
    for (int k = 0; k < 4; ++k) {
        W0 += (double)a0[k] * (double)a0[k];
        W1 += (double)a1[k] * (double)a1[k];
        W2 += (double)a2[k] * (double)a2[k];
        W3 += (double)a3[k] * (double)a3[k];
    }
    for (int iter = 0; iter < 30; ++iter) {
        bool changed = false;
        changed |= tri_jacobi_pair(a0, a1, v0, v1, W0, W1);
        changed |= tri_jacobi_pair(a0, a2, v0, v2, W0, W2);
        changed |= tri_jacobi_pair(a0, a3, v0, v3, W0, W3);
        changed |= tri_jacobi_pair(a1, a2, v1, v2, W1, W2);
        changed |= tri_jacobi_pair(a1, a3, v1, v3, W1, W3);
        changed |= tri_jacobi_pair(a2, a3, v2, v3, W2, W3);
        if (!changed) break;
    }
    W0 = W1 = W2 = W3 = 0;
    for (int k = 0; k < 4; ++k) {
        W0 += (double)a0[k] * (double)a0[k];
        W1 += (double)a1[k] * (double)a1[k];
        W2 += (double)a2[k] * (double)a2[k];
        W3 += (double)a3[k] * (double)a3[k];
    }
    W0 = sqrt(W0); W1 = sqrt(W1); W2 = sqrt(W2); W3 = sqrt(W3);
    {   // i = 0
        int j = 0;
        double wj = W0;
        if (wj < W1) { j = 1; wj = W1; }
        if (wj < W2) { j = 2; wj = W2; }
        if (wj < W3) { j = 3; wj = W3; }
        tri_swap_if(j == 1, W0, W1, v0, v1);
        tri_swap_if(j == 2, W0, W2, v0, v2);
        tri_swap_if(j == 3, W0, W3, v0, v3);
    }
    {   // i = 1
        int j = 1;
        double wj = W1;
        if (wj < W2) { j = 2; wj = W2; }
        if (wj < W3) { j = 3; wj = W3; }
        tri_swap_if(j == 2, W1, W2, v1, v2);
        tri_swap_if(j == 3, W1, W3, v1, v3);
    }
    tri_swap_if(W2 < W3, W2, W3, v2, v3);   // i = 2
    for (int k = 0; k < 4; ++k) v[k] = v3[k];
}

// KeyFrame::UnprojectStereo(i) (src/KeyFrame.cc:676-692) for z > 0: Twc.R * x3Dc + Twc.t with Twc.t = Ow
__host__ __device__ inline void tri_unproject(const TriKf &K, const TriObs &o, float x3D[3])
{
    const float invfx = 1.0f / K.fx, invfy = 1.0f / K.fy;
    const float z = o.depth;
    const float xc[3] = {(o.kx - K.cx) * z * invfx, (o.ky - K.cy) * z * invfy, z};
    float Ow[3];
    tri_center(K.T, Ow);
    tri_rot_wc(K.T, xc, (double)Ow[0], (double)Ow[1], (double)Ow[2], x3D);
}

// row r of [Rcw | tcw] applied to x3D: Rcw.row(r).dot(x3Dt) + tcw.at<float>(r)
__host__ __device__ inline float tri_cam_coord(const float *T, int r, const float x3D[3])
{
    return (float)(tri_dot3(T + 4 * r, x3D) + (double)T[4 * r + 3]);
}

// the reprojection gate of one keyframe (:366-391, :393-417); mbf is mpCurrentKeyFrame's in BOTH keyframes (:384, :410)
__host__ __device__ inline bool tri_reproj_ok(const TriKf &K, const TriObs &o, float mbf, float x, float y, float z)
{
    const float sf = K.sf[o.octave];
    const float sigmaSquare = sf * sf;   // mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i] (ORBextractor.cc:420)
    const float invz = (float)(1.0 / (double)z);
    const float u = K.fx * x * invz + K.cx;
    const float v = K.fy * y * invz + K.cy;
    const float errX = u - o.ux, errY = v - o.uy;
    if (!(o.ur >= 0)) return !((double)(errX * errX + errY * errY) > 5.991 * (double)sigmaSquare);
    const float u_r = u - mbf * invz;
    const float errX_r = u_r - o.ur;
    return !((double)(errX * errX + errY * errY + errX_r * errX_r) > 7.8 * (double)sigmaSquare);
}

// :355-436 on a point in hand: AOS2_TRI_ACCEPTED or the gate that rejected it
__host__ __device__ inline int tri_gates(const TriKf &K1, const TriKf &K2, const TriObs &o1, const TriObs &o2, const float x3D[3])
{
    const float z1 = tri_cam_coord(K1.T, 2, x3D);
    if (z1 <= 0) return AOS2_TRI_DEPTH1;
    const float z2 = tri_cam_coord(K2.T, 2, x3D);
    if (z2 <= 0) return AOS2_TRI_DEPTH2;
    if (!tri_reproj_ok(K1, o1, K1.mbf, tri_cam_coord(K1.T, 0, x3D), tri_cam_coord(K1.T, 1, x3D), z1)) return AOS2_TRI_REPROJ1;
    if (!tri_reproj_ok(K2, o2, K1.mbf, tri_cam_coord(K2.T, 0, x3D), tri_cam_coord(K2.T, 1, x3D), z2)) return AOS2_TRI_REPROJ2;
    float Ow1[3], Ow2[3];
    tri_center(K1.T, Ow1);
    tri_center(K2.T, Ow2);
    const float nrm1[3] = {x3D[0] - Ow1[0], x3D[1] - Ow1[1], x3D[2] - Ow1[2]};
    const float nrm2[3] = {x3D[0] - Ow2[0], x3D[1] - Ow2[1], x3D[2] - Ow2[2]};
    const float dist1 = (float)sqrt(tri_dot3(nrm1, nrm1)), dist2 = (float)sqrt(tri_dot3(nrm2, nrm2));
    if (dist1 == 0 || dist2 == 0) return AOS2_TRI_ZERO_DIST;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = K1.sf[o1.octave] / K2.sf[o2.octave];
    const float ratioFactor = 1.5f * K1.sf[1];   // 1.5f * mpCurrentKeyFrame->mfScaleFactor (:236)
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) return AOS2_TRI_SCALE;
    return AOS2_TRI_ACCEPTED;
}

// vt.row(3) -> Euclidean coordinates (:337-341); false: x3D.at<float>(3) == 0
__host__ __device__ inline bool tri_dehomogenize(const float v[4], float x3D[3])
{
    if (v[3] == 0) return false;
    const float r = (float)(1.0 / (double)v[3]);
    for (int k = 0; k < 3; ++k) x3D[k] = v[k] * r;
    return true;
}

// the whole body for one matched pair: status, and x3D where the status is not NO_MATCH / LOW_PARALLAX / W_ZERO (zeros there)
__host__ __device__ inline int triangulate_pair(const TriKf &K1, const TriKf &K2, const TriObs &o1, const TriObs &o2, float x3D[3])
{
    x3D[0] = x3D[1] = x3D[2] = 0.0f;
    float xn[4];
    const int branch = tri_front(K1, K2, o1, o2, xn);
    if (branch == TRI_BRANCH_NONE) return AOS2_TRI_LOW_PARALLAX;
    if (branch == TRI_BRANCH_SVD) {
        float v[4];
        tri_svd_null(K1, K2, xn, v);
        if (!tri_dehomogenize(v, x3D)) return AOS2_TRI_W_ZERO;
    } else {
        tri_unproject(branch == TRI_BRANCH_STEREO1 ? K1 : K2, branch == TRI_BRANCH_STEREO1 ? o1 : o2, x3D);
    }
    return tri_gates(K1, K2, o1, o2, x3D);
}

// ---- device only: the workgroup form the kernels of triangulate.hip and frames_keyframe.hip run

// number of set bits of a ballot below this lane (v_mbcnt_lo + v_mbcnt_hi)
__device__ __forceinline__ int tri_lanes_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// One matched pair per thread of a 256-thread workgroup whose threads share (K1, K2); every thread of the workgroup calls it.
// The cheap part (rays, parallax, the choice of branch) runs where the match is.  Typically under a tenth of a keyframe's features
// are matched, and the Jacobi SVD is a few thousand f64 instructions: under the divergent `if` most lanes of all four waves would
// idle through it.  So the items that need it are compacted per workgroup (ballot + mbcnt, their xn in LDS), the first `total`
// threads run the SVD on dense lanes -- the sweep loop of a wave ends when none of its lanes rotated; a sweep on a converged lane
// changes nothing, so a lane's result does not depend on its neighbours -- and every item picks its vt.row(3) up again.
__device__ __forceinline__ int tri_block(bool matched, const TriKf &K1, const TriKf &K2, const TriObs &o1, const TriObs &o2, float x3D[3])
{
    __shared__ float s_v[4][256];
    __shared__ int s_wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float xn[4] = {0.f, 0.f, 0.f, 0.f};
    int branch = TRI_BRANCH_NONE;
    if (matched) branch = tri_front(K1, K2, o1, o2, xn);
    const bool need = branch == TRI_BRANCH_SVD;
    const unsigned long long bal = __ballot(need);
    if (lane == 0) s_wcnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = s_wcnt[w];
        if (w < wave) base += c;
        total += c;
    }
    const int slot = base + tri_lanes_below(bal);   // < 256: at most one item per thread
    if (need) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_v[k][slot] = xn[k];
    }
    __syncthreads();
    if (tid < total) {
        float in[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) in[k] = s_v[k][tid];
        tri_svd_null(K1, K2, in, v);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_v[k][tid] = v[k];
    }
    __syncthreads();
    x3D[0] = x3D[1] = x3D[2] = 0.0f;
    if (!matched) return AOS2_TRI_NO_MATCH;
    if (branch == TRI_BRANCH_NONE) return AOS2_TRI_LOW_PARALLAX;
    if (need) {
        const float v[4] = {s_v[0][slot], s_v[1][slot], s_v[2][slot], s_v[3][slot]};
        if (!tri_dehomogenize(v, x3D)) return AOS2_TRI_W_ZERO;
    } else if (branch == TRI_BRANCH_STEREO1) {
        tri_unproject(K1, o1, x3D);
    } else {
        tri_unproject(K2, o2, x3D);
    }
    return tri_gates(K1, K2, o1, o2, x3D);
}

}  // namespace aos2
