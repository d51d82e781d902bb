// The arithmetic of the planner's visibility count -- camera::countVisible (src/camera.cc:135-198) with camera::isInFrustum
// (:263-315), StateValidChecker::MotionCostCamera (src/StateValidChecker.cc:531-541) and camera::IsStateVisiblilty (:242-250) --
// that the device kernels (csrc/visibility.hip) and the host tap (aos2_debug_visibility_host, csrc/debug_taps.hip) share.  ONE
// routine set: both translation units are built with -ffp-contract=off, every float operation is written with its association,
// the divide and the square root are the correctly rounded ones, and cos / sin / atan2 are the double functions rounded to float
// (the rule of csrc/triangulate.h and initializer.h).  DESIGN.md section 2 item 16.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/aos2.h"

namespace aos2 {

// what a point is tested against: rows 0..2 of T_cs (the fourth coordinate of a map point is forced to 1, so row 3 is never
// read) and the two entries of T_sc that the viewing-direction test reads (:301-302)
struct VisState {
    float cs[12];
    float sc03, sc23;
    float pad[2];
};

// the camera's gate constants as the kernels take them
struct VisGates {
    float fx, fy, cx, cy, min_x, max_x, min_y, max_y, max_dist, min_dist;
};

__host__ __device__ inline VisGates vis_gates(const aos2_vis_camera_t &c)
{
    return VisGates{c.fx, c.fy, c.cx, c.cy, c.min_x, c.max_x, c.min_y, c.max_y, c.max_dist, c.min_dist};
}

// C = A * B, row-major 4x4: float products, float sums, ascending inner index
__host__ __device__ inline void vis_mul44(const float *A, const float *B, float *C)
{
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            float s = A[4 * i] * B[j];
            for (int k = 1; k < 4; ++k) s = s + A[4 * i + k] * B[4 * k + j];
            C[4 * i + j] = s;
        }
}

// rows 0..2 of the inverse of a general 4x4 (T_sc.inverse() :149 -- not the rigid shortcut): the cofactors from the twelve 2x2
// minors of the upper and the lower row pair, every entry times 1.0f / det.  The operation order is THIS one (parity unpinned:
// the association inside the reference's Eigen cannot be read here).
__host__ __device__ inline void vis_inverse_rows(const float *m, float *inv)
{
    const float s0 = m[0] * m[5] - m[4] * m[1], s1 = m[0] * m[6] - m[4] * m[2], s2 = m[0] * m[7] - m[4] * m[3];
    const float s3 = m[1] * m[6] - m[5] * m[2], s4 = m[1] * m[7] - m[5] * m[3], s5 = m[2] * m[7] - m[6] * m[3];
    const float c5 = m[10] * m[15] - m[14] * m[11], c4 = m[9] * m[15] - m[13] * m[11], c3 = m[9] * m[14] - m[13] * m[10];
    const float c2 = m[8] * m[15] - m[12] * m[11], c1 = m[8] * m[14] - m[12] * m[10], c0 = m[8] * m[13] - m[12] * m[9];
    const float det = ((((s0 * c5 - s1 * c4) + s2 * c3) + s3 * c2) - s4 * c1) + s5 * c0;
    const float r = 1.0f / det;
    inv[0] = ((m[5] * c5 - m[6] * c4) + m[7] * c3) * r;
    inv[1] = ((m[2] * c4 - m[1] * c5) - m[3] * c3) * r;
    inv[2] = ((m[13] * s5 - m[14] * s4) + m[15] * s3) * r;
    inv[3] = ((m[10] * s4 - m[9] * s5) - m[11] * s3) * r;
    inv[4] = ((m[6] * c2 - m[4] * c5) - m[7] * c1) * r;
    inv[5] = ((m[0] * c5 - m[2] * c2) + m[3] * c1) * r;
    inv[6] = ((m[14] * s2 - m[12] * s5) - m[15] * s1) * r;
    inv[7] = ((m[8] * s5 - m[10] * s2) + m[11] * s1) * r;
    inv[8] = ((m[4] * c4 - m[5] * c2) + m[7] * c0) * r;
    inv[9] = ((m[1] * c2 - m[0] * c4) - m[3] * c0) * r;
    inv[10] = ((m[12] * s4 - m[13] * s2) + m[15] * s0) * r;
    inv[11] = ((m[9] * s2 - m[8] * s4) - m[11] * s0) * r;
}

// Eigen::Matrix4f T_sc = T_sw * T_wb * T_bc; T_cs = T_sc.inverse() (:148-149 / :180-181), T_wb as the cv::Mat overload gets it
__host__ __device__ inline VisState vis_state_from_pose(const float *T_wb, const aos2_vis_camera_t &cam)
{
    float a[16], sc[16];
    vis_mul44(cam.T_sw, T_wb, a);
    vis_mul44(a, cam.T_bc, sc);
    VisState S;
    vis_inverse_rows(sc, S.cs);
    S.sc03 = sc[3];
    S.sc23 = sc[11];
    S.pad[0] = S.pad[1] = 0.0f;
    return S;
}

// T_wb of a planar state (:142-146): (float)cos(theta) with the double cos, the float overloads being the double functions rounded
__host__ __device__ inline VisState vis_state_from_xyt(float x, float y, float theta, const aos2_vis_camera_t &cam)
{
    const float c = (float)cos((double)theta), s = (float)sin((double)theta);
    const float T_wb[16] = {c, -s, 0.0f, x, s, c, 0.0f, y, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
    return vis_state_from_pose(T_wb, cam);
}

// one row of T_cs times the point with its fourth coordinate forced to 1 (:266-268)
__host__ __device__ inline float vis_row(const float *a, float x, float y, float z) { return ((a[0] * x + a[1] * y) + a[2] * z) + a[3]; }

// isInFrustum (:263-315) up to the viewing-direction test: everything but the atan2.  -> whether the point is still in
__host__ __device__ inline bool vis_point_window(const VisGates &g, const VisState &S, float x, float y, float z, float max_range,
                                                 float min_range)
{
    const float PcZ = vis_row(S.cs + 8, x, y, z);
    if (PcZ < 0.05f) return false;                                  // step 1 (:277)
    const float PcX = vis_row(S.cs, x, y, z), PcY = vis_row(S.cs + 4, x, y, z);
    const float inv_z = 1.0f / PcZ;
    const float u = (g.fx * PcX) * inv_z + g.cx, v = (g.fy * PcY) * inv_z + g.cy;
    if (u < g.min_x || u > g.max_x) return false;                   // step 2 (:285-289)
    if (v < g.min_y || v > g.max_y) return false;
    const float dist = sqrtf((PcZ * PcZ + PcY * PcY) + PcX * PcX);
    if (dist < g.min_dist || dist > g.max_dist) return false;       // step 3 (:293-297)
    if (dist < min_range || dist > max_range) return false;
    return true;
}

// step 4 (:301-306), evaluated only for a point that passed everything before it
__host__ __device__ inline bool vis_point_direction(const VisState &S, float x, float z, float upper, float lower)
{
    const float delta_x_s = x - S.sc03, delta_z_s = z - S.sc23;
    const float theta_robot_s = (float)atan2((double)delta_x_s, (double)delta_z_s);
    return !(theta_robot_s < lower || theta_robot_s > upper);
}

__host__ __device__ inline bool vis_point(const VisGates &g, const VisState &S, float x, float y, float z, float upper, float lower,
                                          float max_range, float min_range)
{
    return vis_point_window(g, S, x, y, z, max_range, min_range) && vis_point_direction(S, x, z, upper, lower);
}

// int(round(num_visible)) (:166): std::round(float), half away from zero -- not rintf.  Out of int's range (and NaN): what the
// x86 conversion gives, INT32_MIN.
__host__ __device__ inline int32_t vis_round(float sum)
{
    const float r = roundf(sum);
    return (r >= -2147483648.0f && r < 2147483648.0f) ? (int32_t)r : INT32_MIN;
}

// one term of MotionCostCamera (src/StateValidChecker.cc:538); c == 0 with thr <= 0 gives inf, as there
__host__ __device__ inline double vis_motion_cost_term(int c, int thr) { return c < thr ? 1. / 1e-4 : 1. / (double)c; }

// ---- host side, shared by csrc/visibility.hip and the host tap: the handle's camera and the host copy of its map
struct VisMapView {
    int n = 0;
    const float *x = nullptr, *y = nullptr, *z = nullptr, *upper = nullptr, *lower = nullptr, *max_range = nullptr, *min_range = nullptr,
                *ratio = nullptr;
};
void vis_view(const aos2_vis_t *h, aos2_vis_camera_t *cam, VisMapView *map);
// the argument checks of the four calls (AOS2_ERR_ARG with the error text set); they run before a device is looked for
int vis_check_count(const aos2_vis_t *h, int ns, const float *states, const int32_t *count);
int vis_check_motions(const aos2_vis_t *h, int nm, const int32_t *offsets, const float *states, const double *cost);
int vis_check_advance(const aos2_vis_t *h, int ns, const float *states, const int32_t *index);
// the interior states (i = 1 .. size-2) of every motion, packed, with their offsets [nm + 1]
void vis_interior(int nm, const int32_t *offsets, const float *states, std::vector<float> &packed, std::vector<int32_t> &packed_off);
#if defined(__HIPCC__)
// For the library's other device paths (csrc/motion_tw.hip): countVisible of ns float states [ns][3] that are ON THE DEVICE, enqueued
// on the caller's stream s (the map goes up on s too if it changed) with no wait.  *count: the handle's device array of the ns
// counts, good until the handle's next call.  ns >= 1.  The caller's stream is the only one that may touch the handle meanwhile.
int vis_counts_on_device(aos2_vis_t *h, int ns, const float *d_states, hipStream_t s, const int32_t **count);
#endif

}  // namespace aos2
