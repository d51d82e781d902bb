// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:363-413) with compute_std_pts (:27-37) and the planner's map rows
// (src/Planning.cc:86-96, src/Tracking.cc:1088-1112) over the resident graph of aos2_local_map_*: what csrc/normal_depth.hip shares
// with the host tap aos2_debug_update_normal_depth_host (csrc/debug_taps.hip) -- the argument checks, the arithmetic of one
// observation, of one point's tail and of its planner row, and the serial loop itself, which is the tap.  ONE routine set under the
// rule of csrc/visibility.h: both translation units are built with -ffp-contract=off, every operation is written with its
// association, the divide and the square root are the correctly rounded ones, atan2 is the double function rounded to float.
// The kernel runs the per-observation function with a lane per observation and folds the sums in list order; the serial loop does
// the same on one core.  DESIGN.md section 2 item 21.  They read the graph through LmGraph (csrc/local_map_arrays.h), device or
// host addresses.  No HIP runtime calls: host C++ and kernels.  Internal to the library.
#pragma once
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/aos2.h"
#include "local_map_arrays.h"

#if defined(__HIPCC__)
#define AOS2_ND_HD __host__ __device__ __forceinline__
#else
#define AOS2_ND_HD inline
#endif

namespace aos2 {

// cv::norm of a 3x1 CV_32F matrix: the squares summed in double in index order, the square root in double
AOS2_ND_HD double nd_norm(float d0, float d1, float d2)
{
    const double s = ((double)d0 * (double)d0 + (double)d1 * (double)d1) + (double)d2 * (double)d2;
    return sqrt(s);
}

// :388-394 for one observer: normali / cv::norm(normali) (the entry of mNormalVectors, which is also what `normal` gains) and theta
// (the entry of theta_sVector)
struct NdTerm {
    float u[3], theta;
};
AOS2_ND_HD NdTerm nd_term(const float *P, const float *Owi)
{
    const float d0 = P[0] - Owi[0], d1 = P[1] - Owi[1], d2 = P[2] - Owi[2];
    const float inv = (float)(1.0 / nd_norm(d0, d1, d2));
    NdTerm t;
    t.u[0] = d0 * inv;
    t.u[1] = d1 * inv;
    t.u[2] = d2 * inv;
    t.theta = (float)atan2((double)d0, (double)d2);
    return t;
}

// :398-399  dist = cv::norm(Pos - pRefKF->GetCameraCenter()) as a float
AOS2_ND_HD float nd_dist(const float *P, const float *Oref) { return (float)nd_norm(P[0] - Oref[0], P[1] - Oref[1], P[2] - Oref[2]); }

// :400  pRefKF->mvKeysUn[observations[pRefKF]].octave: idx = the feature of the reference keyframe's own entry, 0 if it has none.
// -1: the reference keyframe has no such feature or the octave is no row of the scale table (the reference reads out of bounds)
AOS2_ND_HD int nd_ref_level(const LmGraph &G, int ref, int idx, int n_levels)
{
    const int f0 = G.kf_mp_off[ref];
    if (idx < 0 || idx >= G.kf_mp_off[ref + 1] - f0) return -1;
    const int level = G.kf_octave[f0 + idx];
    return level < 0 || level >= n_levels ? -1 : level;
}

// :406-408  n = the length of the list
AOS2_ND_HD float nd_normal_scale(int n) { return (float)(1.0 / (double)n); }
AOS2_ND_HD void nd_distances(float dist, float level_scale, float top_scale, float &max_dist, float &min_dist)
{
    max_dist = dist * level_scale;
    min_dist = max_dist / top_scale;
}

// compute_std_pts :29-36 around its two accumulations, which run in double over float operands (the 0.0 of accumulate and
// inner_product) and are rounded to float
AOS2_ND_HD float nd_mean(double sum, int n) { return (float)sum / (float)n; }
AOS2_ND_HD float nd_sq_term(float theta, float mean)
{
    const float diff = theta - mean;
    return diff * diff;
}
AOS2_ND_HD float nd_std(double sq_sum, int n) { return sqrtf((float)sq_sum / (float)n); }

// one row of the planner's map from a point's members
struct NdRows {
    float upper, lower, max_range, min_range;
};
AOS2_ND_HD NdRows nd_rows(int form, float mean, float stdev, float min_dist, float max_dist)
{
    NdRows r;
    r.max_range = 1.2f * max_dist;   // GetMaxDistanceInvariance
    r.min_range = 0.8f * min_dist;   // GetMinDistanceInvariance
    const double wide = (double)stdev * 2.5;
    if (form == AOS2_ND_ROWS_PLANNING) {   // theta_interval is a float member: the sums are float
        const float iv = wide < 30.0 / 57.3 ? (float)(30.0 / 57.3) : (float)wide;
        r.upper = mean + iv;
        r.lower = mean - iv;
    } else {   // a double local: the sums are double, rounded by the push_back's double(...) into the float row
        const double iv = wide < 10.0 / 57.3 ? 10.0 / 57.3 : wide;
        r.upper = (float)((double)mean + iv);
        r.lower = (float)((double)mean - iv);
    }
    return r;
}

// :371 and :378 and the table's edge: AOS2_ND_UPDATED stands for "goes on" (the reference keyframe is judged behind the loop);
// e0 / n = the point's observation row
AOS2_ND_HD int nd_point_gate(const LmGraph &G, int row, int &e0, int &n)
{
    e0 = n = 0;
    if (row >= G.n_points) return AOS2_ND_UNKNOWN;
    if (G.point_bad[row]) return AOS2_ND_BAD;
    e0 = G.obs_off[row];
    n = G.obs_off[row + 1] - e0;
    return n == 0 ? AOS2_ND_NO_OBS : AOS2_ND_UPDATED;
}

inline int nd_refuse(char *msg, size_t len, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
inline int nd_refuse(char *msg, size_t len, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, len, fmt, ap);
    va_end(ap);
    return 1;
}

// The checks of aos2_local_map_update_normal_depth on its own arguments against a graph of n_keyframes rows: 0, or 1 with the
// reason in msg.  The graph is not read.
inline int nd_check(const aos2_normal_depth_t &a, int n_keyframes, char *msg, size_t len)
{
    if (a.n < 0) return nd_refuse(msg, len, "n = %d is negative", a.n);
    if (a.n_levels < 1) return nd_refuse(msg, len, "n_levels = %d is below 1", a.n_levels);
    if (a.rows_form != AOS2_ND_ROWS_PLANNING && a.rows_form != AOS2_ND_ROWS_TRACKING)
        return nd_refuse(msg, len, "rows_form = %d is neither AOS2_ND_ROWS_PLANNING nor AOS2_ND_ROWS_TRACKING", a.rows_form);
    if (!a.scale) return nd_refuse(msg, len, "scale is NULL");
    if (n_keyframes > 0 && !a.kf_center) return nd_refuse(msg, len, "kf_center is NULL with %d keyframes", n_keyframes);
    if (a.n > 0 && (!a.point || !a.xyz || !a.ref_kf)) return nd_refuse(msg, len, "point, xyz or ref_kf is NULL");
    if ((a.term_unit || a.term_theta) && !a.term_off) return nd_refuse(msg, len, "term_unit or term_theta without term_off");
    if (a.term_off && a.term_off[0] != 0) return nd_refuse(msg, len, "term_off[0] = %d is not 0", a.term_off[0]);
    for (int i = 0; i < a.n; ++i) {
        if (a.point[i] < 0) return nd_refuse(msg, len, "point[%d] = %d is negative", i, a.point[i]);
        if (a.ref_kf[i] < 0 || a.ref_kf[i] >= n_keyframes)
            return nd_refuse(msg, len, "ref_kf[%d] = %d is outside [0, %d)", i, a.ref_kf[i], n_keyframes);
        if (a.term_off && a.term_off[i + 1] < a.term_off[i])
            return nd_refuse(msg, len, "term_off[%d] = %d is below term_off[%d] = %d", i + 1, a.term_off[i + 1], i, a.term_off[i]);
    }
    return 0;
}

// where the per-observation outputs of listed point i go: the offset, or -1 if the caller gave no room of exactly n entries
AOS2_ND_HD int nd_term_slot(const int32_t *term_off, int i, int n)
{
    return term_off && term_off[i + 1] - term_off[i] == n ? term_off[i] : -1;
}

// One point's results into the caller's arrays (those that are wanted), listed point i.  The device call runs it over what came
// back, the serial loop over what it has just computed.
struct NdPoint {
    float normal[3], min_dist, max_dist, theta_mean, theta_std;
    int32_t n_terms;
};
inline void nd_store(const aos2_normal_depth_t &a, int i, const NdPoint &p, const NdRows &r)
{
    if (a.normal)
        for (int c = 0; c < 3; ++c) a.normal[3 * (size_t)i + c] = p.normal[c];
    if (a.min_dist) a.min_dist[i] = p.min_dist;
    if (a.max_dist) a.max_dist[i] = p.max_dist;
    if (a.theta_mean) a.theta_mean[i] = p.theta_mean;
    if (a.theta_std) a.theta_std[i] = p.theta_std;
    if (a.n_terms) a.n_terms[i] = p.n_terms;
    if (a.upper) a.upper[i] = r.upper;
    if (a.lower) a.lower[i] = r.lower;
    if (a.max_range) a.max_range[i] = r.max_range;
    if (a.min_range) a.min_range[i] = r.min_range;
}

// The function as the reference runs it, one point and one observation at a time (the arguments have passed nd_check, the graph and
// the view their own checks).
inline void nd_host_run(const LmGraph &G, const aos2_normal_depth_t &a)
{
    std::vector<NdTerm> terms;
    for (int i = 0; i < a.n; ++i) {
        int e0, n;
        int st = nd_point_gate(G, a.point[i], e0, n);
        if (st == AOS2_ND_UPDATED) {
            const float *Pos = a.xyz + 3 * (size_t)i;
            const int pRefKF = a.ref_kf[i];
            terms.resize(n);
            float normal[3] = {0.0f, 0.0f, 0.0f};
            double sum = 0.0;
            int idx = 0;   // observations[pRefKF] of a keyframe that is not in the map
            for (int j = 0; j < n; ++j) {   // :385-396
                const int pKF = G.obs_kf[e0 + j];
                const NdTerm t = terms[j] = nd_term(Pos, a.kf_center + 3 * (size_t)pKF);
                for (int c = 0; c < 3; ++c) normal[c] = normal[c] + t.u[c];
                sum += (double)t.theta;
                if (pKF == pRefKF) idx = G.obs_idx[e0 + j];
            }
            const int level = nd_ref_level(G, pRefKF, idx, a.n_levels);
            if (level < 0) st = AOS2_ND_REF_UNUSABLE;
            else {
                NdPoint p;
                nd_distances(nd_dist(Pos, a.kf_center + 3 * (size_t)pRefKF), a.scale[level], a.scale[a.n_levels - 1], p.max_dist,
                             p.min_dist);
                const float k = nd_normal_scale(n);
                for (int c = 0; c < 3; ++c) p.normal[c] = normal[c] * k;
                p.theta_mean = nd_mean(sum, n);
                double sq_sum = 0.0;
                for (int j = 0; j < n; ++j) sq_sum += (double)nd_sq_term(terms[j].theta, p.theta_mean);
                p.theta_std = nd_std(sq_sum, n);
                p.n_terms = n;
                nd_store(a, i, p, nd_rows(a.rows_form, p.theta_mean, p.theta_std, p.min_dist, p.max_dist));
                const int slot = nd_term_slot(a.term_off, i, n);
                for (int j = 0; slot >= 0 && j < n; ++j) {
                    if (a.term_unit)
                        for (int c = 0; c < 3; ++c) a.term_unit[3 * (size_t)(slot + j) + c] = terms[j].u[c];
                    if (a.term_theta) a.term_theta[slot + j] = terms[j].theta;
                }
            }
        }
        if (a.status) a.status[i] = (uint8_t)st;
    }
}

}  // namespace aos2
