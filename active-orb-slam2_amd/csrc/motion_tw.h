// The arithmetic of the planner's motion checks -- StateValidChecker::GetShortestPath (src/StateValidChecker.cc:313-367) over
// twb_shortpath / twb_gettangent / twb_getangle (:370-518), myprop (:296-311), the state loop of checkMotionTW / reconstructMotionTW /
// MotionCost (:244-294, :543-578), MotionCostLength (:522-529), isValid (:97-119) and collisionDetection::check_collisions
// (src/collisions.cc:70-94) -- that the device kernels (csrc/motion_tw.hip), the host taps (aos2_debug_svc_*_host,
// csrc/debug_taps.hip) and, restated in Python, the tests (tests/motion_tw_ref.py) share.  ONE routine set: every expression is
// written with the reference's association, both translation units are built with -ffp-contract=off, and `/` and sqrt are the
// correctly rounded ones.
//
// The reference calls libm's sin, cos and atan2, whose last bit depends on the glibc version, and the device's math library
// differs again.  Here they are tw_sin / tw_cos / tw_atan2: fixed sequences of IEEE double + - * / (the precedent is
// csrc/sincos_exact.h), so all three sides agree bit for bit; tests pin them against libm within 1 ulp on a dense sample.
//
// INPUT DOMAIN: every component of a state is finite and |theta| <= 1e4 (tw_state_ok; the calls answer AOS2_ERR_ARG otherwise).
// Why: the argument reduction subtracts k * PIO2_1 with k = floor(x * 2/pi + 0.5), and that product must stay EXACT.  PIO2_1 holds
// the first 33 bits of pi/2, so k may have 20 bits.  A heading inside a path is q1's or q2's plus w * t with |w| = 1 / turn_radius,
// and a segment has at most AOS2_SVC_MAX_SEGMENT_STATES states: with the planner's constants that keeps k far below 2^20.
// Outside the domain the routines are still the same sequence on every side, only no longer within an ulp of libm.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/aos2.h"
#include "sincos_exact.h"   // AOS2_HD

namespace aos2 {

// ---------------------------------------------------------------------------------------------- math
// x = k * pi/2 + (r + y), |r| <= pi/4 (about), q = k mod 4.  Cody-Waite in two pieces: pi/2 = PIO2_1 + PIO2_1T (fdlibm's
// e_rem_pio2.c); k * PIO2_1 is exact (above), so t is, and y is the rounding error of r = t - w.  floor, not a cast: negative angles.
struct TwReduced {
    double r, y;
    int q;
};
AOS2_HD TwReduced tw_reduce(double x)
{
    const double fk = floor(x * 6.36619772367581382433e-01 + 0.5);
    TwReduced R;
    if (!(fabs(fk) < 4503599627370496.0)) {   // infinite, NaN, or beyond 2^52 quarter turns: x - x (NaN, or 0)
        R.r = x - x;
        R.y = 0.0;
        R.q = 0;
        return R;
    }
    const double t = x - fk * 1.57079632673412561417e+00;
    const double w = fk * 6.07710050650619224932e-11;
    R.r = t - w;
    R.y = (t - R.r) - w;
    R.q = (int)(fk - 4.0 * floor(fk * 0.25));
    return R;
}
// fdlibm k_sin.c (iy = 1) and k_cos.c (the form without the bit-pattern branch), coefficients on [-pi/4, pi/4]
AOS2_HD double tw_kernel_sin(double x, double y)
{
    const double z = x * x;
    const double v = z * x;
    const double r = 8.33333333332248946124e-03 +
                     z * (-1.98412698298579493134e-04 +
                          z * (2.75573137070700676789e-06 + z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    return x - ((z * (0.5 * y - v * r) - y) - v * -1.66666666666666324348e-01);
}
AOS2_HD double tw_kernel_cos(double x, double y)
{
    const double z = x * x;
    double w = z * z;
    const double r = z * (4.16666666666666019037e-02 + z * (-1.38888888888741095749e-03 + z * 2.48015872894767294178e-05)) +
                     (w * w) * (-2.75573143513906633035e-07 + z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11));
    const double hz = 0.5 * z;
    w = 1.0 - hz;
    return w + (((1.0 - w) - hz) + (z * r - x * y));
}
AOS2_HD double tw_sin(double x)
{
    const TwReduced R = tw_reduce(x);
    switch (R.q) {
        case 0: return tw_kernel_sin(R.r, R.y);
        case 1: return tw_kernel_cos(R.r, R.y);
        case 2: return -tw_kernel_sin(R.r, R.y);
        default: return -tw_kernel_cos(R.r, R.y);
    }
}
AOS2_HD double tw_cos(double x)
{
    const TwReduced R = tw_reduce(x);
    switch (R.q) {
        case 0: return tw_kernel_cos(R.r, R.y);
        case 1: return -tw_kernel_sin(R.r, R.y);
        case 2: return -tw_kernel_cos(R.r, R.y);
        default: return tw_kernel_sin(R.r, R.y);
    }
}
// fdlibm s_atan.c for x >= 0 (the caller carries the sign); NaN stays NaN
AOS2_HD double tw_atan_pos(double x)
{
    double hi, lo;
    int id;
    if (x != x) return x;
    if (x >= 0x1p66) return 1.57079632679489655800e+00 + 6.12323399573676603587e-17;
    if (x < 0.4375) {
        if (x < 0x1p-29) return x;
        id = -1;
        hi = lo = 0.0;
    } else if (x < 1.1875) {
        if (x < 0.6875) {
            id = 0; hi = 4.63647609000806093515e-01; lo = 2.26987774529616870924e-17;
            x = (2.0 * x - 1.0) / (2.0 + x);
        } else {
            id = 1; hi = 7.85398163397448278999e-01; lo = 3.06161699786838301793e-17;
            x = (x - 1.0) / (x + 1.0);
        }
    } else if (x < 2.4375) {
        id = 2; hi = 9.82793723247329054082e-01; lo = 1.39033110312309984516e-17;
        x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
        id = 3; hi = 1.57079632679489655800e+00; lo = 6.12323399573676603587e-17;
        x = -1.0 / x;
    }
    const double z = x * x;
    const double w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 +
                           w * (1.42857142725034663711e-01 +
                                w * (9.09088713343650656196e-02 +
                                     w * (6.66107313738753120669e-02 + w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 +
                           w * (-1.11111104054623557880e-01 +
                                w * (-7.69187620504482999495e-02 + w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    if (id < 0) return x - x * (s1 + s2);
    return hi - ((x * (s1 + s2) - lo) - x);
}
// fdlibm e_atan2.c without its exponent-difference shortcuts (the division and tw_atan_pos give those cases within an ulp too).
// Two infinite arguments give NaN here (inf / inf), where libm gives a multiple of pi/4: no state of the domain produces them.
AOS2_HD double tw_atan2(double y, double x)
{
    const double pi = 3.1415926535897931160e+00, pi_lo = 1.2246467991473531772e-16;
    if (x != x || y != y) return x + y;
    const bool yneg = std::signbit(y), xneg = std::signbit(x);
    if (y == 0.0) return xneg ? (yneg ? -pi : pi) : y;
    if (x == 0.0) return yneg ? -1.5707963267948965580e+00 : 1.5707963267948965580e+00;
    const double z = tw_atan_pos(fabs(y / x));
    if (!xneg) return yneg ? -z : z;
    return yneg ? (z - pi_lo) - pi : pi - (z - pi_lo);
}

// ---------------------------------------------------------------------------------------------- the reference's functions
#define AOS2_TW_PI 3.1416   // QUIRK kept: `#define PI 3.1416` include/StateValidChecker.h:26 is what the +-2*PI wraps of :401-410 use

AOS2_HD bool tw_state_ok(const double *q) { return std::isfinite(q[0]) && std::isfinite(q[1]) && fabs(q[2]) <= 1e4; }

// normDistance (:205-213): sum = 0; sum += (a1[i]-a2[i])*(a1[i]-a2[i]) for i < d; sqrt(sum)
AOS2_HD double tw_norm_distance(const double *a1, const double *a2, int d)
{
    double sum = 0;
    for (int i = 0; i < d; ++i) sum += (a1[i] - a2[i]) * (a1[i] - a2[i]);
    return sqrt(sum);
}

// twb_getangle (:514-518)
AOS2_HD double tw_getangle(const double *q1, const double *q2) { return tw_atan2(q2[1] - q1[1], q2[0] - q1[0]); }

struct TwTangent {
    bool valid;
    double qt1[2], qt2[2];
    double d1mid2[3];
};

// twb_gettangent (:420-512): q1, q2 the centres of two circles of radius r, s1, s2 their orientations
AOS2_HD void tw_gettangent(const double *q1, int s1, const double *q2, int s2, double turn_radius, TwTangent &twt)
{
    if (s1 == s2) {
        const double ux = q2[0] - q1[0];
        const double uy = q2[1] - q1[1];
        const double norm_u = sqrt(ux * ux + uy * uy);
        if (s1 == 1) {   // :434-449
            twt.qt1[0] = q1[0] + turn_radius * uy / norm_u;
            twt.qt1[1] = q1[1] - turn_radius * ux / norm_u;
            twt.qt2[0] = q2[0] + turn_radius * uy / norm_u;
            twt.qt2[1] = q2[1] - turn_radius * ux / norm_u;
        } else {         // :450-465
            twt.qt1[0] = q1[0] - turn_radius * uy / norm_u;
            twt.qt1[1] = q1[1] + turn_radius * ux / norm_u;
            twt.qt2[0] = q2[0] - turn_radius * uy / norm_u;
            twt.qt2[1] = q2[1] + turn_radius * ux / norm_u;
        }
        return;
    }
    // QUIRK kept: "qmid" is half the DIFFERENCE of the centres (:468 "Should it be (+) instead of (-) ???"), i.e. the vector from
    // centre 1 to the midpoint
    double qmid_x = (q2[0] - q1[0]) / 2;
    double qmid_y = (q2[1] - q1[1]) / 2;
    const double L = sqrt(qmid_x * qmid_x + qmid_y * qmid_y);
    const double x = (turn_radius * turn_radius) / L;
    const double y = (turn_radius / L) * sqrt((L * L) - (turn_radius * turn_radius));
    qmid_x /= L;
    qmid_y /= L;
    if (s1 == 1) {       // :466-485
        twt.qt1[0] = q1[0] + x * qmid_x + y * qmid_y;
        twt.qt1[1] = q1[1] + x * qmid_y - y * qmid_x;
        twt.qt2[0] = q2[0] - x * qmid_x - y * qmid_y;
        twt.qt2[1] = q2[1] - x * qmid_y + y * qmid_x;
    } else {             // :486-505
        twt.qt1[0] = q1[0] + x * qmid_x - y * qmid_y;
        twt.qt1[1] = q1[1] + x * qmid_y + y * qmid_x;
        twt.qt2[0] = q2[0] - x * qmid_x + y * qmid_y;
        twt.qt2[1] = q2[1] - x * qmid_y - y * qmid_x;
    }
}

// twb_shortpath (:370-418).  (Its last two stores, twt.qt1[2] and twt.qt2[2] :413-414, write past vectors of size 2 and are read
// by nobody: they are not restated.)
AOS2_HD void tw_shortpath(const double *q1, int s1, const double *q2, int s2, int dir, double turn_radius, TwTangent &twt)
{
    double qc1[2], qc2[2];
    const double h1 = q1[2];
    const double h2 = q2[2];
    qc1[0] = q1[0] - turn_radius * s1 * tw_sin(h1);
    qc1[1] = q1[1] + turn_radius * s1 * tw_cos(h1);
    qc2[0] = q2[0] - turn_radius * s2 * tw_sin(h2);
    qc2[1] = q2[1] + turn_radius * s2 * tw_cos(h2);

    if (s1 * s2 < 0 && tw_norm_distance(qc1, qc2, 2) < 2 * turn_radius) {
        twt.valid = false;
        return;
    }
    tw_gettangent(qc1, dir * s1, qc2, dir * s2, turn_radius, twt);

    double delta1 = tw_getangle(qc1, twt.qt1) - tw_getangle(qc1, q1);
    if (dir * s1 > 0 && delta1 < 0)
        delta1 += 2 * AOS2_TW_PI;
    else if (dir * s1 < 0 && delta1 > 0)
        delta1 -= 2 * AOS2_TW_PI;

    double delta2 = tw_getangle(qc2, q2) - tw_getangle(qc2, twt.qt2);
    if (dir * s2 > 0 && delta2 < 0)
        delta2 += 2 * AOS2_TW_PI;
    else if (dir * s2 < 0 && delta2 > 0)
        delta2 -= 2 * AOS2_TW_PI;

    twt.d1mid2[0] = fabs(turn_radius * delta1);
    twt.d1mid2[1] = tw_norm_distance(twt.qt1, twt.qt2, 2);
    twt.d1mid2[2] = fabs(turn_radius * delta2);
    twt.valid = true;
}

// the candidates of GetShortestPath in the order of its loops (:337-339): s1cur outermost, then s2cur, then dircur, each -1 then 1
AOS2_HD void tw_candidate(int type, int &s1, int &s2, int &dir)
{
    s1 = (type & 4) ? 1 : -1;
    s2 = (type & 2) ? 1 : -1;
    dir = (type & 1) ? 1 : -1;
}
// the number a candidate is compared by (:342): twt.d1mid2[0]+twt.d1mid2[1]+twt.d1mid2[2]
AOS2_HD double tw_total(const double *t) { return t[0] + t[1] + t[2]; }
// QUIRK kept (:333, :342): the incumbent starts at d1 + dmid + d2 = 1e9 + 1e9 + 1e9 and a candidate replaces it only on strict <.
// So among equal totals the FIRST candidate stays, a NaN total never wins, and neither does a path of 3e9 or longer.  The
// incumbent's total is formed again from its three lengths at every comparison, by the same expression: the same number.
AOS2_HD bool tw_can_win(const TwTangent &twt) { return twt.valid && tw_total(twt.d1mid2) < 1e9 + 1e9 + 1e9; }

// myprop (:296-311).  QUIRK kept (:300): the branch is on wi being exactly zero (`if (wi)`).
AOS2_HD void tw_myprop(const double *q, double vi, double wi, double ti, double *out)
{
    const double h = q[2] + wi * ti;
    double x, y;
    if (wi != 0) {
        x = q[0] + ((vi / wi) * (tw_sin(h) - tw_sin(q[2])));
        y = q[1] - ((vi / wi) * (tw_cos(h) - tw_cos(q[2])));
    } else {
        x = q[0] + ti * vi * tw_cos(h);
        y = q[1] + ti * vi * tw_sin(h);
    }
    out[0] = x;
    out[1] = y;
    out[2] = h;
}

// What one motion is propagated from: vwt of GetShortestPath (:360-365) and, for each of its three segments, the loop constants
// of :259-263 -- int m = 1+ceil(t[i]/dt); double dd = t[i] / (m-1); q = Q.back() -- with q worked out for all three.
// QUIRK kept (:261-263): a segment's states are myprop(q, v, w, j*dd), j = 1 .. m-1, every one from the PREVIOUS SEGMENT'S LAST
// state q, not from the state before it.  t[i] == 0 gives m = 1: no state, and dd = 0 / 0 is never read.
struct TwPlan {
    int32_t valid, type, n_states, too_long;
    int32_t v;             // dir, as VectorInt v = {dir, dir, dir}
    int32_t m[3];
    double w[3], t[3], dd[3];
    double start[3][3];    // q of each segment
};
AOS2_HD void tw_plan_none(TwPlan &P)
{
    // QUIRK kept (:355-358 with :561-562): no path leaves vwt.v empty, so Q = {q1}
    P.valid = 0; P.type = -1; P.n_states = 1; P.too_long = 0; P.v = 0;
    for (int i = 0; i < 3; ++i) {
        P.m[i] = 0;
        P.w[i] = P.t[i] = P.dd[i] = 0.0;
        for (int k = 0; k < 3; ++k) P.start[i][k] = 0.0;
    }
}
AOS2_HD void tw_plan(const double *q1, int type, const double *t, double turn_radius, double dt, TwPlan &P)
{
    int s1, s2, dir;
    tw_candidate(type, s1, s2, dir);
    P.valid = 1; P.type = type; P.too_long = 0; P.v = dir;
    P.w[0] = s1 * dir / turn_radius;   // s1*vwt.v[0]/turn_radius :365: an int product, then the division
    P.w[1] = 0;
    P.w[2] = s2 * dir / turn_radius;
    P.n_states = 1;
    double q[3] = {q1[0], q1[1], q1[2]};
    for (int i = 0; i < 3; ++i) {
        P.t[i] = t[i];
        const double md = 1 + ceil(t[i] / dt);
        if (!(md <= (double)AOS2_SVC_MAX_SEGMENT_STATES + 1)) {   // (the reference's int conversion would overflow far later)
            P.too_long = 1;
            P.m[i] = 1;
            P.dd[i] = 0.0;
        } else {
            P.m[i] = (int)md;
            P.dd[i] = t[i] / (P.m[i] - 1);
        }
        for (int k = 0; k < 3; ++k) P.start[i][k] = q[k];
        if (P.m[i] > 1) {
            double last[3];
            tw_myprop(q, P.v, P.w[i], (P.m[i] - 1) * P.dd[i], last);
            for (int k = 0; k < 3; ++k) q[k] = last[k];
            P.n_states += P.m[i] - 1;
        }
    }
}
// state i of Q (i = 0 is q1)
AOS2_HD void tw_plan_state(const double *q1, const TwPlan &P, int i, double *out)
{
    if (i == 0) {
        out[0] = q1[0]; out[1] = q1[1]; out[2] = q1[2];
        return;
    }
    int s = 0, j = i;
    while (s < 2 && j > P.m[s] - 1) {
        j -= P.m[s] - 1;
        ++s;
    }
    tw_myprop(P.start[s], P.v, P.w[s], j * P.dd[s], out);
}

// GetShortestPath (:313-367) with the plan, serially: what the host tap runs
AOS2_HD void tw_shortest_path(const double *q1, const double *q2, double turn_radius, double dt, TwPlan &P)
{
    double d[3] = {1e9, 1e9, 1e9};
    int best = -1;
    for (int type = 0; type < 8; ++type) {
        int s1, s2, dir;
        tw_candidate(type, s1, s2, dir);
        TwTangent twt;
        tw_shortpath(q1, s1, q2, s2, dir, turn_radius, twt);
        if (twt.valid) {
            if (twt.d1mid2[0] + twt.d1mid2[1] + twt.d1mid2[2] < d[0] + d[1] + d[2]) {
                best = type;
                for (int k = 0; k < 3; ++k) d[k] = twt.d1mid2[k];
            }
        }
    }
    if (best < 0)
        tw_plan_none(P);
    else
        tw_plan(q1, best, d, turn_radius, dt, P);
}

// QUIRK kept (:255-268): checkMotionTW pushes q1 without testing it ("we assume that s1 is in the tree and therefore valid") and
// tests the states 1 .. size-1 in index order, returning at the first that isValid refuses.  MotionCost (:561-570) builds the
// same Q whatever isValid says, so both costs cover the whole path also when the motion is not valid.
// one term of MotionCostLength (:522-529): normDistance(Q[i-1], Q[i]).  QUIRK kept: d = -1 means all THREE components, so the
// heading difference is added to the planar ones.
AOS2_HD double tw_length_term(const double *a, const double *b) { return tw_norm_distance(a, b, 3); }

// check_collisions (src/collisions.cc:70-94), the part in front of the nearest-obstacle query.  -> 1 free, 0 not, -1 ask the query
// QUIRK kept (:73): no obstacle at all returns true BEFORE the bounds test.
// QUIRK kept (:77): `q[0] < MIN_X || q[1] > MAX_X || q[2] < MIN_Y || q[2] > MAX_Y` -- x has no upper and y no lower bound, y is
// compared with x's maximum, and it is the HEADING q[2] that is held against +-5 (a path's headings do leave that range).
AOS2_HD int tw_collision_gate(const double *q, int num_of_obs, const aos2_svc_params_t &p)
{
    if (num_of_obs == 0) return 1;
    if (q[0] < p.min_x || q[1] > p.max_x || q[2] < p.min_y || q[2] > p.max_y) return 0;
    return -1;
}
// the squared distance nanoflann's L2_Adaptor forms in dimension 2: result = 0; result += diff * diff per component
AOS2_HD double tw_obstacle_d2(const double *q, double ox, double oy)
{
    double result = 0;
    result += (q[0] - ox) * (q[0] - ox);
    result += (q[1] - oy) * (q[1] - oy);
    return result;
}
// :90 over kNeighbors' sqrt (:121): soln.dist[0] <= robot_radius + obs_r is a collision.  d2min: the minimum over all obstacles.
AOS2_HD bool tw_collision_free(double d2min, double robot_r, double obs_r) { return !(sqrt(d2min) <= robot_r + obs_r); }

// isValid (:97-119) from the two things it asks for.  QUIRK kept: IsStateVisiblilty is `count > threshold`; the heuristic branch
// (heuristicValidityCheck, off in every constructor) asks it only for states nearer to StartState than maxDistHeuristicValidity.
AOS2_HD bool tw_is_valid(const double *q, bool collision_free, int count, int thr, const aos2_svc_params_t &p)
{
    if (!collision_free) return false;
    if (!p.heuristic) return count > thr;
    if ((q[0] - p.start[0]) * (q[0] - p.start[0]) + (q[1] - p.start[1]) * (q[1] - p.start[1]) < p.max_dist_heuristic * p.max_dist_heuristic)
        return count > thr;
    return true;
}

// ---- host side, shared by csrc/motion_tw.hip and the host taps
struct SvcView {
    aos2_svc_params_t params;
    int n_obs = 0;
    const double *obs = nullptr;   // [n_obs][2]
    double obs_r = 0.1;
    aos2_vis_t *vis = nullptr;
    int thr = 0;                   // the threshold in force: params.feature_threshold, or the camera's
};
void svc_view(const aos2_svc_t *h, SvcView *v);
// the argument checks of the two calls (AOS2_ERR_ARG with the error text set); they run before a device is looked for
int svc_check_valid(const aos2_svc_t *h, int ns, const double *states, const uint8_t *valid);
int svc_check_motions(const aos2_svc_t *h, int nm, const double *q1, const double *q2, const aos2_svc_motions_out_t *out);

}  // namespace aos2
