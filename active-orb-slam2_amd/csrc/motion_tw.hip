// The planner's motion checks (StateValidChecker::checkMotionTW / reconstructMotionTW / MotionCost / isValid,
// src/StateValidChecker.cc:97-119, :244-367, :522-578, over collisionDetection::check_collisions src/collisions.cc:70-94) on the
// device, for a batch of (q1, q2) pairs in one call.  The arithmetic is csrc/motion_tw.h, shared with the host taps; the result
// equals the serial loops bit for bit.  DESIGN.md section 5.12.
//   k_tw_paths    eight lanes per motion, one per candidate (s1, s2, dir); the winner by a butterfly over the lane group that keeps
//                 the serial rule (smallest total, lowest candidate among equals, NaN never); the winning lane forms the plan
//   k_tw_scan     one workgroup: the exclusive scan of the motions' state counts; the total is read back ONCE (the call's only
//                 host wait before the results) to size what follows
//   k_tw_states   a lane per state: myprop from its segment's start state, the double state and its float narrowing
//   k_tw_collide  a workgroup per tile of states: the obstacles, resident in HBM, staged through LDS; bounds quirk and nearest obstacle
//   (visibility)  k_vis_setup / k_vis_gate / k_vis_fold of csrc/visibility.hip on the float states (vis_counts_on_device)
//   k_tw_verdict  a wave per motion: the first invalid state from ballots, the two ordered double sums
#include <cmath>
#include <vector>

#include "aos2_common.h"
#include "motion_tw.h"
#include "visibility.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kNT = 256;
constexpr int kWaves = kNT / 64;
constexpr int kCollideStates = 64;     // states of a k_tw_collide workgroup: its four waves take every fourth obstacle each
constexpr int kObsTile = 1024;         // obstacles staged in LDS at a time (16 KiB)

// the better of two candidates of one motion by the serial rule: the smaller total, the lower index among equals.  A candidate
// that cannot win carries +inf.
__device__ __forceinline__ void tw_better(double &total, int &idx, double ot, int oi)
{
    if (ot < total || (ot == total && oi < idx)) {
        total = ot;
        idx = oi;
    }
}

__global__ __launch_bounds__(kNT) void k_tw_paths(const double *__restrict__ q1, const double *__restrict__ q2, int nm, double turn_radius,
                                                  double dt, TwPlan *__restrict__ plans)
{
    const int g = blockIdx.x * kNT + threadIdx.x;
    const int cand = g & 7;
    const int mo = g >> 3;
    const int m = min(mo, nm - 1);   // (a lane past the last motion works on the last one and stores nothing: the DPP steps need all lanes)
    double a[3], b[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = q1[3 * (size_t)m + k];
        b[k] = q2[3 * (size_t)m + k];
    }
    int s1, s2, dir;
    tw_candidate(cand, s1, s2, dir);
    TwTangent twt;
    tw_shortpath(a, s1, b, s2, dir, turn_radius, twt);
    double total = tw_can_win(twt) ? tw_total(twt.d1mid2) : INFINITY;
    int idx = cand;
    // lane ^ 1, lane ^ 2, then the other half of the eight (row_half_mirror: lane ^ 7): every lane ends with the same winner
    tw_better(total, idx, dpp_f64<0xB1>(total), dpp_i32<0xB1>(idx));
    tw_better(total, idx, dpp_f64<0x4E>(total), dpp_i32<0x4E>(idx));
    tw_better(total, idx, dpp_f64<0x141>(total), dpp_i32<0x141>(idx));
    if (mo >= nm) return;
    if (total == INFINITY) {
        if (cand == 0) tw_plan_none(plans[m]);
    } else if (idx == cand) {
        tw_plan(a, cand, twt.d1mid2, turn_radius, dt, plans[m]);
    }
}

// off [nm + 1]: the exclusive scan of n_states; info[0] = the total, info[1] = the first motion that is too long, or -1
__global__ __launch_bounds__(kNT) void k_tw_scan(const TwPlan *__restrict__ plans, int nm, int32_t *__restrict__ off, long long *__restrict__ info)
{
    __shared__ int32_t wsum[kWaves];
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0x7fffffff;
    __syncthreads();
    long long carry = 0;
    for (int base = 0; base < nm; base += kNT) {
        const int m = base + threadIdx.x;
        int c = 0;
        if (m < nm) {
            c = plans[m].n_states;
            if (plans[m].too_long) {
                c = 0;
                atomicMin(&s_bad, m);
            }
        }
        int total;
        const int excl = block_excl_scan_i32<kNT>(c, wsum, total);
        const long long o = carry + excl;
        if (m < nm) off[m] = o > 0x7fffffffll ? 0x7fffffff : (int32_t)o;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        off[nm] = carry > 0x7fffffffll ? 0x7fffffff : (int32_t)carry;
        info[0] = carry;
        info[1] = s_bad == 0x7fffffff ? -1 : s_bad;
    }
}

// the float narrowing countVisible(float, float, float) performs on isValid's doubles (src/camera.cc:135 from :249)
__device__ __forceinline__ void tw_narrow(const double *q, float *f)
{
    f[0] = (float)q[0];
    f[1] = (float)q[1];
    f[2] = (float)q[2];
}

__global__ __launch_bounds__(kNT) void k_tw_states(const double *__restrict__ q1, const TwPlan *__restrict__ plans, const int32_t *__restrict__ off,
                                                   int nm, int total, double *__restrict__ states, float *__restrict__ fstates)
{
    const int i = blockIdx.x * kNT + threadIdx.x;
    if (i >= total) return;
    int lo = 0, hi = nm - 1;   // the motion with off[m] <= i < off[m + 1] (every motion has a state)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid - 1;
    }
    double a[3] = {q1[3 * (size_t)lo], q1[3 * (size_t)lo + 1], q1[3 * (size_t)lo + 2]};
    double q[3];
    tw_plan_state(a, plans[lo], i - off[lo], q);
    for (int k = 0; k < 3; ++k) states[3 * (size_t)i + k] = q[k];
    tw_narrow(q, fstates + 3 * (size_t)i);
}

__global__ __launch_bounds__(kNT) void k_tw_narrow(const double *__restrict__ states, int ns, float *__restrict__ fstates)
{
    const int i = blockIdx.x * kNT + threadIdx.x;
    if (i < ns) tw_narrow(states + 3 * (size_t)i, fstates + 3 * (size_t)i);
}

// check_collisions(q, robot_r) of every state: cfree [ns]
__global__ __launch_bounds__(kNT) void k_tw_collide(const double *__restrict__ states, int ns, const double *__restrict__ obs, int n_obs,
                                                    aos2_svc_params_t p, double obs_r, uint8_t *__restrict__ cfree)
{
    __shared__ double s_obs[2 * kObsTile];
    __shared__ double s_min[kWaves][kCollideStates];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int i = blockIdx.x * kCollideStates + lane;
    const int ic = min(i, ns - 1);
    const double q[3] = {states[3 * (size_t)ic], states[3 * (size_t)ic + 1], states[3 * (size_t)ic + 2]};
    double best = INFINITY;   // (a minimum does not depend on the order: any split of the obstacles gives nanoflann's exact answer)
    for (int base = 0; base < n_obs; base += kObsTile) {
        const int cnt = min(kObsTile, n_obs - base);
        __syncthreads();
        for (int k = threadIdx.x; k < 2 * cnt; k += kNT) s_obs[k] = obs[2 * (size_t)base + k];
        __syncthreads();
        for (int k = part; k < cnt; k += kWaves) {
            const double d2 = tw_obstacle_d2(q, s_obs[2 * k], s_obs[2 * k + 1]);
            best = d2 < best ? d2 : best;
        }
    }
    s_min[part][lane] = best;
    __syncthreads();
    if (part == 0 && i < ns) {
        for (int w = 1; w < kWaves; ++w) best = s_min[w][lane] < best ? s_min[w][lane] : best;
        const int gate = tw_collision_gate(q, n_obs, p);
        cfree[i] = gate >= 0 ? (uint8_t)gate : (uint8_t)(tw_collision_free(best, p.robot_r, obs_r) ? 1 : 0);
    }
}

// isValid of every state from its two halves
__global__ __launch_bounds__(kNT) void k_tw_valid(const double *__restrict__ states, int ns, const uint8_t *__restrict__ cfree,
                                                  const int32_t *__restrict__ count, int thr, aos2_svc_params_t p, uint8_t *__restrict__ valid)
{
    const int i = blockIdx.x * kNT + threadIdx.x;
    if (i >= ns) return;
    const double q[3] = {states[3 * (size_t)i], states[3 * (size_t)i + 1], states[3 * (size_t)i + 2]};
    valid[i] = tw_is_valid(q, cfree[i] != 0, count[i], thr, p) ? 1 : 0;
}

struct TwVerdict {
    double cost_length, cost_camera;
    int32_t first_invalid, valid;
};

// a wave per motion.  checkMotionTW (:258-268): the first state of 1 .. size-1 that is not valid ends it (q1 is never tested).
// MotionCostLength and MotionCostCamera: a lane forms the term of its state, the terms are added in index order.
__global__ __launch_bounds__(kNT) void k_tw_verdict(const TwPlan *__restrict__ plans, const int32_t *__restrict__ off, int nm,
                                                    const double *__restrict__ states, const uint8_t *__restrict__ valid,
                                                    const int32_t *__restrict__ count, int thr, TwVerdict *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * kWaves + (threadIdx.x >> 6);   // wave-uniform
    if (m >= nm) return;
    const int o = off[m], n = off[m + 1] - o;
    int first = -1;
    double len = 0, camc = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        const bool in = i < n;
        if (first < 0) {
            const unsigned long long fails = __ballot(in && i >= 1 && !valid[o + i]);
            if (fails) first = base + __builtin_ctzll(fails);
        }
        double lt = 0, ct = 0;
        if (in && i >= 1) lt = tw_length_term(states + 3 * (size_t)(o + i - 1), states + 3 * (size_t)(o + i));
        if (in && i >= 1 && i < n - 1) ct = vis_motion_cost_term(count[o + i], thr);
        const int cnt = min(64, n - base);   // wave-uniform
        for (int b = 0; b < cnt; ++b) {
            const int gi = base + b;
            if (gi >= 1) len += readlane_f64(lt, b);
            if (gi >= 1 && gi < n - 1) camc += readlane_f64(ct, b);
        }
    }
    if (lane == 0) {
        TwVerdict v;
        const bool path = plans[m].valid != 0;
        v.cost_length = len;   // (without a path Q = {q1}: no term, 0)
        v.cost_camera = camc;
        v.first_invalid = first;
        v.valid = path && first < 0 ? 1 : 0;
        out[m] = v;
    }
}

__global__ __launch_bounds__(kNT) void k_tw_math(const double *__restrict__ x, const double *__restrict__ y, int n, double *__restrict__ out)
{
    const int i = blockIdx.x * kNT + threadIdx.x;
    if (i >= n) return;
    out[i] = tw_sin(x[i]);
    out[(size_t)n + i] = tw_cos(x[i]);
    out[2 * (size_t)n + i] = tw_atan2(y[i], x[i]);
    out[3 * (size_t)n + i] = sqrt(x[i]);
    out[4 * (size_t)n + i] = y[i] / x[i];
}

}  // namespace

struct aos2_svc {
    int device = 0;
    aos2_svc_params_t params;
    aos2_vis_t *vis = nullptr;
    std::vector<double> obs;   // [n][2], the host copy (the host tap reads it)
    double obs_r = 0.1;
    bool obs_dirty = true;
    bool dev_ready = false;
    hipStream_t stream = nullptr;
    hipEvent_t ev[2] = {};
    DevBuf<double> d_obs, d_q, d_states;
    DevBuf<float> d_fstates;
    DevBuf<TwPlan> d_plans;
    DevBuf<int32_t> d_off;
    DevBuf<long long> d_info;
    DevBuf<uint8_t> d_cfree, d_valid;
    DevBuf<TwVerdict> d_verdict;
    std::vector<TwPlan> plans;       // the call's results on the host
    std::vector<TwVerdict> verdicts;
    std::vector<int32_t> off;
    float last_ms = 0;
};

namespace aos2 {

void svc_view(const aos2_svc_t *h, SvcView *v)
{
    v->params = h->params;
    v->n_obs = (int)(h->obs.size() / 2);
    v->obs = h->obs.data();
    v->obs_r = h->obs_r;
    v->vis = h->vis;
    aos2_vis_camera_t cam;
    VisMapView map;
    vis_view(h->vis, &cam, &map);
    v->thr = h->params.feature_threshold == -1 ? cam.feature_threshold : h->params.feature_threshold;
}

static int check_states(const char *what, int n, const double *q)
{
    for (int i = 0; i < n; ++i)
        if (!tw_state_ok(q + 3 * (size_t)i)) {
            set_error("%s %d = (%g, %g, %g): every component must be finite and |theta| <= 1e4", what, i, q[3 * (size_t)i], q[3 * (size_t)i + 1],
                      q[3 * (size_t)i + 2]);
            return AOS2_ERR_ARG;
        }
    return AOS2_OK;
}

int svc_check_valid(const aos2_svc_t *h, int ns, const double *states, const uint8_t *valid)
{
    if (!h || ns < 0 || (ns > 0 && (!states || !valid))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    return check_states("state", ns, states);
}

int svc_check_motions(const aos2_svc_t *h, int nm, const double *q1, const double *q2, const aos2_svc_motions_out_t *out)
{
    if (!h || nm < 0 || !out || (nm > 0 && (!q1 || !q2)) || (out->states && out->states_capacity < 0)) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (int st = check_states("q1 of motion", nm, q1)) return st;
    return check_states("q2 of motion", nm, q2);
}

}  // namespace aos2

namespace {

int init_device(aos2_svc *h)
{
    if (int st = bind_device(h->device)) return st;
    if (h->dev_ready) return AOS2_OK;
    if (int st = stream_create(&h->stream, false)) return st;
    for (auto &e : h->ev) AOS2_HIP_CHECK(hipEventCreate(&e));
    h->dev_ready = true;
    return AOS2_OK;
}

int upload_obstacles(aos2_svc *h)
{
    if (!h->obs_dirty) return AOS2_OK;
    if (int st = h->d_obs.alloc(h->obs.size())) return st;
    if (!h->obs.empty())
        AOS2_HIP_CHECK(hipMemcpyAsync(h->d_obs.p, h->obs.data(), h->obs.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    h->obs_dirty = false;
    return AOS2_OK;
}

// collision flags, counts and isValid of ns states that are in d_states / d_fstates -> d_cfree, *count, d_valid
int launch_state_checks(aos2_svc *h, int ns, int thr, const int32_t **count)
{
    int st;
    hipStream_t s = h->stream;
    if ((st = upload_obstacles(h)) || (st = h->d_cfree.alloc(ns)) || (st = h->d_valid.alloc(ns))) return st;
    hipLaunchKernelGGL(k_tw_collide, dim3((ns + kCollideStates - 1) / kCollideStates), dim3(kNT), 0, s, h->d_states.p, ns, h->d_obs.p,
                       (int)(h->obs.size() / 2), h->params, h->obs_r, h->d_cfree.p);
    AOS2_HIP_CHECK(hipGetLastError());
    if ((st = vis_counts_on_device(h->vis, ns, h->d_fstates.p, s, count))) return st;
    hipLaunchKernelGGL(k_tw_valid, dim3((ns + kNT - 1) / kNT), dim3(kNT), 0, s, h->d_states.p, ns, h->d_cfree.p, *count, thr, h->params,
                       h->d_valid.p);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

int finish(aos2_svc *h)
{
    AOS2_HIP_CHECK(hipStreamSynchronize(h->stream));
    AOS2_HIP_CHECK(hipEventElapsedTime(&h->last_ms, h->ev[0], h->ev[1]));
    return AOS2_OK;
}

}  // namespace

extern "C" {

int aos2_svc_params_default(aos2_svc_params_t *p)
{
    if (!p) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    p->turn_radius = 0.25; p->robot_r = 0.4; p->dt = 0.3;
    p->min_x = -1.15; p->max_x = 6.5; p->min_y = -5; p->max_y = 5;
    p->max_dist_heuristic = 2;
    p->start[0] = p->start[1] = p->start[2] = 0.0;
    p->heuristic = 0;
    p->feature_threshold = -1;
    return AOS2_OK;
}

int aos2_svc_create(int device, aos2_svc_t **out)
{
    if (!out) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    aos2_svc *h = new aos2_svc();
    h->device = device;
    aos2_svc_params_default(&h->params);
    if (int st = aos2_vis_create(device, &h->vis)) {
        delete h;
        return st;
    }
    *out = h;
    return AOS2_OK;
}

void aos2_svc_destroy(aos2_svc_t *h)
{
    if (!h) return;
    if (h->dev_ready) {
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        h->d_obs.release(); h->d_q.release(); h->d_states.release(); h->d_fstates.release(); h->d_plans.release(); h->d_off.release();
        h->d_info.release(); h->d_cfree.release(); h->d_valid.release(); h->d_verdict.release();
        for (auto &e : h->ev) (void)hipEventDestroy(e);
        (void)hipStreamDestroy(h->stream);
    }
    aos2_vis_destroy(h->vis);
    delete h;
}

aos2_vis_t *aos2_svc_vis(aos2_svc_t *h) { return h ? h->vis : nullptr; }

int aos2_svc_set_params(aos2_svc_t *h, const aos2_svc_params_t *p)
{
    if (!h || !p) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    const double v[11] = {p->turn_radius, p->robot_r, p->dt, p->min_x, p->max_x, p->min_y, p->max_y, p->max_dist_heuristic,
                          p->start[0], p->start[1], p->start[2]};
    bool finite = true;
    for (double x : v) finite = finite && std::isfinite(x);
    if (!finite || !(p->turn_radius > 0) || !(p->dt > 0)) {
        set_error("motion checks: a parameter is not finite, or turn_radius or dt is not positive");
        return AOS2_ERR_ARG;
    }
    h->params = *p;
    return AOS2_OK;
}

int aos2_svc_set_obstacles(aos2_svc_t *h, int n, const double *xy, double obs_r)
{
    if (!h || n < 0 || (n > 0 && !xy) || !std::isfinite(obs_r)) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    for (size_t i = 0; i < 2 * (size_t)n; ++i)
        if (!std::isfinite(xy[i])) {
            set_error("motion checks: obstacle %zu is not finite", i / 2);
            return AOS2_ERR_ARG;
        }
    if (h->dev_ready) {   // (a call's copies are waited for before it returns; this is for a call that failed half way)
        if (int st = bind_device(h->device)) return st;
        AOS2_HIP_CHECK(hipStreamSynchronize(h->stream));
    }
    h->obs.assign(xy, xy + 2 * (size_t)n);
    h->obs_r = obs_r;
    h->obs_dirty = true;
    return AOS2_OK;
}

void aos2_svc_collide_tile(int *obstacles, int *states)
{
    if (obstacles) *obstacles = kObsTile;
    if (states) *states = kCollideStates;
}

int aos2_svc_valid(aos2_svc_t *h, int ns, const double *states, uint8_t *valid, uint8_t *collision_free, int32_t *count)
{
    if (int st = svc_check_valid(h, ns, states, valid)) return st;
    if (ns == 0) return AOS2_OK;
    int st;
    if ((st = init_device(h))) return st;
    hipStream_t s = h->stream;
    SvcView V;
    svc_view(h, &V);
    if ((st = h->d_states.alloc(3 * (size_t)ns)) || (st = h->d_fstates.alloc(3 * (size_t)ns))) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(h->d_states.p, states, 3 * (size_t)ns * sizeof(double), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_tw_narrow, dim3((ns + kNT - 1) / kNT), dim3(kNT), 0, s, h->d_states.p, ns, h->d_fstates.p);
    AOS2_HIP_CHECK(hipGetLastError());
    const int32_t *d_count = nullptr;
    if ((st = launch_state_checks(h, ns, V.thr, &d_count))) return st;
    AOS2_HIP_CHECK(hipEventRecord(h->ev[1], s));
    AOS2_HIP_CHECK(hipMemcpyAsync(valid, h->d_valid.p, ns, hipMemcpyDeviceToHost, s));
    if (collision_free) AOS2_HIP_CHECK(hipMemcpyAsync(collision_free, h->d_cfree.p, ns, hipMemcpyDeviceToHost, s));
    if (count) AOS2_HIP_CHECK(hipMemcpyAsync(count, d_count, ns * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return finish(h);
}

int aos2_svc_motions(aos2_svc_t *h, int nm, const double *q1, const double *q2, aos2_svc_motions_out_t *out)
{
    if (int st = svc_check_motions(h, nm, q1, q2, out)) return st;
    out->states_needed = 0;
    if (nm == 0) {
        if (out->offsets) out->offsets[0] = 0;
        return AOS2_OK;
    }
    int st;
    if ((st = init_device(h))) return st;
    hipStream_t s = h->stream;
    SvcView V;
    svc_view(h, &V);
    const size_t N = (size_t)nm;
    if ((st = h->d_q.alloc(6 * N)) || (st = h->d_plans.alloc(N)) || (st = h->d_off.alloc(N + 1)) || (st = h->d_info.alloc(2)) ||
        (st = h->d_verdict.alloc(N)))
        return st;
    double *d_q1 = h->d_q.p, *d_q2 = h->d_q.p + 3 * N;
    AOS2_HIP_CHECK(hipMemcpyAsync(d_q1, q1, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipMemcpyAsync(d_q2, q2, 3 * N * sizeof(double), hipMemcpyHostToDevice, s));
    AOS2_HIP_CHECK(hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_tw_paths, dim3((unsigned)((8 * N + kNT - 1) / kNT)), dim3(kNT), 0, s, d_q1, d_q2, nm, h->params.turn_radius,
                       h->params.dt, h->d_plans.p);
    AOS2_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(k_tw_scan, dim3(1), dim3(kNT), 0, s, h->d_plans.p, nm, h->d_off.p, h->d_info.p);
    AOS2_HIP_CHECK(hipGetLastError());
    // the one host wait of the call before its results: the total sizes the state buffers and the launches over the states
    long long info[2] = {0, -1};
    AOS2_HIP_CHECK(hipMemcpyAsync(info, h->d_info.p, sizeof(info), hipMemcpyDeviceToHost, s));
    AOS2_HIP_CHECK(hipStreamSynchronize(s));
    if (info[1] >= 0) {
        set_error("motion checks: a segment of motion %lld has more than %d states", info[1], AOS2_SVC_MAX_SEGMENT_STATES);
        return AOS2_ERR_ARG;
    }
    const long long total = info[0];
    out->states_needed = total;
    if (total > 0x7fffffffll / 3) {
        set_error("motion checks: the motions have %lld states together, more than a call takes", total);
        return AOS2_ERR_ARG;
    }
    if (out->states && out->states_capacity < total) {
        set_error("motion checks: the states need %lld rows, the buffer has %lld", total, (long long)out->states_capacity);
        return AOS2_ERR_CAPACITY;
    }
    const int ns = (int)total;
    if ((st = h->d_states.alloc(3 * (size_t)ns)) || (st = h->d_fstates.alloc(3 * (size_t)ns))) return st;
    hipLaunchKernelGGL(k_tw_states, dim3((ns + kNT - 1) / kNT), dim3(kNT), 0, s, d_q1, h->d_plans.p, h->d_off.p, nm, ns, h->d_states.p,
                       h->d_fstates.p);
    AOS2_HIP_CHECK(hipGetLastError());
    const int32_t *d_count = nullptr;
    if ((st = launch_state_checks(h, ns, V.thr, &d_count))) return st;
    hipLaunchKernelGGL(k_tw_verdict, dim3((nm + kWaves - 1) / kWaves), dim3(kNT), 0, s, h->d_plans.p, h->d_off.p, nm, h->d_states.p,
                       h->d_valid.p, d_count, V.thr, h->d_verdict.p);
    AOS2_HIP_CHECK(hipGetLastError());
    AOS2_HIP_CHECK(hipEventRecord(h->ev[1], s));
    h->plans.resize(N);
    h->verdicts.resize(N);
    AOS2_HIP_CHECK(hipMemcpyAsync(h->plans.data(), h->d_plans.p, N * sizeof(TwPlan), hipMemcpyDeviceToHost, s));
    AOS2_HIP_CHECK(hipMemcpyAsync(h->verdicts.data(), h->d_verdict.p, N * sizeof(TwVerdict), hipMemcpyDeviceToHost, s));
    if (out->offsets) AOS2_HIP_CHECK(hipMemcpyAsync(out->offsets, h->d_off.p, (N + 1) * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    if (out->states) AOS2_HIP_CHECK(hipMemcpyAsync(out->states, h->d_states.p, 3 * (size_t)ns * sizeof(double), hipMemcpyDeviceToHost, s));
    if ((st = finish(h))) return st;
    for (int m = 0; m < nm; ++m) {
        const TwPlan &P = h->plans[m];
        const TwVerdict &R = h->verdicts[m];
        if (out->path_valid) out->path_valid[m] = (uint8_t)P.valid;
        if (out->type) out->type[m] = P.type;
        for (int k = 0; k < 3; ++k) {
            if (out->t) out->t[3 * (size_t)m + k] = P.t[k];
            if (out->m) out->m[3 * (size_t)m + k] = P.m[k];
        }
        if (out->n_states) out->n_states[m] = P.n_states;
        if (out->valid) out->valid[m] = (uint8_t)R.valid;
        if (out->first_invalid) out->first_invalid[m] = R.first_invalid;
        if (out->cost_length) out->cost_length[m] = R.cost_length;
        if (out->cost_camera) out->cost_camera[m] = R.cost_camera;
    }
    return AOS2_OK;
}

float aos2_svc_last_device_ms(const aos2_svc_t *h) { return h ? h->last_ms : 0.0f; }

int aos2_debug_tw_math(int device, int n, const double *x, const double *y, double *sn, double *cs, double *at, double *sq, double *quot)
{
    if (n < 0 || (n > 0 && (!x || !y || !sn || !cs || !at || !sq || !quot))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (n == 0) return AOS2_OK;
    if (device < 0) {
        for (int i = 0; i < n; ++i) {
            sn[i] = tw_sin(x[i]);
            cs[i] = tw_cos(x[i]);
            at[i] = tw_atan2(y[i], x[i]);
            sq[i] = sqrt(x[i]);
            quot[i] = y[i] / x[i];
        }
        return AOS2_OK;
    }
    int st;
    if ((st = bind_device(device))) return st;
    const size_t N = (size_t)n;
    DevBuf<double> d_in, d_out;
    if ((st = d_in.alloc(2 * N)) || (st = d_out.alloc(5 * N))) {
        d_in.release();
        return st;
    }
    hipError_t e = hipMemcpy(d_in.p, x, N * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in.p + N, y, N * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_tw_math, dim3((n + kNT - 1) / kNT), dim3(kNT), 0, 0, d_in.p, d_in.p + N, n, d_out.p);
        e = hipGetLastError();
    }
    double *outs[5] = {sn, cs, at, sq, quot};
    for (int k = 0; k < 5 && e == hipSuccess; ++k) e = hipMemcpy(outs[k], d_out.p + k * N, N * sizeof(double), hipMemcpyDeviceToHost);
    d_in.release();
    d_out.release();
    if (e != hipSuccess) {
        set_error("aos2_debug_tw_math: %s", hipGetErrorString(e));
        return AOS2_ERR_HIP;
    }
    return AOS2_OK;
}

}  // extern "C"
