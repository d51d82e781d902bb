// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:363-413) for a batch of points over the observation lists that an aos2_local_map
// handle keeps in HBM.  The cost is per observation -- an f64 square root, an f64
// divide and an f64 atan2 behind three gathered floats -- and a point has about 7 of them, so a point gets a GROUP OF 8 LANES, eight
// points to a wave, 32 to a workgroup.  One kernel:
//   terms   a lane per observation, 8 at a time (csrc/normal_depth.h: nd_term), the list walked in chunks of 8 up to the longest
//           list of the wave (the cross-lane steps need every lane active)
//   sums    `normal` (three float sums) and the double sum of the thetas folded STRICTLY IN LIST ORDER, one add after the other
//           (wave_ops.h: group8_sum_ordered): the order of the adds is part of the result, so there is no tree
//   std     the second pass of compute_std_pts needs the thetas again behind the mean: each lane reads back the ones it wrote --
//           from LDS for a list of up to 64 entries, from the handle's global scratch for a longer one (the host plans the slots from
//           the row lengths it keeps)
//   tail    lane 0 of the group: the reference keyframe's octave, the distances, the members and the planner's row
// The points of a batch run in groups whose scratch fits the handle's bound, one group after the other on the handle's stream; the
// arguments go up in one copy and the results come back in one.  The resident graph is never written.
#include <algorithm>
#include <vector>

#include "aos2_common.h"
#include "local_map.h"
#include "normal_depth.h"
#include "regions.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kNT = 256;                       // threads of k_nd
constexpr int kNdPoints = kNT / 8;             // points of a workgroup
constexpr int kNdLdsTerms = 64;                // thetas of one point that wait in LDS
constexpr int kNdLdsStride = kNdLdsTerms + 8;  // ... at a stride that spreads the four points of a half wave over the 32 banks

// one call's arguments and results on the device (the whole batch) and the scratch of one group
struct NdDev {
    int n_levels, rows_form, scratch_floats;
    const int32_t *point, *ref_kf, *soff, *term_off;   // soff: the point's slot in `scratch`, -1 = LDS; term_off NULL: no terms
    const float *xyz, *kf_center, *scale;
    int32_t *status, *n_terms;
    float *normal, *min_dist, *max_dist, *theta_mean, *theta_std, *upper, *lower, *max_range, *min_range;
    float *term_unit, *term_theta;   // NULL: not wanted
    float *scratch;
};

// :363-413 for the listed points [i0, i1)
__global__ __launch_bounds__(kNT) void k_nd(LmGraph G, NdDev D, int i0, int i1)
{
    __shared__ float s_theta[kNdPoints * kNdLdsStride];
    const int tid = threadIdx.x, li = tid & 7;
    const int i = i0 + blockIdx.x * kNdPoints + (tid >> 3);
    const bool listed = i < i1;
    // :365-379, the same in the 8 lanes of a group
    int e0 = 0, n = 0, st = AOS2_ND_UNKNOWN, pRefKF = 0, soff = -1, tslot = -1;
    float Pos[3] = {0.0f, 0.0f, 0.0f};
    if (listed) {
        st = nd_point_gate(G, D.point[i], e0, n);
        pRefKF = D.ref_kf[i];
        soff = D.soff[i];
        tslot = nd_term_slot(D.term_off, i, n);
        for (int c = 0; c < 3; ++c) Pos[c] = D.xyz[3 * (size_t)i + c];
    }
    const bool in_lds = soff < 0;
    float *lds = s_theta + (tid >> 3) * kNdLdsStride;
    float *far = D.scratch + (in_lds ? 0 : soff);
    // (a slot is planned from the row length: the limits only keep a wrong plan from writing outside)
    const int room = in_lds ? kNdLdsTerms : D.scratch_floats - soff;
    const int chunks = wave_max_i32((n + 7) >> 3);
    // :381-396
    float normal[3] = {0.0f, 0.0f, 0.0f};
    double sum = 0.0;
    int idx = -1;
    for (int c = 0; c < chunks; ++c) {
        const int j = c * 8 + li;
        NdTerm t = {{0.0f, 0.0f, 0.0f}, 0.0f};
        if (j < n) {
            const int pKF = G.obs_kf[e0 + j];
            t = nd_term(Pos, D.kf_center + 3 * (size_t)pKF);
            if (pKF == pRefKF) idx = G.obs_idx[e0 + j];
            if (j < room) {
                if (in_lds) lds[j] = t.theta;
                else far[j] = t.theta;
            }
            if (tslot >= 0) {
                if (D.term_unit)
                    for (int k = 0; k < 3; ++k) D.term_unit[3 * (size_t)(tslot + j) + k] = t.u[k];
                if (D.term_theta) D.term_theta[tslot + j] = t.theta;
            }
        }
        const int cnt = min(8, max(0, n - c * 8));
        for (int k = 0; k < 3; ++k) normal[k] = group8_sum_ordered(normal[k], t.u[k], cnt);
        sum = group8_sum_ordered(sum, (double)t.theta, cnt);
    }
    idx = max(group8_max_i32(idx), 0);   // observations[pRefKF]: a keyframe that is not in the map yields 0
    // compute_std_pts :32-35
    const float mean = nd_mean(sum, n);
    double sq_sum = 0.0;
    for (int c = 0; c < chunks; ++c) {
        const int j = c * 8 + li;
        float q = 0.0f;
        if (j < n && j < room) q = nd_sq_term(in_lds ? lds[j] : far[j], mean);
        sq_sum = group8_sum_ordered(sq_sum, (double)q, min(8, max(0, n - c * 8)));
    }
    if (!listed || li != 0) return;
    // :398-410
    const int level = st == AOS2_ND_UPDATED ? nd_ref_level(G, pRefKF, idx, D.n_levels) : -1;
    if (st == AOS2_ND_UPDATED && level < 0) st = AOS2_ND_REF_UNUSABLE;
    D.status[i] = st;
    if (st != AOS2_ND_UPDATED) return;
    float max_dist, min_dist;
    nd_distances(nd_dist(Pos, D.kf_center + 3 * (size_t)pRefKF), D.scale[level], D.scale[D.n_levels - 1], max_dist, min_dist);
    const float k = nd_normal_scale(n), stdev = nd_std(sq_sum, n);
    for (int c = 0; c < 3; ++c) D.normal[3 * (size_t)i + c] = normal[c] * k;
    D.max_dist[i] = max_dist;
    D.min_dist[i] = min_dist;
    D.theta_mean[i] = mean;
    D.theta_std[i] = stdev;
    D.n_terms[i] = n;
    const NdRows r = nd_rows(D.rows_form, mean, stdev, min_dist, max_dist);
    D.upper[i] = r.upper;
    D.lower[i] = r.lower;
    D.max_range[i] = r.max_range;
    D.min_range[i] = r.min_range;
}

}  // namespace

extern "C" {

int aos2_local_map_debug_normal_depth(aos2_local_map_t *h, int lds_terms)
{
    if (!h || lds_terms > kNdLdsTerms) {
        set_error("bad argument (at most %d thetas of an observation list wait in LDS)", kNdLdsTerms);
        return AOS2_ERR_ARG;
    }
    h->nd.lds_terms = lds_terms;
    return AOS2_OK;
}

int aos2_local_map_update_normal_depth(aos2_local_map_t *h, const aos2_normal_depth_t *a)
{
    if (!h || !a) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    static const char *const pre = "update normal and depth";
    if (!h->has_graph) return lm_fail(pre, "aos2_local_map_set comes first");
    if (!h->kfc.has_view) return lm_fail(pre, "aos2_local_map_set_culling_view comes first");
    char why[200];
    if (nd_check(*a, h->n_kfs, why, sizeof why)) return lm_fail(pre, "%s", why);
    NdState &K = h->nd;
    const int n = a->n, lds_terms = K.lds_terms < 0 ? kNdLdsTerms : K.lds_terms;
    // the plan: a slot of the scratch for every list that is too long for LDS (the handle keeps every row's length), and the groups
    // whose slots fit the bound
    const int64_t cap = std::min<int64_t>(h->scratch_bytes / 4, INT32_MAX);
    std::vector<int32_t> soff(n), group_end;
    int64_t used = 0, most = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t len = a->point[i] < h->n_points ? h->row_obs[a->point[i]] : 0;
        soff[i] = -1;
        if (len <= lds_terms) continue;
        if (len > cap)
            return lm_fail(pre, "the %lld observations of point %d need %lld bytes of scratch, the bound is %lld", (long long)len,
                           a->point[i], (long long)len * 4, (long long)h->scratch_bytes);
        if (used + len > cap) {
            group_end.push_back(i);
            used = 0;
        }
        soff[i] = (int32_t)used;
        used += len;
        most = std::max(most, used);
    }
    group_end.push_back(n);
    K.timer.timed = false;
    h->last_groups = 0;
    if (n == 0) return AOS2_OK;
    int st;
    if ((st = bind_device(h->device))) return st;
    if ((st = local_map_upload(h, kLmGraph)) || (st = local_map_upload(h, kLmView))) return st;
    if (!h->stream && (st = stream_create(&h->stream, false))) return st;
    if ((st = h->d_scratch.alloc((size_t)most + 64))) return st;
    const size_t B = (size_t)n, nk = (size_t)h->n_kfs, T = a->term_off ? (size_t)a->term_off[n] : 0;
    const bool terms = T > 0 && (a->term_unit || a->term_theta);
    NdDev D = {};
    // one block: what goes in, then what comes back; the page-locked staging has the same layout
    Regions<24> R;
    R.add(D.point, B); R.add(D.ref_kf, B); R.add(D.soff, B); R.add(D.xyz, 3 * B); R.add(D.kf_center, 3 * nk);
    R.add(D.scale, (size_t)a->n_levels);
    if (terms) R.add(D.term_off, B + 1);
    const size_t in_bytes = R.bytes();
    const size_t out0 = R.add(D.status, B);
    R.add(D.n_terms, B); R.add(D.normal, 3 * B); R.add(D.min_dist, B); R.add(D.max_dist, B); R.add(D.theta_mean, B);
    R.add(D.theta_std, B); R.add(D.upper, B); R.add(D.lower, B); R.add(D.max_range, B); R.add(D.min_range, B);
    if (terms && a->term_unit) R.add(D.term_unit, 3 * T);
    if (terms && a->term_theta) R.add(D.term_theta, T);
    if ((st = K.d_io.alloc(R.bytes() + 256)) || (st = K.io.alloc(R.bytes() + 256))) return st;
    R.bind(K.io.p);   // (the staging first: the same fields name the inputs' places)
    memcpy(const_cast<int32_t *>(D.point), a->point, B * 4);
    memcpy(const_cast<int32_t *>(D.ref_kf), a->ref_kf, B * 4);
    memcpy(const_cast<int32_t *>(D.soff), soff.data(), B * 4);
    memcpy(const_cast<float *>(D.xyz), a->xyz, 3 * B * 4);
    if (nk) memcpy(const_cast<float *>(D.kf_center), a->kf_center, 3 * nk * 4);
    memcpy(const_cast<float *>(D.scale), a->scale, (size_t)a->n_levels * 4);
    if (terms) memcpy(const_cast<int32_t *>(D.term_off), a->term_off, (B + 1) * 4);
    const NdDev S = D;   // the staging's addresses: where the results are read
    R.bind(K.d_io.p);
    D.n_levels = a->n_levels;
    D.rows_form = a->rows_form;
    D.scratch = reinterpret_cast<float *>(h->d_scratch.p);
    D.scratch_floats = (int)most;
    hipStream_t q = h->stream;
    if ((st = K.timer.begin(q))) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(K.d_io.p, K.io.p, in_bytes, hipMemcpyHostToDevice, q));
    int i0 = 0;
    for (const int i1 : group_end) {
        if (i1 > i0) {
            hipLaunchKernelGGL(k_nd, dim3((i1 - i0 + kNdPoints - 1) / kNdPoints), dim3(kNT), 0, q, h->G, D, i0, i1);
            AOS2_HIP_CHECK(hipGetLastError());
            ++h->last_groups;
        }
        i0 = i1;
    }
    AOS2_HIP_CHECK(hipMemcpyAsync(K.io.p + out0, K.d_io.p + out0, R.bytes() - out0, hipMemcpyDeviceToHost, q));
    if ((st = K.timer.end(q, true))) return st;
    // the status of every listed point; the values of the updated ones only -- the others keep what the caller's arrays hold
    for (int i = 0; i < n; ++i) {
        const int s = S.status[i];
        if (a->status) a->status[i] = (uint8_t)s;
        if (s != AOS2_ND_UPDATED) continue;
        NdPoint p = {{S.normal[3 * (size_t)i], S.normal[3 * (size_t)i + 1], S.normal[3 * (size_t)i + 2]}, S.min_dist[i], S.max_dist[i],
                     S.theta_mean[i], S.theta_std[i], S.n_terms[i]};
        nd_store(*a, i, p, NdRows{S.upper[i], S.lower[i], S.max_range[i], S.min_range[i]});
        const int slot = terms ? nd_term_slot(a->term_off, i, p.n_terms) : -1;
        if (slot < 0) continue;
        if (a->term_unit) memcpy(a->term_unit + 3 * (size_t)slot, S.term_unit + 3 * (size_t)slot, (size_t)p.n_terms * 12);
        if (a->term_theta) memcpy(a->term_theta + slot, S.term_theta + slot, (size_t)p.n_terms * 4);
    }
    return AOS2_OK;
}

float aos2_local_map_last_normal_depth_device_ms(aos2_local_map_t *h)
{
    return h ? h->nd.timer.ms() : -1.f;
}

}  // extern "C"
