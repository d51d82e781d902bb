// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:636-700) over the graph that an aos2_local_map handle keeps in HBM
// (DESIGN.md section 2 item 19, section 5.14).  The loop is serial in its effects -- a culled keyframe leaves the observations of
// its points, points fall to nObs <= 2 and go bad, and both change the counts of the candidates behind it -- but between two culls
// every candidate is independent.  So the call runs in rounds over a cursor into the candidate list:
//   k_kfc_init    the overlay of this call: copies of point_nobs / point_bad, no stamp, no erased entry, cursor 0
//   k_kfc_count   a workgroup per candidate at or behind the cursor, a lane per feature (strided): the per-item function of
//                 csrc/kf_culling.h through the overlay, wave sums, nMPs / nRedundantObservations of the candidate AS THE MAP IS NOW
//   k_kfc_apply   one workgroup: scans the verdicts from the cursor in candidate order, finalises everything up to and including
//                 the first CULLED candidate (its counts are those of the serial loop: nothing before it in this round culled),
//                 applies that candidate's erasure with a lane per feature, and moves the cursor behind it
// A call needs culls + 1 rounds; a fixed number is enqueued at a time, every launch returns at once when the cursor is at the
// end, and the host reads the cursor with the results and enqueues again while it is short.  The resident graph is never written.
#include <algorithm>
#include <vector>

#include "aos2_common.h"
#include "kf_culling.h"
#include "local_map.h"
#include "regions.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kIT = 256;           // threads of k_kfc_init
constexpr int kCT = 1024;          // threads of k_kfc_count: a keyframe's 1000-2000 features in one or two strides (the walk is a
                                   // chain of dependent loads, so a lane's features in a row are what a round costs)
constexpr int kAT = 1024;          // threads of k_kfc_apply
constexpr int kRoundsDefault = 4;  // count + apply pairs per enqueue

// ctl: the cursor, the rounds that did work, the points that went bad
enum { kCursor = 0, kRounds = 1, kNBad = 2, kCtlInts = 4 };

// one call's block of scratch behind the overlay.  ctl .. status are read back in one copy.
struct KfcCall {
    int n_cand, monocular;
    const int32_t *cand;
    int32_t *ctl, *n_mps, *n_red;
    uint8_t *status;
    int32_t *c_mps, *c_red;   // the counts of the current round
    int32_t *bad_rows;        // [n_points] in the order they went bad
};

__global__ __launch_bounds__(kIT) void k_kfc_init(LmGraph G, KfcOverlay X, KfcCall C, int n_obs)
{
    const int stride = gridDim.x * kIT, t0 = blockIdx.x * kIT + threadIdx.x;
    for (int p = t0; p < G.n_points; p += stride) {
        X.nobs[p] = G.point_nobs[p];
        X.bad[p] = G.point_bad[p];
        X.stamp[p] = -1;
    }
    for (int e = t0; e < n_obs; e += stride) X.erased[e] = 0;
    if (t0 < kCtlInts) C.ctl[t0] = 0;
}

__global__ __launch_bounds__(kCT) void k_kfc_count(LmGraph G, KfcOverlay X, KfcCall C)
{
    __shared__ int s_sum[2];
    const int ci = blockIdx.x, tid = threadIdx.x;
    if (ci < C.ctl[kCursor]) return;   // (final already; at the end of the list: every workgroup)
    const int kf = C.cand[ci];
    if (tid < 2) s_sum[tid] = 0;
    __syncthreads();
    int mps = 0, red = 0;
    if (!(G.kf_flags[kf] & 1)) {   // :647
        const int f0 = G.kf_mp_off[kf], f1 = G.kf_mp_off[kf + 1];
        for (int f = f0 + tid; f < f1; f += kCT) {
            const int r = kfc_feature(G, X, C.monocular, kf, f);
            mps += r & 1;
            red += r >> 1;
        }
    }
    mps = wave_sum_i32(mps);
    red = wave_sum_i32(red);
    if ((tid & 63) == 0) {
        atomicAdd(&s_sum[0], mps);
        atomicAdd(&s_sum[1], red);
    }
    __syncthreads();
    if (tid == 0) {
        C.c_mps[ci] = s_sum[0];
        C.c_red[ci] = s_sum[1];
    }
}

__global__ __launch_bounds__(kAT) void k_kfc_apply(LmGraph G, KfcOverlay X, KfcCall C)
{
    __shared__ int s_culled, s_next;
    const int tid = threadIdx.x;
    const int cursor = C.ctl[kCursor];
    if (cursor >= C.n_cand) return;
    if (tid == 0) {
        int culled = -1, ci = cursor;
        for (; ci < C.n_cand; ++ci) {
            const int mps = C.c_mps[ci], red = C.c_red[ci];
            const int st = kfc_status(G.kf_flags[C.cand[ci]], mps, red);
            C.status[ci] = (uint8_t)st;
            C.n_mps[ci] = mps;
            C.n_red[ci] = red;
            if (st == AOS2_KFC_CULLED) {
                culled = ci++;
                break;
            }
        }
        s_culled = culled;
        s_next = ci;
    }
    __syncthreads();
    const int ci = s_culled;
    if (ci >= 0) {
        const int kf = C.cand[ci];
        const int f0 = G.kf_mp_off[kf], f1 = G.kf_mp_off[kf + 1];
        for (int f = f0 + tid; f < f1; f += kAT)
            if (kfc_erase(G, X, kf, ci, f)) C.bad_rows[atomicAdd(&C.ctl[kNBad], 1)] = G.kf_mp[f];
    }
    if (tid == 0) {
        C.ctl[kCursor] = s_next;
        C.ctl[kRounds] += 1;
    }
}

}  // namespace

namespace aos2 {

int kf_culling_check_view(const aos2_local_map_graph_t *g, const aos2_kf_culling_view_t *v)
{
    if (!g || !v) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    const size_t np = (size_t)g->n_points, nk = (size_t)g->n_keyframes;
    const LmArrays<LmPtr> A = lm_from_public(*g, v);
    if (lm_null_with_length(A, LmCounts{np, nk, nk, (size_t)A.obs_off[np], (size_t)A.kf_mp_off[nk], 0}, kLmView))
        return lm_fail("keyframe culling", "an array of the view is NULL");
    if (lm_bad_obs_idx("keyframe culling", (int)np, nullptr, A.obs_off, A.obs_kf, A.obs_idx,
                       [&](int kf) { return A.kf_mp_off[kf + 1] - A.kf_mp_off[kf]; }))
        return AOS2_ERR_ARG;
    return AOS2_OK;
}

int kf_culling_check_call(int n_keyframes, int n_cand, const int32_t *cand, const uint8_t *status, const int32_t *n_mps,
                          const int32_t *n_redundant, const int32_t *bad_points, int bad_cap, const int32_t *n_bad_points)
{
    if (n_cand < 0 || bad_cap < 0 || !n_bad_points || (bad_cap > 0 && !bad_points) ||
        (n_cand > 0 && (!cand || !status || !n_mps || !n_redundant)))
        return lm_fail("keyframe culling", "bad argument (%d candidates, room for %d bad points)", n_cand, bad_cap);
    std::vector<uint8_t> listed(n_keyframes, 0);
    for (int i = 0; i < n_cand; ++i) {
        if (cand[i] < 0 || cand[i] >= n_keyframes)
            return lm_fail("keyframe culling", "cand[%d] = %d is outside [0, %d)", i, cand[i], n_keyframes);
        if (listed[cand[i]])
            return lm_fail("keyframe culling", "keyframe %d is listed twice", cand[i]);
        listed[cand[i]] = 1;
    }
    return AOS2_OK;
}

}  // namespace aos2

extern "C" {

int aos2_local_map_set_culling_view(aos2_local_map_t *h, const aos2_kf_culling_view_t *view)
{
    if (!h || !view) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (!h->has_graph)
        return lm_fail("keyframe culling", "aos2_local_map_set comes first");
    aos2_local_map_graph_t g;
    if (int st = aos2_local_map_get(h, &g)) return st;   // (after a rebuild on the device: the download of the host copy)
    if (int st = kf_culling_check_view(&g, view)) return st;
    KfcState &K = h->kfc;
    lm_take(h->M, lm_from_public(g, view), h->counts(), kLmView);
    K.has_view = true;
    K.dirty = true;
    return local_map_upload(h, kLmView);
}

int aos2_local_map_debug_culling_rounds(aos2_local_map_t *h, int rounds)
{
    if (!h) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    h->kfc.rounds = rounds <= 0 ? 0 : rounds;
    return AOS2_OK;
}

int aos2_local_map_last_culling_rounds(const aos2_local_map_t *h) { return h ? h->kfc.last_rounds : 0; }

int aos2_local_map_keyframe_culling(aos2_local_map_t *h, int monocular, int n_cand, const int32_t *cand, uint8_t *status,
                                    int32_t *n_mps, int32_t *n_redundant, int32_t *bad_points, int bad_cap, int32_t *n_bad_points)
{
    if (!h) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    KfcState &K = h->kfc;
    if (!K.has_view)
        return lm_fail("keyframe culling", "aos2_local_map_set_culling_view comes first (aos2_local_map_set drops the view)");
    int st;
    if ((st = kf_culling_check_call(h->n_kfs, n_cand, cand, status, n_mps, n_redundant, bad_points, bad_cap, n_bad_points))) return st;
    const size_t np = (size_t)h->n_points, n_obs = (size_t)h->n_obs, nc = (size_t)n_cand;
    // the overlay and the call's block, in the handle's scratch
    KfcOverlay X;
    KfcCall C = {};
    Regions<12> R;
    R.add(X.nobs, np); R.add(X.stamp, np); R.add(C.bad_rows, np); R.add(X.bad, np); R.add(X.erased, n_obs);
    R.add(C.cand, nc); R.add(C.c_mps, nc); R.add(C.c_red, nc);
    const size_t out0 = R.add(C.ctl, kCtlInts);
    R.add(C.n_mps, nc); R.add(C.n_red, nc); R.add(C.status, nc);
    const size_t out_bytes = R.bytes() - out0;
    if ((int64_t)R.bytes() > h->scratch_bytes)
        return lm_fail("keyframe culling", "%zu points and %zu observations need %zu bytes of scratch, the bound is %lld", np, n_obs,
                       R.bytes(), (long long)h->scratch_bytes);
    K.last_rounds = 0;
    K.timer.timed = false;
    *n_bad_points = 0;
    if (n_cand == 0) return AOS2_OK;
    if ((st = bind_device(h->device))) return st;
    if ((st = local_map_upload(h, kLmGraph)) || (st = local_map_upload(h, kLmView))) return st;
    if (!h->stream && (st = stream_create(&h->stream, false))) return st;
    if ((st = h->d_scratch.alloc((R.bytes() + 256) / 4))) return st;
    R.bind(reinterpret_cast<uint8_t *>(h->d_scratch.p));
    // page-locked: the candidates going in, the results block coming out, the bad rows behind it
    const size_t io_out = up256(nc * 4), io_bad = io_out + up256(out_bytes);
    if ((st = K.io.alloc(io_bad + np * 4 + 256))) return st;
    memcpy(K.io.p, cand, nc * 4);
    const LmGraph &G = h->G;
    C.n_cand = n_cand;
    C.monocular = monocular ? 1 : 0;
    hipStream_t q = h->stream;
    if ((st = K.timer.begin(q))) return st;
    AOS2_HIP_CHECK(hipMemcpyAsync(const_cast<int32_t *>(C.cand), K.io.p, nc * 4, hipMemcpyHostToDevice, q));
    const int init_blocks = (int)std::min<size_t>(1024, (std::max(np, n_obs) + kIT - 1) / kIT + 1);
    hipLaunchKernelGGL(k_kfc_init, dim3(init_blocks), dim3(kIT), 0, q, G, X, C, (int)n_obs);
    const int per_enqueue = K.rounds > 0 ? K.rounds : kRoundsDefault;
    const uint8_t *out = K.io.p + io_out;
    const int32_t *ctl = reinterpret_cast<const int32_t *>(out);
    for (;;) {
        for (int r = 0; r < per_enqueue; ++r) {
            hipLaunchKernelGGL(k_kfc_count, dim3(n_cand), dim3(kCT), 0, q, G, X, C);
            hipLaunchKernelGGL(k_kfc_apply, dim3(1), dim3(kAT), 0, q, G, X, C);
        }
        AOS2_HIP_CHECK(hipGetLastError());
        AOS2_HIP_CHECK(hipMemcpyAsync(K.io.p + io_out, C.ctl, out_bytes, hipMemcpyDeviceToHost, q));
        AOS2_HIP_CHECK(hipStreamSynchronize(q));
        if (ctl[kCursor] >= n_cand) break;
    }
    K.last_rounds = ctl[kRounds];
    memcpy(n_mps, span_copy(out, C.ctl, C.n_mps), nc * 4);
    memcpy(n_redundant, span_copy(out, C.ctl, C.n_red), nc * 4);
    memcpy(status, span_copy(out, C.ctl, C.status), nc);
    const int nb = ctl[kNBad];
    if (nb > 0) {   // in the order they went bad: sorted here, ascending row
        int32_t *rows = reinterpret_cast<int32_t *>(K.io.p + io_bad);
        AOS2_HIP_CHECK(hipMemcpyAsync(rows, C.bad_rows, (size_t)nb * 4, hipMemcpyDeviceToHost, q));
        AOS2_HIP_CHECK(hipStreamSynchronize(q));
        std::sort(rows, rows + nb);
        if (bad_cap > 0) memcpy(bad_points, rows, (size_t)std::min(nb, bad_cap) * 4);
    }
    *n_bad_points = nb;
    return K.timer.end(q, false);
}

int aos2_local_map_get_culling_view(const aos2_local_map_t *ch, aos2_kf_culling_view_t *view, int32_t *has_view)
{
    if (!ch || !view) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    aos2_local_map *h = const_cast<aos2_local_map *>(ch);
    *view = aos2_kf_culling_view_t{};
    if (has_view) *has_view = h->kfc.has_view ? 1 : 0;
    if (!h->kfc.has_view) return AOS2_OK;
    if (int st = local_map_refresh_host(h)) return st;
    lm_to_public(lm_data(h->M), nullptr, view);
    return AOS2_OK;
}

float aos2_local_map_last_culling_device_ms(aos2_local_map_t *h)
{
    return h ? h->kfc.timer.ms() : -1.f;
}

}  // extern "C"
