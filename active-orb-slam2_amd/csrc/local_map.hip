// Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) and the tail of Tracking::TrackLocalMap (:1040-1071) for frame batches:
// the snapshot of Map that UpdateLocalMap reads -- the covisibility graph -- resident in HBM, and mvpLocalKeyFrames /
// mvpLocalMapPoints / mpReferenceKF of every frame of a device-resident batch in one call on the batch's stream, so that the
// list SearchLocalPoints searches never leaves the device.  Integer work only: every result is a function of the frame and the
// graph, whatever else is in the batch.  A workgroup per frame:
//   k_lm_keyframes  the votes as integer atomic adds on a counter per keyframe (LDS while n_keyframes fits, global scratch
//                   otherwise); the first list as an ordered compaction in ascending row, the reference keyframe as the maximum
//                   of (votes, lowest row); the counters then become the "in the list" marks and ONE wave walks the expansion
//                   (at most 81 iterations, serial by nature): lanes test the 10 neighbours, or 64 children, side by side and
//                   a ballot picks the first
//   k_lm_points     the local keyframes in list order, their matches in feature order = candidate positions; pass 1 takes the
//                   minimum position per point in a per-frame table, pass 2 keeps a candidate where it holds that minimum and
//                   compacts in candidate order
//   k_lm_stats      the statistics loop of TrackLocalMap, a lane per feature, wave sums
// The frames of a batch run in groups whose scratch fits a fixed bound, one group after the other on the stream.
#include <algorithm>
#include <vector>

#include "aos2_common.h"
#include "frames.h"
#include "lm_counters.h"
#include "local_map.h"
#include "wave_ops.h"

using namespace aos2;

namespace {

constexpr int kNT = 256;                 // threads of k_lm_keyframes and k_lm_stats
constexpr int kPT = 512;                 // threads of k_lm_points
constexpr int kLdsKfs = kLmLdsKfs;
constexpr int64_t kScratchBytes = kLmScratchBytes;

struct LmOut {
    int32_t *local, *n_local, *local_kfs, *n_local_kfs, *ref_kf;
    int local_cap, kf_cap;
};

// per group of frames: [G][n_kfs] counters (the global form only), [G][n_kfs] the whole keyframe list, [G] its length (-1 =
// no votes: the caller's list stands), [G][n_points] the smallest candidate position of every point
struct LmScratch {
    int32_t *cnt, *klist, *nk;
    uint32_t *minpos;
};

// one wave, all lanes: the first lane of `m` names the keyframe that joins the list
template <bool kLds>
__device__ __forceinline__ void lm_append(unsigned long long m, int cand, int32_t *klist, int32_t *mark, int &nl)
{
    const int a = __builtin_amdgcn_readlane(cand, __builtin_ctzll(m));
    if ((threadIdx.x & 63) == 0) {
        klist[nl] = a;
        lm_store<kLds>(mark + a, 1);
    }
    if constexpr (!kLds) __threadfence();   // (the lanes' next loads of the marks come behind this store)
    ++nl;
}

// Tracking::UpdateLocalKeyFrames (:1411-1519) for frame b0 + blockIdx.x.  The global counters are zero at entry.
template <bool kLds>
__global__ __launch_bounds__(kNT) void k_lm_keyframes(FramesDev S, LmGraph G, LmOut O, LmScratch X, int b0)
{
    __shared__ int32_t s_cnt[kLds ? kLdsKfs : 1];
    __shared__ int32_t s_wsum[kNT / 64];
    __shared__ int s_any, s_n;
    __shared__ unsigned long long s_best;
    const int g = blockIdx.x, b = b0 + g, tid = threadIdx.x;
    int32_t *cnt = kLds ? s_cnt : X.cnt + (size_t)g * G.n_kfs;
    int32_t *klist = X.klist + (size_t)g * G.n_kfs;
    if constexpr (kLds)
        for (int k = tid; k < G.n_kfs; k += kNT) cnt[k] = 0;
    if (tid == 0) {
        s_any = 0;
        s_best = 0ull;
    }
    __syncthreads();
    // :1415-1431  keyframeCounter[it->first]++ for every observation of every matched feature; a bad point leaves the frame
    const int n = max(0, min(S.n[b], S.cap));
    const size_t o = (size_t)b * S.cap;
    for (int i = tid; i < n; i += kNT) {
        const int row = S.mp[o + i];
        if (row < 0 || row >= G.n_points) continue;
        if (G.point_bad[row]) {
            S.mp[o + i] = -1;
            S.mp_state[o + i] = 0;
            continue;
        }
        const int e0 = G.obs_off[row], e1 = G.obs_off[row + 1];
        for (int e = e0; e < e1; ++e) atomicAdd(&cnt[G.obs_kf[e]], 1);
        if (e1 > e0) s_any = 1;
    }
    __threadfence();
    __syncthreads();
    if (!s_any) {   // :1433  keyframeCounter.empty(): mvpLocalKeyFrames and mpReferenceKF stay
        if (tid == 0) X.nk[g] = -1;
        return;
    }
    // :1443-1458  the voted keyframes in ascending row, bad ones skipped; pKFmax = the first strict maximum = the largest
    // (votes, lowest row).  cnt[k] becomes the mark "k is in the list" (mnTrackReferenceForFrame == mCurrentFrame.mnId)
    int n_first = 0;
    for (int base = 0; base < G.n_kfs; base += kNT) {
        const int k = base + tid;
        const int votes = k < G.n_kfs ? lm_load<kLds>(cnt + k) : 0;
        const bool keep = votes > 0 && !G.kf_bad[k];
        int total;
        const int pos = block_excl_scan_i32<kNT>(keep ? 1 : 0, s_wsum, total);
        if (keep) {
            klist[n_first + pos] = k;
            atomicMax(&s_best, ((unsigned long long)votes << 32) | (uint32_t)(0x7fffffff - k));
        }
        if (k < G.n_kfs) lm_store<kLds>(cnt + k, keep ? 1 : 0);
        n_first += total;
        __syncthreads();
    }
    __threadfence();
    __syncthreads();
    // :1462-1512  one wave: the keyframes of the first pass only, while the list holds at most 80
    if (tid < 64) {
        const int lane = tid;
        int nl = n_first;
        for (int it = 0; it < n_first; ++it) {
            if (nl > kLmMaxKfs) break;
            const int kf = klist[it];
            {   // the first of GetBestCovisibilityKeyFrames(10) that is not bad and not in the list
                const int nb = lane < kLmNeighbours ? G.kf_best[(size_t)kf * kLmNeighbours + lane] : -1;
                const bool ok = nb >= 0 && !G.kf_bad[nb] && !lm_load<kLds>(cnt + nb);
                const unsigned long long m = __ballot(ok);
                if (m) lm_append<kLds>(m, nb, klist, cnt, nl);
            }
            const int c1 = G.kf_child_off[kf + 1];
            for (int c0 = G.kf_child_off[kf]; c0 < c1; c0 += 64) {   // GetChilds() in ascending row, 64 at a time
                const int c = c0 + lane < c1 ? G.kf_child[c0 + lane] : -1;
                const bool ok = c >= 0 && !G.kf_bad[c] && !lm_load<kLds>(cnt + c);
                const unsigned long long m = __ballot(ok);
                if (m) {
                    lm_append<kLds>(m, c, klist, cnt, nl);
                    break;
                }
            }
            const int p = G.kf_parent[kf];   // GetParent(): no isBad() test, and its break leaves the OUTER loop
            if (p >= 0 && !lm_load<kLds>(cnt + p)) {
                lm_append<kLds>(~0ull, p, klist, cnt, nl);
                break;
            }
        }
        if (lane == 0) s_n = nl;
    }
    __threadfence();
    __syncthreads();
    const int nl = s_n;
    for (int j = tid; j < O.kf_cap; j += kNT) O.local_kfs[(size_t)b * O.kf_cap + j] = j < nl ? klist[j] : -1;
    if (tid == 0) {
        O.n_local_kfs[b] = nl;
        if (s_best) O.ref_kf[b] = 0x7fffffff - (int)(uint32_t)s_best;   // :1514-1518
        X.nk[g] = nl;
    }
}

// Tracking::UpdateLocalPoints (:1385-1408) for frame b0 + blockIdx.x.  The position table holds 0xffffffff ("no candidate yet") at entry.
__global__ __launch_bounds__(kPT) void k_lm_points(LmGraph G, LmOut O, LmScratch X, int b0)
{
    __shared__ int32_t s_wsum[kPT / 64];
    const int g = blockIdx.x, b = b0 + g, tid = threadIdx.x;
    int nk = X.nk[g];
    const int32_t *list = X.klist + (size_t)g * G.n_kfs;
    if (nk < 0) {   // no votes: the caller's mvpLocalKeyFrames
        list = O.local_kfs + (size_t)b * O.kf_cap;
        nk = max(0, min(O.n_local_kfs[b], O.kf_cap));
    }
    uint32_t *minpos = X.minpos + (size_t)g * G.n_points;
    uint32_t base = 0;
    for (int j = 0; j < nk; ++j) {
        const int kf = list[j];
        if (kf < 0 || kf >= G.n_kfs) continue;
        const int f0 = G.kf_mp_off[kf], nf = G.kf_mp_off[kf + 1] - f0;
        for (int i = tid; i < nf; i += kPT) {
            const int r = G.kf_mp[f0 + i];
            if (r >= 0 && !G.point_bad[r]) atomicMin(&minpos[r], base + (uint32_t)i);
        }
        base += (uint32_t)nf;
    }
    __threadfence();
    __syncthreads();
    int32_t *out = O.local + (size_t)b * O.local_cap;
    int nout = 0;
    base = 0;
    for (int j = 0; j < nk; ++j) {
        const int kf = list[j];
        if (kf < 0 || kf >= G.n_kfs) continue;
        const int f0 = G.kf_mp_off[kf], nf = G.kf_mp_off[kf + 1] - f0;
        for (int i0 = 0; i0 < nf; i0 += kPT) {
            const int i = i0 + tid;
            const int r = i < nf ? G.kf_mp[f0 + i] : -1;
            // mnTrackReferenceForFrame == mCurrentFrame.mnId (:1399): an earlier candidate was the same point
            const bool keep = r >= 0 && !G.point_bad[r] &&
                              __hip_atomic_load(&minpos[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == base + (uint32_t)i;
            int total;
            const int pos = block_excl_scan_i32<kPT>(keep ? 1 : 0, s_wsum, total);
            if (keep && nout + pos < O.local_cap) out[nout + pos] = r;
            nout += total;
            __syncthreads();
        }
        base += (uint32_t)nf;
    }
    for (int j = nout + tid; j < O.local_cap; j += kPT) out[j] = -1;
    if (tid == 0) O.n_local[b] = nout;
}

// :1040-1071 for frame blockIdx.x
__global__ __launch_bounds__(kNT) void k_lm_stats(FramesDev S, LmGraph G, int stereo, int only_tracking, int32_t *__restrict__ stats,
                                                  int32_t *__restrict__ found_inc)
{
    __shared__ int s_sum[3];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (tid < 3) s_sum[tid] = 0;
    __syncthreads();
    const int n = max(0, min(S.n[b], S.cap));
    const size_t o = (size_t)b * S.cap;
    int obsv = 0, inl = 0, tot = 0;
    for (int i = tid; i < n; i += kNT) {
        const int row = S.mp[o + i];
        if (row < 0 || row >= G.n_points) continue;
        ++obsv;
        if (!S.outlier[o + i]) {
            if (found_inc) atomicAdd(&found_inc[row], 1);
            if (!only_tracking) {
                const int nobs = G.point_nobs[row];
                if (nobs > 0) ++inl;
                tot += nobs;
            } else
                ++inl;
        } else if (stereo) {
            S.mp[o + i] = -1;
            S.mp_state[o + i] = 0;
        }
    }
    obsv = wave_sum_i32(obsv);
    inl = wave_sum_i32(inl);
    tot = wave_sum_i32(tot);
    if ((tid & 63) == 0) {
        atomicAdd(&s_sum[0], obsv);
        atomicAdd(&s_sum[1], inl);
        atomicAdd(&s_sum[2], tot);
    }
    __syncthreads();
    if (tid < 3) stats[3 * (size_t)b + tid] = s_sum[tid];
}

}  // namespace

namespace aos2 {

int lm_fail(const char *prefix, const char *fmt, ...)
{
    char msg[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof msg, fmt, ap);
    va_end(ap);
    set_error("%s: %s", prefix, msg);
    return AOS2_ERR_ARG;
}

bool lm_bad_offsets(const char *prefix, const int32_t *off, int n, const char *what)
{
    if (!off) return lm_fail(prefix, "%s is NULL", what);
    if (off[0] != 0) return lm_fail(prefix, "%s starts at %d", what, off[0]);
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return lm_fail(prefix, "%s decreases at row %d", what, i);
    return false;
}

bool lm_bad_values(const char *prefix, const int32_t *v, int64_t n, int lo, int hi, const char *what)
{
    if (n > 0 && !v) return lm_fail(prefix, "%s is NULL", what);
    for (int64_t i = 0; i < n; ++i)
        if (v[i] < lo || v[i] >= hi) return lm_fail(prefix, "%s[%lld] = %d is outside [%d, %d)", what, (long long)i, v[i], lo, hi);
    return false;
}

bool lm_listed_twice(const char *prefix, int n_rows, const int32_t *row_name, const int32_t *obs_off, const int32_t *obs_kf, int nk)
{
    std::vector<int32_t> seen(nk, -1);   // the row that listed a keyframe last
    for (int i = 0; i < n_rows; ++i)
        for (int e = obs_off[i]; e < obs_off[i + 1]; ++e) {
            if (seen[obs_kf[e]] == i) return lm_fail(prefix, "point %d lists keyframe %d twice", row_name ? row_name[i] : i, obs_kf[e]);
            seen[obs_kf[e]] = i;
        }
    return false;
}

int local_map_check(const aos2_local_map_graph_t *g, int *max_features)
{
    static const char *const pre = "local map";
    if (!g) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    const int np = g->n_points, nk = g->n_keyframes;
    if (np < 0 || nk < 0) return lm_fail(pre, "negative count (%d points, %d keyframes)", np, nk);
    const LmArrays<LmPtr> A = lm_from_public(*g, nullptr);
    LmCounts c = {(size_t)np, (size_t)nk, (size_t)nk, 0, 0, 0};   // the rows and offsets; the offsets then give the entries
    if (lm_null_with_length(A, c, kLmGraph)) return lm_fail(pre, "an array is NULL");
    if (lm_bad_offsets(pre, A.obs_off, np, "obs_off") || lm_bad_offsets(pre, A.kf_mp_off, nk, "kf_mp_off") ||
        lm_bad_offsets(pre, A.kf_child_off, nk, "kf_child_off"))
        return AOS2_ERR_ARG;
    c.obs = A.obs_off[np]; c.mp = A.kf_mp_off[nk]; c.child = A.kf_child_off[nk];
    if (lm_null_with_length(A, c, kLmGraph)) return lm_fail(pre, "an array is NULL");
    if (lm_bad_values(pre, A.obs_kf, c.obs, 0, nk, "obs_kf") || lm_bad_values(pre, A.kf_mp, c.mp, -1, np, "kf_mp") ||
        lm_bad_values(pre, A.kf_best, (int64_t)nk * kLmNeighbours, -1, nk, "kf_best") ||
        lm_bad_values(pre, A.kf_child, c.child, 0, nk, "kf_child") || lm_bad_values(pre, A.kf_parent, nk, -1, nk, "kf_parent"))
        return AOS2_ERR_ARG;
    if (lm_listed_twice(pre, np, nullptr, A.obs_off, A.obs_kf, nk)) return AOS2_ERR_ARG;
    int mf = 0;
    for (int k = 0; k < nk; ++k) mf = std::max(mf, A.kf_mp_off[k + 1] - A.kf_mp_off[k]);
    if (max_features) *max_features = mf;
    return AOS2_OK;
}

}  // namespace aos2

namespace aos2 {

int local_map_upload(aos2_local_map *h, int part)
{
    KfcState &K = h->kfc;
    bool &dirty = part == kLmGraph ? h->dirty : K.dirty;
    DevBuf<uint8_t> &buf = part == kLmGraph ? h->d_graph : K.d_view;
    if (!dirty) return AOS2_OK;
    if (int st = local_map_refresh_host(h)) return st;   // (the mirror is what goes up)
    // the other part's pointers stay -- unless that part is the view and is not on the device: NULL until its own upload, and
    // it lies in no block
    if (!K.has_view || K.dirty) K.in_graph_block = false;
    LmGraph G = K.has_view && (part == kLmView || !K.dirty) ? h->G : LmGraph{};
    G.n_points = h->n_points;
    G.n_kfs = h->n_kfs;
    Regions<11> R;
    lm_layout(R, G, h->counts(), part);
    std::vector<uint8_t> stage(R.bytes() + 256);
    R.bind(stage.data());
    lm_copy(G, lm_data(h->M), h->counts(), part);
    if (int st = bind_device(h->device)) return st;
    AOS2_HIP_CHECK(hipDeviceSynchronize());   // (a call that still reads the previous block)
    if (int st = buf.alloc(stage.size())) return st;
    AOS2_HIP_CHECK(hipMemcpy(buf.p, stage.data(), R.bytes(), hipMemcpyHostToDevice));
    R.bind(buf.p);
    h->G = G;
    if (part == kLmView) K.in_graph_block = false;
    dirty = false;
    return AOS2_OK;
}

}  // namespace aos2

extern "C" {

int aos2_local_map_create(int device, aos2_local_map_t **out)
{
    if (!out) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    aos2_local_map *h = new aos2_local_map();
    h->device = device;
    h->M.obs_off.assign(1, 0);
    h->M.kf_mp_off.assign(1, 0);
    h->M.kf_child_off.assign(1, 0);
    *out = h;
    return AOS2_OK;
}

void aos2_local_map_destroy(aos2_local_map_t *h)
{
    if (!h) return;
    if (h->d_graph.p || h->d_scratch.p || h->stream || h->d_spare.p || h->delta_stage.p) {
        (void)hipSetDevice(h->device);
        (void)hipDeviceSynchronize();
        h->d_graph.release();
        h->d_scratch.release();
        h->d_io.release();
        h->d_spare.release();
        h->d_delta.release();
        h->delta_stage.release();
        h->apply_timer.release();
        h->kfc.timer.release();
        h->conn.timer.release();
        h->nd.timer.release();
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

int aos2_local_map_set(aos2_local_map_t *h, const aos2_local_map_graph_t *g)
{
    if (!h) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    int mf = 0;
    if (int st = local_map_check(g, &mf)) return st;
    const int np = g->n_points, nk = g->n_keyframes;
    h->n_points = np;
    h->n_kfs = nk;
    h->max_features = mf;
    h->n_obs = g->obs_off[np]; h->n_mp = g->kf_mp_off[nk]; h->n_child = g->kf_child_off[nk];
    LmArrays<LmVec> &M = h->M;
    lm_take(M, lm_from_public(*g, nullptr), h->counts(), kLmGraph);
    // set<KeyFrame*> spChilds: ascending row stands for the pointer order, each child once
    for (int k = 0; k < nk; ++k) std::sort(M.kf_child.begin() + M.kf_child_off[k], M.kf_child.begin() + M.kf_child_off[k + 1]);
    h->dirty = true;
    h->has_graph = true;
    h->host_stale = false;   // (the mirror is the graph again)
    local_map_recount(h);
    h->kfc.has_view = false;   // (its arrays no longer line up with the graph)
    h->kfc.dirty = true;
    return local_map_upload(h, kLmGraph);
}

int aos2_local_map_get(const aos2_local_map_t *ch, aos2_local_map_graph_t *g)
{
    if (!ch) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    aos2_local_map *h = const_cast<aos2_local_map *>(ch);   // (the graph is not changed: the host mirror of it may be refreshed)
    if (g) {
        if (int st = local_map_refresh_host(h)) return st;
        g->n_points = h->n_points;
        g->n_keyframes = h->n_kfs;
        lm_to_public(lm_data(h->M), g, nullptr);
    }
    return AOS2_OK;
}

int aos2_local_map_debug_limits(aos2_local_map_t *h, int64_t scratch_bytes, int lds_keyframes)
{
    if (!h || lds_keyframes > kLdsKfs) {
        set_error("bad argument (at most %d keyframes have their counters in LDS)", kLdsKfs);
        return AOS2_ERR_ARG;
    }
    h->scratch_bytes = scratch_bytes <= 0 ? kScratchBytes : scratch_bytes;
    h->lds_kfs = lds_keyframes < 0 ? kLdsKfs : lds_keyframes;
    return AOS2_OK;
}

int aos2_local_map_last_groups(const aos2_local_map_t *h) { return h ? h->last_groups : 0; }

// the checks that come before anything is enqueued, the upload if it is due, and the launches of one call on stream q: S names
// n, cap, mp and mp_state of the frames, O the five arrays
static int enqueue_update(aos2_local_map *h, const FramesDev &S, const LmOut &O, hipStream_t q)
{
    // the bound: one frame's tables, and 32-bit candidate positions
    const int64_t np = h->n_points, nk = h->n_kfs;
    const int64_t per_frame = 4 * (np + 2 * nk) + 4;
    if (per_frame > h->scratch_bytes)
        return lm_fail("local map", "%lld points and %lld keyframes need %lld bytes of scratch per frame, the bound is %lld",
                       (long long)np, (long long)nk, (long long)per_frame, (long long)h->scratch_bytes);
    if (std::max<int64_t>(nk, O.kf_cap) * h->max_features >= ((int64_t)1 << 31) - 1)
        return lm_fail("local map", "%lld keyframes of up to %d features exceed the 32-bit candidate positions",
                       (long long)std::max<int64_t>(nk, O.kf_cap), h->max_features);
    int st;
    if ((st = local_map_upload(h, kLmGraph))) return st;
    const int B = S.batch;
    const int group = (int)std::min<int64_t>(B, h->scratch_bytes / per_frame);
    LmScratch X;
    Regions<4> R;
    R.add(X.cnt, (size_t)group * nk); R.add(X.klist, (size_t)group * nk); R.add(X.nk, group); R.add(X.minpos, (size_t)group * np);
    if ((st = h->d_scratch.alloc((R.bytes() + 256) / 4))) return st;
    R.bind(reinterpret_cast<uint8_t *>(h->d_scratch.p));
    const bool lds = h->n_kfs <= h->lds_kfs;
    h->last_groups = 0;
    for (int b0 = 0; b0 < B; b0 += group) {
        const int gs = std::min(group, B - b0);
        if (np) AOS2_HIP_CHECK(hipMemsetAsync(X.minpos, 0xff, (size_t)gs * np * 4, q));
        if (!lds && nk) AOS2_HIP_CHECK(hipMemsetAsync(X.cnt, 0, (size_t)gs * nk * 4, q));
        if (lds) hipLaunchKernelGGL(k_lm_keyframes<true>, dim3(gs), dim3(kNT), 0, q, S, h->G, O, X, b0);
        else hipLaunchKernelGGL(k_lm_keyframes<false>, dim3(gs), dim3(kNT), 0, q, S, h->G, O, X, b0);
        hipLaunchKernelGGL(k_lm_points, dim3(gs), dim3(kPT), 0, q, h->G, O, X, b0);
        AOS2_HIP_CHECK(hipGetLastError());
        ++h->last_groups;
    }
    return AOS2_OK;
}

int aos2_frames_update_local_map(aos2_frames_t *f, const aos2_local_map_t *cm, int32_t *d_local, int local_cap, int32_t *d_n_local,
                                 int32_t *d_local_kfs, int kf_cap, int32_t *d_n_local_kfs, int32_t *d_ref_kf)
{
    aos2_local_map *h = const_cast<aos2_local_map *>(cm);   // (the snapshot is not changed: its upload and the scratch are)
    if (!f || !h || !f->dev_ready || !f->D.n || !d_local || !d_n_local || !d_local_kfs || !d_n_local_kfs || !d_ref_kf || local_cap <= 0 ||
        kf_cap <= 0) {
        set_error("bad argument (aos2_frames_build comes first; five device arrays of positive capacity)");
        return AOS2_ERR_ARG;
    }
    if (f->device != h->device)
        return lm_fail("local map", "the batch is on device %d, the graph on device %d", f->device, h->device);
    if (int st = bind_device(f->device)) return st;
    const LmOut O = {d_local, d_n_local, d_local_kfs, d_n_local_kfs, d_ref_kf, local_cap, kf_cap};
    return enqueue_update(h, f->D, O, f->stream);
}

int aos2_local_map_update(aos2_local_map_t *h, int batch, int cap, const int32_t *n, int32_t *mp, int32_t *local, int local_cap,
                          int32_t *n_local, int32_t *local_kfs, int kf_cap, int32_t *n_local_kfs, int32_t *ref_kf)
{
    if (!h || batch < 0 || cap <= 0 || local_cap <= 0 || kf_cap <= 0 ||
        (batch > 0 && (!n || !mp || !local || !n_local || !local_kfs || !n_local_kfs || !ref_kf))) {
        set_error("bad argument");
        return AOS2_ERR_ARG;
    }
    if (batch == 0) return AOS2_OK;
    int st = bind_device(h->device);
    if (st) return st;
    if (!h->stream && (st = stream_create(&h->stream, false))) return st;
    const size_t B = (size_t)batch;
    FramesDev S = {};
    int32_t *d_n;
    LmOut O = {nullptr, nullptr, nullptr, nullptr, nullptr, local_cap, kf_cap};
    Regions<8> R;
    R.add(d_n, B); R.add(S.mp, B * cap); R.add(S.mp_state, B * cap); R.add(O.local, B * local_cap); R.add(O.n_local, B);
    R.add(O.local_kfs, B * kf_cap); R.add(O.n_local_kfs, B); R.add(O.ref_kf, B);
    if ((st = h->d_io.alloc(R.bytes() + 256))) return st;
    R.bind(h->d_io.p);
    S.batch = batch; S.cap = cap; S.n = d_n;
    hipStream_t q = h->stream;
    AOS2_HIP_CHECK(hipMemcpyAsync(d_n, n, B * 4, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(S.mp, mp, B * cap * 4, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(O.local_kfs, local_kfs, B * kf_cap * 4, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(O.n_local_kfs, n_local_kfs, B * 4, hipMemcpyHostToDevice, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(O.ref_kf, ref_kf, B * 4, hipMemcpyHostToDevice, q));
    if ((st = enqueue_update(h, S, O, q))) {
        (void)hipStreamSynchronize(q);   // (the copies read the caller's arrays)
        return st;
    }
    AOS2_HIP_CHECK(hipMemcpyAsync(mp, S.mp, B * cap * 4, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(local, O.local, B * local_cap * 4, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(n_local, O.n_local, B * 4, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(local_kfs, O.local_kfs, B * kf_cap * 4, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(n_local_kfs, O.n_local_kfs, B * 4, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipMemcpyAsync(ref_kf, O.ref_kf, B * 4, hipMemcpyDeviceToHost, q));
    AOS2_HIP_CHECK(hipStreamSynchronize(q));
    return AOS2_OK;
}

int aos2_frames_track_local_map_stats(aos2_frames_t *f, const aos2_local_map_t *cm, int stereo, int only_tracking, int32_t *d_stats,
                                      int32_t *d_found_inc)
{
    aos2_local_map *h = const_cast<aos2_local_map *>(cm);
    if (!f || !h || !f->dev_ready || !f->D.n || !d_stats || f->device != h->device) {
        set_error("bad argument (aos2_frames_build comes first; the batch and the graph on one device)");
        return AOS2_ERR_ARG;
    }
    int st = bind_device(f->device);
    if (st) return st;
    if ((st = local_map_upload(h, kLmGraph))) return st;
    hipLaunchKernelGGL(k_lm_stats, dim3(f->D.batch), dim3(kNT), 0, f->stream, f->D, h->G, stereo ? 1 : 0, only_tracking ? 1 : 0, d_stats,
                       d_found_inc);
    AOS2_HIP_CHECK(hipGetLastError());
    return AOS2_OK;
}

}  // extern "C"
