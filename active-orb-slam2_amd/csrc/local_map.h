// Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) for frame batches: what csrc/local_map.hip shares with the host tap
// aos2_debug_local_map_host (csrc/debug_taps.hip), and the handle itself, which csrc/kf_culling.hip extends with the view and the
// scratch of LocalMapping::KeyFrameCulling, csrc/connections.hip and csrc/normal_depth.hip with the state of their calls, and
// csrc/local_map_apply.hip rebuilds.  The resident arrays are those of csrc/local_map_arrays.h.  Internal to the library; the
// public entry points are aos2_local_map_* and aos2_frames_update_local_map / aos2_frames_track_local_map_stats of include/aos2.h.
#pragma once
#include <vector>

#include "aos2_common.h"
#include "kf_culling.h"
#include "local_map_arrays.h"

namespace aos2 {

static_assert(kLmNeighbours == AOS2_LOCAL_MAP_NEIGHBOURS, "csrc/local_map_arrays.h and include/aos2.h disagree");
constexpr int kLmMaxKfs = AOS2_LOCAL_MAP_MAX_KFS;
constexpr int kLmLdsKfs = 8192;            // keyframes whose vote counters fit the workgroup's LDS (32 KiB)
constexpr int64_t kLmScratchBytes = (int64_t)256 << 20;

// The public structs have their own field order and a separate view: to and from the internal arrays here, nowhere else.  G =
// aos2_local_map_graph_t or aos2_local_map_delta_t (the same member names); g and v may be NULL.
template <class G>
inline LmArrays<LmPtr> lm_from_public(const G &g, const aos2_kf_culling_view_t *v)
{
    LmArrays<LmPtr> A = {};
    const auto take = [](auto &dst, auto &src, LmLen, auto) { dst = src; };
    lm_each_graph(A, g, take);
    if (v) lm_each_view(A, *v, take);
    return A;
}
inline void lm_to_public(const LmArrays<LmPtr> &A, aos2_local_map_graph_t *g, aos2_kf_culling_view_t *v)
{
    const auto give = [](auto &src, auto &dst, LmLen, auto) { dst = src; };
    if (g) lm_each_graph(A, *g, give);
    if (v) lm_each_view(A, *v, give);
}

// The argument checks that aos2_local_map_set, aos2_local_map_set_culling_view and aos2_local_map_apply share
// (csrc/local_map.hip).  Each returns true with the error text "<prefix>: ..." set, through lm_fail, which returns AOS2_ERR_ARG.
int lm_fail(const char *prefix, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
// CSR offsets over n rows: start at 0, do not decrease
bool lm_bad_offsets(const char *prefix, const int32_t *off, int n, const char *what);
// every value inside [lo, hi)
bool lm_bad_values(const char *prefix, const int32_t *v, int64_t n, int lo, int hi, const char *what);
// a keyframe (of nk) listed twice in one of n_rows observation rows, the first in listing order; row_name (may be NULL: the row
// itself) is what the text calls a row.  O(entries + nk): a mark per keyframe of the map.
bool lm_listed_twice(const char *prefix, int n_rows, const int32_t *row_name, const int32_t *obs_off, const int32_t *obs_kf, int nk);
// obs_idx of every entry inside the feature count of its keyframe, which features_of(kf) gives
template <class Nf>
inline bool lm_bad_obs_idx(const char *prefix, int n_rows, const int32_t *row_name, const int32_t *obs_off, const int32_t *obs_kf,
                           const int32_t *obs_idx, Nf &&features_of)
{
    for (int i = 0; i < n_rows; ++i)
        for (int e = obs_off[i]; e < obs_off[i + 1]; ++e) {
            const int kf = obs_kf[e], nf = features_of(kf);
            if (obs_idx[e] < 0 || obs_idx[e] >= nf)
                return lm_fail(prefix, "obs_idx[%d] = %d of point %d is outside the %d features of keyframe %d", e, obs_idx[e],
                               row_name ? row_name[i] : i, nf, kf);
        }
    return false;
}

// The checks of aos2_local_map_set (include/aos2.h), made before a device is looked for: AOS2_OK or AOS2_ERR_ARG with the
// error text set.  *max_features (may be NULL) = the longest GetMapPointMatches() list.
int local_map_check(const aos2_local_map_graph_t *g, int *max_features);

// device time between two events on a stream; the events are created on first use
struct EventTimer {
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    int begin(hipStream_t q)
    {
        timed = false;
        if (!ev0) {
            AOS2_HIP_CHECK(hipEventCreate(&ev0));
            AOS2_HIP_CHECK(hipEventCreate(&ev1));
        }
        AOS2_HIP_CHECK(hipEventRecord(ev0, q));
        return AOS2_OK;
    }
    int end(hipStream_t q, bool wait)   // wait: for the stream, and nothing counts as timed unless that succeeds
    {
        AOS2_HIP_CHECK(hipEventRecord(ev1, q));
        if (wait) AOS2_HIP_CHECK(hipStreamSynchronize(q));
        timed = true;
        return AOS2_OK;
    }
    float ms() const   // -1: nothing was timed
    {
        float ms = 0.f;
        if (!timed || hipEventSynchronize(ev1) != hipSuccess || hipEventElapsedTime(&ms, ev0, ev1) != hipSuccess) return -1.f;
        return ms;
    }
    void release()
    {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
        ev0 = ev1 = nullptr;
    }
};

// what is specific to culling (aos2_local_map_set_culling_view, aos2_local_map_keyframe_culling): the state of the view, its own
// device block, the page-locked staging of one call's candidates and results
struct KfcState {
    bool has_view = false, dirty = true;
    // Where the view's device arrays (the handle's G.obs_idx .. G.kf_flags) lie: in d_view after an upload of the view, behind
    // the graph in the handle's d_graph after a rebuild on the device.
    bool in_graph_block = false;
    DevBuf<uint8_t> d_view;
    PinnedBuf<uint8_t> io;
    int rounds = 0;    // per enqueue, 0 = the default
    int last_rounds = 0;
    EventTimer timer;   // around the last call's device work
    ~KfcState()
    {
        d_view.release();
        io.release();
    }
};

// what is specific to aos2_local_map_update_connections (csrc/connections.hip): the device block of one call's arguments and
// results, its page-locked staging, the sort switch
struct ConnState {
    DevBuf<uint8_t> d_io;
    PinnedBuf<uint8_t> io;
    int lds_entries = 0;   // ordered lists up to this length are sorted in LDS, 0 = the default
    EventTimer timer;      // around the last call's device work
    ~ConnState()
    {
        d_io.release();
        io.release();
    }
};

// what is specific to aos2_local_map_update_normal_depth (csrc/normal_depth.hip): the device block of one call's arguments and
// results, its page-locked staging, the switch between the two places where the thetas wait
struct NdState {
    DevBuf<uint8_t> d_io;
    PinnedBuf<uint8_t> io;
    int lds_terms = -1;   // observation lists up to this length keep their thetas in LDS, < 0 = the default
    EventTimer timer;     // around the last call's device work
    ~NdState()
    {
        d_io.release();
        io.release();
    }
};

}  // namespace aos2

struct aos2_local_map {
    int device = 0;
    int n_points = 0, n_kfs = 0, max_features = 0;
    // the snapshot, host side (aos2_local_map_get and aos2_local_map_get_culling_view hand these out)
    aos2::LmArrays<aos2::LmVec> M;
    // ... and on the device: the view's pointers are NULL without a view
    bool dirty = true;
    aos2::LmGraph G = {};
    aos2::DevBuf<uint8_t> d_graph;
    aos2::DevBuf<int32_t> d_scratch;
    hipStream_t stream = nullptr;   // aos2_local_map_update (host arrays) runs here
    aos2::DevBuf<uint8_t> d_io;           // ... on device copies of its arrays
    int64_t scratch_bytes = aos2::kLmScratchBytes;
    int lds_kfs = aos2::kLmLdsKfs;
    int last_groups = 0;
    bool has_graph = false;   // aos2_local_map_set has been called
    aos2::KfcState kfc;
    aos2::ConnState conn;
    aos2::NdState nd;
    // aos2_local_map_apply (csrc/local_map_apply.hip).  Always current on the host, each kept in O(delta): the counts above and
    // max_features, the entries of the three CSR arrays, and the length of every row (row_feat is Frame::N of each keyframe, the
    // bound of obs_idx).  M is the MIRROR: after a rebuild on the device it is stale until local_map_refresh_host downloads the
    // block.
    int64_t n_obs = 0, n_mp = 0, n_child = 0;
    std::vector<int32_t> row_obs, row_feat, row_child;
    bool host_stale = false;
    aos2::DevBuf<uint8_t> d_spare;          // the block the next rebuild writes
    size_t block_bytes = 0;                 // of the rebuilt block in d_graph, the span one download copies
    aos2::DevBuf<uint8_t> d_delta;
    aos2::PinnedBuf<uint8_t> delta_stage;
    int apply_tile = 0;                     // rows one workgroup scans, 0 = the default
    int last_apply_path = -1, last_apply_realloc = 0;
    aos2::EventTimer apply_timer;
    int64_t last_apply_bytes = 0;           // uploaded by the last device rebuild

    aos2::LmCounts counts() const
    {
        return aos2::LmCounts{(size_t)n_points, (size_t)n_kfs, (size_t)n_kfs, (size_t)n_obs, (size_t)n_mp, (size_t)n_child};
    }
    int view_part() const { return kfc.has_view ? aos2::kLmView : 0; }
};

namespace aos2 {

// One part of the handle's mirror on the device if it is not there yet (csrc/local_map.hip): the graph (kLmGraph) as one block in
// d_graph, or the view (kLmView) in the block of its own, each copied in one piece.
int local_map_upload(aos2_local_map *h, int part);

// csrc/local_map_apply.hip
// The checks of aos2_local_map_apply against the handle's counts, O(delta + n_keyframes), the graph is not read: AOS2_OK or
// AOS2_ERR_ARG with the error text set.
int local_map_apply_check(const aos2_local_map *h, const aos2_local_map_delta_t *d);
// The rebuild written serially on the handle's mirror (which must be current); the delta has passed the check.
void local_map_apply_host(aos2_local_map *h, const aos2_local_map_delta_t *d);
// the row lengths and entry counts from the mirror (after aos2_local_map_set)
void local_map_recount(aos2_local_map *h);
// the mirror from the device block if it is stale; AOS2_OK or AOS2_ERR_HIP
int local_map_refresh_host(aos2_local_map *h);

}  // namespace aos2
