// Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) for frame batches: what csrc/local_map.hip shares with the host tap
// aos2_debug_local_map_host (csrc/debug_taps.hip), and the handle itself, which csrc/kf_culling.hip extends with the view and the
// scratch of LocalMapping::KeyFrameCulling.  Internal to the library; the public entry points are aos2_local_map_* and
// aos2_frames_update_local_map / aos2_frames_track_local_map_stats of include/aos2.h.
#pragma once
#include <vector>

#include "aos2_common.h"
#include "kf_culling.h"

namespace aos2 {

constexpr int kLmNeighbours = AOS2_LOCAL_MAP_NEIGHBOURS, kLmMaxKfs = AOS2_LOCAL_MAP_MAX_KFS;
constexpr int kLmLdsKfs = 8192;            // keyframes whose vote counters fit the workgroup's LDS (32 KiB)
constexpr int64_t kLmScratchBytes = (int64_t)256 << 20;

// The checks of aos2_local_map_set (include/aos2.h), made before a device is looked for: AOS2_OK or AOS2_ERR_ARG with the
// error text set.  *max_features (may be NULL) = the longest GetMapPointMatches() list.
int local_map_check(const aos2_local_map_graph_t *g, int *max_features);

struct LmGraphDev {
    int n_points, n_kfs;
    const uint8_t *point_bad, *kf_bad;
    const int32_t *point_nobs, *obs_off, *obs_kf, *kf_mp_off, *kf_mp, *kf_best, *kf_child_off, *kf_child, *kf_parent;
};

// the culling view of the handle (aos2_local_map_set_culling_view): host copies, the device block, the page-locked staging of
// one call's candidates and results
struct KfcState {
    bool has_view = false, dirty = true;
    std::vector<int32_t> obs_idx;
    std::vector<int8_t> kf_octave;
    std::vector<float> kf_depth, kf_th_depth;
    std::vector<uint8_t> kf_stereo, kf_flags;
    DevBuf<uint8_t> d_view;
    KfcGraph V = {};   // the six view arrays on the device (the graph's own come from LmGraphDev at the call)
    PinnedBuf<uint8_t> io;
    int rounds = 0;    // per enqueue, 0 = the default
    int last_rounds = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;   // around the last call's device work
    bool timed = false;
    void drop_view()
    {
        has_view = false;
        dirty = true;
    }
    ~KfcState()
    {
        d_view.release();
        io.release();
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

}  // namespace aos2

struct aos2_local_map {
    int device = 0;
    // the snapshot, host side (aos2_local_map_get hands these out)
    int n_points = 0, n_kfs = 0, max_features = 0;
    std::vector<uint8_t> point_bad, kf_bad;
    std::vector<int32_t> point_nobs, obs_off, obs_kf, kf_mp_off, kf_mp, kf_best, kf_child_off, kf_child, kf_parent;
    // ... and on the device
    bool dirty = true;
    aos2::LmGraphDev G = {};
    aos2::DevBuf<uint8_t> d_graph;
    aos2::DevBuf<int32_t> d_scratch;
    hipStream_t stream = nullptr;   // aos2_local_map_update (host arrays) runs here
    aos2::DevBuf<uint8_t> d_io;           // ... on device copies of its arrays
    int64_t scratch_bytes = aos2::kLmScratchBytes;
    int lds_kfs = aos2::kLmLdsKfs;
    int last_groups = 0;
    bool has_graph = false;   // aos2_local_map_set has been called
    aos2::KfcState kfc;
    // aos2_local_map_apply (csrc/local_map_apply.hip).  Always current on the host, each kept in O(delta): the counts above and
    // max_features, the entries of the three CSR arrays, and the length of every row (row_feat is Frame::N of each keyframe, the
    // bound of obs_idx).  The vectors above and the view's are the MIRROR: after a rebuild on the device they are stale until
    // local_map_refresh_host downloads the block.
    int64_t n_obs = 0, n_mp = 0, n_child = 0;
    std::vector<int32_t> row_obs, row_feat, row_child;
    bool host_stale = false;
    aos2::DevBuf<uint8_t> d_spare;          // the block the next rebuild writes; d_graph holds G (and V after a rebuild)
    size_t block_bytes = 0;                 // of the rebuilt block in d_graph, the span one download copies
    aos2::DevBuf<uint8_t> d_delta;
    aos2::PinnedBuf<uint8_t> delta_stage;
    int apply_tile = 0;                     // rows one workgroup scans, 0 = the default
    int last_apply_path = -1, last_apply_realloc = 0;
    hipEvent_t ap_ev0 = nullptr, ap_ev1 = nullptr;
    bool apply_timed = false;
    int64_t last_apply_bytes = 0;           // uploaded by the last device rebuild
};

namespace aos2 {

// the handle's graph on the device if it is not there yet (csrc/local_map.hip)
int local_map_upload(aos2_local_map *h);

// csrc/local_map_apply.hip
// The checks of aos2_local_map_apply against the handle's counts, O(delta): AOS2_OK or AOS2_ERR_ARG with the error text set.
int local_map_apply_check(const aos2_local_map *h, const aos2_local_map_delta_t *d);
// The rebuild written serially on the handle's host vectors (the mirror must be current); the delta has passed the check.
void local_map_apply_host(aos2_local_map *h, const aos2_local_map_delta_t *d);
// the row lengths and entry counts from the host vectors (after aos2_local_map_set)
void local_map_recount(aos2_local_map *h);
// the mirror from the device block if it is stale; AOS2_OK or AOS2_ERR_HIP
int local_map_refresh_host(aos2_local_map *h);

}  // namespace aos2
