// Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) for frame batches: what csrc/local_map.hip shares with the host tap
// aos2_debug_local_map_host (csrc/debug_taps.hip).  Internal to the library; the public entry points are aos2_local_map_* and
// aos2_frames_update_local_map / aos2_frames_track_local_map_stats of include/aos2.h.
#pragma once
#include "aos2_common.h"

namespace aos2 {

constexpr int kLmNeighbours = AOS2_LOCAL_MAP_NEIGHBOURS, kLmMaxKfs = AOS2_LOCAL_MAP_MAX_KFS;

// The checks of aos2_local_map_set (include/aos2.h), made before a device is looked for: AOS2_OK or AOS2_ERR_ARG with the
// error text set.  *max_features (may be NULL) = the longest GetMapPointMatches() list.
int local_map_check(const aos2_local_map_graph_t *g, int *max_features);

}  // namespace aos2
