// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:636-700) over the resident graph of aos2_local_map_*: what csrc/kf_culling.hip
// shares with the host tap aos2_debug_keyframe_culling_host (csrc/debug_taps.hip) -- the argument checks and the three per-item
// functions (a feature's part in nMPs / nRedundantObservations, a candidate's verdict, a culled keyframe's erasure at one of its
// features).  The kernels call them with a lane per item, the tap in the loop's own order on one core.  They read the graph and
// the view through LmGraph (csrc/local_map_arrays.h), device or host addresses.  Internal to the library.
#pragma once
#include "aos2_common.h"
#include "local_map_arrays.h"

#if defined(__HIPCC__)
#define AOS2_KFC_HD __host__ __device__ __forceinline__
#else
#define AOS2_KFC_HD inline
#endif

namespace aos2 {

// What the culls of one call have changed so far.  The graph itself is never written: nobs and bad start as copies of point_nobs
// and point_bad, erased marks the observation entries that EraseObservation removed, stamp holds the last candidate whose erasure
// a point has taken (-1 = none), so that a point which sits at several features of a keyframe takes it once.
struct KfcOverlay {
    int32_t *nobs, *stamp;
    uint8_t *bad, *erased;
};

constexpr int kKfcThObs = 3;   // :651-652

// (single-writer updates: a point is claimed through its stamp before its nObs is touched; on the device they are atomics so
// that the claim of one lane orders the others)
AOS2_KFC_HD int kfc_exchange(int32_t *p, int v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicExch(p, v);
#else
    const int old = *p;
    *p = v;
    return old;
#endif
}
AOS2_KFC_HD int kfc_sub(int32_t *p, int v)   // the value before
{
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicSub(p, v);
#else
    const int old = *p;
    *p = old - v;
    return old;
#endif
}

// :655-695 for the feature at entry f of kf_mp, a feature of keyframe kf: bit 0 = it counts in nMPs, bit 1 = in
// nRedundantObservations
AOS2_KFC_HD int kfc_feature(const LmGraph &G, const KfcOverlay &X, int monocular, int kf, int f)
{
    const int pMP = G.kf_mp[f];
    if (pMP < 0) return 0;      // :658
    if (X.bad[pMP]) return 0;   // :660
    if (!monocular) {           // :662-666, the compare as written (a NaN depth passes both)
        const float d = G.kf_depth[f];
        if (d > G.kf_th_depth[kf] || d < 0) return 0;
    }
    int r = 1;   // :668
    if (X.nobs[pMP] > kKfcThObs) {   // :669  Observations() = nObs
        const int scaleLevel = G.kf_octave[f];
        int nObs = 0;
        const int e1 = G.obs_off[pMP + 1];
        for (int e = G.obs_off[pMP]; e < e1; ++e) {   // :674-687 (any order: the count stops at 3 whichever entries come first)
            if (X.erased[e]) continue;
            const int pKFi = G.obs_kf[e];
            if (pKFi == kf) continue;
            const int scaleLeveli = G.kf_octave[G.kf_mp_off[pKFi] + G.obs_idx[e]];
            if (scaleLeveli <= scaleLevel + 1) {
                nObs++;
                if (nObs >= kKfcThObs) break;
            }
        }
        if (nObs >= kKfcThObs) r |= 2;   // :688-691
    }
    return r;
}

// :647 and :697-698 with KeyFrame::SetBadFlag's own gate (src/KeyFrame.cc:518-524)
AOS2_KFC_HD int kfc_status(int flags, int nMPs, int nRedundantObservations)
{
    if (flags & 1) return AOS2_KFC_SKIPPED;
    if (!(nRedundantObservations > 0.9 * nMPs)) return AOS2_KFC_KEPT;
    return (flags & 2) ? AOS2_KFC_DEFERRED : AOS2_KFC_CULLED;
}

// KeyFrame::SetBadFlag (src/KeyFrame.cc:530-532) of candidate ci = keyframe kf, at entry f of kf_mp:
// mvpMapPoints[i]->EraseObservation(this) (src/MapPoint.cc:144-170).  Returns whether the point went bad here.
AOS2_KFC_HD bool kfc_erase(const LmGraph &G, const KfcOverlay &X, int kf, int ci, int f)
{
    const int pMP = G.kf_mp[f];
    if (pMP < 0) return false;
    if (kfc_exchange(&X.stamp[pMP], ci) == ci) return false;   // (the second call finds mObservations.count(pKF) == 0)
    const int e1 = G.obs_off[pMP + 1];
    for (int e = G.obs_off[pMP]; e < e1; ++e) {
        if (G.obs_kf[e] != kf) continue;   // (a keyframe is listed at most once per point)
        X.erased[e] = 1;
        const int dec = G.kf_stereo[G.kf_mp_off[kf] + G.obs_idx[e]] ? 2 : 1;   // :151-155  mvuRight[idx] of the OBSERVATION's feature
        const int left = kfc_sub(&X.nobs[pMP], dec) - dec;
        if (left <= 2 && !X.bad[pMP]) {   // :163-164
            X.bad[pMP] = 1;
            return true;
        }
        return false;
    }
    return false;   // :149  the point does not list the keyframe
}

// The checks of aos2_local_map_set_culling_view against the graph `g` (already checked): AOS2_OK or AOS2_ERR_ARG with the error
// text set.
int kf_culling_check_view(const aos2_local_map_graph_t *g, const aos2_kf_culling_view_t *v);
// The checks of aos2_local_map_keyframe_culling on its own arguments.
int kf_culling_check_call(int n_keyframes, int n_cand, const int32_t *cand, const uint8_t *status, const int32_t *n_mps,
                          const int32_t *n_redundant, const int32_t *bad_points, int bad_cap, const int32_t *n_bad_points);

}  // namespace aos2
