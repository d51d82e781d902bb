// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:636-700) at the reference's call site, the last step of the loop body of
// LocalMapping::Run (:87):
//
//     // after LocalBundleAdjustment, under mpMap->mMutexMapUpdate like the optimiser's own writes; the view is gathered in the same
//     // walk as the graph, so that its arrays line up:
//     aos2::LocalMapSnapshot snapshot(mpMap, mpMap->GetAllMapPoints(), aos2::CullingView());
//     aos2::KeyFrameCulling(mpCurrentKeyFrame, mbMonocular, snapshot);          // instead of KeyFrameCulling();
//
// One C-ABI call (aos2_local_map_keyframe_culling) gives the verdict of every covisible keyframe as the serial loop would reach it
// -- after the erasures of every keyframe culled before it -- and pKF->SetBadFlag() is then called in candidate order for the
// redundant ones (with mbNotErase set it only marks mbToBeErased, as in the reference): the erasure from the observations, the
// points that go bad, the covisibility graph and the spanning tree are updated by the reference's own code, unchanged.  The
// snapshot is NOT updated: name the keyframes that went bad (and what their erasure touched) in the LocalMapSnapshot::Apply that ends
// the pass, as after every other map change (host/LocalMap.h).  A keyframe of
// GetVectorCovisibleKeyFrames() that the snapshot does not know (added after it was taken) is left out of the call, like
// aos2::UpdateLocalMap leaves one out.  Include AFTER the headers that declare Map, KeyFrame and MapPoint (the reference's, or
// tests/cpp/refstub/kf_culling_stub.h).
#pragma once
#include <cstdint>
#include <mutex>
#include <vector>

#include "LocalMap.h"

namespace aos2 {

// KeyFrame::mbNotErase / mbToBeErased of an UNCHANGED reference KeyFrame: protected (include/KeyFrame.h:236-237), read through
// a member pointer formed in a derived class, under mMutexConnections like SetBadFlag's own read (see MapPointDistances).
template <class KF>
struct KeyFrameEraseFlags : KF {
    static bool NotErase(KF *p)
    {
        std::unique_lock<std::mutex> lock(p->*(&KeyFrameEraseFlags::mMutexConnections));
        return p->*(&KeyFrameEraseFlags::mbNotErase);
    }
    static bool ToBeErased(KF *p)
    {
        std::unique_lock<std::mutex> lock(p->*(&KeyFrameEraseFlags::mMutexConnections));
        return p->*(&KeyFrameEraseFlags::mbToBeErased);
    }
};

// aos2_kf_culling_view_t gathered by LocalMapSnapshot's walk
class CullingView {
public:
    static constexpr bool kGathers = true;
    template <class KF>
    void KeyFrame(KF *pKF)
    {
        DeltaMatches(pKF);
        DeltaLinks(pKF);
    }
    void Observation(size_t idx) { obs_idx.push_back((int32_t)idx); }
    // the hooks of LocalMapSnapshot::Apply: the same gathers for the rows of a delta -- what is parallel to a match row, and the two
    // scalars of a link row -- and the delta pointed at them
    void DeltaObservation(size_t idx) { Observation(idx); }
    template <class KF>
    void DeltaMatches(KF *pKF)
    {
        const size_t n = pKF->GetMapPointMatches().size();
        for (size_t i = 0; i < n; ++i) {
            kf_octave.push_back((int8_t)pKF->mvKeysUn[i].octave);
            kf_depth.push_back(pKF->mvDepth[i]);
            kf_stereo.push_back(pKF->mvuRight[i] >= 0 ? 1 : 0);
        }
    }
    template <class KF>
    void DeltaLinks(KF *pKF)
    {
        kf_th_depth.push_back(pKF->mThDepth);
        kf_flags.push_back((uint8_t)((pKF->mnId == 0 ? 1 : 0) | (KeyFrameEraseFlags<KF>::NotErase(pKF) ? 2 : 0)));
    }
    void PointDelta(aos2_local_map_delta_t &d)
    {
        mView.obs_idx = obs_idx.data(); mView.kf_octave = kf_octave.data(); mView.kf_depth = kf_depth.data();
        mView.kf_stereo = kf_stereo.data(); mView.kf_th_depth = kf_th_depth.data(); mView.kf_flags = kf_flags.data();
        d.view = &mView;
    }
    void Set(aos2_local_map_t *h)
    {
        aos2_kf_culling_view_t v;
        v.obs_idx = obs_idx.data(); v.kf_octave = kf_octave.data(); v.kf_depth = kf_depth.data(); v.kf_stereo = kf_stereo.data();
        v.kf_th_depth = kf_th_depth.data(); v.kf_flags = kf_flags.data();
        check(aos2_local_map_set_culling_view(h, &v), "CullingView");
    }

private:
    std::vector<int32_t> obs_idx;
    std::vector<int8_t> kf_octave;
    std::vector<float> kf_depth, kf_th_depth;
    std::vector<uint8_t> kf_stereo, kf_flags;
    aos2_kf_culling_view_t mView = {};
};

// The loop :644-699.  vStatus (may be NULL): AOS2_KFC_* of every keyframe of GetVectorCovisibleKeyFrames(), in its order
// (AOS2_KFC_KEPT for one the snapshot does not know).
inline void KeyFrameCulling(ORB_SLAM2::KeyFrame *pCurrentKeyFrame, bool bMonocular, const LocalMapSnapshot &S,
                            std::vector<uint8_t> *vStatus = nullptr)
{
    ShimClock clk;
    const std::vector<ORB_SLAM2::KeyFrame *> vpLocalKeyFrames = pCurrentKeyFrame->GetVectorCovisibleKeyFrames();
    std::vector<int32_t> cand;
    std::vector<size_t> where;
    for (size_t j = 0; j < vpLocalKeyFrames.size(); ++j) {
        const int32_t r = S.KeyFrameRow(vpLocalKeyFrames[j]);
        if (r < 0) continue;
        cand.push_back(r);
        where.push_back(j);
    }
    const int n = (int)cand.size();
    std::vector<uint8_t> status(n + 1, AOS2_KFC_KEPT);
    std::vector<int32_t> n_mps(n + 1, 0), n_redundant(n + 1, 0);
    int32_t n_bad = 0;
    last_shim_timing().gather_us = clk.lap();
    check(aos2_local_map_keyframe_culling(S.Handle(), bMonocular ? 1 : 0, n, cand.data(), status.data(), n_mps.data(), n_redundant.data(),
                                          nullptr, 0, &n_bad),
          "KeyFrameCulling");
    last_shim_timing().call_us = clk.lap();
    if (vStatus) vStatus->assign(vpLocalKeyFrames.size(), AOS2_KFC_KEPT);
    for (int j = 0; j < n; ++j) {
        if (vStatus) (*vStatus)[where[j]] = status[j];
        if (status[j] == AOS2_KFC_CULLED || status[j] == AOS2_KFC_DEFERRED) vpLocalKeyFrames[where[j]]->SetBadFlag();   // :698
    }
    last_shim_timing().scatter_us = clk.lap();
}

}  // namespace aos2
