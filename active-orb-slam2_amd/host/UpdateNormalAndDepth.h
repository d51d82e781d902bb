// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:363-413) at the reference's call sites, for one point or a batch:
//
//     // LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:156), once per point of the new keyframe: the snapshot must know the
//     // new keyframe and its AddObservation()s, so Apply the keyframe and its matched points first (host/LocalMap.h), then ONE call
//     // behind the loop instead of one per point:
//     snapshot.Apply({mpCurrentKeyFrame}, {mpCurrentKeyFrame}, vpMatchedMPs, mpMap->GetAllMapPoints(), aos2::CullingView());
//     aos2::UpdateNormalAndDepth(vpMatchedMPs, snapshot);
//
//     // LocalMapping::CreateNewMapPoints (:448) and Tracking's new points (src/Tracking.cc:628, :764, :1298): the new points are
//     // appended to the table and named in the Apply, then one call for all of them.
//     // LocalMapping::SearchInNeighbors (:531), every point of the current keyframe behind Fuse: the same Apply that
//     // aos2::UpdateConnections needs at :537 (host/UpdateConnections.h) serves both.
//
//     // Optimizer::LocalBundleAdjustment (src/Optimizer.cc:777), GlobalBundleAdjustemnt (:227), OptimizeEssentialGraph (:1043) and
//     // LoopClosing::CorrectLoop (src/LoopClosing.cc:502): only positions and poses changed, the observations did not, so NO Apply
//     // is needed -- SetWorldPos / SetPose first, then one call for the window's (3-6 k) or the map's (10^5) points:
//     aos2::UpdateNormalAndDepth(lLocalMapPoints, snapshot);
//
// The snapshot must have been taken WITH a view (aos2::CullingView: it carries the feature of every observation and the octave of
// every feature).  One C-ABI call (aos2_local_map_update_normal_depth) takes GetWorldPos() and the row of GetReferenceKeyFrame() of
// every point and GetCameraCenter() of every keyframe of the snapshot, and the scale table of its first keyframe (mvScaleFactors is
// the same in all).  For the points the call reports as updated, and only for them, the members are written as :404-411 writes
// them: mNormalVector, mfMinDistance and mfMaxDistance under mMutexPos -- protected, reached through member pointers formed in a
// derived class, as aos2::MapPointDistances reads them -- theta_mean and theta_std, and the per-observation mNormalVectors and
// theta_sVector.  A bad point, one without observations (:371, :378) and one the snapshot does not know keep every member; so does
// a point whose reference keyframe the snapshot does not know or cannot be read at the observed feature, where the reference would
// read out of bounds.  Keyframe rows stand for pointer order: the sums run over the observers in
// ascending mnId.  Include AFTER the headers that declare Map, KeyFrame, MapPoint and Frame (the reference's, or
// tests/cpp/refstub/normal_depth_stub.h).
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "LocalMap.h"

namespace aos2 {

// The members of an UNCHANGED reference MapPoint that :404-411 writes: mNormalVector, mfMinDistance and mfMaxDistance are protected
// (include/MapPoint.h:132, 149-150), theta_mean and theta_std public; all five under mMutexPos, as there.
template <class MP>
struct MapPointNormalDepthMembers : MP {
    static void Assign(MP *p, const float *normal, float min_dist, float max_dist, float mean, float stdev)
    {
        using M = MapPointNormalDepthMembers;
        cv::Mat n(3, 1, CV_32F);
        for (int c = 0; c < 3; ++c) n.at<float>(c) = normal[c];
        std::unique_lock<std::mutex> lock3(p->*(&M::mMutexPos));
        p->*(&M::mfMaxDistance) = max_dist;
        p->*(&M::mfMinDistance) = min_dist;
        p->*(&M::mNormalVector) = n;
        p->theta_mean = mean;
        p->theta_std = stdev;
    }
};

// vStatus (may be NULL): AOS2_ND_* of every point of the vector, in its order (AOS2_ND_UNKNOWN for a NULL, for a point outside the
// snapshot's table and for one whose reference keyframe the snapshot does not know)
inline void UpdateNormalAndDepth(const std::vector<ORB_SLAM2::MapPoint *> &vpMPs, const LocalMapSnapshot &S,
                                 std::vector<uint8_t> *vStatus = nullptr)
{
    const char *const what = "UpdateNormalAndDepth";
    ShimClock clk;
    const std::vector<ORB_SLAM2::KeyFrame *> &vpKFs = S.KeyFrames();
    if (vStatus) vStatus->assign(vpMPs.size(), AOS2_ND_UNKNOWN);
    if (vpKFs.empty()) return;
    std::vector<float> kf_center(3 * vpKFs.size());
    for (size_t k = 0; k < vpKFs.size(); ++k) {
        const cv::Mat Ow = vpKFs[k]->GetCameraCenter();
        for (int c = 0; c < 3; ++c) kf_center[3 * k + c] = Ow.at<float>(c);
    }
    const std::vector<float> &scale = vpKFs.front()->mvScaleFactors;
    std::vector<size_t> where;
    std::vector<int32_t> point, ref_kf, term_off(1, 0);
    std::vector<float> xyz;
    for (size_t i = 0; i < vpMPs.size(); ++i) {
        ORB_SLAM2::MapPoint *pMP = vpMPs[i];
        const int32_t row = pMP ? S.PointRow(pMP) : -1, ref = pMP ? S.KeyFrameRow(pMP->GetReferenceKeyFrame()) : -1;
        if (row < 0 || ref < 0) continue;
        where.push_back(i);
        point.push_back(row);
        ref_kf.push_back(ref);
        const cv::Mat Pos = pMP->GetWorldPos();
        for (int c = 0; c < 3; ++c) xyz.push_back(Pos.at<float>(c));
        int32_t n_known = 0;   // the observers the snapshot can list
        const std::map<ORB_SLAM2::KeyFrame *, size_t> observations = pMP->GetObservations();
        for (const auto &ob : observations) n_known += S.KeyFrameRow(ob.first) >= 0 ? 1 : 0;
        term_off.push_back(term_off.back() + n_known);
    }
    const int n = (int)point.size();
    std::vector<uint8_t> status(n + 1, AOS2_ND_UNKNOWN);
    std::vector<float> normal(3 * (size_t)n + 3), min_dist(n + 1), max_dist(n + 1), theta_mean(n + 1), theta_std(n + 1),
        term_unit(3 * (size_t)term_off.back() + 3), term_theta((size_t)term_off.back() + 1);
    std::vector<int32_t> n_terms(n + 1, 0);
    aos2_normal_depth_t a = {};
    a.n = n; a.point = point.data(); a.xyz = xyz.data(); a.ref_kf = ref_kf.data(); a.kf_center = kf_center.data();
    a.n_levels = (int32_t)scale.size(); a.scale = scale.data(); a.rows_form = AOS2_ND_ROWS_PLANNING; a.term_off = term_off.data();
    a.status = status.data(); a.normal = normal.data(); a.min_dist = min_dist.data(); a.max_dist = max_dist.data();
    a.theta_mean = theta_mean.data(); a.theta_std = theta_std.data(); a.n_terms = n_terms.data();
    a.term_unit = term_unit.data(); a.term_theta = term_theta.data();
    last_shim_timing().gather_us = clk.lap();
    check(aos2_local_map_update_normal_depth(S.Handle(), &a), what);
    last_shim_timing().call_us = clk.lap();
    for (int j = 0; j < n; ++j) {
        ORB_SLAM2::MapPoint *pMP = vpMPs[where[j]];
        if (vStatus) (*vStatus)[where[j]] = status[j];
        if (status[j] != AOS2_ND_UPDATED) continue;
        if (n_terms[j] != term_off[j + 1] - term_off[j])
            fail_precondition(what, "a point's observations changed since the snapshot last read them: LocalMapSnapshot::Apply comes first");
        pMP->mNormalVectors.clear();   // :383-384
        pMP->theta_sVector.clear();
        for (int32_t e = term_off[j]; e < term_off[j + 1]; ++e) {
            cv::Mat u(3, 1, CV_32F);
            for (int c = 0; c < 3; ++c) u.at<float>(c) = term_unit[3 * (size_t)e + c];
            pMP->mNormalVectors.push_back(u);
            pMP->theta_sVector.push_back(term_theta[e]);
        }
        MapPointNormalDepthMembers<ORB_SLAM2::MapPoint>::Assign(pMP, &normal[3 * (size_t)j], min_dist[j], max_dist[j], theta_mean[j],
                                                                 theta_std[j]);
    }
    last_shim_timing().scatter_us = clk.lap();
}

inline void UpdateNormalAndDepth(ORB_SLAM2::MapPoint *pMP, const LocalMapSnapshot &S)
{
    UpdateNormalAndDepth(std::vector<ORB_SLAM2::MapPoint *>(1, pMP), S);
}

}  // namespace aos2
