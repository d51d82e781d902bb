// The loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) for the matches of one neighbour keyframe, at the
// reference's call site: between `matcher.SearchForTriangulation(mpCurrentKeyFrame, pKF2, F12, vMatchedIndices, false)` (:272) and
// the `new MapPoint(x3D, mpCurrentKeyFrame, mpMap)` block (:438-453), which stays where it is.
//
//     std::vector<cv::Mat> x3D;
//     std::vector<uint8_t> status;
//     aos2::TriangulateMatches(mpCurrentKeyFrame, pKF2, vMatchedIndices, x3D, status);
//     for (size_t ikp = 0; ikp < vMatchedIndices.size(); ikp++) {
//         if (status[ikp] != AOS2_TRI_ACCEPTED) continue;
//         MapPoint *pMP = new MapPoint(x3D[ikp], mpCurrentKeyFrame, mpMap);      // :438 onwards, unchanged
//         ...
//     }
//
// It snapshots the members the loop reads (both poses and cameras, mvKeysUn / mvKeys / mvuRight / mvDepth of the matched features,
// mvScaleFactors), makes ONE C-ABI call (aos2_triangulate_matches: parallax test, cv::SVD, UnprojectStereo, the gates, all on the
// GPU) and hands the points back as 3x1 CV_32F matrices.  Include AFTER the headers that declare KeyFrame (the reference's, or
// tests/cpp/refstub/slam_stub.h); nothing of the reference's data model changes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "aos2_handles.h"

namespace aos2 {

// status[k]: AOS2_TRI_* of match k (never NO_MATCH or SUPERSEDED: the reference's own loop order does the superseding -- the next
// SearchForTriangulation skips what this call's points were added to); x3D[k]: 3x1 CV_32F where the loop got as far as a point
// (status 1 and 4..9), empty otherwise
inline void TriangulateMatches(ORB_SLAM2::KeyFrame *pKF1, ORB_SLAM2::KeyFrame *pKF2, const std::vector<std::pair<size_t, size_t>> &vMatchedIndices,
                               std::vector<cv::Mat> &x3D, std::vector<uint8_t> &status)
{
    ShimClock clk;
    const size_t n = vMatchedIndices.size();
    x3D.assign(n, cv::Mat());
    status.assign(n, AOS2_TRI_NO_MATCH);
    if (n == 0) return;
    aos2_triang_geom_t g;
    memset(&g, 0, sizeof g);
    const cv::Mat T1 = pKF1->GetPose(), T2 = pKF2->GetPose();
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            g.Tcw1[4 * r + c] = T1.at<float>(r, c);
            g.Tcw2[4 * r + c] = T2.at<float>(r, c);
        }
    g.fx1 = pKF1->fx; g.fy1 = pKF1->fy; g.cx1 = pKF1->cx; g.cy1 = pKF1->cy; g.mb1 = pKF1->mb; g.mbf1 = pKF1->mbf;
    g.fx2 = pKF2->fx; g.fy2 = pKF2->fy; g.cx2 = pKF2->cx; g.cy2 = pKF2->cy; g.mb2 = pKF2->mb; g.mbf2 = pKF2->mbf;
    // (both keyframes come from one ORBextractor; more than 8 levels is refused by the library with its own message)
    g.n_levels = (int32_t)std::min(pKF1->mvScaleFactors.size(), pKF2->mvScaleFactors.size());
    for (int l = 0; l < g.n_levels && l < 8; ++l) {
        g.scale_factors1[l] = pKF1->mvScaleFactors[l];
        g.scale_factors2[l] = pKF2->mvScaleFactors[l];
    }
    std::vector<aos2_triang_obs_t> o1(n), o2(n);
    auto snap = [](ORB_SLAM2::KeyFrame *pKF, size_t i) {
        aos2_triang_obs_t o;
        o.ux = pKF->mvKeysUn[i].pt.x; o.uy = pKF->mvKeysUn[i].pt.y;
        o.kx = pKF->mvKeys[i].pt.x; o.ky = pKF->mvKeys[i].pt.y;
        o.u_right = pKF->mvuRight[i];
        o.depth = pKF->mvDepth[i];
        o.octave = pKF->mvKeysUn[i].octave;
        return o;
    };
    for (size_t k = 0; k < n; ++k) {
        o1[k] = snap(pKF1, vMatchedIndices[k].first);
        o2[k] = snap(pKF2, vMatchedIndices[k].second);
    }
    std::vector<float> pts(3 * n);
    last_shim_timing().gather_us = clk.lap();
    check(aos2_triangulate_matches(matcher_handle(0.6f, false), &g, (int)n, o1.data(), o2.data(), pts.data(), status.data()),
          "CreateNewMapPoints");
    last_shim_timing().call_us = clk.lap();
    for (size_t k = 0; k < n; ++k) {
        if (status[k] == AOS2_TRI_NO_MATCH || status[k] == AOS2_TRI_LOW_PARALLAX || status[k] == AOS2_TRI_W_ZERO) continue;
        x3D[k].create(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) x3D[k].at<float>(r) = pts[3 * k + r];
    }
    last_shim_timing().scatter_us = clk.lap();
}

}  // namespace aos2
