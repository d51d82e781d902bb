// The bodies of ORB_SLAM2::Optimizer::GlobalBundleAdjustemnt and Optimizer::BundleAdjustment (reference src/Optimizer.cc:41-237) at the
// signatures include/Optimizer.h:40-44 declares: :71-184 stay as a gather -- the keyframes and map points that are not bad, mnId == 0
// fixed, every observation of a point by a keyframe of the graph, a point without one left out -- ONE C-ABI call
// (aos2_global_bundle_adjustment) replaces the g2o graph, initializeOptimization() and optimize(nIterations), and :193-235 write the
// result back: SetPose / SetWorldPos + UpdateNormalAndDepth when nLoopKF == 0 (Tracking::CreateInitialMapMonocular,
// src/Tracking.cc:781), mTcwGBA / mPosGBA / mnBAGlobalForKF otherwise (LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:652).
// Both call sites stay unchanged.
// Conventions: a point's observations are emitted by ascending KeyFrame::mnId (the reference walks a
// std::map keyed by pointer); an observer that is bad, has mnId > maxKFid or is not among vpKFs is skipped (the reference would
// dereference a null vertex for the last kind, and GlobalBundleAdjustemnt cannot produce it).
// Include AFTER the headers that declare KeyFrame, MapPoint, Map, and after Optimizer.h's own requirements.
#pragma once
#include <cmath>
#include <cstring>
#include <utility>

#include "Optimizer.h"

namespace ORB_SLAM2 {

inline void Optimizer::GlobalBundleAdjustemnt(Map *pMap, int nIterations, bool *pbStopFlag, const unsigned long nLoopKF, const bool bRobust)
{
    std::vector<KeyFrame *> vpKFs = pMap->GetAllKeyFrames();
    std::vector<MapPoint *> vpMP = pMap->GetAllMapPoints();
    BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust);
}

inline void Optimizer::BundleAdjustment(const std::vector<KeyFrame *> &vpKFs, const std::vector<MapPoint *> &vpMP, int nIterations, bool *pbStopFlag,
                                        const unsigned long nLoopKF, const bool bRobust)
{
    std::vector<bool> vbNotIncludedMP(vpMP.size(), true);
    long unsigned int maxKFid = 0;

    // Set KeyFrame vertices (:71-83)
    std::vector<KeyFrame *> vpVertexKF;
    std::map<KeyFrame *, int32_t> vertex_of;
    std::vector<float> pose_Tcw;
    std::vector<uint8_t> pose_fixed;
    std::vector<int64_t> pose_id;
    float fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;
    for (size_t i = 0; i < vpKFs.size(); i++) {
        KeyFrame *pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const cv::Mat Tcw = pKF->GetPose();
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) pose_Tcw.push_back(Tcw.at<float>(r, c));
        pose_fixed.push_back(pKF->mnId == 0);
        pose_id.push_back((int64_t)pKF->mnId);
        vertex_of[pKF] = (int32_t)vpVertexKF.size();
        vpVertexKF.push_back(pKF);
        if (pKF->mnId > maxKFid) maxKFid = pKF->mnId;
        fx = pKF->fx; fy = pKF->fy; cx = pKF->cx; cy = pKF->cy; bf = pKF->mbf;   // (one camera: the calibration is the same in every keyframe)
    }

    // Set MapPoint vertices and their edges (:89-184)
    std::vector<MapPoint *> vpVertexMP;
    std::vector<size_t> index_of_point;
    std::vector<float> point_xyz, edge_obs, edge_w;
    std::vector<int64_t> point_id;
    std::vector<int32_t> edge_pose, edge_point;
    std::vector<uint8_t> edge_stereo;
    for (size_t i = 0; i < vpMP.size(); i++) {
        MapPoint *pMP = vpMP[i];
        if (pMP->isBad()) continue;
        const std::map<KeyFrame *, size_t> observations = pMP->GetObservations();
        std::vector<std::pair<KeyFrame *, size_t>> obs;
        for (std::map<KeyFrame *, size_t>::const_iterator mit = observations.begin(); mit != observations.end(); mit++) {
            KeyFrame *pKF = mit->first;
            if (pKF->isBad() || pKF->mnId > maxKFid || !vertex_of.count(pKF)) continue;
            obs.push_back(*mit);
        }
        if (obs.empty()) continue;   // removeVertex (:175-179)
        std::sort(obs.begin(), obs.end(), [](const std::pair<KeyFrame *, size_t> &a, const std::pair<KeyFrame *, size_t> &b) { return a.first->mnId < b.first->mnId; });
        vbNotIncludedMP[i] = false;
        const cv::Mat X = pMP->GetWorldPos();
        for (int k = 0; k < 3; ++k) point_xyz.push_back(X.at<float>(k));
        point_id.push_back((int64_t)pMP->mnId);
        for (const std::pair<KeyFrame *, size_t> &o : obs) {
            KeyFrame *pKF = o.first;
            const cv::KeyPoint &kpUn = pKF->mvKeysUn[o.second];
            const float kp_ur = pKF->mvuRight[o.second];
            edge_pose.push_back(vertex_of[pKF]);
            edge_point.push_back((int32_t)vpVertexMP.size());
            edge_obs.push_back(kpUn.pt.x); edge_obs.push_back(kpUn.pt.y); edge_obs.push_back(kp_ur);
            edge_stereo.push_back(kp_ur < 0 ? 0 : 1);   // :116
            edge_w.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
        }
        vpVertexMP.push_back(pMP);
        index_of_point.push_back(i);
    }

    const size_t nk = vpVertexKF.size(), np = vpVertexMP.size();
    std::vector<float> out_T(16 * nk + 16), out_X(3 * np + 3);
    std::vector<uint8_t> included(np + 1);
    aos2_lba_problem_t P;
    memset(&P, 0, sizeof(P));
    P.n_poses = (int32_t)nk; P.n_points = (int32_t)np; P.n_edges = (int32_t)edge_pose.size();
    P.pose_Tcw = pose_Tcw.data(); P.pose_fixed = pose_fixed.data(); P.pose_id = pose_id.data();
    P.point_xyz = point_xyz.data(); P.point_id = point_id.data();
    P.edge_pose = edge_pose.data(); P.edge_point = edge_point.data(); P.edge_obs = edge_obs.data(); P.edge_stereo = edge_stereo.data();
    P.edge_inv_sigma2 = edge_w.data();
    P.fx = fx; P.fy = fy; P.cx = cx; P.cy = cy; P.bf = bf;
    P.stop_flag = reinterpret_cast<const volatile uint8_t *>(pbStopFlag);
    aos2_gba_options_t O;
    O.iterations = nIterations;
    O.robust = bRobust ? 1 : 0;
    const float thHuber2D = sqrt(5.99);    // :85-86
    const float thHuber3D = sqrt(7.815);
    O.huber_mono = thHuber2D;
    O.huber_stereo = thHuber3D;
    aos2_gba_result_t R;
    memset(&R, 0, sizeof(R));
    R.pose_Tcw = out_T.data(); R.point_xyz = out_X.data(); R.point_included = included.data();
    if (nk == 0) return;
    if (aos2_global_bundle_adjustment(aos2::optimizer_handle(), &P, &O, &R) != AOS2_OK) {
        aos2::report("BundleAdjustment");   // the map stays as it was
        return;
    }

    // Recover optimized data: keyframes (:193-210) ...
    for (size_t k = 0; k < nk; ++k) {
        KeyFrame *pKF = vpVertexKF[k];
        cv::Mat Tcw(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) Tcw.at<float>(r, c) = out_T[16 * k + 4 * r + c];
        if (nLoopKF == 0)
            pKF->SetPose(Tcw);
        else {
            pKF->mTcwGBA = Tcw.clone();
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    // ... and points (:213-235): the ones that were not included stay untouched
    for (size_t j = 0; j < np; ++j) {
        MapPoint *pMP = vpVertexMP[j];
        if (vbNotIncludedMP[index_of_point[j]] || pMP->isBad()) continue;
        cv::Mat X(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) X.at<float>(r) = out_X[3 * j + r];
        if (nLoopKF == 0) {
            pMP->SetWorldPos(X);
            pMP->UpdateNormalAndDepth();
        } else {
            pMP->mPosGBA = X.clone();
            pMP->mnBAGlobalForKF = nLoopKF;
        }
    }
}

}  // namespace ORB_SLAM2
