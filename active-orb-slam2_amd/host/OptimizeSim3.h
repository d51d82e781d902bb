// The body of ORB_SLAM2::Optimizer::OptimizeSim3 (reference src/Optimizer.cc:1047-1242) at the signature Optimizer.h declares:
// the loop of :1100-1179 gathers the correspondences into the arrays of aos2_sim3_opt_problem_t, ONE C-ABI call replaces the g2o
// graph, its two optimisations and the outlier pass (:1181-1235), and the result goes back the way :1197, :1231 and :1239 write it.
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:355) calls it unchanged; a caller with several candidates at hand makes one
// aos2_optimize_sim3 call over all of them (INTEGRATION.md "Loop detection").
// Include AFTER Optimizer.h and after the header that defines g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h): only rotation().x() .. w(),
// translation()[k], scale() and the (Quaterniond, Vector3d, double) constructor are used.
#pragma once
#include "Optimizer.h"

namespace ORB_SLAM2 {

inline int Optimizer::OptimizeSim3(KeyFrame *pKF1, KeyFrame *pKF2, std::vector<MapPoint *> &vpMatches1, g2o::Sim3 &g2oS12, const float th2,
                                   const bool bFixScale)
{
    // Camera poses (:1064-1067)
    const cv::Mat R1w = pKF1->GetRotation();
    const cv::Mat t1w = pKF1->GetTranslation();
    const cv::Mat R2w = pKF2->GetRotation();
    const cv::Mat t2w = pKF2->GetTranslation();

    const int N = vpMatches1.size();
    const std::vector<MapPoint *> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<float> X1c, X2c, obs1, obs2, is1, is2;
    std::vector<size_t> vnIndexEdge;
    for (int i = 0; i < N; i++) {   // :1100-1179
        if (!vpMatches1[i]) continue;
        MapPoint *pMP1 = vpMapPoints1[i];
        MapPoint *pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;   // :1113-1115
        const cv::Mat P3D1c = R1w * pMP1->GetWorldPos() + t1w;
        const cv::Mat P3D2c = R2w * pMP2->GetWorldPos() + t2w;
        for (int k = 0; k < 3; ++k) {
            X1c.push_back(P3D1c.at<float>(k));
            X2c.push_back(P3D2c.at<float>(k));
        }
        const cv::KeyPoint &kpUn1 = pKF1->mvKeysUn[i];
        const cv::KeyPoint &kpUn2 = pKF2->mvKeysUn[i2];
        obs1.push_back(kpUn1.pt.x); obs1.push_back(kpUn1.pt.y);
        obs2.push_back(kpUn2.pt.x); obs2.push_back(kpUn2.pt.y);
        is1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
        is2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
        vnIndexEdge.push_back(i);
    }
    const int nCorrespondences = (int)vnIndexEdge.size();

    aos2_sim3_opt_problem_t P;
    memset(&P, 0, sizeof(P));
    P.n = nCorrespondences;
    P.X1c = X1c.data(); P.X2c = X2c.data(); P.obs1 = obs1.data(); P.obs2 = obs2.data();
    P.inv_sigma2_1 = is1.data(); P.inv_sigma2_2 = is2.data();
    P.fx1 = pKF1->fx; P.fy1 = pKF1->fy; P.cx1 = pKF1->cx; P.cy1 = pKF1->cy;   // (mK holds the same floats)
    P.fx2 = pKF2->fx; P.fy2 = pKF2->fy; P.cx2 = pKF2->cx; P.cy2 = pKF2->cy;
    P.q12[0] = g2oS12.rotation().x(); P.q12[1] = g2oS12.rotation().y(); P.q12[2] = g2oS12.rotation().z(); P.q12[3] = g2oS12.rotation().w();
    for (int k = 0; k < 3; ++k) P.t12[k] = g2oS12.translation()[k];
    P.s12 = g2oS12.scale();
    P.th2 = th2;
    P.fix_scale = bFixScale ? 1 : 0;
    std::vector<uint8_t> outlier((size_t)nCorrespondences + 1);
    aos2_sim3_opt_result_t R;
    memset(&R, 0, sizeof(R));
    R.outlier = outlier.data();
    if (aos2_optimize_sim3(aos2::optimizer_handle(), &P, &R, 1) != AOS2_OK) {
        aos2::report("OptimizeSim3");   // the candidate keeps its matches and its Sim3 and counts no inliers: ComputeSim3 drops it
        return 0;
    }
    for (int k = 0; k < nCorrespondences; ++k)   // :1197, :1231
        if (outlier[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint *>(NULL);
    if (nCorrespondences - R.n_bad < 10) return 0;   // :1212: g2oS12 stays as it is
    g2oS12 = g2o::Sim3(Eigen::Quaterniond(R.q12[3], R.q12[0], R.q12[1], R.q12[2]), Eigen::Vector3d(R.t12[0], R.t12[1], R.t12[2]), R.s12);   // :1239
    return R.n_inliers;
}

}  // namespace ORB_SLAM2
