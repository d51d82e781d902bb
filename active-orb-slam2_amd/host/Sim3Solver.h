// ORB_SLAM2::Sim3Solver at the reference's signature (include/Sim3Solver.h:39-49, src/Sim3Solver.cc), for the loop of
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:276-303), which stays as it is:
//
//     Sim3Solver* pSolver = new Sim3Solver(mpCurrentKF, pKF, vvpMapPointMatches[i], mbFixScale);
//     pSolver->SetRansacParameters(0.99, 20, 300);
//     ...
//     cv::Mat Scm = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
//
// The constructor is the reference's (:43-103: the gates, GetIndexInKeyFrame, mvnIndices1, Rcw*X3Dw + tcw as cv::Mat expressions,
// the 9.210*sigmaSquare thresholds).  The FIRST iterate() after SetRansacParameters draws the 3 * mRansacMaxIts integers of all
// iterations from DUtils::Random::RandomInt in iteration order and makes ONE C-ABI call (aos2_sim3_ransac: every hypothesis and its
// inliers on the GPU); that call and the later ones replay :142-206 from the stored result, nIterations at a time.
//
// What differs from the reference, by construction:
//   - For one solver the triples equal the reference's.  Solvers that take turns (ComputeSim3 gives each candidate 5 iterations per
//     round) consume the process-wide generator in another interleaving: each draws all its integers at its first iterate().
//   - GetEstimatedRotation / Translation / Scale return the solver's state where it stops (at the iteration that returned a Sim3,
//     or after mRansacMaxIts), which is what src/LoopClosing.cc:322-324 reads; the reference would also answer between two unsuccessful calls.
//   - After iterate() has returned a Sim3 the solver is spent: further calls count iterations up to bNoMore and find nothing.  The
//     reference would go on with its RANSAC when OptimizeSim3 rejects the Sim3 (:331) and could return another one; the batched
//     result reports the iterations behind first_success as not run.
// Thresholds: the reference keeps mvnMaxError1 / 2 in a std::vector<size_t> (include/Sim3Solver.h:78-79), so 9.210*sigmaSquare is
// truncated to a whole number before :356 compares a float with it.  Kept as written; the library takes the thresholds as floats.
// The cameras are read from the public fx fy cx cy of the keyframes (the same values as mK).
// Include AFTER the headers that declare KeyFrame, MapPoint and DUtils::Random (the reference's, or tests/cpp/refstub/slam_stub.h
// and a stand-in for the generator); nothing of the reference's data model changes.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "aos2_handles.h"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame *pKF1, KeyFrame *pKF2, const std::vector<MapPoint *> &vpMatched12, const bool bFixScale = true)
        : mnIterations(0), mbFixScale(bFixScale)
    {
        mpKF1 = pKF1;
        mpKF2 = pKF2;
        std::vector<MapPoint *> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
        mN1 = (int)vpMatched12.size();
        mvnIndices1.reserve(mN1);
        mvX3Dc1.reserve(3 * (size_t)mN1);
        mvX3Dc2.reserve(3 * (size_t)mN1);
        cv::Mat Rcw1 = pKF1->GetRotation();
        cv::Mat tcw1 = pKF1->GetTranslation();
        cv::Mat Rcw2 = pKF2->GetRotation();
        cv::Mat tcw2 = pKF2->GetTranslation();
        for (int i1 = 0; i1 < mN1; i1++) {
            if (vpMatched12[i1]) {
                MapPoint *pMP1 = vpKeyFrameMP1[i1];
                MapPoint *pMP2 = vpMatched12[i1];
                if (!pMP1) continue;
                if (pMP1->isBad() || pMP2->isBad()) continue;
                int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
                int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
                if (indexKF1 < 0 || indexKF2 < 0) continue;
                const cv::KeyPoint &kp1 = pKF1->mvKeysUn[indexKF1];
                const cv::KeyPoint &kp2 = pKF2->mvKeysUn[indexKF2];
                const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
                const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
                mvnMaxError1.push_back(9.210 * sigmaSquare1);
                mvnMaxError2.push_back(9.210 * sigmaSquare2);
                mvnIndices1.push_back(i1);
                cv::Mat X3D1w = pMP1->GetWorldPos();
                cv::Mat X3Dc1 = Rcw1 * X3D1w + tcw1;
                cv::Mat X3D2w = pMP2->GetWorldPos();
                cv::Mat X3Dc2 = Rcw2 * X3D2w + tcw2;
                for (int r = 0; r < 3; ++r) {
                    mvX3Dc1.push_back(X3Dc1.at<float>(r));
                    mvX3Dc2.push_back(X3Dc2.at<float>(r));
                }
            }
        }
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300)
    {
        mRansacProb = probability;
        mRansacMinInliers = minInliers;
        mRansacMaxIts = maxIterations;
        N = (int)mvnIndices1.size();   // number of correspondences
        // :125-135 (a quotient that is no int is converted the way x86 does it for the reference: INT_MIN)
        float epsilon = (float)mRansacMinInliers / N;
        int nIterations;
        if (mRansacMinInliers == N)
            nIterations = 1;
        else {
            const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow((double)epsilon, 3)));
            nIterations = (v >= -2147483648.0 && v <= 2147483647.0) ? (int)v : INT32_MIN;
        }
        mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
        mnIterations = 0;
        mbSolved = false;
    }

    cv::Mat find(std::vector<bool> &vbInliers12, int &nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers);
    }

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers = std::vector<bool>(mN1, false);
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return cv::Mat();
        }
        if (!mbSolved) Solve();
        int nCurrentIterations = 0;
        while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {
            nCurrentIterations++;
            mnIterations++;
            if (mnIterations - 1 == mnFirstSuccess) {   // :183-199 accepted this hypothesis and it has more than mRansacMinInliers
                nInliers = mnBestInliers;
                for (int i = 0; i < N; i++)
                    if (mvbBestInliers[i]) vbInliers[mvnIndices1[i]] = true;
                return mBestT12;
            }
        }
        if (mnIterations >= mRansacMaxIts) bNoMore = true;
        return cv::Mat();
    }

    cv::Mat GetEstimatedRotation() { return mBestRotation.clone(); }
    cv::Mat GetEstimatedTranslation() { return mBestTranslation.clone(); }
    float GetEstimatedScale() { return mBestScale; }

protected:
    // the draws of all iterations, one aos2_sim3_ransac call, the mBest* members from its result
    void Solve()
    {
        aos2::ShimClock clk;
        std::vector<int32_t> draws(3 * (size_t)mRansacMaxIts);
        for (int k = 0; k < mRansacMaxIts; ++k)
            for (short i = 0; i < 3; ++i) draws[3 * (size_t)k + i] = DUtils::Random::RandomInt(0, N - 1 - i);
        std::vector<float> e1(mvnMaxError1.begin(), mvnMaxError1.end()), e2(mvnMaxError2.begin(), mvnMaxError2.end());   // :356's conversion
        std::vector<uint8_t> inl((size_t)N);
        aos2_sim3_problem_t P = {};
        P.n = N;
        P.X3Dc1 = mvX3Dc1.data(); P.X3Dc2 = mvX3Dc2.data();
        P.max_err1 = e1.data(); P.max_err2 = e2.data();
        P.fx1 = mpKF1->fx; P.fy1 = mpKF1->fy; P.cx1 = mpKF1->cx; P.cy1 = mpKF1->cy;
        P.fx2 = mpKF2->fx; P.fy2 = mpKF2->fy; P.cx2 = mpKF2->cx; P.cy2 = mpKF2->cy;
        P.fix_scale = mbFixScale ? 1 : 0;
        P.probability = mRansacProb;
        P.min_inliers = mRansacMinInliers;
        P.max_iterations = mRansacMaxIts;
        P.draws = draws.data();
        aos2_sim3_result_t R = {};
        R.inliers = inl.data();
        aos2::last_shim_timing().gather_us = clk.lap();
        aos2::check(aos2_sim3_ransac(aos2::matcher_handle(0.75f, true), &P, &R, 1), "Sim3Solver");
        aos2::last_shim_timing().call_us = clk.lap();
        mnFirstSuccess = R.first_success;
        mnBestInliers = R.best_inliers;
        mvbBestInliers.assign(inl.begin(), inl.end());
        mBestT12.create(4, 4, CV_32F);
        mBestRotation.create(3, 3, CV_32F);
        mBestTranslation.create(3, 1, CV_32F);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) mBestT12.at<float>(r, c) = R.T12[4 * r + c];
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) mBestRotation.at<float>(r, c) = R.R12[3 * r + c];
            mBestTranslation.at<float>(r) = R.t12[r];
        }
        mBestScale = R.s12;
        mbSolved = true;
        aos2::last_shim_timing().scatter_us = clk.lap();
    }

    // KeyFrames and matches
    KeyFrame *mpKF1;
    KeyFrame *mpKF2;
    std::vector<float> mvX3Dc1, mvX3Dc2;   // [N][3]
    std::vector<size_t> mvnIndices1;
    std::vector<size_t> mvnMaxError1, mvnMaxError2;   // (size_t as in the reference: whole numbers)
    int N;
    int mN1;

    // Ransac state: where the replay stands, and the result of the one call
    int mnIterations;
    bool mbSolved = false;
    int mnFirstSuccess = -1;
    std::vector<bool> mvbBestInliers;
    int mnBestInliers = 0;
    cv::Mat mBestT12, mBestRotation, mBestTranslation;
    float mBestScale = 0;

    bool mbFixScale;   // scale is fixed to 1 in the stereo/RGBD case
    double mRansacProb;
    int mRansacMinInliers;
    int mRansacMaxIts;
};

}  // namespace ORB_SLAM2
