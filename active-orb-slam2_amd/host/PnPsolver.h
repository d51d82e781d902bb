// ORB_SLAM2::PnPsolver at the reference's signature (include/PnPsolver.h:63-72, src/PnPsolver.cc), for the candidate loop of
// Tracking::Relocalization (src/Tracking.cc:1565-1625), which stays as it is:
//
//     PnPsolver* pSolver = new PnPsolver(mCurrentFrame, vvpMapPointMatches[i]);
//     pSolver->SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991);
//     ...
//     cv::Mat Tcw = pSolver->iterate(5, bNoMore, vbInliers, nInliers);
//
// The constructor and SetRansacParameters are the reference's (:67-157: the gates, mvP2D, mvSigma2, mvP3Dw, mvKeyPointIndices, the
// adjusted mRansacMinInliers / mRansacEpsilon / mRansacMaxIts, mvMaxError as a float product).  iterate() works out how many
// iterations the `while` of :182 allows this call -- `mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`, with ||: the
// first iterate(5) runs max(mRansacMaxIts, 5) -- draws the rows it still lacks from DUtils::Random::RandomInt in iteration order and
// makes ONE C-ABI call (aos2_pnp_ransac: every hypothesis, its inliers and the Refine() of every new best on the GPU) with its state
// carried in.  From the result it replays bNoMore, vbInliers, nInliers and the 4x4 CV_32F matrix (mRefinedTcw, or mBestTcw at the
// exhaustion of :241-255).  The solver is NOT spent after a return: Relocalization calls iterate(5) again when PoseOptimization
// rejects the pose (nGood < 10: continue), and the next call resumes at the iteration behind the return with mnBestInliers /
// mvbBestInliers as they stood.
//
// What differs from the reference, by construction: a call draws the integers of all iterations it may run before it knows where it
// returns; rows behind a return are kept for the next call.  For one solver the sets equal the reference's; solvers that take turns
// consume the process-wide generator in another interleaving.
// Include AFTER the headers that declare Frame, MapPoint and DUtils::Random (the reference's, or tests/cpp/refstub/pnp_stub.h).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "aos2_handles.h"

namespace ORB_SLAM2 {

class PnPsolver {
public:
    PnPsolver(const Frame &F, const std::vector<MapPoint *> &vpMapPointMatches) : mnIterations(0), mnBestInliers(0), N(0)
    {
        mvpMapPointMatches = vpMapPointMatches;
        mvP2D.reserve(2 * F.mvpMapPoints.size());
        mvSigma2.reserve(F.mvpMapPoints.size());
        mvP3Dw.reserve(3 * F.mvpMapPoints.size());
        mvKeyPointIndices.reserve(F.mvpMapPoints.size());
        for (size_t i = 0, iend = vpMapPointMatches.size(); i < iend; i++) {
            MapPoint *pMP = vpMapPointMatches[i];
            if (pMP) {
                if (!pMP->isBad()) {
                    const cv::KeyPoint &kp = F.mvKeysUn[i];
                    mvP2D.push_back(kp.pt.x);
                    mvP2D.push_back(kp.pt.y);
                    mvSigma2.push_back(F.mvLevelSigma2[kp.octave]);
                    cv::Mat Pos = pMP->GetWorldPos();
                    for (int r = 0; r < 3; ++r) mvP3Dw.push_back(Pos.at<float>(r));
                    mvKeyPointIndices.push_back(i);
                }
            }
        }
        // Set camera calibration parameters (widened to double by the library, as :104-107 does)
        fu = F.fx;
        fv = F.fy;
        uc = F.cx;
        vc = F.cy;
        SetRansacParameters();
    }

    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4,
                             float th2 = 5.991)
    {
        mRansacProb = probability;
        mRansacMinSet = minSet;
        N = (int)mvKeyPointIndices.size();   // number of correspondences
        int32_t mi = 0, its = 0;
        aos2::check(aos2_pnp_ransac_parameters(N, probability, minInliers, maxIterations, minSet, epsilon, &mi, &mRansacEpsilon, &its), "PnPsolver");
        mRansacMinInliers = mi;
        mRansacMaxIts = its;
        mvMaxError.resize(mvSigma2.size());
        for (size_t i = 0; i < mvSigma2.size(); i++) mvMaxError[i] = mvSigma2[i] * th2;
    }

    cv::Mat find(std::vector<bool> &vbInliers, int &nInliers)
    {
        bool bFlag;
        return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers);
    }

    cv::Mat iterate(int nIterations, bool &bNoMore, std::vector<bool> &vbInliers, int &nInliers)
    {
        bNoMore = false;
        vbInliers.clear();
        nInliers = 0;
        if (N < mRansacMinInliers) {
            bNoMore = true;
            return cv::Mat();
        }
        if (mRansacMinSet < 4 || mRansacMinSet > 16) aos2::fail("PnPsolver: a minimal set of 4 .. 16 correspondences");
        aos2::ShimClock clk;
        // the iterations the while of :182 allows this call, and the rows of draws they still lack
        const int end = mnIterations + std::max(std::max(mRansacMaxIts - mnIterations, nIterations), 0);
        for (int k = (int)(mvDraws.size() / (size_t)mRansacMinSet); k < end; ++k)
            for (short i = 0; i < mRansacMinSet; ++i) mvDraws.push_back(DUtils::Random::RandomInt(0, N - 1 - i));
        std::vector<uint8_t> refined((size_t)N), best((size_t)N);
        aos2_pnp_problem_t P = {};
        P.n = N;
        P.P3Dw = mvP3Dw.data();
        P.P2D = mvP2D.data();
        P.max_err = mvMaxError.data();
        P.fx = fu; P.fy = fv; P.cx = uc; P.cy = vc;
        P.min_inliers = mRansacMinInliers;
        P.min_set = mRansacMinSet;
        P.first_iteration = mnIterations;
        P.n_iterations = end;
        P.draws = mvDraws.data();
        P.best_inliers_in = mnBestInliers;
        P.best_in = mnBestInliers > 0 ? mvbBestInliers.data() : nullptr;
        aos2_pnp_result_t R = {};
        R.inliers = refined.data();
        R.best = best.data();
        aos2::last_shim_timing().gather_us = clk.lap();
        aos2::check(aos2_pnp_ransac(aos2::matcher_handle(0.75f, true), &P, &R, 1), "PnPsolver");
        aos2::last_shim_timing().call_us = clk.lap();
        if (R.best_iteration >= 0) {   // :212-224
            mnBestInliers = R.best_inliers;
            mvbBestInliers = best;
            mBestTcw = Tcw(R.best_Tcw);
        }
        cv::Mat out;
        if (R.returned_at >= 0) {   // :226-236
            mnIterations = R.returned_at + 1;
            nInliers = R.n_inliers;
            Flags(refined, vbInliers);
            out = Tcw(R.Tcw);
        } else {   // :241-257
            mnIterations = end;
            if (mnIterations >= mRansacMaxIts) {
                bNoMore = true;
                if (mnBestInliers >= mRansacMinInliers) {
                    nInliers = mnBestInliers;
                    Flags(mvbBestInliers, vbInliers);
                    out = mBestTcw.clone();
                }
            }
        }
        aos2::last_shim_timing().scatter_us = clk.lap();
        return out;
    }

protected:
    static cv::Mat Tcw(const float T[16])
    {
        cv::Mat m(4, 4, CV_32F);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) m.at<float>(r, c) = T[4 * r + c];
        return m;
    }
    void Flags(const std::vector<uint8_t> &flags, std::vector<bool> &vbInliers) const
    {
        vbInliers = std::vector<bool>(mvpMapPointMatches.size(), false);
        for (int i = 0; i < N; i++)
            if (flags[i]) vbInliers[mvKeyPointIndices[i]] = true;
    }

    std::vector<MapPoint *> mvpMapPointMatches;
    std::vector<float> mvP2D;      // [N][2]
    std::vector<float> mvSigma2;
    std::vector<float> mvP3Dw;     // [N][3]
    std::vector<size_t> mvKeyPointIndices;   // index in the frame
    float fu, fv, uc, vc;          // (double in the reference, set from the float F.fx ...: the library widens them)

    // RANSAC state
    int mnIterations;
    std::vector<uint8_t> mvbBestInliers;
    int mnBestInliers;
    cv::Mat mBestTcw;
    std::vector<int32_t> mvDraws;  // [iterations drawn so far][mRansacMinSet]
    int N;                         // number of correspondences

    double mRansacProb;
    int mRansacMinInliers;
    int mRansacMaxIts;
    float mRansacEpsilon;
    int mRansacMinSet;
    std::vector<float> mvMaxError; // max square error per scale level: sigma2 * th2, a float product
};

}  // namespace ORB_SLAM2
