// ORB_SLAM2::Initializer at the reference's signature (include/Initializer.h:38-44, src/Initializer.cc:33-121), for
// Tracking::MonocularInitialization (src/Tracking.cc:659-760), whose lines stay as they are:
//
//     mpInitializer = new Initializer(mCurrentFrame, 1.0, 200);                                                   // :675
//     if (mpInitializer->Initialize(mCurrentFrame, mvIniMatches, Rcw, tcw, mvIniP3D, vbTriangulated))             // :709
//
// Initialize() keeps :49-97 literally -- mvMatches12, mvbMatched1, DUtils::Random::SeedRandOnce(0), the 8 draws per iteration with
// the swap-with-back removal -- and then makes ONE C-ABI call (aos2_initializer_initialize: Normalize, the 2 x mMaxIterations models
// and their scores, the pick, ReconstructH or ReconstructF with CheckRT of every hypothesis, all on the GPU).  From the result it
// writes R21, t21 (3x3 and 3x1 CV_32F; empty Mats on failure, as :501-502 leaves them), vP3D and vbTriangulated.
// Where the reference would assert on an empty model matrix (no hypothesis scored above 0), the call reports
// AOS2_INIT_NO_MODEL and Initialize() returns false.
// Include AFTER the headers that declare Frame and DUtils::Random (the reference's, or tests/cpp/refstub/initializer_stub.h).
#pragma once
#include <cstdint>
#include <utility>
#include <vector>

#include "aos2_handles.h"

namespace ORB_SLAM2 {

class Initializer {
    typedef std::pair<int, int> Match;

public:
    // Fix the reference frame
    Initializer(const Frame &ReferenceFrame, float sigma = 1.0, int iterations = 200)
    {
        mK = ReferenceFrame.mK.clone();
        mvKeys1 = ReferenceFrame.mvKeysUn;
        mSigma = sigma;
        mSigma2 = sigma * sigma;
        mMaxIterations = iterations;
    }

    // Computes in parallel a fundamental matrix and a homography, selects a model and tries to recover the motion and the structure
    bool Initialize(const Frame &CurrentFrame, const std::vector<int> &vMatches12, cv::Mat &R21, cv::Mat &t21, std::vector<cv::Point3f> &vP3D,
                    std::vector<bool> &vbTriangulated)
    {
        aos2::ShimClock clk;
        // Fill structures with current keypoints and matches with reference frame
        // Reference Frame: 1, Current Frame: 2
        mvKeys2 = CurrentFrame.mvKeysUn;

        mvMatches12.clear();
        mvMatches12.reserve(mvKeys2.size());
        mvbMatched1.resize(mvKeys1.size());
        for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {
            if (vMatches12[i] >= 0) {
                mvMatches12.push_back(std::make_pair(i, vMatches12[i]));
                mvbMatched1[i] = true;
            } else
                mvbMatched1[i] = false;
        }

        const int N = mvMatches12.size();

        // Indices for minimum set selection
        std::vector<size_t> vAllIndices;
        vAllIndices.reserve(N);
        std::vector<size_t> vAvailableIndices;

        for (int i = 0; i < N; i++) {
            vAllIndices.push_back(i);
        }

        // Generate sets of 8 points for each RANSAC iteration
        mvSets = std::vector<std::vector<size_t>>(mMaxIterations, std::vector<size_t>(8, 0));

        DUtils::Random::SeedRandOnce(0);

        if (N < 8) aos2::fail("Initializer: fewer than 8 matches to draw a minimal set from");
        for (int it = 0; it < mMaxIterations; it++) {
            vAvailableIndices = vAllIndices;

            // Select a minimum set
            for (size_t j = 0; j < 8; j++) {
                int randi = DUtils::Random::RandomInt(0, vAvailableIndices.size() - 1);
                int idx = vAvailableIndices[randi];

                mvSets[it][j] = idx;

                vAvailableIndices[randi] = vAvailableIndices.back();
                vAvailableIndices.pop_back();
            }
        }

        // the problem: both frames' keys as float pairs, the matches, the sets
        std::vector<float> keys1(2 * mvKeys1.size()), keys2(2 * mvKeys2.size());
        for (size_t i = 0; i < mvKeys1.size(); i++) {
            keys1[2 * i] = mvKeys1[i].pt.x;
            keys1[2 * i + 1] = mvKeys1[i].pt.y;
        }
        for (size_t i = 0; i < mvKeys2.size(); i++) {
            keys2[2 * i] = mvKeys2[i].pt.x;
            keys2[2 * i + 1] = mvKeys2[i].pt.y;
        }
        std::vector<int32_t> matches(2 * (size_t)N), sets(8 * (size_t)mMaxIterations);
        for (int i = 0; i < N; i++) {
            matches[2 * i] = mvMatches12[i].first;
            matches[2 * i + 1] = mvMatches12[i].second;
        }
        for (int it = 0; it < mMaxIterations; it++)
            for (size_t j = 0; j < 8; j++) sets[8 * (size_t)it + j] = (int32_t)mvSets[it][j];
        aos2_initializer_problem_t P = {};
        P.n_keys1 = (int32_t)mvKeys1.size();
        P.n_keys2 = (int32_t)mvKeys2.size();
        P.keys1 = keys1.data();
        P.keys2 = keys2.data();
        P.n_matches = N;
        P.matches = matches.data();
        P.sigma = mSigma;
        P.iterations = mMaxIterations;
        P.sets = sets.data();
        P.fx = mK.at<float>(0, 0);
        P.fy = mK.at<float>(1, 1);
        P.cx = mK.at<float>(0, 2);
        P.cy = mK.at<float>(1, 2);
        P.min_parallax = 1.0;      // :116, :118
        P.min_triangulated = 50;
        std::vector<uint8_t> inliersH((size_t)N), inliersF((size_t)N), triangulated(mvKeys1.size());
        std::vector<float> P3D(3 * mvKeys1.size());
        aos2_initializer_result_t R = {};
        R.inliers_h = inliersH.data();
        R.inliers_f = inliersF.data();
        R.P3D = P3D.data();
        R.triangulated = triangulated.data();
        aos2::last_shim_timing().gather_us = clk.lap();
        aos2::check(aos2_initializer_initialize(aos2::matcher_handle(0.9f, true), &P, &R, 1), "Initializer");
        aos2::last_shim_timing().call_us = clk.lap();

        R21 = cv::Mat();
        t21 = cv::Mat();
        if (R.status != AOS2_INIT_OK || !R.initialized) return false;
        R21 = cv::Mat(3, 3, CV_32F);
        t21 = cv::Mat(3, 1, CV_32F);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) R21.at<float>(r, c) = R.R21[3 * r + c];
            t21.at<float>(r) = R.t21[r];
        }
        vP3D.resize(mvKeys1.size());
        vbTriangulated = std::vector<bool>(mvKeys1.size(), false);
        for (size_t i = 0; i < mvKeys1.size(); i++) {
            vP3D[i] = cv::Point3f(P3D[3 * i], P3D[3 * i + 1], P3D[3 * i + 2]);
            vbTriangulated[i] = triangulated[i] != 0;
        }
        aos2::last_shim_timing().scatter_us = clk.lap();
        return true;
    }

private:
    // Keypoints from Reference Frame (Frame 1)
    std::vector<cv::KeyPoint> mvKeys1;

    // Keypoints from Current Frame (Frame 2)
    std::vector<cv::KeyPoint> mvKeys2;

    // Current Matches from Reference to Current
    std::vector<Match> mvMatches12;
    std::vector<bool> mvbMatched1;

    // Calibration
    cv::Mat mK;

    // Standard Deviation and Variance
    float mSigma, mSigma2;

    // Ransac max iterations
    int mMaxIterations;

    // Ransac sets
    std::vector<std::vector<size_t>> mvSets;
};

}  // namespace ORB_SLAM2
