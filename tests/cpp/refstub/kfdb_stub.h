// TEST INFRASTRUCTURE: stand-ins for the members of ORB_SLAM2::KeyFrame and Frame that KeyFrameDatabase
// (active-orb-slam2_amd/host/KeyFrameDatabase.h) touches -- include/KeyFrame.h: mnId, mBowVec, mnLoopQuery, mnLoopWords, mLoopScore,
// mnRelocQuery, mnRelocWords, mRelocScore, GetConnectedKeyFrames(), GetBestCovisibilityKeyFrames(N); include/Frame.h: mnId, mBowVec --
// and for DBoW2::BowVector.  A translation unit of its own: the KeyFrame of slam_stub.h has no covisibility accessors and no query
// members, and is not included here.  mRelocScore starts at 0 (the reference leaves it uninitialised).
#pragma once
#include <map>
#include <set>
#include <vector>

#include "opencv_stub.h"

namespace DBoW2 {
typedef unsigned int WordId;   // Thirdparty/DBoW2/DBoW2/BowVector.h:20
typedef double WordValue;      // :23
typedef unsigned int NodeId;   // :26
class BowVector : public std::map<WordId, WordValue> {};
class FeatureVector : public std::map<NodeId, std::vector<unsigned int>> {};
}  // namespace DBoW2

namespace ORB_SLAM2 {

class KeyFrame {
public:
    std::set<KeyFrame *> GetConnectedKeyFrames() { return mspConnected; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }

    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
    // Variables used by the keyframe database
    long unsigned int mnLoopQuery = 0;
    int mnLoopWords = 0;
    float mLoopScore = 0;
    long unsigned int mnRelocQuery = 0;
    int mnRelocWords = 0;
    float mRelocScore = 0;

    std::set<KeyFrame *> mspConnected;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
};

class Frame {
public:
    long unsigned int mnId = 0;
    DBoW2::BowVector mBowVec;
};

}  // namespace ORB_SLAM2
