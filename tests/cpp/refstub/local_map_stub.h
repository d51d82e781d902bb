// TEST INFRASTRUCTURE: what aos2::LocalMapSnapshot and aos2::UpdateLocalMap (active-orb-slam2_amd/host/LocalMap.h) need from the
// reference's headers -- the members of Map, KeyFrame, MapPoint and Frame that Tracking::UpdateLocalMap reads (include/Map.h,
// include/KeyFrame.h, include/MapPoint.h, include/Frame.h), at their signatures -- so that the class compiles in an image without
// OpenCV, Eigen, DBoW2 and g2o.  Stands alone: not to be combined with slam_stub.h, which declares the same classes for the
// other shims.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <set>
#include <vector>

namespace ORB_SLAM2 {

class KeyFrame;

class MapPoint {
public:
    long unsigned int mnId = 0;
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    std::map<KeyFrame *, size_t> mObservations;
    int nObs = 0;
    bool mbBad = false;
};

class KeyFrame {
public:
    long unsigned int mnId = 0;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &N)
    {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N) return mvpOrderedConnectedKeyFrames;   // src/KeyFrame.cc:195-202
        return std::vector<KeyFrame *>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + N);
    }
    std::set<KeyFrame *> GetChilds() { return mspChildrens; }
    KeyFrame *GetParent() { return mpParent; }
    bool isBad() { return mbBad; }
    std::vector<MapPoint *> mvpMapPoints;
    std::vector<KeyFrame *> mvpOrderedConnectedKeyFrames;
    std::set<KeyFrame *> mspChildrens;
    KeyFrame *mpParent = nullptr;
    bool mbBad = false;
};

class Frame {
public:
    long unsigned int mnId = 0;
    int N = 0;
    std::vector<MapPoint *> mvpMapPoints;
    KeyFrame *mpReferenceKF = nullptr;
};

class Map {
public:
    std::vector<KeyFrame *> GetAllKeyFrames() { return std::vector<KeyFrame *>(mspKeyFrames.begin(), mspKeyFrames.end()); }
    std::vector<MapPoint *> GetAllMapPoints() { return std::vector<MapPoint *>(mspMapPoints.begin(), mspMapPoints.end()); }
    std::mutex mMutexMapUpdate;
    std::set<KeyFrame *> mspKeyFrames;
    std::set<MapPoint *> mspMapPoints;
};

}  // namespace ORB_SLAM2
