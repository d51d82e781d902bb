// TEST INFRASTRUCTURE: what aos2::LocalMapSnapshot, aos2::CullingView and aos2::UpdateNormalAndDepth
// (active-orb-slam2_amd/host/LocalMap.h, host/KeyFrameCulling.h, host/UpdateNormalAndDepth.h) need from the reference's headers --
// the members of Map, KeyFrame, MapPoint and Frame that MapPoint::UpdateNormalAndDepth and the snapshot's walk touch (include/Map.h,
// include/KeyFrame.h, include/MapPoint.h, include/Frame.h), at their signatures and with the same access: mWorldPos, mNormalVector,
// mpRefKF, mfMinDistance, mfMaxDistance and mMutexPos of MapPoint are PROTECTED here as they are there, mNormalVectors,
// theta_sVector, theta_mean and theta_std public -- so that the classes compile in an image without OpenCV, Eigen, DBoW2 and g2o.
// cv::Mat is the one of opencv_stub.h.  Stands alone: not to be combined with the other class stubs of this directory, which declare
// the same classes for the other shims.
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <set>
#include <vector>

#include "opencv_stub.h"

namespace ORB_SLAM2 {

class KeyFrame;

class MapPoint {
public:
    long unsigned int mnId = 0;
    std::map<KeyFrame *, size_t> GetObservations() { return mObservations; }
    int Observations() { return nObs; }
    bool isBad() { return mbBad; }
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    cv::Mat GetNormal() { return mNormalVector.clone(); }
    KeyFrame *GetReferenceKeyFrame() { return mpRefKF; }
    float GetMinDistanceInvariance() { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() { return 1.2f * mfMaxDistance; }
    // test set-up (the reference's constructors, AddObservation, SetWorldPos and SetBadFlag do more)
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }
    void SetReferenceKeyFrame(KeyFrame *pKF) { mpRefKF = pKF; }
    void AddObservation(KeyFrame *pKF, size_t idx)
    {
        if (mObservations.count(pKF)) return;
        mObservations[pKF] = idx;
        nObs++;
    }
    void SetBad() { mbBad = true; }
    int nObs = 0;

    std::vector<cv::Mat> mNormalVectors;
    std::vector<float> theta_sVector;
    float theta_mean = 0.f;
    float theta_std = 0.f;

protected:
    cv::Mat mWorldPos;
    std::map<KeyFrame *, size_t> mObservations;
    cv::Mat mNormalVector;
    KeyFrame *mpRefKF = nullptr;
    bool mbBad = false;
    float mfMinDistance = 0.f, mfMaxDistance = 0.f;
    std::mutex mMutexPos;
};

class KeyFrame {
public:
    long unsigned int mnId = 0;
    std::vector<MapPoint *> GetMapPointMatches() { return mvpMapPoints; }
    std::vector<KeyFrame *> GetVectorCovisibleKeyFrames() { return std::vector<KeyFrame *>(); }
    std::vector<KeyFrame *> GetBestCovisibilityKeyFrames(const int &) { return std::vector<KeyFrame *>(); }
    std::set<KeyFrame *> GetChilds() { return std::set<KeyFrame *>(); }
    KeyFrame *GetParent() { return nullptr; }
    bool isBad() { return false; }
    void SetBadFlag() {}   // (host/KeyFrameCulling.h, which declares the view, calls it; nothing is culled here)
    cv::Mat GetCameraCenter() { return Ow.clone(); }
    void AddMapPoint(MapPoint *pMP, const size_t &idx) { mvpMapPoints[idx] = pMP; }

    explicit KeyFrame(size_t N = 0) : mvKeysUn(N), mvuRight(N, -1.f), mvDepth(N, -1.f), mvpMapPoints(N, static_cast<MapPoint *>(NULL)) {}

    float mThDepth = 0.f;
    int mnScaleLevels = 0;
    std::vector<float> mvScaleFactors;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<float> mvDepth;
    cv::Mat Ow;   // (protected in the reference, behind GetCameraCenter; the test places the cameras through it)

protected:
    std::vector<MapPoint *> mvpMapPoints;
    bool mbNotErase = false;
    bool mbToBeErased = false;
    std::mutex mMutexConnections;
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
    void AddKeyFrame(KeyFrame *pKF) { mspKeyFrames.insert(pKF); }
    void AddMapPoint(MapPoint *pMP) { mspMapPoints.insert(pMP); }
    std::vector<KeyFrame *> GetAllKeyFrames() { return std::vector<KeyFrame *>(mspKeyFrames.begin(), mspKeyFrames.end()); }
    std::vector<MapPoint *> GetAllMapPoints() { return std::vector<MapPoint *>(mspMapPoints.begin(), mspMapPoints.end()); }
    std::mutex mMutexMapUpdate;

protected:
    std::set<KeyFrame *> mspKeyFrames;
    std::set<MapPoint *> mspMapPoints;
};

}  // namespace ORB_SLAM2
