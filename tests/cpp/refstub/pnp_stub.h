// TEST INFRASTRUCTURE: stand-ins for the members of ORB_SLAM2::Frame and MapPoint that PnPsolver (active-orb-slam2_amd/host/PnPsolver.h)
// touches -- include/Frame.h: mvKeysUn, mvLevelSigma2, mvpMapPoints, the static fx fy cx cy; include/MapPoint.h: isBad(),
// GetWorldPos() -- and for Thirdparty/DBoW2/DUtils/Random.h over a recorded rand() sequence.  A translation unit of its own: the Frame
// of slam_stub.h carries no mvLevelSigma2 and is not included here.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "opencv_stub.h"

namespace ORB_SLAM2 {

class MapPoint {
public:
    cv::Mat GetWorldPos() { return mWorldPos.clone(); }
    void SetWorldPos(const cv::Mat &Pos) { mWorldPos = Pos.clone(); }
    bool isBad() { return mbBad; }
    cv::Mat mWorldPos;
    bool mbBad = false;
};

class Frame {
public:
    static float fx, fy, cx, cy;
    std::vector<cv::KeyPoint> mvKeysUn;
    std::vector<float> mvLevelSigma2;
    std::vector<MapPoint *> mvpMapPoints;
};
inline float Frame::fx = 0, Frame::fy = 0, Frame::cx = 0, Frame::cy = 0;

}  // namespace ORB_SLAM2

// the reference's formula (Random.cpp:47-50) over a recorded rand() sequence
namespace DUtils {
struct Random {
    static std::vector<int32_t> &sequence()
    {
        static std::vector<int32_t> s;
        return s;
    }
    static size_t &position()
    {
        static size_t p = 0;
        return p;
    }
    static int RandomInt(int min, int max)
    {
        if (position() >= sequence().size()) {
            fprintf(stderr, "the recorded rand() sequence is used up\n");
            exit(3);
        }
        int d = max - min + 1;
        return int(((double)sequence()[position()++] / ((double)2147483647 + 1.0)) * d) + min;
    }
};
}  // namespace DUtils
