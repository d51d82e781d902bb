// TEST INFRASTRUCTURE: what StateValidChecker (active-orb-slam2_amd/host/StateValidChecker.h) needs from the reference's headers --
// map_data and cv::Mat (camera_stub.h) -- and a stand-in for ob::RealVectorStateSpace::StateType, of which the class reads
// values[i] only, so that it compiles in an image without OpenCV, Eigen and OMPL.
#pragma once
#include "camera_stub.h"

namespace ob {
struct RealVectorState {
    double *values;
};
}  // namespace ob
