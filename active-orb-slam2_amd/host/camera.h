// camera at the reference's signatures (include/camera.h:51-129, src/camera.cc), for the planner's call sites that stay as they
// are -- StateValidChecker::isValid / checkMotion (src/StateValidChecker.cc:97-161), which derive from this class and call
// countVisible / IsStateVisiblilty one state at a time -- and with batch members for the call sites that can hand over all their
// states at once: MotionCostCamera (:531-541), plan_slam::AdvanceStepCamera (src/plan.cc:141-151) and RRTstar::display_costs
// (src/myRRTstar.cc:1142-1163).  INTEGRATION.md has the mapping.
//
// The object keeps the map as the reference does (narrowed to float, src/camera.cc:29-44).  The device side is the calling
// thread's visibility handle (aos2_handles.h): the object uploads its constants and its map when the handle holds another
// object's, so the one camera of a plan uploads once and every later call is one C-ABI call.
//
// Left out, on purpose:
//   camera(std::vector<ORB_SLAM2::MapPoint*>&) and update_map (:73-103, :385-420) fill map_vec and the two bounds but leave
//     max_range / min_range / foundRatio empty, and countVisible indexes all three for every point (:156): undefined behaviour in
//     the reference, so there is nothing to reproduce.  A caller with MapPoints builds a map_data and uses camera(map_data, int).
//   isInFrustum with Eigen arguments, the two setRobotPose, posInGrid, computeMatrixStd, read_text*: declared there, no caller
//     outside the class (setRobotPose and computeMatrixStd have no definition at all).
// Include AFTER the headers that declare cv::Mat and map_data (the reference's, or tests/cpp/refstub/camera_stub.h).
#pragma once
#include <atomic>
#include <cstdint>
#include <vector>

#include "aos2_handles.h"

class camera {
public:
    camera(map_data MD, int thres)
    {
        aos2::check(aos2_vis_camera_default(AOS2_VIS_CAMERA_MAP, &mCam), "camera");
        feature_threshold = thres;
        const size_t n = MD.Map.size();
        mXyz.reserve(3 * n);
        for (size_t i = 0; i < n; ++i)
            for (int k = 0; k < 3; ++k) mXyz.push_back((float)MD.Map[i][k]);
        mUpper.assign(MD.UB.begin(), MD.UB.end());
        mLower.assign(MD.LB.begin(), MD.LB.end());
        mMaxRange.assign(MD.maxDist.begin(), MD.maxDist.end());
        mMinRange.assign(MD.minDist.begin(), MD.minDist.end());
        mFoundRatio.assign(MD.foundRatio.begin(), MD.foundRatio.end());
        // the reference reads upper_bound[i] .. foundRatio[i] for every i < Map.size() (:156): shorter vectors are its undefined behaviour
        if (mUpper.size() != n || mLower.size() != n || mMaxRange.size() != n || mMinRange.size() != n || mFoundRatio.size() != n) {
            std::cerr << "camera: map_data's vectors differ in length" << std::endl;
            std::exit(-1);
        }
    }

    camera()
    {
        aos2::check(aos2_vis_camera_default(AOS2_VIS_CAMERA_PLAIN, &mCam), "camera");
        feature_threshold = mCam.feature_threshold;
    }

    int countVisible(float x_w, float y_w, float theta_rad_w) const
    {
        const float state[3] = {x_w, y_w, theta_rad_w};
        int32_t count = 0;
        aos2::check(aos2_vis_count(Handle(), 1, state, &count, nullptr, nullptr), "camera::countVisible");
        return count;
    }

    // Twb: 4x4 CV_32F, as every pose of the reference is
    int countVisible(cv::Mat Twb) const
    {
        float T[16];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) T[4 * r + c] = Twb.at<float>(r, c);
        int32_t count = 0;
        aos2::check(aos2_vis_count_poses(Handle(), 1, T, &count, nullptr, nullptr), "camera::countVisible");
        return count;
    }

    bool IsStateVisiblilty(double x_w, double y_w, double theta_rad_w, int thres = -1)
    {
        const int cur_ths = thres == -1 ? feature_threshold : thres;
        return countVisible(x_w, y_w, theta_rad_w) > cur_ths;
    }

    // ---- batch members (no reference equivalent; a state is a row x, y, theta of doubles, as the planner's ppMatrix holds it)
    // countVisible of every state of Q in one call
    std::vector<int> countVisibleBatch(const std::vector<std::vector<double> > &Q) const
    {
        const std::vector<float> states = Narrow(Q);
        std::vector<int32_t> count(Q.size());
        aos2::check(aos2_vis_count(Handle(), (int)Q.size(), states.data(), count.data(), nullptr, nullptr), "camera::countVisibleBatch");
        return std::vector<int>(count.begin(), count.end());
    }

    // StateValidChecker::MotionCostCamera of every motion in one call, with feature_threshold as it stands
    std::vector<double> MotionCostCameraBatch(const std::vector<std::vector<std::vector<double> > > &motions) const
    {
        std::vector<int32_t> offsets(1, 0);
        std::vector<float> states;
        for (size_t m = 0; m < motions.size(); ++m) {
            const std::vector<float> s = Narrow(motions[m]);
            states.insert(states.end(), s.begin(), s.end());
            offsets.push_back((int32_t)(states.size() / 3));
        }
        std::vector<double> cost(motions.size());
        aos2_vis_t *h = Handle();
        aos2_vis_camera_t cam = mCam;   // the member is public and may have been changed: thres = -1 reads the handle's
        cam.feature_threshold = feature_threshold;
        aos2::check(aos2_vis_set_camera(h, &cam), "camera::MotionCostCameraBatch");
        aos2::check(aos2_vis_motion_costs(h, (int)motions.size(), offsets.data(), states.data(), -1, cost.data()),
                    "camera::MotionCostCameraBatch");
        return cost;
    }

    // plan_slam::AdvanceStepCamera (src/plan.cc:141-151) over this camera: thres == -1 means feature_threshold, as in IsStateVisiblilty
    int AdvanceStepCamera(const std::vector<std::vector<double> > &M, int thres = -1) const
    {
        const std::vector<float> states = Narrow(M);
        int32_t index = -1;
        aos2::check(aos2_vis_advance(Handle(), (int)M.size(), states.data(), thres == -1 ? feature_threshold : thres, &index),
                    "camera::AdvanceStepCamera");
        return index;
    }

    int feature_threshold;

protected:
    // this object's constants and map onto another visibility handle: the one the checker derived from this class owns
    // (host/StateValidChecker.h, aos2_svc_vis)
    void LoadInto(aos2_vis_t *h) const
    {
        aos2::check(aos2_vis_set_camera(h, &mCam), "camera");
        aos2::check(aos2_vis_set_map(h, (int)mUpper.size(), mXyz.data(), mUpper.data(), mLower.data(), mMaxRange.data(), mMinRange.data(),
                                     mFoundRatio.data()),
                    "camera");
    }

private:
    static std::vector<float> Narrow(const std::vector<std::vector<double> > &Q)
    {
        std::vector<float> s;
        s.reserve(3 * Q.size());
        for (size_t i = 0; i < Q.size(); ++i)
            for (int k = 0; k < 3; ++k) s.push_back((float)Q[i][k]);   // the narrowing of countVisible's float parameters
        return s;
    }

    static unsigned long long NextId()
    {
        static std::atomic<unsigned long long> next(1);
        return next++;
    }

    // the thread's handle with this object's constants and map on it
    aos2_vis_t *Handle() const
    {
        aos2::VisibilitySlot &slot = aos2::visibility_slot();
        if (slot.owner != mId) {
            aos2::check(aos2_vis_set_camera(slot.h, &mCam), "camera");
            aos2::check(aos2_vis_set_map(slot.h, (int)mUpper.size(), mXyz.data(), mUpper.data(), mLower.data(), mMaxRange.data(),
                                         mMinRange.data(), mFoundRatio.data()),
                        "camera");
            slot.owner = mId;
        }
        return slot.h;
    }

    aos2_vis_camera_t mCam;
    // a copy of the object holds the same map: it keeps the id
    unsigned long long mId = NextId();
    std::vector<float> mXyz, mUpper, mLower, mMaxRange, mMinRange, mFoundRatio;
};
