// TEST INFRASTRUCTURE: drives camera (active-orb-slam2_amd/host/camera.h) the way StateValidChecker (src/StateValidChecker.cc:97-161,
// :531-541) and plan_slam::AdvanceStepCamera (src/plan.cc:141-151) do, on the stand-ins of tests/cpp/refstub/camera_stub.h, filled
// from a bundle of tests/test_visibility_class_gpu.py:
//   camera_test in.bundle out.bundle
//   in:  xyz f64[n][3], ub / lb / max_dist / min_dist / ratio f64[n]: map_data; thres i32[1]: camera(map_data, thres);
//        states f64[ns][3]; single i32[]: states asked one at a time; poses f32[][16]: T_wb of the same states;
//        mo_off i32[nm+1]: motions as runs of `states`; tr_off i32[nt+1], tr_idx i32[]: trajectories as indices into `states`
//   out: one i32[] countVisible(x, y, theta); one_pose i32[] countVisible(cv::Mat); visible i32[] IsStateVisiblilty(..., -1);
//        visible_40 i32[] IsStateVisiblilty(..., 40); empty i32[] the same states through a camera() (no map) in between;
//        batch i32[ns] countVisibleBatch; cost f64[nm] MotionCostCameraBatch; advance i32[nt] AdvanceStepCamera(.., -1);
//        advance_40 i32[nt] AdvanceStepCamera(.., 40)
#include "refstub/camera_stub.h"

#include "../../active-orb-slam2_amd/host/camera.h"
#include "bundle_io.h"

typedef std::vector<std::vector<double>> ppMatrix;

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bundle out.bundle\n", argv[0]);
        return 2;
    }
    try {
        const Bundle B = Bundle::load(argv[1]);
        const size_t n = B["ub"].count(), ns = B["states"].count() / 3;
        map_data MD;
        const double *xyz = B["xyz"].as<double>();
        for (size_t i = 0; i < n; ++i) MD.Map.push_back({xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 1.0});
        auto vec = [&](const char *k) { return std::vector<double>(B[k].as<double>(), B[k].as<double>() + n); };
        MD.UB = vec("ub"); MD.LB = vec("lb"); MD.maxDist = vec("max_dist"); MD.minDist = vec("min_dist"); MD.foundRatio = vec("ratio");
        camera cam(MD, B["thres"].scalar<int32_t>());
        camera none;
        const double *st = B["states"].as<double>();
        ppMatrix Q;
        for (size_t i = 0; i < ns; ++i) Q.push_back({st[3 * i], st[3 * i + 1], st[3 * i + 2]});

        std::vector<int32_t> one, one_pose, visible, visible_40, empty;
        const int32_t *single = B["single"].as<int32_t>();
        const float *poses = B["poses"].as<float>();
        for (size_t k = 0; k < B["single"].count(); ++k) {
            const std::vector<double> &q = Q[single[k]];
            one.push_back(cam.countVisible(q[0], q[1], q[2]));
            empty.push_back(none.countVisible(q[0], q[1], q[2]));   // another object takes the thread's handle in between
            cv::Mat Twb(4, 4, CV_32F);
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) Twb.at<float>(r, c) = poses[16 * k + 4 * r + c];
            one_pose.push_back(cam.countVisible(Twb));
            visible.push_back(cam.IsStateVisiblilty(q[0], q[1], q[2]) ? 1 : 0);
            visible_40.push_back(cam.IsStateVisiblilty(q[0], q[1], q[2], 40) ? 1 : 0);
        }
        const std::vector<int> batch = cam.countVisibleBatch(Q);
        std::vector<ppMatrix> motions;
        const int32_t *mo = B["mo_off"].as<int32_t>();
        for (size_t m = 0; m + 1 < B["mo_off"].count(); ++m) motions.push_back(ppMatrix(Q.begin() + mo[m], Q.begin() + mo[m + 1]));
        const std::vector<double> cost = cam.MotionCostCameraBatch(motions);
        std::vector<int32_t> advance, advance_40;
        const int32_t *to = B["tr_off"].as<int32_t>(), *ti = B["tr_idx"].as<int32_t>();
        for (size_t t = 0; t + 1 < B["tr_off"].count(); ++t) {
            ppMatrix M;
            for (int32_t j = to[t]; j < to[t + 1]; ++j) M.push_back(Q[ti[j]]);
            advance.push_back(cam.AdvanceStepCamera(M));
            advance_40.push_back(cam.AdvanceStepCamera(M, 40));
        }
        Bundle O;
        O.put("one", 1, one); O.put("one_pose", 1, one_pose); O.put("visible", 1, visible); O.put("visible_40", 1, visible_40);
        O.put("empty", 1, empty);
        O.put("batch", 1, std::vector<int32_t>(batch.begin(), batch.end()));
        O.put("cost", 4, cost);
        O.put("advance", 1, advance); O.put("advance_40", 1, advance_40);
        O.save(argv[2]);
    } catch (const std::exception &e) {
        fprintf(stderr, "camera_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
