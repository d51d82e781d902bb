// TEST INFRASTRUCTURE: drives aos2::TriangulateMatches (active-orb-slam2_amd/host/NewMapPoints.h) the way
// LocalMapping::CreateNewMapPoints would (src/LocalMapping.cc:272-436), on KeyFrame stand-ins (tests/cpp/refstub) filled from a
// bundle of tests/test_triangulate_gpu.py:  new_map_points_test in.bundle out.bundle
//   in:  per keyframe k = 1, 2: kf<k>_Tcw f32[16], kf<k>_cam f32[6] (fx fy cx cy mb mbf), kf<k>_sf f32[levels],
//        kf<k>_obs f32[N][6] (mvKeysUn x y, mvKeys x y, mvuRight, mvDepth), kf<k>_octave i32[N]; matches i32[n][2]
//   out: status u8[n], x3D f32[n][3] (zeros where the shim returned an empty Mat), has_x3D u8[n]
#include <cstdio>

#include "refstub/slam_stub.h"

#include "../../active-orb-slam2_amd/host/NewMapPoints.h"
#include "bundle_io.h"

static void fill(ORB_SLAM2::KeyFrame &K, const Bundle &B, const std::string &p)
{
    const float *T = B[p + "Tcw"].as<float>(), *cam = B[p + "cam"].as<float>();
    cv::Mat Tcw(4, 4, CV_32F);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) Tcw.at<float>(r, c) = T[4 * r + c];
    K.SetPose(Tcw);
    K.fx = cam[0]; K.fy = cam[1]; K.cx = cam[2]; K.cy = cam[3]; K.mb = cam[4]; K.mbf = cam[5];
    const BundleArray &sf = B[p + "sf"];
    K.mvScaleFactors.assign(sf.as<float>(), sf.as<float>() + sf.count());
    const BundleArray &obs = B[p + "obs"];
    const int32_t *oct = B[p + "octave"].as<int32_t>();
    K.N = (int)obs.dims[0];
    K.mvKeys.resize(K.N); K.mvKeysUn.resize(K.N); K.mvuRight.resize(K.N); K.mvDepth.resize(K.N);
    for (int i = 0; i < K.N; ++i) {
        const float *o = obs.as<float>() + 6 * (size_t)i;
        K.mvKeysUn[i].pt = cv::Point2f(o[0], o[1]);
        K.mvKeys[i].pt = cv::Point2f(o[2], o[3]);
        K.mvKeysUn[i].octave = K.mvKeys[i].octave = oct[i];
        K.mvuRight[i] = o[4];
        K.mvDepth[i] = o[5];
    }
}

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bundle out.bundle\n", argv[0]);
        return 2;
    }
    try {
        const Bundle B = Bundle::load(argv[1]);
        ORB_SLAM2::KeyFrame K1, K2;
        fill(K1, B, "kf1_");
        fill(K2, B, "kf2_");
        const BundleArray &m = B["matches"];
        std::vector<std::pair<size_t, size_t>> vMatchedIndices;
        for (size_t k = 0; k < (size_t)m.dims[0]; ++k) vMatchedIndices.emplace_back((size_t)m.as<int32_t>()[2 * k], (size_t)m.as<int32_t>()[2 * k + 1]);
        std::vector<cv::Mat> x3D;
        std::vector<uint8_t> status;
        aos2::TriangulateMatches(&K1, &K2, vMatchedIndices, x3D, status);
        const size_t n = vMatchedIndices.size();
        std::vector<float> pts(3 * n, 0.0f);
        std::vector<uint8_t> has(n, 0);
        for (size_t k = 0; k < n; ++k) {
            if (x3D[k].empty()) continue;
            if (x3D[k].rows != 3 || x3D[k].cols != 1) throw std::runtime_error("x3D is not 3x1");
            has[k] = 1;
            for (int r = 0; r < 3; ++r) pts[3 * k + r] = x3D[k].at<float>(r);
        }
        Bundle O;
        O.put("status", 0, status);
        O.put("x3D", 2, pts, {(uint64_t)n, 3});
        O.put("has_x3D", 0, has);
        O.save(argv[2]);
    } catch (const std::exception &e) {
        fprintf(stderr, "new_map_points_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
