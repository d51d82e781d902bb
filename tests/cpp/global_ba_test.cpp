// TEST INFRASTRUCTURE: drives ORB_SLAM2::Optimizer::GlobalBundleAdjustemnt (active-orb-slam2_amd/host/GlobalBundleAdjustment.h) the way
// LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:652) and Tracking::CreateInitialMapMonocular (src/Tracking.cc:781) do, on
// a pointer graph of stand-ins (tests/cpp/refstub/global_ba_stub.h) filled from a bundle of tests/test_global_ba_class_gpu.py:
//   global_ba_test in.bundle out.bundle
//   in:  params i32[3] (nIterations, nLoopKF, bRobust); cam f32[5] (fx, fy, cx, cy, mbf); inv_sigma2 f32[levels];
//        keyframes k = 0..n-1 in storage order (= the order of Map::GetAllKeyFrames): kf_id i32[n] (mnId), kf_bad u8[n], kf_Tcw f32[n][16];
//        map points j = 0..M-1 in the order of Map::GetAllMapPoints: mp_id i32[M], mp_bad u8[M], mp_pos f32[M][3];
//        observations: e_kf i32[E], e_mp i32[E], e_obs f32[E][3] (kpUn.pt.x, .pt.y, mvuRight), e_octave i32[E]
//   out: kf_Tcw f32[n][16] (GetPose), kf_TcwGBA f32[n][16] (zeros where empty), kf_gba i64[n] (mnBAGlobalForKF), mp_pos f32[M][3],
//        mp_posGBA f32[M][3], mp_gba i64[M], mp_updates i32[M] (UpdateNormalAndDepth calls), log i64[] (the write log of the stub)
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "refstub/global_ba_stub.h"

#include "../../active-orb-slam2_amd/host/Optimizer.h"
#include "../../active-orb-slam2_amd/host/GlobalBundleAdjustment.h"
#include "bundle_io.h"

int main(int argc, char **argv)
{
    if (argc != 3) {
        fprintf(stderr, "usage: %s in.bundle out.bundle\n", argv[0]);
        return 2;
    }
    try {
        const Bundle B = Bundle::load(argv[1]);
        const int32_t *prm = B["params"].as<int32_t>();
        const float *cam = B["cam"].as<float>();
        const size_t n = B["kf_id"].count(), M = B["mp_id"].count(), E = B["e_kf"].count();
        std::vector<ORB_SLAM2::KeyFrame> kf(n);
        std::vector<ORB_SLAM2::MapPoint> mp(M);
        ORB_SLAM2::Map map;
        for (size_t k = 0; k < n; ++k) {
            kf[k].mnId = (long unsigned int)B["kf_id"].as<int32_t>()[k];
            kf[k].mbBad = B["kf_bad"].as<uint8_t>()[k] != 0;
            kf[k].fx = cam[0]; kf[k].fy = cam[1]; kf[k].cx = cam[2]; kf[k].cy = cam[3]; kf[k].mbf = cam[4];
            kf[k].mvInvLevelSigma2.assign(B["inv_sigma2"].as<float>(), B["inv_sigma2"].as<float>() + B["inv_sigma2"].count());
            cv::Mat T(4, 4, CV_32F);
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) T.at<float>(r, c) = B["kf_Tcw"].as<float>()[16 * k + 4 * r + c];
            kf[k].Tcw = T;
            map.mvpKeyFrames.push_back(&kf[k]);
            map.mnMaxKFid = std::max(map.mnMaxKFid, kf[k].mnId);
        }
        for (size_t j = 0; j < M; ++j) {
            mp[j].mnId = (long unsigned int)B["mp_id"].as<int32_t>()[j];
            mp[j].mbBad = B["mp_bad"].as<uint8_t>()[j] != 0;
            cv::Mat X(3, 1, CV_32F);
            for (int r = 0; r < 3; ++r) X.at<float>(r) = B["mp_pos"].as<float>()[3 * j + r];
            mp[j].mWorldPos = X;
            map.mvpMapPoints.push_back(&mp[j]);
        }
        for (size_t e = 0; e < E; ++e) {
            ORB_SLAM2::KeyFrame &K = kf[B["e_kf"].as<int32_t>()[e]];
            const float *o = B["e_obs"].as<float>() + 3 * e;
            cv::KeyPoint kp;
            kp.pt.x = o[0];
            kp.pt.y = o[1];
            kp.octave = B["e_octave"].as<int32_t>()[e];
            mp[B["e_mp"].as<int32_t>()[e]].mObservations[&K] = K.mvKeysUn.size();
            K.mvKeysUn.push_back(kp);
            K.mvuRight.push_back(o[2]);
        }
        bool stop = false;
        ORB_SLAM2::Optimizer::GlobalBundleAdjustemnt(&map, prm[0], &stop, (unsigned long)prm[1], prm[2] != 0);
        std::vector<float> Tcw(16 * n), TcwGBA(16 * n, 0.f), pos(3 * M), posGBA(3 * M, 0.f);
        std::vector<int64_t> kf_gba(n), mp_gba(M);
        std::vector<int32_t> updates(M);
        for (size_t k = 0; k < n; ++k) {
            for (int r = 0; r < 4; ++r)
                for (int c = 0; c < 4; ++c) {
                    Tcw[16 * k + 4 * r + c] = kf[k].Tcw.at<float>(r, c);
                    if (!kf[k].mTcwGBA.empty()) TcwGBA[16 * k + 4 * r + c] = kf[k].mTcwGBA.at<float>(r, c);
                }
            kf_gba[k] = (int64_t)kf[k].mnBAGlobalForKF;
        }
        for (size_t j = 0; j < M; ++j) {
            for (int r = 0; r < 3; ++r) {
                pos[3 * j + r] = mp[j].mWorldPos.at<float>(r);
                if (!mp[j].mPosGBA.empty()) posGBA[3 * j + r] = mp[j].mPosGBA.at<float>(r);
            }
            mp_gba[j] = (int64_t)mp[j].mnBAGlobalForKF;
            updates[j] = mp[j].nNormalUpdates;
        }
        std::vector<int64_t> log(ORB_SLAM2::write_log().begin(), ORB_SLAM2::write_log().end());
        Bundle O;
        O.put("kf_Tcw", 2, Tcw);
        O.put("kf_TcwGBA", 2, TcwGBA);
        O.put("kf_gba", 3, kf_gba);
        O.put("mp_pos", 2, pos);
        O.put("mp_posGBA", 2, posGBA);
        O.put("mp_gba", 3, mp_gba);
        O.put("mp_updates", 1, updates);
        O.put("log", 3, log);
        O.save(argv[2]);
    } catch (const std::exception &e) {
        fprintf(stderr, "global_ba_test: %s\n", e.what());
        return 1;
    }
    return 0;
}
