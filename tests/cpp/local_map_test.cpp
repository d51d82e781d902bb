// TEST INFRASTRUCTURE: drives aos2::LocalMapSnapshot / aos2::UpdateLocalMap (active-orb-slam2_amd/host/LocalMap.h) the way Tracking
// does -- one snapshot of the map, then frame after frame with mvpLocalKeyFrames and mpReferenceKF carried from one frame to the
// next -- on a pointer graph built from the arrays of a bundle.  The keyframes are allocated in descending mnId, so the order of
// their pointers is not the order of their rows.  usage: local_map_test in.bundle out.bundle
#include "refstub/local_map_stub.h"

#include "../../active-orb-slam2_amd/host/LocalMap.h"
#include "bundle_io.h"

#include <memory>

using namespace ORB_SLAM2;

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const Bundle in = Bundle::load(argv[1]);
    const int np = in["n_points"].scalar<int32_t>(), nk = in["n_keyframes"].scalar<int32_t>();
    std::vector<std::unique_ptr<MapPoint>> points(np);
    std::vector<std::unique_ptr<KeyFrame>> kfs(nk);
    for (int k = nk - 1; k >= 0; --k) {
        kfs[k].reset(new KeyFrame());
        kfs[k]->mnId = 10 + 3 * (long unsigned int)k;
        kfs[k]->mbBad = in["kf_bad"].as<int32_t>()[k] != 0;
    }
    Map map;
    std::vector<MapPoint *> table(np);
    for (int p = 0; p < np; ++p) {
        points[p].reset(new MapPoint());
        points[p]->mnId = (long unsigned int)p;
        points[p]->mbBad = in["point_bad"].as<int32_t>()[p] != 0;
        points[p]->nObs = in["point_nobs"].as<int32_t>()[p];
        for (int e = in["obs_off"].as<int32_t>()[p]; e < in["obs_off"].as<int32_t>()[p + 1]; ++e)
            points[p]->mObservations[kfs[in["obs_kf"].as<int32_t>()[e]].get()] = (size_t)e;
        table[p] = points[p].get();
        map.mspMapPoints.insert(table[p]);
    }
    for (int k = 0; k < nk; ++k) {
        KeyFrame *pKF = kfs[k].get();
        for (int e = in["kf_mp_off"].as<int32_t>()[k]; e < in["kf_mp_off"].as<int32_t>()[k + 1]; ++e) {
            const int r = in["kf_mp"].as<int32_t>()[e];
            pKF->mvpMapPoints.push_back(r < 0 ? nullptr : table[r]);
        }
        for (int j = 0; j < 10; ++j) {
            const int r = in["kf_best"].as<int32_t>()[10 * k + j];
            if (r >= 0) pKF->mvpOrderedConnectedKeyFrames.push_back(kfs[r].get());
        }
        for (int e = in["kf_child_off"].as<int32_t>()[k]; e < in["kf_child_off"].as<int32_t>()[k + 1]; ++e)
            pKF->mspChildrens.insert(kfs[in["kf_child"].as<int32_t>()[e]].get());
        const int par = in["kf_parent"].as<int32_t>()[k];
        pKF->mpParent = par < 0 ? nullptr : kfs[par].get();
        map.mspKeyFrames.insert(pKF);
    }
    aos2::LocalMapSnapshot snapshot(&map, table);
    const int B = (int)in["n"].count(), cap = (int)in["mp"].dims[1];
    std::vector<int32_t> mp_out((size_t)B * cap, -1), kf_off(1, 0), kf_rows, pt_off(1, 0), pt_rows, ref(B, -1);
    std::vector<KeyFrame *> vpLocalKeyFrames;
    std::vector<MapPoint *> vpLocalMapPoints;
    KeyFrame *pReferenceKF = nullptr;
    for (int b = 0; b < B; ++b) {
        Frame F;
        F.mnId = (long unsigned int)b;
        F.N = in["n"].as<int32_t>()[b];
        for (int i = 0; i < F.N; ++i) {
            const int r = in["mp"].as<int32_t>()[(size_t)b * cap + i];
            F.mvpMapPoints.push_back(r < 0 ? nullptr : table[r]);
        }
        aos2::UpdateLocalMap(F, snapshot, vpLocalKeyFrames, vpLocalMapPoints, pReferenceKF);
        for (int i = 0; i < F.N; ++i) mp_out[(size_t)b * cap + i] = F.mvpMapPoints[i] ? (int32_t)F.mvpMapPoints[i]->mnId : -1;
        for (KeyFrame *pKF : vpLocalKeyFrames) kf_rows.push_back((int32_t)((pKF->mnId - 10) / 3));
        for (MapPoint *pMP : vpLocalMapPoints) pt_rows.push_back((int32_t)pMP->mnId);
        kf_off.push_back((int32_t)kf_rows.size());
        pt_off.push_back((int32_t)pt_rows.size());
        ref[b] = pReferenceKF ? (int32_t)((pReferenceKF->mnId - 10) / 3) : -1;
    }
    Bundle out;
    out.put("mp", 1, mp_out, {(uint64_t)B, (uint64_t)cap});
    out.put("kf_off", 1, kf_off);
    out.put("kf_rows", 1, kf_rows);
    out.put("pt_off", 1, pt_off);
    out.put("pt_rows", 1, pt_rows);
    out.put("ref", 1, ref);
    out.save(argv[2]);
    return 0;
}
