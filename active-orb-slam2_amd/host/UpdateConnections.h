// KeyFrame::UpdateConnections (src/KeyFrame.cc:350-440) at the reference's call sites, for one keyframe or a batch:
//
//     // LocalMapping::ProcessNewKeyFrame (src/LocalMapping.cc:168): the new keyframe is not in the snapshot yet.  Nothing extra is
//     // needed -- its own fresh observations would be skipped anyway, and its new points are observed by nobody else:
//     aos2::UpdateConnections(mpCurrentKeyFrame, snapshot);                       // instead of mpCurrentKeyFrame->UpdateConnections();
//
//     // LocalMapping::SearchInNeighbors (:537): Fuse has changed observations.  The snapshot's points and observations must be
//     // current, so Apply the pass's point changes first (host/LocalMap.h):
//     snapshot.Apply(vpTouchedKFs, {}, vpTouchedMPs, mpMap->GetAllMapPoints());
//     aos2::UpdateConnections(mpCurrentKeyFrame, snapshot);
//
//     // LoopClosing::CorrectLoop (src/LoopClosing.cc:434, and the loops at :517 and :556 over every connected keyframe, with the map
//     // mutex held): the same Apply first, then ONE call for the whole loop -- the counting stage reads points and observations
//     // only, never connection weights, so the sequential loop is exact as a batch:
//     aos2::UpdateConnections(vpCorrectedKFs, snapshot);                          // :517, the keyframes of CorrectedSim3
//     // at :550-566 the loop's body reads the keyframe's neighbours in front of the call and behind it; they go in as two hooks:
//     aos2::UpdateConnections(mvpCurrentConnectedKFs, snapshot,
//                             [&](KeyFrame *pKFi) { vpPreviousNeighbors = pKFi->GetVectorCovisibleKeyFrames(); },
//                             [&](KeyFrame *pKFi) { LoopConnections[pKFi] = pKFi->GetConnectedKeyFrames(); /* :558-565 */ });
//
// One C-ABI call (aos2_local_map_update_connections, the explicit-matches form: the matches are pKF->GetMapPointMatches() through
// the snapshot's point rows, the keyframe its row or -1) gives KFcounter and the ordered list of every keyframe.  The verdicts are
// then applied to the pointer graph per keyframe in the vector's order, with the reference's own code: AddConnection(pKF, w) on
// every listed keyframe (weight >= 15, or the single maximum), the three members under mMutexConnections, and on the first
// connection of a keyframe other than mnId 0 its parent, AddChild and the cleared flag.  A keyframe with an empty counter is left
// untouched (:384).  The snapshot is NOT updated: the link rows of the touched keyframes -- each keyframe of the vector and every
// keyframe that got an AddConnection -- go into the next LocalMapSnapshot::Apply as vpRelinkedKFs.  Keyframe rows stand for
// pointer order: the map's iteration order and the tie-break of sort(vPairs).  Include AFTER the
// headers that declare Map, KeyFrame, MapPoint and Frame (the reference's, or tests/cpp/refstub/connections_stub.h).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>

#include "LocalMap.h"

namespace aos2 {

// The connection members of an UNCHANGED reference KeyFrame: protected (include/KeyFrame.h:225-232, 245), reached through member
// pointers formed in a derived class (see KeyFrameEraseFlags, MapPointDistances).  :424-438 as written.
template <class KF>
struct KeyFrameConnectionMembers : KF {
    static void Assign(KF *p, const std::map<KF *, int> &KFcounter, const std::vector<KF *> &vpOrdered, const std::vector<int> &vWeights)
    {
        using M = KeyFrameConnectionMembers;
        std::unique_lock<std::mutex> lockCon(p->*(&M::mMutexConnections));
        p->*(&M::mConnectedKeyFrameWeights) = KFcounter;
        p->*(&M::mvpOrderedConnectedKeyFrames) = vpOrdered;
        p->*(&M::mvOrderedWeights) = vWeights;
        if (p->*(&M::mbFirstConnection) && p->mnId != 0) {
            p->*(&M::mpParent) = vpOrdered.front();
            vpOrdered.front()->AddChild(p);
            p->*(&M::mbFirstConnection) = false;
        }
    }
};

// before(pKF) / after(pKF) run around the application of each keyframe's verdicts, in the vector's order: what the body of a loop
// reads in front of and behind pKF->UpdateConnections() (LoopClosing.cc:553 and :557) sees the pointer graph as the serial loop has it.
template <class Before, class After>
inline void UpdateConnections(const std::vector<ORB_SLAM2::KeyFrame *> &vpKFs, const LocalMapSnapshot &S, Before &&before, After &&after)
{
    ShimClock clk;
    const int n = (int)vpKFs.size();
    std::vector<int32_t> kf(n + 1, -1), n_mp(n + 1, 0);
    std::vector<std::vector<ORB_SLAM2::MapPoint *>> vvpMP(n);
    size_t mp_cap = 1;
    for (int k = 0; k < n; ++k) {
        kf[k] = S.KeyFrameRow(vpKFs[k]);
        vvpMP[k] = vpKFs[k]->GetMapPointMatches();   // :354-359
        n_mp[k] = (int32_t)vvpMP[k].size();
        mp_cap = std::max(mp_cap, vvpMP[k].size());
    }
    std::vector<int32_t> mp((size_t)(n + 1) * mp_cap, -1);
    for (int k = 0; k < n; ++k)
        for (size_t i = 0; i < vvpMP[k].size(); ++i) mp[(size_t)k * mp_cap + i] = S.PointRow(vvpMP[k][i]);
    last_shim_timing().gather_us = clk.lap();
    // a capacity of 256 per list; once more with the largest true count if a row overflowed
    int cap = 256;
    std::vector<int32_t> n_conn(n + 1, 0), n_ordered(n + 1, 0), conn_kf, conn_w, ordered_kf, ordered_w;
    for (;;) {
        conn_kf.assign((size_t)(n + 1) * cap, -1); conn_w.assign((size_t)(n + 1) * cap, 0);
        ordered_kf.assign((size_t)(n + 1) * cap, -1); ordered_w.assign((size_t)(n + 1) * cap, 0);
        check(aos2_local_map_update_connections(S.Handle(), AOS2_CONNECTIONS_TH, n, kf.data(), n_mp.data(), mp.data(), (int)mp_cap,
                                                n_conn.data(), conn_kf.data(), conn_w.data(), cap, n_ordered.data(), ordered_kf.data(),
                                                ordered_w.data(), cap),
              "UpdateConnections");
        int need = 0;
        for (int k = 0; k < n; ++k) need = std::max(need, std::max(n_conn[k], n_ordered[k]));
        if (need <= cap) break;
        cap = need;
    }
    last_shim_timing().call_us = clk.lap();
    const std::vector<ORB_SLAM2::KeyFrame *> &vpRows = S.KeyFrames();
    for (int k = 0; k < n; ++k) {
        ORB_SLAM2::KeyFrame *pKF = vpKFs[k];
        before(pKF);
        if (n_conn[k] == 0) {   // :384
            after(pKF);
            continue;
        }
        std::map<ORB_SLAM2::KeyFrame *, int> KFcounter;
        for (int j = 0; j < n_conn[k]; ++j) KFcounter[vpRows[conn_kf[(size_t)k * cap + j]]] = conn_w[(size_t)k * cap + j];
        std::vector<ORB_SLAM2::KeyFrame *> vpOrdered;
        std::vector<int> vWeights;
        for (int j = 0; j < n_ordered[k]; ++j) {
            ORB_SLAM2::KeyFrame *pKFi = vpRows[ordered_kf[(size_t)k * cap + j]];
            const int w = ordered_w[(size_t)k * cap + j];
            pKFi->AddConnection(pKF, w);   // :405, :412
            vpOrdered.push_back(pKFi);
            vWeights.push_back(w);
        }
        KeyFrameConnectionMembers<ORB_SLAM2::KeyFrame>::Assign(pKF, KFcounter, vpOrdered, vWeights);
        after(pKF);
    }
    last_shim_timing().scatter_us = clk.lap();
}

inline void UpdateConnections(const std::vector<ORB_SLAM2::KeyFrame *> &vpKFs, const LocalMapSnapshot &S)
{
    UpdateConnections(vpKFs, S, [](ORB_SLAM2::KeyFrame *) {}, [](ORB_SLAM2::KeyFrame *) {});
}

inline void UpdateConnections(ORB_SLAM2::KeyFrame *pKF, const LocalMapSnapshot &S)
{
    UpdateConnections(std::vector<ORB_SLAM2::KeyFrame *>(1, pKF), S);
}

}  // namespace aos2
