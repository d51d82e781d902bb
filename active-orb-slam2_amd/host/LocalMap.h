// Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) at the reference's call site, the first line of Tracking::TrackLocalMap (:1034):
//
//     // once per map change (a keyframe inserted, points culled), under mpMap->mMutexMapUpdate like Tracking's own reads:
//     aos2::LocalMapSnapshot snapshot(mpMap, mpMap->GetAllMapPoints());
//     ...
//     // per frame, instead of UpdateLocalMap():
//     aos2::UpdateLocalMap(mCurrentFrame, snapshot, mvpLocalKeyFrames, mvpLocalMapPoints, mpReferenceKF);
//     mCurrentFrame.mpReferenceKF = mpReferenceKF;                      // :1517
//     mpMap->SetReferenceMapPoints(mvpLocalMapPoints);                  // :1378 (visualisation; the reference sets the previous list)
//
// The snapshot walks the pointer graph ONCE into the arrays of aos2_local_map_graph_t and uploads them (aos2_local_map_set); a frame
// then costs one C-ABI call (aos2_local_map_update: the votes, the keyframe list, the ordered point list, all on the GPU) and the
// walk back from rows to pointers.  Keyframe rows are ascending mnId -- the order that stands for the reference's pointer-ordered
// containers -- and point rows are the caller's table.  A map point outside the table is NULL to the
// snapshot, a keyframe added after the snapshot does not exist for it until LocalMapSnapshot::Apply names it.
//
// When the map changes the snapshot takes the change as a DELTA (aos2_local_map_apply: only the named rows cross PCIe, the new
// arrays are built on the device): Apply re-reads ONLY the objects it is given.  One pass of LocalMapping::Run (src/LocalMapping.cc:
// 49-107), under mpMap->mMutexMapUpdate, with the lists the steps already have in hand:
//
//     ProcessNewKeyFrame();  MapPointCulling();  CreateNewMapPoints();  SearchInNeighbors();
//     Optimizer::LocalBundleAdjustment(...);  KeyFrameCulling();
//     // touched: mpCurrentKeyFrame and every keyframe whose mvpMapPoints changed (Fuse / Replace targets, EraseMapPointMatch of a
//     // culled or outlier point); relinked: mpCurrentKeyFrame, its covisibles (UpdateConnections), every keyframe that went bad and the
//     // parents / children its spanning-tree update reached; points: created, culled, fused, replaced, and every point that gained or
//     // lost an observation (the matches of mpCurrentKeyFrame, the points of a culled keyframe)
//     snapshot.Apply(vpTouchedKFs, vpRelinkedKFs, vpTouchedMPs, mpMap->GetAllMapPoints() /* the table, grown at its END */,
//                    aos2::CullingView());
//
// Include AFTER the headers that declare Map, KeyFrame, MapPoint and Frame (the reference's, or tests/cpp/refstub/local_map_stub.h);
// nothing of the reference's data model changes.
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <set>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "aos2_handles.h"

namespace aos2 {

// the hooks of the snapshot's walk for what one more consumer reads (host/KeyFrameCulling.h: aos2::CullingView); this one gathers
// nothing
struct NoSnapshotView {
    static constexpr bool kGathers = false;
    template <class KF> void KeyFrame(KF *) {}
    void Observation(size_t) {}
    void Set(aos2_local_map_t *) {}
    // ... and of LocalMapSnapshot::Apply: DeltaObservation(idx) for every entry of the delta's obs_kf, DeltaMatches(pKF) for every
    // match row, DeltaLinks(pKF) for every link row, PointDelta(d) in front of aos2_local_map_apply
    void DeltaObservation(size_t) {}
    template <class KF> void DeltaMatches(KF *) {}
    template <class KF> void DeltaLinks(KF *) {}
    void PointDelta(aos2_local_map_delta_t &d) { d.view = nullptr; }
};

// a failure of the shim's own preconditions, reported like aos2::fail reports the library's
[[noreturn]] inline void fail_precondition(const char *what, const char *why)
{
#ifdef AOS2_HOST_EXCEPTIONS
    throw std::runtime_error(std::string(what) + ": " + why);
#else
    std::cerr << what << ": " << why << std::endl;
    std::exit(-1);
#endif
}

class LocalMapSnapshot {
public:
    LocalMapSnapshot(ORB_SLAM2::Map *pMap, const std::vector<ORB_SLAM2::MapPoint *> &vpTable) : mvpPoints(vpTable)
    {
        NoSnapshotView none;
        Build(pMap, none);
    }
    // ... with a view gathered in the same walk, so that its arrays line up with the graph's: view.Observation(idx) for every entry
    // of obs_kf, view.KeyFrame(pKF) for every keyframe in row order, view.Set(handle) behind aos2_local_map_set
    template <class View>
    LocalMapSnapshot(ORB_SLAM2::Map *pMap, const std::vector<ORB_SLAM2::MapPoint *> &vpTable, View &&view) : mvpPoints(vpTable)
    {
        Build(pMap, view);
    }

private:
    template <class View>
    void Build(ORB_SLAM2::Map *pMap, View &view)
    {
        mbHasView = std::decay<View>::type::kGathers;
        mvpKeyFrames = pMap->GetAllKeyFrames();
        std::sort(mvpKeyFrames.begin(), mvpKeyFrames.end(),
                  [](ORB_SLAM2::KeyFrame *a, ORB_SLAM2::KeyFrame *b) { return a->mnId < b->mnId; });
        for (size_t k = 0; k < mvpKeyFrames.size(); ++k) mKeyFrameRow[mvpKeyFrames[k]] = (int32_t)k;
        for (size_t p = 0; p < mvpPoints.size(); ++p)
            if (mvpPoints[p]) mPointRow[mvpPoints[p]] = (int32_t)p;
        const size_t np = mvpPoints.size(), nk = mvpKeyFrames.size();
        std::vector<uint8_t> point_bad(np, 1), kf_bad(nk);   // (an empty slot of the table is a bad point: never listed, never votes)
        std::vector<int32_t> point_nobs(np, 0), obs_off(1, 0), obs_kf, kf_mp_off(1, 0), kf_mp, kf_best(nk * AOS2_LOCAL_MAP_NEIGHBOURS, -1),
            kf_child_off(1, 0), kf_child, kf_parent(nk, -1);
        for (size_t p = 0; p < np; ++p) {
            if (ORB_SLAM2::MapPoint *pMP = mvpPoints[p]) {
                point_bad[p] = pMP->isBad() ? 1 : 0;
                point_nobs[p] = pMP->Observations();
                std::map<int32_t, size_t> rows;   // (a keyframe once, in ascending row, with the feature that observes the point)
                const std::map<ORB_SLAM2::KeyFrame *, size_t> observations = pMP->GetObservations();
                for (const auto &ob : observations) {
                    const int32_t r = KeyFrameRow(ob.first);
                    if (r >= 0) rows.insert(std::make_pair(r, ob.second));
                }
                for (const auto &row : rows) {
                    obs_kf.push_back(row.first);
                    view.Observation(row.second);
                }
            }
            obs_off.push_back((int32_t)obs_kf.size());
        }
        for (size_t k = 0; k < nk; ++k) {
            ORB_SLAM2::KeyFrame *pKF = mvpKeyFrames[k];
            kf_bad[k] = pKF->isBad() ? 1 : 0;
            const std::vector<ORB_SLAM2::MapPoint *> vpMPs = pKF->GetMapPointMatches();
            for (ORB_SLAM2::MapPoint *pMP : vpMPs) kf_mp.push_back(PointRow(pMP));
            kf_mp_off.push_back((int32_t)kf_mp.size());
            const std::vector<ORB_SLAM2::KeyFrame *> vNeighs = pKF->GetBestCovisibilityKeyFrames(AOS2_LOCAL_MAP_NEIGHBOURS);
            size_t j = 0;
            for (ORB_SLAM2::KeyFrame *pN : vNeighs) {
                const int32_t r = KeyFrameRow(pN);
                if (r >= 0 && j < (size_t)AOS2_LOCAL_MAP_NEIGHBOURS) kf_best[k * AOS2_LOCAL_MAP_NEIGHBOURS + j++] = r;
            }
            const std::set<ORB_SLAM2::KeyFrame *> spChilds = pKF->GetChilds();
            for (ORB_SLAM2::KeyFrame *pC : spChilds) {
                const int32_t r = KeyFrameRow(pC);
                if (r >= 0) kf_child.push_back(r);
            }
            kf_child_off.push_back((int32_t)kf_child.size());
            kf_parent[k] = KeyFrameRow(pKF->GetParent());
            view.KeyFrame(pKF);
        }
        aos2_local_map_graph_t g;
        g.n_points = (int32_t)np; g.point_bad = point_bad.data(); g.point_nobs = point_nobs.data();
        g.obs_off = obs_off.data(); g.obs_kf = obs_kf.data();
        g.n_keyframes = (int32_t)nk; g.kf_bad = kf_bad.data(); g.kf_mp_off = kf_mp_off.data(); g.kf_mp = kf_mp.data();
        g.kf_best = kf_best.data(); g.kf_child_off = kf_child_off.data(); g.kf_child = kf_child.data(); g.kf_parent = kf_parent.data();
        check(aos2_local_map_create(thread_device(), &mHandle), "LocalMapSnapshot");
        check(aos2_local_map_set(mHandle, &g), "LocalMapSnapshot");
        view.Set(mHandle);
    }

public:
    // The map has changed: re-reads ONLY the named objects and sends them as one delta (aos2_local_map_apply).
    //   vpTouchedKFs   keyframes whose GetMapPointMatches() changed;  vpRelinkedKFs  keyframes whose isBad(), best covisibles, children
    //                  or parent changed.  A keyframe the snapshot does not know, in either list, is APPENDED (and read for both):
    //                  its mnId must be larger than that of every known keyframe, rows being ascending mnId.
    //   vpTouchedMPs   points whose isBad(), Observations() or GetObservations() changed (one outside the table is NULL to the snapshot)
    //   vpTable        the point table, equal to the snapshot's over its length and grown at its end; an appended non-NULL point is read,
    //                  an appended NULL is an empty slot
    // A snapshot taken with a view requires one here (its arrays for the delta's rows are gathered through the same hooks).
    template <class View = NoSnapshotView>
    void Apply(const std::vector<ORB_SLAM2::KeyFrame *> &vpTouchedKFs, const std::vector<ORB_SLAM2::KeyFrame *> &vpRelinkedKFs,
               const std::vector<ORB_SLAM2::MapPoint *> &vpTouchedMPs, const std::vector<ORB_SLAM2::MapPoint *> &vpTable, View &&view = View())
    {
        const char *const what = "LocalMapSnapshot::Apply";
        if (mbHasView != std::decay<View>::type::kGathers)
            fail_precondition(what, mbHasView ? "the snapshot was taken with a view and needs one" : "the snapshot was taken without a view");
        if (vpTable.size() < mvpPoints.size() || !std::equal(mvpPoints.begin(), mvpPoints.end(), vpTable.begin()))
            fail_precondition(what, "an existing row of the point table changed its object");
        // appended keyframes, in ascending mnId behind the known ones
        std::vector<ORB_SLAM2::KeyFrame *> vpNew;
        for (const auto *list : {&vpTouchedKFs, &vpRelinkedKFs})
            for (ORB_SLAM2::KeyFrame *pKF : *list)
                if (pKF && KeyFrameRow(pKF) < 0 && std::find(vpNew.begin(), vpNew.end(), pKF) == vpNew.end()) vpNew.push_back(pKF);
        std::sort(vpNew.begin(), vpNew.end(), [](ORB_SLAM2::KeyFrame *a, ORB_SLAM2::KeyFrame *b) { return a->mnId < b->mnId; });
        if (!vpNew.empty() && !mvpKeyFrames.empty() && !(vpNew.front()->mnId > mvpKeyFrames.back()->mnId))
            fail_precondition(what, "a new keyframe has a smaller mnId than a known one (rows are ascending mnId)");
        for (size_t i = 1; i < vpNew.size(); ++i)
            if (vpNew[i]->mnId == vpNew[i - 1]->mnId) fail_precondition(what, "two new keyframes share their mnId");
        const size_t np0 = mvpPoints.size();
        for (ORB_SLAM2::KeyFrame *pKF : vpNew) {
            mKeyFrameRow[pKF] = (int32_t)mvpKeyFrames.size();
            mvpKeyFrames.push_back(pKF);
        }
        for (size_t p = np0; p < vpTable.size(); ++p) {
            mvpPoints.push_back(vpTable[p]);
            if (vpTable[p]) mPointRow[vpTable[p]] = (int32_t)p;
        }
        // the three row sets, ascending
        std::set<int32_t> sMP, sLink, sPoint;
        for (ORB_SLAM2::KeyFrame *pKF : vpTouchedKFs)
            if (pKF) sMP.insert(KeyFrameRow(pKF));
        for (ORB_SLAM2::KeyFrame *pKF : vpRelinkedKFs)
            if (pKF) sLink.insert(KeyFrameRow(pKF));
        for (ORB_SLAM2::KeyFrame *pKF : vpNew) {
            sMP.insert(KeyFrameRow(pKF));
            sLink.insert(KeyFrameRow(pKF));
        }
        for (ORB_SLAM2::MapPoint *pMP : vpTouchedMPs)
            if (pMP && PointRow(pMP) >= 0) sPoint.insert(PointRow(pMP));
        for (size_t p = np0; p < mvpPoints.size(); ++p)
            if (mvpPoints[p]) sPoint.insert((int32_t)p);
        // the delta: the same reads as Build, of the named rows only
        std::vector<int32_t> point_row(sPoint.begin(), sPoint.end()), point_nobs, obs_off(1, 0), obs_kf, kf_mp_row(sMP.begin(), sMP.end()),
            kf_mp_off(1, 0), kf_mp, kf_link_row(sLink.begin(), sLink.end()), kf_best(kf_link_row.size() * AOS2_LOCAL_MAP_NEIGHBOURS, -1),
            kf_child_off(1, 0), kf_child, kf_parent;
        std::vector<uint8_t> point_bad, kf_bad;
        for (int32_t p : point_row) {
            ORB_SLAM2::MapPoint *pMP = mvpPoints[p];
            point_bad.push_back(pMP->isBad() ? 1 : 0);
            point_nobs.push_back(pMP->Observations());
            std::map<int32_t, size_t> rows;
            const std::map<ORB_SLAM2::KeyFrame *, size_t> observations = pMP->GetObservations();
            for (const auto &ob : observations) {
                const int32_t r = KeyFrameRow(ob.first);
                if (r >= 0) rows.insert(std::make_pair(r, ob.second));
            }
            for (const auto &row : rows) {
                obs_kf.push_back(row.first);
                view.DeltaObservation(row.second);
            }
            obs_off.push_back((int32_t)obs_kf.size());
        }
        for (int32_t k : kf_mp_row) {
            const std::vector<ORB_SLAM2::MapPoint *> vpMPs = mvpKeyFrames[k]->GetMapPointMatches();
            for (ORB_SLAM2::MapPoint *pMP : vpMPs) kf_mp.push_back(PointRow(pMP));
            kf_mp_off.push_back((int32_t)kf_mp.size());
            view.DeltaMatches(mvpKeyFrames[k]);
        }
        for (size_t i = 0; i < kf_link_row.size(); ++i) {
            ORB_SLAM2::KeyFrame *pKF = mvpKeyFrames[kf_link_row[i]];
            kf_bad.push_back(pKF->isBad() ? 1 : 0);
            const std::vector<ORB_SLAM2::KeyFrame *> vNeighs = pKF->GetBestCovisibilityKeyFrames(AOS2_LOCAL_MAP_NEIGHBOURS);
            size_t j = 0;
            for (ORB_SLAM2::KeyFrame *pN : vNeighs) {
                const int32_t r = KeyFrameRow(pN);
                if (r >= 0 && j < (size_t)AOS2_LOCAL_MAP_NEIGHBOURS) kf_best[i * AOS2_LOCAL_MAP_NEIGHBOURS + j++] = r;
            }
            const std::set<ORB_SLAM2::KeyFrame *> spChilds = pKF->GetChilds();
            for (ORB_SLAM2::KeyFrame *pC : spChilds) {
                const int32_t r = KeyFrameRow(pC);
                if (r >= 0) kf_child.push_back(r);
            }
            kf_child_off.push_back((int32_t)kf_child.size());
            kf_parent.push_back(KeyFrameRow(pKF->GetParent()));
            view.DeltaLinks(pKF);
        }
        aos2_local_map_delta_t d;
        d.n_points = (int32_t)mvpPoints.size(); d.n_keyframes = (int32_t)mvpKeyFrames.size();
        d.n_point_rows = (int32_t)point_row.size(); d.point_row = point_row.data(); d.point_bad = point_bad.data();
        d.point_nobs = point_nobs.data(); d.obs_off = obs_off.data(); d.obs_kf = obs_kf.data();
        d.n_kf_mp_rows = (int32_t)kf_mp_row.size(); d.kf_mp_row = kf_mp_row.data(); d.kf_mp_off = kf_mp_off.data(); d.kf_mp = kf_mp.data();
        d.n_kf_link_rows = (int32_t)kf_link_row.size(); d.kf_link_row = kf_link_row.data(); d.kf_bad = kf_bad.data();
        d.kf_best = kf_best.data(); d.kf_child_off = kf_child_off.data(); d.kf_child = kf_child.data(); d.kf_parent = kf_parent.data();
        view.PointDelta(d);
        check(aos2_local_map_apply(mHandle, &d), what);
    }

    ~LocalMapSnapshot() { aos2_local_map_destroy(mHandle); }
    LocalMapSnapshot(const LocalMapSnapshot &) = delete;
    LocalMapSnapshot &operator=(const LocalMapSnapshot &) = delete;

    int32_t KeyFrameRow(ORB_SLAM2::KeyFrame *pKF) const
    {
        const auto it = mKeyFrameRow.find(pKF);
        return it == mKeyFrameRow.end() ? -1 : it->second;
    }
    int32_t PointRow(ORB_SLAM2::MapPoint *pMP) const
    {
        const auto it = mPointRow.find(pMP);
        return it == mPointRow.end() ? -1 : it->second;
    }
    const std::vector<ORB_SLAM2::KeyFrame *> &KeyFrames() const { return mvpKeyFrames; }
    const std::vector<ORB_SLAM2::MapPoint *> &Points() const { return mvpPoints; }
    aos2_local_map_t *Handle() const { return mHandle; }

private:
    std::vector<ORB_SLAM2::KeyFrame *> mvpKeyFrames;
    std::vector<ORB_SLAM2::MapPoint *> mvpPoints;
    std::unordered_map<ORB_SLAM2::KeyFrame *, int32_t> mKeyFrameRow;
    std::unordered_map<ORB_SLAM2::MapPoint *, int32_t> mPointRow;
    aos2_local_map_t *mHandle = nullptr;
    bool mbHasView = false;
};

// UpdateLocalKeyFrames + UpdateLocalPoints of one frame.  F.mvpMapPoints: a feature whose point isBad() loses it (:1428).
// vpLocalKeyFrames / pReferenceKF: in / out, untouched when no feature votes (:1433); vpLocalMapPoints: out.
inline void UpdateLocalMap(ORB_SLAM2::Frame &F, const LocalMapSnapshot &S, std::vector<ORB_SLAM2::KeyFrame *> &vpLocalKeyFrames,
                           std::vector<ORB_SLAM2::MapPoint *> &vpLocalMapPoints, ORB_SLAM2::KeyFrame *&pReferenceKF)
{
    ShimClock clk;
    const int N = F.N;
    const int cap = std::max(N, 1);
    std::vector<int32_t> mp(cap, -1);
    for (int i = 0; i < N; ++i) mp[i] = S.PointRow(F.mvpMapPoints[i]);
    const std::vector<int32_t> held = mp;
    const int kf_cap = (int)std::max<size_t>(std::max(S.KeyFrames().size(), vpLocalKeyFrames.size()), 1);
    const int local_cap = (int)std::max<size_t>(S.Points().size(), 1);
    std::vector<int32_t> kfs(kf_cap, -1), local(local_cap, -1);
    for (size_t j = 0; j < vpLocalKeyFrames.size(); ++j) kfs[j] = S.KeyFrameRow(vpLocalKeyFrames[j]);
    const std::vector<int32_t> kfs_in = kfs;
    int32_t n = N, n_local = 0, n_kfs = (int32_t)vpLocalKeyFrames.size(), ref = S.KeyFrameRow(pReferenceKF);
    last_shim_timing().gather_us = clk.lap();
    check(aos2_local_map_update(S.Handle(), 1, cap, &n, mp.data(), local.data(), local_cap, &n_local, kfs.data(), kf_cap, &n_kfs, &ref),
          "UpdateLocalMap");
    last_shim_timing().call_us = clk.lap();
    for (int i = 0; i < N; ++i)
        if (held[i] >= 0 && mp[i] < 0) F.mvpMapPoints[i] = static_cast<ORB_SLAM2::MapPoint *>(NULL);
    // (no votes: the call leaves the rows as they were passed, and the caller's list -- with any keyframe the snapshot does not know --
    // stands; a list the votes rebuilt has no -1 below its count, so equal rows mean an equal list)
    if (!(kfs == kfs_in && n_kfs == (int32_t)vpLocalKeyFrames.size())) {
        vpLocalKeyFrames.clear();
        for (int j = 0; j < n_kfs; ++j) vpLocalKeyFrames.push_back(S.KeyFrames()[kfs[j]]);
    }
    if (ref >= 0) pReferenceKF = S.KeyFrames()[ref];
    vpLocalMapPoints.clear();
    for (int j = 0; j < n_local; ++j) vpLocalMapPoints.push_back(S.Points()[local[j]]);
    last_shim_timing().scatter_us = clk.lap();
}

}  // namespace aos2
