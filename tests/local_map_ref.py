"""Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) and the statistics loop of Tracking::TrackLocalMap (:1040-1071), restated
line by line from the reference on small Python objects: KeyFrame and MapPoint instances with the members those lines touch,
held in dicts and sets that are walked in ascending keyframe row where the reference walks map<KeyFrame*, ...> / set<KeyFrame*>
in pointer order.  Independent of the library's C++: it shares only the layout of the graph dict
(the fields of aos2_local_map_graph_t).  Integers only."""
import numpy as np


class MapPoint:
    def __init__(self, row, bad, nobs, observations):
        self.row, self.bad, self.nObs = row, bool(bad), int(nobs)
        self.mObservations = observations          # keyframe rows (the keys of map<KeyFrame*, size_t>)
        self.mnTrackReferenceForFrame = -1
        self.found = 0

    def isBad(self):
        return self.bad

    def Observations(self):
        return self.nObs

    def GetObservations(self):
        return sorted(self.mObservations)          # map iteration: ascending key

    def IncreaseFound(self):
        self.found += 1


class KeyFrame:
    def __init__(self, row, bad):
        self.row, self.bad = row, bool(bad)
        self.mvpMapPoints, self.best, self.mspChildrens, self.mpParent = [], [], set(), None
        self.mnTrackReferenceForFrame = -1

    def isBad(self):
        return self.bad


class Map:
    """the objects of a graph dict"""

    def __init__(self, g):
        npnt, nk = int(g["n_points"]), int(g["n_keyframes"])
        oo, ok = np.asarray(g["obs_off"]), np.asarray(g["obs_kf"])
        self.points = [MapPoint(p, g["point_bad"][p], g["point_nobs"][p], [int(k) for k in ok[oo[p]:oo[p + 1]]]) for p in range(npnt)]
        self.kfs = [KeyFrame(k, g["kf_bad"][k]) for k in range(nk)]
        mo, mm = np.asarray(g["kf_mp_off"]), np.asarray(g["kf_mp"])
        co, cc = np.asarray(g["kf_child_off"]), np.asarray(g["kf_child"])
        best = np.asarray(g["kf_best"]).reshape(nk, 10) if nk else np.zeros((0, 10), np.int32)
        for k, kf in enumerate(self.kfs):
            kf.mvpMapPoints = [self.points[r] if r >= 0 else None for r in mm[mo[k]:mo[k + 1]]]
            kf.best = [self.kfs[r] for r in best[k] if r >= 0]                 # GetBestCovisibilityKeyFrames(10)
            kf.mspChildrens = {int(r) for r in cc[co[k]:co[k + 1]]}
            kf.mpParent = self.kfs[g["kf_parent"][k]] if g["kf_parent"][k] >= 0 else None


def update_local_map(m: Map, frame_id, mvpMapPoints, mvpLocalKeyFrames, mpReferenceKF):
    """UpdateLocalKeyFrames + UpdateLocalPoints of one frame.  mvpMapPoints: list of MapPoint | None, changed in place;
    mvpLocalKeyFrames: the previous list (KeyFrame objects).  -> (mvpLocalKeyFrames, mvpLocalMapPoints, mpReferenceKF, voted)"""
    # --- UpdateLocalKeyFrames :1411-1519
    keyframeCounter = {}
    for i in range(len(mvpMapPoints)):                                  # :1415
        if mvpMapPoints[i] is not None:
            pMP = mvpMapPoints[i]
            if not pMP.isBad():
                for kf_row in pMP.GetObservations():                    # :1423
                    keyframeCounter[kf_row] = keyframeCounter.get(kf_row, 0) + 1
            else:
                mvpMapPoints[i] = None                                  # :1428
    voted = len(keyframeCounter) > 0
    if voted:                                                           # :1433 (otherwise: return)
        mx, pKFmax = 0, None
        mvpLocalKeyFrames = []                                          # :1439
        for kf_row in sorted(keyframeCounter):                          # :1443
            pKF = m.kfs[kf_row]
            if pKF.isBad():
                continue
            if keyframeCounter[kf_row] > mx:
                mx, pKFmax = keyframeCounter[kf_row], pKF
            mvpLocalKeyFrames.append(pKF)
            pKF.mnTrackReferenceForFrame = frame_id
        for pKF in list(mvpLocalKeyFrames):                             # :1462 (itEndKF is fixed before the loop)
            if len(mvpLocalKeyFrames) > 80:                             # :1465
                break
            for pNeighKF in pKF.best:                                   # :1472
                if not pNeighKF.isBad():
                    if pNeighKF.mnTrackReferenceForFrame != frame_id:
                        mvpLocalKeyFrames.append(pNeighKF)
                        pNeighKF.mnTrackReferenceForFrame = frame_id
                        break
            for child_row in sorted(pKF.mspChildrens):                  # :1487
                pChildKF = m.kfs[child_row]
                if not pChildKF.isBad():
                    if pChildKF.mnTrackReferenceForFrame != frame_id:
                        mvpLocalKeyFrames.append(pChildKF)
                        pChildKF.mnTrackReferenceForFrame = frame_id
                        break
            pParent = pKF.mpParent                                      # :1501
            if pParent is not None:
                if pParent.mnTrackReferenceForFrame != frame_id:
                    mvpLocalKeyFrames.append(pParent)
                    pParent.mnTrackReferenceForFrame = frame_id
                    break
        if pKFmax is not None:                                          # :1514
            mpReferenceKF = pKFmax
    # --- UpdateLocalPoints :1385-1408
    mvpLocalMapPoints = []
    for pKF in mvpLocalKeyFrames:
        for pMP in pKF.mvpMapPoints:
            if pMP is None:
                continue
            if pMP.mnTrackReferenceForFrame == frame_id:
                continue
            if not pMP.isBad():
                mvpLocalMapPoints.append(pMP)
                pMP.mnTrackReferenceForFrame = frame_id
    return mvpLocalKeyFrames, mvpLocalMapPoints, mpReferenceKF, voted


def update_batch(g, n, mp, local_cap, kf_cap, local_kfs=None, n_local_kfs=None, ref_kf=None):
    """The arrays aos2_frames_update_local_map leaves: n [B], mp [B][cap]; the previous lists default to empty, ref_kf to -1.
    -> dict(mp, local, n_local, local_kfs, n_local_kfs, ref_kf, voted [B], full_kfs: the whole keyframe list of every frame)"""
    m = Map(g)
    mp = np.array(mp, np.int32, ndmin=2)
    B, cap = mp.shape
    n = np.asarray(n).reshape(B)
    lk = np.full((B, kf_cap), -1, np.int32) if local_kfs is None else np.array(local_kfs, np.int32).reshape(B, kf_cap)
    nlk = np.zeros(B, np.int32) if n_local_kfs is None else np.array(n_local_kfs, np.int32).reshape(B)
    ref = np.full(B, -1, np.int32) if ref_kf is None else np.array(ref_kf, np.int32).reshape(B)
    local, n_local = np.full((B, local_cap), -1, np.int32), np.zeros(B, np.int32)
    voted, full = np.zeros(B, bool), []
    for b in range(B):
        N = int(n[b])
        frame = [m.points[r] if 0 <= r < len(m.points) else None for r in mp[b, :N]]
        held = [r for r in mp[b, :N]]
        prev = [m.kfs[r] for r in lk[b, :max(0, min(int(nlk[b]), kf_cap))] if 0 <= r < len(m.kfs)]
        refobj = m.kfs[ref[b]] if 0 <= ref[b] < len(m.kfs) else None
        kfs, pts, refobj2, v = update_local_map(m, b + 1, frame, prev, refobj)
        for i in range(N):
            if frame[i] is None and 0 <= held[i] < len(m.points):
                mp[b, i] = -1
        voted[b] = v
        full.append([k.row for k in kfs])
        if v:
            rows = [k.row for k in kfs]
            lk[b] = -1
            lk[b, :min(len(rows), kf_cap)] = rows[:kf_cap]
            nlk[b] = len(rows)
            if refobj2 is not None:
                ref[b] = refobj2.row
        rows = [p.row for p in pts]
        local[b, :min(len(rows), local_cap)] = rows[:local_cap]
        n_local[b] = len(rows)
    return dict(mp=mp, local=local, n_local=n_local, local_kfs=lk, n_local_kfs=nlk, ref_kf=ref, voted=voted, full_kfs=full)


def stats_batch(g, n, mp, outlier, stereo, only_tracking):
    """:1040-1071 -> dict(stats [B][3] = nObsvMappoints, mnMatchesInliers, totalObservation; mp; found_inc [n_points])"""
    m = Map(g)
    mp = np.array(mp, np.int32, ndmin=2)
    B, cap = mp.shape
    n = np.asarray(n).reshape(B)
    outlier = np.asarray(outlier).reshape(B, cap)
    stats = np.zeros((B, 3), np.int32)
    for b in range(B):
        mnMatchesInliers = nObsvMappoints = totalObservation = 0
        for i in range(int(n[b])):
            pMP = m.points[mp[b, i]] if 0 <= mp[b, i] < len(m.points) else None
            if pMP is not None:
                nObsvMappoints += 1
                if not outlier[b, i]:
                    pMP.IncreaseFound()
                    if not only_tracking:
                        if pMP.Observations() > 0:
                            mnMatchesInliers += 1
                        totalObservation += pMP.Observations()
                    else:
                        mnMatchesInliers += 1
                elif stereo:
                    mp[b, i] = -1
        stats[b] = nObsvMappoints, mnMatchesInliers, totalObservation
    return dict(stats=stats, mp=mp, found_inc=np.array([p.found for p in m.points], np.int32).reshape(-1))
