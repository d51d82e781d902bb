"""LocalMapping::KeyFrameCulling (src/LocalMapping.cc:636-700) restated in plain Python over the arrays of aos2_local_map_graph_t
and aos2_kf_culling_view_t: the map as objects with dicts and lists, the loop statement by statement with the reference's line
numbers, KeyFrame::SetBadFlag (src/KeyFrame.cc:514-532) and MapPoint::EraseObservation (src/MapPoint.cc:144-170) taking effect
at once as they do there.  Shares nothing with the library.  Float compares are made in float32, as the reference's are."""
import numpy as np

KEPT, CULLED, DEFERRED, SKIPPED = 0, 1, 2, 3


class _MapPoint:
    def __init__(self, row, bad, nobs):
        self.row, self.mbBad, self.nObs = row, bool(bad), int(nobs)
        self.mObservations = {}   # keyframe row -> feature index (map<KeyFrame*, size_t>)


class _KeyFrame:
    def __init__(self, row):
        self.row = row
        self.mvpMapPoints, self.octave, self.mvDepth, self.stereo = [], [], [], []
        self.mThDepth, self.first, self.mbNotErase, self.mbToBeErased, self.mbBad = np.float32(0), False, False, False, False


def build(g, v):
    """the arrays -> (points, keyframes)"""
    pts = [_MapPoint(p, g["point_bad"][p], g["point_nobs"][p]) for p in range(g["n_points"])]
    kfs = [_KeyFrame(k) for k in range(g["n_keyframes"])]
    for p, mp in enumerate(pts):
        for e in range(g["obs_off"][p], g["obs_off"][p + 1]):
            mp.mObservations[int(g["obs_kf"][e])] = int(v["obs_idx"][e])
    for k, kf in enumerate(kfs):
        for f in range(g["kf_mp_off"][k], g["kf_mp_off"][k + 1]):
            r = int(g["kf_mp"][f])
            kf.mvpMapPoints.append(pts[r] if r >= 0 else None)
            kf.octave.append(int(v["kf_octave"][f]))
            kf.mvDepth.append(np.float32(v["kf_depth"][f]))
            kf.stereo.append(bool(v["kf_stereo"][f]))   # mvuRight[i] >= 0
        kf.mThDepth = np.float32(v["kf_th_depth"][k])
        kf.first = bool(v["kf_flags"][k] & 1)           # mnId == 0
        kf.mbNotErase = bool(v["kf_flags"][k] & 2)
    return pts, kfs


def _count(pKF, kfs, monocular):
    """:649-695 -> nMPs, nRedundantObservations"""
    thObs = 3                                                           # :651-652
    nRedundantObservations, nMPs = 0, 0                                 # :653-654
    for i, pMP in enumerate(pKF.mvpMapPoints):                          # :655
        if pMP is None:                                                 # :658
            continue
        if pMP.mbBad:                                                   # :660
            continue
        if not monocular:                                               # :662
            if pKF.mvDepth[i] > pKF.mThDepth or pKF.mvDepth[i] < np.float32(0):   # :664
                continue
        nMPs += 1                                                       # :668
        if pMP.nObs > thObs:                                            # :669  Observations()
            scaleLevel = pKF.octave[i]                                  # :671
            nObs = 0                                                    # :673
            for pKFi, idx in pMP.mObservations.items():                 # :674 (any order: the count stops at 3)
                if pKFi == pKF.row:                                     # :677
                    continue
                scaleLeveli = kfs[pKFi].octave[idx]                     # :679
                if scaleLeveli <= scaleLevel + 1:                       # :681
                    nObs += 1
                    if nObs >= thObs:                                   # :684
                        break
            if nObs >= thObs:                                           # :688
                nRedundantObservations += 1
    return nMPs, nRedundantObservations


def _erase_observation(pMP, pKF, went_bad):
    """MapPoint::EraseObservation, src/MapPoint.cc:144-170"""
    if pKF.row in pMP.mObservations:                                    # :149
        idx = pMP.mObservations[pKF.row]                                # :151
        pMP.nObs -= 2 if pKF.stereo[idx] else 1                         # :152-155
        del pMP.mObservations[pKF.row]                                  # :157
        if pMP.nObs <= 2 and not pMP.mbBad:                             # :163-169  SetBadFlag: the point is bad from here on
            pMP.mbBad = True
            went_bad.append(pMP.row)


def _set_bad_flag(pKF, went_bad):
    """KeyFrame::SetBadFlag, src/KeyFrame.cc:514-532 -> whether the keyframe was erased"""
    if pKF.first:                                                       # :518
        return False
    if pKF.mbNotErase:                                                  # :520-524
        pKF.mbToBeErased = True
        return False
    for pMP in pKF.mvpMapPoints:                                        # :530-532
        if pMP is not None:
            _erase_observation(pMP, pKF, went_bad)
    pKF.mbBad = True
    return True


def keyframe_culling(g, v, monocular, cand):
    """-> dict(status uint8 [n], n_mps, n_redundant int32 [n], bad_points = the rows that went bad, ascending, n_bad_points,
    alone uint8 [n] = the status every candidate would get with no erasure applied, n_culled)"""
    pts, kfs = build(g, v)
    n = len(cand)
    alone = np.zeros(n, np.uint8)
    for j, c in enumerate(cand):   # the map as it stands, nothing applied
        pKF = kfs[int(c)]
        if pKF.first:
            alone[j] = SKIPPED
            continue
        nMPs, nRed = _count(pKF, kfs, monocular)
        alone[j] = (DEFERRED if pKF.mbNotErase else CULLED) if nRed > 0.9 * nMPs else KEPT
    status, n_mps, n_red = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
    went_bad = []
    for j, c in enumerate(cand):                                        # :644
        pKF = kfs[int(c)]
        if pKF.first:                                                   # :647
            status[j] = SKIPPED
            continue
        nMPs, nRedundantObservations = _count(pKF, kfs, monocular)
        n_mps[j], n_red[j] = nMPs, nRedundantObservations
        if nRedundantObservations > 0.9 * nMPs:                         # :697  int against double
            status[j] = CULLED if _set_bad_flag(pKF, went_bad) else DEFERRED   # :698
    return dict(status=status, n_mps=n_mps, n_redundant=n_red, bad_points=np.array(sorted(went_bad), np.int32),
                n_bad_points=len(went_bad), alone=alone, n_culled=int((status == CULLED).sum()))
