"""Device-resident frame batches (include/aos2.h: aos2_frames_*).  Device arrays are passed as raw pointers (torch tensors'
data_ptr()); the wrapper owns nothing but the handle."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import FRAMES_MEMBERS, _FramesTriang, _MapPointsDev
from ._core import _Handle, _check, _p, lib


def map_points_dev(n, pos, desc, has_obs, normal=0, min_dist=0, max_dist=0):
    """aos2_map_points_dev_t from device pointers (ints)"""
    t = _MapPointsDev()
    t.n, t.pos, t.desc, t.has_obs, t.normal, t.min_dist, t.max_dist = int(n), pos, desc, has_obs, normal or None, min_dist or None, max_dist or None
    return t


def frame_image_bounds(w, h, fx, fy, cx, cy, dist):
    """Frame::ComputeImageBounds (src/Frame.cc:463-493) -> (mnMinX, mnMaxX, mnMinY, mnMaxY)"""
    d = np.zeros(5, np.float32)
    d[: len(dist)] = np.asarray(dist, np.float32)
    out = np.zeros(4, np.float32)
    _check(lib().aos2_frame_image_bounds(int(w), int(h), float(fx), float(fy), float(cx), float(cy), _p(d), _p(out)))
    return out


class Frames(_Handle):
    MAP_POINTS, OUTLIER, TCW, U_RIGHT, DEPTH, GRID_OFF, GRID_IDX, KEYS_UN_X, KEYS_UN_Y, KEYS_ANGLE, KEYS_OCTAVE = FRAMES_MEMBERS

    KIND = "frames"

    def __init__(self, batch, cap, device=0):
        self._create(device, batch, cap)
        self.batch, self.cap = batch, cap

    def build(self, extractor, d_kps, d_desc, d_n, w, h, d_depth, fx, fy, cx, cy, mbf, depth_stride=None, depth_image_stride=None):
        _check(self.L.aos2_frames_build(self.h, extractor.h, self.batch, d_kps, d_desc, d_n, self.cap, w, h, d_depth or None,
                                        depth_stride or w, depth_image_stride or w * h, fx, fy, cx, cy, mbf))

    def build_stereo(self, extractor_left, d_kps, d_desc, d_n, w, h, d_u_right, d_depth_kp, fx, fy, cx, cy, mbf):
        """Frame::Frame(imLeft, imRight, ...) after ExtractORB x 2 + ComputeStereoMatches (src/Frame.cc:57-113)"""
        _check(self.L.aos2_frames_build_stereo(self.h, extractor_left.h, self.batch, d_kps, d_desc, d_n, self.cap, w, h, d_u_right, d_depth_kp,
                                               fx, fy, cx, cy, mbf))

    def set_pose(self, d_Tcw):
        _check(self.L.aos2_frames_set_pose(self.h, d_Tcw))

    def set_distortion(self, dist):
        """mDistCoef = k1 k2 p1 p2 k3 for the following build() calls"""
        d = list(dist) + [0.0] * (5 - len(dist))
        _check(self.L.aos2_frames_set_distortion(self.h, *[float(v) for v in d[:5]]))

    def set_map_points(self, mp, table, outlier=None):
        mp = np.ascontiguousarray(mp, np.int32).reshape(self.batch, self.cap)
        if outlier is not None:
            outlier = np.ascontiguousarray(outlier, np.uint8).reshape(self.batch, self.cap)
        _check(self.L.aos2_frames_set_map_points(self.h, _p(mp), None if outlier is None else _p(outlier), C.byref(table)))

    def get(self, what):
        B, cap = self.batch, self.cap
        shape, dt = {0: ((B, cap), np.int32), 1: ((B, cap), np.uint8), 2: ((B, 16), np.float32), 3: ((B, cap), np.float32),
                     4: ((B, cap), np.float32), 5: ((B, 64 * 48 + 1), np.int32), 6: ((B, cap), np.int32), 7: ((B, cap), np.float32),
                     8: ((B, cap), np.float32)}.get(what, ((B, cap), np.int32))   # (any other id: the library refuses it, whatever the size)
        a = np.zeros(shape, dt)
        _check(self.L.aos2_frames_get(self.h, what, _p(a), a.nbytes))
        return a

    def SearchByProjectionLast(self, last, table, th, mono=False, check_orientation=True, d_nmatches=0):
        _check(self.L.aos2_frames_search_by_projection_last(self.h, last.h, C.byref(table), th, int(mono), int(check_orientation),
                                                            d_nmatches or None))

    def PoseOptimization(self, table, d_inliers=0):
        _check(self.L.aos2_frames_pose_optimization(self.h, C.byref(table), d_inliers or None))

    def discard_outliers(self):
        _check(self.L.aos2_frames_discard_outliers(self.h))

    def SearchLocalPoints(self, table, d_local, n_local, th, nnratio, d_nmatches=0):
        _check(self.L.aos2_frames_search_local_points(self.h, C.byref(table), d_local, n_local, th, nnratio, d_nmatches or None))

    def set_async_keyframe_calls(self, on=True):
        """SearchForTriangulation / Fuse of this handle return after enqueueing (include/aos2.h); wait() completes them"""
        _check(self.L.aos2_frames_set_async_keyframe_calls(self.h, 1 if on else 0))

    def wait(self):
        _check(self.L.aos2_frames_wait(self.h))

    def stream(self):
        return self.L.aos2_frames_stream(self.h)

    def device_ptr(self, what):
        """device address (int) of a member array [batch][cap]"""
        return self.L.aos2_frames_device_ptr(self.h, int(what)) or 0

    def SearchForTriangulation(self, other, kf1, kf2, F12, epipole, d_node_of1, fv1, fv2, d_match12, d_nmatches,
                               only_stereo=False, check_orientation=True):
        """aos2_frames_search_for_triangulation: pairs (frame kf1[p] of this batch, frame kf2[p] of `other`); kf1 / kf2 int32 [n], F12 float32
        [n][9], epipole float32 [n][2]: host arrays; d_node_of1 and fv1 / fv2 = (fv_node, fv_off, fv_idx, n_fv): device addresses (ints);
        results in d_match12 [n][cap], d_nmatches [n]"""
        kf1, kf2 = np.ascontiguousarray(kf1, np.int32), np.ascontiguousarray(kf2, np.int32)
        F12, epipole = np.ascontiguousarray(F12, np.float32), np.ascontiguousarray(epipole, np.float32)
        q = _FramesTriang()
        q.n_pairs = len(kf1)
        q.kf1, q.kf2, q.F12, q.epipole = kf1.ctypes.data, kf2.ctypes.data, F12.ctypes.data, epipole.ctypes.data
        q.d_node_of1 = int(d_node_of1)
        q.d_fv_node1, q.d_fv_off1, q.d_fv_idx1, q.d_n_fv1 = (int(x) for x in fv1)
        q.d_fv_node2, q.d_fv_off2, q.d_fv_idx2, q.d_n_fv2 = (int(x) for x in fv2)
        _check(self.L.aos2_frames_search_for_triangulation(self.h, other.h, C.byref(q), int(only_stereo), int(check_orientation), d_match12, d_nmatches))

    def Fuse(self, table, target, d_rows, n_pts, th, d_best_idx, d_best_dist):
        """aos2_frames_fuse: target int32 [n] host (frames of this batch), d_rows device [n][n_pts] table rows (-1 = rejected by the loop head)"""
        target = np.ascontiguousarray(target, np.int32)
        _check(self.L.aos2_frames_fuse(self.h, C.byref(table), len(target), int(n_pts), target.ctypes.data, d_rows, float(th), d_best_idx, d_best_dist))

    def TriangulateMatches(self, other, kf1, kf2, d_match12, d_x3D, d_status, d_nnew, first_wins=True):
        """aos2_frames_triangulate_matches: the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) for the pairs
        (frame kf1[p] of this batch, frame kf2[p] of `other`) and the d_match12 [n][cap] SearchForTriangulation wrote for them; results in
        d_x3D float32 [n][cap][3], d_status uint8 [n][cap] (capi.TRI_*), d_nnew int32 [n]: device addresses (ints)"""
        kf1, kf2 = np.ascontiguousarray(kf1, np.int32), np.ascontiguousarray(kf2, np.int32)
        _check(self.L.aos2_frames_triangulate_matches(self.h, other.h, len(kf1), kf1.ctypes.data, kf2.ctypes.data, d_match12, int(bool(first_wins)),
                                                      d_x3D, d_status, d_nnew))

    def wait_for_stream(self, hip_stream=None):
        """device-side ordering: what is enqueued on the batch from now on runs behind the work on `hip_stream` so far"""
        _check(self.L.aos2_frames_wait_for_stream(self.h, hip_stream))
