"""The planner's camera and state checks for batches (include/aos2.h: aos2_vis_*, aos2_svc_*, their host taps, aos2_debug_tw_math)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import AOS2_ERR_CAPACITY, VIS_CAMERAS, SvcParams, VisCamera, _SvcMotionsOut
from ._core import _Handle, AosError, _check, _p, lib


class Visibility(_Handle):
    """camera (include/camera.h:51-129) for batches of states: the planner's map resident on the device, countVisible for ns
    states in one call, MotionCostCamera for many motions and AdvanceStepCamera for a trajectory.  host=True runs the library's
    own serial routine (aos2_debug_visibility_*host) instead."""
    CAMERA_MAP, CAMERA_PLAIN = VIS_CAMERAS

    KIND = "vis"

    def __init__(self, device=0):
        self._create(device)

    @staticmethod
    def camera_default(which=0):
        cam = VisCamera()
        _check(lib().aos2_vis_camera_default(which, C.byref(cam)))
        return cam

    @staticmethod
    def gate_tile():
        """(points a workgroup of the gate kernel takes, states of its tile)"""
        p, s = C.c_int(0), C.c_int(0)
        lib().aos2_vis_gate_tile(C.byref(p), C.byref(s))
        return p.value, s.value

    def set_camera(self, cam: VisCamera):
        _check(self.L.aos2_vis_set_camera(self.h, C.byref(cam)))

    def set_map(self, xyz, upper, lower, max_range, min_range, found_ratio):
        xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
        rest = [np.ascontiguousarray(a, np.float32).reshape(-1) for a in (upper, lower, max_range, min_range, found_ratio)]
        if any(len(a) != len(xyz) for a in rest):
            raise ValueError("the map's arrays differ in length")
        _check(self.L.aos2_vis_set_map(self.h, len(xyz), _p(xyz), *[_p(a) for a in rest]))

    def map_size(self):
        return self.L.aos2_vis_map_size(self.h)

    def last_device_ms(self):
        return float(self.L.aos2_vis_last_device_ms(self.h))

    def _count(self, f, arr, ns, want_sum, want_mask):
        words = (self.map_size() + 63) // 64
        count = np.zeros(ns, np.int32)
        s = np.zeros(ns, np.float32) if want_sum else None
        m = np.zeros((ns, words), np.uint64) if want_mask else None
        _check(f(self.h, ns, _p(arr), _p(count), _p(s) if want_sum else None, _p(m) if want_mask else None))
        return dict(count=count, sum=s, mask=m)

    def count(self, states, sum=True, mask=True, host=False):
        """aos2_vis_count: states [ns][3] = x, y, theta -> dict(count int32 [ns], sum float32 [ns] | None, mask uint64 [ns][words] | None)"""
        st = np.ascontiguousarray(states, np.float32).reshape(-1, 3)
        return self._count(self.L.aos2_debug_visibility_host if host else self.L.aos2_vis_count, st, len(st), sum, mask)

    def count_poses(self, T_wb, sum=True, mask=True, host=False):
        """aos2_vis_count_poses: T_wb [ns][4][4]"""
        T = np.ascontiguousarray(T_wb, np.float32).reshape(-1, 16)
        return self._count(self.L.aos2_debug_visibility_poses_host if host else self.L.aos2_vis_count_poses, T, len(T), sum, mask)

    def motion_costs(self, motions, thres=-1, host=False):
        """aos2_vis_motion_costs: motions = a list of [size][3] state arrays -> float64 [nm]"""
        ms = [np.asarray(m, np.float32).reshape(-1, 3) for m in motions]
        off = np.cumsum([0] + [len(m) for m in ms]).astype(np.int32)
        st = np.ascontiguousarray(np.concatenate(ms) if ms else np.zeros((0, 3)), np.float32)
        return self.motion_costs_raw(off, st, thres, host)

    def motion_costs_raw(self, offsets, states, thres=-1, host=False):
        off, st = np.ascontiguousarray(offsets, np.int32), np.ascontiguousarray(states, np.float32)
        cost = np.zeros(max(len(off) - 1, 0), np.float64)
        f = self.L.aos2_debug_visibility_motion_costs_host if host else self.L.aos2_vis_motion_costs
        _check(f(self.h, len(off) - 1, _p(off), _p(st), int(thres), _p(cost)))
        return cost

    def advance(self, states, thres=-1, host=False):
        """aos2_vis_advance: the last index of the leading run of states with count > thres, -1 if the first one fails"""
        st = np.ascontiguousarray(states, np.float32).reshape(-1, 3)
        idx = C.c_int32(-2)
        f = self.L.aos2_debug_visibility_advance_host if host else self.L.aos2_vis_advance
        _check(f(self.h, len(st), _p(st), int(thres), C.byref(idx)))
        return idx.value


class _OwnedVisibility(Visibility):
    """the visibility handle a StateValidChecker owns: it dies with its owner"""

    def __init__(self, owner, h):
        self.L, self.h, self.owner = lib(), C.c_void_p(h), owner

    def close(self):
        self.h = None


class StateValidChecker(_Handle):
    """StateValidChecker (include/StateValidChecker.h:47-150) for batches: the obstacles and the camera's map resident on the
    device, isValid for ns states and checkMotionTW / reconstructMotionTW / MotionCost for nm pairs of states in one call.
    host=True runs the library's own serial routine (aos2_debug_svc_*host) instead.  `vis` is the camera base: set_camera and
    set_map go there."""
    MOTION_FIELDS = (("path_valid", np.uint8, 1), ("type", np.int32, 1), ("t", np.float64, 3), ("m", np.int32, 3), ("n_states", np.int32, 1),
                     ("valid", np.uint8, 1), ("first_invalid", np.int32, 1), ("cost_length", np.float64, 1), ("cost_camera", np.float64, 1))

    KIND = "svc"

    def __init__(self, device=0):
        self._create(device)
        self.vis = _OwnedVisibility(self, self.L.aos2_svc_vis(self.h))

    def close(self):
        if getattr(self, "h", None):
            self.vis.close()
        _Handle.close(self)

    @staticmethod
    def params_default():
        p = SvcParams()
        _check(lib().aos2_svc_params_default(C.byref(p)))
        return p

    @staticmethod
    def collide_tile():
        """(obstacles a workgroup of the collision kernel stages at a time, states of its tile)"""
        o, s = C.c_int(0), C.c_int(0)
        lib().aos2_svc_collide_tile(C.byref(o), C.byref(s))
        return o.value, s.value

    def set_params(self, p: SvcParams):
        _check(self.L.aos2_svc_set_params(self.h, C.byref(p)))

    def set_obstacles(self, xy, obs_r=0.1):
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        _check(self.L.aos2_svc_set_obstacles(self.h, len(xy), _p(xy), float(obs_r)))

    def last_device_ms(self):
        return float(self.L.aos2_svc_last_device_ms(self.h))

    def valid(self, states, host=False):
        """aos2_svc_valid: states [ns][3] float64 -> dict(valid uint8 [ns], collision_free uint8 [ns], count int32 [ns])"""
        st = np.ascontiguousarray(states, np.float64).reshape(-1, 3)
        out = dict(valid=np.zeros(len(st), np.uint8), collision_free=np.zeros(len(st), np.uint8), count=np.zeros(len(st), np.int32))
        f = self.L.aos2_debug_svc_valid_host if host else self.L.aos2_svc_valid
        _check(f(self.h, len(st), _p(st), _p(out["valid"]), _p(out["collision_free"]), _p(out["count"])))
        return out

    def motions(self, q1, q2, states=True, capacity=None, host=False):
        """aos2_svc_motions: q1, q2 [nm][3] float64 -> a dict of the per-motion arrays (MOTION_FIELDS) and, with states, offsets
        int32 [nm + 1] and states float64 [total][3].  capacity: the rows of the states buffer (default: asked for with a first
        call).  A buffer too small raises AosError(AOS2_ERR_CAPACITY) with .needed = the rows needed."""
        a = np.ascontiguousarray(q1, np.float64).reshape(-1, 3)
        b = np.ascontiguousarray(q2, np.float64).reshape(-1, 3)
        if len(a) != len(b):
            raise ValueError("q1 and q2 differ in length")
        nm = len(a)
        f = self.L.aos2_debug_svc_motions_host if host else self.L.aos2_svc_motions
        out = {k: np.zeros((nm, w) if w > 1 else nm, dt) for k, dt, w in self.MOTION_FIELDS}
        O = _SvcMotionsOut()
        for k in out:
            setattr(O, k, out[k].ctypes.data)
        if states:
            if capacity is None:      # the size first: a call that asks for no states reports the rows needed
                probe = _SvcMotionsOut()
                _check(f(self.h, nm, _p(a), _p(b), C.byref(probe)))
                capacity = probe.states_needed
            out["offsets"] = np.zeros(nm + 1, np.int32)
            buf = np.zeros((max(int(capacity), 1), 3), np.float64)
            O.offsets, O.states, O.states_capacity = out["offsets"].ctypes.data, buf.ctypes.data, int(capacity)
        st = f(self.h, nm, _p(a), _p(b), C.byref(O))
        if st == AOS2_ERR_CAPACITY:
            e = AosError(st, lib().aos2_last_error().decode(errors="replace"))
            e.needed = int(O.states_needed)
            raise e
        _check(st)
        if states:
            out["states"] = buf[: int(O.states_needed)]
        return out


def debug_tw_math(x, y, device=-1):
    """aos2_debug_tw_math: tw_sin(x), tw_cos(x), tw_atan2(y, x), sqrt(x), y / x of csrc/motion_tw.h on the host (device -1) or in a
    kernel -> dict of float64 arrays"""
    x, y = np.ascontiguousarray(x, np.float64).reshape(-1), np.ascontiguousarray(y, np.float64).reshape(-1)
    if len(x) != len(y):
        raise ValueError("x and y differ in length")
    out = {k: np.zeros(len(x), np.float64) for k in ("sin", "cos", "atan2", "sqrt", "quot")}
    _check(lib().aos2_debug_tw_math(int(device), len(x), _p(x), _p(y), *[_p(out[k]) for k in ("sin", "cos", "atan2", "sqrt", "quot")]))
    return out
