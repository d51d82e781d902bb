"""The resident covisibility graph: Tracking::UpdateLocalMap, KeyFrameCulling, UpdateConnections, UpdateNormalAndDepth and the
application of one keyframe's changes (include/aos2.h: aos2_local_map_*, aos2_frames_update_local_map and their host taps)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (AOS2_OK, CONNECTIONS_TH, ND_ROWS_PLANNING, _KFC_FIELDS, _ND_INPUTS, _ND_OUTPUTS, _KfCullingView, _LocalMapDelta,
                   _LocalMapGraph, _NormalDepth)
from ._core import _Handle, _check, _p, lib


_LM_FIELDS = tuple((k, np.int32) for k in ("point_nobs", "obs_off", "obs_kf", "kf_mp_off", "kf_mp", "kf_best", "kf_child_off", "kf_child",
                                           "kf_parent")) + (("point_bad", np.uint8), ("kf_bad", np.uint8))
_LMD_FIELDS = _LM_FIELDS + (("point_row", np.int32), ("kf_mp_row", np.int32), ("kf_link_row", np.int32))


def _set_arrays(s, d, fields, keep):
    """the arrays d[name] of `fields` (name, dtype) as pointers in the struct s: None is NULL, an empty array is not (it points to
    keep[0]); `keep` holds the arrays"""
    for k, dt in fields:
        a = d.get(k)
        if a is None:
            setattr(s, k, None)
            continue
        a = np.ascontiguousarray(a, dt).reshape(-1)
        keep.append(a)
        setattr(s, k, a.ctypes.data if a.size else keep[0].ctypes.data)
    return s


def _local_map_graph(g, keep):
    """a graph dict (the fields of aos2_local_map_graph_t; an array may be None = NULL) -> the struct; `keep` holds the arrays"""
    s = _LocalMapGraph()
    s.n_points, s.n_keyframes = int(g["n_points"]), int(g["n_keyframes"])
    return _set_arrays(s, g, _LM_FIELDS, keep)


def _kf_culling_view(v, keep):
    """a view dict (the fields of aos2_kf_culling_view_t; an array may be None = NULL) -> the struct; `keep` holds the arrays"""
    return _set_arrays(_KfCullingView(), v, _KFC_FIELDS, keep)


def _local_map_delta(d, keep):
    """a delta dict (the fields of aos2_local_map_delta_t; an array may be None = NULL, `view` a view dict or None; the three row
    counts default to the lengths of their row lists) -> the struct; `keep` holds the arrays and the view struct"""
    s = _LocalMapDelta()
    s.n_points, s.n_keyframes = int(d["n_points"]), int(d["n_keyframes"])
    _set_arrays(s, d, _LMD_FIELDS, keep)
    for n, rows in (("n_point_rows", "point_row"), ("n_kf_mp_rows", "kf_mp_row"), ("n_kf_link_rows", "kf_link_row")):
        setattr(s, n, int(d[n]) if n in d else (0 if d.get(rows) is None else len(d[rows])))
    if d.get("view") is not None:
        v = _kf_culling_view(d["view"], keep)
        keep.append(v)
        s.view = C.addressof(v)
    return s


def _kf_culling_call(fn, first, monocular, cand, bad_cap):
    """the arguments that aos2_local_map_keyframe_culling and its host tap share -> dict(status uint8 [n], n_mps, n_redundant int32
    [n], n_bad_points int, bad_points int32 [bad_cap + 1]: one element more than the call may write, preset to -7)"""
    cand = np.ascontiguousarray(cand, np.int32).reshape(-1)
    n = len(cand)
    status = np.full(max(n, 1), 255, np.uint8)
    n_mps, n_red = np.full(max(n, 1), -7, np.int32), np.full(max(n, 1), -7, np.int32)
    bad = np.full(int(bad_cap) + 1, -7, np.int32)
    nb = C.c_int32(-7)
    _check(fn(*first, int(bool(monocular)), n, _p(cand), _p(status), _p(n_mps), _p(n_red), _p(bad), int(bad_cap), C.byref(nb)))
    return dict(status=status[:n], n_mps=n_mps[:n], n_redundant=n_red[:n], n_bad_points=int(nb.value), bad_points=bad)


def _update_connections_call(fn, first, th, kf, mp, conn_cap, ordered_cap, mp_cap=None):
    """the arguments that aos2_local_map_update_connections and its host tap share.  kf: the rows; mp: None (the resident matches)
    or one sequence of point rows per keyframe -> dict(n_conn, n_ordered int32 [n], conn_kf, conn_w int32 [n][conn_cap], ordered_kf,
    ordered_w int32 [n][ordered_cap], guard: the word behind each of the six arrays, preset to -7).  A capacity of 0 passes NULL."""
    kf = np.ascontiguousarray(kf, np.int32).reshape(-1)
    n = len(kf)
    n_mp = mp2 = None
    if mp is not None:
        if len(mp) != n:
            raise ValueError("one list of matches per keyframe")
        n_mp = np.array([len(x) for x in mp] + [0], np.int32)
        mp_cap = max(1, int(n_mp.max())) if mp_cap is None else int(mp_cap)
        mp2 = np.full((max(n, 1), mp_cap), -1, np.int32)
        for k, x in enumerate(mp):
            mp2[k, :min(len(x), mp_cap)] = np.asarray(x, np.int32)[:mp_cap]
    else:
        mp_cap = 0
    conn_cap, ordered_cap = int(conn_cap), int(ordered_cap)
    flat = {k: np.full(n * c + 1, -7, np.int32) for k, c in (("n_conn", 1), ("n_ordered", 1), ("conn_kf", conn_cap), ("conn_w", conn_cap),
                                                             ("ordered_kf", ordered_cap), ("ordered_w", ordered_cap))}

    def arg(k, c):
        return _p(flat[k]) if c > 0 else None
    _check(fn(*first, int(th), n, _p(kf), None if mp is None else _p(n_mp), None if mp is None else _p(mp2), mp_cap,
              _p(flat["n_conn"]), arg("conn_kf", conn_cap), arg("conn_w", conn_cap), conn_cap,
              _p(flat["n_ordered"]), arg("ordered_kf", ordered_cap), arg("ordered_w", ordered_cap), ordered_cap))
    out = dict(n_conn=flat["n_conn"][:n], n_ordered=flat["n_ordered"][:n], guard={k: int(a[-1]) for k, a in flat.items()})
    for k, c in (("conn_kf", conn_cap), ("conn_w", conn_cap), ("ordered_kf", ordered_cap), ("ordered_w", ordered_cap)):
        out[k] = flat[k][:n * c].reshape(n, c)
    return out


def _normal_depth_args(point, xyz, ref_kf, kf_center, scale, rows_form=ND_ROWS_PLANNING, term_off=None, want=None, n=None, n_levels=None,
                       null=()):
    """an aos2_normal_depth_t, which aos2_local_map_update_normal_depth and its host tap share -> (the struct, what keeps its input
    arrays alive, the output arrays by name, each with one guard element behind it).  point int32 [n], xyz float32 [n][3], ref_kf int32
    [n], kf_center float32 [n_keyframes][3], scale float32 [n_levels], term_off int32 [n + 1] or None.  want: the outputs that are
    asked for (default: all of them, the per-observation ones only with term_off); the others go in as NULL.  n / n_levels override
    the counts and `null` names input fields that go in as NULL whatever was passed (what the argument checks are tried with).
    The outputs are [n] or [n][3] or per observation slot, PRESET to a sentinel -- status 255, n_terms -7, the floats -7.0 -- so that
    what the call leaves untouched shows; the call's dict holds them without their guard elements, which are in `guard`."""
    ins = dict(point=point, xyz=xyz, ref_kf=ref_kf, kf_center=kf_center, scale=scale, term_off=term_off)
    s, keep = _NormalDepth(), [np.zeros(1, np.int32)]
    for k, dt in _ND_INPUTS:
        ins[k] = None if ins[k] is None else np.ascontiguousarray(ins[k], dt).reshape(-1)
    count = (0 if ins["point"] is None else len(ins["point"])) if n is None else int(n)
    s.n, s.rows_form = count, int(rows_form)
    s.n_levels = (0 if ins["scale"] is None else len(ins["scale"])) if n_levels is None else int(n_levels)
    _set_arrays(s, {k: None if k in null else a for k, a in ins.items()}, _ND_INPUTS, keep)
    slots = int(ins["term_off"][-1]) if ins["term_off"] is not None and len(ins["term_off"]) else 0
    want = [k for k, _, per in _ND_OUTPUTS if per is not None or term_off is not None] if want is None else list(want)
    flat = {}
    for k, dt, per in _ND_OUTPUTS:
        if k in want:
            size = max(count, 0) * per if per is not None else max(slots, 0) * (3 if k == "term_unit" else 1)
            flat[k] = np.full(size + 1, 255 if dt == np.uint8 else -7, dt)
            setattr(s, k, flat[k].ctypes.data)
    return s, keep, flat


def _update_normal_depth_call(fn, first, *args, **kw):
    """one call with the arguments of _normal_depth_args -> its dict of outputs"""
    s, keep, flat = _normal_depth_args(*args, **kw)
    _check(fn(*first, C.byref(s)))
    out = dict(guard={k: a[-1] for k, a in flat.items()})
    for k, a in flat.items():
        out[k] = a[:-1].reshape(-1, 3) if k in ("normal", "term_unit") else a[:-1]
    return out


class LocalMap(_Handle):
    """The covisibility graph resident on the device and Tracking::UpdateLocalMap (src/Tracking.cc:1375-1519) for the frames of a
    capi.Frames batch.  A graph is a dict with the fields of aos2_local_map_graph_t (numpy arrays, CSR offsets)."""

    KIND = "local_map"

    def __init__(self, device=0):
        self._create(device)

    def set(self, graph, ok=(AOS2_OK,)):
        """aos2_local_map_set; `ok`: the return values that do not raise (a machine without a device keeps a checked graph and
        returns AOS2_ERR_NO_DEVICE)"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_graph(graph, keep)
        return _check(self.L.aos2_local_map_set(self.h, C.byref(s)), ok)

    def graph(self):
        """the handle's snapshot as a graph dict (copies)"""
        s = _LocalMapGraph()
        _check(self.L.aos2_local_map_get(self.h, C.byref(s)))
        npnt, nk = s.n_points, s.n_keyframes
        g = dict(n_points=npnt, n_keyframes=nk)

        def arr(p, n, dt):
            if not n:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8 if dt == np.uint8 else C.c_int32)), (n,)).astype(dt, copy=True)

        for k, n in (("obs_off", npnt + 1), ("kf_mp_off", nk + 1), ("kf_child_off", nk + 1), ("point_nobs", npnt), ("kf_parent", nk),
                     ("kf_best", nk * 10)):
            g[k] = arr(getattr(s, k), n, np.int32)
        g["point_bad"], g["kf_bad"] = arr(s.point_bad, npnt, np.uint8), arr(s.kf_bad, nk, np.uint8)
        for k, off in (("obs_kf", "obs_off"), ("kf_mp", "kf_mp_off"), ("kf_child", "kf_child_off")):
            g[k] = arr(getattr(s, k), int(g[off][-1]), np.int32)
        return g

    def view(self):
        """the handle's culling view as a view dict (copies, parallel to graph()), None if it holds none"""
        s, v = _LocalMapGraph(), _KfCullingView()
        _check(self.L.aos2_local_map_get(self.h, C.byref(s)))
        has = C.c_int32(0)
        _check(self.L.aos2_local_map_get_culling_view(self.h, C.byref(v), C.byref(has)))
        if not has.value:
            return None
        nk = s.n_keyframes
        n_obs = int(np.ctypeslib.as_array(C.cast(s.obs_off, C.POINTER(C.c_int32)), (s.n_points + 1,))[-1])
        n_mp = int(np.ctypeslib.as_array(C.cast(s.kf_mp_off, C.POINTER(C.c_int32)), (nk + 1,))[-1])
        lens = dict(obs_idx=n_obs, kf_octave=n_mp, kf_depth=n_mp, kf_stereo=n_mp, kf_th_depth=nk, kf_flags=nk)
        out = {}
        for k, dt in _KFC_FIELDS:
            n, nbytes = lens[k], lens[k] * np.dtype(dt).itemsize
            out[k] = np.frombuffer(C.string_at(getattr(v, k), nbytes), dt).copy() if n else np.zeros(0, dt)
        return out

    def apply(self, delta, ok=(AOS2_OK,)):
        """aos2_local_map_apply: a delta is a dict with the fields of aos2_local_map_delta_t (`view`: a view dict or None); `ok` as in
        set()"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_delta(delta, keep)
        return _check(self.L.aos2_local_map_apply(self.h, C.byref(s)), ok)

    def apply_host(self, delta, ok=(AOS2_OK,)):
        """aos2_debug_local_map_apply_host: the rebuild forced onto the host, the device copy marked dirty"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_delta(delta, keep)
        return _check(self.L.aos2_debug_local_map_apply_host(self.h, C.byref(s)), ok)

    def last_apply(self):
        """aos2_local_map_last_apply -> dict(path 0 host / 1 device, reallocated, device_ms, bytes uploaded)"""
        path, re, ms = C.c_int32(-1), C.c_int32(0), C.c_float(-1)
        _check(self.L.aos2_local_map_last_apply(self.h, C.byref(path), C.byref(re), C.byref(ms)))
        return dict(path=path.value, reallocated=re.value, device_ms=float(ms.value),
                    bytes=int(self.L.aos2_local_map_last_apply_bytes(self.h)))

    def debug_apply_tile(self, rows=0):
        _check(self.L.aos2_local_map_debug_apply_tile(self.h, int(rows)))

    def update(self, frames, d_local, local_cap, d_n_local, d_local_kfs, kf_cap, d_n_local_kfs, d_ref_kf):
        """aos2_frames_update_local_map: device addresses (ints); enqueued on the batch's stream"""
        _check(self.L.aos2_frames_update_local_map(frames.h, self.h, d_local, int(local_cap), d_n_local, d_local_kfs, int(kf_cap),
                                                   d_n_local_kfs, d_ref_kf))

    def stats(self, frames, d_stats, d_found_inc=0, stereo=False, only_tracking=False):
        """aos2_frames_track_local_map_stats: d_stats int32 [batch][3], d_found_inc int32 [n_points] or 0"""
        _check(self.L.aos2_frames_track_local_map_stats(frames.h, self.h, int(bool(stereo)), int(bool(only_tracking)), d_stats,
                                                        d_found_inc or None))

    def debug_limits(self, scratch_bytes=0, lds_keyframes=-1):
        _check(self.L.aos2_local_map_debug_limits(self.h, int(scratch_bytes), int(lds_keyframes)))

    def last_groups(self):
        return self.L.aos2_local_map_last_groups(self.h)

    def set_culling_view(self, view, ok=(AOS2_OK,)):
        """aos2_local_map_set_culling_view: a view is a dict with the fields of aos2_kf_culling_view_t; `ok` as in set()"""
        keep = [np.zeros(1, np.int32)]
        s = _kf_culling_view(view, keep)
        return _check(self.L.aos2_local_map_set_culling_view(self.h, C.byref(s)), ok)

    def keyframe_culling(self, cand, monocular=False, bad_cap=None):
        """aos2_local_map_keyframe_culling (LocalMapping::KeyFrameCulling, src/LocalMapping.cc:636-700) on the device; bad_cap
        defaults to the number of points of the handle's graph -> the dict of _kf_culling_call"""
        if bad_cap is None:
            s = _LocalMapGraph()
            _check(self.L.aos2_local_map_get(self.h, C.byref(s)))
            bad_cap = s.n_points
        return _kf_culling_call(self.L.aos2_local_map_keyframe_culling, (self.h,), monocular, cand, bad_cap)

    def debug_culling_rounds(self, rounds=0):
        _check(self.L.aos2_local_map_debug_culling_rounds(self.h, int(rounds)))

    def last_culling_rounds(self):
        return self.L.aos2_local_map_last_culling_rounds(self.h)

    def last_culling_device_ms(self):
        return float(self.L.aos2_local_map_last_culling_device_ms(self.h))

    @staticmethod
    def keyframe_culling_host(graph, view, cand, monocular=False, bad_cap=None):
        """aos2_debug_keyframe_culling_host: the same loop on one core, no device"""
        keep = [np.zeros(1, np.int32)]
        g, v = _local_map_graph(graph, keep), _kf_culling_view(view, keep)
        bad_cap = int(graph["n_points"]) if bad_cap is None else bad_cap
        return _kf_culling_call(lib().aos2_debug_keyframe_culling_host, (C.byref(g), C.byref(v)), monocular, cand, bad_cap)

    def update_connections(self, kf, mp=None, th=CONNECTIONS_TH, conn_cap=256, ordered_cap=256, mp_cap=None):
        """aos2_local_map_update_connections (KeyFrame::UpdateConnections, src/KeyFrame.cc:350-440) on the device -> the dict of
        _update_connections_call"""
        return _update_connections_call(self.L.aos2_local_map_update_connections, (self.h,), th, kf, mp, conn_cap, ordered_cap, mp_cap)

    @staticmethod
    def update_connections_host(graph, kf, mp=None, th=CONNECTIONS_TH, conn_cap=256, ordered_cap=256, mp_cap=None):
        """aos2_debug_update_connections_host: the same function on one core, no device"""
        keep = [np.zeros(1, np.int32)]
        g = _local_map_graph(graph, keep)
        return _update_connections_call(lib().aos2_debug_update_connections_host, (C.byref(g),), th, kf, mp, conn_cap, ordered_cap, mp_cap)

    def debug_connections_sort(self, lds_entries=0):
        _check(self.L.aos2_local_map_debug_connections_sort(self.h, int(lds_entries)))

    def last_connections_device_ms(self):
        return float(self.L.aos2_local_map_last_connections_device_ms(self.h))

    def update_normal_depth(self, point, xyz, ref_kf, kf_center, scale, **kw):
        """aos2_local_map_update_normal_depth (MapPoint::UpdateNormalAndDepth, src/MapPoint.cc:363-413) on the device; the keywords
        and the result are those of _update_normal_depth_call"""
        return _update_normal_depth_call(self.L.aos2_local_map_update_normal_depth, (self.h,), point, xyz, ref_kf, kf_center, scale, **kw)

    @staticmethod
    def update_normal_depth_host(graph, view, point, xyz, ref_kf, kf_center, scale, **kw):
        """aos2_debug_update_normal_depth_host: the same function on one core, no device"""
        keep = [np.zeros(1, np.int32)]
        g, v = _local_map_graph(graph, keep), _kf_culling_view(view, keep)
        return _update_normal_depth_call(lib().aos2_debug_update_normal_depth_host, (C.byref(g), C.byref(v)), point, xyz, ref_kf,
                                         kf_center, scale, **kw)

    def debug_normal_depth(self, lds_terms=-1):
        _check(self.L.aos2_local_map_debug_normal_depth(self.h, int(lds_terms)))

    def last_normal_depth_device_ms(self):
        return float(self.L.aos2_local_map_last_normal_depth_device_ms(self.h))

    def update_host(self, n, mp, local_cap, kf_cap, local_kfs=None, n_local_kfs=None, ref_kf=None):
        """aos2_local_map_update: the device kernels on host arrays, arguments and result as host()"""
        return self._on_host_arrays(self.L.aos2_local_map_update, self.h, n, mp, local_cap, kf_cap, local_kfs, n_local_kfs, ref_kf)

    @staticmethod
    def host(graph, n, mp, local_cap, kf_cap, local_kfs=None, n_local_kfs=None, ref_kf=None):
        """aos2_debug_local_map_host: n int32 [B], mp int32 [B][cap]; the previous lists default to empty and ref_kf to -1 ->
        dict(mp, local, n_local, local_kfs, n_local_kfs, ref_kf), new arrays"""
        keep = [np.zeros(1, np.int32)]
        s = _local_map_graph(graph, keep)
        return LocalMap._on_host_arrays(lib().aos2_debug_local_map_host, C.byref(s), n, mp, local_cap, kf_cap, local_kfs, n_local_kfs, ref_kf)

    @staticmethod
    def _on_host_arrays(fn, first, n, mp, local_cap, kf_cap, local_kfs, n_local_kfs, ref_kf):
        mp = np.array(mp, np.int32, ndmin=2)
        B, cap = mp.shape
        n = np.ascontiguousarray(n, np.int32).reshape(B)
        lk = np.full((B, kf_cap), -1, np.int32) if local_kfs is None else np.array(local_kfs, np.int32).reshape(B, kf_cap)
        nlk = np.zeros(B, np.int32) if n_local_kfs is None else np.array(n_local_kfs, np.int32).reshape(B)
        ref = np.full(B, -1, np.int32) if ref_kf is None else np.array(ref_kf, np.int32).reshape(B)
        local, n_local = np.full((B, local_cap), -7, np.int32), np.full(B, -7, np.int32)
        _check(fn(first, B, cap, _p(n), _p(mp), _p(local), int(local_cap), _p(n_local), _p(lk), int(kf_cap), _p(nlk), _p(ref)))
        return dict(mp=mp, local=local, n_local=n_local, local_kfs=lk, n_local_kfs=nlk, ref_kf=ref)

    @staticmethod
    def stats_host(graph, n, mp, outlier, stereo=False, only_tracking=False, found_inc=True):
        """aos2_debug_local_map_stats_host -> dict(stats int32 [B][3], mp, found_inc int32 [n_points] | None)"""
        mp = np.array(mp, np.int32, ndmin=2)
        B, cap = mp.shape
        n = np.ascontiguousarray(n, np.int32).reshape(B)
        outlier = np.ascontiguousarray(outlier, np.uint8).reshape(B, cap)
        stats = np.zeros((B, 3), np.int32)
        inc = np.zeros(max(int(graph["n_points"]), 1), np.int32) if found_inc else None
        keep = [np.zeros(1, np.int32)]
        s = _local_map_graph(graph, keep)
        _check(lib().aos2_debug_local_map_stats_host(C.byref(s), B, cap, _p(n), _p(mp), _p(outlier), int(bool(stereo)),
                                                     int(bool(only_tracking)), _p(stats), _p(inc) if found_inc else None))
        return dict(stats=stats, mp=mp, found_inc=None if inc is None else inc[:int(graph["n_points"])])
