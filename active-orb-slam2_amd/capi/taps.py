"""Test taps of single host routines and device kernels (include/aos2.h: aos2_debug_*)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import _PosePassCase
from ._core import AosError, _check, _p, lib


def debug_octree_host(xs, ys, score, minX, maxX, minY, maxY, N):
    xs = np.ascontiguousarray(xs, np.int16)
    ys = np.ascontiguousarray(ys, np.int16)
    score = np.ascontiguousarray(score, np.uint8)
    out = np.zeros(max(len(xs), 1), np.int32)
    k = lib().aos2_debug_octree_host(_p(xs), _p(ys), _p(score), len(xs), minX, maxX, minY, maxY, N, _p(out), len(out))
    if k < 0:
        raise AosError(k, "octree scratch exhausted")
    return out[:k].copy()


def debug_sincos_host(angle_rad):
    s, c = C.c_float(), C.c_float()
    lib().aos2_debug_sincos_host(float(angle_rad), C.byref(s), C.byref(c))
    return s.value, c.value


def debug_sincos_device(angles, device=0):
    a = np.ascontiguousarray(angles, np.float32)
    s = np.zeros_like(a)
    c = np.zeros_like(a)
    _check(lib().aos2_debug_sincos_device(_p(a), len(a), _p(s), _p(c), device))
    return s, c


WAVE_OPS_I = ("dpp_u32_B1", "dpp_u32_4E", "dpp_u32_141", "dpp_u32_140", "dpp_i32_B1", "dpp_i32_4E", "dpp_i32_141", "dpp_i32_140",
              "row_sum", "sum", "max", "row_min", "min", "incl_scan", "block_excl_scan", "block_total", "block_sum")
WAVE_OPS_D = ("dpp_f64_B1", "dpp_f64_4E", "dpp_f64_141", "dpp_f64_140", "row_sum_f64", "readlane_0", "readlane_63")


def debug_wave_ops_device(vi, vd, device=0):
    """test tap: every primitive of csrc/wave_ops.h; vi (int32), vd (float64) [cases][nt], nt = 128 or 256 threads per workgroup
    -> dict name -> [cases][nt] (WAVE_OPS_I as int32, the row / wave min as uint32; WAVE_OPS_D as float64)"""
    vi = np.ascontiguousarray(vi, np.int32); vd = np.ascontiguousarray(vd, np.float64)
    assert vi.ndim == 2 and vi.shape == vd.shape
    oi = np.zeros(vi.shape + (len(WAVE_OPS_I),), np.int32)
    od = np.zeros(vi.shape + (len(WAVE_OPS_D),), np.float64)
    _check(lib().aos2_debug_wave_ops_device(_p(vi), _p(vd), vi.shape[0], vi.shape[1], _p(oi), _p(od), device))
    out = {k: oi[..., j].copy() for j, k in enumerate(WAVE_OPS_I)}
    out.update({k: od[..., j].copy() for j, k in enumerate(WAVE_OPS_D)})
    for k in ("row_min", "min"):
        out[k] = out[k].view(np.uint32)
    return out


def debug_row_sums_scatter_device(v, device=0):
    """test tap: row_sums_scatter_f64<K> of csrc/wave_ops.h by one wave; v (float64) [64][K], K = 7, 36 or 42
    -> (every lane's slots [64][ceil(K / 16)], owner [K][2] = (lane of a row, slot) of the total of value i)"""
    v = np.ascontiguousarray(v, np.float64)
    assert v.ndim == 2 and v.shape[0] == 64
    K = v.shape[1]
    out = np.zeros((64, (K + 15) // 16), np.float64)
    owner = np.zeros((K, 2), np.int32)
    _check(lib().aos2_debug_row_sums_scatter_device(_p(v), K, _p(out), _p(owner), device))
    return out, owner


def debug_pose_blocks_device(upd, T, Hb, lam, x0, device=0):
    """test tap: the pose solver's exp-map update and 6x6 solve on the device, n independent cases"""
    upd = np.ascontiguousarray(upd, np.float64); T = np.ascontiguousarray(T, np.float64)
    Hb = np.ascontiguousarray(Hb, np.float64); lam = np.ascontiguousarray(lam, np.float64)
    x = np.ascontiguousarray(x0, np.float64).copy()
    n = len(lam)
    To = np.zeros((n, 7)); ok = np.zeros(n, np.uint8)
    _check(lib().aos2_debug_pose_blocks_device(_p(upd), _p(T), _p(To), _p(Hb), _p(lam), _p(x), _p(ok), n, device))
    return To, x, ok


POSE_PASS_FORMS = ((4, 256, 1024), (8, 256, 2048), (9, 128, 1152), (0, 256, None))   # form -> (kEpt, NT, largest n)


def debug_pose_pass_device(cases, mode, device=0):
    """test tap: pose_optimization_body of csrc/pose_opt.h, one workgroup per case in the instantiation POSE_PASS_FORMS[case["form"]].
    cases: synth_pose_problem()-style dicts (n, Xw, obs, stereo, inv_sigma2, fx .. bf) with form, pose (7 doubles qx qy qz qw tx ty tz) and,
    optional, it (0), level1 (zeros), robust (ones), outlier (zeros), chi2 (zeros), [n] each.  mode 1: one edge pass -> sums (28: H upper
    triangle, b, robust chi2), chi2 [n]; mode 2: the reclassification of round it -> outlier, level1, robust, chi2, n_bad; mode 0: the
    whole procedure -> outlier, n_bad, n_inliers, pose_out, Tcw.  -> one dict per case with all of them"""
    n_cases = len(cases)
    S = (_PosePassCase * max(n_cases, 1))()
    keep = []
    for s, c in zip(S, cases):
        n = int(c["n"])
        s.n, s.form, s.it = n, int(c["form"]), int(c.get("it", 0))
        arrs = {}
        for name, dt, fill in (("Xw", np.float32, None), ("obs", np.float32, None), ("inv_sigma2", np.float32, None), ("stereo", np.uint8, None),
                               ("level1", np.uint8, 0), ("robust", np.uint8, 1), ("outlier", np.uint8, 0), ("chi2", np.float64, 0)):
            a = np.full(n, fill, dt) if c.get(name) is None else np.array(c[name], dt, order="C").reshape(-1)
            assert a.size == n * (3 if name in ("Xw", "obs") else 1), name
            a = np.concatenate([a, np.zeros(1, dt)])   # (never an empty array)
            arrs[name] = a
            setattr(s, name, a.ctypes.data)
        keep.append(arrs)
        s.fx, s.fy, s.cx, s.cy, s.bf = (float(np.float32(c[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
        s.pose = (C.c_double * 7)(*[float(x) for x in np.asarray(c["pose"], np.float64).reshape(7)])
    _check(lib().aos2_debug_pose_pass_device(C.byref(S) if n_cases else None, n_cases, int(mode), device))
    return [dict(sums=np.array(list(s.sums), np.float64), pose_out=np.array(list(s.pose_out), np.float64), Tcw=np.array(list(s.Tcw), np.float32),
                 n_bad=int(s.n_bad), n_inliers=int(s.n_inliers), **{k: a[k][:s.n].copy() for k in ("level1", "robust", "outlier", "chi2")})
            for s, a in zip(S, keep)]


def debug_lba_reduced_solve_device(cases, device=0):
    """test tap: LocalBA's reduced-system kernels alone, all cases in one launch of each.  cases: dicts with form (0 = k_ldlt_dev,
    2 = k_ldlt_reg), H (n x n, n = 6 np), bs, b_pose, x0, scale0 (n each: what x / scale_terms hold on entry), lam, T (np x 7)
    -> one dict per case: ok, x, scale_terms (n), T_out, T_backup (np x 7)"""
    cat = lambda k, dt=np.float64: np.ascontiguousarray(np.concatenate([np.asarray(c[k], dt).ravel() for c in cases]))
    nps = np.array([np.asarray(c["bs"]).size // 6 for c in cases], np.int32)
    for c, q in zip(cases, nps):
        assert np.asarray(c["H"]).shape == (6 * q, 6 * q) and np.asarray(c["T"]).shape == (q, 7)
        assert all(np.asarray(c[k]).shape == (6 * q,) for k in ("bs", "b_pose", "x0", "scale0"))
    form = np.array([c["form"] for c in cases], np.int32)
    H, bs, bp, T, x, sc = cat("H"), cat("bs"), cat("b_pose"), cat("T"), cat("x0"), cat("scale0")
    lam = np.array([c["lam"] for c in cases], np.float64)
    To, Tb, ok = np.zeros_like(T), np.zeros_like(T), np.zeros(len(cases), np.uint8)
    _check(lib().aos2_debug_lba_reduced_solve_device(len(cases), _p(nps), _p(form), _p(H), _p(bs), _p(bp), _p(lam), _p(T), _p(x), _p(To), _p(Tb),
                                                     _p(sc), _p(ok), device))
    out, o6, o7 = [], 0, 0
    for q, k in zip(nps, ok):
        out.append(dict(ok=int(k), x=x[o6:o6 + 6 * q].copy(), scale_terms=sc[o6:o6 + 6 * q].copy(),
                        T_out=To[o7:o7 + 7 * q].reshape(q, 7).copy(), T_backup=Tb[o7:o7 + 7 * q].reshape(q, 7).copy()))
        o6 += 6 * q; o7 += 7 * q
    return out
