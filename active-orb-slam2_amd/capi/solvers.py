"""The geometric solvers: triangulation of keyframe matches, Sim3Solver, PnPsolver and Initializer (include/aos2.h:
aos2_triangulate_matches, aos2_sim3_ransac, aos2_pnp_ransac, aos2_initializer_initialize): argument builders and host taps."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (TRIANG_OBS, _InitProblem, _InitResult, _PnpProblem, _PnpResult, _Sim3Problem, _Sim3Result, _TriangGeom)
from ._build import _batch, _out, _set_K
from ._core import _check, _p, lib


def _triang_args(kf1, kf2, obs1, obs2):
    """kf1 / kf2: dicts with Tcw (4x4), fx fy cx cy mb mbf, scale_factors; obs1 / obs2: TRIANG_OBS arrays of the n matches"""
    g = _TriangGeom()
    sf1, sf2 = (np.asarray(k["scale_factors"], np.float32) for k in (kf1, kf2))
    if len(sf1) != len(sf2) or len(sf1) > 8:
        raise ValueError("both keyframes carry the same (at most 8) pyramid levels")
    g.n_levels = len(sf1)
    for tag, k, sf in (("1", kf1, sf1), ("2", kf2, sf2)):
        setattr(g, "Tcw" + tag, (C.c_float * 16)(*[float(v) for v in np.asarray(k["Tcw"], np.float32).reshape(16)]))
        for name in ("fx", "fy", "cx", "cy", "mb", "mbf"):
            setattr(g, name + tag, float(np.float32(k[name])))
        setattr(g, "scale_factors" + tag, (C.c_float * 8)(*[float(v) for v in sf]))
    obs1, obs2 = np.ascontiguousarray(obs1, TRIANG_OBS), np.ascontiguousarray(obs2, TRIANG_OBS)
    if obs1.shape != obs2.shape or obs1.ndim != 1:
        raise ValueError("one observation of each keyframe per match")
    n = len(obs1)
    return g, n, obs1, obs2, np.zeros((n, 3), np.float32), np.zeros(n, np.uint8)


def debug_triangulate_host(kf1, kf2, obs1, obs2):
    """aos2_debug_triangulate_host: the routine of the device kernels on the CPU -> (status uint8 [n], x3D float32 [n][3])"""
    g, n, obs1, obs2, x3D, status = _triang_args(kf1, kf2, obs1, obs2)
    _check(lib().aos2_debug_triangulate_host(C.byref(g), n, _p(obs1), _p(obs2), _p(x3D), _p(status)))
    return status, x3D


def sim3_random_int(rng, lo, hi):
    """DUtils::Random::RandomInt(min, max) (Thirdparty/DBoW2/DUtils/Random.cpp:47-50): d = max - min + 1,
    int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min, with rand() taken from `rng` (a numpy Generator)"""
    d = hi - lo + 1
    return int((float(rng.integers(0, 2 ** 31)) / (2147483647.0 + 1.0)) * d) + lo


def sim3_draws(rng, n, max_iterations):
    """the draws of max_iterations iterations of Sim3Solver::iterate (:166-177) over n correspondences, in iteration order:
    int32 [max_iterations][3], draw i of an iteration = RandomInt(0, n - 1 - i); zeros when n < 3 (nothing to draw from)"""
    d = np.zeros((max_iterations, 3), np.int32)
    if n >= 3:
        for k in range(max_iterations):
            for i in range(3):
                d[k, i] = sim3_random_int(rng, 0, n - 1 - i)
    return d


def _sim3_args(problems, sentinel=None):
    """problems: dicts with X3Dc1 / X3Dc2 [n][3], max_err1 / max_err2 [n], K1 / K2 = (fx, fy, cx, cy), fix_scale, probability,
    min_inliers, max_iterations, draws [max_iterations][3]"""
    P, R, keep, outs = _batch(_Sim3Problem, _Sim3Result, len(problems))
    for i, q in enumerate(problems):
        arr = [np.ascontiguousarray(q[k], np.float32) for k in ("X3Dc1", "X3Dc2", "max_err1", "max_err2")]
        draws = np.ascontiguousarray(q["draws"], np.int32)
        n, its = len(arr[0]), int(q["max_iterations"])
        if arr[0].shape != (n, 3) or arr[1].shape != (n, 3) or arr[2].shape != (n,) or arr[3].shape != (n,) or draws.shape != (max(its, 0), 3):
            raise ValueError("problem %d: X3Dc [n][3], max_err [n], draws [max_iterations][3]" % i)
        inl, counts = _out(n, np.uint8, sentinel), _out(max(its, 0), np.int32, sentinel, -1)
        keep += arr + [draws]
        outs.append((inl, counts))
        P[i].n = n
        P[i].X3Dc1, P[i].X3Dc2, P[i].max_err1, P[i].max_err2, P[i].draws = (a.ctypes.data for a in arr + [draws])
        _set_K(P[i], q["K1"], "1")
        _set_K(P[i], q["K2"], "2")
        P[i].fix_scale, P[i].probability = int(bool(q["fix_scale"])), float(q["probability"])
        P[i].min_inliers, P[i].max_iterations = int(q["min_inliers"]), its
        R[i].inliers, R[i].counts = inl.ctypes.data, counts.ctypes.data
        if sentinel is not None:
            R[i].ransac_max_its = R[i].first_success = R[i].best_iteration = R[i].best_inliers = sentinel
    return P, R, keep, outs


def _sim3_results(R, outs):
    return [dict(ransac_max_its=R[i].ransac_max_its, first_success=R[i].first_success, best_iteration=R[i].best_iteration,
                 best_inliers=R[i].best_inliers, T12=np.array(R[i].T12, np.float32).reshape(4, 4), R12=np.array(R[i].R12, np.float32).reshape(3, 3),
                 t12=np.array(R[i].t12, np.float32), s12=np.float32(R[i].s12), inliers=inl, counts=counts)
            for i, (inl, counts) in enumerate(outs)]


def debug_sim3_host(problems):
    """aos2_debug_sim3_host: the routine of the device kernels on the CPU -> one dict per problem (the fields of aos2_sim3_result_t)"""
    P, R, keep, outs = _sim3_args(problems)
    _check(lib().aos2_debug_sim3_host(P, R, len(problems)))
    return _sim3_results(R, outs)


def pnp_ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """aos2_pnp_ransac_parameters: SetRansacParameters (src/PnPsolver.cc:121-157; the defaults of include/PnPsolver.h:63) ->
    (mRansacMinInliers, mRansacEpsilon, mRansacMaxIts) as adjusted for n correspondences"""
    mi, eps, its = C.c_int32(), C.c_float(), C.c_int32()
    _check(lib().aos2_pnp_ransac_parameters(int(n), float(probability), int(min_inliers), int(max_iterations), int(min_set), float(np.float32(epsilon)),
                                            C.byref(mi), C.byref(eps), C.byref(its)))
    return mi.value, np.float32(eps.value), its.value


def pnp_draws(rng, n, n_iterations, min_set):
    """the draws of n_iterations iterations of PnPsolver::iterate (:191-201) over n correspondences, in iteration order:
    int32 [n_iterations][min_set], draw i of an iteration = RandomInt(0, n - 1 - i); zeros when n < min_set (nothing to draw from)"""
    d = np.zeros((n_iterations, min_set), np.int32)
    if n >= min_set:
        for k in range(n_iterations):
            for i in range(min_set):
                d[k, i] = sim3_random_int(rng, 0, n - 1 - i)
    return d


def _pnp_args(problems, sentinel=None, with_counts=True):
    """problems: dicts with P3Dw [n][3], P2D [n][2], max_err [n], K = (fx, fy, cx, cy), min_inliers (adjusted), min_set, n_iterations,
    draws [n_iterations][min_set], and optionally the carried state first_iteration, best_inliers_in, best_in [n]"""
    P, R, keep, outs = _batch(_PnpProblem, _PnpResult, len(problems))
    for i, q in enumerate(problems):
        arr = [np.ascontiguousarray(q[k], np.float32) for k in ("P3Dw", "P2D", "max_err")]
        n, its, ms = len(arr[0]), int(q["n_iterations"]), int(q["min_set"])
        draws = np.ascontiguousarray(q["draws"], np.int32)
        if arr[0].shape != (n, 3) or arr[1].shape != (n, 2) or arr[2].shape != (n,) or draws.shape != (max(its, 0), ms):
            raise ValueError("problem %d: P3Dw [n][3], P2D [n][2], max_err [n], draws [n_iterations][min_set]" % i)
        inl, best = _out(n, np.uint8, sentinel), _out(n, np.uint8, sentinel)
        counts = _out(max(its, 0), np.int32, sentinel, -1) if with_counts else None
        keep += arr + [draws]
        outs.append((inl, best, counts))
        P[i].n = n
        P[i].P3Dw, P[i].P2D, P[i].max_err, P[i].draws = (a.ctypes.data for a in arr + [draws])
        _set_K(P[i], q["K"])
        P[i].min_inliers, P[i].min_set, P[i].n_iterations = int(q["min_inliers"]), ms, its
        P[i].first_iteration, P[i].best_inliers_in = int(q.get("first_iteration", 0)), int(q.get("best_inliers_in", 0))
        if q.get("best_in") is not None:
            bi = np.ascontiguousarray(q["best_in"], np.uint8)
            if bi.shape != (n,):
                raise ValueError("problem %d: best_in [n]" % i)
            keep.append(bi)
            P[i].best_in = bi.ctypes.data
        R[i].inliers, R[i].best = inl.ctypes.data, best.ctypes.data
        R[i].counts = counts.ctypes.data if with_counts else None
        if sentinel is not None:
            C.memset(C.byref(R[i]), sentinel, _PnpResult.inliers.offset)
            C.memset(C.byref(R[i], _PnpResult.best_iteration.offset), sentinel, _PnpResult.best.offset - _PnpResult.best_iteration.offset)
    return P, R, keep, outs


def _pnp_results(R, outs):
    return [dict(returned_at=R[i].returned_at, Tcw=np.array(R[i].Tcw, np.float32).reshape(4, 4), n_inliers=R[i].n_inliers, inliers=inl,
                 best_iteration=R[i].best_iteration, best_inliers=R[i].best_inliers, best_Tcw=np.array(R[i].best_Tcw, np.float32).reshape(4, 4),
                 best=best, counts=counts)
            for i, (inl, best, counts) in enumerate(outs)]


def debug_pnp_set(n, row):
    """aos2_debug_pnp_set: the indices the draws of one iteration select, as csrc/pnp.h forms them"""
    row = np.ascontiguousarray(row, np.int32)
    out = np.zeros(len(row), np.int32)
    _check(lib().aos2_debug_pnp_set(int(n), _p(row), len(row), _p(out)))
    return [int(i) for i in out]


def debug_pnp_scan(first_iteration, counts, refined, refined_carried, min_inliers, best_inliers_in=0):
    """aos2_debug_pnp_scan: the loop of iterate() over tables -> (returned_at, best_iteration, best_inliers)"""
    counts, refined = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(refined, np.int32)
    r = [C.c_int32() for _ in range(3)]
    _check(lib().aos2_debug_pnp_scan(int(first_iteration), len(counts), _p(counts), _p(refined), int(refined_carried), int(min_inliers),
                                     int(best_inliers_in), *[C.byref(x) for x in r]))
    return tuple(x.value for x in r)


def debug_pnp_host(problems, with_counts=True):
    """aos2_debug_pnp_host: the routine of the device kernels on the CPU -> one dict per problem (the fields of aos2_pnp_result_t)"""
    P, R, keep, outs = _pnp_args(problems, None, with_counts)
    _check(lib().aos2_debug_pnp_host(P, R, len(problems)))
    return _pnp_results(R, outs)


_INIT_SCALARS = ("status", "initialized", "used_homography", "SH", "SF", "best_iteration_h", "best_iteration_f", "n_hypotheses")
_INIT_ARRAYS = (("H21", np.float32), ("F21", np.float32), ("R21", np.float32), ("t21", np.float32), ("n_good", np.int32),
                ("parallax", np.float32))


def initializer_sets(rng, n_matches, iterations):
    """mvSets (src/Initializer.cc:78-97): per iteration 8 indices drawn without replacement by RandomInt(0, size - 1) and the
    swap-with-back removal; int32 [iterations][8]"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n_matches))
        for j in range(8):
            r = sim3_random_int(rng, 0, len(avail) - 1)
            sets[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return sets


def _init_args(problems, sentinel=None):
    """problems: dicts with keys1 [n1][2], keys2 [n2][2], matches [n][2], sets [iterations][8], K = (fx, fy, cx, cy) and optionally
    sigma (1.0), min_parallax (1.0), min_triangulated (50)"""
    P, R, keep, outs = _batch(_InitProblem, _InitResult, len(problems))
    for i, q in enumerate(problems):
        k1, k2 = np.ascontiguousarray(q["keys1"], np.float32), np.ascontiguousarray(q["keys2"], np.float32)
        mt, sets = np.ascontiguousarray(q["matches"], np.int32), np.ascontiguousarray(q["sets"], np.int32)
        if k1.ndim != 2 or k1.shape[1] != 2 or k2.ndim != 2 or k2.shape[1] != 2 or mt.ndim != 2 or mt.shape[1] != 2 or sets.ndim != 2 or sets.shape[1] != 8:
            raise ValueError("problem %d: keys1 [n1][2], keys2 [n2][2], matches [n][2], sets [iterations][8]" % i)
        out = (_out(len(mt), np.uint8, sentinel), _out(len(mt), np.uint8, sentinel), _out((len(k1), 3), np.float32, sentinel, bytewise=True),
               _out(len(k1), np.uint8, sentinel))
        keep += [k1, k2, mt, sets]
        outs.append(out)
        P[i].n_keys1, P[i].n_keys2, P[i].n_matches = len(k1), len(k2), int(q.get("n_matches", len(mt)))
        P[i].iterations = int(q.get("iterations", len(sets)))
        P[i].keys1, P[i].keys2, P[i].matches, P[i].sets = (a.ctypes.data if a.size else None for a in (k1, k2, mt, sets))
        P[i].sigma, P[i].min_parallax = float(np.float32(q.get("sigma", 1.0))), float(np.float32(q.get("min_parallax", 1.0)))
        P[i].min_triangulated = int(q.get("min_triangulated", 50))
        _set_K(P[i], q["K"])
        if sentinel is not None:
            C.memset(C.byref(R[i]), sentinel, C.sizeof(_InitResult))
        R[i].inliers_h, R[i].inliers_f, R[i].P3D, R[i].triangulated = (a.ctypes.data for a in out)
        for name in q.get("null", ()):   # (tests: a missing array)
            setattr(R[i] if name in ("inliers_h", "inliers_f", "P3D", "triangulated") else P[i], name, None)
    return P, R, keep, outs


def _init_results(R, outs):
    res = []
    for i, (ih, jf, p3d, tri) in enumerate(outs):
        d = {k: getattr(R[i], k) for k in _INIT_SCALARS}
        d.update({k: np.array(getattr(R[i], k), t).reshape((3, 3) if k in ("H21", "F21", "R21") else -1) for k, t in _INIT_ARRAYS})
        d["SH"], d["SF"] = np.float32(d["SH"]), np.float32(d["SF"])
        d.update(inliers_h=ih, inliers_f=jf, P3D=p3d, triangulated=tri)
        res.append(d)
    return res


def debug_initializer_host(problems, sentinel=None):
    """aos2_debug_initializer_host: the routines of the device kernels on the CPU -> one dict per problem (aos2_initializer_result_t).
    `sentinel` pre-fills the result buffers; they stay in debug_initializer_host.last (result structs, result arrays, the structs' bytes
    before the call) for a caller that expects an error"""
    P, R, keep, outs = _init_args(problems, sentinel)
    debug_initializer_host.last = (R, outs, [bytes(R[i]) for i in range(len(problems))])
    _check(lib().aos2_debug_initializer_host(P, R, len(problems)))
    return _init_results(R, outs)


def debug_initializer_svd(A):
    """aos2_debug_initializer_svd: cv::SVDecomp of a float matrix as csrc/initializer.h runs it -> (left [n1][m], w [n], right [n][n])"""
    A = np.ascontiguousarray(A, np.float32)
    rows, cols = A.shape
    wide = rows < cols
    n, m = (rows, cols) if wide else (cols, rows)
    left, w, right = np.zeros((cols if wide else n, m), np.float32), np.zeros(n, np.float32), np.zeros((n, n), np.float32)
    _check(lib().aos2_debug_initializer_svd(_p(A), rows, cols, _p(left), _p(w), _p(right)))
    return left, w, right


def debug_initializer_rng(n):
    """the first n values of cv::RNG(0x12345678).next() as csrc/initializer.h generates them"""
    out = np.zeros(n, np.uint32)
    _check(lib().aos2_debug_initializer_rng(int(n), _p(out)))
    return out


def debug_initializer_inv33(S):
    """cv::Mat::inv() and cv::determinant of a float 3x3 -> (inverse, determinant)"""
    S, inv, det = np.ascontiguousarray(S, np.float32), np.zeros((3, 3), np.float32), C.c_double()
    _check(lib().aos2_debug_initializer_inv33(_p(S), _p(inv), C.byref(det)))
    return inv, det.value
