"""ORBmatcher and the Frame members over SoA snapshots, and the device forms of the geometric solvers that run on a matcher handle
(include/aos2.h: aos2_matcher_*, aos2_frame_*, aos2_sim3_ransac, aos2_pnp_ransac, aos2_initializer_initialize, aos2_triangulate_matches)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (MATCHER_THRESHOLDS, _BowFrames, _BowKfPair, _BowPair, _FrameView, _ProjLast, _ProjMp, _ProjPoints, _TriangPair)
from ._core import _Handle, _check, _p, lib
from .solvers import _init_args, _init_results, _pnp_args, _pnp_results, _sim3_args, _sim3_results, _triang_args


_DTYPES = dict(desc_kf=np.uint8, desc_f=np.uint8, kf_has_mp=np.uint8, angle_kf=np.float32, angle_f=np.float32,
               node_id_kf=np.int32, node_off_kf=np.int32, node_idx_kf=np.int32, node_id_f=np.int32,
               node_off_f=np.int32, node_idx_f=np.int32, kp_x=np.float32, kp_y=np.float32, kp_octave=np.int32,
               kp_angle=np.float32, u_right=np.float32, scale_factors=np.float32, grid_off=np.int32,
               grid_idx=np.int32, f_mp_state=np.uint8, track_in_view=np.uint8, pred_level=np.int32,
               view_cos=np.float32, proj_x=np.float32, proj_y=np.float32, proj_xr=np.float32, desc=np.uint8,
               has_obs=np.uint8, last_valid=np.uint8, world_pos=np.float32, last_octave=np.int32,
               last_angle=np.float32, desc1=np.uint8, desc2=np.uint8, has_mp1=np.uint8, has_mp2=np.uint8,
               angle1=np.float32, angle2=np.float32, node_id1=np.int32, node_off1=np.int32, node_idx1=np.int32,
               node_id2=np.int32, node_off2=np.int32, node_idx2=np.int32, x1=np.float32, y1=np.float32, x2=np.float32,
               y2=np.float32, u_right1=np.float32, u_right2=np.float32, octave2=np.int32, scale_factors2=np.float32,
               level_sigma2_2=np.float32, valid=np.uint8, pos=np.float32, max_dist=np.float32, min_dist=np.float32,
               normal=np.float32, q_angle=np.float32, inv_level_sigma2=np.float32)


def _fill_struct(st, d, keep):
    for name, ct in st._fields_:
        if name not in d:
            continue
        v = d[name]
        if ct is C.c_void_p:
            a = np.ascontiguousarray(v, _DTYPES[name])
            keep.append(a)
            setattr(st, name, a.ctypes.data)
        elif isinstance(v, np.ndarray) and hasattr(ct, "_length_"):
            setattr(st, name, ct(*[float(x) for x in v.reshape(-1)]))
        else:
            setattr(st, name, v.item() if hasattr(v, "item") else v)
    return st


class Matcher(_Handle):
    """Mirror of ORBmatcher (include/ORBmatcher.h:37-102) over SoA snapshots."""
    TH_LOW, TH_HIGH, HISTO_LENGTH = MATCHER_THRESHOLDS

    KIND = "matcher"

    def __init__(self, nnratio=0.6, check_orientation=True, device=0):
        self._create(float(nnratio), int(bool(check_orientation)), device)

    def last_device_ms(self):
        return float(self.L.aos2_matcher_last_device_ms(self.h))

    @staticmethod
    def DescriptorDistance(a, b):
        a = np.ascontiguousarray(a, np.uint8)
        b = np.ascontiguousarray(b, np.uint8)
        return lib().aos2_descriptor_distance(_p(a), _p(b))

    def hamming_best2(self, q, t):
        q = np.ascontiguousarray(q, np.uint8)
        t = np.ascontiguousarray(t, np.uint8)
        bi = np.zeros(len(q), np.int32)
        bd = np.zeros(len(q), np.int32)
        sd = np.zeros(len(q), np.int32)
        _check(self.L.aos2_matcher_hamming_best2(self.h, _p(q), len(q), _p(t), len(t), _p(bi), _p(bd), _p(sd)))
        return bi, bd, sd

    def hamming_best2_device(self, d_q, nq, d_t, nt, d_bi, d_bd, d_sd, iters=1):
        ms = C.c_float(0)
        _check(self.L.aos2_matcher_hamming_best2_device(self.h, C.c_void_p(d_q), nq, C.c_void_p(d_t), nt,
                                                        C.c_void_p(d_bi), C.c_void_p(d_bd), C.c_void_p(d_sd),
                                                        iters, C.byref(ms)))
        return ms.value

    def SearchByBoW(self, problems):
        """problems: list of synth_bow_problem()-style dicts (or one dict). Returns [(nmatches, match_f)]."""
        single = isinstance(problems, dict)
        if single:
            problems = [problems]
        keep = []
        arr = (_BowPair * len(problems))()
        outs = []
        for i, p in enumerate(problems):
            d = dict(p)
            d["n_kf"], d["n_f"] = len(p["desc_kf"]), len(p["desc_f"])
            d["n_nodes_kf"], d["n_nodes_f"] = len(p["node_id_kf"]), len(p["node_id_f"])
            _fill_struct(arr[i], d, keep)
            outs.append(np.zeros(max(d["n_f"], 1), np.int32))
        ptrs = (C.c_void_p * len(problems))(*[o.ctypes.data for o in outs])
        nm = np.zeros(len(problems), np.int32)
        _check(self.L.aos2_matcher_search_by_bow(self.h, C.byref(arr), len(problems), ptrs, _p(nm)))
        res = [(int(nm[i]), outs[i][: len(problems[i]["desc_f"])]) for i in range(len(problems))]
        return res[0] if single else res

    def SearchByBoWDevice(self, pairs):
        """aos2_matcher_search_by_bow_device: pairs = list of dicts with DEVICE addresses (ints) desc_kf, desc_f, angle_kf,
        angle_f, sizes n_kf / n_f, and host arrays kf_has_mp, node_id_* / node_off_* / node_idx_* -> [(nmatches, match_f)]"""
        keep = []
        n = len(pairs)
        arr = (_BowPair * n)()
        outs = []
        for i, p in enumerate(pairs):
            a = arr[i]
            a.n_kf, a.n_f = int(p["n_kf"]), int(p["n_f"])
            a.desc_kf, a.desc_f, a.angle_kf, a.angle_f = int(p["desc_kf"]), int(p["desc_f"]), int(p["angle_kf"]), int(p["angle_f"])
            a.n_nodes_kf, a.n_nodes_f = len(p["node_id_kf"]), len(p["node_id_f"])
            for name in ("kf_has_mp", "node_id_kf", "node_off_kf", "node_idx_kf", "node_id_f", "node_off_f", "node_idx_f"):
                v = np.ascontiguousarray(p[name], _DTYPES[name])
                if v.size == 0:
                    v = np.zeros(1, _DTYPES[name])
                keep.append(v)
                setattr(a, name, v.ctypes.data)
            outs.append(np.zeros(max(a.n_f, 1), np.int32))
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nm = np.zeros(n, np.int32)
        _check(self.L.aos2_matcher_search_by_bow_device(self.h, C.byref(arr), n, ptrs, _p(nm)))
        return [(int(nm[i]), outs[i][: int(pairs[i]["n_f"])]) for i in range(n)]

    def SearchByBoWFrames(self, n_frames, cap, kf_has_mp, match_f, nmatches, **dev):
        """aos2_matcher_search_by_bow_frames: dev = the device addresses (ints) named like aos2_bow_frames_t's fields;
        kf_has_mp uint8 [n][cap], match_f int32 [n][cap], nmatches int32 [n]: host arrays (filled in place)"""
        q = _BowFrames()
        q.n_frames, q.cap = int(n_frames), int(cap)
        for k, v in dev.items():
            setattr(q, k, int(v))
        q.kf_has_mp = kf_has_mp.ctypes.data
        _check(self.L.aos2_matcher_search_by_bow_frames(self.h, C.byref(q), _p(match_f), _p(nmatches)))

    def _kfkf(self, struct_t, fn, problems, *extra):
        single = isinstance(problems, dict)
        if single:
            problems = [problems]
        keep = []
        arr = (struct_t * len(problems))()
        outs = []
        for i, p in enumerate(problems):
            d = dict(p)
            d["n1"], d["n2"] = len(p["desc1"]), len(p["desc2"])
            d["n_nodes1"], d["n_nodes2"] = len(p["node_id1"]), len(p["node_id2"])
            if "scale_factors2" in p:
                d["n_levels2"] = len(p["scale_factors2"])
            _fill_struct(arr[i], d, keep)
            outs.append(np.zeros(max(d["n1"], 1), np.int32))
        ptrs = (C.c_void_p * len(problems))(*[o.ctypes.data for o in outs])
        nm = np.zeros(len(problems), np.int32)
        _check(fn(self.h, C.byref(arr), len(problems), *extra, ptrs, _p(nm)))
        res = [(int(nm[i]), outs[i][: len(problems[i]["desc1"])]) for i in range(len(problems))]
        return res[0] if single else res

    def SearchByBoWKF(self, problems):
        """SearchByBoW(pKF1, pKF2, vpMatches12) src/ORBmatcher.cc:522-655; synth_bow_kf_problem()-style dicts.
        Returns (nmatches, match12) per problem."""
        return self._kfkf(_BowKfPair, self.L.aos2_matcher_search_by_bow_kf, problems)

    def SearchForTriangulation(self, problems, only_stereo=False):
        """src/ORBmatcher.cc:657-823; synth_triang_problem()-style dicts. Returns (nmatches, vMatches12)."""
        return self._kfkf(_TriangPair, self.L.aos2_matcher_search_for_triangulation, problems, int(only_stereo))

    def ComputeDistinctiveDescriptors(self, off, desc):
        """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:275-340) for a CSR batch of map points."""
        off = np.ascontiguousarray(off, np.int32)
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(off) - 1
        best = np.zeros(max(n, 1), np.int32)
        _check(self.L.aos2_compute_distinctive_descriptors(self.h, n, _p(off), _p(desc), _p(best)))
        return best[:n]

    def SearchByProjection(self, f, mp, th=3.0):
        keep = []
        fv = _fill_struct(_FrameView(), f, keep)
        pm = _fill_struct(_ProjMp(), mp, keep)
        match = np.zeros(max(f["n_f"], 1), np.int32)
        n = np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection(self.h, C.byref(fv), C.byref(pm), float(th), _p(match), _p(n)))
        return int(n[0]), match[: f["n_f"]]

    def SearchByProjectionBatch(self, frames, mps, th=3.0):
        """n independent SearchByProjection(F, vpMapPoints, th) problems in one launch -> [(nmatches, match_f)]"""
        keep = []
        n = len(frames)
        fa, pa = (_FrameView * n)(), (_ProjMp * n)()
        outs = []
        for i in range(n):
            _fill_struct(fa[i], frames[i], keep)
            _fill_struct(pa[i], mps[i], keep)
            outs.append(np.zeros(max(frames[i]["n_f"], 1), np.int32))
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        nm = np.zeros(n, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_batch(self.h, C.byref(fa), C.byref(pa), n, float(th), ptrs, _p(nm)))
        return [(int(nm[i]), outs[i][: frames[i]["n_f"]]) for i in range(n)]

    def SearchByProjectionLast(self, cur, last, th, mono):
        keep = []
        fv = _fill_struct(_FrameView(), cur, keep)
        pl = _fill_struct(_ProjLast(), last, keep)
        match = np.zeros(max(cur["n_f"], 1), np.int32)
        n = np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_last(self.h, C.byref(fv), C.byref(pl), float(th), int(mono),
                                                             _p(match), _p(n)))
        return int(n[0]), match[: cur["n_f"]]


    # ---- projection family; f / p: synth_proj_gen_problem()-style dicts
    def InitializerInitialize(self, problems, sentinel=None):
        """aos2_initializer_initialize: Initializer::Initialize (src/Initializer.cc) for a batch of monocular sequences; problems as
        debug_initializer_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.init_last for a caller
        that expects an error and wants to see them untouched)"""
        P, R, keep, outs = _init_args(problems, sentinel)
        self.init_last = (R, outs, [bytes(R[i]) for i in range(len(problems))])
        _check(self.L.aos2_initializer_initialize(self.h, P, R, len(problems)))
        return _init_results(R, outs)

    def PnpRansac(self, problems, sentinel=None, with_counts=True):
        """aos2_pnp_ransac: the RANSAC of PnPsolver (src/PnPsolver.cc) for a batch of relocalisation candidates; problems as
        debug_pnp_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.pnp_last for a caller that
        expects a refusal)"""
        P, R, keep, outs = _pnp_args(problems, sentinel, with_counts)
        self.pnp_last = (R, outs)
        _check(self.L.aos2_pnp_ransac(self.h, P, R, len(problems)))
        return _pnp_results(R, outs)

    def Fuse(self, kf, p, sim3=False):
        """search part of Fuse (src/ORBmatcher.cc:825-975, sim3: :977-1100) -> (nFused, best_idx, best_dist)"""
        keep = []
        fv = _fill_struct(_FrameView(), kf, keep)
        pp = _fill_struct(_ProjPoints(), p, keep)
        bi, bd = np.zeros(max(p["n_pts"], 1), np.int32), np.zeros(max(p["n_pts"], 1), np.int32)
        n = np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_fuse(self.h, C.byref(fv), C.byref(pp), int(sim3), _p(bi), _p(bd), _p(n)))
        return int(n[0]), bi[: p["n_pts"]], bd[: p["n_pts"]]

    def SearchByProjectionKF(self, kf, p):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) :290-403 -> (nmatches, match_f)"""
        keep = []
        fv = _fill_struct(_FrameView(), kf, keep)
        pp = _fill_struct(_ProjPoints(), p, keep)
        match, n = np.zeros(max(kf["n_f"], 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_kf(self.h, C.byref(fv), C.byref(pp), _p(match), _p(n)))
        return int(n[0]), match[: kf["n_f"]]

    def SearchBySim3(self, kf1, kf2, p12, p21):
        """SearchBySim3 :1102-1326 -> (nFound, match12)"""
        keep = []
        a, b = _fill_struct(_FrameView(), kf1, keep), _fill_struct(_FrameView(), kf2, keep)
        c, d = _fill_struct(_ProjPoints(), p12, keep), _fill_struct(_ProjPoints(), p21, keep)
        match, n = np.zeros(max(p12["n_pts"], 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_sim3(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), _p(match), _p(n)))
        return int(n[0]), match[: p12["n_pts"]]

    def AssignFeaturesToGrid(self, kp_x, kp_y, min_x, min_y, grid_w_inv, grid_h_inv):
        """Frame::AssignFeaturesToGrid (src/Frame.cc:259-274) -> (grid_off[3073], grid_idx)"""
        kp_x, kp_y = np.ascontiguousarray(kp_x, np.float32), np.ascontiguousarray(kp_y, np.float32)
        off = np.zeros(64 * 48 + 1, np.int32)
        idx = np.zeros(max(len(kp_x), 1), np.int32)
        n = C.c_int32(0)
        _check(self.L.aos2_frame_assign_features_to_grid(self.h, len(kp_x), _p(kp_x), _p(kp_y), float(min_x), float(min_y),
                                                         float(grid_w_inv), float(grid_h_inv), _p(off), _p(idx), C.byref(n)))
        return off, idx[: n.value]

    def ComputeStereoFromRGBD(self, kp_x, kp_y, kpun_x, depth_img, mbf):
        """Frame::ComputeStereoFromRGBD (src/Frame.cc:672-693) -> (mvuRight, mvDepth)"""
        kp_x, kp_y, kpun_x = (np.ascontiguousarray(a, np.float32) for a in (kp_x, kp_y, kpun_x))
        depth_img = np.ascontiguousarray(depth_img, np.float32)
        ur, dp = np.zeros(max(len(kp_x), 1), np.float32), np.zeros(max(len(kp_x), 1), np.float32)
        _check(self.L.aos2_frame_stereo_from_rgbd(self.h, len(kp_x), _p(kp_x), _p(kp_y), _p(kpun_x), _p(depth_img),
                                                  depth_img.shape[1], depth_img.shape[0], depth_img.shape[1], float(mbf),
                                                  _p(ur), _p(dp)))
        return ur[: len(kp_x)], dp[: len(kp_x)]

    def isInFrustum(self, frame, p, viewing_cos_limit=0.5):
        """Frame::isInFrustum (src/Frame.cc:298-354) for all points of p -> dict with the aos2_proj_mp_t arrays"""
        keep = []
        pp = _fill_struct(_ProjPoints(), p, keep)
        n = p["n_pts"]
        iv = np.zeros(max(n, 1), np.uint8)
        px, py, pr, vc = (np.zeros(max(n, 1), np.float32) for _ in range(4))
        lv = np.zeros(max(n, 1), np.int32)
        _check(self.L.aos2_frame_is_in_frustum(self.h, C.byref(pp), float(frame["min_x"]), float(frame["max_x"]),
                                               float(frame["min_y"]), float(frame["max_y"]), int(frame["n_levels"]),
                                               float(viewing_cos_limit), _p(iv), _p(px), _p(py), _p(pr), _p(lv), _p(vc)))
        return dict(track_in_view=iv[:n], proj_x=px[:n], proj_y=py[:n], proj_xr=pr[:n], pred_level=lv[:n], view_cos=vc[:n])

    def SearchForInitialization(self, f2, q, window_size=100):
        """SearchForInitialization :405-520; q = dict(desc1, octave1, angle1, prev_xy) -> (nmatches, vnMatches12)"""
        keep = []
        fv = _fill_struct(_FrameView(), f2, keep)
        d1 = np.ascontiguousarray(q["desc1"], np.uint8)
        o1 = np.ascontiguousarray(q["octave1"], np.int32)
        a1 = np.ascontiguousarray(q["angle1"], np.float32)
        pv = np.ascontiguousarray(q["prev_xy"], np.float32)
        match, n = np.zeros(max(len(d1), 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_for_initialization(self.h, C.byref(fv), len(d1), _p(d1), _p(o1), _p(a1), _p(pv),
                                                             int(window_size), _p(match), _p(n)))
        return int(n[0]), match[: len(d1)]

    def SearchByProjectionReloc(self, frame, p, orb_dist=100):
        """SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) :1472-1599 -> (nmatches, match_f)"""
        keep = []
        fv = _fill_struct(_FrameView(), frame, keep)
        pp = _fill_struct(_ProjPoints(), p, keep)
        match, n = np.zeros(max(frame["n_f"], 1), np.int32), np.zeros(1, np.int32)
        _check(self.L.aos2_matcher_search_by_projection_reloc(self.h, C.byref(fv), C.byref(pp), int(orb_dist), _p(match), _p(n)))
        return int(n[0]), match[: frame["n_f"]]

    def TriangulateMatches(self, kf1, kf2, obs1, obs2):
        """aos2_triangulate_matches: the loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) for the matches of
        ONE (KF1, KF2) pair; arguments as debug_triangulate_host -> (status uint8 [n], x3D float32 [n][3])"""
        g, n, obs1, obs2, x3D, status = _triang_args(kf1, kf2, obs1, obs2)
        _check(self.L.aos2_triangulate_matches(self.h, C.byref(g), n, _p(obs1), _p(obs2), _p(x3D), _p(status)))
        return status, x3D

    def Sim3Ransac(self, problems, sentinel=None):
        """aos2_sim3_ransac: the RANSAC of Sim3Solver (src/Sim3Solver.cc) for a batch of loop candidates; problems as debug_sim3_host
        -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.sim3_last for a caller that expects a refusal)"""
        P, R, keep, outs = _sim3_args(problems, sentinel)
        self.sim3_last = (R, outs)
        _check(self.L.aos2_sim3_ransac(self.h, P, R, len(problems)))
        return _sim3_results(R, outs)
