"""Optimizer: LocalBundleAdjustment, GlobalBundleAdjustment, PoseOptimization, OptimizeSim3 and OptimizeEssentialGraph (include/aos2.h:
aos2_lba_*, aos2_global_bundle_adjustment, aos2_pose_optimization, aos2_optimize_sim3, aos2_optimize_essential_graph) and their taps."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import (AOS2_ERR_STOPPED, AOS2_OK, _LBA_SNAP_ARRAYS, _EssentialGraphProblem, _EssentialGraphResult, _GbaOptions, _GbaResult,
                   _LbaLmState, _LbaProblem, _LbaResult, _LbaSystem, _LbaTrial, _PoseProblem, _PoseResult, _Sim3OptProblem, _Sim3OptResult,
                   _Sim3OptSteps)
from ._build import _batch, _fill_lba_problem, _lba_camera_and_stop, _out, _set_K
from ._core import _Handle, _check, _p, lib


def _sim3_opt_args(problems, sentinel=None):
    """problems: dicts with X1c / X2c [n][3], obs1 / obs2 [n][2], inv_sigma2_1 / inv_sigma2_2 [n], K1 / K2 = (fx, fy, cx, cy),
    q12 (x, y, z, w), t12, s12 (float64), th2, fix_scale"""
    P, R, keep, outs = _batch(_Sim3OptProblem, _Sim3OptResult, len(problems))
    names = ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")
    for i, q in enumerate(problems):
        arr = [np.ascontiguousarray(q[k], np.float32) for k in names]
        n = len(arr[0])
        if [a.shape for a in arr] != [(n, 3), (n, 3), (n, 2), (n, 2), (n,), (n,)]:
            raise ValueError("problem %d: X [n][3], obs [n][2], inv_sigma2 [n]" % i)
        out = _out(n, np.uint8, sentinel)
        keep += arr
        outs.append(out)
        P[i].n = n
        for k, a in zip(names, arr):
            setattr(P[i], k, a.ctypes.data)
        _set_K(P[i], q["K1"], "1")
        _set_K(P[i], q["K2"], "2")
        P[i].q12 = (C.c_double * 4)(*[float(v) for v in q["q12"]])
        P[i].t12 = (C.c_double * 3)(*[float(v) for v in q["t12"]])
        P[i].s12, P[i].th2, P[i].fix_scale = float(q["s12"]), float(np.float32(q["th2"])), int(bool(q["fix_scale"]))
        R[i].outlier = out.ctypes.data
        if sentinel is not None:
            C.memset(C.byref(R[i]), sentinel, _Sim3OptResult.outlier.offset)
            R[i].n_bad = R[i].n_inliers = sentinel
    return P, R, keep, outs


def _sim3_opt_results(R, outs):
    return [dict(q12=np.array(R[i].q12, np.float64), t12=np.array(R[i].t12, np.float64), s12=np.float64(R[i].s12), outlier=out,
                 n_bad=R[i].n_bad, n_inliers=R[i].n_inliers, iterations=tuple(R[i].iterations), trials=tuple(R[i].trials))
            for i, out in enumerate(outs)]


def debug_sim3_opt_host(problems):
    """aos2_debug_sim3_opt_host: the routine of the device kernel on the CPU -> one dict per problem (the fields of aos2_sim3_opt_result_t)"""
    P, R, keep, outs = _sim3_opt_args(problems)
    _check(lib().aos2_debug_sim3_opt_host(P, R, len(problems)))
    return _sim3_opt_results(R, outs)


SIM3_OPT_STEPS_TAIL = 16   # elements the wrappers put behind act / chi / outlier


def _sim3_opt_steps_args(items, sentinel=0x5A, tail_byte=0xA5):
    """items: dicts with problem (as _sim3_opt_args takes it), S_lin / S_trial = (q, t, s), act_in [2n], chi_in [2n], outlier_in [n],
    remove, mask.  Every output buffer is filled with the byte `sentinel`; the SIM3_OPT_STEPS_TAIL elements behind the three planted
    arrays hold the byte `tail_byte` -> (the C items, what has to stay alive, the output arrays per item)"""
    I, keep, outs, tail = (_Sim3OptSteps * max(1, len(items)))(), [], [], SIM3_OPT_STEPS_TAIL
    for i, it in enumerate(items):
        P, _, arrays, _ = _sim3_opt_args([it["problem"]])
        n = P[0].n
        I[i].problem = P[0]
        for name in ("S_lin", "S_trial"):
            q, t, s = it[name]
            setattr(I[i], name, (C.c_double * 8)(*([float(v) for v in q] + [float(v) for v in t] + [float(s)])))
        planted = {}
        for name, count, dtype in (("act_in", 2 * n, np.uint8), ("chi_in", 2 * n, np.float64), ("outlier_in", n, np.uint8)):
            a = np.ascontiguousarray(it[name], dtype)
            if a.shape != (count,):
                raise ValueError("item %d: %s [%d]" % (i, name, count))
            full = np.empty(count + tail, dtype)
            full.view(np.uint8)[:] = tail_byte
            full[:count] = a
            planted[name] = full
            setattr(I[i], name, full.ctypes.data)
        I[i].tail, I[i].remove, I[i].mask = tail, int(bool(it["remove"])), int(it["mask"])
        out = {}
        for name, count, dtype in (("Hb", 36, np.float64), ("pert", 28 * 8, np.float64), ("chi_lin", 2 * n, np.float64), ("trial_sum", 1, np.float64),
                                   ("chi_trial", 2 * n, np.float64), ("flagged", 1, np.int32), ("chi", 2 * n + tail, np.float64),
                                   ("act", 2 * n + tail, np.uint8), ("outlier", n + tail, np.uint8)):
            out[name] = _out(count, dtype, sentinel, bytewise=True)
            setattr(I[i], name, out[name].ctypes.data)
        out["pert"] = out["pert"].reshape(28, 8)
        keep += [arrays, planted]
        outs.append(out)
    return I, keep, outs


def debug_sim3_opt_steps_host(items, sentinel=0x5A):
    """aos2_debug_sim3_opt_steps_host: linearise / trial / reject of the host tap's edges alone -> the output arrays per item"""
    I, keep, outs = _sim3_opt_steps_args(items, sentinel)
    _check(lib().aos2_debug_sim3_opt_steps_host(I, len(items)))
    return outs


def _essential_graph_args(problems, sentinel=None):
    """problems: dicts with Scw [n_vertices][8] (q (x, y, z, w), t, s; float64), fixed, v0 / v1 [n_edges], Sji [n_edges][8], fix_scale,
    iterations (20 when absent), Xw [n_points][3] (float32), ref [n_points].  A count may be forced apart from its arrays with
    n_vertices / n_edges / n_points, an array left out with None (what the argument checks are tried with).  `sentinel` pre-fills
    every result byte."""
    P, R, keep, outs = _batch(_EssentialGraphProblem, _EssentialGraphResult, len(problems))
    for i, q in enumerate(problems):
        def arr(k, dt, cols):
            if q.get(k) is None:
                return None
            a = np.ascontiguousarray(q[k], dt).reshape((-1, cols) if cols else (-1,))
            keep.append(a)
            return a
        Scw, Sji, v0, v1 = arr("Scw", np.float64, 8), arr("Sji", np.float64, 8), arr("v0", np.int32, 0), arr("v1", np.int32, 0)
        Xw, ref = arr("Xw", np.float32, 3), arr("ref", np.int32, 0)
        if v0 is not None and v1 is not None and Sji is not None and not len(v0) == len(v1) == len(Sji):
            raise ValueError("problem %d: v0, v1 [n_edges], Sji [n_edges][8]" % i)
        if Xw is not None and ref is not None and len(Xw) != len(ref):
            raise ValueError("problem %d: Xw [n_points][3], ref [n_points]" % i)
        P[i].n_vertices = int(q.get("n_vertices", 0 if Scw is None else len(Scw)))
        P[i].n_edges = int(q.get("n_edges", 0 if v0 is None else len(v0)))
        P[i].n_points = int(q.get("n_points", 0 if Xw is None else len(Xw)))
        P[i].fixed, P[i].fix_scale, P[i].iterations = int(q["fixed"]), int(bool(q["fix_scale"])), int(q.get("iterations", 20))
        for k, a in (("Scw", Scw), ("Sji", Sji), ("v0", v0), ("v1", v1), ("Xw", Xw), ("ref", ref)):
            setattr(P[i], k, a.ctypes.data if a is not None and a.size else None)
        nv, npt = max(P[i].n_vertices, 0), max(P[i].n_points, 0)
        out = dict(Scw=_out((nv, 8), np.float64, sentinel, bytewise=True), Tiw=_out((nv, 4, 4), np.float32, sentinel, bytewise=True),
                   Xw=_out((npt, 3), np.float32, sentinel, bytewise=True))
        outs.append(out)
        R[i].Scw, R[i].Tiw, R[i].Xw = out["Scw"].ctypes.data, out["Tiw"].ctypes.data, out["Xw"].ctypes.data
        if q.get("null_result"):
            setattr(R[i], q["null_result"], None)
        if sentinel is not None:
            off = _EssentialGraphResult.chi2_initial.offset
            C.memset(C.byref(R[i], off), sentinel, C.sizeof(_EssentialGraphResult) - off)
    return P, R, keep, outs


def _essential_graph_results(R, outs):
    return [dict(Scw=o["Scw"], Tiw=o["Tiw"], Xw=o["Xw"], chi2_initial=R[i].chi2_initial, chi2_final=R[i].chi2_final, iterations=R[i].iterations,
                 trials=R[i].trials, rejected=R[i].rejected, l_blocks=R[i].l_blocks, status=R[i].status) for i, o in enumerate(outs)]


def debug_essential_graph_host(problems, sentinel=None):
    """aos2_debug_essential_graph_host: the arithmetic of the device path on the CPU with a skyline solve -> one dict per problem (the
    fields of aos2_essential_graph_result_t)"""
    P, R, keep, outs = _essential_graph_args(problems, sentinel)
    debug_essential_graph_host.last = (R, outs)
    _check(lib().aos2_debug_essential_graph_host(P, R, len(problems)))
    return _essential_graph_results(R, outs)


def debug_essential_graph_arith_host(what, values):
    """aos2_debug_essential_graph_arith_host: "log" of Sim3s [n][8] -> [n][7]; "residual" of (C, S_v0, S_v1) [n][3][8] -> [n][7];
    "lu3" of (W, t) [n][12] -> [n][3]"""
    code, width, out_w = {"log": (0, 8, 7), "residual": (1, 24, 7), "lu3": (2, 12, 3)}[what]
    a = np.ascontiguousarray(values, np.float64).reshape(-1, width)
    out = np.zeros((len(a), out_w))
    _check(lib().aos2_debug_essential_graph_arith_host(code, _p(a), len(a), _p(out)))
    return out


GBA_HUBER = (float(np.float32(np.sqrt(5.99))), float(np.float32(np.sqrt(7.815))))       # Optimizer.cc:85-86
GBA_HUBER_LOCAL_BA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))   # Optimizer.cc:570-571: what the oracle uses
_GBA_SENTINEL_INT = -12345


def _gba_args(prob, iterations, robust, huber, stop_flag, sentinel=None):
    """the three structs of aos2_global_bundle_adjustment for a synth_lba_problem()-style dict; `sentinel` pre-fills the result"""
    keep = []
    s, o, r = _LbaProblem(), _GbaOptions(), _GbaResult()
    _fill_lba_problem(s, prob, keep, missing_is_null=True)   # (a test of the argument checks leaves an array out)
    _lba_camera_and_stop(s, prob, stop_flag, keep)
    o.iterations, o.robust, o.huber_mono, o.huber_stereo = int(iterations), int(bool(robust)), float(huber[0]), float(huber[1])
    Tout, Pout = _out((max(s.n_poses, 1), 16), np.float32, sentinel), _out((max(s.n_points, 1), 3), np.float32, sentinel)
    inc = _out(max(s.n_points, 1), np.uint8, None if sentinel is None else 77)
    r.pose_Tcw, r.point_xyz, r.point_included = Tout.ctypes.data, Pout.ctypes.data, inc.ctypes.data
    if sentinel is not None:
        r.iterations = r.trials = r.status = _GBA_SENTINEL_INT
    return s, o, r, keep, (Tout[: s.n_poses], Pout[: s.n_points], inc[: s.n_points])


def _gba_result(r, arrs):
    Tout, Pout, inc = arrs
    return dict(status=r.status, pose_Tcw=Tout, point_xyz=Pout, point_included=inc, iterations=r.iterations, trials=r.trials,
                chi2_initial=r.chi2_initial, chi2_final=r.chi2_final, final_lambda=r.final_lambda, polls=r.polls,
                stop_poll=r.stop_poll, h_blocks=r.h_blocks, l_blocks=r.l_blocks, ms_device=r.ms_device)


def debug_global_ba_host(prob, iterations=10, robust=False, huber=GBA_HUBER, stop_flag=None, stop_at_poll=0, sentinel=None):
    """aos2_debug_global_ba_host: the arithmetic and the lists of the device path run serially on the CPU with a skyline solve -> the
    fields of aos2_gba_result_t"""
    s, o, r, keep, arrs = _gba_args(prob, iterations, robust, huber, stop_flag, sentinel)
    debug_global_ba_host.last = (r, arrs)
    _check(lib().aos2_debug_global_ba_host(C.byref(s), C.byref(o), C.byref(r), int(stop_at_poll)))
    return _gba_result(r, arrs)


def lba_host_phase(probs, threads):
    """aos2_lba_debug_host_phase: (build ms, stage ms) of the host part of a LocalBA batch; needs no device"""
    n = len(probs)
    keep = []
    S = (_LbaProblem * n)()
    for i, prob in enumerate(probs):
        _fill_lba_problem(S[i], prob, keep)
    b, st = C.c_double(), C.c_double()
    _check(lib().aos2_lba_debug_host_phase(C.byref(S), n, int(threads), C.byref(b), C.byref(st)))
    return float(b.value), float(st.value)


class LocalBA(_Handle):
    """Optimizer::LocalBundleAdjustment numerical part (include/Optimizer.h:45, src/Optimizer.cc:454-779)."""

    KIND = "lba"

    def __init__(self, device=0):
        self._create(device)

    def _fill(self, s, r, prob, stop_flag, iters, keep):
        _fill_lba_problem(s, prob, keep)
        _lba_camera_and_stop(s, prob, stop_flag, keep)
        s.iters_first, s.iters_second = iters
        Tout = np.zeros((s.n_poses, 16), np.float32)
        Pout = np.zeros((s.n_points, 3), np.float32)
        outl = np.zeros(s.n_edges, np.uint8)
        chi2 = np.zeros(s.n_edges, np.float64)
        r.pose_Tcw, r.point_xyz, r.edge_outlier, r.edge_chi2 = Tout.ctypes.data, Pout.ctypes.data, outl.ctypes.data, chi2.ctypes.data
        return Tout, Pout, outl, chi2

    @staticmethod
    def _result(r, arrs):
        Tout, Pout, outl, chi2 = arrs
        return dict(status=r.status, pose_Tcw=Tout, point_xyz=Pout, edge_outlier=outl, edge_chi2=chi2,
                    iters=(r.iters_done_first, r.iters_done_second), trials=(r.trials_first, r.trials_second),
                    final_chi2=r.final_chi2, final_lambda=r.final_lambda, ms_device=r.ms_device,
                    polls=r.polls, stop_poll=r.stop_poll)

    def LocalBundleAdjustment(self, prob, stop_flag=None, iters=(5, 10)):
        keep = []
        s, r = _LbaProblem(), _LbaResult()
        arrs = self._fill(s, r, prob, stop_flag, iters, keep)
        _check(self.L.aos2_lba_solve(self.h, C.byref(s), C.byref(r)), ok=(AOS2_OK, AOS2_ERR_STOPPED))
        return self._result(r, arrs)

    def LocalBundleAdjustmentBatch(self, probs, stop_flags=None, iters=(5, 10)):
        """aos2_lba_solve_batch: independent windows in one call."""
        n = len(probs)
        keep = []
        S, R = (_LbaProblem * n)(), (_LbaResult * n)()
        arrs = [self._fill(S[i], R[i], probs[i], None if stop_flags is None else stop_flags[i], iters, keep) for i in range(n)]
        _check(self.L.aos2_lba_solve_batch(self.h, C.byref(S), C.byref(R), n))
        return [self._result(R[i], arrs[i]) for i in range(n)]

    def prepare_batch(self, probs, iters=(5, 10), want_chi2=False):
        """ctypes problem / result arrays for repeated aos2_lba_solve_batch calls on the same inputs (bench harness)"""
        n = len(probs)
        keep = []
        S, R = (_LbaProblem * n)(), (_LbaResult * n)()
        arrs = [self._fill(S[i], R[i], probs[i], None, iters, keep) for i in range(n)]
        if not want_chi2:
            for i in range(n):
                R[i].edge_chi2 = None
        return dict(S=S, R=R, arrs=arrs, keep=keep, n=n)

    def solve_prepared(self, prep):
        _check(self.L.aos2_lba_solve_batch(self.h, C.byref(prep["S"]), C.byref(prep["R"]), prep["n"]))
        return prep["R"]

    LAYOUTS = {"slots": 0, "walk": 1}

    def debug_assemble(self, probs, layout="slots", stage=0, lam=None, iters=(5, 10)):
        """test tap aos2_debug_lba_assemble_device: the reduced system of a trial as k_lin / k_lm_init / k_schur assemble it, for a batch
        of windows -> one dict per window (include/aos2.h: aos2_lba_system_t; Hs is npad x npad, Hpp_init np x 6 x 6, Hll nl x 3 x 3)"""
        n = len(probs)
        keep = []
        S, R, O = (_LbaProblem * n)(), (_LbaResult * n)(), (_LbaSystem * n)()
        bufs = []
        for i in range(n):
            self._fill(S[i], R[i], probs[i], None, iters, keep)
            q, m, E = S[i].n_poses, S[i].n_points, S[i].n_edges
            npad = (6 * q + 15) // 16 * 16
            b = dict(hpose=np.zeros(q, np.int32), hpoint=np.zeros(m, np.int32), blk_off=np.zeros(q * (q + 1) // 2 + 1, np.int32),
                     units=np.zeros(q + q * (q - 1) // 2 + 1, np.int32), pose=np.zeros((q, 7)), point=np.zeros((m, 3)),
                     e_level1=np.zeros(E, np.uint8), e_robust=np.zeros(E, np.uint8), Hpp_init=np.zeros(36 * q), b_init=np.zeros(6 * q),
                     b_p=np.zeros(6 * q), Hll=np.zeros(9 * m), b_l=np.zeros(3 * m), Hs=np.zeros(npad * npad), bs=np.zeros(6 * q))
            for k, a in b.items():
                setattr(O[i], k, a.ctypes.data)
            bufs.append(b)
        lam_a = None if lam is None else np.ascontiguousarray(lam, np.float64)
        assert lam_a is None or lam_a.shape == (n,)
        _check(self.L.aos2_debug_lba_assemble_device(self.h, C.byref(S), n, self.LAYOUTS.get(layout, layout), int(stage),
                                                     None if lam_a is None else _p(lam_a), C.byref(O)))
        out = []
        for o, b in zip(O, bufs):
            q, m, npad = o.np, o.nl, o.npad
            out.append(dict(np=q, nl=m, npad=npad, phase=o.phase, trials_first=o.trials_first, iters_done_first=o.iters_done_first,
                            lam=o.lam, current_chi=o.current_chi, hpose=b["hpose"][:q], hpoint=b["hpoint"][:m],
                            blk_off=b["blk_off"][:q * (q + 1) // 2 + 1], units=b["units"][:o.n_units], pose=b["pose"], point=b["point"],
                            e_level1=b["e_level1"], e_robust=b["e_robust"], Hpp_init=b["Hpp_init"][:36 * q].reshape(q, 6, 6),
                            b_init=b["b_init"][:6 * q], b_p=b["b_p"][:6 * q], Hll=b["Hll"][:9 * m].reshape(m, 3, 3), b_l=b["b_l"][:3 * m],
                            Hs=b["Hs"][:npad * npad].reshape(npad, npad), bs=b["bs"][:6 * q]))
        return out

    def debug_trial(self, probs, layout="slots", trials_before=0, lam=None, force_solver_failed=None, tail=0, iters=(5, 10)):
        """test tap aos2_debug_lba_trial_device: the landmark half of a trial, the LM decision, the outlier pass and the final check,
        read between the shipped launches -> one dict per window: np, nl, n_pl, n_part, hpose, hpoint, pt_off, pt_k, pl_pos and the
        snapshots "A" .. "E" (None where `tail` did not reach): dicts of the arrays of aos2_lba_trial_snap_t, pose [n_poses, 7], point
        [n_points, 3] and their backups bk_pose, bk_point, scal3, and st = the LmState scalars (traces cut to ntr)"""
        n = len(probs)
        keep = []
        S, R, O = (_LbaProblem * n)(), (_LbaResult * n)(), (_LbaTrial * n)()
        bufs = []
        for i in range(n):
            self._fill(S[i], R[i], probs[i], None, iters, keep)
            q, m, E = S[i].n_poses, S[i].n_points, S[i].n_edges
            b = dict(hpose=np.zeros(q, np.int32), hpoint=np.zeros(m, np.int32), pt_off=np.zeros(m + 1, np.int32), pt_k=np.zeros(E, np.int32),
                     pl_pos=np.zeros(E, np.int32))
            for k, a in b.items():
                setattr(O[i], k, a.ctypes.data)
            b["snap"] = []
            for j in range(5):
                sb = {k: np.zeros(size(q, m, E), dt) for k, dt, size in _LBA_SNAP_ARRAYS}
                for k, a in sb.items():
                    setattr(O[i].snap[j], k, a.ctypes.data)
                b["snap"].append(sb)
            bufs.append(b)
        lam_a = None if lam is None else np.ascontiguousarray(lam, np.float64)
        fail_a = None if force_solver_failed is None else np.ascontiguousarray(force_solver_failed, np.uint8)
        assert (lam_a is None or lam_a.shape == (n,)) and (fail_a is None or fail_a.shape == (n,))
        _check(self.L.aos2_debug_lba_trial_device(self.h, C.byref(S), n, self.LAYOUTS.get(layout, layout), int(trials_before),
                                                  None if lam_a is None else _p(lam_a), None if fail_a is None else _p(fail_a), int(tail),
                                                  C.byref(O)))
        out = []
        for i, (o, b) in enumerate(zip(O, bufs)):
            q, m, npl = o.np, o.nl, o.n_pl
            NP, NL = S[i].n_poses, S[i].n_points
            w = dict(np=q, nl=m, n_pl=npl, n_part=o.n_part, hpose=b["hpose"][:q], hpoint=b["hpoint"][:m], pt_off=b["pt_off"][:m + 1],
                     pt_k=b["pt_k"], pl_pos=b["pl_pos"])
            for j, name in enumerate("ABCDE"):
                sn, sb = o.snap[j], b["snap"][j]
                if not sn.taken:
                    w[name] = None
                    continue
                st = {k: getattr(sn.st, k) for k, _ in _LbaLmState._fields_ if not k.startswith("tr_") and k not in ("iters_done", "trials")}
                st["iters_done"], st["trials"] = tuple(sn.st.iters_done), tuple(sn.st.trials)
                for k in ("tr_rho", "tr_temp", "tr_cur", "tr_lambda"):
                    st[k] = np.array(getattr(sn.st, k)[:sn.st.ntr], np.float64)
                d = dict(sb, st=st, scal3=sn.scal3, pose=sb["est"][:7 * NP].reshape(NP, 7), point=sb["est"][7 * NP:].reshape(NL, 3),
                         bk_pose=sb["bk"][:7 * NP].reshape(NP, 7), bk_point=sb["bk"][7 * NP:].reshape(NL, 3))
                d.update(x=sb["x"][:6 * q + 3 * m], b=sb["b"][:6 * q + 3 * m], Hll=sb["Hll"][:9 * m].reshape(m, 3, 3), Rl=sb["Rl"][:9 * q].reshape(q, 3, 3),
                         tmp=sb["tmp"][:6 * q], part=sb["part"][:2 * m], lrec=sb["lrec"][:4 * npl].reshape(npl, 4), err=sb["err"].reshape(-1, 3),
                         out_Tcw=sb["out_Tcw"].reshape(NP, 16), out_xyz=sb["out_xyz"].reshape(NL, 3))
                w[name] = d
            out.append(w)
        return out

    def set_host_threads(self, n):
        _check(self.L.aos2_lba_set_host_threads(self.h, int(n)))

    def set_window_groups(self, n):
        """0 = default, 1 = one program for all windows of a batch, 2 = two staggered window groups (include/aos2.h)"""
        _check(self.L.aos2_lba_set_window_groups(self.h, int(n)))

    def last_program(self):
        """(trial slots enqueued for every window, host rounds) of the last solve"""
        a, b = C.c_int32(), C.c_int32()
        _check(self.L.aos2_lba_last_program(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def last_window_slots(self):
        """trial slots of the last solve summed over the windows each round covered (include/aos2.h)"""
        a = C.c_int64()
        _check(self.L.aos2_lba_last_window_slots(self.h, C.byref(a)))
        return int(a.value)

    def debug_stop_at_poll(self, poll):
        _check(self.L.aos2_lba_debug_stop_at_poll(self.h, int(poll)))

    def GlobalBundleAdjustment(self, prob, iterations=10, robust=False, huber=GBA_HUBER, stop_flag=None, sentinel=None):
        """aos2_global_bundle_adjustment: Optimizer::BundleAdjustment (src/Optimizer.cc:41-237) on a synth_lba_problem()-style dict.
        The defaults are LoopClosing::RunGlobalBundleAdjustment's; `sentinel` pre-fills the result (kept in self.global_ba_last for a
        caller that expects a refusal)"""
        s, o, r, keep, arrs = _gba_args(prob, iterations, robust, huber, stop_flag, sentinel)
        self.global_ba_last = (r, arrs)
        _check(self.L.aos2_global_bundle_adjustment(self.h, C.byref(s), C.byref(o), C.byref(r)))
        return _gba_result(r, arrs)

    def global_ba_profile(self, on):
        """aos2_debug_global_ba_profile: switch the per-family events on / off -> the family ms of the last profiled call (linearise +
        sums, landmarks + update, assemble, factor_solve, begin + trial_edges + decide, prepare + finish)"""
        ms = (C.c_float * 6)()
        _check(self.L.aos2_debug_global_ba_profile(self.h, int(bool(on)), ms))
        return [float(v) for v in ms]

    def debug_global_ba_solve(self, n_blocks, rows, cols, val, diag, b, lam, x0=None):
        """aos2_debug_global_ba_solve_device: the symbolic phase and k_gba_factor_solve alone (6x6 blocks) -> (x, ok, l_blocks); x0 =
        what x holds before (kept when the solve fails)"""
        rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        val = np.ascontiguousarray(val, np.float64).reshape(-1, 36)
        diag, b = np.ascontiguousarray(diag, np.float64).reshape(-1, 36), np.ascontiguousarray(b, np.float64).reshape(-1)
        if len(diag) != n_blocks or len(b) != 6 * n_blocks or not len(rows) == len(cols) == len(val):
            raise ValueError("diag [n_blocks][36], b [6 n_blocks], rows / cols / val one per triplet")
        x = np.zeros(6 * n_blocks) if x0 is None else np.array(x0, np.float64).reshape(6 * n_blocks)
        ok, lb = C.c_int32(-1), C.c_int32(-1)
        _check(self.L.aos2_debug_global_ba_solve_device(self.h, int(n_blocks), len(rows), _p(rows), _p(cols), _p(val), _p(diag), _p(b),
                                                        float(lam), _p(x), C.byref(ok), C.byref(lb)))
        return x, int(ok.value), int(lb.value)

    def debug_global_ba_reduced(self, prob, lam, n_free, robust=False, huber=GBA_HUBER):
        """aos2_debug_global_ba_reduced_device: the reduced camera system of the first linearisation at lambda = lam as the device
        assembles it -> (S [6 n_free][6 n_free] with lam on its diagonal, bs [6 n_free], h_blocks)"""
        s, o, r, keep, arrs = _gba_args(prob, 1, robust, huber, None)
        S, bs, hb = np.zeros((6 * n_free, 6 * n_free)), np.zeros(6 * n_free), C.c_int32(-1)
        _check(self.L.aos2_debug_global_ba_reduced_device(self.h, C.byref(s), C.byref(o), float(lam), int(n_free), _p(S), _p(bs), C.byref(hb)))
        return S, bs, int(hb.value)

    def PoseOptimization(self, problems):
        """int Optimizer::PoseOptimization(Frame*) (src/Optimizer.cc:239-452) for one dict or a list of
        synth_pose_problem()-style dicts (one workgroup per frame, one launch)."""
        single = isinstance(problems, dict)
        if single:
            problems = [problems]
        keep = []
        P = (_PoseProblem * len(problems))()
        R = (_PoseResult * len(problems))()
        outs = []
        for i, p in enumerate(problems):
            P[i].n = int(p["n"])
            for name, dt in (("Xw", np.float32), ("obs", np.float32), ("stereo", np.uint8), ("inv_sigma2", np.float32)):
                a = np.ascontiguousarray(p[name], dt)
                keep.append(a)
                setattr(P[i], name, a.ctypes.data)
            P[i].fx, P[i].fy, P[i].cx, P[i].cy, P[i].bf = (float(np.float32(p[k])) for k in ("fx", "fy", "cx", "cy", "bf"))
            P[i].Tcw = (C.c_float * 16)(*[float(x) for x in np.asarray(p["Tcw"], np.float32).reshape(-1)])
            o = np.zeros(max(P[i].n, 1), np.uint8)
            outs.append(o)
            R[i].outlier = o.ctypes.data
        _check(self.L.aos2_pose_optimization(self.h, C.byref(P), C.byref(R), len(problems)))
        res = [dict(n_inliers=R[i].n_inliers, n_bad=R[i].n_bad, outlier=outs[i][: P[i].n].copy(),
                    Tcw=np.array(list(R[i].Tcw), np.float32)) for i in range(len(problems))]
        return res[0] if single else res

    def pose_last_device_ms(self):
        return float(self.L.aos2_pose_optimization_last_device_ms(self.h))

    def OptimizeSim3(self, problems, sentinel=None):
        """aos2_optimize_sim3: Optimizer::OptimizeSim3 (src/Optimizer.cc:1047-1242) for a batch of loop candidates; problems as
        debug_sim3_opt_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in self.sim3_opt_last for a caller
        that expects a refusal)"""
        P, R, keep, outs = _sim3_opt_args(problems, sentinel)
        self.sim3_opt_last = (R, outs)
        _check(self.L.aos2_optimize_sim3(self.h, P, R, len(problems)))
        return _sim3_opt_results(R, outs)

    def debug_sim3_opt_steps(self, items, sentinel=0x5A):
        """aos2_debug_sim3_opt_steps_device: linearise / trial / reject of the device's edges alone; items and result as
        debug_sim3_opt_steps_host"""
        I, keep, outs = _sim3_opt_steps_args(items, sentinel)
        _check(self.L.aos2_debug_sim3_opt_steps_device(self.h, I, len(items)))
        return outs

    def sim3_opt_last_device_ms(self):
        return float(self.L.aos2_optimize_sim3_last_device_ms(self.h))

    def optimize_essential_graph(self, problems, sentinel=None):
        """aos2_optimize_essential_graph: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:782-1045) for a batch of pose graphs;
        problems as debug_essential_graph_host -> one dict per problem.  `sentinel` pre-fills the result buffers (kept in
        self.essential_graph_last for a caller that expects a refusal)"""
        P, R, keep, outs = _essential_graph_args(problems, sentinel)
        self.essential_graph_last = (R, outs)
        _check(self.L.aos2_optimize_essential_graph(self.h, P, R, len(problems)))
        return _essential_graph_results(R, outs)

    def essential_graph_last_device_ms(self):
        return float(self.L.aos2_optimize_essential_graph_last_device_ms(self.h))

    def essential_graph_profile(self, on):
        """aos2_debug_essential_graph_profile: switch the per-family events on / off -> the family ms of the last profiled call
        (perturb + linearise, assemble, factor_solve, begin + trial, finish)"""
        ms = (C.c_float * 5)()
        _check(self.L.aos2_debug_essential_graph_profile(self.h, int(bool(on)), ms))
        return [float(v) for v in ms]

    def debug_essential_graph_solve(self, n_blocks, rows, cols, val, diag, b, lam, x0=None):
        """aos2_debug_essential_graph_solve_device: the symbolic phase and k_eg_factor_solve alone -> (x, ok, l_blocks); x0 = what x
        holds before (kept when the solve fails)"""
        rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        val = np.ascontiguousarray(val, np.float64).reshape(-1, 49)
        diag, b = np.ascontiguousarray(diag, np.float64).reshape(-1, 49), np.ascontiguousarray(b, np.float64).reshape(-1)
        if len(diag) != n_blocks or len(b) != 7 * n_blocks or not len(rows) == len(cols) == len(val):
            raise ValueError("diag [n_blocks][49], b [7 n_blocks], rows / cols / val one per triplet")
        x = np.zeros(7 * n_blocks) if x0 is None else np.array(x0, np.float64).reshape(7 * n_blocks)
        ok, lb = C.c_int32(-1), C.c_int32(-1)
        _check(self.L.aos2_debug_essential_graph_solve_device(self.h, int(n_blocks), len(rows), _p(rows), _p(cols), _p(val), _p(diag), _p(b),
                                                              float(lam), _p(x), C.byref(ok), C.byref(lb)))
        return x, int(ok.value), int(lb.value)

    def debug_essential_graph_linearised(self, problem):
        """aos2_debug_essential_graph_linearised_device: the first linearisation of one problem as the device forms it -> dict(J
        [ne][2][7][7] (a fixed side keeps the bytes 0x5A), E [ne][7], H [7 nf][7 nf], b [7 nf], chi2, chi2_initial, l_blocks)"""
        P, R, keep, outs = _essential_graph_args([problem])
        ne, nf = max(int(P[0].n_edges), 0), max(int(P[0].n_vertices) - 1, 0)
        J, E = np.zeros((ne, 2, 7, 7)), np.zeros((ne, 7))
        H, b, chi = np.zeros((7 * nf, 7 * nf)), np.zeros(7 * nf), np.zeros(2)
        lb = C.c_int32(-1)
        _check(self.L.aos2_debug_essential_graph_linearised_device(self.h, P, _p(J), _p(E), _p(H), _p(b), _p(chi), C.byref(lb)))
        return dict(J=J, E=E, H=H, b=b, chi2=float(chi[0]), chi2_initial=float(chi[1]), l_blocks=int(lb.value))

    EG_CONTROL_D = ("lambda", "ni", "currentChi", "iniChi", "rho", "chi2_initial")
    EG_CONTROL_I = ("nBad", "qmax", "open", "running", "solved", "max_iterations", "iterations", "trials", "rejected", "accepted_first")

    def debug_essential_graph_trial(self, problem, x, lam, current_chi, ni=2.0, solved=1, iterations=0, qmax=0):
        """aos2_debug_essential_graph_trial_device: one k_eg_trial on one problem with the solver's vector x and the seeded control
        words -> dict(est_try, est [nv][8], control (the words of EG_CONTROL_D / EG_CONTROL_I by name), tempChi, scale)"""
        P, R, keep, outs = _essential_graph_args([problem])
        nv, nf = max(int(P[0].n_vertices), 0), max(int(P[0].n_vertices) - 1, 0)
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        if len(x) != 7 * nf:
            raise ValueError("x [7 (n_vertices - 1)]")
        seed_d, seed_i = np.array([lam, current_chi, ni], np.float64), np.array([solved, iterations, qmax], np.int32)
        est_try, est = np.zeros((nv, 8)), np.zeros((nv, 8))
        cd, ci, sums = np.zeros(6), np.zeros(10, np.int32), np.zeros(2)
        _check(self.L.aos2_debug_essential_graph_trial_device(self.h, P, _p(x), _p(seed_d), _p(seed_i), _p(est_try), _p(est), _p(cd), _p(ci), _p(sums)))
        control = dict(zip(self.EG_CONTROL_D, (float(v) for v in cd)))
        control.update(zip(self.EG_CONTROL_I, (int(v) for v in ci)))
        return dict(est_try=est_try, est=est, control=control, tempChi=float(sums[0]), scale=float(sums[1]))
