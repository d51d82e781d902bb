"""The landmark half of one Levenberg-Marquardt trial of LocalBundleAdjustment and the decision that follows it, written from the g2o
operation -- the reference of tests/test_lba_trial_gpu.py (the tap aos2_debug_lba_trial_device: k_points / k_points_walk with solve = 1,
lm_decide, k_lin with init = 0, k_transition, k_final alone), on top of tests/lba_system_ref.py (values with scales, the windows).

The operation (block_solver.hpp:455-480, sparse_optimizer.cpp:61-114 and 422-440, levenberg.cpp:99-164, sparse_optimizer.cpp:372-414),
from the estimates and masks the system was linearised at, lambda and the pose part x_p of the solution (the reduced solve has its own
test: x_p is an input here):
    B_il = J_pose^T (rho' w) J_l,   x_l = (Hll_l + lambda I)^-1 (b_l - sum_i B_il^T x_p,i)      free keyframes i that see landmark l
    X_l += x_l;   scale_l = sum_r x_l[r] (lambda x_l[r] + b_l[r])
    chi2_l = sum over the active edges of l of rho(w e.e) at the trial's estimates (Huber where the edge is robust; cam_project's float
             reciprocal in the stereo residual)
    tempChi = sum_l chi2_l,  scale = sum_l scale_l + sum_j x_p[j] (lambda x_p[j] + b_p[j]) + 1e-3,  rho = (currentChi - tempChi) / scale
Every quantity of the reference is (value, M) like in lba_system_ref: D^-1 carries |D^-1| + |D^-1| M_D |D^-1|, and
omega = |q_dev - q_ref| / (2^-53 M_q).  Two float64 models of the same operation set the tolerance: the textbook form (explicit blocks B,
insertion order) and the record form (B^T x_p = -R^T C E x_p from {x / z, y / z, 1 / z, +-w}, one reciprocal per edge).

canonical_sum restates the order in which the device adds the per-landmark values (a float64 operation: reproducible bit for bit), decide
restates the decision from g2o's text and returns the whole expected state.
"""
import math
import os
import sys

from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import lba_system_ref as S  # noqa: E402
from lba_system_ref import LD, U53, VM, DELTA, camera_points, linearise, make_window, mat3_inverse, residual  # noqa: E402

QUANTITIES = ("x_l", "scale_l", "chi2_l")
DBL_MAX = sys.float_info.max


# ------------------------------------------------------------------------------------------ per-edge chi2
def edge_chi2(win, est, dt=LD):
    """computeError + chi2 + the robust kernel of every edge at the estimates `est` (pose, point, e_level1, e_robust) ->
    dict: chi2, rho (triples value, m, f; rho = chi2 where the edge is not robust), depth, beyond, active"""
    stereo = np.asarray(win["edge_stereo"]).astype(np.uint8)
    _, p = camera_points(win, est, dt)
    e = residual(win, p, np.asarray(win["edge_obs"], np.float32), stereo, dt)
    w = VM(np.asarray(win["edge_inv_sigma2"], np.float32).astype(dt))
    chi2 = (e[0] * e[0] + e[1] * e[1] + e[2] * e[2]) * w
    delta = np.where(stereo == 1, DELTA[1], DELTA[0]).astype(dt)
    beyond = np.asarray(est["e_robust"]).astype(bool) & (chi2.v > delta * delta)
    sq = np.sqrt(np.where(beyond, chi2.v, 1))
    # beyond delta: rho = 2 sqrt(chi2) delta - delta^2; a relative error of chi2 is half that of its root (as in lba_system_ref.linearise)
    rel = np.where(beyond, chi2.f / np.where(beyond, chi2.v, 1), 0) / 2 + 1
    rho = tuple(np.where(beyond, a, b) for a, b in ((2 * sq * delta - delta * delta, chi2.v), (2 * np.sqrt(chi2.m) * delta + delta * delta, chi2.m),
                                                     (2 * sq * delta * (rel + 1) + np.abs(2 * sq * delta - delta * delta), chi2.f)))
    return dict(chi2=(chi2.v, chi2.m, chi2.f), rho=rho, depth=p[2].v, beyond=beyond, active=~np.asarray(est["e_level1"]).astype(bool))


def edge_chi2_records(win, est):
    """a second float64 model of an edge's chi2 (no robust kernel): one reciprocal per edge, a = x iz, b = y iz as the linearisation
    records hold them, and e.(w e) added term by term -> [E]"""
    f8 = np.float64
    fx, fy, cx, cy, bf = S.cam(win, f8)
    ep, el = np.asarray(win["edge_pose"]), np.asarray(win["edge_point"])
    pose, point = np.asarray(est["pose"], f8), np.asarray(est["point"], f8)
    p = np.einsum("eij,ej->ei", S.rot_from_quat(pose[:, :4])[ep], point[el]) + pose[ep, 4:7]
    st = np.asarray(win["edge_stereo"]).astype(bool)
    obs = np.asarray(win["edge_obs"], np.float32).astype(f8)
    w = np.asarray(win["edge_inv_sigma2"], np.float32).astype(f8)
    iz = 1.0 / p[:, 2]
    ivf = iz.astype(np.float32)   # (cam_project's float reciprocal and float product)
    izs = np.where(st, ivf.astype(f8), iz)
    u, v = p[:, 0] * izs * fx + cx, p[:, 1] * izs * fy + cy
    e0, e1 = obs[:, 0] - u, obs[:, 1] - v
    e2 = np.where(st, obs[:, 2] - (u - (np.float32(win["bf"]) * ivf).astype(f8)), 0.0)
    return e0 * (w * e0) + e1 * (w * e1) + e2 * (w * e2)


def chi2_terms(win, est, lh, n_l, dt=LD):
    """chi2_l per landmark (hidx) at `est`: active edges only, in insertion order -> (value, M), the per-edge dict"""
    ed = edge_chi2(win, est, dt)
    act = ed["active"]
    out = []
    for a in ed["rho"]:
        t = np.zeros(n_l, dt)
        np.add.at(t, lh[act], a[act])
        out.append(t)
    return (out[0], out[1] + out[2]), ed


# ------------------------------------------------------------------------------------------ back-substitution, update, scale terms
def lin_estimates(A):
    """the estimates the system of the trial was linearised at, from snapshot A (the reduced solve has updated the free keyframes and
    left their old values in the backup; the landmarks move in the landmark kernel): dict for lba_system_ref.linearise"""
    return dict(pose=A["bk_pose"].copy(), point=A["point"].copy(), e_level1=A["e_level1"], e_robust=A["e_robust"])


def backsub(lin, lam, x_p):
    """x_l and the landmarks' scale terms from a linearisation (lba_system_ref.linearise, any arithmetic), lambda and x_p [6 np] ->
    dict x_l [nl, 3], scale_l [nl] as (value, M) pairs, b_l"""
    dt = lin["dt"]
    lam = dt(lam)
    n_l = len(lin["hpoint"])
    free, ph, lh = lin["free"], lin["ph"], lin["lh"]
    xp = np.asarray(x_p, np.float64).astype(dt).reshape(-1, 6)[np.where(free, ph, 0)] * free.astype(dt)[:, None]   # [E, 6]
    Bv, Bm, Bf = lin["B"]   # [E, 6, 3]
    t = [np.einsum("erc,er->ec", Bv, xp), np.einsum("erc,er->ec", Bm, np.abs(xp)), np.einsum("erc,er->ec", Bf, np.abs(xp))]
    cl = []
    for k in range(3):
        s = np.zeros((n_l, 3), dt)
        np.add.at(s, lh[free], t[k][free])   # (in index order: the edges' insertion order)
        cl.append(lin["b_l"][k] - s if k == 0 else lin["b_l"][k] + s)
    I3 = np.eye(3, dtype=dt)
    Dinv = mat3_inverse(lin["Hll"][0] + lam * I3)
    aD = np.abs(Dinv)
    Dinv_m = aD + aD @ (lin["Hll"][1] + lin["Hll"][2] + lam * I3) @ aD   # (the conditioning of a nearly rank-2 landmark block)
    x = (np.einsum("lrc,lc->lr", Dinv, cl[0]), np.einsum("lrc,lc->lr", Dinv_m, cl[1]), np.einsum("lrc,lc->lr", aD, cl[2]))
    # what x_l's error becomes in the scale terms: its bound M_x = m + f enters as f
    X = VM(x[0], x[1], x[1] + x[2])
    b = VM(*lin["b_l"])
    term = X * (X * lam + b)
    sc = VM(term.v[:, 0], term.m[:, 0], term.f[:, 0]) + VM(term.v[:, 1], term.m[:, 1], term.f[:, 1]) + VM(term.v[:, 2], term.m[:, 2], term.f[:, 2])
    return dict(x_l=(x[0], x[1] + x[2]), scale_l=(sc.v, sc.m + sc.f), b_l=lin["b_l"][0])


def model_textbook(win, est_lin, lam, x_p):
    """float64 model (a): explicit blocks B, every operation in float64, edges in insertion order"""
    return backsub(linearise(win, est_lin, np.float64), lam, x_p)


def model_records(win, est_lin, lam, x_p):
    """float64 model (b): B^T x_p = -R^T C E x_p from the record {a = x iz, b = y iz, iz = 1 / z, W}: C = W iz Pt^T Pt, E x_p = (a, b, 1) x
    omega - iz upsilon; Hll and b_l as lba_system_ref.model_records assembles them; the sum over a landmark's free-keyframe edges by
    ascending keyframe"""
    f8 = np.float64
    lin = linearise(win, est_lin, f8)   # (index structure, masks)
    mdl = S.model_records(win, est_lin, lam)
    Hll, b_l = mdl["Hll"][0], mdl["b_l"][0]
    fx, fy, cx, cy, bf = S.cam(win, f8)
    ep, el = np.asarray(win["edge_pose"]), np.asarray(win["edge_point"])
    pose, point = est_lin["pose"].astype(f8), est_lin["point"].astype(f8)
    R = S.rot_from_quat(pose[:, :4])[ep]
    p = np.einsum("eij,ej->ei", R, point[el]) + pose[ep, 4:7]
    st = np.asarray(win["edge_stereo"]).astype(bool)
    free, ph, lh = lin["free"], lin["ph"], lin["lh"]
    iz = 1.0 / p[:, 2]
    a, b = p[:, 0] * iz, p[:, 1] * iz
    z0 = np.zeros(len(ep))
    Pt = np.moveaxis(np.array([[fx + z0, z0, -a * fx], [z0, fy + z0, -b * fy], [np.where(st, fx, 0), z0, np.where(st, bf * iz - a * fx, 0)]]), -1, 0)
    ed = edge_chi2(win, est_lin, f8)
    w = np.asarray(win["edge_inv_sigma2"], np.float32).astype(f8)
    W = np.where(ed["beyond"], np.where(st, DELTA[1], DELTA[0]) / np.sqrt(np.where(ed["beyond"], ed["chi2"][0], 1.0)), 1.0) * w * free
    C = (W * iz)[:, None, None] * np.einsum("eki,ekj->eij", Pt, Pt)
    xp = np.asarray(x_p, f8).reshape(-1, 6)[np.where(free, ph, 0)]
    om, up = xp[:, :3], xp[:, 3:]
    abl = np.stack([a, b, np.ones_like(a)], 1)
    t = np.cross(abl, om) - iz[:, None] * up
    v = -np.einsum("eji,ej->ei", R, np.einsum("eij,ej->ei", C, t))   # B^T x_p
    order = np.nonzero(free)[0]
    order = order[np.lexsort((ph[order], lh[order]))]
    cl = b_l.copy()
    np.subtract.at(cl, lh[order], v[order])
    Dinv = mat3_inverse(Hll + f8(lam) * np.eye(3))
    x = np.einsum("lrc,lc->lr", Dinv, cl)
    term = x * (f8(lam) * x + b_l)
    return dict(x_l=(x, None), scale_l=(term[:, 0] + term[:, 1] + term[:, 2], None), b_l=b_l)


# ------------------------------------------------------------------------------------------ the measure
def omega(got, pair):
    """worst omega of an array against a (value, M) pair -> (omega, index)"""
    g, v, m = np.asarray(got, LD), np.asarray(pair[0], LD), np.asarray(pair[1], LD)
    if g.size == 0:
        return 0.0, ()
    d = np.abs(g - v)
    om = np.where(d == 0, LD(0), d / (U53 * np.where(m > 0, m, LD("1e-4000"))))
    om = np.where(np.isfinite(d), om, LD(np.inf))   # (a NaN of the device is no agreement)
    k = np.unravel_index(int(np.argmax(om)), om.shape) if om.ndim else ()
    return float(om[k]), tuple(int(x) for x in k)


def model_omegas(win, est_lin, lam, x_p, est_trial, ref=None):
    """-> (worst omega of the two float64 models per quantity, per model, the reference: x_l, scale_l, chi2_l and the per-edge dict)"""
    ref = full_reference(win, est_lin, lam, x_p, est_trial) if ref is None else ref
    lin = ref["lin"]
    per = {}
    for name, f in (("textbook", model_textbook), ("records", model_records)):
        mdl = f(win, est_lin, lam, x_p)
        chi, _ = chi2_terms(win, est_trial, lin["lh"], len(lin["hpoint"]), np.float64)
        per[name] = dict(x_l=omega(mdl["x_l"][0], ref["x_l"])[0], scale_l=omega(mdl["scale_l"][0], ref["scale_l"])[0],
                         chi2_l=omega(chi[0], ref["chi2_l"])[0])
    return {q: max(per[n][q] for n in per) for q in QUANTITIES}, per, ref


def full_reference(win, est_lin, lam, x_p, est_trial):
    lin = linearise(win, est_lin, LD)
    ref = backsub(lin, lam, x_p)
    ref["lin"] = lin
    ref["chi2_l"], ref["edges"] = chi2_terms(win, est_trial, lin["lh"], len(lin["hpoint"]), LD)
    return ref


# ------------------------------------------------------------------------------------------ the sums of a trial
def canonical_sum(values, tail_terms=()):
    """canonical_sums of lba.hip in float64: value i goes to lane i % 128, a lane adds its values in ascending i, then (the scale) the
    pose terms tail_terms[t], tail_terms[t + 128], ...; a tree adds the lanes with h = 64 ... 1"""
    lanes = np.zeros(128)
    for arr in (np.asarray(values, np.float64).ravel(), np.asarray(tail_terms, np.float64).ravel()):
        pad = np.zeros((len(arr) + 127) // 128 * 128)
        pad[:len(arr)] = arr
        for row in pad.reshape(-1, 128):
            lanes = lanes + row
    h = 64
    while h > 0:
        lanes[:h] = lanes[:h] + lanes[h:2 * h]
        h >>= 1
    return float(lanes[0])


# ------------------------------------------------------------------------------------------ the decision
STATE_KEYS = ("lam", "ni", "currentChi", "iniChi", "final_chi2", "final_lambda", "phase", "run", "lin", "initp", "xmark", "it", "qmax", "nBad",
              "iters_done", "trials", "polls", "stop_poll", "n_active", "solver_failed", "err_at", "ntr")


# The relative distance allowed between two lambdas whose good-step factor came from pow() implementations of 1 ulp each: the cubes
# (below 1: an ulp is at most 2^-53) differ by at most 2 ulp = 2^-52; alpha = 1 - cube >= 1/3 takes that as a relative 3 x 2^-52, its own
# rounding adds 2^-53 on either side, and so does the product with lambda: 6 x 2^-53 + 4 x 2^-53, first order
LAMBDA_POW_BOUND = 10 * 2.0 ** -53


def decide(state, tempChi, scale, ok, flag_seen, iters_max=(5, 10), stop_at_poll=0):
    """The end of one pass of the do-while of OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:123-149), what
    follows it when the loop ends (:151-163), the loop condition of SparseOptimizer::optimize (sparse_optimizer.cpp:376) and, when the
    first optimize() returns, Optimizer.cc:663-667 -- on the state record the device keeps (LmState of lba_window.h: the members of the g2o
    objects plus where the program stands).  state: the record before (snapshot A); tempChi = activeRobustChi2() at the trial's
    estimates; scale = computeScale() (the 1e-3 is added here); ok = the linear solve succeeded; flag_seen = *pbStopFlag.
    -> the record after (plus `pow_used`, see below), and `restored` (pop() ran).  The traces get one more entry (the device records rho = -1 for a failed solve,
    where g2o's (currentChi - DBL_MAX) / scale is some negative number: same decisions)."""
    s = {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in state.items() if not k.startswith("tr_")}
    s["pow_used"] = False
    tr = {k: list(state[k]) for k in ("tr_rho", "tr_temp", "tr_cur", "tr_lambda")}
    opt = 0 if s["phase"] == 0 else 1   # which optimize() call runs

    def terminate():   # SparseOptimizer::terminate(): *_forceStopFlag, every evaluation counted
        s["polls"] += 1
        if s["stop_poll"] > 0:
            return True
        if flag_seen or (stop_at_poll > 0 and s["polls"] >= stop_at_poll):
            s["stop_poll"] = s["polls"]
            return True
        return False

    if not ok:   # :126-127
        tempChi = DBL_MAX
        s["solver_failed"] += 1
    rho = s["currentChi"] - tempChi   # :129
    scale = scale + 1e-3              # :131
    rho = rho / scale                 # :132
    if not ok:
        rho = -1.0
    tr["tr_rho"].append(rho); tr["tr_temp"].append(tempChi); tr["tr_cur"].append(s["currentChi"]); tr["tr_lambda"].append(s["lam"])
    s["ntr"] += 1
    accepted = rho > 0 and math.isfinite(tempChi)   # :134
    if accepted:
        # pow((2*rho-1), 3).  What pow returns is the cube to within the accuracy of the C library that g2o is linked with (glibc
        # documents 1 ulp; it differs from the correctly rounded cube for 0.08 % of the arguments), so this one operation of the
        # decision is not reproducible bit for bit: the cube rounded once is taken here, exact through rationals, and `pow_used` says
        # whether it reaches lambda -- not where alpha is cropped to 1/3 or 2/3 (LAMBDA_POW_BOUND)
        cube = float(Fraction(2 * rho - 1) ** 3) if math.isfinite(rho) and abs(rho) < 1e100 else math.pow(2 * rho - 1, 3)
        alpha = 1. - cube
        s["pow_used"] = 1. / 3. < alpha < 2. / 3.
        alpha = min(alpha, 2. / 3.)
        scaleFactor = max(1. / 3., alpha)
        s["lam"] *= scaleFactor
        s["ni"] = 2.0
        s["currentChi"] = tempChi
        s["err_at"] = 1   # discardTop(): the estimates are the trial's, and so are the edges' errors
    else:
        s["lam"] *= s["ni"]
        s["ni"] *= 2
        s["err_at"] = 2   # pop(): the estimates are the old ones, the edges' errors are still the trial's
    s["qmax"] += 1        # :148
    s["trials"][opt] += 1
    s["lin"] = 0
    if rho < 0 and s["qmax"] < 10 and not terminate():   # :149, evaluated left to right
        return dict(s, **tr, iters_done=tuple(s["iters_done"]), trials=tuple(s["trials"])), not accepted
    result_ok = True
    if s["qmax"] == 10 or rho == 0:   # :151-152
        result_ok = False
    else:                             # :155-161
        if (s["iniChi"] - s["currentChi"]) * 1e3 < s["iniChi"]:
            s["nBad"] += 1
        else:
            s["nBad"] = 0
        if s["nBad"] >= 3:
            result_ok = False
    s["it"] += 1                      # sparse_optimizer.cpp:376: i++, then i < iterations && !terminate() && ok
    if s["it"] < iters_max[opt] and not terminate() and result_ok:
        s["qmax"] = 0                     # levenberg.cpp:101
        s["iniChi"] = s["currentChi"]     # :82-85 (the errors at the estimates that stand are the accepted trial's, or unchanged)
        s["lin"] = 1 if accepted else 0   # buildSystem() at unchanged estimates re-forms the same system
    else:
        s["run"] = 0
        s["iters_done"][opt] = s["it"]
        s["final_chi2"], s["final_lambda"] = s["currentChi"], s["lam"]
        if opt == 0:                      # Optimizer.cc:663-667: bDoMore = !*pbStopFlag
            s["phase"], s["xmark"] = 1, 0
            if terminate():
                s["phase"] = 3
            else:
                s["xmark"] = 1
                s["n_active"] = 0         # (counted anew by the outlier pass)
        else:
            s["phase"] = 3
    return dict(s, **tr, iters_done=tuple(s["iters_done"]), trials=tuple(s["trials"])), not accepted


def transition_state(state, n_active, iters_max=(5, 10), stop_at_poll=0):
    """the state record behind the outlier pass (Optimizer.cc:669-708): initializeOptimization(0) finds n_active level-0 edges (none:
    optimize() returns at once), optimize(iters_max[1]) evaluates its loop condition for the first time"""
    s = {k: v for k, v in state.items() if not k.startswith("tr_")}
    if not s["xmark"]:
        return s
    s.update(xmark=0, it=0, err_at=0, n_active=int(n_active))
    stop = False
    if n_active > 0 and iters_max[1] > 0:
        s["polls"] += 1
        stop = s["stop_poll"] > 0 or (stop_at_poll > 0 and s["polls"] >= stop_at_poll)
        if stop and s["stop_poll"] == 0:
            s["stop_poll"] = s["polls"]
    if n_active == 0 or iters_max[1] <= 0 or stop:
        s["phase"] = 3
        s["iters_done"] = (s["iters_done"][0], 0)
    else:
        s["phase"], s["initp"] = 2, 1
    return s


# ------------------------------------------------------------------------------------------ the tail
def pose_matrix(pose, dt=LD):
    """SE3Quat::to_homogeneous_matrix: [n, 7] -> [n, 4, 4] in dt"""
    pose = np.asarray(pose, np.float64).astype(dt)
    T = np.zeros((len(pose), 4, 4), dt)
    T[:, :3, :3] = S.rot_from_quat(pose[:, :4])
    T[:, :3, 3] = pose[:, 4:7]
    T[:, 3, 3] = 1
    return T


THRESHOLD = (5.991, 7.815)   # mono, stereo (Optimizer.cc:681, 697, 724, 739)


# ------------------------------------------------------------------------------------------ a float64 trial (case selection, CPU test)
def se3_exp_apply(upd, pose):
    """VertexSE3Expmap::oplusImpl: exp(upd) * pose, float64 (SE3Quat::exp, se3quat.h:223-257) -> qx qy qz qw tx ty tz"""
    om, up = np.asarray(upd[:3], np.float64), np.asarray(upd[3:], np.float64)
    th = np.linalg.norm(om)
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    Om2 = Om @ Om
    if th < 1e-5:
        R = np.eye(3) + Om + Om2
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * Om2
        V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Om + (th - np.sin(th)) / th ** 3 * Om2
    R0 = S.rot_from_quat(np.asarray(pose[None, :4], np.float64))[0]
    Rn, tn = R @ R0, R @ pose[4:7] + V @ up
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rn, tn
    m = Rn
    tr = m[0, 0] + m[1, 1] + m[2, 2]   # (Eigen's matrix -> quaternion, in float64: S.qt_from_Tcw rounds its input to float32)
    if tr > 0:
        s = np.sqrt(tr + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        q = [(m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s, w]
    else:
        i = int(np.argmax(np.diag(m)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q = [0.0] * 4
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    q = np.array(q)
    return np.concatenate([q / np.linalg.norm(q), tn])


def model_trial(win, est, lam=None, lam_factor=None):
    """One whole trial in float64 from the estimates `est`: lba_system_ref's reduced system, numpy.linalg.solve for x_p, the textbook
    back-substitution, the update, the residual pass -> dict: est_lin, est_trial, lam, x_p, tempChi, currentChi, scale, rho, b_p"""
    lin = linearise(win, est, np.float64)
    lam = float(lin["lambda"][0]) * (1.0 if lam_factor is None else lam_factor) if lam is None else lam
    red = S.reduce(lin, lam)
    x_p = np.linalg.solve(red["Hs"][0], red["bs"][0])
    bs = backsub(lin, lam, x_p)
    x_l = bs["x_l"][0]
    pose, point = est["pose"].copy(), est["point"].copy()
    for i, k in enumerate(lin["hpose"]):
        pose[k] = se3_exp_apply(x_p[6 * i:6 * i + 6], pose[k])
    point[lin["hpoint"]] += x_l
    trial = dict(pose=pose, point=point, e_level1=est["e_level1"], e_robust=est["e_robust"])
    n_l = len(lin["hpoint"])
    chi, _ = chi2_terms(win, trial, lin["lh"], n_l, np.float64)
    b_p = lin["b_p"][0].ravel()
    scale = float(bs["scale_l"][0].sum() + (x_p * (lam * x_p + b_p)).sum()) + 1e-3
    cur = float(lin["chi2"][0])
    temp = float(chi[0].sum())
    return dict(est_lin=est, est_trial=trial, lam=lam, x_p=x_p, tempChi=temp, currentChi=cur, scale=scale, rho=(cur - temp) / scale, lin=lin)


# ------------------------------------------------------------------------------------------ the windows
NL = (1, 31, 32, 33, 127, 128, 129)        # kLmBlock = 32, the walk's workgroup of 128 and a lane's second value in canonical_sums
NL_BIG = (2047, 2048, 2049)                # the second round of canonical_sums' 16-deep loop (128 lanes x 16 values)
FREE_DEGREES = (0, 1, 3, 4, 5, 8, 9, 17)   # around kWalkChunk = 4 and kLmSlots = 8
TOTAL_DEGREES = (1, 5, 6, 7, 12, 13)       # around kWalkChunkE = 6
GENTLE = dict(huber_split=False, noise=0.5, perturb=0.03, depths=(3.0, 40.0))   # an optimisation that accepts its steps
_cache = {}


def sees_nl(n):
    """n landmarks seen by two free keyframes and one of two fixed ones"""
    return [[0, 1, 2 + l % 2] for l in range(n)]


def sees_nl_big(n):
    """n landmarks of degree 2: a free and a fixed keyframe each"""
    return [[l % 2, 2 + (l // 2) % 2] for l in range(n)]


def window_degree():
    """18 free + 6 fixed keyframes: the landmarks of make_lba_walk_bits.sees_degrees (total degrees 1 .. 13 with free-keyframe degrees 0, 1,
    4, 5, 8, 9) and landmarks with 3 and 17 free keyframes; a landmark that is seen once is mono.  -> (window, (total, free) per landmark)"""
    import make_lba_walk_bits as WB
    n_free, n_fixed = 18, 6
    sees, pairs = WB.sees_degrees(n_free, n_fixed)
    rng = np.random.default_rng(21)
    extra = []
    for f, d in ((3, 3), (3, 5), (3, 7), (17, 17), (17, 18), (17, 23)):
        ks = sorted(int(k) for k in rng.choice(n_free, f, replace=False)) + sorted(n_free + int(k) for k in rng.choice(n_fixed, d - f, replace=False))
        extra.append(ks)
    sees = extra + sees
    deg = [(len(ks), sum(k < n_free for k in ks)) for ks in sees]
    mono = [l for l, (d, _) in enumerate(deg) if d == 1]
    win = make_window(2101, n_free, n_fixed, sees, kinds="stereo", mono_only=mono, **GENTLE)
    return WB.shuffled(win, 2102)[0], deg


def tail_window(seed):
    """The structure of lba_system_ref.stage1_window (6 free + 3 fixed keyframes, 150 landmarks, planted gross outliers) with residuals of
    2 standard deviations -- chi2 on both sides of the thresholds 5.991 / 7.815 after the first optimisation -- plus one landmark that
    two fixed keyframes see at its exact projection and that lies BEHIND one of them: flagged by its depth alone.
    -> (window, planted edges, the edge behind its keyframe)"""
    rng = np.random.default_rng(seed)
    n_free, n_fixed = 6, 3
    sees = []
    for l in range(150):
        ks = sorted(int(k) for k in rng.choice(5, int(rng.integers(3, 6)), replace=False))
        if l % 2 == 0:
            ks.append(n_free + l % n_fixed)
        sees.append(ks)
    for l in (7, 31, 64, 90):   # keyframe 5: four observations
        sees[l] = sorted(set(sees[l]) | {5})
    ep = np.array([k for ks in sees for k in ks])
    deg = np.array([len(ks) for ks in sees])
    el = np.array([l for l, ks in enumerate(sees) for _ in ks])
    planted = np.nonzero((rng.uniform(size=len(ep)) < 0.03) & (deg[el] >= 5))[0]
    win = dict(make_window(seed, n_free, n_fixed, sees, huber_split=False, noise=2.0, perturb=0.03, outliers=planted, depths=(3.0, 40.0)))
    T = np.asarray(win["pose_Tcw"], np.float32).astype(np.float64).reshape(-1, 4, 4)
    fixed = np.nonzero(win["pose_fixed"])[0]
    cz = np.array([-(T[k, :3, :3].T @ T[k, :3, 3])[2] for k in fixed])
    near, far = fixed[int(np.argmax(cz))], fixed[int(np.argmin(cz))]   # (camera centres along z: `near` is ahead of `far`)
    cn, cf = (-(T[k, :3, :3].T @ T[k, :3, 3]) for k in (near, far))
    assert cn[2] - cf[2] > 1.0
    X = (0.5 * (cn + cf)).astype(np.float32)   # between the two centres: in front of `far`, behind `near`
    fx, fy, cx, cy = (float(np.float32(win[k])) for k in ("fx", "fy", "cx", "cy"))
    obs = []
    for k in (far, near):
        p = T[k, :3, :3] @ X.astype(np.float64) + T[k, :3, 3]
        obs.append([fx * p[0] / p[2] + cx, fy * p[1] / p[2] + cy, -1.0])
    assert (T[far, :3, :3] @ X + T[far, :3, 3])[2] > 0.3 and (T[near, :3, :3] @ X + T[near, :3, 3])[2] < -0.3
    E = win["n_edges"]
    win.update(n_points=win["n_points"] + 1, n_edges=E + 2, point_xyz=np.vstack([win["point_xyz"], X[None]]).astype(np.float32),
               point_id=np.r_[win["point_id"], win["point_id"].max() + 1], edge_pose=np.r_[win["edge_pose"], far, near].astype(np.int32),
               edge_point=np.r_[win["edge_point"], win["n_points"], win["n_points"]].astype(np.int32),
               edge_obs=np.vstack([win["edge_obs"], np.array(obs)]).astype(np.float32), edge_stereo=np.r_[win["edge_stereo"], 0, 0].astype(np.uint8),
               edge_inv_sigma2=np.r_[win["edge_inv_sigma2"], 1.0, 1.0].astype(np.float32))
    return win, planted, E + 1


def window_all_leave():
    """every observation a gross outlier: the outlier pass leaves no edge"""
    sees = sees_nl(40)
    n_e = sum(len(k) for k in sees)
    return make_window(2301, 2, 2, sees, outliers=np.arange(n_e), **GENTLE)


def cases(family):
    """-> list of dicts: name, win, lam_factor (None: lambda_init); the call's arguments come with the family (CALL)"""
    if family in _cache:
        return _cache[family]
    c = lambda name, win, **kw: dict(dict(name=name, win=win, lam_factor=None, family=family), **kw)
    if family == "nl":
        out = [c("nl%d" % n, make_window(2000 + n, 2, 2, sees_nl(n), **GENTLE)) for n in NL]
        out += [c("nl%d" % n, make_window(2000 + n, 2, 2, sees_nl_big(n), kinds="stereo", **GENTLE)) for n in NL_BIG]
    elif family == "degree":
        win, deg = window_degree()
        out = [c("degree x%g" % f, win, lam_factor=f, degrees=deg) for f in S.LAMBDA_FACTORS]
    elif family == "sizes":
        out = [c(b["name"], b["win"]) for b in S.cases("sizes") if b["name"] in ("np1", "np8", "np40", "np41")]
    elif family == "big":
        import make_lba_walk_bits as WB
        out = [c("big", WB.window_big()), c("small", WB.window_one())]
    elif family == "kinds":
        out = [c(b["name"], b["win"]) for b in S.cases("kinds")]
    elif family == "stage1":
        out = [c(b["name"], b["win"], planted=b["planted"]) for b in S.cases("stage1")]
    elif family == "tail":
        out = []
        for seed in (2501, 2502):
            win, planted, behind = tail_window(seed)
            out.append(c("tail_%d" % seed, win, planted=planted, behind=behind))
    elif family == "nbad":
        out = [c("nl33 x1e9", cases("nl")[3]["win"], lam_factor=1e9)]
    elif family == "all_leave":
        out = [c("all_leave", window_all_leave())]
    else:
        raise KeyError(family)
    _cache[family] = out
    return out


FAMILIES = ("nl", "degree", "sizes", "big", "kinds", "stage1", "tail", "nbad", "all_leave")
# the arguments of the tap call of a family: the trial under test is the first one of the first optimisation, except
#   stage1: the first (and, with one iteration, last) trial of the second optimisation -- masked edges, no robust kernel;
#   tail:   the last trial of the first optimisation, then the outlier pass and the final check
CALL = dict(nl=dict(), degree=dict(), sizes=dict(), big=dict(), kinds=dict(), stage1=dict(trials_before=5, iters=(5, 1), tail=2),
            tail=dict(trials_before=4, tail=2), nbad=dict(trials_before=2), all_leave=dict(iters=(1, 10), tail=1))


TENTH_LAMBDA_FACTOR = 1e-24   # x lambda_init on window_rejecting: ten steps of the first iteration are rejected (rho = -0.57)


def window_rejecting(pkg):
    """make_lba_walk_bits' window `rejected_repeated`: far from the optimum; with 20 iterations its first optimisation rejects a step and
    repeats it, its second optimisation ends in an iteration of ten trials"""
    import make_lba_walk_bits as WB
    if "rejecting" not in _cache:
        _cache["rejecting"] = WB.window_hard(pkg, 43, 1.0, 6, 4)
    return _cache["rejecting"]


def window_rho_zero(pkg):
    """a window of the same kind whose good-step factors of the first optimisation lie inside (1/3, 2/3) and whose second optimisation
    ends at its fourth trial with tempChi == currentChi == 0 (rho == 0)"""
    import make_lba_walk_bits as WB
    if "rho_zero" not in _cache:
        _cache["rho_zero"] = WB.window_hard(pkg, 46, 1.0, 6, 4)
    return _cache["rho_zero"]
