"""Optimizer::BundleAdjustment (reference src/Optimizer.cc:41-237) restated in numpy float64 for the tests of
aos2_global_bundle_adjustment: the numerical part (g2o's edges, quadratic forms, Schur complement and Levenberg-Marquardt control as
oracle/lba_oracle.c states them, with the reduced camera system DENSE and solved by numpy), the problem generator the tests share and
the rule results are compared under.

The oracle (oracle.lba_solve(prob, iters1=n, iters2=0)) already is BundleAdjustment for the robust form with LocalBA's Huber deltas:
it is the primary reference there, and this restatement is pinned to it under the same rule (tests/test_global_ba_cpu.py).  What the
oracle cannot express -- bRobust = false and thHuber2D = sqrt(5.99) -- is compared against this file.

Conventions that differ from the oracle on purpose:
  * terminate() is counted as the C call counts it: no entry check (the oracle's LocalBA has one in front, and one after optimize()).
  * the reduced system is solved by numpy.linalg.solve; "a zero or NaN pivot" becomes "singular or not finite".
Sums over edges / landmarks run in the oracle's order (np.add.at adds in index order); a product of small matrices is written out
term by term so that nothing is re-associated."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

HUBER_GBA = (float(np.float32(np.sqrt(5.99))), float(np.float32(np.sqrt(7.815))))        # Optimizer.cc:85-86
HUBER_LOCAL_BA = (float(np.float32(np.sqrt(5.991))), float(np.float32(np.sqrt(7.815))))  # Optimizer.cc:570-571, the oracle's
TOL = 1e-5                 # the project's pose / point tolerance
RESOLUTION_FACTOR = 4      # ... or this many times the reference's own spread on the problem
MAX_RESOLUTION = 1e-4      # a condition on the generator


# ------------------------------------------------------------------------------------------------- SE3 as g2o has it
def quat_from_rot(m):
    m = np.asarray(m, np.float64)
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def normalize_rot(q):
    q = -q if q[3] < 0 else q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def rot_from_quat(q):
    """q [..., 4] (x y z w) -> R [..., 3, 3], Eigen's toRotationMatrix"""
    q = np.asarray(q, np.float64)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty(q.shape[:-1] + (3, 3))
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - (tyy + tzz), txy - twz, txz + twy
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = txy + twz, 1 - (txx + tzz), tyz - twx
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = txz - twy, tyz + twx, 1 - (txx + tyy)
    return R


def quat_rotate(q, v):
    """Eigen's _transformVector, q [..., 4], v [..., 3]"""
    qv, w = q[..., :3], q[..., 3:4]
    uv = np.cross(qv, v)
    uv = uv + uv
    return v + w * uv + np.cross(qv, uv)


def se3_map(qt, X):
    return quat_rotate(qt[..., :4], X) + qt[..., 4:7]


def quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def se3_exp(upd):
    """SE3Quat::exp (se3quat.h:223-257), update = (omega, upsilon)"""
    omega, ups = np.asarray(upd[:3], np.float64), np.asarray(upd[3:], np.float64)
    theta = np.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = np.array([[0, -omega[2], omega[1]], [omega[2], 0, -omega[0]], [-omega[1], omega[0], 0]])
    Om2 = Om @ Om
    if theta < 0.00001:
        R = np.eye(3) + Om + Om2
        V = R
    else:
        a, b, c = np.sin(theta) / theta, (1 - np.cos(theta)) / (theta * theta), (theta - np.sin(theta)) / theta ** 3
        R = np.eye(3) + a * Om + b * Om2
        V = np.eye(3) + b * Om + c * Om2
    return np.concatenate([normalize_rot(quat_from_rot(R)), V @ ups])


def se3_mul(a, b):
    return np.concatenate([normalize_rot(quat_mul(a[:4], b[:4])), a[4:] + quat_rotate(a[:4], b[4:])])


def pose_from_Tcw(T16):
    """Converter::toSE3Quat: float32 4x4 -> (qx qy qz qw tx ty tz)"""
    T = np.asarray(T16, np.float32).reshape(4, 4).astype(np.float64)
    return np.concatenate([normalize_rot(quat_from_rot(T[:3, :3])), T[:3, 3]])


def pose_to_Tcw(qt):
    """Converter::toCvMat(SE3Quat) as float32 [16]"""
    T = np.zeros((4, 4), np.float32)
    T[:3, :3] = rot_from_quat(qt[:4]).astype(np.float32)
    T[:3, 3] = qt[4:].astype(np.float32)
    T[3, 3] = 1
    return T.reshape(16)


# ------------------------------------------------------------------------------------------------- the edges
class Cam:
    def __init__(self, prob):
        self.fx, self.fy, self.cx, self.cy, self.bf = (float(np.float32(prob[k])) for k in ("fx", "fy", "cx", "cy", "bf"))


def edge_error(cam, qt, X, obs, stereo):
    """Edge{,Stereo}SE3ProjectXYZ::computeError for E edges: qt [E, 7], X [E, 3], obs [E, 3] float64, stereo [E] bool -> [E, 3]"""
    p = se3_map(qt, X)
    er = np.zeros_like(p)
    with np.errstate(all="ignore"):
        u, v = p[:, 0] / p[:, 2], p[:, 1] / p[:, 2]
        mono0, mono1 = obs[:, 0] - (u * cam.fx + cam.cx), obs[:, 1] - (v * cam.fy + cam.cy)
        invz = (1.0 / p[:, 2]).astype(np.float32)                       # const float invz = 1.0f / trans_xyz[2]
        iz = invz.astype(np.float64)
        r0, r1 = p[:, 0] * iz * cam.fx + cam.cx, p[:, 1] * iz * cam.fy + cam.cy
        r2 = r0 - (np.float32(cam.bf) * invz).astype(np.float64)        # bf is a const float& there: a float product
    er[:, 0] = np.where(stereo, obs[:, 0] - r0, mono0)
    er[:, 1] = np.where(stereo, obs[:, 1] - r1, mono1)
    er[:, 2] = np.where(stereo, obs[:, 2] - r2, 0.0)
    return er


def edge_jacobians(cam, qt, X, stereo):
    """linearizeOplus: A = d e / d point [E, 3, 3], B = d e / d pose [E, 3, 6] (row d); the rows a monocular edge lacks are zero"""
    p, R = se3_map(qt, X), rot_from_quat(qt[:, :4])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    z_2, fx, fy, bf = z * z, cam.fx, cam.fy, cam.bf
    E = len(x)
    A, B = np.zeros((E, 3, 3)), np.zeros((E, 3, 6))
    s = -1. / z
    t02, t12 = -x / z * fx, -y / z * fy
    for c in range(3):
        m0 = (s * fx) * R[:, 0, c] + (s * 0) * R[:, 1, c] + (s * t02) * R[:, 2, c]
        m1 = (s * 0) * R[:, 0, c] + (s * fy) * R[:, 1, c] + (s * t12) * R[:, 2, c]
        s0 = -fx * R[:, 0, c] / z + fx * x * R[:, 2, c] / z_2
        s1 = -fy * R[:, 1, c] / z + fy * y * R[:, 2, c] / z_2
        A[:, 0, c] = np.where(stereo, s0, m0)
        A[:, 1, c] = np.where(stereo, s1, m1)
        A[:, 2, c] = np.where(stereo, s0 - bf * R[:, 2, c] / z_2, 0.0)
    B[:, 0, 0] = x * y / z_2 * fx
    B[:, 0, 1] = -(1 + (x * x / z_2)) * fx
    B[:, 0, 2] = y / z * fx
    B[:, 0, 3] = -1. / z * fx
    B[:, 0, 5] = x / z_2 * fx
    B[:, 1, 0] = (1 + y * y / z_2) * fy
    B[:, 1, 1] = -x * y / z_2 * fy
    B[:, 1, 2] = -x / z * fy
    B[:, 1, 4] = -1. / z * fy
    B[:, 1, 5] = y / z_2 * fy
    B[:, 2, 0] = np.where(stereo, B[:, 0, 0] - bf * y / z_2, 0.0)
    B[:, 2, 1] = np.where(stereo, B[:, 0, 1] + bf * x / z_2, 0.0)
    B[:, 2, 2] = np.where(stereo, B[:, 0, 2], 0.0)
    B[:, 2, 3] = np.where(stereo, B[:, 0, 3], 0.0)
    B[:, 2, 5] = np.where(stereo, B[:, 0, 5] - bf / z_2, 0.0)
    return A, B


def seq_sum(v):
    """the sum of v taken in index order (np.sum is pairwise)"""
    return float(np.cumsum(np.asarray(v, np.float64))[-1]) if len(v) else 0.0


def robustify(c, delta):
    """RobustKernelHuber for an array of chi2 -> rho, rho'"""
    dsqr = delta * delta
    with np.errstate(all="ignore"):
        sq = np.sqrt(c)
        return np.where(c <= dsqr, c, 2 * sq * delta - dsqr), np.where(c <= dsqr, 1.0, delta / sq)


# ------------------------------------------------------------------------------------------------- the graph
class Graph:
    """initializeOptimization on a synth_lba_problem()-style dict: the hessian indices and the loop orders of buildSystem / solve"""

    def __init__(self, prob, robust, huber):
        self.prob, self.cam, self.robust = prob, Cam(prob), bool(robust)
        self.ne = int(prob["n_edges"])
        self.ep = np.asarray(prob["edge_pose"], np.int64)
        self.el = np.asarray(prob["edge_point"], np.int64)
        self.obs = np.ascontiguousarray(prob["edge_obs"], np.float32).astype(np.float64).reshape(-1, 3)
        self.stereo = np.asarray(prob["edge_stereo"]).astype(bool)
        self.w = np.ascontiguousarray(prob["edge_inv_sigma2"], np.float32).astype(np.float64)
        self.delta = np.where(self.stereo, float(huber[1]), float(huber[0]))
        n_poses, n_points = int(prob["n_poses"]), int(prob["n_points"])
        pose_act, point_act = np.zeros(n_poses, bool), np.zeros(n_points, bool)
        pose_act[self.ep], point_act[self.el] = True, True
        free = np.flatnonzero(pose_act & (np.asarray(prob["pose_fixed"]) == 0))
        self.hpose = free[np.argsort(np.asarray(prob["pose_id"])[free], kind="stable")]
        act = np.flatnonzero(point_act)
        self.hpoint = act[np.argsort(np.asarray(prob["point_id"])[act], kind="stable")]
        self.np_, self.nl = len(self.hpose), len(self.hpoint)
        self.pose_hidx, self.point_hidx = np.full(n_poses, -1, np.int64), np.full(n_points, -1, np.int64)
        self.pose_hidx[self.hpose] = np.arange(self.np_)
        self.point_hidx[self.hpoint] = np.arange(self.nl)
        self.included = point_act
        self.ehp, self.ehl = self.pose_hidx[self.ep], self.point_hidx[self.el]
        # a landmark's column of Hpl: its edges with a free pose by (pose index, edge); the landmarks in hessian order
        fe = np.flatnonzero(self.ehp >= 0)
        self.pl = fe[np.lexsort((fe, self.ehp[fe], self.ehl[fe]))]
        # the pairs (a, b >= a) of a landmark's column, in solve_schur's order
        start = np.flatnonzero(np.r_[True, self.ehl[self.pl][1:] != self.ehl[self.pl][:-1]]) if len(self.pl) else np.zeros(0, np.int64)
        stop = np.r_[start[1:], len(self.pl)]
        pa, pb = [], []
        for s0, s1 in zip(start, stop):
            m = s1 - s0
            ia, ib = np.triu_indices(m)
            pa.append(self.pl[s0 + ia])
            pb.append(self.pl[s0 + ib])
        self.pair_a = np.concatenate(pa) if pa else np.zeros(0, np.int64)
        self.pair_b = np.concatenate(pb) if pb else np.zeros(0, np.int64)
        self.qt = np.stack([pose_from_Tcw(prob["pose_Tcw"][i]) for i in range(n_poses)]) if n_poses else np.zeros((0, 7))
        self.X = np.ascontiguousarray(prob["point_xyz"], np.float32).astype(np.float64).reshape(-1, 3)

    def h_blocks(self):
        i1, i2 = self.ehp[self.pair_a], self.ehp[self.pair_b]
        return len({(int(a), int(b)) for a, b in zip(i1, i2) if a != b})

    def errors(self, qt=None, X=None):
        qt, X = self.qt if qt is None else qt, self.X if X is None else X
        return edge_error(self.cam, qt[self.ep], X[self.el], self.obs, self.stereo)

    def chi2(self, er):
        """activeRobustChi2 and the per-edge (chi2, rho')"""
        c = (er[:, 0] * (self.w * er[:, 0]) + er[:, 1] * (self.w * er[:, 1])) + np.where(self.stereo, er[:, 2] * (self.w * er[:, 2]), 0.0)
        if not self.robust:
            return seq_sum(c), c, np.ones_like(c)
        rho, rho1 = robustify(c, self.delta)
        return seq_sum(rho), c, rho1

    def build(self):
        """buildSystem at the current estimates -> dict(Hpp [np, 6, 6], bp [np, 6], Hll [nl, 3, 3], bl [nl, 3], Hpl [E, 6, 3], chi,
        and the magnitudes of what was summed: aHpp, abp)"""
        er = self.errors()
        chi, _, rho1 = self.chi2(er)
        A, B = edge_jacobians(self.cam, self.qt[self.ep], self.X[self.el], self.stereo)
        om = -(self.w[:, None] * er)
        om[~self.stereo, 2] = 0.0
        wo = self.w.copy()
        if self.robust:
            wo = rho1 * self.w
            om = om * rho1[:, None]

        def quad(L, Rm):   # sum over d of L[d, r] * wo * R[d, c], d in order -> [E, r, c] and the sum of the magnitudes
            t = [(L[:, d, :, None] * wo[:, None, None]) * Rm[:, d, None, :] for d in range(3)]
            return (t[0] + t[1]) + t[2], (np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])

        def lin(L):        # sum over d of L[d, r] * om[d]
            t = [L[:, d, :] * om[:, d, None] for d in range(3)]
            return (t[0] + t[1]) + t[2], (np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])

        S = dict(chi=chi, er=er)
        f = self.ehp >= 0
        for name, (val, mag), idx, shape in (("Hpp", quad(B, B), self.ehp, (self.np_, 6, 6)), ("bp", lin(B), self.ehp, (self.np_, 6)),
                                            ("Hll", quad(A, A), self.ehl, (self.nl, 3, 3)), ("bl", lin(A), self.ehl, (self.nl, 3))):
            sel = f if name in ("Hpp", "bp") else np.ones(self.ne, bool)
            S[name], S["a" + name] = np.zeros(shape), np.zeros(shape)
            np.add.at(S[name], idx[sel], val[sel])
            np.add.at(S["a" + name], idx[sel], mag[sel])
        S["Hpl"] = quad(B, A)[0]
        S["Hpl"][~f] = 0.0
        return S

    def reduce(self, S, lam):
        """BlockSolver::solve up to the linear solve: the dense reduced system of H + lam I (both triangles, from the upper block
        triangle as the solver reads it), b_s, the 3x3 inverses, and for the bound of tests/test_global_ba_reduced_gpu.py the number
        and the summed magnitude of the terms of every entry"""
        n = self.np_
        Hll = S["Hll"].copy()
        Hll[:, [0, 1, 2], [0, 1, 2]] += lam
        m = Hll.reshape(-1, 9).T
        c00, c10, c20 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
        with np.errstate(all="ignore"):
            idet = 1.0 / (m[0] * c00 + m[1] * c10 + m[2] * c20)
        Dinv = np.stack([c00 * idet, (m[2] * m[7] - m[1] * m[8]) * idet, (m[1] * m[5] - m[2] * m[4]) * idet,
                         c10 * idet, (m[0] * m[8] - m[2] * m[6]) * idet, (m[2] * m[3] - m[0] * m[5]) * idet,
                         c20 * idet, (m[1] * m[6] - m[0] * m[7]) * idet, (m[0] * m[4] - m[1] * m[3]) * idet], 1).reshape(-1, 3, 3)
        bl = S["bl"]
        db = (Dinv[:, :, 0] * bl[:, None, 0] + Dinv[:, :, 1] * bl[:, None, 1]) + Dinv[:, :, 2] * bl[:, None, 2]
        Hpl = S["Hpl"]
        ea, eb = self.pair_a, self.pair_b
        Da = Dinv[self.ehl[ea]]
        Bi, Bj = Hpl[ea], Hpl[eb]
        BD = (Bi[:, :, 0, None] * Da[:, None, 0, :] + Bi[:, :, 1, None] * Da[:, None, 1, :]) + Bi[:, :, 2, None] * Da[:, None, 2, :]
        t = [BD[:, :, None, k] * Bj[:, None, :, k] for k in range(3)]
        T, aT = (t[0] + t[1]) + t[2], (np.abs(t[0]) + np.abs(t[1])) + np.abs(t[2])
        H4, a4, n4 = np.zeros((n, n, 6, 6)), np.zeros((n, n, 6, 6)), np.zeros((n, n, 6, 6))
        d = np.arange(n)
        H4[d, d] = S["Hpp"]
        H4[d[:, None], d[:, None], np.arange(6), np.arange(6)] += lam
        a4[d, d] = S["aHpp"] + abs(lam) * np.eye(6)
        cnt = np.zeros(n)
        np.add.at(cnt, self.ehp[self.ehp >= 0], 3.0)
        n4[d, d] = cnt[:, None, None] + np.eye(6)
        i1, i2 = self.ehp[ea], self.ehp[eb]
        np.subtract.at(H4, (i1, i2), T)
        np.add.at(a4, (i1, i2), aT)
        np.add.at(n4, (i1, i2), 9.0)
        dense = lambda M: M.transpose(0, 2, 1, 3).reshape(6 * n, 6 * n)   # noqa: E731
        sym = lambda M: np.triu(M) + np.triu(M, 1).T                      # noqa: E731
        pl = self.pl
        dbl = db[self.ehl[pl]]
        Bp = Hpl[pl]
        ct = [Bp[:, :, k] * dbl[:, None, k] for k in range(3)]
        coeff, acoeff = np.zeros((n, 6)), np.zeros((n, 6))
        np.add.at(coeff, self.ehp[pl], (ct[0] + ct[1]) + ct[2])
        np.add.at(acoeff, self.ehp[pl], (np.abs(ct[0]) + np.abs(ct[1])) + np.abs(ct[2]))
        nb = cnt.copy()
        np.add.at(nb, self.ehp[pl], 3.0)
        return dict(S=sym(dense(H4)), bs=(S["bp"] - coeff).reshape(-1), Dinv=Dinv, abs_S=sym(dense(a4)), n_S=sym(dense(n4)),
                    abs_bs=(S["abp"] + acoeff).reshape(-1), n_bs=np.repeat(nb, 6))

    def step(self, S, lam, x_prev):
        """BlockSolver::solve: (solved, x [6 np + 3 nl])"""
        n6 = 6 * self.np_
        Rd = self.reduce(S, lam)
        x = x_prev.copy()
        if n6:
            try:
                with np.errstate(all="ignore"):
                    xp = np.linalg.solve(Rd["S"], Rd["bs"])
            except np.linalg.LinAlgError:
                return False, x
            if not np.isfinite(xp).all():
                return False, x
            x[:n6] = xp
        pl = self.pl
        contrib = np.einsum("erc,er->ec", S["Hpl"][pl], -x[:n6].reshape(-1, 6)[self.ehp[pl]])
        cl = S["bl"].copy()
        np.add.at(cl, self.ehl[pl], contrib)
        Dinv = Rd["Dinv"]
        x[n6:] = ((Dinv[:, :, 0] * cl[:, None, 0] + Dinv[:, :, 1] * cl[:, None, 1]) + Dinv[:, :, 2] * cl[:, None, 2]).reshape(-1)
        return True, x

    def apply(self, x):
        n6 = 6 * self.np_
        for h, v in enumerate(self.hpose):
            self.qt[v] = se3_mul(se3_exp(x[6 * h: 6 * h + 6]), self.qt[v])
        self.X[self.hpoint] += x[n6:].reshape(-1, 3)


def solve(prob, iterations=10, robust=False, huber=HUBER_GBA, stop_at_poll=0):
    """initializeOptimization(); optimize(iterations) -> the fields of aos2_gba_result_t (pose_qt / point_xyz64 beside them)"""
    G = Graph(prob, robust, huber)
    polls = stop_poll = trials = its = 0

    def terminate():
        nonlocal polls, stop_poll
        polls += 1
        if stop_poll == 0 and stop_at_poll > 0 and polls >= stop_at_poll:
            stop_poll = polls
        return stop_poll > 0

    lam = ni = 0.0
    nBad = 0
    chi_initial = current = 0.0
    x = np.zeros(6 * G.np_ + 3 * G.nl)
    ok = True
    if G.ne > 0:
        for i in range(iterations):
            if terminate() or not ok:
                break
            S = G.build()
            current = ini = S["chi"]
            if i == 0:
                diag = np.r_[np.abs(S["Hpp"][:, range(6), range(6)]).reshape(-1), np.abs(S["Hll"][:, range(3), range(3)]).reshape(-1)]
                lam, ni, nBad, chi_initial = 1e-5 * float(diag.max()), 2.0, 0, current
            rho, qmax = 0.0, 0
            b = np.r_[S["bp"].reshape(-1), S["bl"].reshape(-1)]
            while True:
                trials += 1
                bk_qt, bk_X = G.qt.copy(), G.X.copy()
                solved, x = G.step(S, lam, x)
                G.apply(x)
                temp = G.chi2(G.errors())[0]
                if not solved:
                    temp = 1.7976931348623157e308
                rho = current - temp
                scale = seq_sum(x * (lam * x + b)) + 1e-3
                rho /= scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1. - (2 * rho - 1) ** 3, 2. / 3.)
                    lam *= max(1. / 3., alpha)
                    ni = 2.0
                    current = temp
                else:
                    lam *= ni
                    ni *= 2
                    G.qt, G.X = bk_qt, bk_X
                qmax += 1
                if not (rho < 0 and qmax < 10 and not terminate()):
                    break
            its += 1
            if qmax == 10 or rho == 0:
                ok = False
            else:
                nBad = nBad + 1 if (ini - current) * 1e3 < ini else 0
                ok = nBad < 3
    Tout = np.stack([pose_to_Tcw(G.qt[i]) for i in range(len(G.qt))]) if len(G.qt) else np.zeros((0, 16), np.float32)
    return dict(status=0, pose_Tcw=Tout, point_xyz=G.X.astype(np.float32), point_included=G.included.astype(np.uint8), pose_qt=G.qt,
                point_xyz64=G.X, iterations=its, trials=trials, chi2_initial=chi_initial, chi2_final=current, final_lambda=lam,
                polls=polls, stop_poll=stop_poll, h_blocks=G.h_blocks())


# ------------------------------------------------------------------------------------------------- the generator
# name: (keyframes (keyframe 0 is fixed), candidate points, stereo share, iterations, loop, window)
# window = w: a point keeps the observations within w / 2 keyframes of one of its observers, so that the reduced system is a band
# (synth_lba_problem's points are seen along the whole arc: 45 keyframes share a point pairwise, the system is full)
CASES = {
    "init": (2, 24, 0.0, 20, False, 0),     # Tracking::CreateInitialMapMonocular's shape: two keyframes, monocular, 20 iterations
    "pair": (3, 36, 1.0, 10, False, 0),
    "mixed": (12, 300, 0.5, 10, False, 0),
    "band": (45, 1200, 1.0, 10, False, 8),
    "loop": (45, 1200, 1.0, 10, True, 8),
    "past_lba": (160, 1500, 1.0, 10, False, 0),   # 159 free keyframes: just past LocalBundleAdjustment's 154
}
SEEDS = {"init": 1, "pair": 1, "mixed": 1, "band": 1, "loop": 1, "past_lba": 1}


def _true_poses(n_poses):
    """synth_lba_problem's trajectory: (Rwc, twc) of keyframe i"""
    out = []
    for i in range(n_poses):
        s = i / max(n_poses - 1, 1)
        ang = 0.6 * s
        out.append((np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]]),
                    np.array([40.0 * np.sin(ang) * 0.8, 0.05 * np.sin(7 * s), 40.0 * s * 0.8])))
    return out


def problem(name, seed=None, n_loop=12):
    """A map for GlobalBundleAdjustemnt: synth_lba_problem with only keyframe 0 fixed, plus one point without an edge, one point seen
    by keyframe 0 alone, with a window the band form, and, with loop, n_loop points seen by the first three and the last three keyframes (far ahead of the arc, so
    that all six see them in front; their projections may leave the image, which the optimiser does not know)."""
    K, n_points, stereo_frac, _, loop, window = CASES[name]
    seed = SEEDS[name] if seed is None else seed
    synth = graft.load_package().synth
    p = synth.synth_lba_problem(seed, n_local=K, n_fixed=0, n_points=n_points, include_kf0=True, stereo_frac=stereo_frac)
    rng = np.random.default_rng([seed, K, 0x6BA])
    if window:   # (keyframe = slot here; every point keeps the observations within window / 2 keyframes of one of its observers)
        ep, el = np.asarray(p["edge_pose"]), np.asarray(p["edge_point"])
        anchor = np.zeros(p["n_points"], np.int64)
        anchor[el] = ep                                    # the last observer ...
        pick = rng.random(len(ep)) < 0.3
        anchor[el[pick]] = ep[pick]                        # ... or another one
        keep = np.abs(ep - anchor[el]) <= window // 2
        p = dict(p)
        for k in ("edge_pose", "edge_point", "edge_obs", "edge_stereo", "edge_inv_sigma2"):
            p[k] = np.asarray(p[k])[keep]
        p["n_edges"] = int(keep.sum())
    poses = _true_poses(K)
    fx, fy, cx, cy, bf = (p[k] for k in ("fx", "fy", "cx", "cy", "bf"))
    xyz, pid = [p["point_xyz"]], list(p["point_id"])
    e = {k: list(p[k]) for k in ("edge_pose", "edge_point", "edge_obs", "edge_stereo", "edge_inv_sigma2")}
    n = p["n_points"]

    def add_point(Xw, slots, stereo):
        nonlocal n
        xyz.append((Xw + rng.normal(0, 0.05, 3)).astype(np.float32)[None])
        pid.append(int(pid[-1]) + 3)
        for slot in slots:
            Rwc, twc = poses[slot]
            Xc = Rwc.T @ (Xw - twc)
            assert Xc[2] > 1.0
            u, v = fx * Xc[0] / Xc[2] + cx + rng.normal(0, 1), fy * Xc[1] / Xc[2] + cy + rng.normal(0, 1)
            ur = u - bf / Xc[2] + rng.normal(0, 1) if stereo else -1.0
            e["edge_pose"].append(slot)
            e["edge_point"].append(n)
            e["edge_obs"].append((np.float32(u), np.float32(v), np.float32(ur)))
            e["edge_stereo"].append(1 if stereo else 0)
            e["edge_inv_sigma2"].append(np.float32(1.0))
        n += 1

    slot0 = int(np.flatnonzero(np.asarray(p["pose_id"]) == 0)[0])
    add_point(np.array([1.0, -0.5, 12.0]), [], False)                       # no edge: removeVertex
    add_point(np.array([-2.0, 0.5, 15.0]), [slot0], stereo_frac > 0)        # seen by the fixed keyframe alone
    if loop:
        Rm, tm = poses[K // 2]
        ends = sorted(set(list(range(3)) + list(range(K - 3, K))))
        for _ in range(n_loop):
            add_point(tm + Rm @ np.array([rng.uniform(-10, 10), rng.uniform(-3, 3), rng.uniform(60, 100)]), ends, True)
    q = dict(p)
    q.update(n_points=n, n_edges=len(e["edge_pose"]), point_xyz=np.concatenate(xyz).astype(np.float32), point_id=np.array(pid, np.int64),
             edge_pose=np.array(e["edge_pose"], np.int32), edge_point=np.array(e["edge_point"], np.int32),
             edge_obs=np.array(e["edge_obs"], np.float32).reshape(-1, 3), edge_stereo=np.array(e["edge_stereo"], np.uint8),
             edge_inv_sigma2=np.array(e["edge_inv_sigma2"], np.float32))
    return q


def big_map(n_kf, n_points, obs=8, loop=False, seed=0, cfg="kitti"):
    """A map-sized problem for tools/gpu_global_ba_prof.py, built without Python loops: n_kf keyframes 0.6 m apart on a circle, looking
    along it; every point lies 6..40 m ahead of an anchor keyframe and is seen (stereo) by the anchor and the obs - 1 keyframes before
    it -- a banded reduced system.  loop: the keyframes before keyframe 0 are the last ones (the circle closes: points seen by the
    first and the last keyframes); otherwise a point near the start has fewer observers.  Only keyframe 0 is fixed.  Projections may
    leave the image, which the optimiser does not know."""
    rng = np.random.default_rng([seed, n_kf, n_points, int(loop)])
    c = graft.load_package().synth.CONFIGS[cfg]
    fx, fy, cx, cy, bf, W, H = (c[k] for k in ("fx", "fy", "cx", "cy", "bf", "w", "h"))
    th = 2 * np.pi * np.arange(n_kf) / n_kf
    r = n_kf * 0.6 / (2 * np.pi)
    phi = np.pi / 2 - th
    Rwc = np.zeros((n_kf, 3, 3))
    Rwc[:, 0, 0], Rwc[:, 0, 2], Rwc[:, 1, 1], Rwc[:, 2, 0], Rwc[:, 2, 2] = np.cos(phi), np.sin(phi), 1, -np.sin(phi), np.cos(phi)
    twc = np.stack([r * np.sin(th), 0.05 * np.sin(7 * th), r * (1 - np.cos(th))], 1)
    a = rng.integers(0 if loop else 1, n_kf, n_points)
    z = rng.uniform(6.0, 40.0, n_points)
    Xc = np.stack([(rng.uniform(0, W, n_points) - cx) / fx * z, (rng.uniform(0, H, n_points) - cy) / fy * z, z], 1)
    Xw = np.einsum("nij,nj->ni", Rwc[a], Xc) + twc[a]
    k = a[:, None] - np.arange(obs)[None, ::-1]                 # the observers, ascending
    valid = np.ones_like(k, bool) if loop else k >= 0
    k = np.sort(np.where(valid, k % n_kf, n_kf), 1)             # (ascending mnId after the wrap; the missing ones last)
    valid = k < n_kf
    ep, el = k[valid], np.broadcast_to(np.arange(n_points)[:, None], k.shape)[valid]
    p = np.einsum("eji,ej->ei", Rwc[ep], Xw[el] - twc[ep])
    assert (p[:, 2] > 1.0).all()
    u = fx * p[:, 0] / p[:, 2] + cx + rng.normal(0, 1, len(ep))
    v = fy * p[:, 1] / p[:, 2] + cy + rng.normal(0, 1, len(ep))
    ur = u - bf / p[:, 2] + rng.normal(0, 1, len(ep))
    Tcw = np.zeros((n_kf, 4, 4), np.float32)
    rv = rng.normal(0, 0.005, (n_kf, 3))
    rv[0] = 0
    for i in range(n_kf):
        K = np.array([[0, -rv[i, 2], rv[i, 1]], [rv[i, 2], 0, -rv[i, 0]], [-rv[i, 1], rv[i, 0], 0]])
        Rcw = (np.eye(3) + K + 0.5 * K @ K) @ Rwc[i].T
        Tcw[i, :3, :3] = Rcw
        Tcw[i, :3, 3] = -Rwc[i].T @ twc[i] + (rng.normal(0, 0.03, 3) if i else 0)
        Tcw[i, 3, 3] = 1
    fixed = np.zeros(n_kf, np.uint8)
    fixed[0] = 1
    return dict(n_poses=n_kf, n_points=n_points, n_edges=len(ep), pose_Tcw=Tcw.reshape(n_kf, 16), pose_fixed=fixed, pose_id=np.arange(n_kf, dtype=np.int64),
                point_xyz=(Xw + rng.normal(0, 0.05, Xw.shape)).astype(np.float32), point_id=np.arange(n_points, dtype=np.int64) * 3 + 7,
                edge_pose=ep.astype(np.int32), edge_point=el.astype(np.int32), edge_obs=np.stack([u, v, ur], 1).astype(np.float32),
                edge_stereo=np.ones(len(ep), np.uint8), edge_inv_sigma2=np.ones(len(ep), np.float32), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf)


def iterations_of(name):
    return CASES[name][3]


def free_keyframes(prob):
    act = np.zeros(prob["n_poses"], bool)
    act[np.asarray(prob["edge_pose"])] = True
    return int((act & (np.asarray(prob["pose_fixed"]) == 0)).sum())


def reversed_edges(prob):
    q = dict(prob)
    for k in ("edge_pose", "edge_point", "edge_obs", "edge_stereo", "edge_inv_sigma2"):
        q[k] = np.ascontiguousarray(np.asarray(prob[k])[::-1])
    return q


# ------------------------------------------------------------------------------------------------- the comparison rule
def worst(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max()) if a.size else 0.0


def resolution_by_reference(prob, iterations, robust, huber):
    """the spread of this restatement on the problem: itself under reversed edge order (what parity.lba_resolution measures with the
    oracle for the robust form)"""
    w0, w1 = solve(prob, iterations, robust, huber), solve(reversed_edges(prob), iterations, robust, huber)
    return dict(pose=worst(w0["pose_Tcw"], w1["pose_Tcw"]), point=worst(w0["point_xyz"], w1["point_xyz"]),
                decisions_equal=w0["iterations"] == w1["iterations"] and w0["trials"] == w1["trials"]), w0


def from_oracle(want):
    """oracle.lba_solve(prob, iters1=n, iters2=0) in the fields of aos2_gba_result_t"""
    return dict(pose_Tcw=want["pose_Tcw"], point_xyz=want["point_xyz"], iterations=want["iters"][0], trials=want["trials"],
                chi2_final=float(want["chi2_trace"][-1]) if len(want["chi2_trace"]) else 0.0, polls=want["polls"], stop_poll=want["stop_poll"])


def mismatches(got, want, resolution, tag=""):
    """The project's rule: iterations and trials exact, poses and points within max(1e-5, 4 x resolution), chi2_final within the same
    factor of 1e-6 (relative).  Every figure is printed before it is judged."""
    tp = max(TOL, RESOLUTION_FACTOR * resolution["pose"])
    tx = max(TOL, RESOLUTION_FACTOR * resolution["point"])
    tc = 1e-6 * max(tp, tx) / TOL
    dp, dx = worst(got["pose_Tcw"], want["pose_Tcw"]), worst(got["point_xyz"], want["point_xyz"])
    dc = abs(got["chi2_final"] - want["chi2_final"]) / max(abs(want["chi2_final"]), 1e-300)
    print(f"{tag}: iterations {got['iterations']} / {want['iterations']}, trials {got['trials']} / {want['trials']}, poses off {dp:.3g} "
          f"(allowed {tp:.3g}), points off {dx:.3g} (allowed {tx:.3g}), chi2 off {dc:.3g} relative (allowed {tc:.3g})")
    bad = []
    if got["iterations"] != want["iterations"]:
        bad.append(f"{tag}: {got['iterations']} iterations, reference {want['iterations']}")
    if got["trials"] != want["trials"]:
        bad.append(f"{tag}: {got['trials']} LM trials, reference {want['trials']}")
    if dp > tp:
        bad.append(f"{tag}: poses off by {dp:.3g}, allowed {tp:.3g}")
    if dx > tx:
        bad.append(f"{tag}: points off by {dx:.3g}, allowed {tx:.3g}")
    if not dc <= tc:
        bad.append(f"{tag}: chi2_final {got['chi2_final']!r}, reference {want['chi2_final']!r}")
    return bad
