"""CPU restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:782-1045) for the essential-graph tests, written from the
reference's lines and g2o's (types/sim3.h:70-272; types/types_seven_dof_expmap.h:60-69, 106-114; core/base_binary_edge.hpp:55-205;
core/optimization_algorithm_levenberg.cpp:61-189).  It does not call the library.

numpy float64 over the edges with a DENSE solve of H + lambda I (LAPACK's LU: nothing of the library's block-sparse LDL^T is in it).
The sums of the normal equations can be taken in another edge order or in long double, and the system solved in another elimination
order: that is how `resolution` measures what this computation determines (status exact, values within
max(1e-5, 4 x the problem's measured resolution)).

Also here: the seeded generator the CPU and GPU tests share, and the comparison of a result with the reference."""
import numpy as np

import sim3_opt_ref as S3

DELTA = S3.DELTA
EPS = S3.EPS
DBL_MAX = S3.DBL_MAX
FLOOR = 1e-5
EG_OK, EG_NO_STEP = 0, 1


# ---------------------------------------------------------------------------------------------- g2o::Sim3 over arrays
# a Sim3 array is [n][8]: q (x, y, z, w), t, s
def rot_of(q):
    """Eigen toRotationMatrix of q [n][4] -> [n][3][3]"""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], axis=1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], axis=1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def quat_rotate(q, v):
    uv = np.cross(q[:, :3], v)
    uv = uv + uv
    return v + q[:, 3:4] * uv + np.cross(q[:, :3], uv)


def mul(a, b):
    """operator* (sim3.h:266-272), row by row"""
    p, q = a[:, :4], b[:, :4]
    r = np.stack([p[:, 3] * q[:, 0] + p[:, 0] * q[:, 3] + p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1],
                  p[:, 3] * q[:, 1] + p[:, 1] * q[:, 3] + p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2],
                  p[:, 3] * q[:, 2] + p[:, 2] * q[:, 3] + p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0],
                  p[:, 3] * q[:, 3] - p[:, 0] * q[:, 0] - p[:, 1] * q[:, 1] - p[:, 2] * q[:, 2]], axis=1)
    t = a[:, 7:8] * quat_rotate(p, b[:, 4:7]) + a[:, 4:7]
    return np.concatenate([r, t, a[:, 7:8] * b[:, 7:8]], axis=1)


def inverse(S):
    c = S[:, :4] * np.array([-1.0, -1.0, -1.0, 1.0])
    return np.concatenate([c, quat_rotate(c, (-1 / S[:, 7:8]) * S[:, 4:7]), 1 / S[:, 7:8]], axis=1)


def smap(S, X):
    return S[:, 7:8] * quat_rotate(S[:, :4], X) + S[:, 4:7]


def exp1(u):
    """Sim3(Vector7d) of one update -> [8]"""
    q, t, s = S3.sim3_exp(np.asarray(u, np.float64))
    return np.concatenate([q, t, [s]])


def skew(w):
    z = np.zeros(len(w))
    return np.stack([np.stack([z, -w[:, 2], w[:, 1]], axis=1), np.stack([w[:, 2], z, -w[:, 0]], axis=1), np.stack([-w[:, 1], w[:, 0], z], axis=1)], axis=1)


def log(S):
    """Sim3::log (sim3.h:148-230), row by row -> [n][7].  Every branch is evaluated and the line's own condition selects."""
    s = S[:, 7]
    sigma = np.log(s)
    R = rot_of(S[:, :4])
    d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], axis=1)
    small_s, small_r = np.abs(sigma) < EPS, d > 1 - EPS
    with np.errstate(all="ignore"):
        theta = np.arccos(np.where(small_r, 0.0, d))
        theta2, sigma2 = theta * theta, sigma * sigma
        f = np.where(small_r, 0.5, theta / (2 * np.sqrt(1 - d * d)))
        a, b, c = s * np.sin(theta), s * np.cos(theta), theta2 + sigma2
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        A = np.where(small_s, np.where(small_r, 0.5, (1 - np.cos(theta)) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (a * sigma + (1 - b) * theta) / (theta * c)))
        B = np.where(small_s, np.where(small_r, 1.0 / 6.0, (theta - np.sin(theta)) / (theta2 * theta)),
                     np.where(small_r, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma), (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2))
    omega = f[:, None] * dR
    Om = skew(omega)
    W = A[:, None, None] * Om + (B[:, None, None] * Om) @ Om + C[:, None, None] * np.eye(3)
    ups = np.linalg.solve(W, S[:, 4:7, None])[:, :, 0]   # W.lu().solve(t): LU with row pivoting
    return np.concatenate([omega, ups, sigma[:, None]], axis=1)


def residuals(C, est, v0, v1):
    """EdgeSim3::computeError of every edge: log(C * S_v0 * S_v1^-1)"""
    return log(mul(mul(C, est[v0]), inverse(est[v1])))


def oplus_all(u, fix_scale, est):
    """oplusImpl with one update for every row"""
    u = np.array(u, np.float64)
    if fix_scale:
        u[6] = 0
    return mul(np.broadcast_to(exp1(u), est.shape), est)


# ---------------------------------------------------------------------------------------------- the optimisation
def jacobians(P, est, order):
    """computeActiveErrors and the central differences of every edge, in the edge order `order` -> e [ne][7], J0, J1 [ne][7][7]
    (the Jacobian of a fixed side is computed like any other; linearise does not use it)"""
    fix = bool(P["fix_scale"])
    v0, v1, C = P["v0"][order], P["v1"][order], P["Sji"][order]
    e = residuals(C, est, v0, v1)
    scalar = 1.0 / (2 * DELTA)
    J0, J1 = np.zeros((len(v0), 7, 7)), np.zeros((len(v0), 7, 7))
    inv = inverse(est)
    for d in range(7):
        u = np.zeros(7)
        u[d] = DELTA
        plus = oplus_all(u, fix, est)
        u[d] = -DELTA
        minus = oplus_all(u, fix, est)
        CA = mul(C, est[v0])
        J0[:, :, d] = scalar * (log(mul(mul(C, plus[v0]), inv[v1])) - log(mul(mul(C, minus[v0]), inv[v1])))
        J1[:, :, d] = scalar * (log(mul(CA, inverse(plus)[v1])) - log(mul(CA, inverse(minus)[v1])))
    return e, J0, J1


def linearise(P, est, order, acc):
    """computeActiveErrors, the central differences, constructQuadraticForm -> H [7 nv][7 nv] (the fixed vertex's rows stay zero),
    b, chi2; the sums in the edge order `order`, accumulated in dtype `acc`"""
    nv = len(est)
    v0, v1 = P["v0"][order], P["v1"][order]
    e, J0, J1 = jacobians(P, est, order)
    H = np.zeros((nv, nv, 7, 7), acc)
    b = np.zeros((nv, 7), acc)
    f0, f1 = v0 != P["fixed"], v1 != P["fixed"]
    J0, J1, ea = J0.astype(acc), J1.astype(acc), e.astype(acc)
    np.add.at(H, (v0[f0], v0[f0]), np.einsum("nra,nrb->nab", J0[f0], J0[f0]))
    np.add.at(H, (v1[f1], v1[f1]), np.einsum("nra,nrb->nab", J1[f1], J1[f1]))
    both = f0 & f1
    cross = np.einsum("nra,nrb->nab", J0[both], J1[both])
    np.add.at(H, (v0[both], v1[both]), cross)
    np.add.at(H, (v1[both], v0[both]), cross.transpose(0, 2, 1))
    np.add.at(b, v0[f0], -np.einsum("nra,nr->na", J0[f0], ea[f0]))
    np.add.at(b, v1[f1], -np.einsum("nra,nr->na", J1[f1], ea[f1]))
    chi = acc(0)
    for c in (ea * ea).sum(axis=1):
        chi = chi + c
    H = H.transpose(0, 2, 1, 3).reshape(7 * nv, 7 * nv)
    return H.astype(np.float64), b.reshape(-1).astype(np.float64), float(chi)


def chi2(P, est, order, acc):
    e = residuals(P["Sji"][order], est, P["v0"][order], P["v1"][order]).astype(acc)
    chi = acc(0)
    for c in (e * e).sum(axis=1):
        chi = chi + c
    return float(chi)


def dense_solve(H, b, lam, keep, perm):
    """(H + lambda I) x = b over the rows `keep` (the free vertices), eliminated in the order `perm` of them; None when it fails"""
    idx = keep[perm]
    A = H[np.ix_(idx, idx)] + lam * np.eye(len(idx))
    try:
        x = np.linalg.solve(A, b[idx])
    except np.linalg.LinAlgError:
        return None
    if not np.isfinite(x).all():
        return None
    out = np.zeros(len(b))
    out[idx] = x
    return out


def optimize(P, order=None, acc=np.float64, perm_seed=None):
    """:986-1044 -> dict(Scw, Tiw, Xw, chi2_initial, chi2_final, iterations, trials, rejected, status)"""
    est = np.array(P["Scw"], np.float64)
    nv, ne, fix, fixed = len(est), len(P["v0"]), bool(P["fix_scale"]), int(P["fixed"])
    order = np.arange(ne) if order is None else order
    log_ = dict(iterations=0, trials=0, rejected=0, accepted_first=0, chi2_initial=0.0, chi2_final=0.0)
    runs = nv > 1 and ne > 0
    if runs:
        keep = np.flatnonzero(np.repeat(np.arange(nv) != fixed, 7))
        perm = np.arange(len(keep)) if perm_seed is None else np.random.default_rng(perm_seed).permutation(len(keep))
        x = np.zeros(7 * nv)
        lam, ni, n_bad, ok, i = 1e-16, 2.0, 0, True, 0
        while i < int(P.get("iterations", 20)) and ok:
            H, b, current = linearise(P, est, order, acc)
            ini = current
            if i == 0:
                log_["chi2_initial"] = current
            rho, qmax = 0.0, 0
            while True:
                sol = dense_solve(H, b, lam, keep, perm)
                if sol is not None:
                    x = sol
                trial = est.copy()
                for v in range(nv):
                    if v != fixed:
                        u = x[7 * v:7 * v + 7].copy()
                        if fix:
                            u[6] = 0
                        trial[v] = mul(exp1(u)[None], est[v:v + 1])[0]
                temp = chi2(P, trial, order, acc)
                if sol is None:
                    temp = DBL_MAX
                rho = current - temp
                scale = float((x * (lam * x + b)).sum()) + 1e-3
                rho = rho / scale
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam, ni, current, est = lam * max(1.0 / 3.0, alpha), 2.0, temp, trial
                    if i == 0:
                        log_["accepted_first"] += 1
                else:
                    lam, ni = lam * ni, ni * 2
                    log_["rejected"] += 1
                qmax += 1
                log_["trials"] += 1
                if not (rho < 0 and qmax < 10):
                    break
            log_["iterations"] += 1
            i += 1
            if qmax == 10 or rho == 0:
                ok = False
            else:
                n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
                ok = n_bad < 3
            log_["chi2_final"] = current
    Tiw = np.zeros((nv, 4, 4), np.float32)
    Tiw[:, :3, :3] = rot_of(est[:, :4]).astype(np.float32)
    Tiw[:, :3, 3] = (est[:, 4:7] * (1.0 / est[:, 7:8])).astype(np.float32)
    Tiw[:, 3, 3] = 1
    ref = np.asarray(P["ref"], np.int64)
    X = np.asarray(P["Xw"], np.float32).astype(np.float64).reshape(-1, 3)
    Xw = smap(inverse(est)[ref], smap(np.asarray(P["Scw"], np.float64)[ref], X)).astype(np.float32) if len(ref) else np.zeros((0, 3), np.float32)
    status = EG_NO_STEP if runs and log_["accepted_first"] == 0 else EG_OK
    return dict(Scw=est, Tiw=Tiw, Xw=Xw, status=status, **log_)


# ---------------------------------------------------------------------------------------------- comparison
def values(res):
    """R(q), t, s of every vertex as one vector"""
    S = np.asarray(res["Scw"], np.float64)
    return np.concatenate([rot_of(S[:, :4]).reshape(-1), S[:, 4:8].reshape(-1)])


def resolution(P, base=None):
    """the largest difference of R(q), t, s between the restatement and re-associations of itself: another edge order, another
    elimination order, long double sums -> (resolution, status all equal)"""
    base = base or optimize(P)
    ne = len(P["v0"])
    worst, same_status = 0.0, True
    for kw in (dict(order=np.random.default_rng(ne + 17).permutation(ne)), dict(perm_seed=ne + 5), dict(acc=np.longdouble)):
        v = optimize(P, **kw)
        same_status = same_status and v["status"] == base["status"]
        worst = max(worst, float(np.abs(values(v) - values(base)).max()))
    return worst, same_status


def tolerance(res):
    return max(FLOOR, 4 * res)


def same(got, want, P, res):
    """the comparison rule: status exact, the fixed vertex bit-identical, with fix_scale every s bit-identical, R(q), t, s of every
    vertex within max(1e-5, 4 x resolution), Tiw and Xw likewise in float; iterations / trials are not compared -> (ok, message)"""
    tol = tolerance(res)
    Sin, Sg = np.asarray(P["Scw"], np.float64), np.asarray(got["Scw"], np.float64)
    if got["status"] != want["status"]:
        return False, "status %d / %d" % (got["status"], want["status"])
    if Sg[P["fixed"]].tobytes() != Sin[P["fixed"]].tobytes():
        return False, "the fixed vertex moved"
    if P["fix_scale"] and Sg[:, 7].tobytes() != Sin[:, 7].tobytes():
        return False, "fix_scale: a scale changed"
    d = float(np.abs(values(got) - values(want)).max())
    dT = float(np.abs(np.asarray(got["Tiw"], np.float64) - want["Tiw"]).max())
    dX = float(np.abs(np.asarray(got["Xw"], np.float64) - want["Xw"]).max()) if len(want["Xw"]) else 0.0
    return max(d, dT, dX) <= tol, "Scw differs by %.3g, Tiw by %.3g, Xw by %.3g, tolerance %.3g" % (d, dT, dX, tol)


# ---------------------------------------------------------------------------------------------- generator
SIZES = (1, 2, 3, 9, 17, 64, 65, 130, 300)
FIX_SCALE = (False, True, False, True, False, True, False, True, False)   # both values, and both at a size with a loop (9 / 17, 64 / 65, ...)


def _truth(n):
    """keyframes half a metre apart on a circle that nearly closes, looking along the tangent: Scw [n][8], s = 1"""
    r = max(1.5, 0.5 * n / (2 * np.pi))
    phi = 2 * np.pi * 0.97 * np.arange(n) / max(n, 1)
    out = np.zeros((n, 8))
    for i in range(n):
        Rm = S3._rotation([0.1, 1.0, 0.05], -phi[i])
        c = r * np.array([np.cos(phi[i]), 0.05 * np.sin(3 * phi[i]), np.sin(phi[i])])
        q = S3.quat_from_rot(Rm)
        out[i] = np.concatenate([q / np.linalg.norm(q), -Rm @ c, [1.0]])
    return out


def edges_of(n, more=0):
    """the edges in the insertion order of :853-984 for the generator's map -> v0, v1, kind (0 LoopConnections, 1 spanning tree,
    2 loop edge, 3 covisibility), and the keyframes of CorrectedSim3.  Keyframe 1 is pLoopKF, n - 1 pCurKF; keyframe 0 is joined to
    keyframe 1 alone."""
    loop, cur = min(1, n - 1), n - 1
    cur_side = list(range(n - min(3, max(1, n // 8)), n)) if n >= 3 else []
    targets = [j for j in (1, 2, 3) if j < (cur_side[0] - 1 if cur_side else 0)] or ([loop] if n >= 3 else [])
    v0, v1, kind, inserted = [], [], [], set()

    def add(a, b, k):
        v0.append(a), v1.append(b), kind.append(k)

    if n >= 3:
        add(loop, cur, 0)                       # LoopConnections[pLoopKF] holds pCurKF: the loop edge in the other orientation
        inserted.add((loop, cur))
        for i in cur_side:
            for j in targets:
                add(i, j, 0)
                inserted.add((min(i, j), max(i, j)))
            if i == cur and n >= 5:
                add(i, i - 1, 0)                # ... and its parent: the pair of a spanning-tree edge
                inserted.add((i - 1, i))
    early = (n // 2, 2) if n >= 9 else None     # a loop closed earlier
    for i in range(n):
        if i > 0:
            add(i, i - 1, 1)
        if early and i == early[0]:
            add(i, early[1], 2)
        for j in range(i - 2, max(0, i - 2 - (2 + more + i % 5)), -1):   # 2-6 (+ more) earlier keyframes, never keyframe 0
            if j < 1 or (early and (i, j) == early) or (j, i) in inserted:
                continue
            add(i, j, 3)
    return np.array(v0, np.int32), np.array(v1, np.int32), np.array(kind, np.int32), cur_side


def problem(seed, n, fix_scale, planted=False, n_points=None, drift=1.0, more=0):
    """a keyframe chain with planted poses, estimates that drifted away from them along the chain (and in scale unless fix_scale), the
    Sim3 correction of the loop for the current keyframe and its neighbours, measurements formed as :858-868 and :890-973 form them,
    and map points with their reference keyframes.  planted: the measurements are the truth's, the fixed vertex is at the truth."""
    rng = np.random.default_rng([seed, n, int(fix_scale), int(planted)])
    T = _truth(n)
    step = np.concatenate([0.002 * rng.normal(size=(n, 3)), 0.01 * rng.normal(size=(n, 3)), (0.0 if fix_scale else 0.002) * rng.normal(size=(n, 1))], axis=1)
    walk = np.cumsum(step * drift, axis=0)
    U = np.stack([mul(exp1(walk[i])[None], T[i:i + 1])[0] for i in range(n)]) if n else T
    if not planted:
        U[:, 7] = 1.0   # keyframe poses are SE3
    v0, v1, kind, cur_side = edges_of(n, more)
    loop, cur = min(1, n - 1), n - 1
    vScw = U.copy()
    if planted:
        vScw[loop] = T[loop]
        Sji = mul(T[v1], inverse(T)[v0]) if len(v0) else np.zeros((0, 8))
    else:
        if cur_side:
            rel = mul(T[cur:cur + 1], inverse(T[loop:loop + 1]))
            rel[0, 7] = 1.0 if fix_scale else 0.96
            corrected_cur = mul(rel, U[loop:loop + 1])
            for k in cur_side:   # g2oCorrectedSiw = g2oSic * mg2oScw
                vScw[k] = mul(mul(U[k:k + 1], inverse(U[cur:cur + 1])), corrected_cur)[0]
        if len(v0):
            lc = kind == 0
            Sji = np.where(lc[:, None], mul(vScw[v1], inverse(vScw)[v0]), mul(U[v1], inverse(U)[v0]))
        else:
            Sji = np.zeros((0, 8))
    n_points = 4 * n if n_points is None else n_points
    ref = rng.integers(0, n, n_points).astype(np.int32)
    Xc = np.stack([rng.uniform(-2, 2, n_points), rng.uniform(-1, 1, n_points), rng.uniform(2, 8, n_points)], axis=1)
    Xw = smap(inverse(U)[ref], Xc).astype(np.float32) if n_points else np.zeros((0, 3), np.float32)
    return dict(Scw=vScw, fixed=loop, v0=v0, v1=v1, Sji=Sji, fix_scale=bool(fix_scale), iterations=20, Xw=Xw, ref=ref, kind=kind, truth=T,
                uncorrected=U, cur_side=cur_side)


_CASE = {}


def generator_case(seed):
    """the problems of SIZES for `seed`: problems, want (the restatement's results) and the resolution of each.  Once per process."""
    if seed not in _CASE:
        problems = [problem(seed, n, fix) for n, fix in zip(SIZES, FIX_SCALE)]
        want = [optimize(P) for P in problems]
        res = []
        for P, w in zip(problems, want):
            r, same_status = resolution(P, w) if len(P["v0"]) else (0.0, True)
            if not same_status:
                raise RuntimeError("the re-associations disagree on the status")
            res.append(r)
        _CASE[seed] = dict(problems=problems, want=want, resolution=res)
    return _CASE[seed]
