"""CPU restatement of Optimizer::OptimizeSim3 (src/Optimizer.cc:1047-1242) for the OptimizeSim3 tests, written from the reference's
lines and g2o's (types/sim3.h:70-146, 233-272; types/types_seven_dof_expmap.h:60-69, 130-171; core/base_binary_edge.hpp:55-205;
core/optimization_algorithm_levenberg.cpp:61-189; core/robust_kernel_impl.cpp:78-91).  It does not call the library.

numpy over the correspondences, in float64 or np.longdouble; the sums of the normal equations can be taken in another edge order or
per wave-sized chunk, which is how `resolution` measures what this computation determines (the comparison
rule is decisions exact, values within 4 x the problem's measured resolution).

Also here: the seeded generator the CPU and GPU tests share, and the comparison of a result with the reference."""
import numpy as np

DELTA = 1e-9     # base_binary_edge.hpp:147
EPS = 0.00001    # sim3.h:90
DBL_MAX = 1.7976931348623157e308
TH2 = 10.0       # LoopClosing.cc:355
MARGIN = 1e-3    # relative distance every decision chi2 keeps from th2
FLOOR = 1e-5


# ---------------------------------------------------------------------------------------------- g2o::Sim3
def quat_from_rot(m):
    """Eigen Quaterniond(Matrix3d): (x, y, z, w), not normalised"""
    T = m.dtype.type
    q = np.zeros(4, m.dtype)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + T(1))
        q[3] = T(0.5) * t
        t = T(0.5) / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + T(1))
        q[i] = T(0.5) * t
        t = T(0.5) / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def rot_of(q):
    """Eigen toRotationMatrix of (x, y, z, w)"""
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], dtype=np.asarray(q).dtype)


def quat_rotate(q, v):
    """Eigen's q * v: v + w uv + qv x uv, uv = 2 qv x v; v [..., 3]"""
    uv = np.cross(q[:3], v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(q[:3], uv)


def skew(w):
    z = w.dtype.type(0)
    return np.array([[z, -w[2], w[1]], [w[2], z, -w[0]], [-w[1], w[0], z]], dtype=w.dtype)


def sim3_exp(u):
    """Sim3(const Vector7d&), sim3.h:70-142 -> (q, t, s)"""
    T = u.dtype.type
    omega, ups, sigma = u[:3], u[3:6], u[6]
    theta = np.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = skew(omega)
    Om2 = Om @ Om
    I = np.eye(3, dtype=u.dtype)
    s = np.exp(sigma)
    if abs(sigma) < EPS:
        C = T(1)
        if theta < EPS:
            A, B = T(1) / T(2), T(1) / T(6)
            R = I + Om + Om2
        else:
            theta2 = theta * theta
            A = (1 - np.cos(theta)) / theta2
            B = (theta - np.sin(theta)) / (theta2 * theta)
            R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
    else:
        C = (s - 1) / sigma
        if theta < EPS:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((T(0.5) * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = I + Om + Om2
        else:
            R = I + np.sin(theta) / theta * Om + (1 - np.cos(theta)) / (theta * theta) * Om2
            a, b = s * np.sin(theta), s * np.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1 / theta2
    W = A * Om + B * Om2 + C * I
    return quat_from_rot(R), W @ ups, s


def sim3_mul(a, b):
    """operator*, sim3.h:266-272 (the quaternion is not renormalised)"""
    p, q = a[0], b[0]
    r = np.array([p[3] * q[0] + p[0] * q[3] + p[1] * q[2] - p[2] * q[1],
                  p[3] * q[1] + p[1] * q[3] + p[2] * q[0] - p[0] * q[2],
                  p[3] * q[2] + p[2] * q[3] + p[0] * q[1] - p[1] * q[0],
                  p[3] * q[3] - p[0] * q[0] - p[1] * q[1] - p[2] * q[2]], dtype=p.dtype)
    return r, a[2] * quat_rotate(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inverse(S):
    q, t, s = S
    c = np.array([-q[0], -q[1], -q[2], q[3]], dtype=q.dtype)
    return c, quat_rotate(c, (-1 / s) * t), 1 / s


def sim3_map(S, X):
    return S[2] * quat_rotate(S[0], X) + S[1]


def oplus(u, fix_scale, S):
    """VertexSim3Expmap::oplusImpl: zeroes u[6] in place"""
    if fix_scale:
        u[6] = 0
    return sim3_mul(sim3_exp(u), S)


# ---------------------------------------------------------------------------------------------- the graph
class Graph:
    """the edges of one problem in `dtype`; row 2c = e12 of correspondence c, row 2c + 1 = its e21"""

    def __init__(self, P, dtype, order=None, chunk=None, delta=DELTA):
        f = lambda k: np.asarray(P[k], np.float32).astype(dtype)   # noqa: E731
        self.T, self.dtype = dtype, dtype
        self.X1, self.X2, self.o1, self.o2, self.w1, self.w2 = (f(k) for k in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"))
        self.K1 = np.asarray(P["K1"], np.float32).astype(dtype)
        self.K2 = np.asarray(P["K2"], np.float32).astype(dtype)
        self.n = len(self.X1)
        self.active = np.ones(self.n, bool)
        self.chi12, self.chi21 = np.zeros(self.n, dtype), np.zeros(self.n, dtype)
        self.order, self.chunk, self.delta = order, chunk, dtype(delta)
        self.huber = dtype(np.sqrt(np.float32(P["th2"])))   # deltaHuber: a float (:1096)

    @staticmethod
    def _res(obs, K, p):
        return np.stack([obs[:, 0] - (p[:, 0] / p[:, 2] * K[0] + K[2]), obs[:, 1] - (p[:, 1] / p[:, 2] * K[1] + K[3])], axis=1)

    def residuals(self, S):
        return self._res(self.o1, self.K1, sim3_map(S, self.X2)), self._res(self.o2, self.K2, sim3_map(sim3_inverse(S), self.X1))

    def _total(self, terms):
        """sum of the rows of terms [2n][k] of the active correspondences: in index order, a given order, or per chunk first"""
        rows = np.repeat(self.active, 2)
        idx = np.arange(2 * self.n) if self.order is None else self.order
        t = terms[idx][rows[idx]]
        if self.chunk:
            parts = [t[k:k + self.chunk].sum(axis=0) for k in range(0, len(t), self.chunk)]
            return np.sum(np.array(parts, dtype=self.dtype), axis=0) if parts else np.zeros(terms.shape[1], self.dtype)
        acc = np.zeros(terms.shape[1], self.dtype)
        for row in t:
            acc = acc + row
        return acc

    def _robust(self, e, w):
        chi = e[:, 0] * (w * e[:, 0]) + e[:, 1] * (w * e[:, 1])
        dsqr = self.huber * self.huber
        big = chi > dsqr
        sq = np.sqrt(np.where(big, chi, self.T(1)))
        return chi, np.where(big, 2 * sq * self.huber - dsqr, chi), np.where(big, self.huber / sq, self.T(1))

    def _store(self, c12, c21):
        self.chi12 = np.where(self.active, c12, self.chi12)
        self.chi21 = np.where(self.active, c21, self.chi21)

    def trial(self, S):
        e12, e21 = self.residuals(S)
        c12, r12, _ = self._robust(e12, self.w1)
        c21, r21, _ = self._robust(e21, self.w2)
        self._store(c12, c21)
        return self._total(np.stack([r12, r21], axis=1).reshape(-1, 1))[0]

    def jacobians(self, S, fix_scale):
        """g2o's central differences -> J12, J21 [n][2][7]"""
        scalar = self.T(1) / (2 * self.delta)
        J12, J21 = np.zeros((self.n, 2, 7), self.dtype), np.zeros((self.n, 2, 7), self.dtype)
        for d in range(7):
            add = np.zeros(7, self.dtype)
            add[d] = self.delta
            p12, p21 = self.residuals(oplus(add, fix_scale, S))
            add[d] = -self.delta
            m12, m21 = self.residuals(oplus(add, fix_scale, S))
            J12[:, :, d], J21[:, :, d] = scalar * (p12 - m12), scalar * (p21 - m21)
        return J12, J21

    def edge_terms(self, S, fix_scale):
        """computeActiveErrors + what constructQuadraticForm adds per edge -> [2n][36]: H (upper triangle row by row), b, rho[0];
        row 2c = e12 of correspondence c, row 2c + 1 = its e21 (the chi2 of the active correspondences are stored)"""
        e12, e21 = self.residuals(S)
        J12, J21 = self.jacobians(S, fix_scale)
        c12, r12, w12 = self._robust(e12, self.w1)
        c21, r21, w21 = self._robust(e21, self.w2)
        self._store(c12, c21)
        iu = np.triu_indices(7)

        def terms(J, e, w, rho0, rho1):
            H = np.einsum("nir,n,nic->nrc", J, rho1 * w, J)[:, iu[0], iu[1]]
            b = np.einsum("nir,ni->nr", J, -(w[:, None] * e) * rho1[:, None])
            return np.concatenate([H, b, rho0[:, None]], axis=1)

        return np.stack([terms(J12, e12, self.w1, r12, w12), terms(J21, e21, self.w2, r21, w21)], axis=1).reshape(2 * self.n, 36)

    def linearise(self, S, fix_scale):
        """computeActiveErrors + activeRobustChi2 + buildSystem -> H [7][7], b [7], chi"""
        iu = np.triu_indices(7)
        tot = self._total(self.edge_terms(S, fix_scale))
        H = np.zeros((7, 7), self.dtype)
        H[iu] = tot[:28]
        H = H + np.triu(H, 1).T
        return H, tot[28:35], tot[35]

    def reject(self, th2, remove):
        bad = self.active & ((self.chi12 > th2) | (self.chi21 > th2))
        margin = np.abs(np.concatenate([self.chi12[self.active], self.chi21[self.active]]) - th2).min() / th2 if self.active.any() else np.inf
        if remove:
            self.active = self.active & ~bad
        return bad, float(margin)


def closed_form_jacobians(G, S):
    """d e12 / d u and d e21 / d u at u = 0 for exp(u) S: exp(u) Y = Y + omega x Y + upsilon + sigma Y + O(u^2), and
    (exp(u) S)^-1 = S^-1 exp(-u)"""
    q, t, s = S
    Rm = rot_of(q / np.linalg.norm(q))

    def dproj(K, p):
        z = p[:, 2]
        o = np.zeros_like(z)
        return -np.stack([np.stack([K[0] / z, o, -K[0] * p[:, 0] / (z * z)], axis=1), np.stack([o, K[1] / z, -K[1] * p[:, 1] / (z * z)], axis=1)], axis=1)

    def dexp(Y):   # [n][3][7]
        return np.concatenate([np.stack([-skew(y) for y in Y]), np.broadcast_to(np.eye(3), (len(Y), 3, 3)), Y[:, :, None]], axis=2)

    p = s * G.X2 @ Rm.T + t
    J12 = dproj(G.K1, p) @ dexp(p)
    qv = (G.X1 - t) @ Rm / s
    J21 = dproj(G.K2, qv) @ (-(1.0 / s) * Rm.T @ dexp(G.X1))
    return J12, J21


def cholesky_solve(H, b):
    """LinearSolverDense: LL^T of the 7x7; None when a pivot is not positive"""
    n, T = len(b), H.dtype.type
    L = np.zeros((n, n), H.dtype)
    for j in range(n):
        d = H[j, j] - (L[j, :j] * L[j, :j]).sum()
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, n):
            L[i, j] = (H[i, j] - (L[i, :j] * L[j, :j]).sum()) / L[j, j]
    y = np.zeros(n, H.dtype)
    for i in range(n):
        y[i] = (b[i] - (L[i, :i] * y[:i]).sum()) / L[i, i]
    x = np.zeros(n, H.dtype)
    for i in reversed(range(n)):
        x[i] = (y[i] - (L[i + 1:, i] * x[i + 1:]).sum()) / L[i, i]
    return x + T(0)


def lm_optimize(G, S, iterations, fix_scale, x, log):
    """SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg (levenberg.cpp:61-164) -> S"""
    T = G.T
    lam, ni, n_bad, ok = T(0), T(2), 0, True
    i = 0
    while i < iterations and ok:
        H, b, current = G.linearise(S, fix_scale)
        ini = current
        if i == 0:
            lam, ni, n_bad = T(1e-5) * np.abs(np.diag(H)).max(), T(2), 0
        rho, qmax = T(0), 0
        while True:
            backup = S
            sol = cholesky_solve(H + lam * np.eye(7, dtype=G.dtype), b)
            if sol is not None:
                x[:] = sol
            S = oplus(x, fix_scale, backup)
            temp = G.trial(S)
            if sol is None:
                temp = T(DBL_MAX)
            rho = current - temp
            scale = (x * (lam * x + b)).sum() + T(1e-3)
            rho = rho / scale
            if rho > 0 and np.isfinite(temp):
                alpha = min(1 - (2 * rho - 1) ** 3, T(2) / T(3))
                lam, ni, current = lam * max(T(1) / T(3), alpha), T(2), temp
            else:
                lam, ni, S = lam * ni, ni * 2, backup
                log["rejected"] += 1
            qmax += 1
            log["trials"] += 1
            if not (rho < 0 and qmax < 10):
                break
        log["iterations"] += 1
        i += 1
        if qmax == 10 or rho == 0:
            ok = False
        else:
            n_bad = n_bad + 1 if (ini - current) * T(1e3) < ini else 0
            ok = n_bad < 3
    return S


def optimize_sim3(P, dtype=np.float64, order=None, chunk=None, delta=DELTA):
    """:1181-1241 -> dict(q12, t12, s12, outlier, n_bad, n_inliers, wrote, iterations, trials, rejected, margin)"""
    S_in = (np.asarray(P["q12"], np.float64).astype(dtype), np.asarray(P["t12"], np.float64).astype(dtype), dtype(P["s12"]))
    n, th2, fix = len(P["X1c"]), dtype(np.float32(P["th2"])), bool(P["fix_scale"])
    out = dict(q12=np.asarray(P["q12"], np.float64), t12=np.asarray(P["t12"], np.float64), s12=np.float64(P["s12"]), outlier=np.zeros(n, np.uint8),
               n_bad=0, n_inliers=0, wrote=0, iterations=[0, 0], trials=[0, 0], rejected=0, margin=np.inf)
    if n == 0:
        return out
    G = Graph(P, dtype, order, chunk, delta)
    x = np.zeros(7, dtype)
    logs = [dict(iterations=0, trials=0, rejected=0), dict(iterations=0, trials=0, rejected=0)]
    S = lm_optimize(G, S_in, 5, fix, x, logs[0])
    bad, m1 = G.reject(th2, True)
    n_bad = int(bad.sum())
    out.update(n_bad=n_bad, outlier=bad.astype(np.uint8), margin=m1)
    if n - n_bad >= 10:
        S = lm_optimize(G, S, 10 if n_bad > 0 else 5, fix, x, logs[1])
        bad2, m2 = G.reject(th2, False)
        out.update(outlier=(bad | bad2).astype(np.uint8), n_inliers=int(n - n_bad - bad2.sum()), wrote=1, margin=min(m1, m2),
                   q12=np.asarray(S[0], np.float64), t12=np.asarray(S[1], np.float64), s12=np.float64(S[2]))
        out["S_exact"] = S
    out.update(iterations=[l["iterations"] for l in logs], trials=[l["trials"] for l in logs], rejected=sum(l["rejected"] for l in logs))
    return out


# ---------------------------------------------------------------------------------------------- comparison
def values(res):
    """R(q12), t12, s12 as one vector"""
    return np.concatenate([rot_of(np.asarray(res["q12"], np.float64)).ravel(), np.asarray(res["t12"], np.float64), [float(res["s12"])]])


def decisions(res):
    return (np.asarray(res["outlier"], np.uint8).tobytes(), int(res["n_bad"]), int(res["n_inliers"]))


def resolution(P, base=None):
    """the largest difference of R(q12), t12, s12 between the restatement and re-associations of itself: another edge order, long
    double arithmetic, sums per wave-sized chunk -> (resolution, decisions all equal)"""
    base = base or optimize_sim3(P)
    n = len(P["X1c"])
    order = np.random.default_rng(n + 17).permutation(2 * n)
    worst, same_dec = 0.0, True
    for kw in (dict(order=order), dict(dtype=np.longdouble), dict(chunk=64)):
        v = optimize_sim3(P, **kw)
        same_dec = same_dec and decisions(v) == decisions(base) and v["wrote"] == base["wrote"]
        worst = max(worst, float(np.abs(values(v) - values(base)).max()))
    return worst, same_dec


def tolerance(res):
    return max(FLOOR, 4 * res)


def same(got, want, P, res):
    """the comparison rule: decisions exact (flags, n_bad, n_inliers, the return path), values within max(1e-5, 4 x resolution);
    iterations / trials are not compared -> (ok, message)"""
    if decisions(got) != decisions(want):
        return False, "decisions: n_bad %d / %d, n_inliers %d / %d, flags differ at %s" % (
            got["n_bad"], want["n_bad"], got["n_inliers"], want["n_inliers"], np.flatnonzero(np.asarray(got["outlier"]) != want["outlier"])[:8])
    raw_in = np.concatenate([np.asarray(P["q12"], np.float64), np.asarray(P["t12"], np.float64), [np.float64(P["s12"])]]).tobytes()
    raw_out = np.concatenate([np.asarray(got["q12"], np.float64), np.asarray(got["t12"], np.float64), [np.float64(got["s12"])]]).tobytes()
    if not want["wrote"]:
        return raw_in == raw_out, "the return through :1212 leaves g2oS12 bit for bit"
    d = float(np.abs(values(got) - values(want)).max())
    return d <= tolerance(res), "S12 differs by %.3g, tolerance %.3g" % (d, tolerance(res))


# ---------------------------------------------------------------------------------------------- generator
K_A = (520.9, 521.0, 325.1, 249.7)
K_B = (535.4, 539.2, 320.1, 247.6)
# n, gross outliers (a prefix), fix_scale, start far from the planted Sim3
BATCH = ((0, 0, False, False), (9, 2, False, False), (10, 0, True, False), (31, 0, False, False), (32, 6, True, True), (33, 25, False, False),
         (64, 10, False, True), (127, 30, True, False), (128, 0, False, True), (129, 40, False, False), (300, 60, True, True), (10, 1, False, False))
SIZES = tuple(b[0] for b in BATCH)


def _rotation(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = skew(a)
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _project(K, X):
    return np.stack([X[:, 0] / X[:, 2] * K[0] + K[2], X[:, 1] / X[:, 2] * K[1] + K[3]], axis=1)


def problem(rng, n, n_out, fix_scale, far, noise=1.0, baseline=0.3):
    """points 2-8 m in front of camera 2, a planted Sim3 S12 (X1 = s R X2 + t), pixel noise sigma = 1.2^octave, gross outliers of
    5-40 px on a prefix, inputs rounded to float32, a start perturbed from the planted Sim3.  `baseline` bounds |t| per axis: the
    scale is seen through it alone (e21 projects R^T (X1 - t) / s, which s does not move, and e12 projects s (R X2 + t / s))"""
    KA, KB = np.float32(K_A).astype(np.float64), np.float32(K_B).astype(np.float64)   # the cameras are their float32 intrinsics
    z = rng.uniform(2, 8, n)
    uv = np.stack([rng.uniform(60, 580, n), rng.uniform(60, 420, n)], axis=1)
    X2 = np.stack([(uv[:, 0] - K_B[2]) / K_B[0] * z, (uv[:, 1] - K_B[3]) / K_B[1] * z, z], axis=1)
    R = _rotation(rng.normal(size=3), rng.uniform(0.05, 0.3))
    t = rng.uniform(-baseline, baseline, 3)
    s = 1.0 if fix_scale else rng.uniform(0.9, 1.1)
    X1 = s * X2 @ R.T + t
    oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    obs1 = _project(KA, X1) + noise * rng.normal(size=(n, 2)) * (1.2 ** oct1)[:, None]
    obs2 = _project(KB, X2) + noise * rng.normal(size=(n, 2)) * (1.2 ** oct2)[:, None]
    ang = rng.uniform(0, 2 * np.pi, n_out)
    obs1[:n_out] += rng.uniform(5, 40, n_out)[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    k = 8.0 if far else 1.0
    R0 = _rotation(rng.normal(size=3), 0.01 * k) @ R
    q0 = quat_from_rot(R0)
    return dict(X1c=X1.astype(np.float32), X2c=X2.astype(np.float32), obs1=obs1.astype(np.float32), obs2=obs2.astype(np.float32),
                inv_sigma2_1=(1.0 / 1.44 ** oct1).astype(np.float32), inv_sigma2_2=(1.0 / 1.44 ** oct2).astype(np.float32), K1=K_A, K2=K_B,
                q12=q0 / np.linalg.norm(q0), t12=t + 0.02 * k * rng.normal(size=3), s12=np.float64(s if fix_scale else s * (1 + 0.01 * k)),
                th2=np.float32(TH2), fix_scale=fix_scale, planted=dict(R=R, t=t, s=s), oct1=oct1.astype(np.int32), oct2=oct2.astype(np.int32))


_CASES = {}


def generator_case(seed):
    """the batch of BATCH for `seed`: problems, want (the restatement's results), resolution per problem, and how many candidate
    problems were dropped because a decision chi2 came within MARGIN of th2 (of how many drawn).  Computed once per process."""
    if seed in _CASES:
        return _CASES[seed]
    problems, want, res, dropped, drawn = [], [], [], 0, 0
    for k, (n, n_out, fix, far) in enumerate(BATCH):
        for j in range(16):
            drawn += 1
            P = problem(np.random.default_rng([seed, k, j]), n, n_out, fix, far)
            w = optimize_sim3(P)
            if w["margin"] >= MARGIN:
                break
            dropped += 1
        else:
            raise RuntimeError("no candidate of problem %d keeps the decision margin" % k)
        r, same_dec = resolution(P, w) if n else (0.0, True)
        if not same_dec:
            raise RuntimeError("problem %d: the re-associations disagree on a decision" % k)
        problems.append(P)
        want.append(w)
        res.append(r)
    _CASES[seed] = dict(problems=problems, want=want, resolution=res, dropped=dropped, drawn=drawn)
    return _CASES[seed]
