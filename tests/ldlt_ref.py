"""CPU reference for the reduced-system solve of LocalBA (csrc/ldlt_reg.h: ldlt_reg_solve, csrc/lba.hip: ldlt_body), both an unpivoted
dense LDL^T + two substitutions that fail on a zero / NaN pivot only (Eigen::SimplicialLDLT's rule).  It does not call the library.

* `ldlt_solve(H, b, dtype)`: the textbook right-looking recurrence, vectorised by outer products; with numpy.longdouble (64-bit
  significand, eps 1.08e-19) it is THE reference, with float64 it is the "plain" model.
* `blocked_f64(H, b)`: a float64 model of the kernels' blocked form -- 16-wide panels over the matrix padded with an identity tail,
  explicit T_k = L_kk^-1, W = A T_k^T, L = W (1 / d), A -= W L^T, y_k = T_k r_k, x_k = T_k^T (z_k - sum L_Ik^T x_I).
  The two float64 models exist to show, without a GPU, that the condition below can be met by float64 arithmetic of this shape.
* `omega(H, b, x, L, d)`: the componentwise backward error of x in units of the bound of an unpivoted LDL^T solve in float64,

      omega = max_i |b - H x|_i / ((3 n + 1) 2^-53 (|L| |D| |L|^T |x|)_i)

  (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.4 with |L||D||L|^T for |R|^T|R|: the computed solution
  solves (H + dH) x = b with |dH| <= gamma_{3n+1} |L||D||L|^T), with L, d from the long double factorisation and the residual formed
  in long double.  A correct float64 solve has omega <= 1 whatever the conditioning or scaling; an error in one tile shows in its rows.
* seeded generators, one per family, and `gpu_systems()`: the systems tests/test_lba_reduced_gpu.py runs, which
  tests/test_ldlt_ref_cpu.py runs through both float64 models."""
import numpy as np

LD = np.longdouble
U64 = 2.0 ** -53
REG_NP = tuple(range(1, 41))                                  # k_ldlt_reg: every size it takes (nb = 1..15)
DEV_NP = (1, 2, 3, 5, 8, 16, 24, 40, 41, 43, 48, 56, 64)      # k_ldlt_dev
ALL_NP = tuple(sorted(set(REG_NP) | set(DEV_NP)))
FLOAT_FAMILIES = ("bench", "graded", "lm", "indef")


def ldlt_solve(H, b, dtype=LD):
    """(L, d, x) of the unpivoted LDL^T solve in `dtype`, or None on a zero / NaN pivot"""
    A = np.array(H, dtype)
    n = A.shape[0]
    L = np.eye(n, dtype=dtype)
    d = np.zeros(n, dtype)
    for j in range(n):
        dj = A[j, j]
        if dj == 0 or dj != dj:
            return None
        d[j] = dj
        col = A[j + 1:, j].copy()
        lj = col / dj
        L[j + 1:, j] = lj
        A[j + 1:, j + 1:] -= np.outer(lj, col)
    r = np.array(b, dtype)
    for j in range(n):              # L y = b
        r[j + 1:] -= L[j + 1:, j] * r[j]
    r = r / d
    for j in range(n - 1, -1, -1):  # L^T x = D^-1 y
        r[:j] -= L[j, :j] * r[j]
    return L, d, r


def blocked_f64(H, b, bs=16):
    """float64 model of the kernels' blocked form -> (L, d, x) of the leading n x n part, or None on a zero / NaN pivot"""
    n = len(b)
    npad = -(-n // bs) * bs
    nb = npad // bs
    A = np.eye(npad)
    A[:n, :n] = H
    r = np.zeros(npad)
    r[:n] = b
    L = np.eye(npad)
    d = np.zeros(npad)
    z = np.zeros(npad)
    x = np.zeros(npad)
    Ts = []
    for k in range(nb):
        s = slice(bs * k, bs * k + bs)
        lo = slice(bs * k + bs, npad)
        D = A[s, s].copy()
        T = np.eye(bs)
        for j in range(bs):
            dj = D[j, j]
            if dj == 0 or dj != dj:
                return None
            rd = 1.0 / dj
            col = D[j + 1:, j].copy()
            L[bs * k + j + 1:bs * k + bs, bs * k + j] = col * rd
            D[j + 1:, j + 1:] -= np.outer(col * rd, col)
            T[j + 1:, :] -= np.outer(col, rd * T[j, :])   # T <- (I - l_j e_j^T) T
            d[bs * k + j] = dj
        Ts.append(T)
        rdk = 1.0 / d[s]
        z[s] = (T @ r[s]) * rdk
        if k < nb - 1:
            W = A[lo, s] @ T.T
            Lk = W * rdk[None, :]
            L[lo, s] = Lk
            r[lo] -= W @ z[s]
            A[lo, lo] -= W @ Lk.T
    for k in range(nb - 1, -1, -1):
        s = slice(bs * k, bs * k + bs)
        lo = slice(bs * k + bs, npad)
        x[s] = Ts[k].T @ (z[s] - L[lo, s].T @ x[lo])
    return L[:n, :n], d[:n], x[:n]


def omega(H, b, x, L, d):
    """(omega, row of the maximum) of a float64 solution x; L, d: the long double factors.  inf for a non-finite x."""
    n = len(b)
    x = np.asarray(x, np.float64)
    if not np.isfinite(x).all():
        return np.inf, int(np.argmax(~np.isfinite(x)))
    xl = x.astype(LD)
    res = np.abs(np.asarray(b, np.float64).astype(LD) - (np.asarray(H, np.float64).astype(LD) * xl[None, :]).sum(1))
    aL = np.abs(L)
    den = LD((3 * n + 1) * U64) * ((aL * (np.abs(d) * (aL.T * np.abs(xl)[None, :]).sum(1))[None, :]).sum(1))
    q = np.where(res == 0, LD(0), res / np.where(den == 0, LD(1), den))
    q = np.where((den == 0) & (res != 0), LD(np.inf), q)
    i = int(np.argmax(q))
    return float(q[i]), i


# ---------------------------------------------------------------------------------------------------- generators: (H, b), seeded
def gen_bench(rng, n):
    """the recipe of tools/microbench/ldlt_reg_bench.hip: G G^T / n * 50 + diag(1 + 100 |r|)"""
    G = rng.normal(size=(n, n))
    H = G @ G.T / n * 50 + np.diag(1 + 100 * np.abs(rng.normal(size=n)))
    return (H + H.T) / 2, rng.normal(size=n)


def gen_graded(rng, n):
    """A^T A with column scales 10^U(-2, 3) (the scaling of the pose-block test) + 10^U(-8, 2) I: cond up to 1e12"""
    A = rng.normal(size=(n, n)) * 10.0 ** rng.uniform(-2, 3, n)[None, :]
    H = A.T @ A + 10.0 ** rng.uniform(-8, 2) * np.eye(n)
    H = (H + H.T) / 2
    return H, rng.normal(size=n) * np.sqrt(np.diag(H))


def gen_lm(rng, n):
    """a gauge-deficient system under a small damping: A^T A with n - min(7, n - 1) rows + 1e-7 I"""
    A = rng.normal(size=(n - min(7, n - 1), n))
    H = A.T @ A + 1e-7 * np.eye(n)
    return (H + H.T) / 2, A.T @ rng.normal(size=A.shape[0])


def gen_indef(rng, n):
    """(L D) L^T, L unit lower with entries U(-0.3, 0.3), D = +- 10^U(-1, 1): indefinite, no zero pivot"""
    L = np.tril(rng.uniform(-0.3, 0.3, (n, n)), -1) + np.eye(n)
    D = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-1, 1, n)
    H = (L * D[None, :]) @ L.T
    return (H + H.T) / 2, rng.normal(size=n)


def gen_dyadic(rng, n, zero_at=None):
    """-> (H, b, x0, L, D): L unit lower with two entries of +-1 per row at random earlier columns, D in +-{0.5, 1, 2, 4} (0 at
    zero_at), integer x0 in [-8, 8], H = L D L^T and b = H x0 formed exactly: every intermediate of an elimination in any order is a
    small dyadic number and every reciprocal pivot a power of two, so a correct float64 solve returns x0 bit for bit"""
    L = np.eye(n)
    for i in range(1, n):
        for c in rng.choice(i, size=min(i, 2), replace=False):
            L[i, c] = rng.choice([-1.0, 1.0])
    D = rng.choice([-1.0, 1.0], n) * rng.choice([0.5, 1.0, 2.0, 4.0], n)
    if zero_at is not None:
        D[zero_at] = 0.0
    x0 = rng.integers(-8, 9, n).astype(np.float64)
    H = (L * D[None, :]) @ L.T
    assert (H == H.T).all()
    return H, H @ x0, x0, L, D


GEN = dict(bench=gen_bench, graded=gen_graded, lm=gen_lm, indef=gen_indef)


def system(family, np_):
    """the system of (family, free keyframes): the same for both kernels and for the CPU models"""
    rng = np.random.default_rng([FLOAT_FAMILIES.index(family), np_, 20240])
    return GEN[family](rng, 6 * np_)


def dyadic_system(np_, zero_at=None, seed=0):
    return gen_dyadic(np.random.default_rng([77, np_, seed]), 6 * np_, zero_at)


_ref_cache = {}


def reference(family, np_):
    """(H, b, L, d) with the long double factors of system(family, np_), computed once per process"""
    key = (family, np_)
    if key not in _ref_cache:
        H, b = system(family, np_)
        L, d, _ = ldlt_solve(H, b, LD)
        _ref_cache[key] = (H, b, L, d)
    return _ref_cache[key]


def gpu_systems():
    """(family, np, forms) of every float system the GPU test runs: form 2 = k_ldlt_reg, 0 = k_ldlt_dev"""
    return [(f, q, tuple(fm for fm, sizes in ((2, REG_NP), (0, DEV_NP)) if q in sizes)) for f in FLOAT_FAMILIES for q in ALL_NP]


def lba_star_window(q):
    """a LocalBA problem (the dict capi.LocalBA takes) with q free keyframes: one fixed keyframe, q map points, point i seen by free
    keyframe i and by the fixed one -- for the tests of the size limit, which is decided on the host before anything is solved"""
    T = np.tile(np.eye(4, dtype=np.float32).reshape(16), (q + 1, 1))
    pts = np.stack([np.linspace(-2, 2, q), np.zeros(q), np.full(q, 10.0)], 1).astype(np.float32)
    ep = np.concatenate([np.arange(q), np.full(q, q)]).astype(np.int32)
    pt = np.concatenate([np.arange(q), np.arange(q)]).astype(np.int32)
    obs = np.stack([600 + 70 * pts[pt, 0], np.full(2 * q, 180.0), np.full(2 * q, -1.0)], 1).astype(np.float32)
    return dict(n_poses=q + 1, n_points=q, n_edges=2 * q, pose_Tcw=T, pose_fixed=np.array([0] * q + [1], np.uint8),
                pose_id=np.arange(1, q + 2, dtype=np.int64), point_xyz=pts, point_id=np.arange(q, dtype=np.int64), edge_pose=ep,
                edge_point=pt, edge_obs=obs, edge_stereo=np.zeros(2 * q, np.uint8), edge_inv_sigma2=np.ones(2 * q, np.float32),
                fx=700.0, fy=700.0, cx=600.0, cy=180.0, bf=380.0)
