"""CPU restatement of Sim3Solver (src/Sim3Solver.cc: SetRansacParameters :114-138, iterate :140-207, ComputeCentroid :215-224,
ComputeSim3 :226-337, CheckInliers :340-364, Project :382-403, FromCameraToImage :405-423) for the Sim3 RANSAC tests, written from
the reference's lines and the OpenCV conventions of DESIGN.md section 2 item 9.  It does not call the library.

The closed form of one hypothesis is scalar Python: float32 values are carried as Python floats that are exactly representable in
float32 and a float operation is the double operation rounded once more (`f32`), which for + - * / and sqrt of float32 operands IS
the float operation (53 >= 2 * 24 + 2 bits).  The inlier test of one hypothesis over all correspondences is numpy: float32 arrays
for the float operations, float64 arrays rounded once where the convention accumulates in double.

Also here: the seeded generator the CPU and GPU tests share, and the comparison of a result with the reference."""
import math
import struct

import numpy as np

FLT_EPSILON = 2.0 ** -23
DBL_EPSILON = 2.0 ** -52
INT_MIN = -2 ** 31
NAN, INF = float("nan"), float("inf")


def f32(x):
    try:
        return struct.unpack("f", struct.pack("f", x))[0]
    except OverflowError:
        return math.copysign(INF, x)


def ddiv(a, b):
    """IEEE double division (Python raises on a zero divisor)"""
    if b == 0 and not math.isnan(b):
        if a == 0 or math.isnan(a):
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def _cos(x):
    return NAN if math.isinf(x) else math.cos(x)


def _sin(x):
    return NAN if math.isinf(x) else math.sin(x)


# ---------------------------------------------------------------------------------------------- SetRansacParameters, the draws
def ransac_max_its(n, probability, min_inliers, max_iterations):
    """:125-135.  epsilon is a float; pow / log / ceil are the double functions; a quotient that is no int converts as the x86
    instruction does it for the reference (INT_MIN)"""
    if n == 0:
        epsilon = NAN if min_inliers == 0 else math.copysign(INF, min_inliers)
    else:
        epsilon = f32(min_inliers / n)
    if min_inliers == n:
        n_iterations = 1
    else:
        num = math.log(1 - probability) if probability < 1 else (-INF if probability == 1 else NAN)
        arg = 1 - epsilon ** 3 if math.isfinite(epsilon) else (NAN if math.isnan(epsilon) else -epsilon)
        den = math.log(arg) if arg > 0 else (-INF if arg == 0 else NAN)
        v = ddiv(num, den)
        n_iterations = int(math.ceil(v)) if math.isfinite(v) and -2.0 ** 31 <= math.ceil(v) <= 2.0 ** 31 - 1 else INT_MIN
    return max(1, min(n_iterations, max_iterations))


def random_int(rng, lo, hi):
    """DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50), rand() drawn from the numpy Generator `rng`"""
    d = hi - lo + 1
    return int((float(rng.integers(0, 2 ** 31)) / (2147483647.0 + 1.0)) * d) + lo


def draws_for(rng, n, max_iterations):
    d = np.zeros((max_iterations, 3), np.int32)
    if n >= 3:
        for k in range(max_iterations):
            for i in range(3):
                d[k, i] = random_int(rng, 0, n - 1 - i)
    return d


def triple_literal(n, draws):
    """:163-177 as written: vAvailableIndices = mvAllIndices, swap with the back, pop"""
    avail = list(range(n))
    out = []
    for r in draws:
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return tuple(out)


def triple(n, r0, r1, r2):
    """the closed form of the same removal"""
    i0 = r0
    i1 = n - 1 if r1 == r0 else r1
    back2 = n - 1 if r0 == n - 2 else n - 2
    i2 = back2 if r2 == r1 else (n - 1 if r2 == r0 else r2)
    return i0, i1, i2


# ---------------------------------------------------------------------------------------------- cv::eigen (JacobiImpl_<float>)
def _hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = f32(b / a)
        return f32(a * f32(math.sqrt(f32(1 + f32(b * b)))))
    if b > 0:
        a = f32(a / b)
        return f32(b * f32(math.sqrt(f32(1 + f32(a * a)))))
    return 0.0


def jacobi_eigen(N):
    """cv::eigen on a symmetric float n x n (OpenCV 3.2 core/src/lapack.cpp, JacobiImpl_<float>): the classical Jacobi that rotates
    the largest off-diagonal element, found through the per-row / per-column maxima indR / indC -> (eigenvalues descending,
    eigenvectors in ROWS, rotations made)"""
    n = len(N)
    A = [[f32(v) for v in row] for row in N]
    V = [[1.0 if i == j else 0.0 for j in range(n)] for i in range(n)]
    W = [A[k][k] for k in range(n)]
    indR, indC = [0] * n, [0] * n

    def track(idx):
        if idx < n - 1:
            m, mv = idx + 1, abs(A[idx][idx + 1])
            for i in range(idx + 2, n):
                val = abs(A[idx][i])
                if mv < val:
                    mv, m = val, i
            indR[idx] = m
        if idx > 0:
            m, mv = 0, abs(A[0][idx])
            for i in range(1, idx):
                val = abs(A[i][idx])
                if mv < val:
                    mv, m = val, i
            indC[idx] = m

    for k in range(n):
        track(k)
    rotations = 0
    for _ in range(n * n * 30):
        k, mv = 0, abs(A[0][indR[0]])
        for i in range(1, n - 1):
            val = abs(A[i][indR[i]])
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[indC[i]][i])
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[k][l]
        if abs(p) <= FLT_EPSILON:
            break
        y = f32(f32(W[l] - W[k]) * 0.5)
        t = f32(abs(y) + _hypot(p, y))
        s = _hypot(p, t)
        c = f32(t / s)
        s = f32(p / s)
        t = f32(f32(p / t) * p)
        if y < 0:
            s, t = -s, -t
        A[k][l] = 0.0
        W[k] = f32(W[k] - t)
        W[l] = f32(W[l] + t)

        def rot(a0, b0):
            return f32(f32(a0 * c) - f32(b0 * s)), f32(f32(a0 * s) + f32(b0 * c))

        for i in range(k):
            A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l):
            A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n):
            A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n):
            V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        track(k)
        track(l)
        rotations += 1
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return W, V, rotations


# ---------------------------------------------------------------------------------------------- ComputeSim3
def _centroid(P):
    third = f32(1.0 / 3)
    C = [f32(f32(f32(P[r][0] + P[r][1]) + P[r][2]) * third) for r in range(3)]
    return [[f32(P[r][i] - C[r]) for i in range(3)] for r in range(3)], C


def horn_N(P1, P2):
    """steps 1-3 of :226-265: P1 / P2 are 3x3 lists whose COLUMN i is point i -> (N 4x4, Pr1, Pr2, O1, O2)"""
    Pr1, O1 = _centroid(P1)
    Pr2, O2 = _centroid(P2)
    M = [[f32((Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1]) + Pr2[i][2] * Pr1[j][2]) for j in range(3)] for i in range(3)]
    N11 = f32(f32(M[0][0] + M[1][1]) + M[2][2])
    N12 = f32(M[1][2] - M[2][1])
    N13 = f32(M[2][0] - M[0][2])
    N14 = f32(M[0][1] - M[1][0])
    N22 = f32(f32(M[0][0] - M[1][1]) - M[2][2])
    N23 = f32(M[0][1] + M[1][0])
    N24 = f32(M[2][0] + M[0][2])
    N33 = f32(f32(-M[0][0] + M[1][1]) - M[2][2])
    N34 = f32(M[1][2] + M[2][1])
    N44 = f32(f32(-M[0][0] - M[1][1]) + M[2][2])
    N = [[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]
    return N, Pr1, Pr2, O1, O2


def rodrigues(vec):
    rx, ry, rz = vec
    theta = math.sqrt((rx * rx + ry * ry) + rz * rz)
    if theta < DBL_EPSILON:
        return [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    c, s = _cos(theta), _sin(theta)
    c1, itheta = 1.0 - c, (ddiv(1.0, theta) if theta else 0.0)
    rx, ry, rz = rx * itheta, ry * itheta, rz * itheta
    rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
    r_x = [0.0, -rz, ry, rz, 0.0, -rx, -ry, rx, 0.0]
    return [f32((c * (1.0 if k % 4 == 0 else 0.0) + c1 * rrt[k]) + s * r_x[k]) for k in range(9)]


def horn(pts1, pts2, fix_scale):
    """ComputeSim3 for three points of each set (pts[i] = point i) -> dict R [9], t [3], s, T12 [12], T21 [12] (rows 0-2), N, q"""
    P1 = [[float(pts1[i][r]) for i in range(3)] for r in range(3)]
    P2 = [[float(pts2[i][r]) for i in range(3)] for r in range(3)]
    N, Pr1, Pr2, O1, O2 = horn_N(P1, P2)
    _, V, rotations = jacobi_eigen(N)
    q = V[0]
    nrm = math.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
    ang = math.atan2(nrm, q[0])
    f = f32((2 * ang) * ddiv(1.0, nrm))
    vec = [f32(q[1] * f), f32(q[2] * f), f32(q[3] * f)]
    R = rodrigues(vec)
    if not fix_scale:
        nom = den = 0.0
        for i in range(3):
            for j in range(3):
                P3 = f32((R[3 * i] * Pr2[0][j] + R[3 * i + 1] * Pr2[1][j]) + R[3 * i + 2] * Pr2[2][j])
                nom += Pr1[i][j] * P3
                den += f32(P3 * P3)
        s = f32(ddiv(nom, den))
    else:
        s = 1.0
    sinv = f32(ddiv(1.0, s))
    t = [f32(O1[i] - s * ((R[3 * i] * O2[0] + R[3 * i + 1] * O2[1]) + R[3 * i + 2] * O2[2])) for i in range(3)]
    T12, T21, sRinv = [0.0] * 12, [0.0] * 12, [0.0] * 9
    for i in range(3):
        for j in range(3):
            T12[4 * i + j] = f32(R[3 * i + j] * s)
            sRinv[3 * i + j] = T21[4 * i + j] = f32(R[3 * j + i] * sinv)
        T12[4 * i + 3] = t[i]
    for i in range(3):
        T21[4 * i + 3] = f32(-((sRinv[3 * i] * t[0] + sRinv[3 * i + 1] * t[1]) + sRinv[3 * i + 2] * t[2]))
    return dict(R=R, t=t, s=s, T12=T12, T21=T21, N=N, q=q, rotations=rotations)


# ---------------------------------------------------------------------------------------------- CheckInliers (numpy over the points)
def _to_image(K, X, Y, Z):
    fx, fy, cx, cy = (np.float32(v) for v in K)
    invz = np.float32(1) / Z
    x, y = X * invz, Y * invz
    return fx * x + cx, fy * y + cy


def _project(T, K, P):
    T = [np.float64(v) for v in T]
    P = P.astype(np.float64)
    c = [((((T[4 * i] * P[:, 0] + T[4 * i + 1] * P[:, 1]) + T[4 * i + 2] * P[:, 2]) + T[4 * i + 3])).astype(np.float32) for i in range(3)]
    return _to_image(K, c[0], c[1], c[2])


def errors(model, K1, K2, X1, X2):
    """err1, err2 of :350-354 for every correspondence (float32 arrays)"""
    with np.errstate(all="ignore"):
        p1u, p1v = _to_image(K1, X1[:, 0], X1[:, 1], X1[:, 2])
        p2u, p2v = _to_image(K2, X2[:, 0], X2[:, 1], X2[:, 2])
        q1u, q1v = _project(model["T12"], K1, X2)
        q2u, q2v = _project(model["T21"], K2, X1)
        d = [(p1u - q1u).astype(np.float64), (p1v - q1v).astype(np.float64), (q2u - p2u).astype(np.float64), (q2v - p2v).astype(np.float64)]
        return (d[0] * d[0] + d[1] * d[1]).astype(np.float32), (d[2] * d[2] + d[3] * d[3]).astype(np.float32)


def _margin_ulps(err, max_err):
    """smallest distance of a finite error from its threshold, in float32 units of the last place of the larger of the two"""
    ok = np.isfinite(err)
    if not ok.any():
        return INF
    e, m = err[ok].astype(np.float64), max_err[ok].astype(np.float64)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.maximum(np.abs(e), np.abs(m)).astype(np.float32)).astype(np.float64)
        return float((np.abs(e - m) / ulp).min())


# ---------------------------------------------------------------------------------------------- iterate
def scan_literal(counts, min_inliers):
    """the loop of :158-201 over the counts of the iterations -> (first_success, best_iteration, best_inliers, iterations run)"""
    best_inliers, best_iteration = 0, -1
    for it, c in enumerate(counts):
        if c >= best_inliers:
            best_inliers, best_iteration = c, it
            if c > min_inliers:
                return it, best_iteration, best_inliers, it + 1
    return -1, best_iteration, best_inliers, len(counts)


def solve(P):
    """one problem (a dict as capi.debug_sim3_host takes it) -> the fields of aos2_sim3_result_t, plus what the tests assert about
    the batch: counts_all (every hypothesis up to ransac_max_its), nan_hyps, margin_ulps, models"""
    X1, X2 = np.ascontiguousarray(P["X3Dc1"], np.float32), np.ascontiguousarray(P["X3Dc2"], np.float32)
    e1, e2 = np.ascontiguousarray(P["max_err1"], np.float32), np.ascontiguousarray(P["max_err2"], np.float32)
    n, max_it = len(X1), int(P["max_iterations"])
    its = ransac_max_its(n, P["probability"], P["min_inliers"], max_it)
    out = dict(ransac_max_its=its, first_success=-1, best_iteration=-1, best_inliers=0, T12=np.zeros((4, 4), np.float32),
               R12=np.zeros((3, 3), np.float32), t12=np.zeros(3, np.float32), s12=np.float32(0), inliers=np.zeros(n, np.uint8),
               counts=np.full(max_it, -1, np.int32), counts_all=np.zeros(0, np.int32), nan_hyps=[], margin_ulps=INF, models=[])
    if n < P["min_inliers"]:
        return out
    draws = np.asarray(P["draws"], np.int32)
    counts_all, flags_all, models, margin = [], [], [], INF
    for it in range(its):
        idx = triple(n, *(int(v) for v in draws[it]))
        m = horn([X1[i] for i in idx], [X2[i] for i in idx], P["fix_scale"])
        err1, err2 = errors(m, P["K1"], P["K2"], X1, X2)
        flags = (err1 < e1) & (err2 < e2)
        margin = min(margin, _margin_ulps(err1, e1), _margin_ulps(err2, e2))
        counts_all.append(int(flags.sum()))
        flags_all.append(flags)
        models.append(m)
        if any(math.isnan(v) for v in m["T12"] + m["T21"]):
            out["nan_hyps"].append(it)
    first, best, best_inl, ran = scan_literal(counts_all, P["min_inliers"])
    m = models[best]
    T12 = np.eye(4, dtype=np.float32)
    T12[:3] = np.array(m["T12"], np.float32).reshape(3, 4)
    out.update(first_success=first, best_iteration=best, best_inliers=best_inl, T12=T12, R12=np.array(m["R"], np.float32).reshape(3, 3),
               t12=np.array(m["t"], np.float32), s12=np.float32(m["s"]), inliers=flags_all[best].astype(np.uint8),
               counts_all=np.array(counts_all, np.int32), margin_ulps=margin, models=models)
    out["counts"][:ran] = counts_all[:ran]
    return out


def same(got, want):
    """the comparison of a result of the library with the reference: integers, counts and flags exactly; T12 / R12 / t12 / s12 bit for
    bit where finite, NaN in the same places"""
    for k in ("ransac_max_its", "first_success", "best_iteration", "best_inliers"):
        if int(got[k]) != int(want[k]):
            return False
    if not (np.array_equal(got["counts"], want["counts"]) and np.array_equal(got["inliers"], want["inliers"])):
        return False
    for k in ("T12", "R12", "t12", "s12"):
        g, w = np.asarray(got[k], np.float32).ravel(), np.asarray(want[k], np.float32).ravel()
        nan = np.isnan(w)
        if not (np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan].view(np.uint32), w[~nan].view(np.uint32))):
            return False
    return True


# ---------------------------------------------------------------------------------------------- the generator
K_A = (520.9, 521.0, 325.1, 249.7)
K_B = (535.4, 539.2, 320.1, 247.6)
SIZES = (19, 20, 21, 65, 130, 300, 40, 30)   # the last: three points with equal coordinates and one with z = 0
OUTLIER_SHARE = (0.0, 0.0, 0.0, 0.5, 0.3, 0.2, 1.0, 0.2)
NOISE_M = 0.01
MIN_INLIERS, MAX_ITERATIONS, PROBABILITY = 20, 300, 0.99


def level_sigma2(n_levels=8, scale_factor=1.2):
    """mvLevelSigma2[i] = mvScaleFactor[i] * mvScaleFactor[i] in float (src/ORBextractor.cc:416-421)"""
    sf = [1.0]
    for _ in range(1, n_levels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return [f32(v * v) for v in sf]


def _rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


def _box(rng, n):
    """points in a 4 x 3 x 6.5 m box, 1.5 to 8 m deep"""
    return np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(1.5, 8.0, n)], 1)


def problem(rng, n, outlier_share, scale, noise=NOISE_M):
    """a planted Sim3 (X1 = s R X2 + t: rotation 0.2-0.5 rad, translation a few decimetres), `outlier_share` of the correspondences
    replaced by unrelated points, octaves 0-7"""
    R = _rotation(rng.normal(size=3), rng.uniform(0.2, 0.5))
    t = rng.uniform(-0.4, 0.4, 3)
    X1 = _box(rng, n)
    X2 = (X1 - t) @ R / scale          # R^T (X1 - t) / s
    n_out = int(round(outlier_share * n))
    out = rng.permutation(n)[:n_out]
    X2[out] = _box(rng, n_out)
    X1n, X2n = X1 + rng.normal(scale=noise, size=X1.shape), X2 + rng.normal(scale=noise, size=X2.shape)
    s2 = level_sigma2()
    oct1, oct2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    return dict(X3Dc1=X1n.astype(np.float32), X3Dc2=X2n.astype(np.float32),
                max_err1=np.array([f32(9.210 * s2[o]) for o in oct1], np.float32), max_err2=np.array([f32(9.210 * s2[o]) for o in oct2], np.float32),
                K1=K_A, K2=K_B, fix_scale=scale == 1.0, probability=PROBABILITY, min_inliers=MIN_INLIERS, max_iterations=MAX_ITERATIONS,
                planted=dict(R=R, t=t, s=scale), outliers=np.sort(out))


_cases = {}


def generator_case(seed):
    """the batch of problems the CPU and GPU tests share (SIZES) with their draws and the reference's results: dict problems, want.
    Computed once per seed and never modified by the tests."""
    if seed in _cases:
        return _cases[seed]
    rng = np.random.default_rng(seed)
    problems = []
    for k, (n, share) in enumerate(zip(SIZES, OUTLIER_SHARE)):
        P = problem(rng, n, share, 1.0 if k % 2 == 0 else 1.3)
        if k == len(SIZES) - 1:
            P["X3Dc1"][1] = P["X3Dc1"][2] = P["X3Dc1"][0]
            P["X3Dc2"][1] = P["X3Dc2"][2] = P["X3Dc2"][0]
            P["X3Dc1"][3, 2] = 0.0
        P["draws"] = draws_for(rng, n, MAX_ITERATIONS)
        if k == len(SIZES) - 1:
            P["draws"][1] = (0, 1, 2)      # the three equal points: Pr = 0, norm(vec) = 0, a model of NaNs
        problems.append(P)
    _cases[seed] = dict(problems=problems, want=[solve(P) for P in problems])
    return _cases[seed]
