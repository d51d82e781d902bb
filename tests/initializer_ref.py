"""An independent restatement of Initializer::Initialize (src/Initializer.cc) with numpy float32 / float64 values, written from the
reference's source and DESIGN.md section 2 item 12, not from csrc/initializer.h.  Every rounding is explicit: a float32 array
operation rounds once per element, a double one is spelled with float64 arrays.  Where the reference loops over independent things
(the RANSAC iterations, the matches of CheckRT) the restatement carries them as a leading array axis; every SUM keeps the
reference's order (a Python loop over the summed index).

solve(problem) -> the fields of aos2_initializer_result_t, plus margin_ulps: how close the nearest decision of the run comes to its
threshold, in float32 ulps of the threshold (the generator condition of the tests), and margins: the same per kind of decision."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
TH_H, TH_F = f32(5.991), f32(3.841)
FLT_EPSILON, FLT_MIN = f32(np.finfo(np.float32).eps), f64(np.finfo(np.float32).tiny)
CV_PI = 3.1415926535897932384626433832795


# ----------------------------------------------------------------------------------------------------------------- OpenCV pieces
def rng_values(n, seed=0x12345678):
    """cv::RNG(seed).next(): state = (uint32)state * 4164903690 + (state >> 32), the low 32 bits"""
    state, out = seed, []
    for _ in range(n):
        state = ((state & 0xFFFFFFFF) * 4164903690 + (state >> 32)) & 0xFFFFFFFFFFFFFFFF
        out.append(state & 0xFFFFFFFF)
    return out


class Rng:
    def __init__(self, seed=0x12345678):
        self.state = seed

    def next(self):
        self.state = ((self.state & 0xFFFFFFFF) * 4164903690 + (self.state >> 32)) & 0xFFFFFFFFFFFFFFFF
        return self.state & 0xFFFFFFFF


def dsum_sq(rows):
    """sum over the last axis of (double)t * t, in index order"""
    r = rows.astype(f64)
    s = np.zeros(r.shape[:-1], f64)
    for k in range(r.shape[-1]):
        s = s + r[..., k] * r[..., k]
    return s


def jacobi_batch(At):
    """JacobiSVDImpl_<float> up to and including the sort, for a batch: At [b][n][m] float32 (n rows of length m).
    -> (At, W [b][n] float64 = the row norms, V [b][n][n]) sorted into descending W.  A lane whose sweep made no rotation makes
    none in later sweeps either (nothing changed), so the batch runs until every lane is still."""
    At = np.array(At, f32)
    b, n, m = At.shape
    V = np.zeros((b, n, n), f32)
    V[:, np.arange(n), np.arange(n)] = 1
    W = dsum_sq(At)
    eps = f64(FLT_EPSILON * f32(2))
    with np.errstate(all="ignore"):
        for _ in range(30):
            changed = np.zeros(b, bool)
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a, c_ = W[:, i], W[:, j]
                    Ai, Aj = At[:, i].astype(f64), At[:, j].astype(f64)
                    p = np.zeros(b, f64)
                    for k in range(m):
                        p = p + Ai[:, k] * Aj[:, k]
                    rot = ~(np.abs(p) <= eps * np.sqrt(a * c_))   # (`continue` on <=: a NaN rotates)
                    if not rot.any():
                        continue
                    p = p * 2
                    beta = a - c_
                    gamma = np.sqrt(p * p + beta * beta)
                    neg = beta < 0
                    s_n = np.sqrt(((gamma - beta) * 0.5) / gamma).astype(f32)
                    c_n = (p / (gamma * s_n.astype(f64) * 2)).astype(f32)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2)).astype(f32)
                    s_p = (p / (gamma * c_p.astype(f64) * 2)).astype(f32)
                    c, s = np.where(neg, c_n, c_p)[:, None], np.where(neg, s_n, s_p)[:, None]
                    x, y = At[:, i].copy(), At[:, j].copy()
                    t0 = c * x + s * y
                    t1 = -s * x + c * y
                    At[:, i] = np.where(rot[:, None], t0, x)
                    At[:, j] = np.where(rot[:, None], t1, y)
                    W[:, i] = np.where(rot, dsum_sq(t0), W[:, i])
                    W[:, j] = np.where(rot, dsum_sq(t1), W[:, j])
                    x, y = V[:, i].copy(), V[:, j].copy()
                    V[:, i] = np.where(rot[:, None], c * x + s * y, x)
                    V[:, j] = np.where(rot[:, None], -s * x + c * y, y)
                    changed |= rot
            if not changed.any():
                break
        W = np.sqrt(dsum_sq(At))
    lanes = np.arange(b)
    for i in range(n - 1):
        j = np.full(b, i)
        for k in range(i + 1, n):
            j = np.where(W[lanes, j] < W[:, k], k, j)
        for M in (W, At, V):
            ti, tj = M[:, i].copy(), M[lanes, j].copy()
            M[:, i] = tj
            M[lanes, j] = ti
    return At, W, V


def svd_tail(At, W, m, n, n1):
    """the tail loop of JacobiSVDImpl_ for ONE matrix: At [n1][m] float32 (rows >= n are filled here), W [n] float64"""
    rng = Rng()
    eps = FLT_EPSILON * f32(2)
    with np.errstate(all="ignore"):
        for i in range(n1):
            sd = f64(W[i]) if i < n else f64(0)
            ii = 0
            while ii < 100 and sd <= FLT_MIN:
                val0 = f32(f64(1.) / f64(m))
                for k in range(m):
                    At[i, k] = val0 if (rng.next() & 256) != 0 else -val0
                for _ in range(2):
                    for j in range(i):
                        sd = f64(0)
                        for k in range(m):
                            sd = sd + f64(At[i, k] * At[j, k])          # a float product, widened
                        asum = f32(0)
                        for k in range(m):
                            t = f32(f64(At[i, k]) - sd * f64(At[j, k]))
                            At[i, k] = t
                            asum = asum + np.abs(t)
                        asum = f32(1) / asum if asum > eps * f32(100) else f32(0)
                        for k in range(m):
                            At[i, k] = At[i, k] * asum
                sd = f64(0)
                for k in range(m):
                    sd = sd + f64(At[i, k]) * f64(At[i, k])
                sd = np.sqrt(sd)
                ii += 1
            s = f32(f64(1) / sd if sd > FLT_MIN else f64(0))
            At[i] = At[i] * s
    return At


def svd_general(A):
    """cv::SVDecomp(A, w, u, vt, FULL_UV) of one float matrix, rows >= cols: At = A^T.  -> (left [n][m], w float64 [n], V [n][n]);
    u[i][k] = left[k][i], vt = V"""
    A = np.asarray(A, f32)
    m, n = A.shape
    At, W, V = jacobi_batch(A.T[None].copy())
    return svd_tail(At[0], W[0], m, n, n), W[0], V[0]


def svd_wide(A):
    """the same for rows < cols: OpenCV swaps the roles, the Jacobi runs on the rows of A itself; vt = the left factor completed to
    cols rows.  -> (vt [cols][cols], w, V [rows][rows])"""
    A = np.asarray(A, f32)
    n, m = A.shape
    At, W, V = jacobi_batch(A[None].copy())
    full = np.zeros((m, m), f32)
    full[:n] = At[0]
    return svd_tail(full, W[0], m, n, m), W[0], V[0]


def svd33(M):
    """-> (u, w float32, vt) of a general float 3x3"""
    left, W, V = svd_general(M)
    return left.T.copy(), W.astype(f32), V


def gemm(A, B, alpha=None, add=None):
    """cv::gemm on float matrices (leading axes broadcast): products and sums in double in index order, alpha and the addend applied
    in double, one rounding"""
    A64, B64 = np.asarray(A, f32).astype(f64), np.asarray(B, f32).astype(f64)
    s = None
    with np.errstate(all="ignore"):
        for k in range(A64.shape[-1]):
            t = A64[..., :, k, None] * B64[..., None, k, :]
            s = t if s is None else s + t
        if alpha is not None:
            s = f64(alpha) * s
        if add is not None:
            s = s + np.asarray(add, f32).astype(f64)
        return s.astype(f32)


def det33(M):
    """cv::determinant of a float 3x3 (leading axes allowed): in double, returned as the double"""
    m = np.asarray(M, f32).astype(f64)
    with np.errstate(all="ignore"):
        return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1]) -
                m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0]) +
                m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def inv33(M):
    """cv::Mat::inv() of a float 3x3 (leading axes allowed): adjugate terms as double products times 1/det, rounded once; the zero
    matrix where det == 0"""
    S = np.asarray(M, f32).astype(f64)
    d = det33(M)
    with np.errstate(all="ignore"):
        r = f64(1.) / d
        e = lambda i, j: S[..., i, j]   # noqa: E731
        t = [(e(1, 1) * e(2, 2) - e(1, 2) * e(2, 1)) * r, (e(0, 2) * e(2, 1) - e(0, 1) * e(2, 2)) * r, (e(0, 1) * e(1, 2) - e(0, 2) * e(1, 1)) * r,
             (e(1, 2) * e(2, 0) - e(1, 0) * e(2, 2)) * r, (e(0, 0) * e(2, 2) - e(0, 2) * e(2, 0)) * r, (e(0, 2) * e(1, 0) - e(0, 0) * e(1, 2)) * r,
             (e(1, 0) * e(2, 1) - e(1, 1) * e(2, 0)) * r, (e(0, 1) * e(2, 0) - e(0, 0) * e(2, 1)) * r, (e(0, 0) * e(1, 1) - e(0, 1) * e(1, 0)) * r]
        out = np.stack(t, -1).reshape(S.shape).astype(f32)
    out[np.asarray(d == 0)] = 0
    return out


def unit(t):
    """t / cv::norm(t): one scale by the double reciprocal of the double norm"""
    t = np.asarray(t, f32)
    with np.errstate(all="ignore"):
        return (t.astype(f64) * (f64(1.0) / np.sqrt(dsum_sq(t)))).astype(f32)


# ------------------------------------------------------------------------------------------------------------------- the solver
def normalize(keys):
    """Normalize (:749-795) over all keys -> (normalised points [n][2], T)"""
    keys = np.asarray(keys, f32)
    N = len(keys)
    meanX = meanY = f32(0)
    for i in range(N):
        meanX = meanX + keys[i, 0]
        meanY = meanY + keys[i, 1]
    meanX, meanY = meanX / f32(N), meanY / f32(N)
    pts = np.stack([keys[:, 0] - meanX, keys[:, 1] - meanY], 1)
    devX = devY = f32(0)
    for i in range(N):
        devX = devX + np.abs(pts[i, 0])
        devY = devY + np.abs(pts[i, 1])
    devX, devY = devX / f32(N), devY / f32(N)
    with np.errstate(all="ignore"):
        sX, sY = f32(f64(1.0) / f64(devX)), f32(f64(1.0) / f64(devY))
        pts = np.stack([pts[:, 0] * sX, pts[:, 1] * sY], 1)
        T = np.array([[sX, 0, -meanX * sX], [0, sY, -meanY * sY], [0, 0, 1]], f32)
    return pts, T


def compute_h21(p1, p2):
    """ComputeH21 (:226-266) for a batch of sets: p1, p2 [b][8][2] -> Hn [b][3][3]"""
    b = len(p1)
    A = np.zeros((b, 16, 9), f32)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A[:, 0::2, 3], A[:, 0::2, 4], A[:, 0::2, 5] = -u1, -v1, -1
    A[:, 0::2, 6], A[:, 0::2, 7], A[:, 0::2, 8] = v2 * u1, v2 * v1, v2
    A[:, 1::2, 0], A[:, 1::2, 1], A[:, 1::2, 2] = u1, v1, 1
    A[:, 1::2, 6], A[:, 1::2, 7], A[:, 1::2, 8] = -u2 * u1, -u2 * v1, -u2
    _, _, V = jacobi_batch(A.transpose(0, 2, 1).copy())   # tall: At = A^T, vt = the rotations
    return V[:, 8].reshape(b, 3, 3)


def compute_f21(p1, p2, flip_null=False):
    """ComputeF21 (:268-303) for a batch of sets -> Fn [b][3][3]"""
    b = len(p1)
    A = np.zeros((b, 8, 9), f32)
    u1, v1, u2, v2 = p1[..., 0], p1[..., 1], p2[..., 0], p2[..., 1]
    A[..., 0], A[..., 1], A[..., 2] = u2 * u1, u2 * v1, u2
    A[..., 3], A[..., 4], A[..., 5] = v2 * u1, v2 * v1, v2
    A[..., 6], A[..., 7], A[..., 8] = u1, v1, 1
    At, W, _ = jacobi_batch(A)                            # wide: the rows of A itself
    out = np.zeros((b, 3, 3), f32)
    for k in range(b):
        full = np.zeros((9, 9), f32)
        full[:8] = At[k]
        Fpre = svd_tail(full, W[k], 9, 8, 9)[8].reshape(3, 3)
        if flip_null:
            Fpre = -Fpre
        u, w, vt = svd33(Fpre)
        w[2] = 0
        out[k] = gemm(gemm(u, np.diag(w)), vt)
    return out


def reciprocal(x):
    """(float)(1.0 / x) for a float x"""
    with np.errstate(all="ignore"):
        return (f64(1.0) / np.asarray(x, f32).astype(f64)).astype(f32)


def chi_h(H21, H12, u1, v1, u2, v2, invSigmaSquare):
    """the two chi squares of CheckHomography (:337-385); H21, H12 [b][3][3] against matches [N] -> [b][N] each"""
    h, g = H21[:, :, :, None], H12[:, :, :, None]
    with np.errstate(all="ignore"):
        w2in1inv = reciprocal(g[:, 2, 0] * u2 + g[:, 2, 1] * v2 + g[:, 2, 2])
        u2in1 = (g[:, 0, 0] * u2 + g[:, 0, 1] * v2 + g[:, 0, 2]) * w2in1inv
        v2in1 = (g[:, 1, 0] * u2 + g[:, 1, 1] * v2 + g[:, 1, 2]) * w2in1inv
        chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * invSigmaSquare
        w1in2inv = reciprocal(h[:, 2, 0] * u1 + h[:, 2, 1] * v1 + h[:, 2, 2])
        u1in2 = (h[:, 0, 0] * u1 + h[:, 0, 1] * v1 + h[:, 0, 2]) * w1in2inv
        v1in2 = (h[:, 1, 0] * u1 + h[:, 1, 1] * v1 + h[:, 1, 2]) * w1in2inv
        chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * invSigmaSquare
    return chi1, chi2


def chi_f(F21, u1, v1, u2, v2, invSigmaSquare):
    """the two chi squares of CheckFundamental (:413-465)"""
    f = F21[:, :, :, None]
    with np.errstate(all="ignore"):
        a2 = f[:, 0, 0] * u1 + f[:, 0, 1] * v1 + f[:, 0, 2]
        b2 = f[:, 1, 0] * u1 + f[:, 1, 1] * v1 + f[:, 1, 2]
        c2 = f[:, 2, 0] * u1 + f[:, 2, 1] * v1 + f[:, 2, 2]
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invSigmaSquare
        a1 = f[:, 0, 0] * u2 + f[:, 1, 0] * v2 + f[:, 2, 0]
        b1 = f[:, 0, 1] * u2 + f[:, 1, 1] * v2 + f[:, 2, 1]
        c1 = f[:, 0, 2] * u2 + f[:, 1, 2] * v2 + f[:, 2, 2]
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invSigmaSquare
    return chi1, chi2


def ulps_from(values, threshold):
    """the smallest distance of `values` from `threshold` in float32 ulps of the threshold (NaNs and infinities decide nothing)"""
    v = np.asarray(values, f64).ravel()
    v = v[np.isfinite(v)]
    if v.size == 0:
        return math.inf
    return float(np.abs(v - f64(threshold)).min() / f64(np.spacing(f32(threshold))))


def score_and_pick(chi1, chi2, th, th_score):
    """the float score of every iteration, summed in match order (:337-385), and the pick of :165 -> (scores, best, flags of best)"""
    b, N = chi1.shape
    score = np.zeros(b, f32)
    with np.errstate(all="ignore"):
        for i in range(N):
            score = np.where(chi1[:, i] > th, score, score + (th_score - chi1[:, i]))
            score = np.where(chi2[:, i] > th, score, score + (th_score - chi2[:, i]))
    best, best_score = -1, f32(0.0)
    for it in range(b):
        if score[it] > best_score:
            best, best_score = it, score[it]
    flags = np.zeros(N, np.uint8)
    if best >= 0:
        flags = (~(chi1[best] > th) & ~(chi2[best] > th)).astype(np.uint8)
    return score, best, best_score, flags


def check_rt(R, t, K4, keys1, keys2, matches, inliers, th2):
    """CheckRT (:798-907) -> (nGood, parallax, vP3D [n_keys1][3], vbGood [n_keys1], margin)"""
    fx, fy, cx, cy = K4
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)
    n1 = len(keys1)
    vP3D, vbGood = np.zeros((n1, 3), f32), np.zeros(n1, np.uint8)
    P1 = np.zeros((3, 4), f32)
    P1[:, :3] = K
    P2 = gemm(K, np.concatenate([R, t.reshape(3, 1)], 1))
    O2 = gemm(R.T, t.reshape(3, 1), alpha=-1.0).ravel()
    idx = np.nonzero(inliers)[0]
    if len(idx) == 0:
        return 0, f32(0), vP3D, vbGood, dict(cos=math.inf, reproj=math.inf)
    k1, k2 = keys1[matches[idx, 0]], keys2[matches[idx, 1]]
    with np.errstate(all="ignore"):
        # Triangulate (:734-747): A.row(0) = kp1.pt.x * P1.row(2) - P1.row(0) ...: float products, float differences
        A = np.stack([k1[:, 0, None] * P1[2] - P1[0], k1[:, 1, None] * P1[2] - P1[1],
                      k2[:, 0, None] * P2[2] - P2[0], k2[:, 1, None] * P2[2] - P2[1]], 1).astype(f32)
        _, _, V = jacobi_batch(A.transpose(0, 2, 1).copy())
        v = V[:, 3]
        p = v[:, :3] * reciprocal(v[:, 3])[:, None]
        finite = np.isfinite(p).all(1)
        p64 = p.astype(f64)
        dist1 = np.sqrt(dsum_sq(p)).astype(f32)
        nrm2 = p - O2
        dist2 = np.sqrt(dsum_sq(nrm2)).astype(f32)
        dot = np.zeros(len(idx), f64)
        for k in range(3):
            dot = dot + p64[:, k] * nrm2.astype(f64)[:, k]
        cosP = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        low = cosP.astype(f64) < 0.99998
        p2 = gemm(R, p[:, :, None], add=t.reshape(3, 1))[:, :, 0]
        invZ1 = reciprocal(p[:, 2])
        im1x, im1y = fx * p[:, 0] * invZ1 + cx, fy * p[:, 1] * invZ1 + cy
        err1 = (im1x - k1[:, 0]) * (im1x - k1[:, 0]) + (im1y - k1[:, 1]) * (im1y - k1[:, 1])
        invZ2 = reciprocal(p2[:, 2])
        im2x, im2y = fx * p2[:, 0] * invZ2 + cx, fy * p2[:, 1] * invZ2 + cy
        err2 = (im2x - k2[:, 0]) * (im2x - k2[:, 0]) + (im2y - k2[:, 1]) * (im2y - k2[:, 1])
    cosines, margin = [], dict(cos=math.inf, reproj=math.inf)

    def near(kind, value, threshold):
        margin[kind] = min(margin[kind], ulps_from(value, threshold))

    for n, i in enumerate(idx):                      # (a margin is taken where the reference evaluates the comparison)
        first = matches[i, 0]
        if not finite[n]:
            vbGood[first] = 0
            continue
        if p[n, 2] <= 0:
            near("cos", cosP[n], 0.99998)
            if low[n]:
                continue
        if p2[n, 2] <= 0:
            near("cos", cosP[n], 0.99998)
            if low[n]:
                continue
        near("reproj", err1[n], th2)
        if err1[n] > th2:
            continue
        near("reproj", err2[n], th2)
        if err2[n] > th2:
            continue
        cosines.append(cosP[n])
        vP3D[first] = p[n]
        near("cos", cosP[n], 0.99998)
        if low[n]:
            vbGood[first] = 1
    parallax = f32(0)
    if cosines:
        c = sorted(cosines)[min(50, len(cosines) - 1)]
        with np.errstate(all="ignore"):
            a = f32(np.arccos(f64(c)))                                # (NaN for a cosine that rounded above 1)
        parallax = f32(f64(a * f32(180)) / CV_PI)
    return len(cosines), parallax, vP3D, vbGood, margin


def hypotheses_f(F21, K):
    """ReconstructF :479-487 + DecomposeE -> [(R1, t1), (R2, t1), (R1, t2), (R2, t2)]"""
    E = gemm(gemm(K.T, F21), K)
    u, w, vt = svd33(E)
    t = unit(u[:, 2])
    Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    R1 = gemm(gemm(u, Wm), vt)
    if det33(R1) < 0:
        R1 = -R1
    R2 = gemm(gemm(u, Wm.T), vt)
    if det33(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def hypotheses_h(H21, K):
    """ReconstructH :584-686 -> the eight (R, t), or None at the d1/d2 < 1.00001 exit"""
    A = gemm(gemm(inv33(K), H21), K)
    U, w, Vt = svd33(A)
    s = f32(det33(U) * det33(Vt))
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        if f64(d1 / d2) < 1.00001 or f64(d2 / d3) < 1.00001:
            return None
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
        aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
        out = []
        for i in range(4):
            Rp = np.eye(3, dtype=f32)
            Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
            R = gemm(gemm(U, Rp, alpha=s), Vt)
            tp = np.array([x1[i], 0, -x3[i]], f32) * (d1 - d3)
            out.append((R, unit(gemm(U, tp.reshape(3, 1)).ravel())))
        for i in range(4):
            Rp = np.eye(3, dtype=f32)
            Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], -1, sphi[i], -cphi
            R = gemm(gemm(U, Rp, alpha=s), Vt)
            tp = np.array([x1[i], 0, x3[i]], f32) * (d1 + d3)
            out.append((R, unit(gemm(U, tp.reshape(3, 1)).ravel())))
    return out


def solve(P, flip_null=False):
    keys1, keys2 = np.asarray(P["keys1"], f32), np.asarray(P["keys2"], f32)
    matches, sets = np.asarray(P["matches"], np.int64), np.asarray(P["sets"], np.int64)
    sigma = f32(P.get("sigma", 1.0))
    K4 = tuple(f32(v) for v in P["K"])
    minParallax, minTriangulated = f32(P.get("min_parallax", 1.0)), int(P.get("min_triangulated", 50))
    N, n1 = len(matches), len(keys1)
    res = dict(status=0, initialized=0, used_homography=0, H21=np.zeros((3, 3), f32), F21=np.zeros((3, 3), f32), R21=np.zeros((3, 3), f32),
               t21=np.zeros(3, f32), P3D=np.zeros((n1, 3), f32), triangulated=np.zeros(n1, np.uint8), n_good=np.zeros(8, np.int32),
               parallax=np.zeros(8, f32), n_hypotheses=0)
    vPn1, T1 = normalize(keys1)
    vPn2, T2 = normalize(keys2)
    p1, p2 = vPn1[matches[sets, 0]], vPn2[matches[sets, 1]]            # [its][8][2]
    u1, v1, u2, v2 = keys1[matches[:, 0], 0], keys1[matches[:, 0], 1], keys2[matches[:, 1], 0], keys2[matches[:, 1], 1]
    invSigmaSquare = f32(f64(1.0) / f64(sigma * sigma))
    # FindHomography (:124-172)
    Hn = compute_h21(p1, p2)
    if flip_null:
        Hn = -Hn
    H21 = gemm(gemm(inv33(T2), Hn), T1)
    H12 = inv33(H21)
    c1, c2 = chi_h(H21, H12, u1, v1, u2, v2, invSigmaSquare)
    scoresH, bh, SH, inlH = score_and_pick(c1, c2, TH_H, TH_H)
    margins = dict(chi_h=min(ulps_from(c1, TH_H), ulps_from(c2, TH_H)))
    # FindFundamental (:175-223)
    F21 = gemm(gemm(T2.T, compute_f21(p1, p2, flip_null)), T1)
    c1, c2 = chi_f(F21, u1, v1, u2, v2, invSigmaSquare)
    scoresF, bf, SF, inlF = score_and_pick(c1, c2, TH_F, TH_H)
    margins["chi_f"] = min(ulps_from(c1, TH_F), ulps_from(c2, TH_F))
    margins["tie"] = math.inf
    for scores, b in ((scoresH, bh), (scoresF, bf)):
        if b >= 0 and (scores == scores[b]).sum() > 1:
            margins["tie"] = 0.0                                         # two iterations tie for the best score
    res.update(SH=SH, SF=SF, best_iteration_h=bh, best_iteration_f=bf, inliers_h=inlH, inliers_f=inlF, scores_h=scoresH, scores_f=scoresF)
    if bh >= 0:
        res["H21"] = H21[bh]
    if bf >= 0:
        res["F21"] = F21[bf]
    with np.errstate(all="ignore"):
        RH = SH / (SH + SF)
    use_h = bool(f64(RH) > 0.40)
    margins["RH"] = ulps_from(RH, 0.40)
    res["used_homography"] = int(use_h)
    res["margins"] = margins
    if (bh if use_h else bf) < 0:
        res.update(status=1, margin_ulps=min(margins.values()))
        return res
    K = np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1]], f32)
    inl = inlH if use_h else inlF
    Nin = int(inl.sum())
    hyps = hypotheses_h(res["H21"], K) if use_h else hypotheses_f(res["F21"], K)
    if hyps is None:
        res["margin_ulps"] = min(margins.values())
        return res
    res["n_hypotheses"] = len(hyps)
    th2 = f32(f64(4.0) * f64(sigma * sigma))
    outs = []
    for h, (R, t) in enumerate(hyps):
        nGood, parallax, vP3D, vbGood, mg = check_rt(R, t, K4, keys1, keys2, matches, inl, th2)
        res["n_good"][h], res["parallax"][h] = nGood, parallax
        outs.append((vP3D, vbGood))
        for k, v in mg.items():
            margins[k] = min(margins.get(k, math.inf), v)
    nG, par = [int(x) for x in res["n_good"]], res["parallax"]
    pick = -1
    if use_h:                                                             # :689-731
        bestGood, secondBestGood, bestIdx, bestParallax = 0, 0, -1, f32(-1)
        for i in range(8):
            if nG[i] > bestGood:
                secondBestGood, bestGood, bestIdx, bestParallax = bestGood, nG[i], i, par[i]
            elif nG[i] > secondBestGood:
                secondBestGood = nG[i]
        if bestIdx >= 0:
            margins["parallax"] = ulps_from(bestParallax, minParallax)
        if secondBestGood < 0.75 * bestGood and bestParallax >= minParallax and bestGood > minTriangulated and bestGood > 0.9 * Nin:
            pick = bestIdx
    else:                                                                 # :499-569
        maxGood = max(nG[:4])
        nMinGood = max(int(0.9 * Nin), minTriangulated)
        nsimilar = sum(1 for k in range(4) if nG[k] > 0.7 * maxGood)
        if not (maxGood < nMinGood or nsimilar > 1):
            k = nG[:4].index(maxGood)
            margins["parallax"] = ulps_from(par[k], minParallax)
            if par[k] > minParallax:
                pick = k
    res["margin_ulps"] = min(margins.values())
    res["pick"] = pick
    if pick >= 0:
        res.update(initialized=1, R21=hyps[pick][0], t21=hyps[pick][1], P3D=outs[pick][0], triangulated=outs[pick][1])
    return res


def collinear(n=12, iterations=3):
    """all keys of both frames on one line: H21i is singular (its inverse the zero matrix), every F is rank deficient in a way that
    makes a2 = b2 = 0 for points on the line; no hypothesis scores above 0"""
    x = np.arange(n, dtype=np.float32) * 20 + 50
    keys = np.stack([x, np.full(n, 100, np.float32)], 1)
    matches = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    sets = np.stack([np.roll(np.arange(n), -k)[:8] for k in range(iterations)]).astype(np.int32)
    return dict(keys1=keys, keys2=keys + np.float32([3, 0]), matches=matches, sets=sets, K=(517.3, 516.5, 318.6, 255.3))


RESULT_KEYS = ("status", "initialized", "used_homography", "SH", "SF", "H21", "F21", "best_iteration_h", "best_iteration_f", "inliers_h",
               "inliers_f", "R21", "t21", "P3D", "triangulated", "n_good", "n_hypotheses")


def raw(res, keys=RESULT_KEYS):
    """every byte of a result except parallax"""
    out = []
    for k in keys:
        v = res[k]
        out.append(np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else
                   np.float32(v).tobytes() if k in ("SH", "SF") else np.int32(v).tobytes())
    return b"".join(out)


def parallax_ulps(a, b):
    """the largest distance between two parallax arrays in float32 ulps; a NaN (acos of a cosine that rounded above 1) only equals a NaN"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    if (np.isnan(a) != np.isnan(b)).any():
        return math.inf
    ok = ~np.isnan(a) & (a != b)
    if not ok.any():
        return 0.0
    return float((np.abs(a[ok].astype(f64) - b[ok].astype(f64)) / np.spacing(np.maximum(np.abs(a[ok]), np.abs(b[ok])))).max())


def same(got, want):
    return raw(got) == raw(want) and parallax_ulps(got["parallax"], want["parallax"]) <= 1
