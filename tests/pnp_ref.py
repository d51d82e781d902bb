"""PnPsolver (src/PnPsolver.cc) restated in plain Python / numpy for the tests: the conventions of DESIGN.md section 2 item 11 written
out independently of csrc/pnp.h -- the one-sided Jacobi SVD in double, the pseudo-inverse solves, EPnP's compute_pose, CheckInliers
with its float / double widths, the literal swap-with-back index removal, the literal loop of iterate() with a literal Refine() at
every qualifying iteration (nothing memoised), SetRansacParameters -- and the generator of the problems the CPU and GPU tests share.

Python floats are IEEE doubles and every sum below is an explicit left-to-right loop (the built-in sum() may compensate); float
widths are numpy.float32 scalars, whose operations round once each."""
import functools
import math

import numpy as np

DBL_EPSILON = 2.220446049250313e-16
F = np.float32


def ssum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def x86_int(v):
    """a double on its way into an int: truncation, INT_MIN where it is NaN or does not fit"""
    if v != v or v <= -2147483649.0 or v >= 2147483648.0:
        return -2 ** 31
    return int(v)


def _div(a, b):
    """a / b with IEEE results for b == 0"""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan   # (NaN compares false: lands here too)


# ---- SetRansacParameters (:121-157)
def ransac_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    eps = F(epsilon)
    m = x86_int(float(F(n) * eps))
    m = max(m, min_inliers, min_set)
    with np.errstate(all="ignore"):
        q = F(m) / F(n)
    if eps < q:
        eps = q
    if m == n:
        its = 1
    else:
        with np.errstate(all="ignore"):
            den = np.log(np.float64(1) - np.float64(eps) ** 3)
            its = x86_int(float(np.ceil(np.log(np.float64(1 - probability)) / den)))
    return m, F(eps), max(1, min(its, max_iterations))


# ---- the draws and the index removal (:188-201)
def random_int(rng, lo, hi):
    d = hi - lo + 1
    return int((float(rng.integers(0, 2 ** 31)) / (2147483647.0 + 1.0)) * d) + lo


def draws_for(rng, n, n_iterations, min_set):
    d = np.zeros((n_iterations, min_set), np.int32)
    if n >= min_set:
        for k in range(n_iterations):
            for i in range(min_set):
                d[k, i] = random_int(rng, 0, n - 1 - i)
    return d


def set_literal(n, row):
    """vAvailableIndices = 0..n-1; every draw takes a position, which receives the back, which is popped"""
    avail = list(range(n))
    out = []
    for r in row:
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def draws_selecting(n, indices):
    """the draws that make set_literal return `indices`"""
    avail = list(range(n))
    row = []
    for idx in indices:
        r = avail.index(idx)
        row.append(r)
        avail[r] = avail[-1]
        avail.pop()
    return row


# ---- the dense routines of item 11
def jacobi_svd(At):
    """one-sided Jacobi on the rows of At (n rows of m) -> (W descending, the rotated rows, V rows = accumulated rotations, sweeps)"""
    At = [np.array(r, np.float64) for r in At]
    n, m = len(At), len(At[0])
    V = [np.array([1.0 if i == k else 0.0 for k in range(n)]) for i in range(n)]
    W = [ssum((r * r).tolist()) for r in At]
    eps = 10 * DBL_EPSILON
    sweeps = 0
    with np.errstate(all="ignore"):
        for sweeps in range(1, 31):
            changed = False
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a, b = W[i], W[j]
                    p = ssum((At[i] * At[j]).tolist())
                    if abs(p) <= eps * _sqrt(a * b):
                        continue
                    p *= 2
                    beta = a - b
                    gamma = _sqrt(p * p + beta * beta)
                    if beta < 0:
                        delta = (gamma - beta) * 0.5
                        s = _sqrt(_div(delta, gamma))
                        c = _div(p, gamma * s * 2)
                    else:
                        c = _sqrt(_div(gamma + beta, gamma * 2))
                        s = _div(p, gamma * c * 2)
                    t0 = c * At[i] + s * At[j]
                    t1 = -s * At[i] + c * At[j]
                    At[i], At[j] = t0, t1
                    W[i], W[j] = ssum((t0 * t0).tolist()), ssum((t1 * t1).tolist())
                    changed = True
                    V[i], V[j] = c * V[i] + s * V[j], -s * V[i] + c * V[j]
            if not changed:
                break
    W = [_sqrt(ssum((r * r).tolist())) for r in At]
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            At[i], At[j] = At[j], At[i]
            V[i], V[j] = V[j], V[i]
    return W, At, V, sweeps


def svd_solve(A, bs):
    """cvSolve(A, b, x, CV_SVD) / cvInvert(A, ., CV_SVD) for the m x n matrix A (rows) and each right-hand side of bs"""
    m, n = len(A), len(A[0])
    W, At, V, _ = jacobi_svd([[A[k][i] for k in range(m)] for i in range(n)])
    with np.errstate(all="ignore"):
        U = [At[i] * _div(1.0, W[i]) for i in range(n)]
    thr = ssum(W) * (2 * DBL_EPSILON)
    out = []
    for b in bs:
        x = [0.0] * n
        for i in range(n):
            if abs(W[i]) <= thr:
                continue
            wi = _div(1.0, W[i])
            with np.errstate(all="ignore"):
                s = ssum([float(U[i][k]) * b[k] for k in range(m)]) * wi
                for j in range(n):
                    x[j] += s * float(V[i][j])
        out.append(x)
    return out


def qr_solve(A, b, x):
    """the Householder solve of :860-950 on copies of A (nr x nc rows) and b; x is returned unchanged when a column is singular"""
    A = [list(r) for r in A]
    b = list(b)
    nr, nc = len(A), len(A[0])
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        eta = abs(A[k][k])
        for i in range(k + 1, nr):   # the reference's pointer is read before it moves: rows k .. nr-2
            elt = abs(A[i - 1][k])
            if eta < elt:
                eta = elt
        if eta == 0:
            return list(x), False
        inv_eta = 1.0 / eta
        s = 0.0
        for i in range(k, nr):
            A[i][k] *= inv_eta
            s += A[i][k] * A[i][k]
        sigma = _sqrt(s)
        if A[k][k] < 0:
            sigma = -sigma
        A[k][k] += sigma
        A1[k] = sigma * A[k][k]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s = 0.0
            for i in range(k, nr):
                s += A[i][k] * A[i][j]
            tau = _div(s, A1[k])
            for i in range(k, nr):
                A[i][j] -= tau * A[i][k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i][j] * b[i]
        tau = _div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i][j]
    x = list(x)
    x[nc - 1] = _div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i][j] * x[j]
        x[i] = _div(b[i] - s, A2[i])
    return x, True


# ---- EPnP (:375-858)
def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _dist2(p, q):
    return (p[0] - q[0]) * (p[0] - q[0]) + (p[1] - q[1]) * (p[1] - q[1]) + (p[2] - q[2]) * (p[2] - q[2])


def mtm_of(M):
    """cvMulTransposed(M, MtM, 1): every entry a sum over the rows of M in order (numpy adds one outer product per row)"""
    out = np.zeros((12, 12))
    for row in M:
        out += np.outer(row, row)
    return out


def compute_pose(pws, us, K, null_signs=(1, 1, 1, 1), detail=None):
    """compute_pose (:477-525) of n >= 4 correspondences (lists of doubles) -> (R rows, t, the three reprojection errors).
    null_signs flips the four null-space rows (for the test that their sign does not matter)"""
    fu, fv, uc, vc = K
    n = len(pws)
    with np.errstate(all="ignore"):
        c0 = [_div(ssum([p[j] for p in pws]), float(n)) for j in range(3)]
        pw0 = [[p[j] - c0[j] for j in range(3)] for p in pws]
        ptp = [[ssum([d[r] * d[c] for d in pw0]) for c in range(3)] for r in range(3)]
        dc, _, uct, _ = jacobi_svd(ptp)
        cws = [c0]
        for i in range(1, 4):
            k = _sqrt(_div(dc[i - 1], float(n)))
            cws.append([c0[j] + k * float(uct[i - 1][j]) for j in range(3)])
        cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
        cols = svd_solve(cc, [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
        ci = [[cols[c][r] for c in range(3)] for r in range(3)]
        alphas = []
        for p in pws:
            d = [p[0] - cws[0][0], p[1] - cws[0][1], p[2] - cws[0][2]]
            a = [0.0] + [ci[j][0] * d[0] + ci[j][1] * d[1] + ci[j][2] * d[2] for j in range(3)]
            a[0] = 1.0 - a[1] - a[2] - a[3]
            alphas.append(a)
        M = []
        for a, (u, v) in zip(alphas, us):
            M.append([x for i in range(4) for x in (a[i] * fu, 0.0, a[i] * (uc - u))])
            M.append([x for i in range(4) for x in (0.0, a[i] * fv, a[i] * (vc - v))])
        mtm = mtm_of(np.array(M))
        D, _, ut, sweeps = jacobi_svd(mtm)
        v = [null_signs[i] * ut[11 - i] for i in range(4)]
        L = []
        for a, b in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            dv = [[float(v[q][3 * a + c]) - float(v[q][3 * b + c]) for c in range(3)] for q in range(4)]
            L.append([_dot3(dv[0], dv[0]), 2.0 * _dot3(dv[0], dv[1]), _dot3(dv[1], dv[1]), 2.0 * _dot3(dv[0], dv[2]), 2.0 * _dot3(dv[1], dv[2]),
                      _dot3(dv[2], dv[2]), 2.0 * _dot3(dv[0], dv[3]), 2.0 * _dot3(dv[1], dv[3]), 2.0 * _dot3(dv[2], dv[3]), _dot3(dv[3], dv[3])])
        rho = [_dist2(cws[a], cws[b]) for a, b in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))]
        cands = []
        for cand in (1, 2, 3):
            if cand == 1:
                b4 = svd_solve([[r[0], r[1], r[3], r[6]] for r in L], [rho])[0]
                sg = -1.0 if b4[0] < 0 else 1.0
                b0 = _sqrt(sg * b4[0])
                betas = [b0, _div(sg * b4[1], b0), _div(sg * b4[2], b0), _div(sg * b4[3], b0)]
            else:
                bb = svd_solve([r[:3] if cand == 2 else r[:5] for r in L], [rho])[0]
                if bb[0] < 0:
                    betas = [_sqrt(-bb[0]), _sqrt(-bb[2]) if bb[2] < 0 else 0.0]
                else:
                    betas = [_sqrt(bb[0]), _sqrt(bb[2]) if bb[2] > 0 else 0.0]
                if bb[1] < 0:
                    betas[0] = -betas[0]
                betas += [0.0 if cand == 2 else _div(bb[3], betas[0]), 0.0]
            x = [0.0] * 4
            for _ in range(5):   # gauss_newton (:840-858)
                A, bvec = [], []
                for r, rh in zip(L, rho):
                    A.append([2 * r[0] * betas[0] + r[1] * betas[1] + r[3] * betas[2] + r[6] * betas[3],
                              r[1] * betas[0] + 2 * r[2] * betas[1] + r[4] * betas[2] + r[7] * betas[3],
                              r[3] * betas[0] + r[4] * betas[1] + 2 * r[5] * betas[2] + r[8] * betas[3],
                              r[6] * betas[0] + r[7] * betas[1] + r[8] * betas[2] + 2 * r[9] * betas[3]])
                    bvec.append(rh - (r[0] * betas[0] * betas[0] + r[1] * betas[0] * betas[1] + r[2] * betas[1] * betas[1] + r[3] * betas[0] * betas[2] +
                                      r[4] * betas[1] * betas[2] + r[5] * betas[2] * betas[2] + r[6] * betas[0] * betas[3] + r[7] * betas[1] * betas[3] +
                                      r[8] * betas[2] * betas[3] + r[9] * betas[3] * betas[3]))
                x, _ = qr_solve(A, bvec, x)
                betas = [betas[i] + x[i] for i in range(4)]
            # compute_R_and_t (:651-662)
            ccs = [[0.0] * 3 for _ in range(4)]
            for i in range(4):
                for j in range(4):
                    for k in range(3):
                        ccs[j][k] += betas[i] * float(v[i][3 * j + k])
            pcs = [[a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j] for j in range(3)] for a in alphas]
            if pcs[0][2] < 0.0:
                ccs = [[-x_ for x_ in r] for r in ccs]
                pcs = [[-x_ for x_ in r] for r in pcs]
            pc0 = [_div(ssum([p[j] for p in pcs]), float(n)) for j in range(3)]
            pwm = [_div(ssum([p[j] for p in pws]), float(n)) for j in range(3)]
            abt = [[ssum([(pc[j] - pc0[j]) * (pw[c] - pwm[c]) for pc, pw in zip(pcs, pws)]) for c in range(3)] for j in range(3)]
            Wd, At, Vv, _ = jacobi_svd([[abt[k][i] for k in range(3)] for i in range(3)])
            Uc = [At[k] * _div(1.0, Wd[k]) for k in range(3)]   # U[i][k] = Uc[k][i], V[j][k] = Vv[k][j]
            R = [[float(Uc[0][i]) * float(Vv[0][j]) + float(Uc[1][i]) * float(Vv[1][j]) + float(Uc[2][i]) * float(Vv[2][j]) for j in range(3)]
                 for i in range(3)]
            det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                   R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
            if det < 0:
                R[2] = [-x_ for x_ in R[2]]
            t = [pc0[i] - _dot3(R[i], pwm) for i in range(3)]
            s2 = 0.0
            for pw, (u, vv) in zip(pws, us):
                Xc, Yc, iz = _dot3(R[0], pw) + t[0], _dot3(R[1], pw) + t[1], _div(1.0, _dot3(R[2], pw) + t[2])
                ue, ve = uc + fu * Xc * iz, vc + fv * Yc * iz
                s2 += _sqrt((u - ue) * (u - ue) + (vv - ve) * (vv - ve))
            cands.append((R, t, _div(s2, float(n))))
    errs = [c[2] for c in cands]
    N = 0
    if errs[1] < errs[0]:
        N = 1
    if errs[2] < errs[N]:
        N = 2
    if detail is not None:
        detail.update(mtm=mtm, D=D, ut=ut, sweeps=sweeps, cands=cands, winner=N, M=np.array(M))
    return cands[N][0], cands[N][1], errs


def pose_of(P, indices, **kw):
    pws = [[float(x) for x in P["P3Dw"][i]] for i in indices]
    us = [[float(x) for x in P["P2D"][i]] for i in indices]
    return compute_pose(pws, us, [float(F(k)) for k in P["K"]], **kw)


def check_inliers(P, R, t):
    """CheckInliers (:308-339) -> (flags, count, the smallest distance of an error from its threshold in float ulps of the threshold)"""
    fu, fv, uc, vc = [float(F(k)) for k in P["K"]]
    n = len(P["P3Dw"])
    flags = np.zeros(n, np.uint8)
    margin = math.inf
    with np.errstate(all="ignore"):
        for i in range(n):
            x, y, z = (float(c) for c in P["P3Dw"][i])
            Xc = F(R[0][0] * x + R[0][1] * y + R[0][2] * z + t[0])
            Yc = F(R[1][0] * x + R[1][1] * y + R[1][2] * z + t[1])
            invZc = F(_div(1.0, R[2][0] * x + R[2][1] * y + R[2][2] * z + t[2]))
            ue = uc + fu * float(Xc) * float(invZc)
            ve = vc + fv * float(Yc) * float(invZc)
            dX = F(float(P["P2D"][i][0]) - ue)
            dY = F(float(P["P2D"][i][1]) - ve)
            e2 = F(F(dX * dX) + F(dY * dY))
            me = F(P["max_err"][i])
            flags[i] = bool(e2 < me)
            if np.isfinite(e2):
                margin = min(margin, abs(float(e2) - float(me)) / float(np.spacing(me)))
    return flags, int(flags.sum()), margin


def tcw_of(R, t):
    T = np.eye(4, dtype=np.float32)
    with np.errstate(all="ignore"):
        T[:3, :3] = np.array(R, np.float64).astype(np.float32)
        T[:3, 3] = np.array(t, np.float64).astype(np.float32)
    return T


# ---- the loop of iterate (:182-239) and Refine (:260-305), literal
def scan_literal(first, counts, refine_count_of, min_inliers, best_inliers_in=0):
    """the loop over given counts; refine_count_of(best_iteration) -> Refine()'s count for the best set of that iteration (-1: the
    carried set), CALLED AT EVERY QUALIFYING ITERATION -> (returned_at, best_iteration, best_inliers)"""
    best, best_it = best_inliers_in, -1
    for k, c in enumerate(counts):
        it = first + k
        if c >= min_inliers:
            if c > best:
                best, best_it = c, it
            if refine_count_of(best_it) > min_inliers:
                return it, best_it, best
    return -1, best_it, best


def solve(P, ignore_returns=False):
    """PnPsolver::iterate on problem P over iterations [first_iteration, n_iterations) -> the fields of aos2_pnp_result_t, and
    diagnostics.  ignore_returns: the loop goes on after a return; every return is recorded in `events`."""
    n, its, first = len(P["P3Dw"]), int(P["n_iterations"]), int(P.get("first_iteration", 0))
    out = dict(returned_at=-1, Tcw=np.zeros((4, 4), np.float32), n_inliers=0, inliers=np.zeros(n, np.uint8), best_iteration=-1,
               best_inliers=int(P.get("best_inliers_in", 0)), best_Tcw=np.zeros((4, 4), np.float32),
               best=np.array(P["best_in"], np.uint8).copy() if P.get("best_inliers_in", 0) > 0 else np.zeros(n, np.uint8),
               counts=np.full(its, -1, np.int32), margin_ulps=math.inf, nan_hyps=[], refines=[], events=[])
    if n < P["min_inliers"] or first >= its:
        return out
    for it in range(first, its):
        idx = set_literal(n, P["draws"][it])
        R, t, _ = pose_of(P, idx)
        flags, count, margin = check_inliers(P, R, t)
        out["margin_ulps"] = min(out["margin_ulps"], margin)
        if not np.isfinite(np.array(R)).all():
            out["nan_hyps"].append(it)
        out["counts"][it] = count
        if count < P["min_inliers"]:
            continue
        if count > out["best_inliers"]:
            out.update(best=flags, best_inliers=count, best_iteration=it, best_Tcw=tcw_of(R, t))
        # Refine()
        Rr, tr, _ = pose_of(P, [i for i in range(n) if out["best"][i]])
        rflags, rcount, margin = check_inliers(P, Rr, tr)
        out["margin_ulps"] = min(out["margin_ulps"], margin)
        ok = rcount > P["min_inliers"]
        out["refines"].append((it, out["best_iteration"], rcount, ok))
        if ok:
            ev = dict(returned_at=it, Tcw=tcw_of(Rr, tr), n_inliers=rcount, inliers=rflags, best_iteration=out["best_iteration"],
                      best_inliers=out["best_inliers"], best=out["best"].copy(), best_Tcw=out["best_Tcw"].copy())
            out["events"].append(ev)
            if not ignore_returns:
                out.update(returned_at=it, Tcw=ev["Tcw"], n_inliers=rcount, inliers=rflags)
                out["counts"][it + 1:] = -1
                return out
    return out


def same(got, want, counts=True):
    """the fields of aos2_pnp_result_t equal, poses bit for bit"""
    ok = all(int(got[k]) == int(want[k]) for k in ("returned_at", "n_inliers", "best_iteration", "best_inliers"))
    ok = ok and all(np.array(got[k], np.uint8).tobytes() == np.array(want[k], np.uint8).tobytes() for k in ("inliers", "best"))
    ok = ok and all(np.array(got[k], np.float32).tobytes() == np.array(want[k], np.float32).tobytes() for k in ("Tcw", "best_Tcw"))
    if counts and got.get("counts") is not None:
        ok = ok and (np.array(got["counts"]) == np.array(want["counts"])).all()
    return bool(ok)


# ---- the generator
SIZES = (9, 10, 11, 15, 40, 64, 65, 150)
CAMERA = (517.3, 516.5, 318.6, 255.3)
PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5)
TH2 = F(5.991)


def level_sigma2(n_levels=8, scale_factor=1.2):
    s, out = F(1.0), [F(1.0)]
    for _ in range(1, n_levels):
        s = F(s * F(scale_factor))
        out.append(F(s * s))
    return out


def _rotation(axis, angle):
    a = np.array(axis, np.float64)
    a /= np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * Kx + (1 - math.cos(angle)) * Kx @ Kx


def planted_pose(rng):
    return _rotation(rng.normal(size=3), rng.uniform(0.1, 0.6)), rng.uniform(-0.5, 0.5, size=3)


def project(R, t, X, K=CAMERA):
    c = X @ R.T + t
    return np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], axis=1)


def problem(rng, n, structures, noise=0.3, params=PARAMS, n_iterations=None):
    """n correspondences: structures = [(count, pose)] are consistent with a pose each (pixel noise `noise` * the level's sigma), the
    rest are outliers (a random pixel).  The RANSAC parameters are adjusted as SetRansacParameters does; n_iterations defaults to what
    the first iterate(5) runs: max(mRansacMaxIts, 5)."""
    sig2 = level_sigma2()
    X = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 8, n)], axis=1).astype(np.float32)
    octave = rng.integers(0, 8, n)
    uv = np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], axis=1)
    k = 0
    for cnt, (R, t) in structures:
        Xw = (X[k:k + cnt].astype(np.float64) - t) @ R   # world points whose camera coordinates are X
        X[k:k + cnt] = Xw.astype(np.float32)
        s = np.sqrt(np.array([float(sig2[o]) for o in octave[k:k + cnt]]))
        uv[k:k + cnt] = project(R, t, X[k:k + cnt].astype(np.float64)) + noise * s[:, None] * rng.normal(size=(cnt, 2))
        k += cnt
    perm = rng.permutation(n)
    X, uv, octave = X[perm], uv[perm], octave[perm]
    max_err = np.array([F(sig2[o] * TH2) for o in octave], np.float32)
    mi, eps, its = ransac_parameters(n, **params)
    if n_iterations is None:
        n_iterations = max(its, 5)
    member = np.full(n, -1)
    k = 0
    for s_i, (cnt, _) in enumerate(structures):
        member[np.argsort(perm)[k:k + cnt]] = s_i
        k += cnt
    return dict(P3Dw=X, P2D=uv.astype(np.float32), max_err=max_err, K=CAMERA, min_inliers=mi, min_set=params["min_set"],
                n_iterations=n_iterations, ransac_max_its=its, draws=draws_for(rng, n, n_iterations, params["min_set"]),
                member=member, structures=structures, octave=octave.astype(np.int32))


def good_set(P, rng, structure, want_count, size=None, tries=400):
    """members of a structure whose EPnP pose has exactly want_count inliers (searched with the reference: a minimal set does not
    reliably give the planted pose back)"""
    pool = np.flatnonzero(P["member"] == structure)
    for _ in range(tries):
        idx = [int(i) for i in rng.choice(pool, size or P["min_set"], replace=False)]
        R, t, _ = pose_of(P, idx)
        if check_inliers(P, R, t)[1] == want_count:
            return idx
    raise AssertionError("no minimal set of structure %d gives %d inliers" % (structure, want_count))


def bad_set(P, rng, tries=400):
    """a minimal set whose pose has fewer than min_inliers inliers"""
    n = len(P["P3Dw"])
    for _ in range(tries):
        idx = [int(i) for i in rng.choice(n, P["min_set"], replace=False)]
        R, t, _ = pose_of(P, idx)
        if check_inliers(P, R, t)[1] < P["min_inliers"]:
            return idx
    raise AssertionError("no bad set")


@functools.lru_cache(maxsize=None)
def generator_case(seed):
    """the batch of the tests: one problem per size of SIZES (tests/test_pnp_cpu.py asserts what they cover) and what the reference
    gives for each -> dict(problems, want)"""
    rng = np.random.default_rng(seed)
    A, B = planted_pose(rng), planted_pose(rng)
    sizes = iter(SIZES)
    problems = []
    # 9: below the adjusted minimum of 10, nothing runs
    problems.append(problem(rng, next(sizes), [(9, A)]))
    # 10: every point an inlier, mRansacMaxIts = 1 and five iterations run; Refine() cannot find more than 10: the exhaustion
    # returns the unrefined best.  Iteration 1 is a set that finds all ten.
    P = problem(rng, next(sizes), [(10, A)], noise=0.05)
    P["draws"][1] = draws_selecting(10, good_set(P, rng, 0, 10))
    problems.append(P)
    # 11: mRansacMaxIts = 4, five iterations run
    problems.append(problem(rng, next(sizes), [(11, B)], noise=0.05))
    # 15, min_set = 5: iteration 0 finds the thirteen inliers and returns
    P = problem(rng, next(sizes), [(13, A)], noise=0.1, params=dict(PARAMS, min_set=5))
    P["draws"][0] = draws_selecting(15, good_set(P, rng, 0, 13))
    problems.append(P)
    # 40 with 40 % outliers; points 0 .. 3 are one map point.  Iteration 3 draws two of them: a rank-deficient set, whose model
    # item 11 keeps finite (the pseudo-inverse drops the vanished direction); iteration 5 draws all four: PW0 vanishes, so do rho
    # and the betas, 0 / 0 follows and the model is NaN.
    P = problem(rng, next(sizes), [(24, B)])
    for key in ("P3Dw", "P2D", "max_err", "octave"):
        P[key][1:4] = P[key][0]
    P["member"][1:4] = P["member"][0]
    rest = [int(i) for i in rng.choice(np.arange(4, 40), 2, replace=False)]
    P["draws"][3] = draws_selecting(40, [0, rest[0], 1, rest[1]])
    P["draws"][5] = draws_selecting(40, [2, 0, 3, 1])
    problems.append(P)
    # 64, epsilon = 0.2: min_inliers 12 and 300 iterations.  Exactly 12 points follow pose A, 30 follow pose B.  Iteration 2 finds
    # the twelve: Refine() on them cannot find more than 12 and fails; iteration 4 finds them again (it does not beat the best: the
    # same Refine()); iteration 7 finds the thirty, a new best whose Refine() returns.  The other early iterations find nothing.
    P = problem(rng, next(sizes), [(12, A), (30, B)], noise=0.1, params=dict(PARAMS, epsilon=0.2))
    assert (P["min_inliers"], P["n_iterations"]) == (12, 300)
    for it in range(10):
        P["draws"][it] = draws_selecting(64, bad_set(P, rng))
    P["draws"][2] = draws_selecting(64, good_set(P, rng, 0, 12))
    P["draws"][4] = draws_selecting(64, good_set(P, rng, 0, 12))
    P["draws"][7] = draws_selecting(64, good_set(P, rng, 1, 30))
    problems.append(P)
    # 65: all outliers
    problems.append(problem(rng, next(sizes), []))
    # 150 with 40 % outliers
    problems.append(problem(rng, next(sizes), [(90, A)]))
    return dict(problems=problems, want=[solve(P) for P in problems])
