"""tests/lba_system_ref.py checked on its own, without a device: the Jacobians against finite differences, the Schur complement against
the dense system, and the two float64 models of the assembly against the long-double reference on every input of
tests/test_lba_system_gpu.py -- their worst omega per quantity and family is what the GPU tests' tolerance is 4 x of, and it has to stay
below 16: a larger one means the scale M misses a conditioning term."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_system_ref as S  # noqa: E402

LD = S.LD


def se3_exp_ld(xi):
    """exp of (omega, upsilon) -> (R, t) in long double"""
    w, u = xi[:3], xi[3:]
    th = np.sqrt((w * w).sum())
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], LD)
    I = np.eye(3, dtype=LD)
    if th < LD(1e-30):
        return I + K, u
    A, B, C_ = np.sin(th) / th, (1 - np.cos(th)) / (th * th), (th - np.sin(th)) / (th * th * th)
    return I + A * K + B * K @ K, (I + B * K + C_ * K @ K) @ u


def one_edge_window(rng, stereo):
    w = S.make_window(int(rng.integers(1 << 30)), 1, 1, [[0, 1]], kinds="stereo" if stereo else "mono")
    return w, S.host_estimates(w)


@pytest.mark.parametrize("stereo", [0, 1])
def test_jacobians_equal_central_differences(stereo):
    """J_pose and J_l of linearizeOplus against central differences of the residual under exp(xi) T and X + d, in long double, at two steps:
    the difference falls with the square of the step (the truncation order), and at h = 1e-5 it is below 1e-7 of the entry's scale.  The
    stereo rows are differenced on a residual with an exact reciprocal (the float one of cam_project is a step function)."""
    rng = np.random.default_rng(20 + stereo)
    for _ in range(6):
        w, est = one_edge_window(rng, stereo)
        w = dict(w, n_edges=1, edge_pose=w["edge_pose"][:1], edge_point=w["edge_point"][:1], edge_obs=w["edge_obs"][:1],
                 edge_stereo=w["edge_stereo"][:1], edge_inv_sigma2=w["edge_inv_sigma2"][:1])
        R, p = S.camera_points(w, est, LD)
        Jl, Jp = S.jacobians(w, R, p, w["edge_stereo"], LD)
        Jl = np.array([[Jl[r][c].v[0] for c in range(3)] for r in range(3)])
        Jp = np.array([[Jp[r][c].v[0] for c in range(6)] for r in range(3)])
        Rm = np.array([[R[r][c].v[0] for c in range(3)] for r in range(3)])
        p0 = np.array([p[i].v[0] for i in range(3)])

        def res(pc):
            e = S.residual(w, [S.VM(np.array([pc[i]], LD)) for i in range(3)], w["edge_obs"], w["edge_stereo"], LD, exact_reciprocal=True)
            return np.array([e[i].v[0] for i in range(3)])

        errs = []
        for h in (LD(1e-4), LD(1e-5)):
            fd_p, fd_l = np.zeros((3, 6), LD), np.zeros((3, 3), LD)
            for k in range(6):
                xi = np.zeros(6, LD)
                xi[k] = h
                Ra, ta = se3_exp_ld(xi)
                Rb, tb = se3_exp_ld(-xi)
                fd_p[:, k] = (res(Ra @ p0 + ta) - res(Rb @ p0 + tb)) / (2 * h)
            for k in range(3):
                d = np.zeros(3, LD)
                d[k] = h
                fd_l[:, k] = (res(p0 + Rm @ d) - res(p0 - Rm @ d)) / (2 * h)
            errs.append(max(np.abs(fd_p - Jp).max() / np.abs(Jp).max(), np.abs(fd_l - Jl).max() / np.abs(Jl).max()))
        assert errs[1] < 1e-7 and errs[1] < errs[0] / 50, errs
        if not stereo:
            assert not Jp[2].any() and not Jl[2].any()


def dense_solution(ref_lin, lam):
    """the full (6 np + 3 nl) system assembled densely and solved in long double (Gaussian elimination with partial pivoting) -> pose part"""
    n_p, n_l = len(ref_lin["hpose"]), len(ref_lin["hpoint"])
    n = 6 * n_p + 3 * n_l
    H, b = np.zeros((n, n), LD), np.zeros(n, LD)
    for i in range(n_p):
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = ref_lin["Hpp"][0][i]
    for l in range(n_l):
        H[6 * n_p + 3 * l:6 * n_p + 3 * l + 3, 6 * n_p + 3 * l:6 * n_p + 3 * l + 3] = ref_lin["Hll"][0][l]
    for e in np.nonzero(ref_lin["free"])[0]:
        i, l = ref_lin["ph"][e], ref_lin["lh"][e]
        H[6 * i:6 * i + 6, 6 * n_p + 3 * l:6 * n_p + 3 * l + 3] += ref_lin["B"][0][e]
        H[6 * n_p + 3 * l:6 * n_p + 3 * l + 3, 6 * i:6 * i + 6] += ref_lin["B"][0][e].T
    H += lam * np.eye(n, dtype=LD)
    b[:6 * n_p] = ref_lin["b_p"][0].ravel()
    b[6 * n_p:] = ref_lin["b_l"][0].ravel()
    return gauss_solve(H, b)[:6 * n_p]


def gauss_solve(A, b):
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]] = A[[piv, k]]
            b[[k, piv]] = b[[piv, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, LD)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


@pytest.mark.parametrize("name", ["co0", "co17", "np3", "np8"])
def test_schur_identity(name):
    """the pose part of the solution of the full system equals the solution of (Hs, bs) to 1e-15 relative, in long double, at lambda_init
    and at 100 x lambda_init"""
    case = [c for f in ("counts", "sizes") for c in S.cases(f) if c["name"] == name][0]
    lin = S.linearise(case["win"], S.host_estimates(case["win"]), LD)
    for factor in (1, 100):
        lam = lin["lambda"][0] * factor
        red = S.reduce(lin, lam)
        x_full = dense_solution(lin, lam)
        x_red = gauss_solve(red["Hs"][0], red["bs"][0])
        assert np.abs(x_full - x_red).max() <= 1e-15 * np.abs(x_full).max(), (name, factor, float(np.abs(x_full - x_red).max() / np.abs(x_full).max()))
        assert (red["Hs"][1] >= np.abs(red["Hs"][0])).all() and (red["bs"][1] >= np.abs(red["bs"][0])).all()   # M >= |q|


def stage1_estimates(case, oracle):
    r = oracle.lba_solve(case["win"], iters1=5, iters2=0)
    return r, dict(pose=r["pose_qt"], point=r["point_xyz64"], e_level1=r["edge_level1"], e_robust=np.zeros(case["win"]["n_edges"], np.uint8))


def test_stage1_seeds_mask_exactly_the_planted_edges(oracle):
    """the windows of the stage-1 test: the oracle's outlier pass after optimize(5) masks the planted edges and no other, and every one of its
    five steps is accepted"""
    for case in S.cases("stage1"):
        r, _ = stage1_estimates(case, oracle)
        assert r["iters"][0] == 5 and r["trials"] == 5, (case["name"], r["iters"], r["trials"])
        assert np.nonzero(r["edge_level1"])[0].tolist() == case["planted"].tolist(), case["name"]
        assert (r["edge_outlier"] == r["edge_level1"]).all(), case["name"]


@pytest.mark.parametrize("family", S.FAMILIES)
def test_float64_models_against_the_reference(family, oracle):
    """both float64 models on every input of the GPU tests: worst omega per quantity, printed (the table of DESIGN.md 5.3), below 16"""
    worst = {"textbook": {}, "records": {}}
    for case in S.cases(family):
        est = stage1_estimates(case, oracle)[1] if case["stage"] == 1 else S.host_estimates(case["win"])
        _, _, per = S.evaluate(case, est)
        for m in per:
            for q, (v, _) in per[m].items():
                worst[m][q] = max(worst[m].get(q, 0.0), v)
    for q in S.QUANTITIES:
        if q in worst["textbook"]:
            print(f"worst omega {family:8s} {q:8s} textbook {worst['textbook'][q]:9.3g}   records {worst['records'][q]:9.3g}")
    for m in worst:
        for q, v in worst[m].items():
            assert v <= 16.0, (family, m, q, v)


def test_inputs_are_what_the_gpu_tests_say():
    """the windows' properties the GPU tests rely on, checked without a device: the unit kinds of the item-count family, the packing of the
    21-block window, depths 0.5 .. 50, |t| up to 10, both sides of the Huber delta"""
    for case, n_co in zip(S.cases("counts"), S.COUNTS):
        lin = S.linearise(case["win"], S.host_estimates(case["win"]), np.float64)
        both = np.bincount(lin["lh"][lin["free"]], minlength=len(lin["hpoint"])) == 2
        assert both.sum() == n_co
    for family in ("counts", "pack", "diag", "sizes", "degree", "kinds"):
        for case in S.cases(family):
            est = S.host_estimates(case["win"])
            lin = S.linearise(case["win"], est, np.float64)
            assert 0.5 <= lin["depth"].min() and lin["depth"].max() <= 50, (case["name"], lin["depth"].min(), lin["depth"].max())
            assert np.abs(est["pose"][:, 4:]).max() <= 10.5
            frac = lin["beyond"].mean()
            assert 0.2 <= frac <= 0.8, (case["name"], frac)
