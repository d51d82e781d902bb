"""tests/ldlt_ref.py held to account without a GPU: the long double solve against 50-digit arithmetic, the backward-error measure against
its own formula evaluated at 50 digits, the condition omega <= 1 met by both float64 models on every system the GPU test runs, and
the exactness of the dyadic family."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldlt_ref as R  # noqa: E402

import mpmath as mp  # noqa: E402


def _mp_ldlt(H):
    n = H.shape[0]
    A = mp.matrix(H.tolist())
    L, d = mp.eye(n), [mp.mpf(0)] * n
    for j in range(n):
        d[j] = A[j, j]
        for i in range(j + 1, n):
            L[i, j] = A[i, j] / d[j]
        for i in range(j + 1, n):
            for c in range(j + 1, i + 1):
                A[i, c] -= L[i, j] * A[c, j]
                A[c, i] = A[i, c]
    return L, d


def _mp_bound_matrix(L, d, n):
    """|L| |D| |L|^T at 50 digits"""
    aL = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            aL[i, j] = abs(L[i, j])
    aD = mp.diag([abs(v) for v in d])
    return aL * aD * aL.T


@pytest.mark.parametrize("family", R.FLOAT_FAMILIES)
def test_long_double_solve_against_50_digits(family):
    """x of the long double solve lies within the forward bound that follows from ITS backward bound, unit roundoff 2^-64:
    |x - x_exact| <= (3n+1) 2^-64 |H^-1| |L||D||L|^T |x| componentwise, everything on the right at 50 digits.  And omega() of a float64
    solution equals the same formula evaluated at 50 digits to 2^-11 absolute: the long double residual b - H x is off by at most
    (n + 1) 2^-64 (|H| |x|)_i, and |H| <= |L||D||L|^T, so omega is off by at most (n + 1) 2^-64 / ((3n + 1) 2^-53) < 2^-11 -- the
    measure resolves 5e-4 where the condition is omega <= 1 (the factors' own rounding moves the denominator by parts in 1e-17)."""
    mp.mp.dps = 50
    for np_ in (1, 2, 3):
        H, b = R.system(family, np_)
        n = len(b)
        Ll, dl, xl = R.ldlt_solve(H, b, R.LD)
        Hm, bm = mp.matrix(H.tolist()), mp.matrix(b.tolist())
        xm = mp.lu_solve(Hm, bm)
        Lm, dm = _mp_ldlt(H)
        Bm = _mp_bound_matrix(Lm, dm, n)
        Hinv = Hm ** -1
        absinv = mp.matrix(n, n)
        for i in range(n):
            for j in range(n):
                absinv[i, j] = abs(Hinv[i, j])
        fw = absinv * (Bm * mp.matrix([abs(mp.mpf(float(v))) + abs(mp.mpf(float(v - R.LD(float(v))))) for v in xl]))
        for i in range(n):
            xi = mp.mpf(float(xl[i])) + mp.mpf(float(xl[i] - R.LD(float(xl[i]))))   # the long double value, exactly, as two doubles
            assert abs(xi - xm[i]) <= (3 * n + 1) * mp.mpf(2) ** -64 * fw[i], (family, np_, i)
        # the measure itself, on the float64 solve of the same system
        xf = R.ldlt_solve(H, b, np.float64)[2]
        got, _ = R.omega(H, b, xf, Ll, dl)
        xfm = mp.matrix(xf.tolist())
        res = bm - Hm * xfm
        den = Bm * mp.matrix([abs(v) for v in xfm])
        want = max(abs(res[i]) / ((3 * n + 1) * mp.mpf(2) ** -53 * den[i]) for i in range(n))
        assert abs(got - float(want)) <= 2.0 ** -11 + 1e-6 * float(want), (family, np_, got, float(want))


def test_both_float64_models_meet_the_condition_on_every_gpu_system():
    """omega <= 1 is satisfiable: the plain float64 recurrence and the float64 model of the blocked form (explicit T_k, W = A T^T,
    L = W / d) both stay far below it on every system tests/test_lba_reduced_gpu.py runs.  Worst values when this was written,
    plain / blocked: bench 0.06 / 0.06, graded 0.10 / 0.08, lm 0.02 / 0.15, indef 0.04 / 0.06."""
    worst = {}
    for family, np_, _ in R.gpu_systems():
        H, b, L, d = R.reference(family, np_)
        for name, sol in (("plain", R.ldlt_solve(H, b, np.float64)), ("blocked", R.blocked_f64(H, b))):
            assert sol is not None
            om, row = R.omega(H, b, sol[2], L, d)
            worst[family, name] = max(worst.get((family, name), 0.0), om)
            assert om <= 1.0, (family, np_, name, om, row)
    print({k: round(v, 3) for k, v in worst.items()})


def test_dyadic_family_is_exact_in_both_float64_models():
    """x0, L and D bit for bit at every size the GPU test runs, also with H and b scaled by 2^200 and 2^-200; a zero in D is a zero
    pivot in both; the magnitudes stay small (H and b: a few hundred)"""
    for np_ in R.ALL_NP:
        H, b, x0, L, D = R.dyadic_system(np_)
        assert np.abs(H).max() <= 64 and np.abs(b).max() <= 4096
        for s in (1.0, 2.0 ** 200, 2.0 ** -200):
            for sol in (R.ldlt_solve(H * s, b * s, np.float64), R.blocked_f64(H * s, b * s)):
                assert sol is not None
                assert (sol[2] == x0).all() and (sol[0] == L).all() and (sol[1] == D * s).all(), (np_, s)
    for np_, j in ((1, 0), (3, 15), (3, 16), (7, 31), (5, 29), (8, 47), (40, 120)):
        H, b, *_ = R.dyadic_system(np_, zero_at=j)
        assert R.ldlt_solve(H, b, np.float64) is None and R.blocked_f64(H, b) is None and R.ldlt_solve(H, b, R.LD) is None
        Hn = H.copy()
        Hn[j, j] = np.nan
        assert R.ldlt_solve(Hn, b, np.float64) is None and R.blocked_f64(Hn, b) is None
