"""k_ldlt_reg (csrc/ldlt_reg.h) and k_ldlt_dev (csrc/lba.hip: ldlt_body) alone -- the linear solve of a Levenberg-Marquardt trial and
its epilogue, through the tap aos2_debug_lba_reduced_solve_device, which launches the shipped kernels with the shipped LDS sizing --
against tests/ldlt_ref.py.  The condition on a float solve is omega <= 1 (ldlt_ref.omega: componentwise backward error in units of
the bound of an unpivoted LDL^T solve in float64, factors and residual in long double); a solve that is exact by construction
(the dyadic family) must be exact.

Worst omega, float64 models on the CPU (tests/test_ldlt_ref_cpu.py), plain recurrence / blocked model:
    bench 0.06 / 0.06, graded 0.10 / 0.08, lm 0.02 / 0.15, indef 0.04 / 0.06
Worst omega measured on the MI355X, k_ldlt_reg / k_ldlt_dev (DESIGN.md 5.3 has the table):
    bench 0.062 / 0.062, graded 0.048 / 0.101, lm 0.084 / 0.042, indef 0.039 / 0.043
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ldlt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

X_SENT, S_SENT = 7.25, -3.5     # what x / scale_terms hold on entry
FORM_NAME = {2: "k_ldlt_reg", 0: "k_ldlt_dev"}


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def poses(rng, q):
    qt = rng.normal(size=(q, 4))
    qt /= np.linalg.norm(qt, axis=1, keepdims=True)
    qt[qt[:, 3] < 0] *= -1
    return np.concatenate([qt, rng.normal(0, 3.0, (q, 3))], 1)


def case(form, H, b, rng, **extra):
    n = len(b)
    c = dict(form=form, H=H, bs=b, b_pose=rng.normal(size=n), x0=np.full(n, X_SENT), scale0=np.full(n, S_SENT),
             lam=10.0 ** rng.uniform(-6, 2), T=poses(rng, n // 6))
    c.update(extra)
    return c


def where(c, row=None):
    n = len(c["bs"])
    s = f"{FORM_NAME[c['form']]} np={n // 6} n={n} nb={(n + 15) // 16}"
    return s if row is None else s + f" worst row {row} (16-block {row // 16})"


def check_epilogue(c, g, oracle=None):
    """a healthy case's epilogue: backup, scale terms bit for bit; the pose update when the oracle is given"""
    assert g["ok"] == 1, where(c)
    assert bits(g["T_backup"]) == bits(c["T"]), where(c)
    assert bits(g["scale_terms"]) == bits(g["x"] * (c["lam"] * g["x"] + c["b_pose"])), where(c)   # (-ffp-contract=off: no FMA)
    if oracle is not None:
        for i, T in enumerate(c["T"]):
            want = oracle.se3_mul(oracle.se3_exp(g["x"][6 * i:6 * i + 6]), T)
            assert np.abs(g["T_out"][i] - want).max() < 1e-12 * (1 + np.abs(want).max()), (where(c), i, g["T_out"][i], want)


def check_failed(c, g):
    assert g["ok"] == 0, where(c)
    assert bits(g["x"]) == bits(c["x0"]) and bits(g["scale_terms"]) == bits(c["scale0"]), where(c)
    assert bits(g["T_out"]) == bits(c["T"]) and bits(g["T_backup"]) == bits(c["T"]), where(c)


def test_every_size_both_forms(pkg, gpu):
    """omega <= 1: the register form at every np in 1..40 (every nb in 1..15; np = 8, 16, 24, 32, 40 without an identity tail), the
    device-memory form at np in {1, 2, 3, 5, 8, 16, 24, 40, 41, 43, 48, 56, 64}, four families of systems each, one launch.  Where
    both forms ran the same system both must meet the condition (they are not compared with each other)."""
    rng = np.random.default_rng(1)
    cases, key = [], []
    for family, q, forms in R.gpu_systems():
        H, b, _, _ = R.reference(family, q)
        for form in forms:
            cases.append(case(form, H, b, rng))
            key.append((family, q))
    got = pkg.capi.debug_lba_reduced_solve_device(cases)
    worst, bad = {}, []
    for c, g, (family, q) in zip(cases, got, key):
        _, _, L, d = R.reference(family, q)
        om, row = (np.inf, 0) if g["ok"] != 1 else R.omega(c["H"], c["bs"], g["x"], L, d)
        k = (FORM_NAME[c["form"]], family)
        if om > worst.get(k, (0.0, ""))[0]:
            worst[k] = (om, where(c, row))
        if not om <= 1.0:
            bad.append(f"{family}: omega {om:.3g}, ok {g['ok']}: {where(c, row)}")
        if g["ok"] == 1:
            check_epilogue(c, g)
    for k in sorted(worst):
        print(f"worst omega {k[0]} {k[1]}: {worst[k][0]:.3f} at {worst[k][1]}")
    assert not bad, "\n".join(bad)


def test_dyadic_systems_are_solved_exactly(pkg, gpu):
    """The dyadic family (every intermediate of any elimination order a small dyadic number, every reciprocal pivot a power of two):
    x == x0 for both forms at every size, also with H and b scaled by 2^200 and 2^-200.  Bit for bit up to the sign of a zero: an
    x0_i = 0 can legitimately come out as -0.0 (0 / negative pivot), so both sides pass through `+ 0.0` first."""
    rng = np.random.default_rng(2)
    cases, want = [], []
    for form, sizes in ((2, R.REG_NP), (0, R.DEV_NP)):
        for q in sizes:
            H, b, x0, _, _ = R.dyadic_system(q)
            for s in (1.0, 2.0 ** 200, 2.0 ** -200):
                cases.append(case(form, H * s, b * s, rng))
                want.append(x0)
    got = pkg.capi.debug_lba_reduced_solve_device(cases)
    bad = []
    for c, g, x0 in zip(cases, got, want):
        if g["ok"] != 1 or bits(g["x"] + 0.0) != bits(x0 + 0.0):
            rows = np.nonzero(~(g["x"] == x0))[0]
            bad.append(f"{where(c)} scale {np.abs(c['H']).max():.3g}: ok {g['ok']}, {len(rows)} rows differ, first {rows[:4]} (16-blocks {rows[:4] // 16})")
        else:
            check_epilogue(c, g)
    assert not bad, "\n".join(bad)


def test_reciprocal_pivots_are_within_one_ulp(pkg, gpu):
    """Both kernels multiply by 1 / d_j from v_rcp_f64 + two Newton steps, documented as "1 / d within 1 ulp" (lr_rcp, rcp_newton).  A
    diagonal H with b = 1 returns exactly those reciprocals as x (every other term of both substitutions is a product with an exact
    zero), so the contract is checked as it stands: |x_i - 1 / d_i| <= ulp(1 / d_i), the quotient in long double, over 13 k pivots with
    random significands, both signs and exponents in +-30, in every block of the largest size of either form."""
    rng = np.random.default_rng(7)
    cases = []
    for form, q, count in ((2, 40, 40), (0, 64, 10)):
        for _ in range(count):
            n = 6 * q
            d = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-30, 31, n)
            cases.append(case(form, np.diag(d), np.ones(n), rng))
    got = pkg.capi.debug_lba_reduced_solve_device(cases)
    worst = {}
    for c, g in zip(cases, got):
        assert g["ok"] == 1, where(c)
        want = R.LD(1) / np.diag(c["H"]).astype(R.LD)
        err = np.abs(g["x"].astype(R.LD) - want) / np.spacing(np.abs(want.astype(np.float64))).astype(R.LD)
        i = int(np.argmax(err))
        worst[c["form"]] = max(worst.get(c["form"], 0.0), float(err[i]))
        assert err[i] <= 1.0, (where(c, i), float(err[i]), c["H"][i, i], g["x"][i])
    print("worst reciprocal error in ulp:", {FORM_NAME[k]: round(v, 4) for k, v in worst.items()})


def test_zero_and_nan_pivots_fail_and_nothing_else_does(pkg, gpu):
    """SimplicialLDLT's rule: an exactly zero pivot (the dyadic family with d_j = 0: the arithmetic before the pivot is exact, so the
    device meets an exact zero) or a NaN one (H[j][j] = NaN) fails the solve -- ok = 0, x and the scale terms as the caller passed
    them, pose and backup both the trial's starting pose -- at j in {0, 15, 16, 31, n/2, n-1}, which includes the last pivot of a
    size without tail and pivots in the last block of padded sizes; an indefinite matrix without a zero does not fail.  Healthy cases
    before, between and after the failing ones in the same launch are solved exactly."""
    rng = np.random.default_rng(3)
    cases, kind = [], []

    def healthy(form, q, seed):
        H, b, x0, _, D = R.dyadic_system(q, seed=seed)
        assert (D < 0).any() and (D > 0).any() or q == 1
        cases.append(case(form, H, b, rng))
        kind.append(x0)

    for form, sizes in ((2, (1, 3, 6, 8, 40)), (0, (1, 3, 6, 8, 43))):
        for q in sizes:
            n = 6 * q
            healthy(form, q, 100)
            for t, j in enumerate(sorted({j for j in (0, 15, 16, 31, n // 2, n - 1) if j < n})):
                Hz, bz, *_ = R.dyadic_system(q, zero_at=j, seed=t)
                cases.append(case(form, Hz, bz, rng))
                kind.append("zero pivot %d" % j)
                Hn, bn, *_ = R.dyadic_system(q, seed=t)
                Hn = Hn.copy()
                Hn[j, j] = np.nan
                cases.append(case(form, Hn, bn, rng))
                kind.append("NaN pivot %d" % j)
                healthy(form, q, 101 + t)
    got = pkg.capi.debug_lba_reduced_solve_device(cases)
    for c, g, k in zip(cases, got, kind):
        if isinstance(k, str):
            try:
                check_failed(c, g)
            except AssertionError as e:
                raise AssertionError(f"{k}: {e}") from None
        else:
            assert g["ok"] == 1 and bits(g["x"] + 0.0) == bits(k + 0.0), where(c)
            check_epilogue(c, g)


def test_epilogue_pose_update_and_scale_terms(pkg, oracle, gpu):
    """On healthy solves: T_backup = T and scale_terms = x (lambda x + b_pose) bit for bit, T_out = exp(x_i) T_i to the 1e-12 that
    test_pose_solver_building_blocks holds se3_oplus_fast to -- with right-hand sides b = H x_target whose rotation parts span tiny
    (below 1e-5 rad: the first-order branch), small and 0.05-0.7 rad updates."""
    rng = np.random.default_rng(4)
    cases = []
    for form, sizes in ((2, (1, 7, 19, 40)), (0, (5, 41, 64))):
        for q in sizes:
            H, _, _, _ = R.reference("bench", q)
            ax = rng.normal(size=(q, 3))
            ax /= np.linalg.norm(ax, axis=1, keepdims=True)
            ang = np.array([(10.0 ** rng.uniform(-9, -5.3), 10.0 ** rng.uniform(-4.7, -1.4), rng.uniform(0.05, 0.7))[(i + q) % 3] for i in range(q)])
            xt = np.concatenate([ax * ang[:, None], rng.normal(0, 0.5, (q, 3))], 1).ravel()
            cases.append(case(form, H, H @ xt, rng))
    got = pkg.capi.debug_lba_reduced_solve_device(cases)
    seen = np.zeros(3, int)
    for c, g in zip(cases, got):
        check_epilogue(c, g, oracle)
        th = np.linalg.norm(g["x"].reshape(-1, 6)[:, :3], axis=1)
        seen += [(th < 1e-5).sum(), ((th >= 1e-5) & (th < 0.05)).sum(), ((th >= 0.05) & (th <= 0.7)).sum()]
    assert (seen >= 10).all(), seen


def test_cases_of_one_launch_do_not_depend_on_each_other(pkg, gpu):
    """One launch whose cases mix 1, 40 and 64 free keyframes of both forms in shuffled order -- the LDS is sized by the largest, every
    case lays itself out by its own npad -- gives every case the bits it gives as the only case of a call."""
    rng = np.random.default_rng(5)
    cases = []
    for family in ("bench", "lm"):
        for form, q in ((2, 1), (0, 1), (2, 40), (0, 40), (0, 64)):
            H, b, _, _ = R.reference(family, q)
            cases.append(case(form, H, b, rng))
    cases = [cases[i] for i in rng.permutation(len(cases))]
    together = pkg.capi.debug_lba_reduced_solve_device(cases)
    for c, g in zip(cases, together):
        alone = pkg.capi.debug_lba_reduced_solve_device([c])[0]
        assert g["ok"] == alone["ok"] == 1, where(c)
        for k in ("x", "scale_terms", "T_out", "T_backup"):
            assert bits(g[k]) == bits(alone[k]), (where(c), k)


def test_which_parts_of_the_matrix_each_form_reads(pkg, gpu):
    """k_ldlt_reg loads the diagonal 16 x 16 tiles and the strictly UPPER block triangle (its tiles are stored transposed), k_ldlt_dev
    whole diagonal blocks and the strictly LOWER block triangle: NaNs everywhere else change no bit of the result.
    (k_schur writes both triangles today: this is what a change to it may stop writing.)"""
    rng = np.random.default_rng(6)
    cases = []
    for form, sizes in ((2, (3, 7, 16, 40)), (0, (3, 7, 16, 43))):
        for q in sizes:
            H, b, _, _ = R.reference("graded", q)
            blk = np.arange(6 * q) // 16
            unread = blk[:, None] > blk[None, :] if form == 2 else blk[:, None] < blk[None, :]
            assert unread.any()
            c = case(form, H, b, rng)
            cases += [c, dict(c, H=np.where(unread, np.nan, H))]
    got = pkg.capi.debug_lba_reduced_solve_device(cases)
    for i in range(0, len(cases), 2):
        clean, poisoned = got[i], got[i + 1]
        assert clean["ok"] == poisoned["ok"] == 1, where(cases[i])
        for k in ("x", "scale_terms", "T_out", "T_backup"):
            assert bits(clean[k]) == bits(poisoned[k]), (where(cases[i]), k)


def test_a_window_beyond_the_lds_cap_is_refused(pkg, gpu):
    """155 free keyframes: k_ldlt_dev's panel and vectors would need more LDS than a compute unit has; aos2_lba_solve says so with
    AOS2_ERR_ARG before anything is enqueued (nothing near the cap is launched here)."""
    ba = pkg.LocalBA()
    with pytest.raises(pkg.capi.AosError) as e:
        ba.LocalBundleAdjustment(R.lba_star_window(155))
    assert e.value.code == pkg.capi.AOS2_ERR_ARG and "155 free keyframes" in str(e.value)
    small = pkg.synth.synth_lba_problem(1, n_local=3, n_fixed=2, n_points=60, stereo_frac=0.5)
    assert ba.LocalBundleAdjustment(small)["status"] == 0   # the handle is as good as before
