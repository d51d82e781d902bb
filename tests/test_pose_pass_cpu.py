"""tests/pose_pass_ref.py checked on its own, without a device: the Jacobians against central differences, the two float64 models of the edge
pass against the long-double reference on every input of tests/test_pose_pass_gpu.py (omega <= 16, the bound test_lba_system_cpu.py holds its
models to), the inputs' properties the GPU tests rely on, and the evidence that the GPU tests' criterion -- omega <= 4 x the worst omega of
the models over the family -- rejects wrong assemblies that the end-to-end criterion (Tcw within 1e-5, equal outlier flags) lets pass."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_pass_ref as P  # noqa: E402
from test_lba_system_cpu import se3_exp_ld  # noqa: E402

LD = P.LD


@pytest.mark.parametrize("stereo", [0, 1])
def test_jacobians_equal_central_differences(stereo):
    """linearizeOplus of both pose-only edges against central differences of the reference's own residual under exp(xi) T, in long double, at
    two steps: the difference falls with the square of the step, and at h = 1e-5 it is below 1e-7 of the Jacobian's scale.  The stereo rows
    are differenced on a residual with an exact reciprocal (the float one of cam_project is a step function)."""
    base = P.problem(30 + stereo, 12, stereo, stereo_frac=float(stereo))
    assert np.asarray(base["stereo"]).all() == bool(stereo) and np.asarray(base["stereo"]).any() == bool(stereo)
    p = P.camera_points(base, LD)
    J = np.array([[c.v for c in row] for row in P.jacobian(base, p, LD)])   # [3, 6, n]
    p0 = np.array([c.v for c in p])   # [3, n]

    def res(pc):
        e, _ = P.residual(base, [P.VM(pc[i]) for i in range(3)], LD, exact_reciprocal=True)
        return np.array([c.v for c in e])

    errs = []
    for h in (LD(1e-4), LD(1e-5)):
        fd = np.zeros_like(J)
        for k in range(6):
            xi = np.zeros(6, LD)
            xi[k] = h
            (Ra, ta), (Rb, tb) = se3_exp_ld(xi), se3_exp_ld(-xi)
            fd[:, k] = (res(Ra @ p0 + ta[:, None]) - res(Rb @ p0 + tb[:, None])) / (2 * h)
        errs.append(float((np.abs(fd - J).max(axis=(0, 1)) / np.abs(J).max(axis=(0, 1))).max()))
    assert errs[1] < 1e-7 and errs[1] < errs[0] / 50, errs
    if not stereo:
        assert not J[2].any()


@pytest.mark.parametrize("family,form", P.PASS_FAMILIES)
def test_float64_models_against_the_reference(family, form):
    """both float64 models on every input of the GPU tests' edge-pass families: worst omega per quantity, printed, below 16"""
    worst = {"textbook": {}, "kernel": {}}
    for case in P.cases(family, form):
        _, per = P.model_omegas(case)
        for m in per:
            for q, v in per[m].items():
                worst[m][q] = max(worst[m].get(q, 0.0), v)
    for q in P.QUANTITIES:
        print(f"worst omega {family:8s} form {form} {q:9s} textbook {worst['textbook'][q]:9.3g}   kernel form {worst['kernel'][q]:9.3g}")
    for m in worst:
        for q, v in worst[m].items():
            assert v <= 16.0, (family, form, m, q, v)


def test_recomputed_chi2_models_against_the_reference():
    """the outlier pass's chi2 of an edge: the quaternion-rotate form (po_edge_error) and the matrix form in float64, omega <= 16"""
    for form in range(4):
        for case in P.cases("slots", form):
            ref = P.reference(case)
            every = np.ones(case["n"], bool)
            for got in (P.chi2_quat_f64(case), P.model_kernel(case, form)["chi2_edge"]):
                assert P.omegas(ref, dict(chi2_edge=got), every)["chi2_edge"] <= 16.0, (form, case["name"])


def test_inputs_are_what_the_gpu_tests_say():
    """Huber shares (at least 20 % of the active edges on each side of delta^2 where the edges are robust, every frame with n >= 64), the
    depth ranges, no frame left out for a float reciprocal at a rounding boundary, the outlier decisions left out within 1 in 1000, and
    the slot counts per wave the sizes were chosen for"""
    for family, form in P.PASS_FAMILIES:
        for case in P.cases(family, form):
            name = (family, form, case["name"])
            assert case["n"] <= (P.FORM_MAX[form] or case["n"])
            assert not P.near_float_boundary(case).any(), name
            ref = P.reference(case)
            d = ref["depth"].astype(np.float64)
            if family != "geometry":
                assert 2.5 < d.min() and d.max() < 41, name
                if case["n"] >= 64 and P.flags(case, "robust", 1).all():
                    share = ref["beyond"][ref["active"]].mean()
                    assert 0.2 <= share <= 0.8, (name, share)
    for form in (0, 3):
        g = {c["name"]: (c, P.reference(c)["depth"].astype(np.float64)) for c in P.cases("geometry", form)}
        d = g["depth"][1]
        assert 0.5 <= d.min() < 0.7 and 40 < d.max() <= 50
        c = g["far_pose"][0]
        assert 9.9 < np.abs(c["pose"][4:]).max() <= 10.1 and 2 * np.arccos(abs(c["pose"][3])) > np.pi - 0.05
        w = g["levels"][0]["inv_sigma2"]
        assert len(np.unique(w)) == 8 and np.allclose(np.sort(np.unique(w))[0], 1.2 ** -14, rtol=1e-5)
        assert 0.15 < (g["behind"][1] < 0).mean() < 0.25 and (np.abs(g["behind"][1]) > 2.5).all()
    # slot counts: the slots family of a form reaches every count of slots a wave can use, and n = 300 gives waves of different counts
    for form, (ept, nt) in enumerate(P.FORMS):
        counts = set()
        for n in P.SLOT_SIZES[form]:
            per_wave = [max(0, (n - 64 * w + nt - 1) // nt) for w in range(nt // 64)]
            counts |= set(per_wave)
            if form == 0 and n == 300:
                assert len(set(per_wave)) == 2
        if ept:
            assert counts >= set(range(1, ept + 1)) - ({2, 3, 4, 7} if form == 1 else {3, 4, 5, 6, 7} if form == 2 else set()), (form, counts)
    # outlier decisions left out: at most 1 in 1000 over the whole family, on the reference alone
    left = total = 0
    for form in range(4):
        tol = P.recomputed_tolerance(form)
        for case in P.cases("outlier", form):
            o = P.outlier_reference(case, tol)
            left += int(o["left_out"].sum())
            total += case["n"]
            assert case["outlier"].sum() == max(1, case["n"] // 3) and (case["level1"] == case["outlier"]).all()
            assert (np.asarray(case["chi2"])[case["outlier"] == 1] == 1e9).all()
    assert left * 1000 <= total, (left, total)


@pytest.mark.parametrize("mutation", P.MUTATIONS)
def test_the_criterion_rejects_wrong_assemblies(mutation):
    """a wrong assembly applied to the kernel-form model exceeds, on some quantity of some frame, the tolerance the GPU test applies to the
    family -- for every form, on the families that have what the mistake needs (a level-1 edge: the flags family)"""
    for form in range(4):
        family = "flags" if mutation == "level1_chi2" else "slots"
        cases = P.cases(family, form)
        tol = P.family_tolerance(cases)
        caught = []
        for case in cases:
            om = P.omegas(P.reference(case), P.model_kernel(case, form, mutate=mutation))
            caught += [(case["name"], q, v) for q, v in om.items() if v > tol[q]]
        assert caught, (mutation, form)
        right = [q for case in cases for q, v in P.omegas(P.reference(case), P.model_kernel(case, form)).items() if v > tol[q]]
        assert not right, (form, right)
        print(f"{mutation:12s} form {form}: {len(caught)} quantities of {len(cases)} frames beyond the tolerance, worst "
              f"{max(caught, key=lambda t: t[2] / tol[t[1]])}")
