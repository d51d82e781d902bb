"""Optimizer::OptimizeSim3 (src/Optimizer.cc:1047-1242) without a GPU: the CPU restatement the GPU tests compare against
(tests/sim3_opt_ref.py) checked against independent knowledge (planted transformations, the closed-form Jacobian of the two
projections, the identity, continuity of the exponential's branches), the library's host tap (aos2_debug_sim3_opt_host: the header
the device kernel runs, csrc/sim3_opt.h) checked against it under the comparison rule, the conditions the shared generator's seeds
have to meet, the argument checks, and the host class's compile + link."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_opt_ref as R  # noqa: E402

SEEDS = (3, 4)
DBL_EPSILON = 2.0 ** -52


def planted_error(res, planted):
    return (np.abs(R.rot_of(np.asarray(res["q12"])) - planted["R"]).max(), np.abs(np.asarray(res["t12"]) - planted["t"]).max(),
            abs(float(res["s12"]) - planted["s"]))


@pytest.mark.parametrize("fix_scale", [False, True])
def test_noise_free_problems_give_the_planted_sim3_back(pkg, fix_scale):
    """1e-6 in R and s, 1e-5 in t, from a start 0.01 rad / 2 cm / 1 % away: the restatement, and the host tap on the same problems.
    The keyframes are up to 1.5 m apart per axis: s moves no projection of e21 and those of e12 only through t / s, so with the two
    cameras in one place the scale is a flat valley in which ten LM iterations do not arrive, here or in g2o (with |t| <= 0.3 m and
    150 points the restatement and the tap both stop 8e-5 short in s after 5 + 5 iterations, half of their trials rejected)."""
    rng = np.random.default_rng(21)
    probs = [R.problem(rng, n, 0, fix_scale, False, noise=0.0, baseline=1.5) for n in (12, 40, 150)]
    taps = pkg.capi.debug_sim3_opt_host(probs)
    for P, tap in zip(probs, taps):
        for name, res in (("restatement", R.optimize_sim3(P)), ("host tap", tap)):
            dR, dt, ds = planted_error(res, P["planted"])
            print(name, "n", len(P["X1c"]), "dR %.2e dt %.2e ds %.2e" % (dR, dt, ds), "iterations", res["iterations"])
            assert res["n_inliers"] == len(P["X1c"]) and res["n_bad"] == 0
            assert dR <= 1e-6 and ds <= 1e-6 and dt <= 1e-5


closed_form_jacobians = R.closed_form_jacobians   # (shared with the step tests)


def test_central_difference_jacobian_agrees_with_the_closed_form():
    """Bound, per entry of J: the truncation error of a central difference is f''' delta^2 / 6 ~ 1e-15, nothing; what is left is the
    rounding of the two residuals that are subtracted.  A residual is obs - (x / z * f + c): about k = 20 roundings (the quaternion
    rotation, the scale, the division, the camera map), each relative DBL_EPSILON / 2 of an intermediate whose image-plane size is at
    most M = the largest |pixel coordinate| among obs and the projections, so |error of e| <= k M DBL_EPSILON / 2, the difference of
    two twice that, times scalar = 1 / (2 delta):  |J - J_closed| <= k M DBL_EPSILON / (2 delta)."""
    worst = 0.0
    for seed in range(6):
        P = R.problem(np.random.default_rng(40 + seed), 60, 0, False, seed % 2 == 1)
        G = R.Graph(P, np.float64)
        S = (np.asarray(P["q12"]), np.asarray(P["t12"]), np.float64(P["s12"]))
        J12, J21 = G.jacobians(S, False)
        C12, C21 = closed_form_jacobians(G, S)
        e12, e21 = G.residuals(S)
        M = max(np.abs(G.o1).max(), np.abs(G.o2).max(), np.abs(G.o1 - e12).max(), np.abs(G.o2 - e21).max())
        bound = 20 * M * DBL_EPSILON / (2 * R.DELTA)
        err = max(np.abs(J12 - C12).max(), np.abs(J21 - C21).max())
        worst = max(worst, err / bound)
        print("seed", seed, "largest |J| %.1f" % max(np.abs(C12).max(), np.abs(C21).max()), "largest difference %.3e" % err, "bound %.3e" % bound)
        assert err <= bound
        Jf, _ = G.jacobians(S, True)   # _fix_scale: both perturbations of column 6 are the same transform
        assert (Jf[:, :, 6] == 0).all() and (Jf[:, :, :6] == J12[:, :, :6]).all()
    print("worst difference / bound:", worst)


def test_exp_of_a_zero_update_is_the_identity_and_the_branches_are_continuous():
    q, t, s = R.sim3_exp(np.zeros(7))
    assert (q == [0, 0, 0, 1]).all() and (t == 0).all() and s == 1.0
    S = (np.array([0.1, -0.2, 0.3, 0.9]), np.array([0.5, -1.0, 2.0]), 1.3)
    q, t, s = R.sim3_mul(R.sim3_exp(np.zeros(7)), S)
    assert (q == S[0]).all() and (t == S[1]).all() and s == S[2]
    # across eps = 1e-5 the formulas change, not the function.  What a crossing may cost (|upsilon| = v):
    #   theta: R = I + Omega + Omega^2 against Rodrigues (Omega^2 / 2): theta^2 / 2 = 5e-11 in R, i.e. in q; B = 1/6 against
    #          (theta - sin theta) / theta^3, whose numerator is all cancellation: up to B theta^2 v = 1e-10 v / 6; A: 1e-6 relative
    #          (cancellation in 1 - cos) of theta v / 2: 5e-12 v.  Together below 2e-10 (1 + v).
    #   sigma: C = 1 against (s - 1) / sigma = 1 + sigma / 2 + ...: sigma v / 2 = 5e-6 v in t (g2o's own approximation), A and B
    #          change by sigma / 3 and sigma / 8 of terms that carry theta and theta^2.  Below 0.51 eps v.
    #   theta at |sigma| >= eps: sim3.h:116 reads B = (sigma^2 / 2 - sigma + 1) s / sigma^3 where the limit of the general branch's
    #          B (:132) is that minus 1 / sigma^3 (about 1/6): as written it is about 1 / sigma^3, and B Omega^2 upsilon jumps by
    #          B theta^2 v at the crossing (1.7e-5 at sigma = 0.02, and without bound as sigma comes down to eps).  Reproduced as
    #          written; the bound uses the line's own value.
    # plus the distance of the two arguments (2e-14) times a Lipschitz constant of order 1 + v.
    axis = np.array([0.6, -0.48, 0.64])
    ups = np.array([0.7, -1.1, 0.4])
    v = np.linalg.norm(ups)
    step = 1e-9

    def jump(u_lo, u_hi):
        a, b = R.sim3_exp(u_lo), R.sim3_exp(u_hi)
        return max(np.abs(a[0] - b[0]).max(), np.abs(a[1] - b[1]).max(), abs(a[2] - b[2]))

    for sigma in (0.0, 0.3 * R.EPS, 0.02):   # theta crosses eps in both sigma branches
        lo = np.concatenate([axis * R.EPS * (1 - step), ups, [sigma]])
        hi = np.concatenate([axis * R.EPS * (1 + step), ups, [sigma]])
        assert np.linalg.norm(lo[:3]) < R.EPS < np.linalg.norm(hi[:3])
        j = jump(lo, hi)
        print("theta crossing at sigma = %g: jump %.3e" % (sigma, j))
        B_line_116 = (0.5 * sigma * sigma - sigma + 1) * np.exp(sigma) / sigma ** 3 if sigma >= R.EPS else 0.0
        assert j <= 2e-10 * (1 + v) + 4 * (1 + v) * 2e-14 + B_line_116 * R.EPS ** 2 * v
    for theta in (0.0, 0.3 * R.EPS, 0.02):   # sigma crosses eps in both theta branches, from both signs
        for sign in (1.0, -1.0):
            lo = np.concatenate([axis * theta, ups, [sign * R.EPS * (1 - step)]])
            hi = np.concatenate([axis * theta, ups, [sign * R.EPS * (1 + step)]])
            j = jump(lo, hi)
            print("sigma crossing at theta = %g, sign %+d: jump %.3e" % (theta, sign, j))
            # (0 < theta < eps: the side with |sigma| >= eps is line :116 again, there about theta^2 v / eps^3 = 1e5 theta^2 v / eps^2)
            B_line_116 = (0.5 * R.EPS ** 2 - R.EPS + 1) * np.exp(R.EPS) / R.EPS ** 3 * 1.01 if 0 < theta < R.EPS else 0.0
            assert j <= 0.51 * R.EPS * v + 4 * (1 + v) * 2e-14 + B_line_116 * theta ** 2 * v


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_seed_meets_its_conditions(seed):
    c = R.generator_case(seed)
    P, w = c["problems"], c["want"]
    assert tuple(len(p["X1c"]) for p in P) == R.SIZES and set((0, 9, 10, 31, 32, 33, 64, 127, 128, 129, 300)) <= set(R.SIZES)
    print(seed, "n_bad", [x["n_bad"] for x in w], "n_inliers", [x["n_inliers"] for x in w], "iterations", [x["iterations"] for x in w],
          "trials", [x["trials"] for x in w], "rejected", [x["rejected"] for x in w], "margin", ["%.1e" % x["margin"] for x in w],
          "dropped", c["dropped"], "of", c["drawn"])
    # no decision hangs on rounding: every chi2 at :1194 and :1228 keeps a relative 1e-3 from th2, and that cost few candidates
    assert min(x["margin"] for x in w) >= R.MARGIN
    assert 2 * c["dropped"] <= c["drawn"]
    assert any(x["wrote"] and x["n_bad"] == 0 and x["iterations"][1] <= 5 for x in w)     # 5 further iterations
    assert any(x["wrote"] and x["n_bad"] > 0 for x in w)                                   # 10 further iterations
    assert any(not x["wrote"] and x["outlier"].any() for x in w)                           # :1212 with matches erased
    assert any(x["rejected"] > 0 for x in w)                                               # a rejected trial
    assert {bool(p["fix_scale"]) for p, x in zip(P, w) if x["wrote"]} == {True, False}
    i0, i9 = R.SIZES.index(0), R.SIZES.index(9)
    assert (w[i0]["n_inliers"], w[i0]["n_bad"], w[i0]["wrote"], w[i0]["iterations"]) == (0, 0, 0, [0, 0])
    assert w[i9]["n_inliers"] == 0 and not w[i9]["wrote"] and w[i9]["iterations"][0] > 0 and w[i9]["iterations"][1] == 0
    assert any(x["wrote"] and x["n_inliers"] == 10 for p, x in zip(P, w) if len(p["X1c"]) == 10)   # the smallest n that returns non-zero
    # the outliers that were planted are found, and the result is near the planted Sim3
    for p, x in zip(P, w):
        if x["wrote"]:
            dR, dt, ds = planted_error(x, p["planted"])
            assert dR < 2e-2 and dt < 5e-2 and ds < 5e-2


def test_resolution_is_measured_and_written():
    """the restatement against re-associations of itself (another edge order, long double, sums per chunk of 64): identical decisions
    (generator_case raises otherwise) and the differences of R(q12), t12, s12, written to profiles/sim3_opt_resolution.txt"""
    lines = ["# OptimizeSim3: resolution of the generator's problems (tests/sim3_opt_ref.py resolution(): the restatement against itself",
             "# with another edge order, in long double, with sums per chunk of 64); tolerance = max(1e-5, 4 x resolution)",
             "# seed  problem  n  fix_scale  n_bad  n_inliers  resolution  tolerance"]
    worst = 0.0
    for seed in SEEDS:
        c = R.generator_case(seed)
        for k, (P, w, r) in enumerate(zip(c["problems"], c["want"], c["resolution"])):
            lines.append("%d %2d %3d %d %2d %3d %.1e %.1e" % (seed, k, len(P["X1c"]), int(P["fix_scale"]), w["n_bad"], w["n_inliers"], r, R.tolerance(r)))
            worst = max(worst, r)
    print("\n".join(lines))
    assert worst < 1e-4   # a computation that determined its result no better than this would make the rule empty
    with open(os.path.join(ROOT, "profiles", "sim3_opt_resolution.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


@pytest.mark.parametrize("seed", SEEDS)
def test_host_tap_agrees_with_the_reference(pkg, seed):
    c = R.generator_case(seed)
    got = pkg.capi.debug_sim3_opt_host(c["problems"])
    for k, (g, w, P, r) in enumerate(zip(got, c["want"], c["problems"], c["resolution"])):
        ok, msg = R.same(g, w, P, r)
        assert ok, (k, msg)
    one = pkg.capi.debug_sim3_opt_host(c["problems"][5:6])[0]   # a problem alone
    assert R.values(one).tobytes() == R.values(got[5]).tobytes() and R.decisions(one) == R.decisions(got[5])


def test_fix_scale_leaves_s12_bit_identical(pkg):
    c = R.generator_case(SEEDS[0])
    fixed = [dict(P, fix_scale=True, s12=np.float64(1.0371)) for P in c["problems"] if len(P["X1c"]) >= 10]
    for g, P in zip(pkg.capi.debug_sim3_opt_host(fixed), fixed):
        assert np.float64(g["s12"]).tobytes() == np.float64(P["s12"]).tobytes()
    w = R.optimize_sim3(fixed[2])
    assert w["wrote"] and np.float64(w["s12"]).tobytes() == np.float64(1.0371).tobytes()


def test_bad_arguments_are_refused_and_an_empty_batch_succeeds(pkg):
    P = R.generator_case(SEEDS[0])["problems"][4]
    assert pkg.capi.debug_sim3_opt_host([]) == []
    with pytest.raises(pkg.AosError) as e:
        pkg.capi.debug_sim3_opt_host([P] * 65)
    assert e.value.code == pkg.capi.AOS2_ERR_ARG
    for th2 in (0.0, -1.0, float("nan")):
        with pytest.raises(pkg.AosError) as e:
            pkg.capi.debug_sim3_opt_host([P, dict(P, th2=th2)])
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
    # straight through the C ABI: n < 0, missing arrays; nothing is written
    L = pkg.capi.lib()
    Pc, Rc, keep, outs = pkg.capi._sim3_opt_args([P])
    assert L.aos2_debug_sim3_opt_host(Pc, Rc, 1) == 0
    for field, value in (("n", -1), ("X1c", None), ("X2c", None), ("obs1", None), ("obs2", None), ("inv_sigma2_1", None), ("inv_sigma2_2", None)):
        Pc, Rc, keep, outs = pkg.capi._sim3_opt_args([P, P], sentinel=0x5A)
        setattr(Pc[1], field, value)
        assert L.aos2_debug_sim3_opt_host(Pc, Rc, 2) == pkg.capi.AOS2_ERR_ARG, field
        assert all((o == 0x5A).all() for o in outs) and Rc[0].n_inliers == 0x5A and Rc[1].n_bad == 0x5A
    Pc, Rc, keep, outs = pkg.capi._sim3_opt_args([P])
    Rc[0].outlier = None
    assert L.aos2_debug_sim3_opt_host(Pc, Rc, 1) == pkg.capi.AOS2_ERR_ARG
    assert L.aos2_debug_sim3_opt_host(None, None, 1) == pkg.capi.AOS2_ERR_ARG and L.aos2_debug_sim3_opt_host(None, None, 0) == 0
    assert L.aos2_optimize_sim3(None, Pc, Rc, 1) == pkg.capi.AOS2_ERR_ARG
    # n == 0 needs no arrays
    Pc, Rc, keep, outs = pkg.capi._sim3_opt_args([R.generator_case(SEEDS[0])["problems"][0]])
    for field in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2"):
        setattr(Pc[0], field, None)
    Rc[0].outlier = None
    assert L.aos2_debug_sim3_opt_host(Pc, Rc, 1) == 0 and Rc[0].n_inliers == 0 and Rc[0].s12 == Pc[0].s12


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_host_class_compiles_and_links_against_the_refstub(pkg, tmp_path, flags):
    """host/OptimizeSim3.h compiles (-Wall -Werror, both error conventions) against the unchanged stand-ins of tests/cpp/refstub plus
    the Sim3 stand-in and links against libaos2 (the run needs the GPU: tests/test_sim3_opt_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "optimize_sim3_test.cpp"),
                           "-o", str(tmp_path / "optimize_sim3_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
