"""Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:782-1045) without a GPU: the CPU restatement the GPU tests compare against
(tests/essential_graph_ref.py) checked against independent knowledge (log of exp, the closed-form Jacobian of the edge's residual,
planted poses), the library's host tap (aos2_debug_essential_graph_host: the header the device kernels run,
csrc/essential_graph.h, with a skyline solve) checked against it under the comparison rule, the conditions the shared generator
has to meet, and the argument checks."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_graph_ref as R  # noqa: E402
import essential_graph_cases as K  # noqa: E402
from essential_graph_cases import adjoint, inverse_left_jacobian, small_adjoint  # noqa: E402,F401

SEED = 3
DBL_EPSILON = 2.0 ** -52
THETA_LOG = np.sqrt(2 * R.EPS)   # d = cos(theta) > 1 - eps: log's small-rotation branch reaches up to here, exp's to eps


def coefficients(theta, sigma, small_r):
    """A, B, C of sim3.h:89-139 / :168-213 as the lines read, in the branch (|sigma| < eps, small_r)"""
    s = np.exp(sigma)
    if abs(sigma) < R.EPS:
        if small_r:
            return 0.5, 1.0 / 6.0, 1.0
        return (1 - np.cos(theta)) / theta ** 2, (theta - np.sin(theta)) / theta ** 3, 1.0
    C = (s - 1) / sigma
    if small_r:
        return ((sigma - 1) * s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * s) / sigma ** 3, C
    a, b, c = s * np.sin(theta), s * np.cos(theta), theta ** 2 + sigma ** 2
    return (a * sigma + (1 - b) * theta) / (theta * c), (C - ((b - 1) * sigma + a * theta) / c) / theta ** 2, C


def W_of(omega, A, B, C):
    Om = R.S3.skew(omega)
    return A * Om + B * (Om @ Om) + C * np.eye(3)


@pytest.mark.parametrize("theta", [0.0, 0.3 * R.EPS, R.EPS * (1 - 1e-9), R.EPS * (1 + 1e-9), 1e-3, THETA_LOG * 0.999, THETA_LOG * 1.001, 0.02, 0.7, 2.5])
@pytest.mark.parametrize("sigma", [0.0, 0.3 * R.EPS, R.EPS * (1 - 1e-9), R.EPS * (1 + 1e-9), -R.EPS * (1 + 1e-9), 0.02, -0.3])
def test_log_of_exp_gives_the_update_back(theta, sigma):
    """All four (sigma, rotation) branches of log, both eps crossings of sigma and of the rotation -- exp's (theta = eps) and log's
    (d = 1 - eps, theta = sqrt(2 eps)).  What log(exp(u)) may differ from u by, from the lines themselves:
      sigma: log(exp(sigma)): two roundings of a number of size 1, 2 DBL_EPSILON.
      omega: with log's general branch, theta / (2 sqrt(1 - d^2)) deltaR is exact but for the rounding of d near 1: d carries
             DBL_EPSILON of 1, acos(d) and sqrt(1 - d^2) turn that into DBL_EPSILON / theta^2 relative (3e-12 at theta = sqrt(2 eps),
             less above); with the small branch omega = deltaR / 2 = (sin theta / theta) omega: theta^3 / 6 (1.5e-8 at its upper end).
             exp's small branch (theta < eps) builds R = I + Omega + Omega^2, not a rotation by theta^2 / 2 = 5e-11; that passes
             through the unnormalised quaternion into deltaR.  Bound: theta^3 / 6 + 4e-10 theta / eps + 1e-11 in the small branch,
             2e-11 in the general one.
      upsilon: exp forms t = W_exp upsilon with the A, B, C of ITS branch and log solves W_log x = t with those of ITS branch.
             The branches agree in theta only below eps and above sqrt(2 eps); between, and wherever line :116 / :199 is taken
             (B = (sigma^2 / 2 - sigma + 1) s / sigma^3, about 1 / sigma^3 where the limit of the general B is about 1 / 6), the two W
             differ and log(exp(u)) is NOT u: it is W_log^-1 W_exp upsilon.  That is asserted: the expected value is formed from
             the lines' own A, B, C at the omega log recovers, and the result must agree with it within the rounding of the 3x3 solve,
             cond(W) * 64 DBL_EPSILON * |upsilon| + |W_log^-1| * (what the error of omega moves W by)."""
    axis = np.array([0.6, -0.48, 0.64])
    ups = np.array([0.7, -1.1, 0.4])
    v = np.linalg.norm(ups)
    u = np.concatenate([axis * theta, ups, [sigma]])
    S = R.exp1(u)
    got = R.log(S[None])[0]
    assert abs(got[6] - sigma) <= 2 * DBL_EPSILON
    d = 0.5 * (np.trace(R.rot_of(S[None, :4])[0]) - 1)
    small_log = d > 1 - R.EPS
    err_omega = np.abs(got[:3] - u[:3]).max()
    bound_omega = theta ** 3 / 6 + 4e-10 * theta / R.EPS + 1e-11 if small_log else 2e-11
    print("theta %.3g sigma %.3g: log branch small = %s, omega error %.2e (bound %.2e)" % (theta, sigma, small_log, err_omega, bound_omega))
    assert err_omega <= bound_omega
    W_exp = W_of(u[:3], *coefficients(theta, sigma, theta < R.EPS))
    th_log = np.linalg.norm(got[:3])
    W_log = W_of(got[:3], *coefficients(th_log, got[6], small_log))
    expected = np.linalg.solve(W_log, W_exp @ ups)
    inv_norm = np.linalg.norm(np.linalg.inv(W_log), 2)
    A_l, B_l, _ = coefficients(th_log, got[6], small_log)
    bound_ups = np.linalg.cond(W_log) * 64 * DBL_EPSILON * v + inv_norm * (abs(A_l) + 2 * abs(B_l) * max(theta, 1e-300)) * bound_omega * v * 2 + 1e-13
    err_ups = np.abs(got[3:6] - expected).max()
    print("   upsilon: as written differs from u by %.2e; from the expected W_log^-1 W_exp upsilon by %.2e (bound %.2e)" % (
        np.abs(got[3:6] - ups).max(), err_ups, bound_ups))
    assert err_ups <= bound_ups
    if (theta < R.EPS) == bool(small_log):
        # exp and log took the same lines: upsilon itself comes back (W_log differs from W_exp by the error of omega alone, which
        # the second term of the bound covers once more)
        assert np.abs(got[3:6] - ups).max() <= 2 * bound_ups


def test_central_difference_jacobian_agrees_with_the_closed_form():
    """With T = C S_i S_j^-1 and e = log T:  C exp(u) S_i S_j^-1 = exp(Ad_C u) T, so d e / d u_i = Jl^-1(e) Ad_C, and
    C S_i (exp(u) S_j)^-1 = T exp(-u) = exp(-Ad_T u) T, so d e / d u_j = -Jl^-1(e) Ad_T (the series of Jl^-1 converges to
    1e-16 for the |e| <= 0.4 used here).  Bound, per entry: the truncation of a central difference is f''' delta^2 / 6 ~ 1e-18,
    nothing; what is left is the rounding of the two residuals that are subtracted.  A residual is two Sim3 products and a log with a
    3x3 solve: about k = 100 roundings, each DBL_EPSILON / 2 of an intermediate no larger than M = max(1, the largest |t| among C,
    S_i, S_j^-1 and T) times cond(W) <= 2, so |error of e| <= k M DBL_EPSILON, the difference of two twice that, times
    1 / (2 delta):  |J - J_closed| <= k M DBL_EPSILON / delta."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for trial in range(12):
        P = R.problem(40 + trial, 9, trial % 2 == 1)
        est = np.array(P["Scw"])
        est[:, 7] *= 1 + 0.05 * rng.normal(size=len(est)) * (trial % 2 == 0)
        e = int(rng.integers(len(P["v0"])))
        i, j = int(P["v0"][e]), int(P["v1"][e])
        xi = np.concatenate([0.1 * rng.normal(size=3), 0.1 * rng.normal(size=3), [0.05 * rng.normal()]])   # the residual to be had
        T = R.exp1(xi)
        C = R.mul(T[None], R.mul(est[j:j + 1], R.inverse(est[i:i + 1])))[0]
        one = dict(P, v0=np.array([i], np.int32), v1=np.array([j], np.int32), Sji=C[None], fixed=-1, fix_scale=False)
        J = np.zeros((2, 7, 7))
        scalar = 1 / (2 * R.DELTA)
        for d in range(7):
            for side, v in ((0, i), (1, j)):
                ep = []
                for sign in (1, -1):
                    u = np.zeros(7)
                    u[d] = sign * R.DELTA
                    pert = est.copy()
                    pert[v] = R.oplus_all(u, False, est[v:v + 1])[0]
                    ep.append(R.residuals(one["Sji"], pert, one["v0"], one["v1"])[0])
                J[side, :, d] = scalar * (ep[0] - ep[1])
        Tnow = R.mul(R.mul(C[None], est[i:i + 1]), R.inverse(est[j:j + 1]))[0]
        err = R.log(Tnow[None])[0]
        Jl = inverse_left_jacobian(err)
        closed = np.stack([Jl @ adjoint(C), -Jl @ adjoint(Tnow)])
        M = max(1.0, np.abs(C[4:7]).max(), np.abs(est[i, 4:7]).max(), np.abs(R.inverse(est[j:j + 1])[0, 4:7]).max(), np.abs(Tnow[4:7]).max())
        bound = 100 * M * DBL_EPSILON / R.DELTA
        got = np.abs(J - closed).max()
        worst = max(worst, got / bound)
        print("trial", trial, "|e| %.3f" % np.linalg.norm(err), "largest |J| %.2f" % np.abs(closed).max(), "largest difference %.3e" % got, "bound %.3e" % bound)
        assert got <= bound
        H, b, chi = R.linearise(dict(one, fixed=-1, fix_scale=True), est, np.arange(1), np.float64)   # _fix_scale: column 6 is exactly 0
        assert (H[:, 6::7] == 0).all() and (H[6::7, :] == 0).all()
    print("worst difference / bound:", worst)


def planted_error(S, T):
    return (float(np.abs(R.rot_of(S[:, :4]) - R.rot_of(T[:, :4])).max()), float(np.abs(S[:, 4:7] - T[:, 4:7]).max()), float(np.abs(S[:, 7] - T[:, 7]).max()))


@pytest.mark.parametrize("n,fix_scale", [(17, False), (130, False), (130, True)])
def test_noise_free_measurements_give_the_planted_poses_back(pkg, n, fix_scale):
    """measurements taken from the planted poses, the fixed vertex at its planted pose, every other estimate drifted away along the
    chain (a random walk of 0.002 rad, 1 cm and 0.2 % per keyframe): the restatement, and the host tap on the same problem, arrive
    within 1e-6 in R and s and 1e-5 in t in 20 iterations.  (Reached when written: 1e-14 .. 1e-9 in all three.)"""
    P = R.problem(5, n, fix_scale, planted=True)
    for name, res in (("restatement", R.optimize(P)), ("host tap", pkg.capi.debug_essential_graph_host([P])[0])):
        dR, dt, ds = planted_error(np.asarray(res["Scw"]), P["truth"])
        print(name, "n", n, "dR %.2e dt %.2e ds %.2e" % (dR, dt, ds), "chi2 %.3e -> %.3e" % (res["chi2_initial"], res["chi2_final"]),
              "iterations", res["iterations"], "trials", res["trials"])
        assert res["status"] == R.EG_OK and res["chi2_final"] < res["chi2_initial"]
        assert dR <= 1e-6 and ds <= 1e-6 and dt <= 1e-5


def test_generator_meets_its_conditions():
    c = R.generator_case(SEED)
    P, w = c["problems"], c["want"]
    assert tuple(len(p["Scw"]) for p in P) == R.SIZES == (1, 2, 3, 9, 17, 64, 65, 130, 300)
    print("edges", [len(p["v0"]) for p in P], "iterations", [x["iterations"] for x in w], "trials", [x["trials"] for x in w],
          "rejected", [x["rejected"] for x in w], "chi2", ["%.2e -> %.2e" % (x["chi2_initial"], x["chi2_final"]) for x in w])
    assert any(x["rejected"] > 0 for x in w)                                               # a rejected trial
    assert {bool(p["fix_scale"]) for p in P if len(p["v0"]) > 8} == {True, False}
    for p, x in zip(P, w):
        n = len(p["Scw"])
        assert x["status"] == R.EG_OK
        if n >= 2:
            assert x["chi2_final"] < x["chi2_initial"] or n == 2
            pairs = np.stack([p["v0"], p["v1"]], axis=1)
            touching0 = pairs[(pairs == 0).any(axis=1)]
            assert len(touching0) and ((touching0 == p["fixed"]).any(axis=1)).all()        # keyframe 0: its only edges go to the fixed vertex
        if n >= 3:
            und = [tuple(sorted(e)) for e in pairs.tolist()]
            dup = [e for e in pairs.tolist() if und.count(tuple(sorted(e))) > 1]
            assert any([b, a] in dup for a, b in dup)                                      # a pair twice, in both orientations
        if n >= 5:
            assert any(k == 0 and [a, b] in pairs[p["kind"] == 1].tolist() for a, b, k in zip(p["v0"], p["v1"], p["kind"]))   # LoopConnections on a tree edge
        if n >= 9:
            assert (p["kind"] == 2).any() and set(p["kind"].tolist()) == {0, 1, 2, 3}       # an earlier loop edge, all four kinds
            drift = np.abs(R.values(dict(Scw=p["Scw"])) - R.values(dict(Scw=p["truth"]))).max()
            assert drift > 1e-3                                                             # the estimates are away from the truth
    assert w[0]["iterations"] == 0 and w[0]["Scw"].tobytes() == P[0]["Scw"].tobytes()


def test_resolution_is_measured_and_written():
    """the restatement against re-associations of itself (another edge order, another elimination order, long double sums): the same
    status (generator_case raises otherwise) and the differences of R(q), t, s, written to profiles/essential_graph_resolution.txt"""
    c = R.generator_case(SEED)
    lines = ["# OptimizeEssentialGraph: resolution of the generator's problems (tests/essential_graph_ref.py resolution(): the restatement",
             "# against itself with another edge order, another elimination order, sums in long double); tolerance = max(1e-5, 4 x resolution)",
             "# seed  n_vertices  n_edges  fix_scale  iterations  trials  rejected  resolution  tolerance"]
    for P, w, r in zip(c["problems"], c["want"], c["resolution"]):
        lines.append("%d %3d %4d %d %2d %2d %2d %.1e %.1e" % (SEED, len(P["Scw"]), len(P["v0"]), int(P["fix_scale"]), w["iterations"], w["trials"],
                                                            w["rejected"], r, R.tolerance(r)))
    print("\n".join(lines))
    assert max(c["resolution"]) < 1e-4   # a computation that determined its result no better than this would make the rule empty
    with open(os.path.join(ROOT, "profiles", "essential_graph_resolution.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_host_tap_agrees_with_the_reference(pkg):
    c = R.generator_case(SEED)
    got = pkg.capi.debug_essential_graph_host(c["problems"])
    for k, (g, w, P, r) in enumerate(zip(got, c["want"], c["problems"], c["resolution"])):
        ok, msg = R.same(g, w, P, r)
        print(len(P["Scw"]), msg, "iterations", g["iterations"], w["iterations"], "trials", g["trials"], w["trials"], "l_blocks", g["l_blocks"])
        assert ok, (k, msg)
    for k in (3, 7):   # a problem alone: the same bytes as in the batch
        one = pkg.capi.debug_essential_graph_host(c["problems"][k:k + 1])[0]
        assert all(np.asarray(one[f]).tobytes() == np.asarray(got[k][f]).tobytes() for f in ("Scw", "Tiw", "Xw"))
        assert (one["status"], one["iterations"], one["trials"], one["chi2_final"]) == (got[k]["status"], got[k]["iterations"], got[k]["trials"], got[k]["chi2_final"])


def test_degenerate_graphs_come_back_through_the_recovery_arithmetic(pkg):
    c = R.generator_case(SEED)
    P = dict(c["problems"][4])
    none = dict(P, v0=P["v0"][:0], v1=P["v1"][:0], Sji=P["Sji"][:0])
    for Q in (none, c["problems"][0]):
        g, w = pkg.capi.debug_essential_graph_host([Q])[0], R.optimize(Q)
        assert g["Scw"].tobytes() == np.asarray(Q["Scw"], np.float64).tobytes() and (g["iterations"], g["trials"], g["status"], g["l_blocks"]) == (0, 0, 0, 0)
        assert np.abs(g["Tiw"] - w["Tiw"]).max() <= 1e-6 and np.abs(g["Xw"] - w["Xw"]).max() <= 1e-5
        assert np.abs(g["Xw"] - np.asarray(Q["Xw"])).max() <= 4 * np.spacing(np.float32(np.abs(Q["Xw"]).max()))   # Swr Srw = identity


def test_bad_arguments_are_refused_and_an_empty_batch_succeeds(pkg):
    """straight through the C ABI with sentinel-filled outputs: AOS2_ERR_ARG and not a byte written"""
    capi = pkg.capi
    L = capi.lib()
    P = R.generator_case(SEED)["problems"][3]
    assert capi.debug_essential_graph_host([]) == []
    with pytest.raises(pkg.AosError) as e:
        capi.debug_essential_graph_host([P] * 17)
    assert e.value.code == capi.AOS2_ERR_ARG
    with pytest.raises(pkg.AosError) as e:
        capi.debug_essential_graph_host([R.problem(1, 513, False, n_points=0)])
    assert e.value.code == capi.AOS2_ERR_CAPACITY
    bad_v0, bad_v1, loop_edge, bad_ref = (np.array(P[k]) for k in ("v0", "v1", "v0", "ref"))
    bad_v0[2], bad_v1[1], bad_ref[0] = len(P["Scw"]), -1, len(P["Scw"])
    loop_edge[3] = P["v1"][3]
    cases = [dict(n_vertices=-1), dict(n_vertices=0), dict(n_edges=-1), dict(n_points=-1), dict(iterations=0), dict(fixed=-1), dict(fixed=len(P["Scw"])),
             dict(Scw=None, n_vertices=9), dict(v0=None, n_edges=len(P["v0"])), dict(v1=None, n_edges=len(P["v0"])), dict(Sji=None, n_edges=len(P["v0"])),
             dict(Xw=None, n_points=len(P["ref"])), dict(ref=None, n_points=len(P["ref"])), dict(v0=bad_v0), dict(v1=bad_v1), dict(v0=loop_edge), dict(ref=bad_ref),
             dict(null_result="Scw"), dict(null_result="Tiw"), dict(null_result="Xw")]
    for case in cases:
        Pc, Rc, keep, outs = capi._essential_graph_args([P, dict(P, **case)], sentinel=0x5A)
        assert L.aos2_debug_essential_graph_host(Pc, Rc, 2) == capi.AOS2_ERR_ARG, case
        for o in outs:
            assert all((a.view(np.uint8) == 0x5A).all() for a in o.values()), case
        assert all(Rc[k].status == 0x5A5A5A5A and Rc[k].trials == 0x5A5A5A5A and Rc[k].l_blocks == 0x5A5A5A5A for k in (0, 1)), case
        assert L.aos2_optimize_essential_graph(None, Pc, Rc, 2) == capi.AOS2_ERR_ARG
    Pc, Rc, keep, outs = capi._essential_graph_args([P], sentinel=0x5A)
    assert L.aos2_debug_essential_graph_host(None, None, 1) == capi.AOS2_ERR_ARG and L.aos2_debug_essential_graph_host(None, None, 0) == 0
    assert L.aos2_debug_essential_graph_host(Pc, Rc, -1) == capi.AOS2_ERR_ARG
    assert all((a.view(np.uint8) == 0x5A).all() for a in outs[0].values())
    assert L.aos2_debug_essential_graph_host(Pc, Rc, 1) == 0 and Rc[0].status == 0


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_host_class_compiles_and_links_against_its_refstub(pkg, tmp_path, flags):
    """host/OptimizeEssentialGraph.h compiles (-Wall -Werror, both error conventions) behind host/Optimizer.h against the stand-ins of
    tests/cpp/refstub/essential_graph_stub.h and links against libaos2 (the run needs the GPU: tests/test_essential_graph_class_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "essential_graph_test.cpp"),
                           "-o", str(tmp_path / "essential_graph_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])


# ---------------------------------------------------------------------------------------------- the C header itself (csrc/essential_graph.h)
def test_header_log_agrees_with_the_restatement_on_every_branch_and_crossing(pkg):
    """eg_log of the header on exp(u) over the grid of the log-of-exp test (all four branches, exp's and log's crossings of both
    eps) against R.log.  Both are float64 evaluations of the same lines, so they take the same branch (asserted through sigma and the
    size of the difference) and differ by rounding alone: sigma 2 DBL_EPSILON; omega 16 DBL_EPSILON (theta + 1 / theta) in the
    general branch (d = cos(theta) carries DBL_EPSILON, acos turns it into DBL_EPSILON / theta), 16 DBL_EPSILON theta + 1e-18 in the
    small one; upsilon the rounding of the 3x3 solve, cond(W) 64 DBL_EPSILON |t|, plus |W^-1| times what that omega moves W by."""
    axis, ups = np.array([0.6, -0.48, 0.64]), np.array([0.7, -1.1, 0.4])
    thetas = [0.0, 0.3 * R.EPS, R.EPS * (1 - 1e-9), R.EPS * (1 + 1e-9), 1e-3, THETA_LOG * 0.999, THETA_LOG * 1.001, 0.02, 0.7, 2.5]
    sigmas = [0.0, 0.3 * R.EPS, R.EPS * (1 - 1e-9), R.EPS * (1 + 1e-9), -R.EPS * (1 + 1e-9), 0.02, -0.3]
    S = np.stack([R.exp1(np.concatenate([axis * th, ups, [sg]])) for th in thetas for sg in sigmas])
    want, got = R.log(S), pkg.capi.debug_essential_graph_arith_host("log", S)
    worst = 0.0
    for k, (th, sg) in enumerate((th, sg) for th in thetas for sg in sigmas):
        d = 0.5 * (np.trace(R.rot_of(S[k:k + 1, :4])[0]) - 1)
        small = d > 1 - R.EPS
        b_omega = 16 * DBL_EPSILON * th + 1e-18 if small else 16 * DBL_EPSILON * (th + 1 / th)
        A_l, B_l, C_l = coefficients(np.linalg.norm(want[k, :3]), want[k, 6], small)
        W = W_of(want[k, :3], A_l, B_l, C_l)
        t = np.linalg.norm(S[k, 4:7])
        b_ups = np.linalg.cond(W) * 64 * DBL_EPSILON * t + np.linalg.norm(np.linalg.inv(W), 2) * (abs(A_l) + 2 * abs(B_l) * th) * b_omega * t * 2 + 1e-15
        e_omega, e_ups = np.abs(got[k, :3] - want[k, :3]).max(), np.abs(got[k, 3:6] - want[k, 3:6]).max()
        worst = max(worst, e_omega / b_omega if b_omega else 0.0, e_ups / b_ups)
        assert abs(got[k, 6] - want[k, 6]) <= 2 * DBL_EPSILON and e_omega <= b_omega and e_ups <= b_ups, (th, sg, e_omega, b_omega, e_ups, b_ups)
    print("worst difference / bound:", worst)


def _lu3(A, t, last_on_ties=False):
    """PartialPivLU of a 3x3 and its solve in float64 scalars: the pivot of column k is the largest magnitude in rows k..2, the
    first one on ties"""
    a, b = [[np.float64(v) for v in row] for row in A], [np.float64(v) for v in t]
    for k in range(3):
        p = k
        for i in range(k + 1, 3):
            if abs(a[i][k]) > abs(a[p][k]) or (last_on_ties and abs(a[i][k]) == abs(a[p][k])):
                p = i
        a[k], a[p], b[k], b[p] = a[p], a[k], b[p], b[k]
        for i in range(k + 1, 3):
            a[i][k] = a[i][k] / a[k][k]
            for j in range(k + 1, 3):
                a[i][j] = a[i][j] - a[i][k] * a[k][j]
    b[1] = b[1] - a[1][0] * b[0]
    b[2] = b[2] - a[2][0] * b[0]
    b[2] = b[2] - a[2][1] * b[1]
    x2 = b[2] / a[2][2]
    x1 = (b[1] - a[1][2] * x2) / a[1][1]
    x0 = (b[0] - a[0][1] * x1 - a[0][2] * x2) / a[0][0]
    return np.array([x0, x1, x2])


def test_header_lu_pivots_on_the_largest_magnitude_and_takes_the_first_on_ties(pkg):
    """bit for bit against the scalar model above, on matrices that need each row swap, on ties in the first and in the second column
    (where the model that takes the LAST of equal magnitudes gives other bits: the test can tell the two apart), and on random ones
    against numpy's LU within cond(W) 64 DBL_EPSILON |x|"""
    rng = np.random.default_rng(5)
    cases = [([[0.1, 0.7, 0.3], [0.9, 0.2, 0.5], [0.4, 0.6, 0.8]], [0.3, 0.7, 1.1]),          # swap in the first column
             ([[0.9, 0.2, 0.5], [0.3, 0.1, 0.7], [0.6, 0.8, 0.3]], [1.3, 0.7, 0.1]),          # swap in the second
             ([[0.7, 0.3, 0.1], [-0.7, 0.9, 0.3], [0.7, 0.1, 1.3]], [0.3, 1.7, 1.1]),         # a three-way tie in the first column
             ([[0.9, 0.3, 0.1], [0.0, 0.7, 0.3], [0.0, -0.7, 1.3]], [0.3, 1.7, 1.1])]         # a tie in the second
    cases += [(rng.normal(size=(3, 3)).tolist(), rng.normal(size=3).tolist()) for _ in range(40)]
    packed = np.array([np.concatenate([np.ravel(A), t]) for A, t in cases])
    got = pkg.capi.debug_essential_graph_arith_host("lu3", packed)
    told_apart = 0
    for k, (A, t) in enumerate(cases):
        want = _lu3(A, t)
        assert got[k].tobytes() == want.tobytes(), (k, got[k], want)
        told_apart += _lu3(A, t, last_on_ties=True).tobytes() != want.tobytes()
        ref = np.linalg.solve(np.array(A), np.array(t))
        assert np.abs(got[k] - ref).max() <= np.linalg.cond(np.array(A)) * 64 * DBL_EPSILON * max(1.0, np.abs(ref).max())
    assert told_apart >= 1


def test_header_residual_agrees_with_the_restatement(pkg):
    """eg_residual = log(C * S_v0 * S_v1^-1) of the header on the generator's edges and estimates, against the restatement: the two
    products and the inverse are the same scalar operations in both (differences of a few DBL_EPSILON M, M = the largest |t|), then
    the log as above: 64 DBL_EPSILON M cond(W) with cond(W) <= 2 for these residuals (|e| < 0.5)."""
    worst = 0.0
    for P in R.generator_case(SEED)["problems"][3:7]:
        est, v0, v1 = np.asarray(P["Scw"]), P["v0"], P["v1"]
        want = R.residuals(P["Sji"], est, v0, v1)
        got = pkg.capi.debug_essential_graph_arith_host("residual", np.concatenate([P["Sji"], est[v0], est[v1]], axis=1))
        M = max(1.0, np.abs(P["Sji"][:, 4:7]).max(), np.abs(est[:, 4:7]).max(), np.abs(R.inverse(est)[:, 4:7]).max())
        bound = 64 * DBL_EPSILON * M * 2
        err = np.abs(got - want).max()
        worst = max(worst, err / bound)
        print(len(est), "largest |e| %.3f" % np.abs(want).max(), "largest difference %.2e" % err, "bound %.2e" % bound)
        assert np.abs(want).max() < 0.5 and err <= bound
    print("worst difference / bound:", worst)


# ---------------------------------------------------------------------------------------------- the turned inputs and the replay
def _restated(P):
    est = np.asarray(P["Scw"], np.float64)
    e, J0, J1 = R.jacobians(P, est, np.arange(len(P["v0"])))
    return est, np.stack([J0, J1], axis=1), e


@pytest.mark.parametrize("name", list(K.cases()))
def test_replay_agrees_with_the_restatement_and_notices_a_wrong_block_on_turned_inputs(name):
    """K.replay on the restatement's own J and e against R.linearise (numpy's sums): the same products in another order, so an entry
    of n products differs by at most 4 n 2^-53 sum |products| (nothing where no edge adds).  Then the two ways of getting the block
    below the diagonal wrong: with the two forms exchanged, and with J1^T J0 formed as J0^T J1, the replay gives another H."""
    P = K.cases()[name]
    est, J, e = _restated(P)
    H, b, nH, aH, nb, ab = K.replay(P, J, e, stats=True)
    Hr, br, _ = R.linearise(P, est, np.arange(len(P["v0"])), np.float64)
    keep = np.flatnonzero(np.repeat(np.arange(len(est)) != P["fixed"], 7))
    dH, db = np.abs(H - Hr[np.ix_(keep, keep)]), np.abs(b - br[keep])
    bH, bb = 4 * nH * 2.0 ** -53 * aH, 4 * nb * 2.0 ** -53 * ab
    print(name, "edges", len(P["v0"]), "free pairs (J0^T J1, J1^T J0)", K.free_pairs(P),
          "largest |H - ref| / bound %.3g, |b - ref| / bound %.3g" % (K.worst(dH, bH), K.worst(db, bb)))
    assert (dH <= bH).all() and (db <= bb).all()
    assert (nH > 0).tobytes() == K.pattern(P).tobytes() and np.array_equal(H, H.T)
    if name == "n2_single_edge":
        assert K.free_pairs(P) == (0, 0)
        return
    assert min(K.free_pairs(P)) >= 1
    for mutant in ("exchanged", "kind3"):
        assert K.replay(P, J, e, mutant=mutant)[0].tobytes() != H.tobytes(), mutant


def test_generator_never_forms_the_block_of_a_lower_first_vertex():
    """the hole the turned inputs close: on every problem of the generator no edge between free vertices has vertex 0 at the lower
    hessian index, so a replay that forms J1^T J0 wrongly is IDENTICAL to the right one there"""
    total = 0
    for P in R.generator_case(SEED)["problems"]:
        if not len(P["v0"]):
            continue
        est, J, e = _restated(P)
        assert K.free_pairs(P)[1] == 0
        total += K.free_pairs(P)[0]
        H, b = K.replay(P, J, e)
        Hm, bm = K.replay(P, J, e, mutant="kind3")
        assert H.tobytes() == Hm.tobytes() and b.tobytes() == bm.tobytes()
        assert P["fixed"] == min(1, len(est) - 1)   # ... and the fixed vertex is always this one
    assert total > 1000
    assert sum(K.free_pairs(P)[1] for P in K.cases().values()) > 500


@pytest.mark.parametrize("name", list(K.cases()))
def test_central_differences_of_turned_edges_agree_with_the_closed_form(name):
    """the bound of test_central_difference_jacobian_agrees_with_the_closed_form, 100 M DBL_EPSILON / delta, on every edge of the
    turned inputs, both sides; with fix_scale column 6 is exactly 0 and the other six are compared"""
    P = K.cases()[name]
    est, J, e = _restated(P)
    closed, bound, emax = K.closed_form(P, est)
    assert emax < 0.5
    cols = 6 if P["fix_scale"] else 7
    ratio = (np.abs(J - closed)[..., :cols].max(axis=(1, 2, 3)) / bound).max()
    print(name, "largest |e| %.3f" % emax, "largest |J - closed| / bound %.3g" % ratio)
    assert ratio <= 1
    if P["fix_scale"]:
        assert (J[..., 6] == 0).all()


def test_host_tap_agrees_with_the_reference_on_turned_inputs(pkg):
    c = K.optimised()
    assert max(c["resolution"]) < 1e-4
    got = pkg.capi.debug_essential_graph_host(c["problems"])
    for k, (g, w, P, r) in enumerate(zip(got, c["want"], c["problems"], c["resolution"])):
        ok, msg = R.same(g, w, P, r)
        print(c["names"][k], "resolution %.1e" % r, msg, "iterations", g["iterations"], w["iterations"], "trials", g["trials"], w["trials"])
        assert ok, (k, msg)
        assert w["status"] == R.EG_OK and w["chi2_final"] < w["chi2_initial"]


def test_a_measurement_that_is_not_a_number_leaves_the_estimates_as_they_were(pkg):
    """a NaN in one Sji: chi2 is NaN, every solve fails (x keeps its zeros, tempChi = DBL_MAX), rho is NaN -- neither > 0 nor < 0 --
    so every iteration is one rejected trial and nothing ends the call before its 20 iterations"""
    P = K.with_nan(K.cases()["n17_fix0_fixed16"])
    with np.errstate(all="ignore"):
        want = R.optimize(P)
    got = pkg.capi.debug_essential_graph_host([P])[0]
    for name, res in (("restatement", want), ("host tap", got)):
        assert (res["status"], res["iterations"], res["trials"], res["rejected"]) == (R.EG_NO_STEP, 20, 20, 20), name
        assert np.asarray(res["Scw"]).tobytes() == np.asarray(P["Scw"], np.float64).tobytes(), name
