"""Optimizer::BundleAdjustment (src/Optimizer.cc:41-237) without a GPU: the numpy restatement the GPU tests compare against
(tests/global_ba_ref.py) pinned to the oracle on the form the oracle can express (robust, LocalBA's Huber deltas) under the project's
comparison rule, its Jacobians checked against central differences, the library's host tap (aos2_debug_global_ba_host: the header and
the per-item functions the kernels run, with a skyline solve) checked against it in all four modes, the conditions the shared
generator has to meet, the argument checks, and the host class compiled against its stand-ins."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import global_ba_ref as R  # noqa: E402

CASES = list(R.CASES)
# nominal free keyframes / candidate points of the cases (the generator keeps the points that two keyframes see)
SIZES = {"init": (1, 24), "pair": (2, 36), "mixed": (11, 300), "band": (44, 1200), "loop": (44, 1200), "past_lba": (159, 1500)}
MODES = [(True, R.HUBER_LOCAL_BA), (True, R.HUBER_GBA), (False, R.HUBER_LOCAL_BA), (False, R.HUBER_GBA)]
_cache = {}


def case(oracle, name):
    """problem, iterations, the oracle's result and the oracle's own spread (parity.lba_resolution), once per session"""
    if name not in _cache:
        import parity
        prob, n = R.problem(name), R.iterations_of(name)
        want = oracle.lba_solve(prob, iters1=n, iters2=0)
        _cache[name] = dict(prob=prob, n=n, want=R.from_oracle(want), resolution=parity.lba_resolution(prob, want=want, iters=(n, 0)))
    return _cache[name]


@pytest.mark.parametrize("name", CASES)
def test_reference_agrees_with_the_oracle_on_the_robust_form(oracle, name):
    c = case(oracle, name)
    got = R.solve(c["prob"], c["n"], True, R.HUBER_LOCAL_BA)
    assert not R.mismatches(got, c["want"], c["resolution"], name)
    # terminate() is counted without the oracle's entry check and its check after optimize()
    assert got["polls"] == c["want"]["polls"] - 2 and got["stop_poll"] == 0


def test_reference_jacobians_agree_with_central_differences():
    """d e / d point and d e / d pose (oplus: exp(u) * T) of both edge types.  The stereo projection rounds 1 / z to float, so its
    error is a step function of the estimates at the scale 2^-24 |e|: the differences are taken of the same lines with a double invz
    (the mono lines for u, v; u - bf / z for the third row), which is what linearizeOplus differentiates.  Central differences at
    h = 1e-6: truncation ~ h^2 |f'''| and rounding ~ 1e-16 |f| / h, both below 1e-6 of the largest entry here."""
    prob = R.problem("mixed")
    G = R.Graph(prob, False, R.HUBER_GBA)
    cam = G.cam
    A, B = R.edge_jacobians(cam, G.qt[G.ep], G.X[G.el], G.stereo)

    def smooth_error(qt, X):
        p = R.se3_map(qt, X)
        u, v = p[:, 0] / p[:, 2] * cam.fx + cam.cx, p[:, 1] / p[:, 2] * cam.fy + cam.cy
        return np.stack([G.obs[:, 0] - u, G.obs[:, 1] - v, np.where(G.stereo, G.obs[:, 2] - (u - cam.bf / p[:, 2]), 0.0)], 1)

    h = 1e-6
    qt, X = G.qt[G.ep], G.X[G.el]
    scale = max(np.abs(A).max(), np.abs(B).max())
    for d in range(3):
        dX = np.zeros(3)
        dX[d] = h
        num = (smooth_error(qt, X + dX) - smooth_error(qt, X - dX)) / (2 * h)
        assert np.abs(num - A[:, :, d]).max() <= 1e-6 * scale
    for d in range(6):
        u = np.zeros(6)
        u[d] = h
        plus = np.stack([R.se3_mul(R.se3_exp(u), q) for q in G.qt])[G.ep]
        minus = np.stack([R.se3_mul(R.se3_exp(-u), q) for q in G.qt])[G.ep]
        num = (smooth_error(plus, X) - smooth_error(minus, X)) / (2 * h)
        assert np.abs(num - B[:, :, d]).max() <= 1e-6 * scale


@pytest.mark.parametrize("robust,huber", MODES)
@pytest.mark.parametrize("name", ["init", "pair", "mixed", "loop"])
def test_host_tap_agrees_with_the_reference_in_all_four_modes(pkg, name, robust, huber):
    prob, n = R.problem(name), R.iterations_of(name)
    res, want = R.resolution_by_reference(prob, n, robust, huber)
    assert res["decisions_equal"]
    got = pkg.capi.debug_global_ba_host(prob, n, robust, huber)
    assert not R.mismatches(got, want, res, "%s robust %d delta %.4f" % (name, robust, huber[0]))
    assert (got["polls"], got["stop_poll"], got["h_blocks"]) == (want["polls"], 0, want["h_blocks"])
    assert got["point_included"].tolist() == want["point_included"].tolist()


def test_host_tap_agrees_with_the_oracle_past_local_ba(pkg, oracle):
    c = case(oracle, "past_lba")
    got = pkg.capi.debug_global_ba_host(c["prob"], c["n"], True, R.HUBER_LOCAL_BA)
    assert not R.mismatches(got, c["want"], c["resolution"], "past_lba")


def test_generator_meets_its_conditions_and_the_resolutions_are_written(pkg, oracle):
    """conditions on the generator, not tolerances: the sizes, one point without an edge and one seen by keyframe 0 alone in every
    case, fill on the loop case, and on every case equal decisions and a spread <= 1e-4 of the oracle against its re-associations
    (the robust form) and of the restatement against itself under reversed edge order (LoopClosing's form: not robust, delta 5.99)"""
    lines = ["# GlobalBundleAdjustment: resolution of the generator's problems; tolerance = max(1e-5, 4 x resolution)",
             "# robust: oracle/parity.py lba_resolution(iters=(n, 0)); plain: tests/global_ba_ref.py against itself under reversed edge order",
             "# case free_keyframes points edges iterations | robust: pose point decisions_equal | plain: pose point decisions_equal"]
    for name in CASES:
        c = case(oracle, name)
        prob = c["prob"]
        assert R.free_keyframes(prob) == SIZES[name][0] and R.CASES[name][:2] == (SIZES[name][0] + 1, SIZES[name][1])
        deg = np.bincount(prob["edge_point"], minlength=prob["n_points"])
        assert (deg == 0).sum() >= 1
        kf0 = int(np.flatnonzero(np.asarray(prob["pose_id"]) == 0)[0])
        only0 = [j for j in np.flatnonzero(deg > 0) if set(prob["edge_pose"][prob["edge_point"] == j]) == {kf0}]
        assert len(only0) >= 1 and prob["pose_fixed"].sum() == 1
        plain, _ = R.resolution_by_reference(prob, c["n"], False, R.HUBER_GBA)
        for res in (c["resolution"], plain):
            assert res["decisions_equal"] and max(res["pose"], res["point"]) <= R.MAX_RESOLUTION, (name, res)
        lines.append("%s %d %d %d %d | %.3g %.3g %s | %s" % (name, R.free_keyframes(prob), prob["n_points"], prob["n_edges"], c["n"], c["resolution"]["pose"],
                                                          c["resolution"]["point"], c["resolution"]["decisions_equal"],
                                                          "%.3g %.3g %s" % (plain["pose"], plain["point"], plain["decisions_equal"])))
    loop = pkg.capi.debug_global_ba_host(R.problem("loop"), 1, False, R.HUBER_GBA)
    band = pkg.capi.debug_global_ba_host(R.problem("band"), 1, False, R.HUBER_GBA)
    assert loop["l_blocks"] > loop["h_blocks"] > band["h_blocks"]
    lines.append("# blocks below the diagonal, reduced system / factor: band %d / %d, loop %d / %d" % (band["h_blocks"], band["l_blocks"], loop["h_blocks"], loop["l_blocks"]))
    with open(os.path.join(ROOT, "profiles", "global_ba_resolution.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")


def test_stop_at_every_poll_agrees_with_the_reference(pkg):
    """the host tap stopped at poll k against the restatement stopped at poll k: the same polls, iterations, trials and estimates"""
    prob, n = R.problem("pair"), R.iterations_of("pair")
    free = pkg.capi.debug_global_ba_host(prob, n, True, R.HUBER_LOCAL_BA)
    assert free["stop_poll"] == 0
    for k in range(1, free["polls"] + 1):
        got = pkg.capi.debug_global_ba_host(prob, n, True, R.HUBER_LOCAL_BA, stop_at_poll=k)
        want = R.solve(prob, n, True, R.HUBER_LOCAL_BA, stop_at_poll=k)
        assert (got["stop_poll"], got["polls"], got["iterations"], got["trials"]) == (k, want["polls"], want["iterations"], want["trials"]), k
        assert R.worst(got["pose_Tcw"], want["pose_Tcw"]) <= R.TOL and R.worst(got["point_xyz"], want["point_xyz"]) <= R.TOL
    first = pkg.capi.debug_global_ba_host(prob, n, True, R.HUBER_LOCAL_BA, stop_at_poll=1)
    assert first["iterations"] == 0 and first["trials"] == 0   # the head of optimize()'s loop: nothing ran


def test_degenerate_maps(pkg):
    prob = R.problem("pair")
    none = dict(prob, n_edges=0, **{k: prob[k][:0] for k in ("edge_pose", "edge_point", "edge_obs", "edge_stereo", "edge_inv_sigma2")})
    got = pkg.capi.debug_global_ba_host(none, 10, False)
    assert got["iterations"] == 0 and got["trials"] == 0 and not got["point_included"].any()
    assert got["point_xyz"].tobytes() == np.ascontiguousarray(prob["point_xyz"], np.float32).tobytes()
    assert np.abs(got["pose_Tcw"] - prob["pose_Tcw"]).max() <= 1e-6   # through toSE3Quat and back
    # every keyframe fixed: the landmarks are still optimised
    fixed = dict(prob, pose_fixed=np.ones_like(prob["pose_fixed"]))
    got, want = pkg.capi.debug_global_ba_host(fixed, 10, False), R.solve(fixed, 10, False)
    assert got["iterations"] == want["iterations"] > 0 and got["trials"] == want["trials"] and got["h_blocks"] == got["l_blocks"] == 0
    assert R.worst(got["point_xyz"], want["point_xyz"]) <= R.TOL and np.abs(got["point_xyz"] - prob["point_xyz"]).max() > 1e-4


def test_bad_arguments_are_refused_with_no_result_byte_written(pkg):
    capi = pkg.capi
    prob = R.problem("pair")
    bad_edge = prob["edge_pose"].copy()
    bad_edge[3] = prob["n_poses"]
    bad_point = prob["edge_point"].copy()
    bad_point[0] = -1
    cases = [dict(it=0), dict(it=-3), dict(huber=(0.0, 1.0)), dict(prob=dict(prob, edge_pose=bad_edge)), dict(prob=dict(prob, edge_point=bad_point)),
             dict(prob=dict(prob, pose_Tcw=None)), dict(prob=dict(prob, point_id=None)), dict(prob=dict(prob, edge_obs=None)), dict(prob=dict(prob, n_points=-1))]
    for c in cases:
        with pytest.raises(capi.AosError) as e:
            capi.debug_global_ba_host(c.get("prob", prob), c.get("it", 10), False, c.get("huber", R.HUBER_GBA), sentinel=0x5A)
        assert e.value.code == capi.AOS2_ERR_ARG, c
        r, (Tout, Pout, inc) = capi.debug_global_ba_host.last
        assert (Tout == 0x5A).all() and (Pout == 0x5A).all() and (inc == 77).all(), c
        assert r.iterations == r.trials == r.status == capi._GBA_SENTINEL_INT, c
    L = capi.lib()
    assert L.aos2_debug_global_ba_host(None, None, None, 0) == capi.AOS2_ERR_ARG


@pytest.mark.parametrize("flags", [[], ["-DAOS2_HOST_EXCEPTIONS"]])
def test_host_class_compiles_and_links_against_its_refstub(pkg, tmp_path, flags):
    """host/GlobalBundleAdjustment.h compiles (-Wall -Werror, both error conventions) behind host/Optimizer.h against the stand-ins of
    tests/cpp/refstub/global_ba_stub.h and links against libaos2 (the run needs the GPU: tests/test_global_ba_class_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "global_ba_test.cpp"),
                           "-o", str(tmp_path / "global_ba_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
