"""The RANSAC of Sim3Solver (src/Sim3Solver.cc) without a GPU: the CPU restatement the GPU tests compare against (tests/sim3_ref.py)
checked against independent knowledge (planted transformations, numpy's eigensolver, a literal replay of the index removal), the
library's host tap (aos2_debug_sim3_host: the routine the device kernels run, csrc/sim3.h) checked against it bit for bit, the
conditions the shared generator's seeds have to meet, the argument checks, and the host shim's compile + link."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_ref as R  # noqa: E402

SEEDS = (3, 4, 5)
EPS = R.FLT_EPSILON


def noise_free_triples(seed, count):
    """three points in the generator's box and their images under a planted Sim3, rounded to float32"""
    rng = np.random.default_rng(seed)
    for k in range(count):
        P = R.problem(rng, 3, 0.0, 1.0 if k % 2 == 0 else 1.3, noise=0.0)
        yield P


def gap_of(N):
    """g = (lambda1 - lambda2) / |lambda1| of the 4x4 N, and numpy's eigen-decomposition of it (ascending)"""
    w, v = np.linalg.eigh(np.array(N, np.float64))
    return (w[3] - w[2]) / abs(w[3]), w, v


def test_noise_free_triples_give_the_planted_sim3_back():
    """bound on R12: 16 FLT_EPSILON / g, for the triples with g >= 1e-2 (a double eigensolver on the float-rounded inputs shows
    2.1 FLT_EPSILON / g: the rounding of the inputs alone)"""
    worst, qualify = 0.0, 0
    for P in noise_free_triples(11, 200):
        m = R.horn(P["X3Dc1"], P["X3Dc2"], P["fix_scale"])
        g, _, _ = gap_of(m["N"])
        if g < 1e-2:
            continue
        qualify += 1
        err = np.abs(np.array(m["R"]).reshape(3, 3) - P["planted"]["R"]).max()
        worst = max(worst, err * g / EPS)
        assert err <= 16 * EPS / g, (err, g, err * g / EPS)
        assert abs(m["s"] - P["planted"]["s"]) <= 1e-4 and np.abs(np.array(m["t"]) - P["planted"]["t"]).max() <= 1e-4
    print("triples with g >= 1e-2:", qualify, "of 200; worst |R12 - R| * g / FLT_EPSILON of the float Jacobi:", worst)
    assert qualify >= 150


def test_jacobi_agrees_with_numpy_eigh():
    worst_vec = worst_val = 0.0
    mats = [R.horn(P["X3Dc1"], P["X3Dc2"], True)["N"] for P in noise_free_triples(12, 100)]
    rng = np.random.default_rng(13)
    for _ in range(100):   # and symmetric matrices that come from no rotation
        A = rng.normal(size=(4, 4))
        mats.append((A + A.T).astype(np.float32).tolist())
    for N in mats:
        W, V, rotations = R.jacobi_eigen(N)
        assert rotations < 4 * 4 * 30
        g, w, v = gap_of(N)
        norm = max(abs(w[0]), abs(w[3]))
        assert all(W[i] >= W[i + 1] for i in range(3))
        for i in range(4):
            worst_val = max(worst_val, abs(W[i] - w[3 - i]) / (EPS * norm))
            assert abs(W[i] - w[3 - i]) <= 8 * EPS * norm, (i, W, w)
        if g >= 1e-2:
            q, want = np.array(V[0]), v[:, 3]
            err = min(np.abs(q - want).max(), np.abs(q + want).max())
            worst_vec = max(worst_vec, err * g / EPS)
            assert err <= 16 * EPS / g, (err, g)
    print("worst eigenvalue difference / (FLT_EPSILON |N|):", worst_val, "worst eigenvector difference * g / FLT_EPSILON:", worst_vec)


def test_eigenvector_sign_does_not_matter_for_the_rotation():
    """q and -q give the same R12 through atan2 / the scale of vec / Rodrigues up to rounding"""
    q = np.array([0.9, 0.3, -0.2, 0.1])
    q /= np.linalg.norm(q)
    Rs = []
    for sgn in (1.0, -1.0):
        v = sgn * q
        nrm = math.sqrt(v[1] ** 2 + v[2] ** 2 + v[3] ** 2)
        f = 2 * math.atan2(nrm, v[0]) / nrm
        Rs.append(np.array(R.rodrigues([R.f32(v[1] * f), R.f32(v[2] * f), R.f32(v[3] * f)])))
    assert np.abs(Rs[0] - Rs[1]).max() <= 8 * EPS


def test_closed_form_of_the_index_removal_equals_the_literal_one():
    rng = np.random.default_rng(14)
    for n in (3, 4, 5, 7, 64):
        seen = set()
        for _ in range(400):
            d = tuple(R.random_int(rng, 0, n - 1 - i) for i in range(3))
            seen.add(d)
            got = R.triple(n, *d)
            assert got == R.triple_literal(n, d), (n, d)
            assert len(set(got)) == 3 and all(0 <= i < n for i in got)
        if n <= 5:
            assert len(seen) == n * (n - 1) * (n - 2)   # every draw that exists


def test_literal_scan_equals_first_count_above_min_inliers():
    assert R.scan_literal([3, 5, 5, 2], 20) == (-1, 2, 5, 4)           # a tie in the best count goes to the later iteration
    assert R.scan_literal([0, 0], 20) == (-1, 1, 0, 2)
    assert R.scan_literal([3, 21, 40], 20) == (1, 1, 21, 2)            # stops at the first success, not at the best
    assert R.scan_literal([25, 21, 22], 20) == (0, 0, 25, 1)
    assert R.scan_literal([20, 20, 19], 20) == (-1, 1, 20, 3)          # `>` min_inliers
    for seed in SEEDS:
        for P, w in zip(R.generator_case(seed)["problems"], R.generator_case(seed)["want"]):
            above = np.flatnonzero(w["counts_all"] > P["min_inliers"])
            assert w["first_success"] == (int(above[0]) if len(above) else -1)


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_seed_meets_its_conditions(seed):
    c = R.generator_case(seed)
    P, w = c["problems"], c["want"]
    assert tuple(len(p["X3Dc1"]) for p in P) == R.SIZES
    first = [x["first_success"] for x in w]
    print(seed, "ransac_max_its", [x["ransac_max_its"] for x in w], "first_success", first, "best_inliers", [x["best_inliers"] for x in w],
          "NaN models", [len(x["nan_hyps"]) for x in w], "margin (ulps)", ["%.0f" % x["margin_ulps"] for x in w])
    assert any(0 <= f < 5 for f in first)                       # success within the first round of five
    assert any(f >= 5 for f in first)                           # a replay in fives crosses a call
    # n = 19: below min_inliers, nothing runs; n = 20: equal to it, one iteration, which cannot have more than 20 inliers;
    # n = 21: three iterations, and a success would need every point
    assert (w[0]["ransac_max_its"], w[0]["first_success"], w[0]["best_iteration"], w[0]["best_inliers"]) == (1, -1, -1, 0)
    assert (w[0]["counts"] == -1).all() and not w[0]["inliers"].any()
    assert (w[1]["ransac_max_its"], w[1]["first_success"], w[1]["best_iteration"]) == (1, -1, 0) and w[1]["counts"][0] == w[1]["best_inliers"] <= 20
    assert w[2]["ransac_max_its"] == 3 and (w[2]["first_success"] < 0 or w[2]["best_inliers"] == 21)
    # all outliers: never succeeds, every iteration runs
    assert w[6]["first_success"] == -1 and (w[6]["counts"][: w[6]["ransac_max_its"]] >= 0).all() and w[6]["ransac_max_its"] == 35
    assert w[5]["ransac_max_its"] == 300
    # a degenerate triple: a model of NaNs, count 0, no error
    assert 1 in w[7]["nan_hyps"] and w[7]["counts_all"][1] == 0
    assert np.isnan(w[7]["models"][1]["T12"]).all()
    # no decision hangs on the last bits of cos / sin / atan2
    assert min(x["margin_ulps"] for x in w) >= 16
    # both scale modes occur among the problems that succeed
    assert {bool(p["fix_scale"]) for p, x in zip(P, w) if x["first_success"] >= 0} == {True, False}


def test_ransac_max_its_edge_cases():
    assert R.ransac_max_its(20, 0.99, 20, 300) == 1
    assert R.ransac_max_its(21, 0.99, 20, 300) == 3
    assert R.ransac_max_its(19, 0.99, 20, 300) == 1      # epsilon > 1: log of a negative number
    assert R.ransac_max_its(0, 0.99, 20, 300) == 1
    assert R.ransac_max_its(300, 0.99, 20, 300) == 300
    assert R.ransac_max_its(65, 0.99, 20, 300) == 156
    assert R.ransac_max_its(65, 1.0, 20, 300) == 1       # log(0): the quotient is infinite


@pytest.mark.parametrize("seed", SEEDS)
def test_host_tap_equals_reference_bit_for_bit(pkg, seed):
    c = R.generator_case(seed)
    got = pkg.capi.debug_sim3_host(c["problems"])
    for k, (g, w) in enumerate(zip(got, c["want"])):
        assert R.same(g, w), (k, g, w["counts"])
    # a problem alone, and without the counts array
    one = pkg.capi.debug_sim3_host(c["problems"][3:4])[0]
    assert R.same(one, c["want"][3])
    edge = [dict(c["problems"][4], probability=p, min_inliers=m, max_iterations=i) for p, m, i in ((1.0, 20, 300), (0.5, 130, 7), (0.99, 0, 2))]
    for g, P in zip(pkg.capi.debug_sim3_host([dict(P, draws=P["draws"][: P["max_iterations"]]) for P in edge]), edge):
        assert R.same(g, R.solve(dict(P, draws=P["draws"][: P["max_iterations"]])))


def test_draw_helper_follows_the_reference_formula(pkg):
    a = pkg.capi.sim3_draws(np.random.default_rng(5), 40, 50)
    b = R.draws_for(np.random.default_rng(5), 40, 50)
    assert a.dtype == np.int32 and (a == b).all()
    assert (a >= 0).all() and (a[:, 0] <= 39).all() and (a[:, 1] <= 38).all() and (a[:, 2] <= 37).all() and a[:, 0].max() > 30


def test_bad_arguments_are_refused_and_an_empty_batch_succeeds(pkg):
    P = R.generator_case(SEEDS[0])["problems"][3]
    assert pkg.capi.debug_sim3_host([]) == []
    n = len(P["X3Dc1"])
    for i, bad in ((0, n), (1, n - 1), (2, n - 2), (0, -1)):
        d = P["draws"].copy()
        d[17, i] = bad
        with pytest.raises(pkg.AosError) as e:
            pkg.capi.debug_sim3_host([P, dict(P, draws=d)])
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
    with pytest.raises(pkg.AosError):
        pkg.capi.debug_sim3_host([dict(P, max_iterations=0, draws=P["draws"][:0])])
    with pytest.raises(pkg.AosError):
        pkg.capi.debug_sim3_host([P] * 65)
    # straight through the C ABI: n < 0, missing arrays
    C, L = pkg.capi.C, pkg.capi.lib()
    Pc, Rc, keep, outs = pkg.capi._sim3_args([P])
    assert L.aos2_debug_sim3_host(Pc, Rc, 1) == 0
    for field, value in (("n", -1), ("X3Dc1", None), ("X3Dc2", None), ("max_err1", None), ("max_err2", None), ("draws", None)):
        Pc, Rc, keep, outs = pkg.capi._sim3_args([P])
        setattr(Pc[0], field, value)
        assert L.aos2_debug_sim3_host(Pc, Rc, 1) == pkg.capi.AOS2_ERR_ARG, field
    Pc, Rc, keep, outs = pkg.capi._sim3_args([P])
    Rc[0].inliers = None
    assert L.aos2_debug_sim3_host(Pc, Rc, 1) == pkg.capi.AOS2_ERR_ARG
    assert L.aos2_debug_sim3_host(None, None, 1) == pkg.capi.AOS2_ERR_ARG and L.aos2_debug_sim3_host(None, None, 0) == 0
    Rc[0].inliers, Rc[0].counts = outs[0][0].ctypes.data, None   # counts is optional
    assert L.aos2_debug_sim3_host(Pc, Rc, 1) == 0 and Rc[0].first_success == R.generator_case(SEEDS[0])["want"][3]["first_success"]


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_shim_compiles_and_links_against_the_refstub(pkg, tmp_path, flags):
    """host/Sim3Solver.h compiles (-Wall -Werror, both error conventions) against the unchanged stand-ins of tests/cpp/refstub and
    links against libaos2 (the run needs the GPU: tests/test_sim3_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "sim3_solver_test.cpp"),
                           "-o", str(tmp_path / "sim3_solver_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
