"""The RANSAC of PnPsolver (src/PnPsolver.cc) without a GPU: the CPU restatement the GPU tests compare against (tests/pnp_ref.py)
checked against independent knowledge (numpy's SVD and least squares, planted poses, a literal replay of the index removal and of
the loop), the library's host tap (aos2_debug_pnp_host: the routines the device kernels run, csrc/pnp.h) checked against it bit for
bit, the conditions the shared generator has to meet, the argument checks, and the host class's compile + link."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ref as R  # noqa: E402

SEEDS = (3, 4, 5)
EPS = R.DBL_EPSILON
SENTINEL = 0x5A
K = [float(np.float32(k)) for k in R.CAMERA]


def public(P):
    return {k: v for k, v in P.items() if k not in ("member", "structures", "ransac_max_its", "octave")}


def noise_free(rng, n):
    """n points in the generator's box and their exact projections under a planted pose, rounded to float32"""
    pose = R.planted_pose(rng)
    P = R.problem(rng, n, [(n, pose)], noise=0.0)
    return P, pose


# ---------------------------------------------------------------------------------------- the reference against independent knowledge
def test_jacobi_svd_agrees_with_numpy():
    """Singular values of random 6x4 / 3x3 / 6x5 / 6x3 inputs and of the M'M below: within 28 DBL_EPSILON |A| (measured: 6.8; 4x
    margin).  The projector onto the four smallest directions of M'M for the M of 4-point (8x12: those four singular values are
    rounding noise, single vectors mean nothing) and 30-point (60x12) noise-free sets, taken from the accumulated rotations:
    max |P - P_numpy| * gap / |M'M| is measured at 0.44 DBL_EPSILON (8x12) and 0.29 (60x12) over the cases below, gap = the distance
    between the fourth and fifth smallest eigenvalues; asserted with a 4x margin at 1.8 DBL_EPSILON.  The rotations stay orthonormal
    to 16 DBL_EPSILON."""
    rng = np.random.default_rng(21)
    worst = 0.0
    for shape in ((6, 4), (3, 3), (6, 5), (6, 3)):
        for _ in range(30):
            A = rng.normal(size=shape)
            W, At, V, sweeps = R.jacobi_svd(A.T.tolist())
            assert sweeps < 30 and all(W[i] >= W[i + 1] for i in range(len(W) - 1))
            s = np.linalg.svd(A, compute_uv=False)
            worst = max(worst, np.abs(np.array(W) - s).max() / (EPS * s[0]))
            Vm = np.array(V)
            assert np.abs(Vm @ Vm.T - np.eye(len(V))).max() <= 16 * EPS
            # A = U diag(W) V': the rotated rows are W[i] u_i
            assert np.abs((np.array(At).T / np.array(W)) @ np.diag(W) @ Vm - A).max() <= 32 * EPS * s[0]
    worst_proj = {4: 0.0, 30: 0.0}
    for n in (4, 30):
        for _ in range(20):
            P, _ = noise_free(rng, n)
            d = {}
            R.pose_of(P, list(range(n)), detail=d)
            mtm = d["mtm"]
            s = np.linalg.svd(mtm, compute_uv=False)
            worst = max(worst, np.abs(np.array(d["D"]) - s).max() / (EPS * s[0]))
            Vm = np.array(d["ut"])
            assert np.abs(Vm @ Vm.T - np.eye(12)).max() <= 16 * EPS
            w, v = np.linalg.eigh(mtm)
            gap = w[4] - w[3]
            proj = Vm[8:].T @ Vm[8:]
            want = v[:, :4] @ v[:, :4].T
            worst_proj[n] = max(worst_proj[n], np.abs(proj - want).max() * gap / (EPS * s[0]))
    print("worst singular value difference / (DBL_EPSILON |A|):", worst, "worst projector difference * gap / (DBL_EPSILON |M'M|):", worst_proj)
    assert worst <= 28
    assert max(worst_proj.values()) <= 1.8


def test_qr_solve_agrees_with_lstsq():
    """6x4 systems with a condition number below 1e3: |x - lstsq| <= 1e3 * 64 DBL_EPSILON |x| (Householder QR is backward stable; the
    bound is condition * a small multiple of the unit roundoff)"""
    rng = np.random.default_rng(22)
    worst, used = 0.0, 0
    for _ in range(200):
        A, b = rng.normal(size=(6, 4)), rng.normal(size=6)
        if np.linalg.cond(A) > 1e3:
            continue
        used += 1
        x, ok = R.qr_solve(A.tolist(), b.tolist(), [0.0] * 4)
        want = np.linalg.lstsq(A, b, rcond=None)[0]
        worst = max(worst, np.abs(np.array(x) - want).max() / (EPS * np.abs(want).max()))
        assert ok and np.abs(np.array(x) - want).max() <= 1e3 * 64 * EPS * np.abs(want).max()
    assert used >= 150
    print("worst |x - lstsq| / (DBL_EPSILON |x|):", worst)
    # a singular column: x keeps what it held
    x, ok = R.qr_solve([[0.0] * 4 for _ in range(6)], [1.0] * 6, [1.0, 2.0, 3.0, 4.0])
    assert not ok and x == [1.0, 2.0, 3.0, 4.0]


def test_noise_free_sets_of_ten_and_more_points_give_the_planted_pose_back():
    """n = 10, 30, 100 exact projections rounded to float32 (the pixels carry 3e-5 of rounding, the points 2.4e-7 relative): the
    planted pose comes back within 2.4e-7 on R and 1.3e-6 on t (measured over the sets below: 5.8e-8 and 3.2e-7; 4x margin)"""
    rng = np.random.default_rng(23)
    worst_R = worst_t = 0.0
    for n in (10, 30, 100):
        for _ in range(12):
            P, (Rp, tp) = noise_free(rng, n)
            Rg, tg, errs = R.pose_of(P, list(range(n)))
            worst_R = max(worst_R, np.abs(np.array(Rg) - Rp).max())
            worst_t = max(worst_t, np.abs(np.array(tg) - tp).max())
    print("worst |R - planted|:", worst_R, "worst |t - planted|:", worst_t)
    assert worst_R <= 2.4e-7 and worst_t <= 1.3e-6


def test_quadruples_order_their_candidates_and_ignore_the_sign_of_the_null_space_rows():
    """4-point EPnP does not reliably give the planted pose back (the count is printed), so only: the winner is the candidate with
    the smallest reprojection error under the strict test in the order 1, 2, 3, and a sign flip of any null-space row leaves R and t
    unchanged up to rounding -- negation is exact, so every intermediate keeps its magnitude: 64 DBL_EPSILON of the pose's scale"""
    rng = np.random.default_rng(24)
    recovered = total = 0
    for _ in range(40):
        P, (Rp, tp) = noise_free(rng, 4)
        d = {}
        Rg, tg, errs = R.pose_of(P, [0, 1, 2, 3], detail=d)
        total += 1
        recovered += bool(np.abs(np.array(Rg) - Rp).max() < 1e-3)
        N = 0
        if errs[1] < errs[0]:
            N = 1
        if errs[2] < errs[N]:
            N = 2
        assert d["winner"] == N and (np.array(Rg) == np.array(d["cands"][N][0])).all()
        assert all(not errs[k] < errs[N] for k in range(3))
        scale = max(1.0, np.abs(np.array(tg)).max())
        for flip in ((-1, 1, 1, 1), (1, -1, 1, 1), (1, 1, -1, 1), (1, 1, 1, -1), (-1, -1, -1, -1)):
            Rf, tf, errs_f = R.pose_of(P, [0, 1, 2, 3], null_signs=flip)
            assert np.abs(np.array(Rf) - np.array(Rg)).max() <= 64 * EPS * scale and np.abs(np.array(tf) - np.array(tg)).max() <= 64 * EPS * scale
    print("noise-free quadruples that give the planted pose back:", recovered, "of", total)


def test_index_removal_of_the_library_equals_the_literal_vector(pkg):
    rng = np.random.default_rng(25)
    for n, ms in ((4, 4), (5, 4), (6, 5), (9, 4), (64, 4), (20, 16), (16, 16)):
        seen = set()
        for _ in range(300):
            row = [R.random_int(rng, 0, n - 1 - i) for i in range(ms)]
            seen.add(tuple(row))
            got = pkg.capi.debug_pnp_set(n, row)
            assert got == R.set_literal(n, row), (n, row)
            assert len(set(got)) == ms and all(0 <= i < n for i in got)
            assert R.draws_selecting(n, got) == row
        if n == 4:
            assert len(seen) == 24   # every draw that exists
    a = pkg.capi.pnp_draws(np.random.default_rng(5), 40, 50, 5)
    assert a.dtype == np.int32 and (a == R.draws_for(np.random.default_rng(5), 40, 50, 5)).all()
    assert all((a[:, i] >= 0).all() and (a[:, i] <= 39 - i).all() for i in range(5)) and a[:, 0].max() > 30


def test_memoised_scan_of_the_library_equals_the_literal_loop(pkg):
    """random count and Refine() tables, with and without a carried-in best, started anywhere"""
    rng = np.random.default_rng(26)
    returns = carried = 0
    for _ in range(600):
        its = int(rng.integers(0, 40))
        first = int(rng.integers(0, its + 1))
        mn = int(rng.integers(4, 12))
        counts = rng.integers(0, 2 * mn, its)
        refined = rng.integers(mn - 3, mn + 3, its)
        best_in = int(rng.choice([0, 0, mn, mn + 2, 2 * mn]))
        refined_carried = int(rng.integers(mn - 2, mn + 2))
        calls = []

        def refine_count_of(best_it):
            calls.append(best_it)
            return refined_carried if best_it < 0 else int(refined[best_it])

        want = R.scan_literal(first, counts[first:], refine_count_of, mn, best_in)
        got = pkg.capi.debug_pnp_scan(first, counts, refined, refined_carried, mn, best_in)
        assert got == want, (first, counts, refined, mn, best_in, refined_carried)
        returns += want[0] >= 0
        carried += -1 in calls
    assert returns >= 100 and carried >= 50
    assert pkg.capi.debug_pnp_scan(0, [5, 12, 12, 30], [0, 12, 99, 31], 0, 12) == (3, 3, 30)   # `>` min_inliers, a tie keeps the earlier best
    assert pkg.capi.debug_pnp_scan(0, [12, 13], [13, 12], 0, 12) == (0, 0, 12)
    assert pkg.capi.debug_pnp_scan(0, [12, 13], [12, 12], 0, 12) == (-1, 1, 13)


def test_ransac_parameters_edge_cases(pkg):
    p = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=4, epsilon=0.5)
    for f in (R.ransac_parameters, pkg.capi.pnp_ransac_parameters):
        assert f(9, **p)[0] == 10                                    # n = 9 is below the minimum: iterate() gives up at once
        assert (f(10, **p)[0], f(10, **p)[2]) == (10, 1)              # ... and iterate(5) still runs max(1, 5) iterations
        assert (f(11, **p)[0], f(11, **p)[2]) == (10, 4)
        assert all((f(n, **p)[0], f(n, **p)[2]) == (max(10, n // 2), 35) for n in (20, 21, 40, 64, 65, 150))
        assert f(64, **dict(p, epsilon=0.2)) == (12, np.float32(0.2), 300)
        assert f(15, **dict(p, min_set=5))[2] == 14
        assert f(0, **p)[2] == 1 and f(3, **dict(p, min_inliers=1, min_set=4))[0] == 4
        assert f(40, **dict(p, probability=1.0))[2] == 1              # log(0): the quotient is infinite, INT_MIN, so 1
        assert f(40, **dict(p, epsilon=float("nan")))[0] == 10        # N * epsilon is no int: INT_MIN, so the given minimum
    for n in (0, 1, 7, 10, 11, 33, 64, 150, 1000):
        for eps in (0.1, 0.2, 0.4, 0.5, 0.9):
            assert R.ransac_parameters(n, 0.99, 10, 300, 4, eps) == pkg.capi.pnp_ransac_parameters(n, 0.99, 10, 300, 4, eps), (n, eps)


# ---------------------------------------------------------------------------------------- the generator and the host tap
@pytest.mark.parametrize("seed", SEEDS)
def test_generator_seed_meets_its_conditions(seed):
    c = R.generator_case(seed)
    P, w = c["problems"], c["want"]
    assert tuple(len(p["P3Dw"]) for p in P) == R.SIZES
    ret = [x["returned_at"] for x in w]
    print(seed, "n_iterations", [p["n_iterations"] for p in P], "min_inliers", [p["min_inliers"] for p in P], "returned_at", ret,
          "best_inliers", [x["best_inliers"] for x in w], "refines", [len(x["refines"]) for x in w], "NaN models", [x["nan_hyps"] for x in w],
          "margin (ulps)", ["%.0f" % x["margin_ulps"] for x in w])
    assert [p["n_iterations"] for p in P] == [5, 5, 5, 14, 35, 300, 35, 35] and [p["min_set"] for p in P] == [4, 4, 4, 5, 4, 4, 4, 4]
    assert [p["ransac_max_its"] for p in P][:3] == [1, 1, 4]
    # 9: nothing runs
    assert ret[0] == -1 and (w[0]["counts"] == -1).all() and w[0]["best_iteration"] == -1 and not w[0]["best"].any()
    # a return within the first five iterations, and one later
    assert any(0 <= r < 5 for r in ret) and any(r >= 5 for r in ret)
    # 10: the exhaustion returns the unrefined best -- count >= min but Refine()'s count not above it
    assert ret[1] == -1 and w[1]["best_inliers"] == 10 == P[1]["min_inliers"] and w[1]["best"].all() and (w[1]["counts"] >= 0).all()
    assert w[1]["refines"] and all(r[2] <= 10 and not r[3] for r in w[1]["refines"]) and w[1]["best_Tcw"][3, 3] == 1
    # 65: all outliers, an exhaustion with nothing
    assert ret[6] == -1 and w[6]["best_inliers"] == 0 and w[6]["best_iteration"] == -1 and (w[6]["counts"] >= 0).all() and not w[6]["refines"]
    # 64: a Refine() that fails, a qualifying iteration that does not beat the best (the same Refine() again), then a record that returns
    assert [(r[0], r[1], r[3]) for r in w[5]["refines"]] == [(2, 2, False), (4, 2, False), (7, 7, True)] and ret[5] == 7
    assert w[5]["counts"][4] == w[5]["counts"][2] == 12 and w[5]["counts"][7] == 30
    # 40: a rank-deficient minimal set (two draws of one map point) stays finite under item 11, four draws of it give a NaN model;
    # both count 0 and nothing traps
    whole = R.solve(P[4], ignore_returns=True)
    assert whole["nan_hyps"] == [5] and whole["counts"][5] == 0 and whole["counts"][3] == 0
    Rn, tn, _ = R.pose_of(P[4], R.set_literal(40, P[4]["draws"][5]))
    assert np.isnan(np.array(Rn)).all() and np.isnan(np.array(tn)).all()
    # no inlier decision of any hypothesis or Refine() hangs on the last bits
    assert min(x["margin_ulps"] for x in w) >= 16 and whole["margin_ulps"] >= 16


@pytest.mark.parametrize("seed", SEEDS)
def test_host_tap_equals_reference_bit_for_bit(pkg, seed):
    c = R.generator_case(seed)
    problems = [public(P) for P in c["problems"]]
    got = pkg.capi.debug_pnp_host(problems)
    for k, (g, w) in enumerate(zip(got, c["want"])):
        assert R.same(g, w), (k, g["returned_at"], w["returned_at"], g["counts"][:12], w["counts"][:12])
    # a problem alone, and without the counts array
    for k in (4, 5):
        one = pkg.capi.debug_pnp_host(problems[k:k + 1], with_counts=False)[0]
        assert one["counts"] is None and R.same(one, c["want"][k], counts=False)
    # the NaN model and its neighbours: all 35 iterations of the n = 40 problem, whatever the loop does with them
    every = R.solve(c["problems"][4], ignore_returns=True)
    for it in (3, 5, 6):
        g = pkg.capi.debug_pnp_host([dict(problems[4], first_iteration=it, n_iterations=it + 1, draws=problems[4]["draws"][: it + 1])])[0]
        assert g["counts"][it] == every["counts"][it]


@pytest.mark.parametrize("seed", SEEDS)
def test_resumed_host_tap_equals_the_uninterrupted_loop(pkg, seed):
    """run to returned_at, then a second call from returned_at + 1 with the state carried in: the concatenation equals ONE literal
    loop that ignores the first return (its second return, or its exhaustion)"""
    c = R.generator_case(seed)
    second_returns = carried = 0
    for P0, first_call in zip(c["problems"], c["want"]):
        if first_call["returned_at"] < 0:
            continue
        P = public(P0)
        a = pkg.capi.debug_pnp_host([P])[0]
        whole = R.solve(P0, ignore_returns=True)
        Q = dict(P, first_iteration=a["returned_at"] + 1, best_inliers_in=a["best_inliers"], best_in=a["best"])
        b = pkg.capi.debug_pnp_host([Q])[0]
        assert R.same(b, R.solve(Q))   # the reference started from the carried state
        first = Q["first_iteration"]
        assert (b["counts"][:first] == -1).all()
        if len(whole["events"]) > 1:
            ev = whole["events"][1]
            second_returns += 1
            assert b["returned_at"] == ev["returned_at"] and b["n_inliers"] == ev["n_inliers"] and (b["inliers"] == ev["inliers"]).all()
            assert b["Tcw"].tobytes() == ev["Tcw"].tobytes() and b["best_inliers"] == ev["best_inliers"] and (b["best"] == ev["best"]).all()
            if ev["best_iteration"] >= first:
                assert b["best_iteration"] == ev["best_iteration"] and b["best_Tcw"].tobytes() == ev["best_Tcw"].tobytes()
            else:
                carried += 1
                assert b["best_iteration"] == -1 and not b["best_Tcw"].any()
            stop = ev["returned_at"] + 1
        else:
            assert b["returned_at"] == -1 and b["best_inliers"] == whole["best_inliers"] and (b["best"] == whole["best"]).all()
            stop = P["n_iterations"]
        assert (b["counts"][first:stop] == whole["counts"][first:stop]).all() and (b["counts"][stop:] == -1).all()
    print(seed, "second returns:", second_returns, "of them on the carried set:", carried)
    assert second_returns >= 1 and carried >= 1


def test_bad_arguments_are_refused_and_an_empty_batch_succeeds(pkg):
    P = public(R.generator_case(SEEDS[0])["problems"][4])
    want = R.generator_case(SEEDS[0])["want"][4]
    capi = pkg.capi
    assert capi.debug_pnp_host([]) == []
    n = len(P["P3Dw"])

    def refused(problems):
        with pytest.raises(pkg.AosError) as e:
            capi.debug_pnp_host(problems)
        assert e.value.code == capi.AOS2_ERR_ARG

    for it, i, bad in ((17, 0, n), (17, 1, n - 1), (34, 3, n - 3), (0, 0, -1)):
        d = P["draws"].copy()
        d[it, i] = bad
        refused([P, dict(P, draws=d)])
        if it == 17:   # rows below first_iteration are not read
            assert R.same(capi.debug_pnp_host([dict(P, draws=d, first_iteration=18)])[0], R.solve(dict(P, draws=d, first_iteration=18)))
    refused([P] * 65)
    refused([dict(P, first_iteration=36)])
    refused([dict(P, first_iteration=-1)])
    refused([dict(P, best_inliers_in=25)])                      # a carried count without its flags
    refused([dict(P, best_inliers_in=-1)])
    refused([dict(P, min_set=3, draws=P["draws"][:, :3])])
    refused([dict(P, min_set=17, draws=np.zeros((35, 17), np.int32))])
    small = {k: P[k][:3] for k in ("P3Dw", "P2D", "max_err")}
    refused([dict(P, **small, min_inliers=2, draws=np.zeros((35, 4), np.int32))])   # n < min_set with something to run
    ok = capi.debug_pnp_host([dict(P, **small, draws=np.zeros((35, 4), np.int32))])[0]   # n < min_inliers: nothing runs, no error
    assert ok["returned_at"] == -1 and (ok["counts"] == -1).all()
    ok = capi.debug_pnp_host([dict(P, first_iteration=35)])[0]   # nothing left to run
    assert ok["returned_at"] == -1 and (ok["counts"] == -1).all() and ok["best_inliers"] == 0
    # straight through the C ABI, with sentinel-filled result buffers that must stay untouched
    C, L = capi.C, capi.lib()
    Pc, Rc, keep, outs = capi._pnp_args([P])
    assert L.aos2_debug_pnp_host(Pc, Rc, 1) == 0 and Rc[0].returned_at == want["returned_at"]

    def untouched(Rc, outs):
        head = capi._PnpResult.inliers.offset
        return bytes(Rc[0])[:head] == bytes([SENTINEL]) * head and all((a == SENTINEL).all() for a in outs[0])

    for field, value in (("n", -1), ("P3Dw", None), ("P2D", None), ("max_err", None), ("draws", None), ("min_set", 3), ("first_iteration", 36)):
        Pc, Rc, keep, outs = capi._pnp_args([P], sentinel=SENTINEL)
        setattr(Pc[0], field, value)
        assert L.aos2_debug_pnp_host(Pc, Rc, 1) == capi.AOS2_ERR_ARG, field
        assert untouched(Rc, outs), field
    for field in ("inliers", "best"):
        Pc, Rc, keep, outs = capi._pnp_args([P], sentinel=SENTINEL)
        setattr(Rc[0], field, None)
        assert L.aos2_debug_pnp_host(Pc, Rc, 1) == capi.AOS2_ERR_ARG
    assert L.aos2_debug_pnp_host(None, None, 1) == capi.AOS2_ERR_ARG and L.aos2_debug_pnp_host(None, None, 0) == 0
    assert L.aos2_pnp_ransac_parameters(-1, 0.99, 10, 300, 4, 0.5, None, None, None) == capi.AOS2_ERR_ARG
    with pytest.raises(pkg.AosError):
        capi.debug_pnp_set(3, [0, 0, 0, 0])
    with pytest.raises(pkg.AosError):
        capi.debug_pnp_set(5, [0, 4, 0, 0])


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_class_compiles_and_links_against_the_refstub(pkg, tmp_path, flags):
    """host/PnPsolver.h compiles (-Wall -Werror, both error conventions) against the stand-ins of tests/cpp/refstub and links against
    libaos2 (the run needs the GPU)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "pnp_solver_test.cpp"),
                           "-o", str(tmp_path / "pnp_solver_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
