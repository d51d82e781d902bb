"""aos2_sim3_ransac / host/Sim3Solver.h on the GPU against tests/sim3_ref.py: ransac_max_its, first_success, the best state, the counts
and the inlier flags exactly, T12 / R12 / t12 / s12 bit for bit where finite and NaN in the same places.  The workload is the
generator's batch (tests/test_sim3_cpu.py asserts what its seeds cover)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import sim3_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 3
SENTINEL = 0x5A


def raw(res):
    """every byte of a result"""
    return b"".join([np.array([res[k] for k in ("ransac_max_its", "first_success", "best_iteration", "best_inliers")], np.int32).tobytes()] +
                    [np.ascontiguousarray(res[k]).tobytes() for k in ("T12", "R12", "t12", "s12", "inliers", "counts")])


@pytest.fixture(scope="module")
def world(pkg, gpu):
    c = R.generator_case(SEED)
    M = pkg.capi.Matcher(0.75, True, device=0)
    return c, M, M.Sim3Ransac(c["problems"])


def test_batch_equals_the_reference_and_one_problem_at_a_time_equals_the_batch(world):
    c, M, batch = world
    for k, (g, w) in enumerate(zip(batch, c["want"])):
        assert R.same(g, w), (k, {x: g[x] for x in ("ransac_max_its", "first_success", "best_iteration", "best_inliers")}, g["counts"][:12], w["counts"][:12])
    for k, P in enumerate(c["problems"]):
        assert raw(M.Sim3Ransac([P])[0]) == raw(batch[k]), k
    assert M.Sim3Ransac([]) == []


def test_two_consecutive_calls_give_identical_bytes(world):
    c, M, batch = world
    again = M.Sim3Ransac(c["problems"])
    assert [raw(a) for a in again] == [raw(b) for b in batch]


def test_a_problem_below_min_inliers_leaves_its_neighbours_unchanged(world):
    c, M, batch = world
    P = c["problems"]
    assert len(P[0]["X3Dc1"]) == 19 and batch[0]["first_success"] == -1 and batch[0]["best_iteration"] == -1 and (batch[0]["counts"] == -1).all()
    without = M.Sim3Ransac(P[1:])
    assert [raw(a) for a in without] == [raw(b) for b in batch[1:]]
    order = [3, 0, 5, 0, 7]   # ... in the middle of a batch, and twice
    mixed = M.Sim3Ransac([P[k] for k in order])
    assert [raw(a) for a in mixed] == [raw(batch[k]) for k in order]
    only = M.Sim3Ransac([P[0]])   # nothing to launch at all
    assert raw(only[0]) == raw(batch[0])


def test_bad_draws_are_refused_and_the_result_buffers_keep_their_sentinel(pkg, world):
    c, M, batch = world
    P = c["problems"]
    n = len(P[4]["X3Dc1"])
    for it, i, bad in ((0, 0, n), (299, 2, n - 2), (150, 1, -1)):
        d = P[4]["draws"].copy()
        d[it, i] = bad
        with pytest.raises(pkg.AosError) as e:
            M.Sim3Ransac([P[3], dict(P[4], draws=d), P[5]], sentinel=SENTINEL)
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
        Rc, outs = M.sim3_last
        for k in range(3):
            assert (outs[k][0] == SENTINEL).all() and (outs[k][1] == SENTINEL).all()
            assert Rc[k].first_success == SENTINEL and Rc[k].best_inliers == SENTINEL and Rc[k].ransac_max_its == SENTINEL
    assert [raw(a) for a in M.Sim3Ransac(P)] == [raw(b) for b in batch]   # the handle is as good as before


# ---------------------------------------------------------------------------------------------- the class at the reference's signature
def _rigid(rng):
    Rm = R._rotation(rng.normal(size=3), rng.uniform(0.1, 1.0))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, rng.uniform(-1, 1, 3)
    return T.astype(np.float32)


def _stub_transform(T, Xw):
    """Rcw * X3Dw + tcw as the stand-in cv::Mat of tests/cpp/refstub forms it: the product accumulated in double and rounded, then a
    float sum"""
    Rm, X = T[:3, :3].astype(np.float64), Xw.astype(np.float64)
    prod = ((Rm[:, 0] * X[:, 0:1] + Rm[:, 1] * X[:, 1:2]) + Rm[:, 2] * X[:, 2:3]).astype(np.float32)
    return prod + T[:3, 3]


EXTRA1 = {0: 0, 3: 2, 5: 3, 7: 1, 9: 1, 11: 1}   # feature of keyframe 1 -> mp1_state, for the features the constructor's gates reject


def solver_case(rng, P, per_call):
    """keyframes, map points and matches whose Sim3Solver has the correspondences of problem P (in order) after the gates of :62-103,
    and one feature for every gate -> (bundle arrays, the problem as the solver forms it, the keyframe-1 feature of each correspondence)"""
    n = len(P["X3Dc1"])
    N1, M = n + len(EXTRA1), n + 2
    feat1 = np.array([i for i in range(N1) if i not in EXTRA1], np.int32)
    feat2 = rng.permutation(n + 3)[:n].astype(np.int32)
    T1, T2 = _rigid(rng), _rigid(rng)
    s2 = np.array(R.level_sigma2(), np.float32)
    oct1, oct2 = rng.integers(0, 8, N1).astype(np.int32), rng.integers(0, 8, n + 3).astype(np.int32)

    def world_of(T, Xc):
        return ((Xc.astype(np.float64) - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)).astype(np.float32)

    mp1_pos, mp1_state = np.zeros((N1, 3), np.float32), np.ones(N1, np.int32)
    mp1_pos[feat1] = world_of(T1, P["X3Dc1"])
    for f, st in EXTRA1.items():
        mp1_state[f] = st
    mp2_pos = np.zeros((M, 3), np.float32)
    mp2_pos[:n] = world_of(T2, P["X3Dc2"])
    mp2_feat, mp2_bad = np.concatenate([feat2, [0, -1]]).astype(np.int32), np.zeros(M, np.uint8)
    mp2_bad[n] = 1
    matched12 = np.full(N1, -1, np.int32)
    matched12[feat1] = np.arange(n)
    matched12[[0, 3, 5]] = 0           # rejected by keyframe 1's side: no map point, a bad one, one that does not observe the keyframe
    matched12[7], matched12[9] = n, n + 1   # rejected by keyframe 2's side: a bad point, one that does not observe the keyframe
    # (feature 11: a good map point without a match)
    arrays = dict(ransac=np.array([P["min_inliers"], P["max_iterations"], per_call, int(P["fix_scale"])], np.int32), prob=np.array([P["probability"]], np.float64),
                  kf1_Tcw=T1.reshape(16), kf2_Tcw=T2.reshape(16), kf1_cam=np.array(P["K1"], np.float32), kf2_cam=np.array(P["K2"], np.float32),
                  kf1_sigma2=s2, kf2_sigma2=s2, kf1_octave=oct1, kf2_octave=oct2, mp1_pos=mp1_pos, mp1_state=mp1_state, mp2_pos=mp2_pos,
                  mp2_feat=mp2_feat, mp2_bad=mp2_bad, matched12=matched12)
    # the thresholds as the class forms them: 9.210 * sigmaSquare stored in a vector<size_t> (include/Sim3Solver.h:78-79)
    trunc = lambda o: np.array([float(int(9.210 * float(s2[k]))) for k in o], np.float32)   # noqa: E731
    Q = dict(P, X3Dc1=_stub_transform(T1, mp1_pos[feat1]), X3Dc2=_stub_transform(T2, mp2_pos[:n]), max_err1=trunc(oct1[feat1]), max_err2=trunc(oct2[feat2]))
    return arrays, Q, feat1


def solver_cases(seed):
    """two solvers in one process, as LoopClosing::ComputeSim3 sets them up: SetRansacParameters(0.99, 20, 300), iterate(5, ...)"""
    c = R.generator_case(seed)
    rng = np.random.default_rng(seed + 100)
    rand = rng.integers(0, 2 ** 31, 3 * 400).astype(np.int32)
    arrays, expect, pos = {"rand": rand}, [], 0
    for k, P in enumerate((c["problems"][3], c["problems"][6])):
        a, Q, feat1 = solver_case(rng, P, 5)
        n = len(Q["X3Dc1"])
        its = R.ransac_max_its(n, Q["probability"], Q["min_inliers"], Q["max_iterations"])
        draws = np.zeros((its, 3), np.int32)
        for it in range(its):       # the class draws 3 * mRansacMaxIts integers in iteration order at its first iterate()
            for i in range(3):
                d = n - 1 - i + 1
                draws[it, i] = int((float(rand[pos]) / (2147483647.0 + 1.0)) * d)
                pos += 1
        want = R.solve(dict(Q, max_iterations=its, draws=draws))
        arrays.update({"c%d_%s" % (k, name): v for name, v in a.items()})
        expect.append((want, feat1, len(a["matched12"])))
    return arrays, expect


def test_solver_cases_cover_a_late_success_and_an_exhausted_solver():
    """(needs no device) what the next test relies on"""
    _, expect = solver_cases(SEED)
    (w0, _, _), (w1, _, _) = expect
    print("first_success", w0["first_success"], w1["first_success"], "its", w0["ransac_max_its"], w1["ransac_max_its"], "margin", w0["margin_ulps"], w1["margin_ulps"])
    assert w0["first_success"] >= 5 and w0["best_inliers"] > 20
    assert w1["first_success"] == -1 and w1["ransac_max_its"] == 35
    assert min(w0["margin_ulps"], w1["margin_ulps"]) >= 16


def test_sim3solver_class_replays_the_reference_loop(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "sim3_solver_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "sim3_solver_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    arrays, expect = solver_cases(SEED)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    bits = lambda a: np.ascontiguousarray(a, np.float32).ravel().view(np.uint32)   # noqa: E731
    # the candidate that succeeds: in the call that holds iteration first_success
    want, feat1, N1 = expect[0]
    assert int(out["c0_found"][0]) == 1 and int(out["c0_no_more"][0]) == 0
    assert int(out["c0_calls"][0]) == want["first_success"] // 5 + 1
    assert int(out["c0_n_inliers"][0]) == want["best_inliers"]
    vb = np.zeros(N1, np.uint8)
    vb[feat1] = want["inliers"]
    assert (out["c0_inliers"] == vb).all() and vb.sum() == want["best_inliers"]
    assert (bits(out["c0_T12"]) == bits(want["T12"])).all() and (bits(out["c0_R12"]) == bits(want["R12"])).all()
    assert (bits(out["c0_t12"]) == bits(want["t12"])).all() and (bits(out["c0_s12"]) == bits(want["s12"])).all()
    # all outliers: bNoMore after ceil(ransac_max_its / 5) calls, never a matrix
    want, feat1, N1 = expect[1]
    assert int(out["c1_found"][0]) == 0 and int(out["c1_no_more"][0]) == 1
    assert int(out["c1_calls"][0]) == -(-want["ransac_max_its"] // 5) == 7
    assert int(out["c1_n_inliers"][0]) == 0 and not out["c1_inliers"].any() and len(out["c1_inliers"]) == N1
