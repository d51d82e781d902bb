"""aos2_optimize_sim3 / host/OptimizeSim3.h on the GPU against tests/sim3_opt_ref.py under the comparison rule (decisions exact: the
outlier flags, n_bad, n_inliers, the return path; R(q12), t12, s12 within max(1e-5, 4 x the problem's measured resolution);
iterations / trials not compared), and against itself byte for byte: alone or in a batch, from call to call, in any order.  The
workload is the generator's batch (tests/test_sim3_opt_cpu.py asserts what its seeds cover and that no decision is marginal)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import sim3_opt_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 3
SENTINEL = 0x5A


def raw(res):
    """every byte of a result"""
    return b"".join([np.ascontiguousarray(res[k], np.float64).tobytes() for k in ("q12", "t12", "s12")] + [np.ascontiguousarray(res["outlier"]).tobytes()] +
                    [np.array([res["n_bad"], res["n_inliers"]] + list(res["iterations"]) + list(res["trials"]), np.int32).tobytes()])


def s12_in(P):
    return b"".join(np.ascontiguousarray(P[k], np.float64).tobytes() for k in ("q12", "t12", "s12"))


@pytest.fixture(scope="module")
def world(pkg, gpu):
    c = R.generator_case(SEED)
    L = pkg.capi.LocalBA(device=0)
    return c, L, L.OptimizeSim3(c["problems"])


def test_batch_equals_the_reference_and_one_problem_at_a_time_equals_the_batch(world):
    c, L, batch = world
    assert set((0, 9, 10, 31, 32, 33, 64, 127, 128, 129, 300)) <= set(len(P["X1c"]) for P in c["problems"])
    for k, (g, w, P, r) in enumerate(zip(batch, c["want"], c["problems"], c["resolution"])):
        ok, msg = R.same(g, w, P, r)
        print(k, "n", len(P["X1c"]), "difference %.2e" % np.abs(R.values(g) - R.values(w)).max(), "tolerance %.1e" % R.tolerance(r), "iterations", g["iterations"],
              w["iterations"], "trials", g["trials"], w["trials"])
        assert ok, (k, msg)
    for k, P in enumerate(c["problems"]):
        assert raw(L.OptimizeSim3([P])[0]) == raw(batch[k]), k
    assert L.OptimizeSim3([]) == []


def test_two_consecutive_calls_give_identical_bytes(world):
    c, L, batch = world
    again = L.OptimizeSim3(c["problems"])
    assert [raw(a) for a in again] == [raw(b) for b in batch]


def test_a_reordered_batch_with_a_repeated_problem_gives_the_same_bytes_per_problem(world):
    c, L, batch = world
    order = [10, 3, 7, 3, 0, 11, 5, 1, 9, 3, 2, 8, 6, 4]
    mixed = L.OptimizeSim3([c["problems"][k] for k in order])
    assert [raw(a) for a in mixed] == [raw(batch[k]) for k in order]


def test_an_empty_problem_and_an_early_return_leave_their_neighbours_unchanged(world):
    c, L, batch = world
    P, w = c["problems"], c["want"]
    i0, i1212 = R.SIZES.index(0), len(R.SIZES) - 1
    assert len(P[i0]["X1c"]) == 0 and not w[i1212]["wrote"] and w[i1212]["outlier"].any() and len(P[i1212]["X1c"]) == 10
    order = [6, i0, 4, i1212, 8]
    mixed = L.OptimizeSim3([P[k] for k in order])
    assert [raw(a) for a in mixed] == [raw(batch[k]) for k in order]
    without = L.OptimizeSim3([P[6], P[4], P[8]])
    assert [raw(a) for a in without] == [raw(batch[k]) for k in (6, 4, 8)]
    for k in (1, 3):   # their own S12: the input, bit for bit
        assert raw(mixed[k])[:64] == s12_in(P[order[k]]) and mixed[k]["n_inliers"] == 0
    assert mixed[1]["n_bad"] == 0 and mixed[3]["n_bad"] == w[i1212]["n_bad"] > 0 and (mixed[3]["outlier"] == w[i1212]["outlier"]).all()
    only = L.OptimizeSim3([P[i0]])   # nothing to launch at all
    assert raw(only[0]) == raw(batch[i0])


def test_fix_scale_leaves_s12_bit_identical(world):
    c, L, batch = world
    fixed = [dict(P, fix_scale=True, s12=np.float64(1.0371)) for P in c["problems"] if len(P["X1c"]) >= 10]
    got = L.OptimizeSim3(fixed)
    assert any(g["n_inliers"] > 0 for g in got)
    for g in got:
        assert np.float64(g["s12"]).tobytes() == np.float64(1.0371).tobytes()
    for g, P in zip(batch, c["problems"]):
        if P["fix_scale"]:
            assert np.float64(g["s12"]).tobytes() == np.float64(P["s12"]).tobytes()


def test_a_refused_call_leaves_the_sentinel_and_the_handle_works_afterwards(pkg, world):
    c, L, batch = world
    P = c["problems"]
    for bad in (dict(P[5], th2=0.0), dict(P[5], th2=-3.0)):
        with pytest.raises(pkg.AosError) as e:
            L.OptimizeSim3([P[4], bad, P[6]], sentinel=SENTINEL)
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
        Rc, outs = L.sim3_opt_last
        for k in range(3):
            assert (outs[k] == SENTINEL).all() and Rc[k].n_bad == SENTINEL and Rc[k].n_inliers == SENTINEL
            assert bytes(bytearray(Rc[k])[:64]) == bytes([SENTINEL]) * 64
    Pc, Rc, keep, outs = pkg.capi._sim3_opt_args([P[4], P[5]], sentinel=SENTINEL)
    Pc[1].obs2 = None
    assert L.L.aos2_optimize_sim3(L.h, Pc, Rc, 2) == pkg.capi.AOS2_ERR_ARG
    assert all((o == SENTINEL).all() for o in outs) and Rc[0].n_inliers == SENTINEL
    assert [raw(a) for a in L.OptimizeSim3(P)] == [raw(b) for b in batch]   # the handle is as good as before


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


# feature of keyframe 1 -> (mp1_state, match): one feature for every way out of :1102-1137
GATES = {0: (0, "good"), 3: (2, "good"), 5: (1, "bad"), 7: (1, "unseen"), 9: (1, None)}


def class_case(rng, P):
    """keyframes, map points and matches from which the loop of :1100-1179 gathers the correspondences of problem P (in order), with
    one feature for every gate -> (bundle arrays, the problem as the class forms it, the keyframe-1 feature of each correspondence)"""
    n = len(P["X1c"])
    N1, M = n + len(GATES), n + 2
    feat1 = np.array([i for i in range(N1) if i not in GATES], np.int32)
    feat2 = rng.permutation(n + 3)[:n].astype(np.int32)
    T1, T2 = _rigid(rng), _rigid(rng)
    inv_s2 = (1.0 / 1.44 ** np.arange(8)).astype(np.float32)

    def world_of(T, Xc):
        return ((Xc.astype(np.float64) - T[:3, 3].astype(np.float64)) @ T[:3, :3].astype(np.float64)).astype(np.float32)

    mp1_pos, mp1_state = np.zeros((N1, 3), np.float32), np.ones(N1, np.int32)
    mp1_pos[feat1] = world_of(T1, P["X1c"])
    mp1_pos[[3, 5, 7, 9]] = mp1_pos[feat1[:4]]
    mp2_pos = np.zeros((M, 3), np.float32)
    mp2_pos[:n] = world_of(T2, P["X2c"])
    mp2_pos[n:] = mp2_pos[:2]
    mp2_feat, mp2_bad = np.concatenate([feat2, [0, -1]]).astype(np.int32), np.zeros(M, np.uint8)
    mp2_bad[n] = 1
    matched12 = np.full(N1, -1, np.int32)
    matched12[feat1] = np.arange(n)
    for f, (state, match) in GATES.items():
        mp1_state[f] = state
        matched12[f] = {"good": 0, "bad": n, "unseen": n + 1, None: -1}[match]
    oct1, pt1 = rng.integers(0, 8, N1).astype(np.int32), rng.uniform(0, 600, (N1, 2)).astype(np.float32)
    oct2, pt2 = rng.integers(0, 8, n + 3).astype(np.int32), rng.uniform(0, 600, (n + 3, 2)).astype(np.float32)
    oct1[feat1], pt1[feat1], oct2[feat2], pt2[feat2] = P["oct1"], P["obs1"], P["oct2"], P["obs2"]
    arrays = dict(params=np.array([P["th2"], float(P["fix_scale"])], np.float32), sim3=np.concatenate([P["q12"], P["t12"], [P["s12"]]]).astype(np.float64),
                  kf1_Tcw=T1.reshape(16), kf2_Tcw=T2.reshape(16), kf1_cam=np.array(P["K1"], np.float32), kf2_cam=np.array(P["K2"], np.float32),
                  kf1_inv_sigma2=inv_s2, kf2_inv_sigma2=inv_s2, kf1_octave=oct1, kf2_octave=oct2, kf1_pt=pt1, kf2_pt=pt2, mp1_pos=mp1_pos,
                  mp1_state=mp1_state, mp2_pos=mp2_pos, mp2_feat=mp2_feat, mp2_bad=mp2_bad, matched12=matched12)
    Q = dict(P, X1c=_stub_transform(T1, mp1_pos[feat1]), X2c=_stub_transform(T2, mp2_pos[:n]))
    assert (inv_s2[P["oct1"]] == P["inv_sigma2_1"]).all() and (inv_s2[P["oct2"]] == P["inv_sigma2_2"]).all()
    return arrays, Q, feat1, matched12 >= 0


_CLASS = {}


def class_cases(seed):
    """two candidates in one process: one that is accepted (64 correspondences, 10 gross outliers, a far start) and one that returns
    through :1212 with a match erased (10 correspondences, one gross outlier)"""
    if seed not in _CLASS:
        c = R.generator_case(seed)
        rng = np.random.default_rng(seed + 200)
        arrays, expect = {}, []
        for k, P in enumerate((c["problems"][6], c["problems"][len(R.SIZES) - 1])):
            a, Q, feat1, matched = class_case(rng, P)
            want = R.optimize_sim3(Q)
            arrays.update({"c%d_%s" % (k, name): v for name, v in a.items()})
            expect.append((Q, want, R.resolution(Q, want), feat1, matched))
        _CLASS[seed] = (arrays, expect)
    return _CLASS[seed]


def test_class_cases_cover_an_accepted_candidate_and_an_early_return():
    """(needs no device) what the next test relies on"""
    _, expect = class_cases(SEED)
    (Q0, w0, (r0, same0), _, _), (Q1, w1, (r1, same1), _, _) = expect
    print("n_bad", w0["n_bad"], w1["n_bad"], "n_inliers", w0["n_inliers"], w1["n_inliers"], "margin", w0["margin"], w1["margin"], "resolution", r0, r1)
    assert w0["wrote"] and w0["n_bad"] > 0 and w0["n_inliers"] >= 20
    assert not w1["wrote"] and w1["n_bad"] > 0 and w1["n_inliers"] == 0
    assert min(w0["margin"], w1["margin"]) >= R.MARGIN and same0 and same1


def test_optimizer_class_gathers_calls_and_writes_back_like_the_reference(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "optimize_sim3_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "optimize_sim3_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    arrays, expect = class_cases(SEED)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    for k, (Q, want, (res, _), feat1, matched) in enumerate(expect):
        after = matched.copy()
        after[feat1[want["outlier"] != 0]] = False   # nulled at the feature indices of the outliers; the gated features keep their matches
        assert (out["c%d_matched" % k] != 0).tolist() == after.tolist(), k
        assert int(out["c%d_ret" % k][0]) == want["n_inliers"], k
        s = out["c%d_sim3" % k]
        got = dict(q12=s[:4], t12=s[4:7], s12=s[7], outlier=want["outlier"], n_bad=want["n_bad"], n_inliers=int(out["c%d_ret" % k][0]))
        ok, msg = R.same(got, want, Q, res)
        assert ok, (k, msg)
    assert expect[0][1]["wrote"] and out["c0_sim3"].tobytes() != arrays["c0_sim3"].tobytes()
    assert not expect[1][1]["wrote"] and out["c1_sim3"].tobytes() == arrays["c1_sim3"].tobytes()   # g2oS12 untouched
