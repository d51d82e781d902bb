"""The loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:290-436) without a GPU: the CPU restatement the GPU tests
compare against (tests/triangulation_ref.py) checked against independent knowledge, the library's host tap
(aos2_debug_triangulate_host: the routine the device kernels run, csrc/triangulate.h) checked against it bit for bit, the
conditions the shared generator's seeds have to meet, and the host shim's compile + link."""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import triangulation_ref as R  # noqa: E402

SEEDS = (2, 3, 4)
CAM = dict(fx=520.9, fy=521.0, cx=325.1, cy=249.7, mbf=80.0)


def pose(center=(0.0, 0.0, 0.0), yaw=0.0):
    """Tcw of a camera at `center`, rotated by `yaw` about its y axis"""
    c, s = np.cos(yaw), np.sin(yaw)
    Rcw = np.array([[c, 0, -s], [0, 1, 0], [s, 0, c]])
    T = np.eye(4)
    T[:3, :3] = Rcw
    T[:3, 3] = -Rcw @ np.asarray(center, float)
    return T.astype(np.float32)


def kf(T, cam=CAM):
    return R.keyframe(T, cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"], R.scale_factors())


def observe(K, Pw, octave=0, stereo=False, du=0.0, dv=0.0, dur=0.0):
    """the noise-free observation of the world point Pw in keyframe K (+ pixel offsets)"""
    pc = K["Tcw"].astype(float) @ np.append(np.asarray(Pw, float), 1.0)
    u = K["fx"] * pc[0] / pc[2] + K["cx"] + du
    v = K["fy"] * pc[1] / pc[2] + K["cy"] + dv
    o = np.zeros((), R.OBS)
    o["ux"], o["uy"], o["kx"], o["ky"], o["octave"] = u, v, u, v, octave
    o["u_right"], o["depth"] = (u - K["mbf"] / pc[2] + dur, pc[2]) if stereo else (-1.0, -1.0)
    return o


def run(K1, K2, o1, o2):
    info = {}
    st, x = R.triangulate_pair(K1, K2, o1, o2, info)
    return st, np.array(x), info


def test_noise_free_projections_give_the_point_back():
    rng = np.random.default_rng(5)
    K1, K2 = kf(pose((0.01, -0.02, 0.0), 0.02)), kf(pose((0.41, 0.03, -0.02), -0.03))
    for _ in range(40):
        P = np.array([rng.uniform(-1, 1), rng.uniform(-0.7, 0.7), rng.uniform(1.5, 8.0)])
        st, x, info = run(K1, K2, observe(K1, P), observe(K2, P))
        assert st == R.ACCEPTED and info["branch"] == R.BRANCH_SVD
        assert np.linalg.norm(x - P) <= 1e-4 * np.linalg.norm(P), (x, P)


def test_jacobi_null_vector_agrees_with_numpy_svd():
    rng = np.random.default_rng(6)
    worst = 0.0
    for _ in range(200):
        A = rng.normal(size=(4, 4)).astype(np.float32)
        V, sweeps = R.jacobi_vt(A.tolist())
        assert sweeps < 30
        v = np.array(V[3])
        want = np.linalg.svd(A.astype(np.float64))[2][3]
        err = min(np.abs(v - want).max(), np.abs(v + want).max())
        worst = max(worst, err)
        assert err < 1e-5, (err, A)
    print("worst null-vector difference", worst)


def test_hand_made_case_for_every_reachable_status_and_branch():
    P = np.array([0.1, -0.05, 3.0])
    K1, side, ahead = kf(pose()), kf(pose((0.4, 0.0, 0.0))), kf(pose((0.0, 0.0, 0.12)))
    # the three ways to a point, all accepted and all at P
    for K2, o1, o2, branch in ((side, observe(K1, P), observe(side, P), R.BRANCH_SVD),
                               (ahead, observe(K1, P, stereo=True), observe(ahead, P), R.BRANCH_STEREO1),
                               (ahead, observe(K1, P), observe(ahead, P, stereo=True), R.BRANCH_STEREO2)):
        st, x, info = run(K1, K2, o1, o2)
        assert (st, info["branch"]) == (R.ACCEPTED, branch)
        assert np.linalg.norm(x - P) <= 1e-4 * np.linalg.norm(P)
    # 2: no stereo and the rays nearly parallel (0.4 m baseline at 80 m: cos = 1 - 1.25e-5 > 0.9998)
    far = np.array([0.5, 0.2, 80.0])
    assert run(K1, side, observe(K1, far), observe(side, far))[0] == R.LOW_PARALLAX
    # 2 as well: the stereo fallback on a feature whose mvDepth is not positive (UnprojectStereo returns an empty Mat)
    o = observe(K1, P, stereo=True)
    o["depth"] = 0.0
    assert run(K1, ahead, o, observe(ahead, P))[0] == R.LOW_PARALLAX
    # 4: the disparity has the wrong sign, the rays meet behind both cameras
    st, x, info = run(K1, side, observe(side, P), observe(K1, P))
    assert (st, info["branch"]) == (R.DEPTH1, R.BRANCH_SVD) and x[2] < 0
    # 5: the point unprojected from keyframe 1 lies behind a keyframe 2 that stands beyond it
    beyond = kf(pose((0.0, 0.0, 5.0)))
    st, x, info = run(K1, beyond, observe(K1, P, stereo=True), observe(K1, P))
    assert (st, info["branch"]) == (R.DEPTH2, R.BRANCH_STEREO1)
    # 6: the two observations are 10 px off the epipolar line, in opposite directions: keyframe 1 is tested first
    assert run(K1, side, observe(K1, P, dv=5.0), observe(side, P, dv=-5.0))[0] == R.REPROJ1
    # 6 through the stereo term alone: mvuRight off by 6 px, 36 > 7.8
    assert run(K1, side, observe(K1, P, stereo=True, dur=6.0), observe(side, P))[0] == R.REPROJ1
    # 7: 2.6 px either way passes at octave 7 (sigma2 = 12.8) and fails at octave 0 (6.8 > 5.991)
    assert run(K1, side, observe(K1, P, octave=7, dv=2.6), observe(side, P, dv=-2.6))[0] == R.REPROJ2
    # 7 through keyframe 2's stereo term, which uses keyframe 1's mbf (:410): the same observation passes with equal cameras and
    # fails when keyframe 1's mbf differs
    K1b = R.keyframe(pose(), CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"], 2 * CAM["mbf"], R.scale_factors())
    assert run(K1, side, observe(K1, P), observe(side, P, stereo=True))[0] == R.ACCEPTED
    assert run(K1b, side, observe(K1b, P), observe(side, P, stereo=True))[0] == R.REPROJ2
    # 9: equal distances, seven octaves apart
    assert run(K1, side, observe(K1, P), observe(side, P, octave=7))[0] == R.SCALE
    assert run(K1, side, observe(K1, P, octave=7), observe(side, P))[0] == R.SCALE


def test_first_wins_supersedes_later_neighbours_only():
    st = np.array([[1, 1, 6, 0], [1, 9, 1, 1], [1, 1, 1, 0], [1, 1, 1, 1]], np.uint8)
    R.resolve_first_wins([0, 0, 1, 0], st)
    assert st.tolist() == [[1, 1, 6, 0], [10, 9, 1, 1], [1, 1, 1, 0], [10, 10, 10, 10]]


@pytest.mark.parametrize("seed", SEEDS)
def test_generator_seed_meets_its_conditions(seed):
    """what the GPU tests rely on: every reachable status and branch occurs, and no decision hangs on the last bit of atan2 / cos"""
    for cams in ("same", "mixed"):
        c = R.generator_case(seed, cams)
        status = collections.Counter(c["status"].ravel().tolist())
        branch = collections.Counter(i["branch"] for i in c["infos"])
        margin = min(i["margin_ulps"] for i in c["infos"])
        sweeps = max(i["sweeps"] for i in c["infos"])
        print(seed, cams, dict(sorted(status.items())), dict(sorted(branch.items())), "margin", margin, "sweeps", sweeps)
        for s in (R.ACCEPTED, R.LOW_PARALLAX, R.DEPTH1, R.DEPTH2, R.REPROJ1, R.REPROJ2, R.SCALE, R.SUPERSEDED):
            assert status[s] >= 3, (s, status)
        for b in (R.BRANCH_SVD, R.BRANCH_STEREO1, R.BRANCH_STEREO2):
            assert branch[b] >= 3, (b, branch)
        assert margin >= 16 and sweeps < 30
        assert status[R.W_ZERO] == 0 and status[R.ZERO_DIST] == 0


@pytest.mark.parametrize("seed", SEEDS)
def test_host_tap_equals_reference_bit_for_bit(pkg, seed):
    for cams, distort in (("same", False), ("mixed", True)):
        c = R.generator_case(seed, cams, distort)
        S = c["scene"]
        for p, (a, b) in enumerate(R.PAIRS6):
            idx = np.flatnonzero(c["match12"][p] >= 0)
            st, x = pkg.capi.debug_triangulate_host(S["kfs"][a], S["kfs"][b], S["obs"][a][idx], S["obs"][b][c["match12"][p][idx]])
            assert (st == c["status_all"][p][idx]).all()
            assert (x.view(np.uint32) == c["x3D"][p][idx].view(np.uint32)).all()


def test_host_tap_rejects_what_it_would_index_out_of_range(pkg):
    c = R.generator_case(SEEDS[0])
    S = c["scene"]
    o = S["obs"][0][:4].copy()
    o["octave"][2] = 8
    with pytest.raises(pkg.AosError):
        pkg.capi.debug_triangulate_host(S["kfs"][0], S["kfs"][1], o, S["obs"][1][:4])
    st, x = pkg.capi.debug_triangulate_host(S["kfs"][0], S["kfs"][1], o[:0], o[:0])
    assert len(st) == 0 and x.shape == (0, 3)


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_shim_compiles_and_links_against_the_refstub(pkg, tmp_path, flags):
    """host/NewMapPoints.h compiles (-Wall -Werror, both error conventions) against the unchanged stand-ins of tests/cpp/refstub and
    links against libaos2 (the run needs the GPU: tests/test_triangulate_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "new_map_points_test.cpp"),
                           "-o", str(tmp_path / "new_map_points_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
