"""The planner's visibility count (camera::countVisible, src/camera.cc:135-198) without a GPU: the Python restatement the GPU tests
compare against (tests/visibility_ref.py) checked against independent knowledge (a float64 vectorised geometry, a brute-force
advance, a plain loop for the motion cost), the conditions the shared generator has to meet, the library's host tap
(aos2_debug_visibility_*host: the routines of csrc/visibility.h on one core) against the restatement bit for bit, the argument
checks, and the host class's compile + link."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visibility_ref as R  # noqa: E402

SEED = 5
SHAPES = (0, 1, 63, 64, 65, 130)


def same(got, case, k=None):
    """every output of a count call against the restatement's first k states, bit for bit"""
    k = len(case.states) if k is None else k
    assert (got["count"] == case.count[:k]).all()
    assert got["sum"].tobytes() == case.sum[:k].tobytes()
    assert got["mask"].tobytes() == case.mask[:k].tobytes()


# ---------------------------------------------------------------------------------------- the restatement against independent knowledge
def geometry_f64(cam, m, states):
    """the decision of every (state, point) from float64 geometry, and whether a gate quantity is within 1e-4 relative of a threshold"""
    T_sw, T_bc = np.array(cam.T_sw, np.float64).reshape(4, 4), np.array(cam.T_bc, np.float64).reshape(4, 4)
    P = np.concatenate([m.xyz.astype(np.float64), np.ones((m.n, 1))], 1)
    dec, close = np.zeros((len(states), m.n), bool), np.zeros((len(states), m.n), bool)
    g = {k: float(getattr(cam, k)) for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "min_dist", "max_dist")}
    for k, (x, y, t) in enumerate(states.astype(np.float64)):
        T_wb = np.array([[np.cos(t), -np.sin(t), 0, x], [np.sin(t), np.cos(t), 0, y], [0, 0, 1, 0], [0, 0, 0, 1]])
        T_sc = T_sw @ T_wb @ T_bc
        Pc = P @ np.linalg.inv(T_sc).T
        with np.errstate(all="ignore"):
            u, v = g["fx"] * Pc[:, 0] / Pc[:, 2] + g["cx"], g["fy"] * Pc[:, 1] / Pc[:, 2] + g["cy"]
            dist = np.linalg.norm(Pc[:, :3], axis=1)
            theta = np.arctan2(P[:, 0] - T_sc[0, 3], P[:, 2] - T_sc[2, 3])
            gates = [(Pc[:, 2], 0.05, np.inf), (u, g["min_x"], g["max_x"]), (v, g["min_y"], g["max_y"]), (dist, g["min_dist"], g["max_dist"]),
                     (dist, m.min_range.astype(np.float64), m.max_range.astype(np.float64)),
                     (theta, m.lower.astype(np.float64), m.upper.astype(np.float64))]
            ok = np.ones(m.n, bool)
            for q, lo, hi in gates:
                ok &= ~(q < lo) & ~(q > hi)
                for thr in (lo, hi):
                    close[k] |= np.isfinite(thr) & (np.abs(q - thr) <= 1e-4 * np.maximum(np.abs(thr), 1e-3))
        dec[k] = ok
    return dec, close


@pytest.mark.parametrize("which", ("random", "golden"))
def test_restatement_decides_like_float64_geometry(which):
    case = R.random_case(SEED, 130) if which == "random" else R.golden_case()
    k = len(case.states) if which == "random" else 60
    dec, close = geometry_f64(case.cam, case.map, case.states[:k])
    got = case.codes[:k] == R.OK
    print(which, "pairs", dec.size, "visible", int(dec.sum()), "close to a threshold", int(close.sum()))
    assert (got == dec)[~close].all() and close.mean() < 0.01 and dec.sum() > 100


def test_mask_count_and_sum_agree_inside_the_restatement():
    case = R.random_case(SEED, 130)
    for s in range(len(case.states)):
        bits = np.unpackbits(case.mask[s].view(np.uint8), bitorder="little")[: case.map.n].astype(bool)
        assert (bits == (case.codes[s] == R.OK)).all()
        assert abs(float(case.sum[s]) - float(case.map.ratio[bits].astype(np.float64).sum())) <= 1e-4
        assert case.count[s] == int(np.floor(float(case.sum[s]) + 0.5))      # (the sums are positive)


def test_motion_cost_against_a_plain_loop_and_advance_by_brute_force():
    case = R.random_case(SEED, 130)
    thr = int(np.median(case.count))
    motions, counts = R.motions_of(case)
    want = [0.0, 0.0] + [sum(1e4 if c < thr else 1.0 / c for c in cs[1:-1]) for cs in counts[2:]]
    got = [float(R.motion_cost(cs, thr)) for cs in counts]
    assert got == want and got[3] > got[2] > 0
    inner = counts[3][1:-1]
    assert (inner < thr).any() and (inner >= thr).any()                      # both branches of the term
    assert R.motion_cost([5, 0, 5], 0) == np.inf
    for name, (idx, want_i) in R.trajectories_of(case, thr).items():
        ok = case.count[idx] > thr
        brute = max([i for i in range(len(idx)) if ok[: i + 1].all()], default=-1)
        assert want_i == brute, name
    t = R.trajectories_of(case, thr)
    assert t["first"][1] == -1 and t["middle"][1] == 4 and t["late"][1] == 65 and t["absent"][1] == 69


def test_round_is_half_away_from_zero():
    F = np.float32
    assert [R.round_half_away(F(v)) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997, 8388609.0, 16777216.0)] == \
        [1, 2, 3, -1, -3, 0, 8388609, 16777216]
    assert R.round_half_away(F(3e9)) == R.INT32_MIN and R.round_half_away(F(np.nan)) == R.INT32_MIN


# ---------------------------------------------------------------------------------------- the generator and the planted cases
def test_origin_state_is_the_identity():
    """T_sw * T_bc = I in float, so state (0, 0, 0) makes T_sc = T_cs = I exactly: the planted points rest on it"""
    cs, sc03, sc23 = R.state_from_xyt(0, 0, 0, R.camera_exact())
    assert [float(v) for v in cs] == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and sc03 == 0 and sc23 == 0


def test_planted_points_leave_by_the_planted_return():
    P = R.planted_cases()
    want = [code for _, code in R.PLANTED]
    assert list(P["returns"].codes[0]) == want
    assert set(want) == set(range(12)) and want.count(R.OK) == 10            # every return, and a point ON every threshold
    assert list(P["depth_on"].codes[0]) == [R.OK, R.DEPTH]
    assert float(P["big_first"].sum[0]) == 16777216.0 and P["big_first"].count[0] == 16777216
    assert float(P["big_last"].sum[0]) == 16777280.0
    assert int(np.unpackbits(P["big_first"].mask[0].view(np.uint8)).sum()) == 65
    assert (P["half"].sum[0], P["half"].count[0]) == (0.5, 1)
    assert (P["two_and_half"].sum[0], P["two_and_half"].count[0]) == (2.5, 3)


def test_redraws_are_rare():
    """re-draws stay under 1 % of the points drawn, over the cases of this file (a share of a single small map would be decided by
    one point: the 64-point map has one re-draw, a max_range two ulps from its point's distance)"""
    cases = [R.random_case(SEED, n) for n in SHAPES]
    drawn, redrawn = sum(c.drawn for c in cases), sum(c.redrawn for c in cases)
    print("drawn", drawn, "redrawn", redrawn, [(c.map.n, c.redrawn) for c in cases])
    assert redrawn < 0.01 * drawn


@pytest.mark.parametrize("n", SHAPES[1:])
def test_generator_conditions(n):
    """no pair of a case sits on a rounding boundary, and no comparison below is vacuous"""
    case = R.random_case(SEED, n)
    vis = (case.codes == R.OK).sum(1)
    print("n", n, "visible per state: max", vis.max(), "states that see something", int((vis > 0).sum()))
    assert not R.near_pairs(case.cam, case.map, case.states).any()
    if n >= 63:
        assert (vis > 0).sum() >= 30 and vis.max() >= 3
    if n >= 130:
        assert set(np.unique(case.codes)) == set(range(12))                 # every return of isInFrustum is taken


def test_golden_map_conditions():
    """the reference's planner map (2681 points): fewer than 1 % of the states replaced, and at least 10 % of them on each side of
    both thresholds in use (20 and 40)"""
    case = R.golden_case()
    ns = len(case.states)
    print("replaced", case.replaced, "of", ns, "; > 20:", int((case.count > 20).sum()), "> 40:", int((case.count > 40).sum()),
          "median", float(np.median(case.count)), "max", int(case.count.max()))
    assert case.map.n == 2681 and ns == 300 and case.replaced < 0.01 * ns
    for thr in (20, 40):
        assert (case.count > thr).sum() >= 0.1 * ns and (case.count <= thr).sum() >= 0.1 * ns
    rows = case.map.rows()
    assert R.count_visible(case.cam, rows, R.state_from_xyt(0, 0, 0, case.cam), case.map.n)[0] > 500   # most of the map from the origin


# ---------------------------------------------------------------------------------------- the host tap against the restatement
@pytest.mark.parametrize("n", SHAPES)
def test_host_tap_equals_the_restatement(pkg, n):
    case = R.random_case(SEED, n)
    V = case.load(pkg)
    same(V.count(case.states, host=True), case)
    same(V.count(case.states[:65], host=True), case, 65)
    same(V.count_poses(case.poses(), host=True), case)
    only = V.count(case.states, sum=False, mask=False, host=True)
    assert only["sum"] is None and only["mask"] is None and (only["count"] == case.count).all()


def test_host_tap_on_the_planted_cases(pkg):
    for name, case in R.planted_cases().items():
        same(case.load(pkg).count(case.states, host=True), case)


def test_host_tap_on_the_golden_map(pkg):
    case = R.golden_case()
    same(case.load(pkg).count(case.states, host=True), case)


def test_host_tap_motion_costs_and_advance(pkg):
    case = R.random_case(SEED, 130)
    V = case.load(pkg)
    thr = int(np.median(case.count))
    motions, counts = R.motions_of(case)
    want = np.array([R.motion_cost(c, thr) for c in counts], np.float64)
    assert V.motion_costs(motions, thr, host=True).tobytes() == want.tobytes()
    cam = case.cam.to_capi(pkg)
    cam.feature_threshold = thr                                               # thres < 0: the camera's threshold
    V.set_camera(cam)
    assert V.motion_costs(motions, -1, host=True).tobytes() == want.tobytes()
    assert V.motion_costs(motions, -7, host=True).tobytes() == want.tobytes()
    assert V.motion_costs([case.states[:3]], 0, host=True)[0] == R.motion_cost(case.count[:3], 0)
    for name, (idx, want_i) in R.trajectories_of(case, thr).items():
        assert V.advance(case.states[idx], thr, host=True) == want_i, name
        assert V.advance(case.states[idx], -1, host=True) == want_i, name
    assert V.advance(np.zeros((0, 3)), thr, host=True) == -1


def test_set_map_twice(pkg):
    big, small = R.random_case(SEED, 130), R.random_case(SEED, 63)
    V = big.load(pkg)
    same(V.count(big.states, host=True), big)
    V.set_map(*small.map.args())
    assert V.map_size() == 63
    same(V.count(small.states, host=True), small)


# ---------------------------------------------------------------------------------------- argument checks
def test_camera_defaults(pkg):
    for which, ref in ((0, R.camera_with_map()), (1, R.camera_plain())):
        c = pkg.Visibility.camera_default(which)
        for k in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y", "max_dist", "min_dist"):
            assert np.float32(getattr(c, k)) == getattr(ref, k), k
        assert c.feature_threshold == 20 and list(c.T_sw) == [float(v) for v in ref.T_sw] and list(c.T_bc) == [float(v) for v in ref.T_bc]
    with pytest.raises(pkg.AosError):
        pkg.Visibility.camera_default(2)


def test_refusals(pkg):
    E = pkg.capi.AOS2_ERR_ARG
    case = R.random_case(SEED, 63)
    V = case.load(pkg)
    L, h = V.L, V.h
    st = np.ascontiguousarray(case.states[:4])
    cnt = np.full(4, -9, np.int32)
    cost = np.full(2, -9.0)
    idx = np.full(1, -9, np.int32)
    p = pkg.capi._p
    for host in (True, False):      # the checks run before a device is looked for
        count = L.aos2_debug_visibility_host if host else L.aos2_vis_count
        poses = L.aos2_debug_visibility_poses_host if host else L.aos2_vis_count_poses
        costs = L.aos2_debug_visibility_motion_costs_host if host else L.aos2_vis_motion_costs
        adv = L.aos2_debug_visibility_advance_host if host else L.aos2_vis_advance
        assert count(None, 4, p(st), p(cnt), None, None) == E
        assert count(h, -1, p(st), p(cnt), None, None) == E
        assert count(h, 4, None, p(cnt), None, None) == E
        assert count(h, 4, p(st), None, None, None) == E
        assert poses(h, 4, None, p(cnt), None, None) == E
        assert count(h, 0, None, None, None, None) == 0                      # no states: nothing to do
        for off in ([0, 2, 2], [0, 3, 2], [1, 2, 4]):                        # an empty motion, descending offsets, a start that is not 0
            assert costs(h, 2, p(np.array(off, np.int32)), p(st), 5, p(cost)) == E
        assert costs(h, 2, None, p(st), 5, p(cost)) == E
        assert costs(h, 2, p(np.array([0, 2, 4], np.int32)), None, 5, p(cost)) == E
        assert costs(h, 2, p(np.array([0, 2, 4], np.int32)), p(st), 5, None) == E
        assert costs(h, -1, p(np.array([0], np.int32)), p(st), 5, p(cost)) == E
        assert costs(h, 0, p(np.array([0], np.int32)), None, 5, None) == 0
        assert adv(h, 4, p(st), 5, None) == E and adv(h, -1, p(st), 5, idx.ctypes.data_as(pkg.capi.C.POINTER(pkg.capi.C.c_int32))) == E
        assert adv(h, 4, None, 5, idx.ctypes.data_as(pkg.capi.C.POINTER(pkg.capi.C.c_int32))) == E
    assert (cnt == -9).all() and (cost == -9).all() and (idx == -9).all()     # a refusal writes nothing
    # sizes 1 and 2 need no device either: their cost is 0
    assert list(V.motion_costs([case.states[:1], case.states[1:3]], 5)) == [0.0, 0.0]
    assert L.aos2_vis_set_map(h, -1, *[None] * 6) == E and L.aos2_vis_set_map(h, 3, *[None] * 6) == E
    assert L.aos2_vis_set_map(h, 0, *[None] * 6) == 0 and V.map_size() == 0   # an empty map is legal
    assert (V.count(case.states, host=True)["count"] == 0).all()
    for field, bad in (("fx", np.inf), ("min_dist", np.nan), ("max_x", -np.inf)):
        cam = case.cam.to_capi(pkg)
        setattr(cam, field, bad)
        with pytest.raises(pkg.AosError) as e:
            V.set_camera(cam)
        assert e.value.code == E
    cam = case.cam.to_capi(pkg)
    cam.T_bc[7] = np.nan
    with pytest.raises(pkg.AosError):
        V.set_camera(cam)
    assert L.aos2_vis_set_camera(h, None) == E and L.aos2_vis_create(0, None) == E


# ---------------------------------------------------------------------------------------- the host class
@pytest.mark.parametrize("flags", ([], ["-DAOS2_HOST_EXCEPTIONS"]))
def test_host_class_compiles_and_links(pkg, tmp_path, flags):
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "camera_test.cpp"), "-o", str(tmp_path / "camera_test"),
                           "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
