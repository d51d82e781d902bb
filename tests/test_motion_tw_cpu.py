"""The planner's motion checks without a device.  Three layers: the restatement (tests/motion_tw_ref.py) against independent
knowledge -- its sin / cos / atan2 against libm, a reconstructed path against the goal it was asked to reach and against the
length it claims; the library's host taps (aos2_debug_svc_*_host, aos2_debug_tw_math on the host: the routines of csrc/motion_tw.h
that the device kernels also run) against the restatement, bit for bit; and the conditions the seeded draws and the planted cases
have to meet for the GPU tests to mean what they say."""
import math
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_tw_ref as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AOS2_ERR_ARG, AOS2_ERR_CAPACITY = -1, -2


def ulps(got, want):
    """|got - want| in units of the spacing of doubles at `want`"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_restated_math_is_within_one_ulp_of_libm():
    x, ay, ax = M.math_samples()
    assert ulps([M.tw_sin(float(v)) for v in x], [math.sin(v) for v in x]).max() <= 1
    assert ulps([M.tw_cos(float(v)) for v in x], [math.cos(v) for v in x]).max() <= 1
    got = np.array([M.tw_atan2(float(a), float(b)) for a, b in zip(ay, ax)])
    want = np.array([math.atan2(a, b) for a, b in zip(ay, ax)])
    nz = want != 0
    assert ulps(got[nz], want[nz]).max() <= 1
    assert (got[~nz] == 0).all() and (np.signbit(got[~nz]) == np.signbit(want[~nz])).all()      # the signed zeros
    assert M.tw_sin(-0.0) == 0 and math.copysign(1, M.tw_sin(-0.0)) < 0 and M.tw_cos(0.0) == 1.0


def test_host_math_equals_the_restatement(pkg):
    x, ay, ax = M.math_samples()
    x = np.concatenate([x, [-1e4, 1e4, 9999.5, -7.48, 6.11, 0.0, -0.0, 1e300, np.inf, np.nan]])
    got = pkg.debug_tw_math(x, np.resize(ay, len(x)))
    assert got["sin"].tobytes() == np.array([M.tw_sin(float(v)) for v in x]).tobytes()
    assert got["cos"].tobytes() == np.array([M.tw_cos(float(v)) for v in x]).tobytes()
    got = pkg.debug_tw_math(ax, ay)
    assert got["atan2"].tobytes() == np.array([M.tw_atan2(float(a), float(b)) for a, b in zip(ay, ax)]).tobytes()
    with np.errstate(all="ignore"):
        assert got["sqrt"].tobytes() == np.sqrt(ax).tobytes() and got["quot"].tobytes() == (ay / ax).tobytes()


def test_a_reconstructed_path_ends_at_its_goal_and_has_the_length_it_claims():
    """The end: on a CPU prototype the worst planar end error over 40 motions was 2.4e-5 (the 3.1416 of the wraps and the float
    rounding of the tangent points).  The length: a segment of duration t is m - 1 steps of dd = t / (m - 1) <= dt.  The straight
    segment's chords add up to t.  On an arc of radius r a step turns by a = dd / r and its chord is 2 r sin(a / 2), which lies
    between dd (1 - a^2 / 24) and dd.  So the planar polyline is at most sum(t) and at least sum(t) (1 - (dt / r)^2 / 24), each
    within 1e-9 sum(t) for the rounding of some dozens of operations."""
    D = M.golden_draw()
    w, p = D.want, D.scene.p
    deficit = (p.dt / p.turn_radius) ** 2 / 24
    seen = 0
    for k in range(len(D.q1)):
        if not w["path_valid"][k]:
            continue
        Q = w["states"][w["offsets"][k]:w["offsets"][k + 1]]
        assert len(Q) == 1 + sum(int(m) - 1 for m in w["m"][k])
        assert math.hypot(Q[-1][0] - D.q2[k][0], Q[-1][1] - D.q2[k][1]) < 1e-3
        total = float(w["t"][k].sum())
        planar = sum(math.hypot(b[0] - a[0], b[1] - a[1]) for a, b in zip(Q, Q[1:]))
        assert total * (1 - deficit) - 1e-9 * total <= planar <= total * (1 + 1e-9)
        seen += 1
        if seen == 40:
            break
    assert seen == 40


def test_the_draw_meets_its_conditions():
    """37 of the 300 states of visibility_ref.golden_case() are valid starts; the 90 motions drawn from them have to take every
    outcome often enough, stop at several indices and win with most candidates"""
    assert len(M.golden_starts()) == 37
    D = M.golden_draw()
    w = D.want
    out = Counter(M.outcome(D))
    assert min(out["valid"], out["collision"], out["visibility"]) >= 15, out
    assert len(set(w["first_invalid"][w["first_invalid"] >= 0])) >= 4
    assert len(set(w["type"][w["type"] >= 0])) >= 5
    assert D.replaced <= 0.05 * len(D.q1)
    # the first and the last state of a motion as the one that stops it
    assert (w["first_invalid"] == 1).any() and (w["first_invalid"] == w["n_states"] - 1).any()
    assert M.sweep_draw().replaced <= 0.05 * 300
    sw = M.sweep_draw().want
    assert 30 <= sw["valid"].sum() <= 270 and len(set(sw["type"])) >= 5


def test_the_planted_motions_are_what_they_claim():
    D = M.planted_scene()
    w, p = D.want, D.scene.p
    at = {n: i for i, n in enumerate(D.names)}
    Q = lambda n: w["states"][w["offsets"][at[n]]:w["offsets"][at[n] + 1]]
    for t in range(8):                                                   # each of the eight candidates wins somewhere
        assert w["type"][at["type%d" % t]] == t and w["path_valid"][at["type%d" % t]]
    tot = [None if t is None else t[0] + t[1] + t[2] for t in M.candidates(*M.PLANTED_MOTIONS["tie"], p.turn_radius)]
    k = at["tie"]                                                        # bit-equal totals: the lowest candidate stays
    assert tot[1] == tot[7] == min(tot) and tot[0] > tot[1] and w["type"][k] == 1
    assert list(w["m"][k]) == [1, 5, 1] and w["t"][k][0] == 0 and w["t"][k][2] == 0 and w["n_states"][k] == 5   # t == 0: m == 1, no state
    assert (Q("tie")[1:, 2] == 0).all() and w["m"][k][1] > 1             # the middle segment: w == 0, the straight branch
    close = M.candidates(*M.PLANTED_MOTIONS["close"], p.turn_radius)     # all four opposite-turn candidates infeasible
    assert [c is None for c in close] == [False, False, True, True, True, True, False, False] and w["path_valid"][at["close"]]
    same = M.candidates(*M.PLANTED_MOTIONS["same"], p.turn_radius)       # q1 == q2: the same-turn candidates are NaN and never win
    assert all(math.isnan(sum(same[i])) for i in (0, 1, 6, 7)) and w["type"][at["same"]] == 2 and w["n_states"][at["same"]] == 1
    k = at["none"]                                                       # no candidate at all: Q = {q1}, costs 0, not valid
    assert (w["path_valid"][k], w["type"][k], w["n_states"][k], w["valid"][k], w["first_invalid"][k]) == (0, -1, 1, 0, -1)
    assert w["cost_length"][k] == 0 and w["cost_camera"][k] == 0
    h = Q("heading5")[:, 2]                                              # a heading that crosses 5: rejected by the bounds test
    assert h[1] < 5 < h[-1] and w["first_invalid"][at["heading5"]] == int(np.nonzero(h > 5)[0][0])
    y = Q("y65")[:, 1]                                                   # y beyond 6.5, x's maximum; 6.5 itself passes
    assert w["first_invalid"][at["y65"]] == int(np.nonzero(y > 6.5)[0][0]) >= 1
    far = math.sqrt(min(D.scene.nearest2(q) for n in ("heading5", "y65") for q in Q(n)))
    assert far > 10                                                      # (not by an obstacle)


def test_the_planted_states_are_what_they_claim():
    D = M.planted_states()
    w, S = D.want, D.scene
    thr, free, cnt = S.thr, w["collision_free"].astype(bool), w["count"]
    assert S.p.robot_r + S.obs_r == 0.5 and math.sqrt(S.nearest2(D.states[D.on])) == 0.5 and not free[D.on]    # <= rejects
    assert math.sqrt(S.nearest2(D.states[D.off])) > 0.5 and free[D.off] and w["valid"][D.off]
    assert cnt[D.eq] == thr and free[D.eq] and not w["valid"][D.eq]                                            # > rejects
    assert (~free & (cnt > thr)).any() and (free & (cnt <= thr)).any() and (~free & (cnt <= thr)).any() and w["valid"].any()
    H = M.heuristic_scene()
    hw = H.valid(D.states)
    d2 = (D.states[:, 0] - H.p.start[0]) ** 2 + (D.states[:, 1] - H.p.start[1]) ** 2
    low = hw["collision_free"].astype(bool) & (hw["count"] <= thr)
    assert (low & (d2 < 4) & (hw["valid"] == 0)).any() and (low & (d2 > 4) & (hw["valid"] == 1)).any()


def test_host_taps_equal_the_restatement(pkg):
    for D in (M.golden_draw(), M.planted_scene()):
        S = D.scene.load(pkg)
        M.same(S.motions(D.q1, D.q2, host=True), D.want)
        got = S.valid(D.want["states"], host=True)
        want = D.scene.valid(D.want["states"])
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)
    D = M.sweep_draw()
    M.same(D.scene.load(pkg).motions(D.q1[:64], D.q2[:64], host=True), D.want, 64)
    P = M.planted_states()
    for scene in (P.scene, M.heuristic_scene()):
        got, want = scene.load(pkg).valid(P.states, host=True), scene.valid(P.states)
        assert all(got[k].tobytes() == want[k].tobytes() for k in want)


def test_host_tap_outputs_are_optional_and_the_capacity_is_checked(pkg):
    D = M.golden_draw()
    S = D.scene.load(pkg)
    total = int(D.want["offsets"][-1])
    M.same(S.motions(D.q1, D.q2, capacity=total, host=True), D.want)
    with pytest.raises(pkg.AosError) as e:
        S.motions(D.q1, D.q2, capacity=total - 1, host=True)
    assert e.value.code == AOS2_ERR_CAPACITY and e.value.needed == total
    bare = S.motions(D.q1, D.q2, states=False, host=True)
    assert "states" not in bare and bare["cost_camera"].tobytes() == D.want["cost_camera"].tobytes()
    none = S.motions(np.zeros((0, 3)), np.zeros((0, 3)), host=True)
    assert len(none["valid"]) == 0 and list(none["offsets"]) == [0] and len(none["states"]) == 0
    assert len(S.valid(np.zeros((0, 3)), host=True)["valid"]) == 0


@pytest.mark.parametrize("host", [True, False])
def test_arguments_are_checked_before_a_device_is_looked_for(pkg, host):
    """also the device calls: a bad argument is reported without a GPU"""
    S = M.golden_scene().load(pkg, device=0)
    ok = np.array([[1.0, 1.0, 0.0]])
    for bad in ([np.nan, 0, 0], [0, np.inf, 0], [0, 0, np.nan], [0, 0, 1.0001e4], [0, 0, -1.0001e4], [-np.inf, 0, 0]):
        for a, b in ((np.array([bad], np.float64), ok), (ok, np.array([bad], np.float64))):
            with pytest.raises(pkg.AosError) as e:
                S.motions(a, b, host=host)
            assert e.value.code == AOS2_ERR_ARG
        with pytest.raises(pkg.AosError) as e:
            S.valid(np.array([bad], np.float64), host=host)
        assert e.value.code == AOS2_ERR_ARG
    if host:   # a segment of more than AOS2_SVC_MAX_SEGMENT_STATES states (the device finds it on the device: tests/test_motion_tw_gpu.py)
        with pytest.raises(pkg.AosError) as e:
            S.motions(ok, np.array([[1e6, 1.0, 0.0]]), host=True)
        assert e.value.code == AOS2_ERR_ARG
    p = M.Params().to_capi(pkg)
    for field, v in (("dt", 0.0), ("turn_radius", -1.0), ("robot_r", np.nan), ("max_x", np.inf)):
        q = M.Params().to_capi(pkg)
        setattr(q, field, v)
        with pytest.raises(pkg.AosError) as e:
            S.set_params(q)
        assert e.value.code == AOS2_ERR_ARG
    S.set_params(p)
    with pytest.raises(pkg.AosError) as e:
        S.set_obstacles([[0.0, np.nan]])
    assert e.value.code == AOS2_ERR_ARG
    d = pkg.StateValidChecker.params_default()
    assert (d.turn_radius, d.robot_r, d.dt, d.min_x, d.max_x, d.min_y, d.max_y) == (0.25, 0.4, 0.3, -1.15, 6.5, -5, 5)
    assert (d.heuristic, d.max_dist_heuristic, d.feature_threshold, list(d.start)) == (0, 2, -1, [0, 0, 0])


# ---------------------------------------------------------------------------------------- the host class
@pytest.mark.parametrize("flags", ([], ["-DAOS2_HOST_EXCEPTIONS"]))
def test_host_class_compiles_and_links(pkg, tmp_path, flags):
    """host/StateValidChecker.h against tests/cpp/refstub/state_valid_checker_stub.h, in both error conventions (it runs on the GPU:
    tests/test_state_valid_checker_class_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "state_valid_checker_test.cpp"), "-o", str(tmp_path / "state_valid_checker_test"),
                           "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
