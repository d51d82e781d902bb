"""The planner's visibility count on the device (csrc/visibility.hip: aos2_vis_count / _count_poses / _motion_costs / _advance)
against the literal restatement of camera::countVisible (tests/visibility_ref.py), exact in every output: the mask words, the bits of
the float sum, the counts, the cost doubles and the indices.  The shapes sit around the kernels' block sizes (64 points per mask
word, the points of a gate workgroup, the states of its tile, 64 states per round of the advance wave); the planted cases take
every return of isInFrustum, sit ON every threshold and fix the order of the sum and the rounding."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import visibility_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 5
GATE_POINTS, GATE_STATES = 512, 32           # what aos2_vis_gate_tile reports (asserted below)
POINTS = (0, 1, 63, 64, 65, 130, GATE_POINTS + 1)
STATES = (1, 63, 65, 300, GATE_STATES + 1)


def same(got, case, k=None):
    k = len(case.states) if k is None else k
    assert (got["count"] == case.count[:k]).all()
    assert got["sum"].tobytes() == case.sum[:k].tobytes()
    assert got["mask"].tobytes() == case.mask[:k].tobytes()


def test_the_shapes_are_the_kernels_block_sizes(pkg, gpu):
    assert pkg.Visibility.gate_tile() == (GATE_POINTS, GATE_STATES)


@pytest.mark.parametrize("n", POINTS)
def test_device_equals_the_restatement(pkg, gpu, n):
    case = R.random_case(SEED, n)
    V = case.load(pkg, gpu)
    for k in STATES:
        same(V.count(case.states[:k]), case, k)
    assert V.last_device_ms() > 0
    if n >= 63:
        assert (case.count > 0).sum() >= 30


def test_planted_returns_thresholds_sum_order_and_rounding(pkg, gpu):
    P = R.planted_cases()
    for name, case in P.items():
        same(case.load(pkg, gpu).count(case.states), case)
    got = P["big_first"].load(pkg, gpu).count(R.ORIGIN)          # a chunked or tree sum gives 16777280
    assert got["sum"][0] == np.float32(16777216.0) and got["count"][0] == 16777216
    assert P["big_last"].load(pkg, gpu).count(R.ORIGIN)["sum"][0] == np.float32(16777280.0)
    assert P["half"].load(pkg, gpu).count(R.ORIGIN)["count"][0] == 1          # rintf gives 0
    assert P["two_and_half"].load(pkg, gpu).count(R.ORIGIN)["count"][0] == 3  # rintf gives 2


def test_golden_planner_map(pkg, gpu):
    """the reference's own planner map, 300 states: every output; the poses form; the optional outputs absent; a call per state"""
    case = R.golden_case()
    V = case.load(pkg, gpu)
    same(V.count(case.states), case)
    same(V.count_poses(case.poses()), case)
    only = V.count(case.states, sum=False, mask=False)
    assert only["sum"] is None and only["mask"] is None and (only["count"] == case.count).all()
    singles = [V.count(case.states[i:i + 1]) for i in range(len(case.states))]
    same({k: np.concatenate([s[k] for s in singles]) for k in ("count", "sum", "mask")}, case)


def test_motion_costs_in_one_call(pkg, gpu):
    case = R.random_case(SEED, 130)
    V = case.load(pkg, gpu)
    thr = int(np.median(case.count))
    motions, counts = R.motions_of(case, (1, 2, 3, 40))
    want = np.array([R.motion_cost(c, thr) for c in counts], np.float64)
    assert want[0] == 0 and want[1] == 0 and want[3] > want[2] > 0
    assert V.motion_costs(motions, thr).tobytes() == want.tobytes()
    cam = case.cam.to_capi(pkg)
    cam.feature_threshold = thr
    V.set_camera(cam)
    assert V.motion_costs(motions, -1).tobytes() == want.tobytes()
    assert V.motion_costs(motions[2:3], 0)[0] == R.motion_cost(counts[2], 0)
    many = [case.states[i:i + 3] for i in range(0, 297)]      # more motions than a workgroup has lanes
    want = np.array([R.motion_cost(case.count[i:i + 3], thr) for i in range(0, 297)], np.float64)
    assert V.motion_costs(many, thr).tobytes() == want.tobytes()


def test_advance(pkg, gpu):
    case = R.random_case(SEED, 130)
    V = case.load(pkg, gpu)
    thr = int(np.median(case.count))
    t = R.trajectories_of(case, thr)
    assert (t["first"][1], t["middle"][1], t["late"][1], t["absent"][1]) == (-1, 4, 65, 69)
    for name, (idx, want) in t.items():
        assert V.advance(case.states[idx], thr) == want, name
    cam = case.cam.to_capi(pkg)
    cam.feature_threshold = thr
    V.set_camera(cam)
    for name, (idx, want) in t.items():
        assert V.advance(case.states[idx], -1) == want, name


def test_set_map_twice_on_one_handle(pkg, gpu):
    """larger, then smaller: nothing of the first map is left in the second one's answer"""
    big, small = R.random_case(SEED, GATE_POINTS + 1), R.random_case(SEED, 63)
    V = big.load(pkg, gpu)
    same(V.count(big.states), big)
    V.set_map(*small.map.args())
    same(V.count(small.states), small)
    V.set_map(*big.map.args())
    same(V.count(big.states[:GATE_STATES + 1]), big, GATE_STATES + 1)
