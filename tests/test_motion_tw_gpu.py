"""The planner's motion checks on the device (csrc/motion_tw.hip: aos2_svc_motions / aos2_svc_valid) against the literal restatement
(tests/motion_tw_ref.py), exact in every output: path validity and type, the three durations and segment counts, the state counts,
the verdicts and first invalid indices, the bits of both costs, the offsets and every state.  The shapes sit around the kernels'
block sizes (8 lanes per motion and 32 motions per workgroup of the path kernel, 256 motions per round of the scan, 4
per workgroup of the verdict kernel; 64 states and 1024 staged obstacles per collision workgroup); the planted cases take every branch the header keeps."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_tw_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu
AOS2_ERR_ARG, AOS2_ERR_CAPACITY = -1, -2
OBS_TILE, STATE_TILE = 1024, 64             # what aos2_svc_collide_tile reports (asserted below)
MOTIONS = (0, 1, 7, 8, 9, 63, 64, 65, 300)
OBSTACLES = (0, 1, 63, 64, 65, OBS_TILE + 1)


def same_valid(got, want):
    assert all(got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes() for k in want)


def test_the_shapes_are_the_kernels_block_sizes(pkg, gpu):
    assert pkg.StateValidChecker.collide_tile() == (OBS_TILE, STATE_TILE)


def test_device_math_equals_the_hosts(pkg, gpu):
    """sin, cos, atan2 of csrc/motion_tw.h, and the device's sqrt and division: the same bits as on the host"""
    x, ay, ax = M.math_samples()
    x = np.concatenate([x, [-1e4, 1e4, 9999.5, -7.48, 6.11, 0.0, -0.0, 1e300, np.inf, np.nan]])
    for a, b in ((x, np.resize(ay, len(x))), (ax, ay), (np.abs(ax) * 3.7, ay)):
        host, dev = pkg.debug_tw_math(a, b), pkg.debug_tw_math(a, b, device=gpu)
        for k in host:
            assert dev[k].tobytes() == host[k].tobytes(), k


def test_every_motion_count(pkg, gpu):
    D = M.sweep_draw()
    S = D.scene.load(pkg, gpu)
    for nm in MOTIONS:
        M.same(S.motions(D.q1[:nm], D.q2[:nm]), D.want, nm)       # (also: call after call on one handle)
    assert S.last_device_ms() > 0
    M.same(S.motions(D.q1, D.q2), D.want)
    bare = S.motions(D.q1, D.q2, states=False)
    assert "states" not in bare and all(bare[k].tobytes() == D.want[k].tobytes() for k in bare)


@pytest.mark.parametrize("n", OBSTACLES)
def test_every_obstacle_count(pkg, gpu, n):
    D = M.sweep_draw()
    scene, want = M.with_obstacles(D, n)
    S = scene.load(pkg, gpu)
    M.same(S.motions(D.q1[:64], D.q2[:64]), want)
    v = scene.valid(want["states"])
    same_valid(S.valid(want["states"]), v)
    if n == 0:
        assert v["collision_free"].all()       # before the bounds test
    else:
        assert 0 < v["collision_free"].sum() < len(v["collision_free"])


def test_visibility_maps(pkg, gpu):
    """no point at all, and the reference's own planner map with its obstacles (130 points: every other test here)"""
    D = M.sweep_draw()
    scene, want = M.with_map(D, M.empty_map())
    M.same(scene.load(pkg, gpu).motions(D.q1[:64], D.q2[:64]), want)
    assert not want["valid"].any()
    G = M.golden_draw()
    S = G.scene.load(pkg, gpu)
    M.same(S.motions(G.q1, G.q2), G.want)
    same_valid(S.valid(G.want["states"]), G.scene.valid(G.want["states"]))


def test_valid_on_300_states(pkg, gpu):
    D = M.sweep_draw()
    st = D.want["states"][:300]
    want = D.scene.valid(st)
    S = D.scene.load(pkg, gpu)
    same_valid(S.valid(st), want)
    assert 0 < want["valid"].sum() < 300 and S.last_device_ms() > 0
    same_valid(S.valid(st[:1]), {k: v[:1] for k, v in want.items()})
    assert len(S.valid(np.zeros((0, 3)))["valid"]) == 0


def test_planted_motions(pkg, gpu):
    """what tests/test_motion_tw_cpu.py asserts them to be: each candidate winning, the tie, q1 == q2, infeasible candidates, no
    path, t == 0, the straight branch, the heading beyond 5 and y beyond 6.5"""
    D = M.planted_scene()
    S = D.scene.load(pkg, gpu)
    M.same(S.motions(D.q1, D.q2), D.want)
    for k in range(len(D.q1)):                # one at a time: a motion without a path alone, a single state alone
        one = S.motions(D.q1[k:k + 1], D.q2[k:k + 1])
        assert one["type"][0] == D.want["type"][k] and one["cost_length"].tobytes() == D.want["cost_length"][k:k + 1].tobytes()
        assert one["states"].tobytes() == D.want["states"][D.want["offsets"][k]:D.want["offsets"][k + 1]].tobytes()


def test_planted_states(pkg, gpu):
    """the obstacle exactly robot_r + obs_r away, count == threshold, each way of being invalid, the heuristic mode on both sides"""
    P = M.planted_states()
    for scene in (P.scene, M.heuristic_scene()):
        same_valid(scene.load(pkg, gpu).valid(P.states), scene.valid(P.states))


def test_states_capacity(pkg, gpu):
    D = M.golden_draw()
    S = D.scene.load(pkg, gpu)
    total = int(D.want["offsets"][-1])
    M.same(S.motions(D.q1, D.q2, capacity=total), D.want)
    with pytest.raises(pkg.AosError) as e:
        S.motions(D.q1, D.q2, capacity=total - 1)
    assert e.value.code == AOS2_ERR_CAPACITY and e.value.needed == total
    M.same(S.motions(D.q1, D.q2), D.want)                     # the handle goes on after the refusal
    with pytest.raises(pkg.AosError) as e:                     # a segment of more states than a call takes
        S.motions(D.q1[:3], np.array([D.q2[0], [1e6, 1.0, 0.0], D.q2[2]]))
    assert e.value.code == AOS2_ERR_ARG
    M.same(S.motions(D.q1[:9], D.q2[:9]), D.want, 9)


def test_set_obstacles_twice_on_one_handle(pkg, gpu):
    """larger, then smaller: nothing of the first set is left in the second one's answer"""
    D = M.sweep_draw()
    big, want_big = M.with_obstacles(D, OBS_TILE + 1)
    small, want_small = M.with_obstacles(D, 63)
    S = big.load(pkg, gpu)
    M.same(S.motions(D.q1[:64], D.q2[:64]), want_big)
    S.set_obstacles(small.obs, small.obs_r)
    M.same(S.motions(D.q1[:64], D.q2[:64]), want_small)
    S.set_obstacles(big.obs, big.obs_r)
    M.same(S.motions(D.q1[:64], D.q2[:64]), want_big)
    assert want_big["valid"].tobytes() != want_small["valid"].tobytes() or want_big["first_invalid"].tobytes() != want_small["first_invalid"].tobytes()
