"""LocalMapping::KeyFrameCulling on the device (aos2_local_map_keyframe_culling, csrc/kf_culling.hip) against the plain-Python
restatement tests/keyframe_culling_ref.py: every status byte, every count, the bad-point list and its length equal, on the planted
cases and the seeded sweep of tests/keyframe_culling_cases.py; the same outputs whatever the rounds per enqueue; and the resident
graph untouched by the call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import keyframe_culling_cases as cases   # noqa: E402
import local_map_cases as lm_cases       # noqa: E402
import local_map_ref as lm_ref           # noqa: E402
from test_keyframe_culling_cpu import PLANTED, same, want   # noqa: E402

pytestmark = pytest.mark.gpu


def device(capi, c, rounds=0):
    """the case on a fresh handle -> (result, rounds the call ran)"""
    m = capi.LocalMap()
    m.set(c["g"])
    m.set_culling_view(c["v"])
    m.debug_culling_rounds(rounds)
    r = m.keyframe_culling(c["cand"], c["monocular"], c["bad_cap"])
    n = m.last_culling_rounds()
    m.close()
    return r, n


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, gpu, c):
    w = want(c)
    got, rounds = device(pkg.capi, c)
    same(got, w, c)
    if len(c["cand"]):   # culls + 1 rounds, or culls when the last candidate is the last cull
        assert rounds == w["n_culled"] + (w["status"][-1] != cases.CULLED), (c["name"], rounds)
    if c["name"] == "none_redundant":
        assert rounds == 1


@pytest.mark.parametrize("seed", cases.SWEEP_SEEDS)
def test_sweep(pkg, gpu, seed):
    c = cases.random_case(seed)
    same(device(pkg.capi, c)[0], want(c), c)


def test_outputs_do_not_depend_on_the_rounds_per_enqueue(pkg, gpu):
    c = next(c for c in PLANTED if c["name"] == "chain")
    w = want(c)
    runs = [device(pkg.capi, c, rounds) for rounds in (0, 1, 2)]
    for got, n in runs:
        same(got, w, c)
        assert n >= 4 and n == 5
    for got, _ in runs[1:]:
        for k in ("status", "n_mps", "n_redundant", "bad_points"):
            assert got[k].tobytes() == runs[0][0][k].tobytes(), k


def test_the_resident_graph_is_read_only(pkg, gpu):
    """two calls in a row give equal results (the overlay is rebuilt), aos2_local_map_get returns the same arrays before and after,
    and aos2_local_map_update on the same handle still equals its restatement"""
    capi = pkg.capi
    c = cases.random_case(cases.SWEEP_SEEDS[0])
    w = want(c)
    assert w["n_culled"] >= 2 and w["n_bad_points"] > 0
    g = c["g"]
    m = capi.LocalMap()
    m.set(g)
    m.set_culling_view(c["v"])
    before = m.graph()
    frames = lm_cases.random_frames(np.random.default_rng(5), g, 6, (40, 0, 25, 64, 3))
    n, mp = lm_cases.frames_arrays(frames, cap=64)
    nk = g["n_keyframes"]
    lm_want = lm_ref.update_batch(g, n, mp, g["n_points"], nk, np.full((6, nk), -1, np.int32), np.zeros(6, np.int32), np.full(6, -1, np.int32))

    def update_equals_the_restatement():
        got = m.update_host(n, mp, g["n_points"], nk)
        for k in ("mp", "local", "n_local", "local_kfs", "n_local_kfs", "ref_kf"):
            assert np.array_equal(got[k], lm_want[k]), k
    update_equals_the_restatement()
    first = m.keyframe_culling(c["cand"], c["monocular"])
    second = m.keyframe_culling(c["cand"], c["monocular"])
    same(first, w, c)
    same(second, w, c)
    after = m.graph()
    assert all(np.array_equal(before[k], after[k]) for k in before)
    update_equals_the_restatement()
    third = m.keyframe_culling(c["cand"], c["monocular"])   # (the update used the same scratch)
    same(third, w, c)
    m.close()
