"""MapPoint::UpdateNormalAndDepth on the device (aos2_local_map_update_normal_depth, csrc/normal_depth.hip) against the numpy
restatement tests/normal_depth_ref.py and against the host tap, BIT FOR BIT (floats as uint32, NaN against NaN aside): every planted
case -- observation lists of 0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65 and 257 entries, batches of 1, 63, 64, 65 and 257 points -- and
50 seeded random cases, each with the thetas waiting in LDS up to 64, 16 and 8 entries and in global scratch throughout; a batch
split into groups by the scratch bound; the graph after an aos2_local_map_apply on the device; calls of different sizes on one
handle; the device time."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import local_map_apply_cases as acases   # noqa: E402
import normal_depth_cases as cases       # noqa: E402
import normal_depth_ref as ref           # noqa: E402
from test_update_normal_depth_cpu import PLANTED, call_args, host, same, want   # noqa: E402

pytestmark = pytest.mark.gpu

# the longest list whose thetas wait in LDS: the default (64), two lower seams, none (every list in global scratch)
FORMS = {"lds": -1, "lds16": 16, "lds8": 8, "global": 0}


def handle(capi, c, form="lds", scratch=0):
    m = capi.LocalMap()
    m.set(c["g"])
    m.set_culling_view(c["v"])
    m.debug_limits(scratch, -1)
    m.debug_normal_depth(FORMS[form])
    return m


def device(capi, c, form="lds", scratch=0, **kw):
    """the case on a fresh handle -> (result, groups the batch ran in, device ms)"""
    m = handle(capi, c, form, scratch)
    a, k = call_args(c)
    r = m.update_normal_depth(*a, **dict(k, **kw))
    out = r, m.last_groups(), m.last_normal_depth_device_ms()
    m.close()
    return out


def same_bytes(a, b, name):
    assert set(a) == set(b)
    for k in a:
        if k != "guard":
            assert a[k].tobytes() == b[k].tobytes(), (name, k)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, gpu, c, form):
    w = want(c)
    got, groups, ms = device(pkg.capi, c, form)
    same(got, w, c["name"])
    same(got, host(pkg.capi, c), c["name"])
    if len(c["point"]):
        assert groups == 1 and ms > 0
    else:
        assert groups == 0 and ms == -1


@pytest.mark.parametrize("form", list(FORMS))
def test_random_cases(pkg, gpu, form):
    for seed in range(50):
        c = cases.random_case(seed)
        got = device(pkg.capi, c, form)[0]
        same(got, cases.want(c), c["name"])
        same(got, host(pkg.capi, c), c["name"])


def planned_groups(c, lds_terms, bound):
    """the plan of include/aos2.h: a list longer than the LDS form holds takes 4 bytes per observation of the scratch, and a group
    ends where the next list no longer fits the bound"""
    lens = np.diff(c["g"]["obs_off"])
    groups, used = 1, 0
    for p in c["point"]:
        n = int(lens[p]) if p < len(lens) else 0
        if n <= lds_terms:
            continue
        if used + n > bound // 4:
            groups, used = groups + 1, 0
        used += n
    return groups


@pytest.mark.parametrize("form", ["lds16", "global"])
def test_a_batch_split_into_groups_gives_the_same_outputs(pkg, gpu, form):
    c = next(c for c in PLANTED if c["name"] == "term_off/matching_and_not")
    w = want(c)
    whole, groups, _ = device(pkg.capi, c, form)
    assert groups == 1
    same(whole, w, c["name"])
    seen = set()
    for bound in (4 * 257, 4 * 257 + 3, 4 * 400, 4 * 600, 4 * 1000):   # (the longest list has 257 entries: one of it must fit)
        got, groups, _ = device(pkg.capi, c, form, scratch=bound)
        assert groups == planned_groups(c, FORMS[form], bound) > 1, (bound, groups)
        seen.add(groups)
        same(got, w, c["name"])
        same_bytes(got, whole, (form, bound))
    assert len(seen) >= 3


def test_the_call_reads_the_graph_that_apply_built_on_the_device(pkg, gpu):
    """a delta that appends a keyframe and a point and adds the keyframe to an old point's observers, applied on the device path: the
    results are the reference's on the post-delta graph"""
    capi = pkg.capi
    rng = np.random.RandomState(7)
    nk = 12
    octaves = [[(k + f) % 8 for f in range(3)] for k in range(nk)]
    obs = [[(k, (p + k) % 3) for k in range(p % 4, nk, 1 + p % 3)] for p in range(9)]
    g0, v0 = cases.build(octaves, obs)
    m0 = acases.to_model(g0, v0)
    m1 = copy.deepcopy(m0)
    m1["kfs"].append(dict(bad=0, feats=[(9, 5, 1.0, 0), (2, 7, 1.0, 0)], best=[], children=[], parent=-1, th=40.0, flags=0))
    m1["pts"].append(dict(bad=0, nobs=2, obs=[(3, 1), (nk, 0)]))
    m1["pts"][2]["obs"].append((nk, 1))
    m1["pts"][2]["nobs"] += 1
    g1, v1 = acases.to_arrays(m1)
    delta = acases.delta_between(m0, m1)
    centre = rng.uniform(-5, 5, (nk + 1, 3)).astype(np.float32)
    point, rk = np.array([2, 9, 9, 4], np.int32), np.array([nk, nk, 3, 1], np.int32)
    xyz = rng.uniform(-3, 3, (4, 3)).astype(np.float32)
    off = np.array([0, len(m1["pts"][2]["obs"]), 0, 2, 0], np.int32).cumsum().astype(np.int32)
    after = ref.update_normal_depth(g1, v1, point, xyz, rk, centre, cases.SCALE, ref.ROWS_TRACKING, off)
    assert list(after["status"]) == [ref.UPDATED] * 4 and after["n_terms"][1] == 2
    for form in FORMS:
        m = handle(capi, dict(g=g0, v=v0), form)
        before = m.update_normal_depth([2, 9], xyz[:2], [0, 0], centre[:nk], cases.SCALE)
        same(before, ref.update_normal_depth(g0, v0, [2, 9], xyz[:2], [0, 0], centre[:nk], cases.SCALE), "before/" + form)
        assert list(before["status"]) == [ref.UPDATED, ref.UNKNOWN]
        m.apply(delta)
        assert m.last_apply()["path"] == 1
        got = m.update_normal_depth(point, xyz, rk, centre, cases.SCALE, rows_form=ref.ROWS_TRACKING, term_off=off)
        same(got, after, "after/" + form)
        same(got, capi.LocalMap.update_normal_depth_host(g1, v1, point, xyz, rk, centre, cases.SCALE, rows_form=ref.ROWS_TRACKING,
                                                         term_off=off), "tap/" + form)
        m.close()


def test_calls_of_different_sizes_on_one_handle(pkg, gpu):
    """the staging is laid out again for every call: a large batch, a small one with other outputs, the large one again"""
    big = next(c for c in PLANTED if c["name"] == "batch/257")
    small = next(c for c in PLANTED if c["name"] == "specials/tracking")
    m = handle(pkg.capi, big)
    a, k = call_args(big)
    first = m.update_normal_depth(*a, **k)
    assert m.last_normal_depth_device_ms() > 0 and m.last_groups() == 1
    a2, k2 = call_args(small)
    second = m.update_normal_depth(*a2, **dict(k2, want=("status", "normal", "lower")))
    empty = m.update_normal_depth([], np.zeros((0, 3)), [], big["kf_center"], big["scale"])
    assert m.last_normal_depth_device_ms() == -1 and m.last_groups() == 0 and len(empty["status"]) == 0
    third = m.update_normal_depth(*a, **k)
    assert m.last_normal_depth_device_ms() > 0
    m.close()
    same(first, want(big), "first")
    same(second, {x: want(small)[x] for x in ("status", "normal", "lower")}, "second")
    same_bytes(first, third, "third")
