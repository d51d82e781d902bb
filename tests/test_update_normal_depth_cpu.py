"""MapPoint::UpdateNormalAndDepth on the host (aos2_debug_update_normal_depth_host: the arithmetic of csrc/normal_depth.h that the
device kernel runs, serially) against the numpy restatement tests/normal_depth_ref.py, BIT FOR BIT (floats compared as uint32; two
NaNs count as equal whatever their payload): every planted case of tests/normal_depth_cases.py and 50 seeded random cases, with the
output arrays preset so that what a point that is not updated leaves behind is checked too; the restatement itself on a
hand-computed example; the host side under the address and undefined-behaviour sanitizers; and every AOS2_ERR_ARG of the new entry
points.  No GPU."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import normal_depth_cases as cases   # noqa: E402
import normal_depth_ref as ref       # noqa: E402

PLANTED = cases.planted()
_WANT = {}


def want(c):
    """the reference's result, computed once per case and shared"""
    if c["name"] not in _WANT:
        _WANT[c["name"]] = cases.want(c)
    return _WANT[c["name"]]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def same(got, w, name):
    """every output equal to the reference's in every bit (NaN against NaN aside), and nothing written behind any array"""
    assert set(w) <= set(got), (name, sorted(w), sorted(got))
    for k, x in w.items():
        if k == "guard":   # (w may be another call's result)
            continue
        y = got[k]
        assert y.dtype == x.dtype and y.shape == x.shape, (name, k, y.dtype, y.shape, x.shape)
        ok = bits(x) == bits(y)
        if x.dtype == np.float32:
            ok |= np.isnan(x) & np.isnan(y)
        assert ok.all(), (name, k, np.argwhere(~ok)[:4].tolist(), x[~ok][:4], y[~ok][:4])
    assert all(v == (255 if k == "status" else -7) for k, v in got["guard"].items()), (name, got["guard"])


def call_args(c):
    return (c["point"], c["xyz"], c["ref_kf"], c["kf_center"], c["scale"]), dict(rows_form=c["rows_form"], term_off=c["term_off"])


def host(capi, c, **kw):
    a, k = call_args(c)
    return capi.LocalMap.update_normal_depth_host(c["g"], c["v"], *a, **dict(k, **kw))


def test_the_restatement_on_a_hand_computed_example():
    F = np.float32
    # cameras at (-1, 0, 0) and (1, 0, 0), the point at (0, 0, 1): d = (+-1, 0, 1), |d| = sqrt 2, theta = +-pi / 4
    g, v = cases.build([[2], [0, 1]], [[(0, 0), (1, 1)]])
    centre = np.array([[-1, 0, 0], [1, 0, 0]], F)
    r = ref.update_normal_depth(g, v, [0], [[0, 0, 1]], [1], centre, [1, 2, 4], ref.ROWS_TRACKING, np.array([0, 2], np.int32))
    inv = F(1 / np.sqrt(2.0))
    assert r["status"][0] == ref.UPDATED and r["n_terms"][0] == 2
    assert r["term_unit"].tolist() == [[inv, 0, inv], [-inv, 0, inv]] and r["term_theta"].tolist() == [F(np.pi / 4), -F(np.pi / 4)]
    assert r["normal"][0].tolist() == [0, 0, (inv + inv) * F(0.5)] and r["theta_mean"][0] == 0 and r["theta_std"][0] == F(np.pi / 4)
    # the reference keyframe 1 observes the point at its feature 1: octave 1, scale 2; the top scale is 4
    assert r["max_dist"][0] == F(np.sqrt(2.0)) * F(2) and r["min_dist"][0] == r["max_dist"][0] / F(4)
    assert r["max_range"][0] == F(1.2) * r["max_dist"][0] and r["min_range"][0] == F(0.8) * r["min_dist"][0]
    wide = np.float64(r["theta_std"][0]) * 2.5
    assert r["upper"][0] == F(wide) and r["lower"][0] == F(-wide)
    # as a non-observer keyframe 0 is read at feature 0 (octave 2): scale 4
    r = ref.update_normal_depth(cases.build([[2], [0, 1]], [[(1, 1)]])[0], cases.build([[2], [0, 1]], [[(1, 1)]])[1], [0, 0, 1],
                                np.zeros((3, 3), F), [0, 1, 0], centre, [1, 2, 4])
    assert list(r["status"]) == [ref.UPDATED, ref.UPDATED, ref.UNKNOWN] and r["max_dist"][0] == 4 and r["max_dist"][1] == 2
    assert r["theta_std"][0] == 0 and r["upper"][0] == r["theta_mean"][0] + F(30.0 / 57.3) and r["upper"][2] == -7


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, c):
    w = want(c)   # (asserts what the case was planted for)
    same(host(pkg.capi, c), w, c["name"])


def test_random_cases(pkg):
    seen = set()
    for seed in range(50):
        c = cases.random_case(seed)
        w = cases.want(c)
        same(host(pkg.capi, c), w, c["name"])
        seen |= set(w["status"].tolist())
    assert seen == {ref.UPDATED, ref.BAD, ref.NO_OBS, ref.UNKNOWN}   # (the unusable reference keyframes are planted)


def test_outputs_that_are_not_wanted_may_be_null(pkg):
    c = next(c for c in PLANTED if c["name"] == "specials/tracking")
    w = want(c)
    got = host(pkg.capi, c, want=("status", "theta_std", "lower"))
    assert sorted(k for k in got if k != "guard") == ["lower", "status", "theta_std"]
    same(got, {k: w[k] for k in ("status", "theta_std", "lower")}, "some")
    assert host(pkg.capi, c, want=()) == dict(guard={})


def test_host_side_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/normal_depth.h -- the checks, the arithmetic and the serial loop of the host tap -- in a stand-alone program of its own
    (tests/cpp/normal_depth_host_check.cpp), built with -fsanitize=address,undefined and run on the CPU: every output array is
    allocated at exactly its size there, so a write behind one stops the program"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "normal_depth_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(root, "tests", "cpp", "normal_depth_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_arguments_are_checked_before_a_device_is_looked_for(pkg):
    """every AOS2_ERR_ARG of aos2_local_map_update_normal_depth, on a machine without a device too, with the handle usable
    afterwards; the host tap makes the same checks"""
    capi = pkg.capi
    c = next(c for c in PLANTED if c["name"] == "specials/planning")
    g, v = c["g"], c["v"]
    uploaded = (capi.AOS2_OK, capi.AOS2_ERR_NO_DEVICE)
    ARG = capi.AOS2_ERR_ARG
    point, xyz, rk = c["point"][:3], c["xyz"][:3], c["ref_kf"][:3]
    args = (point, xyz, rk, c["kf_center"], c["scale"])

    def refused(fn, *a, **kw):
        with pytest.raises(capi.AosError) as e:
            fn(*a, **kw)
        assert e.value.code == ARG, (a, kw)

    m = capi.LocalMap()
    refused(m.update_normal_depth, *args)                                   # no graph is set
    assert m.set(g, ok=uploaded) in uploaded
    refused(m.update_normal_depth, *args)                                   # no culling view is set
    assert m.set_culling_view(v, ok=uploaded) in uploaded
    tap = capi.LocalMap.update_normal_depth_host
    for call in (m.update_normal_depth, lambda *a, **kw: tap(g, v, *a, **kw)):
        refused(call, *args, n=-1)                                          # a negative count
        refused(call, *args, n_levels=0)
        refused(call, *args, n_levels=-3)
        for k in ("point", "xyz", "ref_kf", "kf_center", "scale"):         # NULL with a non-zero length
            refused(call, *args, null=(k,))
        refused(call, point, xyz, [0, cases.NK, 0], *args[3:])              # a reference keyframe outside the graph
        refused(call, point, xyz, [0, 0, -1], *args[3:])
        refused(call, [0, -1, 0], *args[1:])                                # a point row below 0
        refused(call, *args, term_off=[1, 2, 3, 4])                         # does not start at 0
        refused(call, *args, term_off=[0, 2, 1, 4])                         # descends
        refused(call, *args, want=("status", "term_unit"))                  # the term arrays without term_off
        refused(call, *args, want=("term_theta",))
        refused(call, *args, rows_form=2)
        refused(call, *args, rows_form=-1)
    L = capi.lib()
    assert L.aos2_local_map_update_normal_depth(None, None) == ARG and L.aos2_local_map_update_normal_depth(m.h, None) == ARG
    # ONE list whose thetas do not fit the scratch bound: every list waits in global scratch, 4 bytes per observation
    m.debug_normal_depth(0)
    m.debug_limits(scratch_bytes=4 * 2 - 1)
    refused(m.update_normal_depth, *args)                                   # (the first listed point has two observations)
    m.debug_limits()
    m.debug_normal_depth()
    with pytest.raises(capi.AosError) as e:                                 # the hook: at most 64 thetas in LDS
        m.debug_normal_depth(65)
    assert e.value.code == ARG
    # n == 0 is valid and needs no device
    r = m.update_normal_depth([], np.zeros((0, 3)), [], c["kf_center"], c["scale"])
    assert len(r["status"]) == 0 and r["normal"].shape == (0, 3) and m.last_normal_depth_device_ms() == -1 and m.last_groups() == 0
    # the host tap checks the graph and the view as the set calls do
    bad = dict(v, obs_idx=v["obs_idx"].copy())
    bad["obs_idx"][0] = 99
    refused(tap, g, bad, *args)
    # the handle is still usable
    assert m.graph()["n_keyframes"] == cases.NK and m.view() is not None
    m.close()
