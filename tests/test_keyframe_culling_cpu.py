"""LocalMapping::KeyFrameCulling on the host (aos2_debug_keyframe_culling_host, csrc/debug_taps.hip: the per-item functions the
device kernels run, serially) against the plain-Python restatement tests/keyframe_culling_ref.py: every status byte, every count,
the bad-point list and its length equal, on the planted cases of tests/keyframe_culling_cases.py and on the seeded sweep; the checks
that keep the cases honest, made with the reference alone; and every AOS2_ERR_ARG of the new entry points.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import keyframe_culling_cases as cases   # noqa: E402
import keyframe_culling_ref as ref       # noqa: E402

PLANTED = cases.planted()
_WANT = {}


def want(c):
    """the reference's result, computed once per case and shared"""
    if c["name"] not in _WANT:
        _WANT[c["name"]] = cases.want(c)
    return _WANT[c["name"]]


def same(got, w, c):
    """every output equal; bad_points: the first min(count, cap) rows, and nothing written behind them"""
    name = c["name"]
    for k in ("status", "n_mps", "n_redundant"):
        assert got[k].dtype == w[k].dtype and np.array_equal(got[k], w[k]), (name, k, got[k], w[k])
    assert got["n_bad_points"] == w["n_bad_points"], (name, got["n_bad_points"], w["n_bad_points"])
    cap = len(got["bad_points"]) - 1
    m = min(cap, w["n_bad_points"])
    assert list(got["bad_points"][:m]) == list(w["bad_points"][:m]), (name, got["bad_points"][:m], w["bad_points"][:m])
    assert (got["bad_points"][m:] == -7).all(), name


def host(capi, c):
    return capi.LocalMap.keyframe_culling_host(c["g"], c["v"], c["cand"], c["monocular"], c["bad_cap"])


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, c):
    w = want(c)   # (asserts what the case was planted for)
    same(host(pkg.capi, c), w, c)


def test_small_bad_cap_leaves_the_rest_alone(pkg):
    c = next(c for c in PLANTED if c["name"] == "small_bad_cap")
    got = host(pkg.capi, c)
    assert got["n_bad_points"] == 5 and list(got["bad_points"]) == [60, 61, -7]
    got = pkg.capi.LocalMap.keyframe_culling_host(c["g"], c["v"], c["cand"], c["monocular"], bad_cap=0)
    assert got["n_bad_points"] == 5 and list(got["bad_points"]) == [-7]


@pytest.mark.parametrize("seed", cases.SWEEP_SEEDS)
def test_sweep(pkg, seed):
    c = cases.random_case(seed)
    same(host(pkg.capi, c), want(c), c)


def test_the_sweep_shows_what_it_is_for():
    """from the reference alone: at least half the seeds cull, at least four cull twice or more, at least four hold a verdict that
    an erasure flipped"""
    rs = [want(cases.random_case(s)) for s in cases.SWEEP_SEEDS]
    assert len(rs) == 24
    culls = [r["n_culled"] for r in rs]
    flipped = [bool(((r["alone"] != r["status"])).any()) for r in rs]
    assert sum(n >= 1 for n in culls) >= 12, culls
    assert sum(n >= 2 for n in culls) >= 4, culls
    assert sum(flipped) >= 4, flipped
    assert any(r["n_bad_points"] > 0 for r in rs) and any((r["status"] == ref.DEFERRED).any() for r in rs)
    assert any((r["status"] == ref.SKIPPED).any() for r in rs)


def _copy(d):
    return {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in d.items()}


def test_arguments_are_checked_before_a_device_is_looked_for(pkg):
    """every AOS2_ERR_ARG of aos2_local_map_set_culling_view and aos2_local_map_keyframe_culling, on a machine without a device
    too, with the handle usable afterwards; the host tap makes the same checks"""
    capi = pkg.capi
    c = next(c for c in PLANTED if c["name"] == "flip_to_kept")
    g, v = c["g"], c["v"]
    uploaded = (capi.AOS2_OK, capi.AOS2_ERR_NO_DEVICE)

    def refused(fn, *a, **kw):
        with pytest.raises(capi.AosError) as e:
            fn(*a, **kw)
        assert e.value.code == capi.AOS2_ERR_ARG, (a, kw)

    m = capi.LocalMap()
    refused(m.set_culling_view, v, ok=uploaded)         # no graph is set
    refused(m.keyframe_culling, [0])                    # no view
    assert m.set(g, ok=uploaded) in uploaded
    refused(m.keyframe_culling, [0])                    # still no view
    for k in v:                                         # an array NULL while the graph gives it a length
        bad = _copy(v)
        bad[k] = None
        refused(m.set_culling_view, bad, ok=uploaded)
        refused(capi.LocalMap.keyframe_culling_host, g, bad, [0])
    for e, idx in ((0, 10), (3, -1)):                   # an obs_idx outside its keyframe's features
        bad = _copy(v)
        bad["obs_idx"][e] = idx
        refused(m.set_culling_view, bad, ok=uploaded)
        refused(capi.LocalMap.keyframe_culling_host, g, bad, [0])
    refused(m.keyframe_culling, [0])                    # a refused view is not the handle's
    assert m.set_culling_view(v, ok=uploaded) in uploaded
    for cand in ([4], [-1], [0, 1, 0]):                 # a row out of range, a row twice
        refused(m.keyframe_culling, cand)
        refused(capi.LocalMap.keyframe_culling_host, g, v, cand)
    m.debug_limits(scratch_bytes=64)                    # an overlay above the scratch bound
    refused(m.keyframe_culling, [0])
    m.debug_limits()
    L = capi.lib()
    nb =capi.C.c_int32(0)
    one = np.zeros(1, np.int32)
    st = np.zeros(1, np.uint8)
    p = capi._p
    assert L.aos2_local_map_keyframe_culling(m.h, 1, -1, p(one), p(st), p(one), p(one), None, 0, capi.C.byref(nb)) == capi.AOS2_ERR_ARG
    assert L.aos2_local_map_keyframe_culling(m.h, 1, 1, None, p(st), p(one), p(one), None, 0, capi.C.byref(nb)) == capi.AOS2_ERR_ARG
    # n_cand == 0 is valid, and needs no device
    r = m.keyframe_culling([])
    assert r["n_bad_points"] == 0 and len(r["status"]) == 0 and m.last_culling_rounds() == 0
    # the handle is still usable: the graph stands, and a new graph drops the view
    assert m.graph()["n_keyframes"] == 4
    assert m.set(g, ok=uploaded) in uploaded
    refused(m.keyframe_culling, [0])
    m.debug_culling_rounds(1)
    m.debug_culling_rounds(0)
    m.close()
