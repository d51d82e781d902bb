"""Tracking::UpdateLocalMap on the host (aos2_debug_local_map_host, csrc/debug_taps.hip) against the line-by-line restatement
tests/local_map_ref.py: every output equal as integers, on the planted cases of tests/local_map_cases.py, on seeded random
graphs, and the argument checks of aos2_local_map_set.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import local_map_cases as cases   # noqa: E402
import local_map_ref as ref       # noqa: E402

KEYS = ("mp", "local", "n_local", "local_kfs", "n_local_kfs", "ref_kf")
PLANTED = cases.planted()


def host(capi, c):
    return capi.LocalMap.host(c["g"], c["n"], c["mp"], c["local_cap"], c["kf_cap"], c["local_kfs"], c["n_local_kfs"], c["ref_kf"])


def same(got, want, name):
    for k in KEYS:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, c):
    want = cases.want(c)
    before = {k: c[k].copy() for k in ("mp", "local_kfs", "n_local_kfs", "ref_kf")}
    same(host(pkg.capi, c), want, c["name"])
    assert all(np.array_equal(c[k], before[k]) for k in before)   # (the binding works on copies)


@pytest.mark.parametrize("seed,nk,npnt,B", [(1, 12, 40, 24), (2, 1, 5, 8), (3, 40, 300, 24), (4, 200, 1500, 12), (5, 7, 0, 4), (6, 0, 9, 4),
                                            (7, 0, 0, 3)])
def test_random_sweep(pkg, seed, nk, npnt, B):
    c = cases.random_case(seed, nk, npnt, B, sizes=(0, 1, 8, 17, 33, 64))
    want = cases.want(c)
    same(host(pkg.capi, c), want, c["name"])
    if nk >= 12 and npnt:
        assert want["voted"].any() and not want["voted"].all() and (want["n_local"] > 0).any()
    # small capacities: the true counts and the first rows
    lk = np.full((B, 3), -1, np.int32)
    w = min(3, c["kf_cap"])
    lk[:, :w] = c["local_kfs"][:, :w]
    c2 = dict(c, local_cap=5, kf_cap=3, local_kfs=lk, n_local_kfs=np.minimum(c["n_local_kfs"], 3))
    want2 = cases.want(c2)
    same(host(pkg.capi, c2), want2, c["name"] + "/small")


def test_stats_host_vs_ref(pkg):
    rng = np.random.default_rng(11)
    g = cases.random_graph(rng, 10, 60)
    n, mp = cases.frames_arrays(cases.random_frames(rng, g, 9, (0, 5, 31, 64)), cap=64)
    outlier = (rng.random(mp.shape) < 0.3).astype(np.uint8)
    for stereo in (False, True):
        for only_tracking in (False, True):
            want = ref.stats_batch(g, n, mp, outlier, stereo, only_tracking)
            got = pkg.capi.LocalMap.stats_host(g, n, mp, outlier, stereo, only_tracking)
            for k in ("stats", "mp", "found_inc"):
                assert np.array_equal(got[k], want[k]), (stereo, only_tracking, k)
            assert (want["mp"] != mp).any() == stereo and want["stats"][:, 0].sum() > 0
            assert (want["stats"][:, 2] == 0).all() == only_tracking
    assert (g["point_nobs"] != np.diff(g["obs_off"])).any()   # Observations() is not the length of the list


def bad_graphs():
    g0 = cases.make_graph(4, [[0, 1], [1, 2, -1], [3]], best={0: [1, 2]}, children={0: [1, 2]}, parent={1: 0, 2: 0})

    def mod(**kw):
        g = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g0.items()}
        for k, v in kw.items():
            if callable(v):
                v(g[k])
            else:
                g[k] = v
        return g

    def put(i, v):
        def f(a):
            a[i] = v
        return f
    return g0, [
        ("negative points", mod(n_points=-1)), ("negative keyframes", mod(n_keyframes=-1)),
        ("obs_kf out of range", mod(obs_kf=put(0, 3))), ("obs_kf negative", mod(obs_kf=put(0, -1))),
        ("kf_mp out of range", mod(kf_mp=put(0, 4))), ("kf_mp below -1", mod(kf_mp=put(0, -2))),
        ("kf_best out of range", mod(kf_best=put(0, 3))), ("kf_best below -1", mod(kf_best=put(3, -2))),
        ("kf_child out of range", mod(kf_child=put(0, 3))), ("kf_child negative", mod(kf_child=put(0, -1))),
        ("kf_parent out of range", mod(kf_parent=put(1, 3))), ("kf_parent below -1", mod(kf_parent=put(1, -2))),
        ("obs_off decreases", mod(obs_off=put(2, 0))), ("kf_mp_off decreases", mod(kf_mp_off=put(1, 6))),
        ("kf_child_off decreases", mod(kf_child_off=put(1, 3))), ("obs_off starts past 0", mod(obs_off=put(0, 1))),
        ("point_bad NULL", mod(point_bad=None)), ("point_nobs NULL", mod(point_nobs=None)), ("obs_off NULL", mod(obs_off=None)),
        ("obs_kf NULL", mod(obs_kf=None)), ("kf_bad NULL", mod(kf_bad=None)), ("kf_mp_off NULL", mod(kf_mp_off=None)),
        ("kf_mp NULL", mod(kf_mp=None)), ("kf_best NULL", mod(kf_best=None)), ("kf_child_off NULL", mod(kf_child_off=None)),
        ("kf_child NULL", mod(kf_child=None)), ("kf_parent NULL", mod(kf_parent=None)),
        ("keyframe twice in one point", mod(obs_kf=put(2, 0))),
    ]


def test_set_validates_before_a_device_is_looked_for(pkg):
    """Every refused graph gives AOS2_ERR_ARG -- on a machine without a device too -- and leaves the previous graph; a valid one is
    the handle's even where its upload finds no device."""
    capi = pkg.capi
    g0, bad = bad_graphs()
    assert list(g0["obs_kf"][:3]) == [0, 0, 1]   # ("keyframe twice" rewrites point 1's second entry)
    m = capi.LocalMap()
    uploaded = (capi.AOS2_OK, capi.AOS2_ERR_NO_DEVICE)
    assert m.set(g0, ok=uploaded) in uploaded
    kept = m.graph()
    assert kept["n_points"] == 4 and kept["n_keyframes"] == 3
    for name, g in bad:
        with pytest.raises(capi.AosError) as e:
            m.set(g, ok=uploaded)
        assert e.value.code == capi.AOS2_ERR_ARG, name
        now = m.graph()
        assert all(np.array_equal(now[k], kept[k]) for k in kept), name
        with pytest.raises(capi.AosError) as e:   # the host tap makes the same checks
            capi.LocalMap.host(g, [1], [[0]], 4, 4)
        assert e.value.code == capi.AOS2_ERR_ARG, name
    for k in g0:   # the snapshot is the graph that was set (children in ascending row)
        assert np.array_equal(kept[k], g0[k]), k
    empty = cases.make_graph(0, [])
    assert m.set(empty, ok=uploaded) in uploaded
    assert m.graph()["n_points"] == 0 and m.graph()["n_keyframes"] == 0
    r = capi.LocalMap.host(empty, [2], [[0, -1]], 4, 4)
    assert r["n_local"][0] == 0 and r["n_local_kfs"][0] == 0 and list(r["mp"][0]) == [0, -1]
    m.close()
