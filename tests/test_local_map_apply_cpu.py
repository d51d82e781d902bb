"""aos2_local_map_apply on a graph that is not resident (the host restatement, csrc/local_map_apply.hip) against
tests/local_map_apply_ref.py: every array of the handle's snapshot and of its view exactly equal, on the planted deltas of
tests/local_map_apply_cases.py and on sequences of random deltas; the checks of the call, made before a device is looked for; and the
self-check of the generator that the GPU tests share.  No GPU."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import local_map_apply_cases as cases   # noqa: E402
import local_map_apply_ref as ref       # noqa: E402

PLANTED = cases.planted()
SEQUENCE_SEEDS, sequence = cases.SEQUENCE_SEEDS, cases.sequence


def uploaded(capi):
    return (capi.AOS2_OK, capi.AOS2_ERR_NO_DEVICE)


def handle(capi, g, v):
    """a handle that was never uploaded: aos2_local_map_apply rebuilds its host copy"""
    m = capi.LocalMap()
    if g["n_keyframes"] or g["n_points"] or v is not None:
        m.set(g, ok=uploaded(capi))
        if v is not None:
            m.set_culling_view(v, ok=uploaded(capi))
    return m


def check(m, g, v, what):
    assert ref.same_graph(m.graph(), g) is None, (what, ref.same_graph(m.graph(), g))
    assert ref.same_view(m.view(), v) is None, (what, ref.same_view(m.view(), v))


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_delta_on_the_host(pkg, c):
    capi = pkg.capi
    g, v = cases.want(c)
    m = handle(capi, c["g"], c["v"])
    assert m.apply(c["delta"], ok=uploaded(capi)) in uploaded(capi)
    check(m, g, v, c["name"])
    m.close()


@pytest.mark.parametrize("seed", SEQUENCE_SEEDS)
def test_random_sequence_on_the_host(pkg, seed):
    capi = pkg.capi
    g, v, steps = sequence(seed)
    m = handle(capi, g, v)
    for i, (d, g1, v1) in enumerate(steps):
        gr, vr = ref.apply(g, v, d)
        assert ref.same_graph(gr, g1) is None and ref.same_view(vr, v1) is None   # (the reference reproduces the edited model)
        assert m.apply(d, ok=uploaded(capi)) in uploaded(capi)
        check(m, gr, vr, (seed, i))
        g, v = gr, vr
    m.close()


def test_the_generator_grows_shrinks_appends_and_keeps_rows():
    """a sweep that only ever appends proves little: over the sequences used here and on the GPU every kind of change occurs, in
    every single delta for the observation rows"""
    for seed in SEQUENCE_SEEDS:
        g, v, steps = sequence(seed)
        total = dict(grew=0, shrank=0, appended=0, stayed=0)
        for d, g1, _ in steps:
            ch = cases.row_changes(g, g1)
            assert ch["grew"] > 0 and ch["shrank"] > 0 and ch["appended"] > 0 and ch["stayed"] > 0, (seed, ch)
            assert g1["n_keyframes"] == g["n_keyframes"] + 1 and g1["n_points"] > g["n_points"]
            assert 0 < len(d["kf_mp_row"]) and 0 < len(d["kf_link_row"]) and 0 < len(d["point_row"]) < g1["n_points"]
            for k in total:
                total[k] += ch[k]
            g = g1
        assert min(total.values()) > 0


def bad_deltas(c):
    """(name, delta) for every check of aos2_local_map_apply, each one change away from the valid delta of the planted case
    append_keyframe"""
    d0 = c["delta"]

    def mod(view=None, **kw):
        d = copy.deepcopy(d0)
        for k, x in kw.items():
            if callable(x):
                x(d[k])
            else:
                d[k] = x
        for k, x in (view or {}).items():
            if callable(x):
                x(d["view"][k])
            else:
                d["view"][k] = x
        return d

    def put(i, x):
        def f(a):
            a[i] = x
        return f
    # the valid delta: point rows [15, 16, 19, 20, 21], match row [6] (6 features), link rows [5, 6]
    out = [("fewer points", mod(n_points=19)), ("fewer keyframes", mod(n_keyframes=5)),
           ("point_row not ascending", mod(point_row=put(1, 15))), ("point_row descending", mod(point_row=put(0, 17))),
           ("point_row outside", mod(point_row=put(4, 22))), ("point_row negative", mod(point_row=put(0, -1))),
           ("kf_mp_row outside", mod(kf_mp_row=put(0, 7))), ("kf_link_row twice", mod(kf_link_row=put(0, 6))),
           ("appended keyframe not in kf_mp_row", mod(kf_mp_row=np.zeros(0, np.int32), kf_mp_off=np.zeros(1, np.int32), n_kf_mp_rows=0)),
           ("appended keyframe not in kf_link_row", mod(kf_link_row=put(1, 4), n_kf_link_rows=1)),
           ("point_row NULL", mod(point_row=None, n_point_rows=5)), ("point_bad NULL", mod(point_bad=None)),
           ("point_nobs NULL", mod(point_nobs=None)), ("obs_off NULL", mod(obs_off=None)), ("obs_kf NULL", mod(obs_kf=None)),
           ("kf_mp_row NULL", mod(kf_mp_row=None, n_kf_mp_rows=1)), ("kf_mp_off NULL", mod(kf_mp_off=None)), ("kf_mp NULL", mod(kf_mp=None)),
           ("kf_link_row NULL", mod(kf_link_row=None, n_kf_link_rows=2)), ("kf_bad NULL", mod(kf_bad=None)), ("kf_best NULL", mod(kf_best=None)),
           ("kf_child_off NULL", mod(kf_child_off=None)), ("kf_child NULL", mod(kf_child=None)), ("kf_parent NULL", mod(kf_parent=None)),
           ("obs_off starts past 0", mod(obs_off=put(0, 1))), ("obs_off decreases", mod(obs_off=put(1, 0))),
           ("kf_mp_off starts past 0", mod(kf_mp_off=put(0, 1))), ("kf_child_off decreases", mod(kf_child_off=np.array([0, 1, 0], np.int32))),
           ("obs_kf outside", mod(obs_kf=put(0, 7))), ("obs_kf negative", mod(obs_kf=put(0, -1))),
           ("kf_mp outside", mod(kf_mp=put(0, 22))), ("kf_mp below -1", mod(kf_mp=put(0, -2))),
           ("kf_best outside", mod(kf_best=put(0, 7))), ("kf_best below -1", mod(kf_best=put(0, -2))),
           ("kf_child outside", mod(kf_child=put(0, 7))), ("kf_child negative", mod(kf_child=put(0, -1))),
           ("kf_parent outside", mod(kf_parent=put(1, 7))), ("kf_parent below -1", mod(kf_parent=put(1, -2))),
           ("keyframe twice in one point", mod(obs_kf=put(1, int(d0["obs_kf"][0])))),
           ("view missing", dict(copy.deepcopy(d0), view=None)),
           ("view obs_idx NULL", mod(view=dict(obs_idx=None))), ("view kf_octave NULL", mod(view=dict(kf_octave=None))),
           ("view kf_th_depth NULL", mod(view=dict(kf_th_depth=None))),
           ("obs_idx outside the new keyframe", mod(view=dict(obs_idx=put(len(d0["obs_kf"]) - 1, 6)))),
           ("obs_idx negative", mod(view=dict(obs_idx=put(0, -1))))]
    # a match row of an EXISTING keyframe of another length, and an obs_idx past the features of an existing keyframe
    n5 = int(np.diff(c["g"]["kf_mp_off"])[5])
    d = mod(kf_mp_row=np.array([5, 6], np.int32), kf_mp_off=np.array([0, n5 - 1, n5 + 5], np.int32),
            kf_mp=np.concatenate([np.full(n5 - 1, -1, np.int32), d0["kf_mp"]]),
            view=dict(kf_octave=np.zeros(n5 + 5, np.int8), kf_depth=np.zeros(n5 + 5, np.float32), kf_stereo=np.zeros(n5 + 5, np.uint8)))
    out.append(("existing match row changes its length", d))
    e = int(d0["obs_off"][1]) - 2   # (an entry of point 15 that an existing keyframe holds)
    kf = int(d0["obs_kf"][e])
    assert kf < 6
    out.append(("obs_idx outside an existing keyframe", mod(view=dict(obs_idx=put(e, int(np.diff(c["g"]["kf_mp_off"])[kf]))))))
    return out


def test_apply_validates_before_a_device_is_looked_for(pkg):
    """every refused delta gives AOS2_ERR_ARG -- on a machine without a device too -- and leaves graph and view as they were"""
    capi = pkg.capi
    c = next(c for c in PLANTED if c["name"] == "append_keyframe")
    m = handle(capi, c["g"], c["v"])
    kept_g, kept_v = m.graph(), m.view()
    for name, d in bad_deltas(c):
        with pytest.raises(capi.AosError) as e:
            m.apply(d, ok=uploaded(capi))
        assert e.value.code == capi.AOS2_ERR_ARG, name
        check(m, kept_g, kept_v, name)
    # a view given to a handle that holds none
    plain = handle(capi, c["g"], None)
    with pytest.raises(capi.AosError) as e:
        plain.apply(c["delta"], ok=uploaded(capi))
    assert e.value.code == capi.AOS2_ERR_ARG
    check(plain, kept_g, None, "view without a resident view")
    plain.close()
    # NULL handle and NULL delta
    L = capi.lib()
    assert L.aos2_local_map_apply(None, None) == capi.AOS2_ERR_ARG and L.aos2_local_map_apply(m.h, None) == capi.AOS2_ERR_ARG
    # the valid delta still applies afterwards, and a second one on top of it
    g, v = cases.want(c)
    assert m.apply(c["delta"], ok=uploaded(capi)) in uploaded(capi)
    check(m, g, v, "valid")
    assert m.last_apply()["path"] == 0
    d2 = dict(c["delta"], n_points=21)   # a count below the one the handle has NOW
    with pytest.raises(capi.AosError) as e:
        m.apply(d2, ok=uploaded(capi))
    assert e.value.code == capi.AOS2_ERR_ARG
    check(m, g, v, "after the second refusal")
    m.close()


def test_empty_delta_and_handle_without_a_set(pkg):
    capi = pkg.capi
    m = capi.LocalMap()
    empty = dict(n_points=0, n_keyframes=0)
    assert m.apply(empty, ok=uploaded(capi)) in uploaded(capi)
    assert m.graph()["n_points"] == 0 and m.graph()["n_keyframes"] == 0 and m.view() is None
    c = next(c for c in PLANTED if c["name"] == "onto_empty_map")
    assert m.apply(c["delta"], ok=uploaded(capi)) in uploaded(capi)
    check(m, c["g1"], None, "onto the empty map")
    m.close()
