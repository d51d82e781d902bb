"""KeyFrame::UpdateConnections on the device (aos2_local_map_update_connections, csrc/connections.hip) against the plain-Python
restatement tests/update_connections_ref.py and against the host tap, byte for byte: the planted cases, the graph of 300 keyframes
with ordered lists of 1, 2, 63, 64, 65 and 257 entries on both sides of the scan's seam, and 50 seeded random cases -- each with the
counters in LDS and in global scratch and with the list sorted in LDS and in global scratch; a batch split into groups by the
scratch bound; the resident and the explicit form of the matches; and the graph after an aos2_local_map_apply on the device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import local_map_cases as lm_cases         # noqa: E402
import update_connections_cases as cases   # noqa: E402
import update_connections_ref as ref       # noqa: E402
from test_update_connections_cpu import PLANTED, host, same, same_bytes, want   # noqa: E402

pytestmark = pytest.mark.gpu

# (largest n_keyframes with the counters in LDS, longest list sorted in LDS): the defaults, counters in global scratch, the sort
# in global scratch for every list of two or more, both
FORMS = {"lds": (-1, 0), "global_counters": (0, 0), "global_sort": (-1, 1), "global_both": (0, 1)}


def device(capi, c, form="lds", scratch=0):
    """the case on a fresh handle -> (result, groups the batch ran in, device ms)"""
    lds_kfs, lds_sort = FORMS[form]
    m = capi.LocalMap()
    m.set(c["g"])
    m.debug_limits(scratch, lds_kfs)
    m.debug_connections_sort(lds_sort)
    r = m.update_connections(c["kf"], c["mp"], c["th"], c["conn_cap"], c["ordered_cap"])
    out = r, m.last_groups(), m.last_connections_device_ms()
    m.close()
    return out


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, gpu, c, form):
    w = want(c)
    got, groups, ms = device(pkg.capi, c, form)
    same(got, w, c)
    same_bytes(got, host(pkg.capi, c), c["name"])
    if len(c["kf"]):
        assert groups == 1 and ms > 0
    else:
        assert groups == 0 and ms == -1


@pytest.mark.parametrize("form", list(FORMS))
def test_random_cases(pkg, gpu, form):
    for seed in range(50):
        c = cases.random_case(seed)
        got = device(pkg.capi, c, form)[0]
        same(got, cases.want(c), c)
        same_bytes(got, host(pkg.capi, c), c["name"])


@pytest.mark.parametrize("form", ["lds", "global_both"])
def test_a_batch_split_into_groups_gives_the_same_outputs(pkg, gpu, form):
    c = dict(next(c for c in PLANTED if c["name"] == "long_lists"))
    c["kf"] = [5, 0, 1, 2, 3, 4, 6, 5]
    w = cases.ref.update_connections(c["g"], c["kf"], None, c["th"], c["conn_cap"], c["ordered_cap"])
    assert list(w["n_ordered"]) == [257, 1, 2, 63, 64, 65, 1, 257]
    whole, groups, _ = device(pkg.capi, c, form)
    assert groups == 1
    same(whole, w, c)
    per_kf = 12 * c["g"]["n_keyframes"] + 16
    for bound, n_groups in ((3 * per_kf + 5, 3), (per_kf, 8), (8 * per_kf - 1, 2)):
        got, groups, _ = device(pkg.capi, c, form, scratch=bound)
        assert groups == n_groups, (bound, groups)
        same(got, w, c)
        same_bytes(got, whole, form)


def test_resident_and_explicit_matches_agree(pkg, gpu):
    c = next(c for c in PLANTED if c["name"] == "long_lists")
    e = dict(c)
    e["mp"] = [ref.resident_matches(c["g"], k) for k in c["kf"]]
    a, b = device(pkg.capi, c)[0], device(pkg.capi, e)[0]
    same(a, want(c), c)
    same_bytes(a, b, "explicit")
    # ... and both forms on one handle, one call after the other (the staging is laid out again)
    m = pkg.capi.LocalMap()
    m.set(c["g"])
    first = m.update_connections(e["kf"], e["mp"], c["th"], c["conn_cap"], c["ordered_cap"])
    second = m.update_connections(c["kf"], None, c["th"], c["conn_cap"], c["ordered_cap"])
    third = m.update_connections(c["kf"][:2], None, c["th"], 2, 1)
    assert m.last_connections_device_ms() > 0
    m.close()
    same_bytes(first, a, "first")
    same_bytes(second, a, "second")
    assert list(third["n_ordered"]) == [1, 2] and third["ordered_kf"].shape == (2, 1) and all(v == -7 for v in third["guard"].values())


def test_the_call_reads_the_graph_that_apply_built_on_the_device(pkg, gpu):
    """a delta that adds observations to three points, applied on the device path: the result is the reference's on the post-delta
    graph, and differs from the one before"""
    capi = pkg.capi
    nk, th = 300, 3
    kf_mp = [[] for _ in range(nk)]
    kf_mp[0] = [0, 1, 2, 3]
    obs0 = {0: [0, 10, 299], 1: [0, 10], 2: [0, 299], 3: [0]}
    obs1 = {0: [0, 10, 299, 260], 1: [0, 10, 260], 2: [0, 299, 260], 3: [0, 10]}
    g0, g1 = lm_cases.make_graph(4, kf_mp, obs=obs0), lm_cases.make_graph(4, kf_mp, obs=obs1)
    rows = [0, 1, 2, 3]
    delta = dict(n_points=4, n_keyframes=nk, point_row=np.array(rows, np.int32), point_bad=np.zeros(4, np.uint8),
                 point_nobs=g1["point_nobs"], obs_off=g1["obs_off"], obs_kf=g1["obs_kf"], view=None)
    before = ref.update_connections(g0, [0], None, th, 8, 8)
    after = ref.update_connections(g1, [0], None, th, 8, 8)
    assert before["ordered"][0] == [(10, 2)] and after["ordered"][0] == [(260, 3), (10, 3)]
    for form in FORMS:
        m = capi.LocalMap()
        m.set(g0)
        m.debug_limits(0, FORMS[form][0])
        m.debug_connections_sort(FORMS[form][1])
        c = dict(name="apply/" + form)
        same(m.update_connections([0], None, th, 8, 8), before, c)
        m.apply(delta)
        assert m.last_apply()["path"] == 1
        got = m.update_connections([0], None, th, 8, 8)
        same(got, after, c)
        same_bytes(got, capi.LocalMap.update_connections_host(g1, [0], None, th, 8, 8), form)
        m.close()
