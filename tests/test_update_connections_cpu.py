"""KeyFrame::UpdateConnections on the host (aos2_debug_update_connections_host: the per-item functions of csrc/connections.h that the
device kernel runs, serially) against the plain-Python restatement tests/update_connections_ref.py: every count, every row of the
four arrays and the words behind them, compared exactly, on the planted cases of tests/update_connections_cases.py, the graph of
300 keyframes and 200 seeded random cases; the restatement itself on hand-computed examples; and every AOS2_ERR_ARG of the new
entry points.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import local_map_cases as lm_cases       # noqa: E402
import update_connections_cases as cases   # noqa: E402
import update_connections_ref as ref       # noqa: E402

PLANTED = cases.planted() + [cases.long_lists()]
_WANT = {}
ARRAYS = ("conn_kf", "conn_w", "ordered_kf", "ordered_w")


def want(c):
    """the reference's result, computed once per case and shared"""
    if c["name"] not in _WANT:
        _WANT[c["name"]] = cases.want(c)
    return _WANT[c["name"]]


def same(got, w, c):
    """every output equal to the reference's, and nothing written behind any array"""
    name = c["name"]
    for k in ("n_conn", "n_ordered") + ARRAYS:
        assert got[k].dtype == w[k].dtype and got[k].shape == w[k].shape and np.array_equal(got[k], w[k]), (name, k, got[k], w[k])
    assert all(v == -7 for v in got["guard"].values()), (name, got["guard"])


def same_bytes(a, b, name):
    for k in ("n_conn", "n_ordered") + ARRAYS:
        assert a[k].tobytes() == b[k].tobytes(), (name, k)


def host(capi, c):
    return capi.LocalMap.update_connections_host(c["g"], c["kf"], c["mp"], c["th"], c["conn_cap"], c["ordered_cap"])


def test_the_restatement_on_hand_computed_examples():
    # observations: point 0 by {0, 1, 2}, 1 by {0, 1}, 2 by {0}, 3 by {2, 3}
    g = lm_cases.make_graph(4, [[0, 1, 2], [0, 1], [0, 3], [3]])
    one = ref.update_connections_one
    assert one(g, 0, [0, 1, 2], 2) == ({1: 2, 2: 1}, [(1, 2)])
    assert one(g, 0, [0, 1, 2], 1) == ({1: 2, 2: 1}, [(1, 2), (2, 1)])
    assert one(g, 0, [0, 1, 2], 15) == ({1: 2, 2: 1}, [(1, 2)])           # nothing over 15: the maximum
    assert one(g, 2, [0, 3], 15) == ({0: 1, 1: 1, 3: 1}, [(0, 1)])          # a three-way tie at the maximum: the lowest row
    assert one(g, 2, [0, 3], 1) == ({0: 1, 1: 1, 3: 1}, [(3, 1), (1, 1), (0, 1)])   # the same tie over the threshold: descending row
    assert one(g, 3, [3], 15) == ({2: 1}, [(2, 1)])
    assert one(g, 0, [2], 15) == ({}, [])                                   # seen by itself only
    assert one(g, -1, [2, -1, 9], 15) == ({0: 1}, [(0, 1)])                 # nobody to skip; NULL and an unknown row
    assert one(g, 1, [0, 0, 1], 3) == ({0: 3, 2: 2}, [(0, 3)])              # a point twice counts twice
    r = ref.update_connections(g, [2, 0], None, 1, conn_cap=2, ordered_cap=4)
    assert list(r["n_conn"]) == [3, 2] and list(r["n_ordered"]) == [3, 2]
    assert r["conn_kf"].tolist() == [[0, 1], [1, 2]] and r["conn_w"].tolist() == [[1, 1], [2, 1]]
    assert r["ordered_kf"].tolist() == [[3, 1, 0, -1], [1, 2, -1, -1]] and r["ordered_w"].tolist() == [[1, 1, 1, 0], [2, 1, 0, 0]]


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(pkg, c):
    w = want(c)   # (asserts what the case was planted for)
    same(host(pkg.capi, c), w, c)


def test_random_cases(pkg):
    forms = set()
    for seed in range(200):
        c = cases.random_case(seed)
        w = cases.want(c)
        same(host(pkg.capi, c), w, c)
        for k in range(len(c["kf"])):
            forms.add((c["mp"] is None, w["n_conn"][k] == 0, w["n_ordered"][k] > 1, bool(w["n_conn"][k] > w["n_ordered"][k] == 1)))
    # both forms with an empty counter, a list over the threshold and the single maximum among several
    for resident in (True, False):
        assert (resident, True, False, False) in forms
        assert any(f[0] == resident and f[2] for f in forms) and any(f[0] == resident and f[3] for f in forms)


def test_host_side_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """csrc/connections.h -- the checks and the serial loop of the host tap -- in a stand-alone program of its own (tests/cpp/
    connections_host_check.cpp), built with -fsanitize=address,undefined and run on the CPU: every output array is allocated at
    exactly its size there, so a write behind one stops the program"""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "connections_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(root, "tests", "cpp", "connections_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout[-2000:], r.stderr[-2000:])


def test_arguments_are_checked_before_a_device_is_looked_for(pkg):
    """every AOS2_ERR_ARG of aos2_local_map_update_connections, on a machine without a device too, with the handle usable
    afterwards; the host tap makes the same checks"""
    capi = pkg.capi
    C = capi.C
    c = next(c for c in PLANTED if c["name"] == "th_and_th_minus_1")
    g = c["g"]
    uploaded = (capi.AOS2_OK, capi.AOS2_ERR_NO_DEVICE)
    ARG = capi.AOS2_ERR_ARG

    def refused(fn, *a, **kw):
        with pytest.raises(capi.AosError) as e:
            fn(*a, **kw)
        assert e.value.code == ARG, (a, kw)

    m = capi.LocalMap()
    refused(m.update_connections, [0])                                  # no graph is set
    assert m.set(g, ok=uploaded) in uploaded
    tap = capi.LocalMap.update_connections_host
    for call in (m.update_connections, lambda *a, **kw: tap(g, *a, **kw)):
        refused(call, [0], th=0)                                        # th < 1
        refused(call, [0], conn_cap=-1)
        refused(call, [0], ordered_cap=-1)
        refused(call, [4])                                              # a row out of range
        refused(call, [-1])                                             # -1 needs explicit matches
        refused(call, [4], mp=[[0]])
        refused(call, [-2], mp=[[0]])
        refused(call, [0], mp=[[0, 1, 2]], mp_cap=2)                    # n_mp above mp_cap
        refused(call, [0], mp=[[0, -2]])                                # an entry below -1
    L = capi.lib()
    p = capi._p
    keep = [np.zeros(1, np.int32)]
    gs = capi._local_map_graph(g, keep)
    kf, one, mp = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(4, np.int32)
    out = [np.zeros(4, np.int32) for _ in range(6)]
    nc, ck, cw, no, ok_, ow = (p(a) for a in out)
    for fn, first in ((L.aos2_local_map_update_connections, m.h), (L.aos2_debug_update_connections_host, C.byref(gs))):
        assert fn(first, 3, -1, p(kf), None, None, 0, nc, ck, cw, 4, no, ok_, ow, 4) == ARG          # a negative count
        assert fn(first, 3, 1, p(kf), None, None, -1, nc, ck, cw, 4, no, ok_, ow, 4) == ARG         # a negative capacity
        assert fn(first, 3, 1, None, None, None, 0, nc, ck, cw, 4, no, ok_, ow, 4) == ARG           # NULL arrays with a length
        assert fn(first, 3, 1, p(kf), None, None, 0, None, ck, cw, 4, no, ok_, ow, 4) == ARG
        assert fn(first, 3, 1, p(kf), None, None, 0, nc, ck, cw, 4, None, ok_, ow, 4) == ARG
        assert fn(first, 3, 1, p(kf), None, None, 0, nc, None, cw, 4, no, ok_, ow, 4) == ARG
        assert fn(first, 3, 1, p(kf), None, None, 0, nc, ck, None, 4, no, ok_, ow, 4) == ARG
        assert fn(first, 3, 1, p(kf), None, None, 0, nc, ck, cw, 4, no, None, ow, 4) == ARG
        assert fn(first, 3, 1, p(kf), None, None, 0, nc, ck, cw, 4, no, ok_, None, 4) == ARG
        assert fn(first, 3, 1, p(kf), None, None, 4, nc, ck, cw, 4, no, ok_, ow, 4) == ARG          # mp NULL with room for matches
        assert fn(first, 3, 1, p(kf), p(one), None, 4, nc, ck, cw, 4, no, ok_, ow, 4) == ARG        # n_mp without mp
        assert fn(first, 3, 1, p(kf), None, p(mp), 4, nc, ck, cw, 4, no, ok_, ow, 4) == ARG         # mp without n_mp
        one[0] = -1
        assert fn(first, 3, 1, p(kf), p(one), p(mp), 4, nc, ck, cw, 4, no, ok_, ow, 4) == ARG       # n_mp below 0
        one[0] = 1
    assert L.aos2_local_map_update_connections(None, 3, 0, None, None, None, 0, None, None, None, 0, None, None, None, 0) == ARG
    m.debug_limits(scratch_bytes=12 * 4 + 15)                           # ONE keyframe's scratch (12 n_keyframes + 16) above the bound
    refused(m.update_connections, [0])
    m.debug_limits()
    with pytest.raises(capi.AosError) as e:                             # the sort hook: at most 2048 entries in LDS
        m.debug_connections_sort(2049)
    assert e.value.code == ARG
    m.debug_connections_sort(1)
    m.debug_connections_sort(0)
    # n == 0 is valid, needs no device, and with capacities of 0 every array may be NULL
    r = m.update_connections([])
    assert len(r["n_conn"]) == 0 and r["conn_kf"].shape == (0, 256) and m.last_connections_device_ms() == -1
    assert L.aos2_local_map_update_connections(m.h, 3, 0, None, None, None, 0, None, None, None, 0, None, None, None, 0) == capi.AOS2_OK
    # the host tap checks the graph as aos2_local_map_set does
    bad = dict(g)
    bad["obs_kf"] = g["obs_kf"].copy()
    bad["obs_kf"][0] = 4
    refused(tap, bad, [0])
    # the handle is still usable
    assert m.graph()["n_keyframes"] == 4
    m.close()
