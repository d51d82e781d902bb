"""Stage driver: aos2_local_map_update_connections on the map of tools/gpu_local_map_prof.py -- UC_KFS (1 000) keyframes along a
trajectory, UC_POINTS (10^5) points, a keyframe has 1 000 features, 700 of them matched to points of its stretch of the map, so
700 000 observations, about 7 per point -- for batches of 1, 16 and 64 keyframes (the rows around the middle of the map) in the
resident form, one keyframe in the explicit form (the new keyframe of LocalMapping.cc:168, kf = -1), and a batch of 16 keyframes of
2 000 features (1 400 matched: the matches of two neighbouring rows) in the explicit form.  th = 15, capacities of 256.  3 warm-up
calls, then the median of UC_REPS (30) calls: wall time around the C call, device time between two events on the handle's stream
(aos2_local_map_last_connections_device_ms).  Beside it aos2_debug_update_connections_host, the repository's own loop on one core
(median of 5; it is NOT the reference binary): the tap checks the whole graph on every call, so the time of a call with no keyframes
is taken off.  The outputs of the two are compared.  UC_LDS_KFS / UC_LDS_SORT set the two hooks (aos2_local_map_debug_limits,
aos2_local_map_debug_connections_sort) for a run with the counters or the sort in global scratch.  One JSON line.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_update_connections_ms.py (a run of its own)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
pkg = g.load_package()


def synthetic_map(rng, nk, npnt, feats=1000, matched=700):
    """the graph of tools/gpu_local_map_prof.py (the same draws)"""
    span = min(npnt, 1200)   # the stretch of the map a keyframe sees
    centre = np.linspace(0, npnt - span, nk).astype(np.int64)
    kf_mp = np.full((nk, feats), -1, np.int32)
    for k in range(nk):
        kf_mp[k, rng.permutation(feats)[:matched]] = centre[k] + rng.permutation(span)[:matched]
    flat = kf_mp.reshape(-1)
    idx = np.flatnonzero(flat >= 0)
    order = idx[np.argsort(flat[idx], kind="stable")]
    obs_kf = (order // feats).astype(np.int32)
    obs_off = np.concatenate([[0], np.cumsum(np.bincount(flat[idx], minlength=npnt))]).astype(np.int32)
    best = np.full((nk, 10), -1, np.int32)
    for j, d in enumerate((1, -1, 2, -2, 3, -3, 4, -4, 5, -5)):
        r = np.arange(nk) + d
        best[:, j] = np.where((r >= 0) & (r < nk), r, -1)
    return dict(n_points=npnt, n_keyframes=nk, point_bad=(rng.random(npnt) < 0.01).astype(np.uint8),
                point_nobs=np.diff(obs_off).astype(np.int32), obs_off=obs_off, obs_kf=obs_kf,
                kf_bad=(rng.random(nk) < 0.01).astype(np.uint8), kf_mp_off=(np.arange(nk + 1) * feats).astype(np.int32), kf_mp=flat,
                kf_best=best.reshape(-1), kf_child_off=np.minimum(np.arange(nk + 1), nk - 1).astype(np.int32),
                kf_child=np.arange(1, nk, dtype=np.int32), kf_parent=np.arange(nk, dtype=np.int32) - 1)


def main():
    nk, npnt = int(os.environ.get("UC_KFS", "1000")), int(os.environ.get("UC_POINTS", "100000"))
    reps = int(os.environ.get("UC_REPS", "30"))
    rng = np.random.default_rng(5)
    graph = synthetic_map(rng, nk, npnt)
    capi = pkg.capi
    lm = capi.LocalMap()
    lm.set(graph)
    lm.debug_limits(0, int(os.environ.get("UC_LDS_KFS", "-1")))
    lm.debug_connections_sort(int(os.environ.get("UC_LDS_SORT", "0")))
    out = dict(keyframes=nk, points=npnt, observations=int(graph["obs_off"][-1]), lds_keyframes=os.environ.get("UC_LDS_KFS", "default"),
               lds_sort=os.environ.get("UC_LDS_SORT", "default"))
    mid = nk // 2
    near = [mid] + [mid + d * s for d in range(1, nk) for s in (1, -1) if 0 <= mid + d * s < nk]
    rows = graph["kf_mp"].reshape(nk, -1)
    batches = [("resident_%d" % n, near[:n], None) for n in (1, 16, 64)]
    batches.append(("explicit_new_keyframe_1", [-1], [rows[mid].tolist()]))
    batches.append(("explicit_2000_features_16", near[:16], [np.concatenate([rows[k], rows[min(k + 1, nk - 1)]]).tolist() for k in near[:16]]))
    L, p, cap, th15 = capi.lib(), capi._p, 256, capi.CONNECTIONS_TH
    keep = [np.zeros(1, np.int32)]
    gs = capi._local_map_graph(graph, keep)
    for name, kf, mp in batches:
        # the arrays once, the C calls alone inside the clock
        n = len(kf)
        kf_a = np.array(kf, np.int32)
        n_mp = mp_a = None
        mp_cap = 0
        if mp is not None:
            n_mp, mp_cap = np.array([len(x) for x in mp], np.int32), max(len(x) for x in mp)
            mp_a = np.full((n, mp_cap), -1, np.int32)
            for k, x in enumerate(mp):
                mp_a[k, :len(x)] = x
        r, h = ({k: np.full(n * (1 if k.startswith("n_") else cap), -7, np.int32)
                 for k in ("n_conn", "n_ordered", "conn_kf", "conn_w", "ordered_kf", "ordered_w")} for _ in range(2))

        def call(fn, first, o, count):
            return fn(first, th15, count, p(kf_a), None if mp is None else p(n_mp), None if mp is None else p(mp_a), mp_cap, p(o["n_conn"]),
                      p(o["conn_kf"]), p(o["conn_w"]), cap, p(o["n_ordered"]), p(o["ordered_kf"]), p(o["ordered_w"]), cap)
        wall, dev = [], []
        for it in range(reps + 3):
            t0 = time.perf_counter()
            st = call(L.aos2_local_map_update_connections, lm.h, r, n)
            t1 = time.perf_counter()
            assert st == 0, st
            if it >= 3:
                wall.append((t1 - t0) * 1e3)
                dev.append(lm.last_connections_device_ms())
        th, tc = [], []
        for it in range(6):
            t0 = time.perf_counter()
            st0 = call(L.aos2_debug_update_connections_host, capi.C.byref(gs), h, 0)
            t1 = time.perf_counter()
            st1 = call(L.aos2_debug_update_connections_host, capi.C.byref(gs), h, n)
            t2 = time.perf_counter()
            assert st0 == 0 and st1 == 0
            tc.append((t1 - t0) * 1e3)
            th.append((t2 - t1) * 1e3 - (t1 - t0) * 1e3)
        for k in r:
            assert np.array_equal(r[k], h[k]), (name, k)
        assert (r["n_conn"] > 0).all() and (r["n_conn"] <= cap).all()
        out[name] = dict(keyframes=len(kf), n_conn_mean=float(r["n_conn"].mean()), n_ordered_mean=float(r["n_ordered"].mean()),
                         wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
                         device_ms_median=float(np.median(dev)), device_ms_min=float(np.min(dev)),
                         own_host_routine_one_core_ms_median=float(np.median(th[1:])), host_check_ms_median=float(np.median(tc[1:])))
    lm.close()
    print(json.dumps(out))


main()
