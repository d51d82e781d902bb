"""Stage driver: aos2_local_map_keyframe_culling on the map of tools/gpu_local_map_prof.py -- KC_KFS (1 000) keyframes along a
trajectory, KC_POINTS (10^5) points, a keyframe has 1 000 features, 700 of them matched to points of its stretch of the map, so
700 000 observations, about 7 per point -- for 20, 50 and 100 candidates (the rows around a keyframe in the middle of the map,
nearest first) with 0, 1 and 3 culls each.  The culls are planted through the octaves: every feature sits at level 4, except that a
candidate that is to stay has a fifth of its features at level 0, where fewer than three other observers pass the scale gate;
the candidates that are to go sit at a quarter, a half and three quarters of the list.  Every point's observations are walked
either way.  5 warm-up calls, then the median of KC_REPS (30) calls: wall time around the C call, device time between two events
on the handle's stream (aos2_local_map_last_culling_device_ms: the host's waits between enqueues are inside it).  Beside it
aos2_debug_keyframe_culling_host, the same per-item functions in the loop's own order on one core (median of 5): the tap checks
the whole graph and view on every call, so the time of a call with no candidates is taken off.  The outputs of the two are
compared, and the number of culls is asserted.  Also the time of one aos2_local_map_set_culling_view.  One JSON line.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_keyframe_culling_prof.py (a run of its own)."""
import ctypes as C
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
    """the graph of tools/gpu_local_map_prof.py (the same draws), and the feature of every observation"""
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
    graph = dict(n_points=npnt, n_keyframes=nk, point_bad=(rng.random(npnt) < 0.01).astype(np.uint8),
                 point_nobs=np.diff(obs_off).astype(np.int32), obs_off=obs_off, obs_kf=obs_kf,
                 kf_bad=(rng.random(nk) < 0.01).astype(np.uint8), kf_mp_off=(np.arange(nk + 1) * feats).astype(np.int32), kf_mp=flat,
                 kf_best=best.reshape(-1), kf_child_off=np.minimum(np.arange(nk + 1), nk - 1).astype(np.int32),
                 kf_child=np.arange(1, nk, dtype=np.int32), kf_parent=np.arange(nk, dtype=np.int32) - 1)
    return graph, (order % feats).astype(np.int32)


def view_for(rng, graph, obs_idx, cand, go, feats=1000):
    nk = graph["n_keyframes"]
    octave = np.full((nk, feats), 4, np.int8)
    for j, k in enumerate(cand):
        if j not in go:
            octave[k, rng.random(feats) < 0.2] = 0
    return dict(obs_idx=obs_idx, kf_octave=octave.reshape(-1), kf_depth=np.ones(nk * feats, np.float32),
                kf_stereo=np.zeros(nk * feats, np.uint8), kf_th_depth=np.full(nk, 2.0, np.float32), kf_flags=np.zeros(nk, np.uint8))


def main():
    nk, npnt = int(os.environ.get("KC_KFS", "1000")), int(os.environ.get("KC_POINTS", "100000"))
    reps = int(os.environ.get("KC_REPS", "30"))
    rng = np.random.default_rng(5)
    graph, obs_idx = synthetic_map(rng, nk, npnt)
    capi = pkg.capi
    L = capi.lib()
    lm = capi.LocalMap()
    lm.set(graph)
    out = dict(keyframes=nk, points=npnt, observations=int(graph["obs_off"][-1]))
    mid = nk // 2
    near = [mid + d * s for d in range(1, nk) for s in (1, -1) if 0 <= mid + d * s < nk]
    t_view = []
    for n_cand in (20, 50, 100):
        cand = np.array(near[:n_cand], np.int32)
        for culls in (0, 1, 3):
            go = {0: (), 1: (n_cand // 2,), 3: (n_cand // 4, n_cand // 2, 3 * n_cand // 4)}[culls]
            view = view_for(rng, graph, obs_idx, cand, go)
            t0 = time.perf_counter()
            lm.set_culling_view(view)
            t_view.append((time.perf_counter() - t0) * 1e3)
            status, n_mps, n_red = np.zeros(n_cand, np.uint8), np.zeros(n_cand, np.int32), np.zeros(n_cand, np.int32)
            bad, nb = np.zeros(npnt, np.int32), C.c_int32(0)
            wall, dev = [], []
            for it in range(reps + 5):
                t0 = time.perf_counter()
                st = L.aos2_local_map_keyframe_culling(lm.h, 1, n_cand, capi._p(cand), capi._p(status), capi._p(n_mps), capi._p(n_red),
                                                       capi._p(bad), npnt, C.byref(nb))
                t1 = time.perf_counter()
                assert st == 0, capi.last_error() if hasattr(capi, "last_error") else st
                if it >= 5:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(lm.last_culling_device_ms())
            th, tc = [], []
            for it in range(6):
                t0 = time.perf_counter()
                capi.LocalMap.keyframe_culling_host(graph, view, [], True)
                t1 = time.perf_counter()
                h = capi.LocalMap.keyframe_culling_host(graph, view, cand, True)
                t2 = time.perf_counter()
                tc.append((t1 - t0) * 1e3)
                th.append((t2 - t1) * 1e3 - (t1 - t0) * 1e3)
            assert np.array_equal(h["status"], status) and np.array_equal(h["n_mps"], n_mps) and np.array_equal(h["n_redundant"], n_red)
            assert h["n_bad_points"] == nb.value and np.array_equal(h["bad_points"][:nb.value], bad[:nb.value])
            assert int((status == capi.KFC_CULLED).sum()) == culls, (n_cand, culls, list(status))
            assert [j for j in range(n_cand) if status[j] == capi.KFC_CULLED] == list(go)
            out["cand_%d_culls_%d" % (n_cand, culls)] = dict(
                rounds=lm.last_culling_rounds(), bad_points=int(nb.value), redundant_share_mean=float((n_red / np.maximum(n_mps, 1)).mean()),
                wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
                device_ms_median=float(np.median(dev)), device_ms_min=float(np.min(dev)),
                own_host_routine_one_core_ms_median=float(np.median(th[1:])), host_check_ms_median=float(np.median(tc[1:])))
    out["set_culling_view_ms_median"] = float(np.median(t_view[1:]))
    lm.close()
    print(json.dumps(out))


main()
