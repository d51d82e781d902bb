"""Stage driver: aos2_local_map_update_normal_depth on the map of tools/gpu_update_connections_ms.py -- ND_KFS (1 000) keyframes
along a trajectory, ND_POINTS (10^5) points, 700 000 observations, about 7 per point -- with the culling view beside it (the feature
of every observation, an octave per feature), camera centres along a line and the points beside it.  Batches of 1 point, 5 000
points (the points of a LocalBA window: a stretch in the middle of the map) and all 10^5 points, each WITHOUT and WITH the
per-observation outputs (term_off, mNormalVectors, theta_sVector).  3 warm-up calls, then the median of ND_REPS (20) calls: wall time
around the C call alone (the arrays are made once), device time between two events on the handle's stream
(aos2_local_map_last_normal_depth_device_ms).  Beside it aos2_debug_update_normal_depth_host, the repository's own loop on one core
(median of 5; it is NOT the reference binary): the tap checks the whole graph and view on every call, so the time of a call with no
points is taken off.  The outputs of the two are compared bit for bit.  ND_LDS_TERMS sets the hook (aos2_local_map_debug_normal_depth)
for a run with the thetas in global scratch.  One JSON line.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_normal_depth_ms.py (a run of its own)."""
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
    """the graph of tools/gpu_update_connections_ms.py (the same draws) and a view for it"""
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
    view = dict(obs_idx=(order % feats).astype(np.int32), kf_octave=rng.integers(0, 8, nk * feats).astype(np.int8),
                kf_depth=np.ones(nk * feats, np.float32), kf_stereo=np.zeros(nk * feats, np.uint8), kf_th_depth=np.full(nk, 40, np.float32),
                kf_flags=np.zeros(nk, np.uint8))
    return graph, view


def main():
    nk, npnt = int(os.environ.get("ND_KFS", "1000")), int(os.environ.get("ND_POINTS", "100000"))
    reps = int(os.environ.get("ND_REPS", "20"))
    rng = np.random.default_rng(5)
    graph, view = synthetic_map(rng, nk, npnt)
    capi = pkg.capi
    lm = capi.LocalMap()
    lm.set(graph)
    lm.set_culling_view(view)
    lm.debug_normal_depth(int(os.environ.get("ND_LDS_TERMS", "-1")))
    # the cameras along x, the points along the same line a few metres off it
    centre = np.stack([np.linspace(0, 100, nk), rng.normal(0, 0.1, nk), rng.normal(0, 0.1, nk)], 1).astype(np.float32)
    world = np.stack([np.linspace(0, 100, npnt), rng.normal(0, 1, npnt), rng.uniform(2, 10, npnt)], 1).astype(np.float32)
    scale = (1.2 ** np.arange(8)).astype(np.float32)
    lens = np.diff(graph["obs_off"])
    out = dict(keyframes=nk, points=npnt, observations=int(graph["obs_off"][-1]), lds_terms=os.environ.get("ND_LDS_TERMS", "default"))
    mid = npnt // 2
    batches = [("points_1", np.array([mid])), ("points_5000", np.arange(mid - 2500, mid + 2500)), ("points_all", np.arange(npnt))]
    L = capi.lib()
    keep = [np.zeros(1, np.int32)]
    gs, vs = capi._local_map_graph(graph, keep), capi._kf_culling_view(view, keep)
    for name, rows in batches:
        rows = rows[rows < npnt].astype(np.int32)
        n = len(rows)
        ref_kf = graph["obs_kf"][np.minimum(graph["obs_off"][rows], len(graph["obs_kf"]) - 1)]   # the first observer (any row for an empty list)
        for with_terms in (False, True):
            term_off = np.concatenate([[0], np.cumsum(lens[rows])]).astype(np.int32) if with_terms else None
            args = (rows, world[rows], ref_kf, centre, scale)
            d_s, d_keep, d_out = capi._normal_depth_args(*args, term_off=term_off)
            h_s, h_keep, h_out = capi._normal_depth_args(*args, term_off=term_off)
            e_s, e_keep, e_out = capi._normal_depth_args(rows[:0], world[:0], ref_kf[:0], centre, scale)
            wall, dev = [], []
            for it in range(reps + 3):
                t0 = time.perf_counter()
                st = L.aos2_local_map_update_normal_depth(lm.h, capi.C.byref(d_s))
                t1 = time.perf_counter()
                assert st == 0, st
                if it >= 3:
                    wall.append((t1 - t0) * 1e3)
                    dev.append(lm.last_normal_depth_device_ms())
            th, tc = [], []
            for it in range(6):
                t0 = time.perf_counter()
                st0 = L.aos2_debug_update_normal_depth_host(capi.C.byref(gs), capi.C.byref(vs), capi.C.byref(e_s))
                t1 = time.perf_counter()
                st1 = L.aos2_debug_update_normal_depth_host(capi.C.byref(gs), capi.C.byref(vs), capi.C.byref(h_s))
                t2 = time.perf_counter()
                assert st0 == 0 and st1 == 0
                tc.append((t1 - t0) * 1e3)
                th.append((t2 - t1) * 1e3 - (t1 - t0) * 1e3)
            for k in d_out:
                a, b = d_out[k], h_out[k]
                same = a.view(np.uint32) == b.view(np.uint32) if a.dtype == np.float32 else a == b
                if a.dtype == np.float32:
                    same |= np.isnan(a) & np.isnan(b)
                assert same.all(), (name, k, int((~same).sum()))
            status = d_out["status"][:-1]
            out[name + ("_with_terms" if with_terms else "")] = dict(
                points=n, updated=int((status == capi.ND_UPDATED).sum()), observations=int(lens[rows].sum()), groups=lm.last_groups(),
                wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
                device_ms_median=float(np.median(dev)), device_ms_min=float(np.min(dev)),
                own_host_routine_one_core_ms_median=float(np.median(th[1:])), host_check_ms_median=float(np.median(tc[1:])))
    lm.close()
    print(json.dumps(out))


main()
