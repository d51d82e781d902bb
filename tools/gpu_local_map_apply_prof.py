"""Stage driver: aos2_local_map_apply on the map of tools/gpu_local_map_prof.py / gpu_keyframe_culling_prof.py -- LA_KFS (1 000)
keyframes of 1 000 features along a trajectory, LA_POINTS (10^5) points, 700 000 observations, with the culling view -- for three
deltas:
  small       no keyframe appended: 70 point rows that gain an observation of the last keyframe, 10 appended points, 5 link rows
  insertion   ONE keyframe inserted: 1 appended keyframe of 1 000 features, 700 of them matched (600 to existing points, 100 to
              appended points), so 700 point rows that gain an observation, 50 link rows (the keyframe and its neighbours)
  large       ten times the rows: 10 appended keyframes, 1 000 appended points, 7 000 point rows, 500 link rows
Every repetition starts from the same resident map (aos2_local_map_set + aos2_local_map_set_culling_view, which are timed on the
FINAL graph of each delta for comparison: they are what a caller pays without the delta call).  Per delta, medians of LA_REPS (20):
wall time around aos2_local_map_apply and its device time between two events on the handle's stream (from the delta's upload to
the last kernel), the bytes uploaded, the lazy download separately (the first aos2_local_map_get behind the call, against a second
one), and the wall time of the forced host path (aos2_debug_local_map_apply_host).  The graph and view that the device rebuild
leaves are compared with the host path's, exactly.  One JSON line.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_local_map_apply_prof.py (a run of its own)."""
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
FEATS = 1000


def synthetic_map(rng, nk, npnt, feats=FEATS, matched=700):
    """the graph of tools/gpu_local_map_prof.py (the same draws), and a view over it"""
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
                kf_depth=rng.random(nk * feats).astype(np.float32) * 4, kf_stereo=(rng.random(nk * feats) < 0.3).astype(np.uint8),
                kf_th_depth=np.full(nk, 2.0, np.float32), kf_flags=np.zeros(nk, np.uint8))
    return graph, view


def make_delta(rng, graph, view, n_new_kfs, per_kf_existing, per_kf_new_points, n_link_rows):
    """n_new_kfs keyframes appended behind the map (none: the points gain an observation of the LAST keyframe's spare features),
    each matched to per_kf_existing existing points of the map's end and to per_kf_new_points appended points"""
    nk, npnt = graph["n_keyframes"], graph["n_points"]
    off, okf, oidx = graph["obs_off"], graph["obs_kf"], view["obs_idx"]
    writers = list(range(nk, nk + n_new_kfs)) if n_new_kfs else [nk - 1]
    pool = rng.permutation(np.arange(npnt - 20000, npnt - 1300))[:len(writers) * per_kf_existing]   # (points the last keyframe does not see)
    rows, lists = [], {}
    mp_rows, mp, octave, depth, stereo = [], [], [], [], []
    for j, k in enumerate(writers):
        old = pool[j * per_kf_existing:(j + 1) * per_kf_existing]
        new = npnt + j * per_kf_new_points + np.arange(per_kf_new_points)
        if n_new_kfs:
            feat = rng.permutation(FEATS)[:len(old) + len(new)]
            row = np.full(FEATS, -1, np.int32)
            row[feat] = np.concatenate([old, new])
            mp_rows.append(k)
            mp.append(row)
            octave.append(rng.integers(0, 8, FEATS).astype(np.int8))
            depth.append(rng.random(FEATS).astype(np.float32) * 4)
            stereo.append((rng.random(FEATS) < 0.3).astype(np.uint8))
        else:   # the last keyframe's match row is not changed: the observations name features of it
            feat = rng.permutation(FEATS)[:len(old) + len(new)]
        for p, f in zip(np.concatenate([old, new]), feat):
            p = int(p)
            a, b = (off[p], off[p + 1]) if p < npnt else (0, 0)
            lists[p] = (list(okf[a:b]) + [k], list(oidx[a:b]) + [int(f)])
    rows = sorted(lists)
    n_app_points = len(writers) * per_kf_new_points
    d = dict(n_points=npnt + n_app_points, n_keyframes=nk + n_new_kfs, point_row=np.array(rows, np.int32),
             point_bad=np.zeros(len(rows), np.uint8), point_nobs=np.array([len(lists[p][0]) for p in rows], np.int32),
             obs_off=np.cumsum([0] + [len(lists[p][0]) for p in rows]).astype(np.int32),
             obs_kf=np.array([x for p in rows for x in lists[p][0]], np.int32),
             kf_mp_row=np.array(mp_rows, np.int32), kf_mp_off=(np.arange(len(mp_rows) + 1) * FEATS).astype(np.int32),
             kf_mp=np.concatenate(mp) if mp else np.zeros(0, np.int32))
    # link rows: the appended keyframes and the rows in front of them -- the new keyframes enter the covisibility lists, the
    # spanning tree goes on in a chain
    nk1 = nk + n_new_kfs
    link = np.arange(nk1 - n_link_rows, nk1, dtype=np.int32)
    best = np.full((len(link), 10), -1, np.int32)
    for i, k in enumerate(link):
        cand = [k + dd for dd in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5) if 0 <= k + dd < nk1]
        best[i, :len(cand)] = cand
    child = [[k + 1] if k + 1 < nk1 else [] for k in link]
    d.update(kf_link_row=link, kf_bad=np.zeros(len(link), np.uint8), kf_best=best.reshape(-1),
             kf_child_off=np.cumsum([0] + [len(c) for c in child]).astype(np.int32), kf_child=np.array([c for r in child for c in r], np.int32),
             kf_parent=(link - 1).astype(np.int32))
    d["view"] = dict(obs_idx=np.array([x for p in rows for x in lists[p][1]], np.int32),
                     kf_octave=np.concatenate(octave) if mp else np.zeros(0, np.int8),
                     kf_depth=np.concatenate(depth) if mp else np.zeros(0, np.float32),
                     kf_stereo=np.concatenate(stereo) if mp else np.zeros(0, np.uint8),
                     kf_th_depth=np.full(len(link), 2.0, np.float32), kf_flags=np.zeros(len(link), np.uint8))
    return d


def med(x):
    return float(np.median(x))


def main():
    nk, npnt = int(os.environ.get("LA_KFS", "1000")), int(os.environ.get("LA_POINTS", "100000"))
    reps = int(os.environ.get("LA_REPS", "20"))
    rng = np.random.default_rng(5)
    graph, view = synthetic_map(rng, nk, npnt)
    capi = pkg.capi
    L = capi.lib()
    out = dict(keyframes=nk, points=npnt, observations=int(graph["obs_off"][-1]), reps=reps)
    deltas = (("small", make_delta(rng, graph, view, 0, 60, 10, 5)), ("insertion", make_delta(rng, graph, view, 1, 600, 100, 50)),
              ("large", make_delta(rng, graph, view, 10, 600, 100, 500)))
    lm = capi.LocalMap()
    for name, d in deltas:
        keep = [np.zeros(1, np.int32)]
        s = capi._local_map_delta(d, keep)
        gs = capi._LocalMapGraph()
        wall, dev, get_first, get_second, host_wall, nbytes, realloc = [], [], [], [], [], 0, 0
        final = None
        for it in range(reps + 3):
            lm.set(graph)
            lm.set_culling_view(view)
            t0 = time.perf_counter()
            st = L.aos2_local_map_apply(lm.h, C.byref(s))
            t1 = time.perf_counter()
            assert st == 0, st
            la = lm.last_apply()
            assert la["path"] == 1
            t2 = time.perf_counter()
            L.aos2_local_map_get(lm.h, C.byref(gs))   # the lazy download of graph and view
            t3 = time.perf_counter()
            L.aos2_local_map_get(lm.h, C.byref(gs))
            t4 = time.perf_counter()
            if it >= 3:
                wall.append((t1 - t0) * 1e3)
                dev.append(la["device_ms"])
                get_first.append((t3 - t2) * 1e3)
                get_second.append((t4 - t3) * 1e3)
                realloc += la["reallocated"]
            nbytes = la["bytes"]
        final = (lm.graph(), lm.view())
        for it in range(5):   # the forced host path on the same resident map
            lm.set(graph)
            lm.set_culling_view(view)
            t0 = time.perf_counter()
            st = L.aos2_debug_local_map_apply_host(lm.h, C.byref(s))
            host_wall.append((time.perf_counter() - t0) * 1e3)
            assert st == 0 and lm.last_apply()["path"] == 0
        hg, hv = lm.graph(), lm.view()
        assert all(np.array_equal(final[0][k], hg[k]) for k in hg) and all(final[1][k].tobytes() == hv[k].tobytes() for k in hv)
        assert hg["n_points"] == d["n_points"] and hg["n_keyframes"] == d["n_keyframes"]
        t_set, t_view = [], []
        fresh = capi.LocalMap()
        for it in range(8):   # what the caller pays without the delta call: set + view of the same final graph
            t0 = time.perf_counter()
            fresh.set(final[0])
            t1 = time.perf_counter()
            fresh.set_culling_view(final[1])
            t2 = time.perf_counter()
            t_set.append((t1 - t0) * 1e3)
            t_view.append((t2 - t1) * 1e3)
        fresh.close()
        out[name] = dict(point_rows=len(d["point_row"]), match_rows=len(d["kf_mp_row"]), link_rows=len(d["kf_link_row"]),
                         appended_points=d["n_points"] - npnt, appended_keyframes=d["n_keyframes"] - nk, bytes_uploaded=nbytes,
                         apply_wall_ms_median=med(wall), apply_wall_ms_min=float(np.min(wall)), apply_wall_ms_max=float(np.max(wall)),
                         apply_device_ms_median=med(dev), apply_device_ms_min=float(np.min(dev)), reallocated_calls=realloc,
                         lazy_download_ms_median=med(get_first), get_without_download_ms_median=med(get_second),
                         forced_host_wall_ms_median=med(host_wall[1:]),
                         set_ms_median=med(t_set[2:]), set_culling_view_ms_median=med(t_view[2:]),
                         set_plus_view_ms_median=med(np.array(t_set[2:]) + np.array(t_view[2:])))
    lm.close()
    print(json.dumps(out))


main()
