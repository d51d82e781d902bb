"""Stage driver: aos2_frames_update_local_map on a synthetic map of LM_KFS (1 000) keyframes along a trajectory and LM_POINTS (10^5)
points -- a keyframe has 1 000 features, 700 of them matched to points of its stretch of the map, its 10 best covisibles are its
nearest rows, its parent the row before it; 1 % of the points and of the keyframes are bad -- for batches of 1, 64 and 512 frames
of 512 features, about 300 of them matched to points around one keyframe.  5 warm-up calls, then the median of LM_REPS (30) calls:
device time between two events on the batch's stream around the call's launches, wall time around the call and the wait that
follows it.  The same work through aos2_debug_local_map_host, this repository's own serial routine on one core (median of 3):
the tap checks the whole graph on every call, so the time of a call with no frames is taken off, and a batch of fewer than 256
frames is repeated inside one call up to 256 frames and the time divided.  Also the time of one
aos2_local_map_set of that graph (median of 5).  One JSON line.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_local_map_prof.py (a run of its own)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
pkg = g.load_package()
import torch  # noqa: E402

CAP, MATCHED = 512, 300


def synthetic_map(rng, nk, npnt, feats=1000, matched=700):
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
    parent = np.arange(nk, dtype=np.int32) - 1
    child = np.arange(1, nk, dtype=np.int32)
    child_off = np.minimum(np.arange(nk + 1), nk - 1).astype(np.int32)
    graph = dict(n_points=npnt, n_keyframes=nk, point_bad=(rng.random(npnt) < 0.01).astype(np.uint8),
                 point_nobs=np.diff(obs_off).astype(np.int32), obs_off=obs_off, obs_kf=obs_kf,
                 kf_bad=(rng.random(nk) < 0.01).astype(np.uint8), kf_mp_off=(np.arange(nk + 1) * feats).astype(np.int32), kf_mp=flat,
                 kf_best=best.reshape(-1), kf_child_off=child_off, kf_child=child, kf_parent=parent)
    return graph, centre, span


def frames_of(rng, B, centre, span):
    mp = np.full((B, CAP), -1, np.int32)
    for b in range(B):
        c = centre[int(rng.integers(0, len(centre)))]
        mp[b, rng.permutation(CAP)[:MATCHED]] = c + rng.integers(0, span, MATCHED)
    return np.full(B, CAP, np.int32), mp


def main():
    nk, npnt = int(os.environ.get("LM_KFS", "1000")), int(os.environ.get("LM_POINTS", "100000"))
    reps = int(os.environ.get("LM_REPS", "30"))
    rng = np.random.default_rng(5)
    graph, centre, span = synthetic_map(rng, nk, npnt)
    capi, dev = pkg.capi, torch.device("cuda", 0)
    lm = capi.LocalMap()
    t_set = []
    for _ in range(6):
        t0 = time.perf_counter()
        lm.set(graph)
        t_set.append((time.perf_counter() - t0) * 1e3)
    out = dict(keyframes=nk, points=npnt, observations=int(graph["obs_off"][-1]), set_ms_median=float(np.median(t_set[1:])))
    ex = capi.Extractor(nfeatures=500)
    local_cap, kf_cap = 16384, 128
    tc = []
    for _ in range(6):
        t0 = time.perf_counter()
        capi.LocalMap.host(graph, np.zeros(0, np.int32), np.zeros((0, CAP), np.int32), local_cap, kf_cap)
        tc.append((time.perf_counter() - t0) * 1e3)
    check_ms = float(np.median(tc[1:]))
    out["host_graph_check_ms"] = check_ms
    for B in (1, 64, 512):
        n, mp = frames_of(rng, B, centre, span)
        f = capi.Frames(B, CAP)
        keep = (torch.zeros((B, CAP, 7), dtype=torch.float32, device=dev), torch.zeros((B, CAP, 32), dtype=torch.uint8, device=dev),
                torch.from_numpy(n).to(dev), torch.ones(npnt, dtype=torch.uint8, device=dev))
        f.build(ex, keep[0].data_ptr(), keep[1].data_ptr(), keep[2].data_ptr(), 640, 480, 0, 500.0, 500.0, 320.0, 240.0, 40.0)
        f.set_map_points(mp, capi.map_points_dev(npnt, 0, 0, keep[3].data_ptr()))
        d = [torch.full((B, local_cap), -9, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
             torch.full((B, kf_cap), -1, dtype=torch.int32, device=dev), torch.zeros(B, dtype=torch.int32, device=dev),
             torch.full((B,), -1, dtype=torch.int32, device=dev)]
        torch.cuda.synchronize()
        stream = torch.cuda.ExternalStream(f.stream(), device=dev)
        wall, devms = [], []
        for it in range(reps + 5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            lm.update(f, d[0].data_ptr(), local_cap, d[1].data_ptr(), d[2].data_ptr(), kf_cap, d[3].data_ptr(), d[4].data_ptr())
            e1.record(stream)
            f.wait()
            t1 = time.perf_counter()
            if it >= 5:
                wall.append((t1 - t0) * 1e3)
                devms.append(e0.elapsed_time(e1))
        got = [x.cpu().numpy() for x in d]
        th, tile = [], max(1, 256 // B)   # (small batches repeated inside one call, so that the check taken off is small beside it)
        for it in range(3):
            t0 = time.perf_counter()
            h = capi.LocalMap.host(graph, np.tile(n, tile), np.tile(mp, (tile, 1)), local_cap, kf_cap)
            th.append(((time.perf_counter() - t0) * 1e3 - check_ms) / tile)
        h = {k: v[:B] for k, v in h.items()}
        assert np.array_equal(h["local"], got[0]) and np.array_equal(h["n_local"], got[1]) and np.array_equal(h["local_kfs"], got[2])
        assert np.array_equal(h["n_local_kfs"], got[3]) and np.array_equal(h["ref_kf"], got[4])
        out["frames_%d" % B] = dict(local_points_mean=float(got[1].mean()), local_keyframes_mean=float(got[3].mean()), groups=lm.last_groups(),
                                    device_ms_median=float(np.median(devms)), device_ms_min=float(np.min(devms)),
                                    wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
                                    own_host_routine_one_core_ms_median=float(np.median(th)))
        f.close()
    lm.close()
    print(json.dumps(out))


main()
