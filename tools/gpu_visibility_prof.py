"""Stage driver: aos2_vis_count calls on the reference's planner map (tests/golden/planner_map_s.npz, 2 681 points, the
camera(map_data, int) constants) and on random maps of 10^4 and 10^5 points around the same area, for 1, 64 and 4 096 states per call
drawn like the tests' (x in [-2, 6], y in [-3, 3], theta in [-pi, pi]), returning the counts: 5 warm-up calls, then the median of
VIS_REPS (30) calls, as wall time around the C call and as device time of its three kernels (HIP events of the handle); one JSON line.
VIS_HOST=1 also times the same call through aos2_debug_visibility_host, this repository's own routine on one core, which runs the
reference's loop (median of 3 calls; one call where it takes seconds).  VIS_SIZES=2681,10000 picks the maps.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_visibility_prof.py (a run of its own)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g
pkg = g.load_package()
FLT_MAX = np.finfo(np.float32).max


def planner_map(rng, n):
    """-> xyz, upper, lower, max_range, min_range, found_ratio"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "planner_map_s.npz"))
    if n == len(z["xyz"]):
        return z["xyz"], z["upper"], z["lower"], np.full(n, FLT_MAX, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32)
    xyz = np.stack([rng.uniform(-5, 5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-4, 9, n)], 1)
    lower = rng.uniform(-np.pi, 0.5, n)
    return xyz, lower + rng.uniform(1.0, 4.0, n), lower, rng.uniform(2, 9, n), rng.uniform(0, 1.5, n), rng.uniform(0.2, 1.0, n)


def timed(V, states, host, reps):
    st = np.ascontiguousarray(states, np.float32)
    count = np.zeros(len(st), np.int32)
    p = pkg.capi._p
    wall, dev = [], []
    for it in range(reps + 5):
        t0 = time.perf_counter()
        rc = V.L.aos2_vis_count(V.h, len(st), p(st), p(count), None, None)
        t1 = time.perf_counter()
        assert rc == 0
        if it >= 5:
            wall.append((t1 - t0) * 1e3)
            dev.append(V.last_device_ms())
    out = dict(states=len(st), visible_mean=float(count.mean()), states_above_20=int((count > 20).sum()),
               wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
               kernels_ms_median=float(np.median(dev)), kernels_ms_min=float(np.min(dev)))
    if host:
        want, t = count.copy(), []
        for it in range(3):
            t0 = time.perf_counter()
            assert V.L.aos2_debug_visibility_host(V.h, len(st), p(st), p(count), None, None) == 0
            t.append((time.perf_counter() - t0) * 1e3)
            if t[-1] > 2000:
                break
        assert (count == want).all()
        out["own_host_routine_one_core_ms_median"] = float(np.median(t))
    return out


def main():
    sizes = [int(s) for s in os.environ.get("VIS_SIZES", "2681,10000,100000").split(",")]
    host, reps = bool(os.environ.get("VIS_HOST")), int(os.environ.get("VIS_REPS", "30"))
    out = {}
    for n in sizes:
        rng = np.random.default_rng(11)
        V = pkg.Visibility(device=0)
        V.set_map(*planner_map(rng, n))
        states = np.stack([rng.uniform(-2, 6, 4096), rng.uniform(-3, 3, 4096), rng.uniform(-np.pi, np.pi, 4096)], 1)
        out["points_%d" % n] = {"states_%d" % k: timed(V, states[:k], host, reps) for k in (1, 64, 4096)}
        V.close()
    print(json.dumps(out))


main()
