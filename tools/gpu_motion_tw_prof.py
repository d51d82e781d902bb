"""Stage driver: aos2_svc_motions calls on the reference's planner map (tests/golden/planner_map_s.npz, 2 681 points, the
camera(map_data, int) constants) and obstacles (tests/golden/planner_obstacles.npz, 2 800), for 1, 2, 4, 8, 16, 256 and 4 096 motions per call
drawn like the tests' (a start that isValid accepts among states x in [-2, 6], y in [-3, 3], theta in [-pi, pi]; the goal 0.2-1.2 m
ahead within +-0.6 rad of the heading, its heading changed by +-0.5 rad), returning what RRT* asks for per neighbour: the verdict of
checkMotionTW and both motion costs.  5 warm-up calls, then the median of TW_REPS (30) calls, as wall time around the C call and as
device time between the handle's HIP events (the call's one host wait, for the state total, lies between them); one JSON line.
TW_HOST=1 also times the same call through aos2_debug_svc_motions_host, this repository's own routine on one core, which runs the
reference's loops (median of 3 calls; one call where it takes seconds), and checks that it returns the same bytes.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_motion_tw_prof.py (a run of its own)."""
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
FLT_MAX = np.finfo(np.float32).max


def checker():
    z = np.load(os.path.join(ROOT, "tests", "golden", "planner_map_s.npz"))
    n = len(z["xyz"])
    S = pkg.StateValidChecker(device=0)
    S.vis.set_map(z["xyz"], z["upper"], z["lower"], np.full(n, FLT_MAX, np.float32), np.zeros(n, np.float32), np.ones(n, np.float32))
    S.set_obstacles(np.load(os.path.join(ROOT, "tests", "golden", "planner_obstacles.npz"))["xy"], 0.1)
    return S


def draw(S, rng, nm):
    st = np.stack([rng.uniform(-2, 6, 2000), rng.uniform(-3, 3, 2000), rng.uniform(-np.pi, np.pi, 2000)], 1)
    starts = st[S.valid(st, host=True)["valid"] != 0]
    q1 = starts[rng.integers(len(starts), size=nm)]
    d, a = rng.uniform(0.2, 1.2, nm), q1[:, 2] + rng.uniform(-0.6, 0.6, nm)
    q2 = np.stack([q1[:, 0] + d * np.cos(a), q1[:, 1] + d * np.sin(a), q1[:, 2] + rng.uniform(-0.5, 0.5, nm)], 1)
    return np.ascontiguousarray(q1), np.ascontiguousarray(q2), len(starts)


def timed(S, q1, q2, host, reps):
    nm, p = len(q1), pkg.capi._p
    res = [dict(valid=np.zeros(nm, np.uint8), n_states=np.zeros(nm, np.int32), cost_length=np.zeros(nm), cost_camera=np.zeros(nm)) for _ in range(2)]
    outs = []
    for r in res:
        O = pkg.capi._SvcMotionsOut()
        for k, a in r.items():
            setattr(O, k, a.ctypes.data)
        outs.append(O)
    wall, dev = [], []
    for it in range(reps + 5):
        t0 = time.perf_counter()
        rc = S.L.aos2_svc_motions(S.h, nm, p(q1), p(q2), C.byref(outs[0]))
        t1 = time.perf_counter()
        assert rc == 0
        if it >= 5:
            wall.append((t1 - t0) * 1e3)
            dev.append(S.last_device_ms())
    out = dict(motions=nm, states=int(res[0]["n_states"].sum()), valid=int(res[0]["valid"].sum()),
               wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
               device_ms_median=float(np.median(dev)), device_ms_min=float(np.min(dev)))
    if host:
        t = []
        for it in range(3):
            t0 = time.perf_counter()
            assert S.L.aos2_debug_svc_motions_host(S.h, nm, p(q1), p(q2), C.byref(outs[1])) == 0
            t.append((time.perf_counter() - t0) * 1e3)
            if t[-1] > 2000:
                break
        assert all(res[0][k].tobytes() == res[1][k].tobytes() for k in res[0])
        out["own_host_routine_one_core_ms_median"] = float(np.median(t))
    return out


def main():
    host, reps = bool(os.environ.get("TW_HOST")), int(os.environ.get("TW_REPS", "30"))
    sizes = [int(s) for s in os.environ.get("TW_SIZES", "1,2,4,8,16,256,4096").split(",")]
    S = checker()
    q1, q2, starts = draw(S, np.random.default_rng(11), max(sizes))
    out = dict(map_points=S.vis.map_size(), obstacles=2800, starts=starts)
    for k in sizes:
        out["motions_%d" % k] = timed(S, q1[:k], q2[:k], host, reps)
    S.close()
    print(json.dumps(out))


main()
