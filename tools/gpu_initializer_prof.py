"""Stage driver: aos2_initializer_initialize calls of the monocular-initialisation shape -- 1, 5 and 64 sequences of 300 and of 1000
matches (20 % gross outliers, 0.5 px noise, 200 unmatched keys per frame), 200 iterations each as Tracking.cc:675 sets them -- timed
as wall time around the C call and as device time of its seven kernels (HIP events of the handle); one JSON line.  Per kernel:
rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_initializer_prof.py (a run of its own; tools/kstats.py
prints the csv).  INIT_REPS = timed calls (after 5 warm-ups; medians are reported); INIT_HOST=1 also times
aos2_debug_initializer_host, this repository's own C++ routine on one core (it is not the reference's Initializer, which goes through
OpenCV and runs H and F on two threads)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
capi = pkg.capi


def sequence(seed, n):
    P = pkg.synth.synth_two_view(seed, ("general", "planar")[seed % 2], n_matches=n, n_extra=200, outlier_frac=0.2, noise=0.5, iterations=200)
    return {k: v for k, v in P.items() if k not in ("kind", "R21", "t21", "outlier")}


def timed(M, problems, host):
    res = M.InitializerInitialize(problems)
    P, R, keep, outs = capi._init_args(problems)
    wall, dev = [], []
    for it in range(int(os.environ.get("INIT_REPS", "30")) + 5):
        t0 = time.perf_counter()
        st = M.L.aos2_initializer_initialize(M.h, P, R, len(problems))
        t1 = time.perf_counter()
        assert st == 0
        if it >= 5:
            wall.append((t1 - t0) * 1e3)
            dev.append(M.last_device_ms())
    out = dict(problems=len(problems), n_matches=len(problems[0]["matches"]), hypotheses=400 * len(problems),
               initialized=int(sum(r["initialized"] for r in res)), used_homography=int(sum(r["used_homography"] for r in res)),
               wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)),
               kernels_ms_median=float(np.median(dev)), kernels_ms_min=float(np.min(dev)))
    if host:
        t = []
        for it in range(3 if len(problems) > 5 else 7):
            t0 = time.perf_counter()
            assert M.L.aos2_debug_initializer_host(P, R, len(problems)) == 0
            t.append((time.perf_counter() - t0) * 1e3)
        out["own_host_routine_one_core_ms_median"] = float(np.median(t))
    return out


M = capi.Matcher(0.9, True, device=0)
host = bool(os.environ.get("INIT_HOST"))
out = dict(iterations=200, cases=[])
for n in (300, 1000):
    for batch in (1, 5, 64):
        out["cases"].append(timed(M, [sequence(s, n) for s in range(batch)], host))
print(json.dumps(out))
