"""Stage driver: aos2_optimize_sim3 on three batches of the generator's problems (tests/sim3_opt_ref.py: a planted Sim3, pixel noise
of 1.2^octave, 20 % gross outliers, a perturbed start) -- 5 problems x 150 correspondences (what LoopClosing::ComputeSim3 sees),
64 x 150, 1 x 300 -- timed as device time of the kernel (HIP events of the handle) and as wall time around the C call; beside it
the wall time of aos2_debug_sim3_opt_host, this repository's own header on one core of the same box (the reference's g2o graph,
which allocates per vertex and per edge, is not what it measures).  One line per batch.  SIM3_OPT_REPS = timed calls."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import sim3_opt_ref as R  # noqa: E402

pkg = g.load_package()
capi = pkg.capi
L = capi.LocalBA(device=0)
n_rep = int(os.environ.get("SIM3_OPT_REPS", "20"))
print("# aos2_optimize_sim3: device ms of the kernel (HIP events), wall ms of the call, and aos2_debug_sim3_opt_host on one core; medians of %d calls" % n_rep)
print("# problems  n  device_ms  wall_ms  host_one_core_ms  iterations(mean)  trials(mean)")
for count, n in ((5, 150), (64, 150), (1, 300)):
    problems = [R.problem(np.random.default_rng([11, count, k]), n, n // 5, k % 2 == 0, k % 3 == 0) for k in range(count)]
    res = L.OptimizeSim3(problems)
    P, Rc, keep, outs = capi._sim3_opt_args(problems)
    wall, dev, host = [], [], []
    for it in range(n_rep + 3):
        t0 = time.perf_counter()
        st = L.L.aos2_optimize_sim3(L.h, P, Rc, count)
        t1 = time.perf_counter()
        assert st == 0
        if it >= 3:
            wall.append((t1 - t0) * 1e3)
            dev.append(L.sim3_opt_last_device_ms())
    for it in range(5):
        t0 = time.perf_counter()
        assert L.L.aos2_debug_sim3_opt_host(P, Rc, count) == 0
        host.append((time.perf_counter() - t0) * 1e3)
    print("%3d %4d %8.3f %8.3f %8.3f %6.1f %6.1f" % (count, n, np.median(dev), np.median(wall), np.median(host),
                                                  np.mean([sum(r["iterations"]) for r in res]), np.mean([sum(r["trials"]) for r in res])))
