"""Stage driver: aos2_optimize_essential_graph on generator graphs (tests/essential_graph_ref.py: a keyframe chain with a spanning
tree, 5-9 covisible earlier keyframes, one loop and an earlier one; about 8 edges per keyframe, 10^5 map points) of 300, 1 500 and
5 000 keyframes, one problem per call -- timed as device time of the whole call (HIP events of the handle: upload done to last kernel
done, the per-iteration reads of the control words included) and as wall time around the C call; in a second, profiled set of calls
the device time per kernel family (events around every launch, which slows the call down: those figures are not part of the first
two).  Beside the 300-keyframe graph: aos2_debug_essential_graph_host, this repository's own header with a skyline solve on one
core of the same box.  One line per graph.  EG_REPS = timed calls."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import essential_graph_ref as R  # noqa: E402

pkg = g.load_package()
capi = pkg.capi
L = capi.LocalBA(device=0)
n_rep = int(os.environ.get("EG_REPS", "5"))
print("# aos2_optimize_essential_graph: one graph per call; device ms and wall ms of the call (medians of %d calls), device ms per kernel" % n_rep)
print("# family from profiled calls (perturb+linearise, assemble, factor_solve, begin+trial, finish), aos2_debug_essential_graph_host on one core")
print("# keyframes  edges  points  l_blocks  iterations  trials  device_ms  wall_ms  | lin_ms  asm_ms  factor_ms  trial_ms  finish_ms | host_one_core_ms")
for n in (300, 1500, 5000):
    P = R.problem(7, n, False, n_points=100000, more=3)
    res = L.optimize_essential_graph([P])[0]
    Pc, Rc, keep, outs = capi._essential_graph_args([P])
    wall, dev, fam = [], [], []
    for it in range(n_rep + 1):
        t0 = time.perf_counter()
        st = L.L.aos2_optimize_essential_graph(L.h, Pc, Rc, 1)
        t1 = time.perf_counter()
        assert st == 0
        if it >= 1:
            wall.append((t1 - t0) * 1e3)
            dev.append(L.essential_graph_last_device_ms())
    L.essential_graph_profile(True)
    for it in range(3):
        assert L.L.aos2_optimize_essential_graph(L.h, Pc, Rc, 1) == 0
        fam.append(L.essential_graph_profile(True))
    L.essential_graph_profile(False)
    host = float("nan")
    if n <= 512:
        t = []
        for it in range(3):
            t0 = time.perf_counter()
            assert L.L.aos2_debug_essential_graph_host(Pc, Rc, 1) == 0
            t.append((time.perf_counter() - t0) * 1e3)
        host = np.median(t)
    f = np.median(np.array(fam), axis=0)
    print("%5d %6d %7d %7d %3d %3d %10.3f %10.3f | %8.3f %8.3f %10.3f %8.3f %8.3f | %8.3f" % (
        n, len(P["v0"]), len(P["ref"]), res["l_blocks"], res["iterations"], res["trials"], np.median(dev), np.median(wall), f[0], f[1], f[2], f[3], f[4], host), flush=True)
