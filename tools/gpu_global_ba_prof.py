"""Stage driver: aos2_global_bundle_adjustment on generator maps (tests/global_ba_ref.py big_map: keyframes on a circle, 10^5 stereo
points, 8 observations each: a banded reduced system) of 300 and 1 500 keyframes, and 1 500 with the loop closed, 10 iterations, not
robust (LoopClosing::RunGlobalBundleAdjustment's form), one map per call -- timed as device time of the whole call (HIP events of the
handle: upload done to last kernel done, the per-iteration reads of the control words included) and as wall time around the C call
(the symbolic phase on the host included); in a second, profiled set of calls the device time per kernel family (events around every
family of launches, which slows the call down: those figures are not part of the first two).  Beside the 300-keyframe map:
aos2_debug_global_ba_host, this repository's own header with a skyline solve on one core of the same box.  One line per map.
GBA_REPS = timed calls."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import global_ba_ref as R  # noqa: E402

pkg = g.load_package()
capi = pkg.capi
L = capi.LocalBA(device=0)
n_rep = int(os.environ.get("GBA_REPS", "5"))
n_points = int(os.environ.get("GBA_POINTS", "100000"))
print("# aos2_global_bundle_adjustment: one map per call, 10 iterations, not robust; device ms and wall ms of the call (medians of %d calls)," % n_rep)
print("# device ms per kernel family from profiled calls (linearise+sums, landmarks+update, assemble, factor_solve, begin+trial_edges+decide,")
print("# prepare+finish), aos2_debug_global_ba_host on one core")
print("# keyframes loop  points   edges  h_blocks  l_blocks  iterations  trials  device_ms  wall_ms  | lin_ms  landmark_ms  asm_ms  factor_ms  trial_ms  ends_ms | host_one_core_ms")
for n, loop in ((300, False), (1500, False), (1500, True)):
    P = R.big_map(n, n_points, loop=loop)
    res = L.GlobalBundleAdjustment(P, 10)
    wall, dev, fam = [], [], []
    for it in range(n_rep + 1):
        t0 = time.perf_counter()
        r = L.GlobalBundleAdjustment(P, 10)
        t1 = time.perf_counter()
        if it >= 1:
            wall.append((t1 - t0) * 1e3)
            dev.append(r["ms_device"])
    L.global_ba_profile(True)
    for it in range(3):
        L.GlobalBundleAdjustment(P, 10)
        fam.append(L.global_ba_profile(True))
    L.global_ba_profile(False)
    host = float("nan")
    if n <= 512:
        t = []
        for it in range(3):
            t0 = time.perf_counter()
            capi.debug_global_ba_host(P, 10)
            t.append((time.perf_counter() - t0) * 1e3)
        host = np.median(t)
    f = np.median(np.array(fam), axis=0)
    print("%5d %d %7d %7d %7d %7d %3d %3d %10.3f %10.3f | %8.3f %8.3f %8.3f %10.3f %8.3f %8.3f | %10.3f" % (
        n, loop, P["n_points"], P["n_edges"], res["h_blocks"], res["l_blocks"], res["iterations"], res["trials"], np.median(dev), np.median(wall),
        f[0], f[1], f[2], f[3], f[4], f[5], host), flush=True)
