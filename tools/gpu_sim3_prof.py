"""Stage driver: one aos2_sim3_ransac call of a loop-closure shape -- 5 candidate keyframes, 150-300 correspondences each, 30 %
outliers, SetRansacParameters(0.99, 20, 300), so ransac_max_its = 300 for every candidate -- timed as wall time around the C call
and as device time of its three kernels (HIP events of the handle); one JSON line.  Per kernel:
rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_sim3_prof.py (a run of its own; tools/kstats.py prints
the csv).  SIM3_REPS = timed calls; SIM3_HOST=1 also times aos2_debug_sim3_host, this repository's own C++ routine on one core (it stops at first_success, so its time depends on the
draws; the reference's Sim3Solver, which allocates a cv::Mat per projected point, is not what it measures)."""
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
capi = pkg.capi


def candidate(rng, n, fix_scale):
    """a planted Sim3 between two views of n points 1.5-8 m deep, 1 cm noise, 30 % of the correspondences unrelated"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.2, 0.5)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm = np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * (Kx @ Kx)
    box = lambda k: np.stack([rng.uniform(-2, 2, k), rng.uniform(-1.5, 1.5, k), rng.uniform(1.5, 8.0, k)], 1)   # noqa: E731
    X1 = box(n)
    X2 = (X1 - rng.uniform(-0.4, 0.4, 3)) @ Rm / (1.0 if fix_scale else 1.3)
    out = rng.permutation(n)[: int(0.3 * n)]
    X2[out] = box(len(out))
    sigma2 = np.float32(1.2) ** (2 * rng.integers(0, 8, (2, n)))
    return dict(X3Dc1=X1 + rng.normal(scale=0.01, size=X1.shape), X3Dc2=X2 + rng.normal(scale=0.01, size=X2.shape),
                max_err1=(9.210 * sigma2[0]).astype(np.float32), max_err2=(9.210 * sigma2[1]).astype(np.float32),
                K1=(520.9, 521.0, 325.1, 249.7), K2=(535.4, 539.2, 320.1, 247.6), fix_scale=fix_scale, probability=0.99, min_inliers=20,
                max_iterations=300, draws=capi.sim3_draws(rng, n, 300))


rng = np.random.default_rng(7)
problems = [candidate(rng, n, k % 2 == 0) for k, n in enumerate((150, 190, 230, 270, 300))]
M = capi.Matcher(0.75, True, device=0)
res = M.Sim3Ransac(problems)
P, R, keep, outs = capi._sim3_args(problems)
wall, dev = [], []
n_rep = int(os.environ.get("SIM3_REPS", "30"))
for it in range(n_rep + 5):
    t0 = time.perf_counter()
    st = M.L.aos2_sim3_ransac(M.h, P, R, len(problems))
    t1 = time.perf_counter()
    assert st == 0
    if it >= 5:
        wall.append((t1 - t0) * 1e3)
        dev.append(M.last_device_ms())
out = dict(candidates=len(problems), n=[len(p["X3Dc1"]) for p in problems], ransac_max_its=[r["ransac_max_its"] for r in res],
           hypotheses=int(sum(r["ransac_max_its"] for r in res)), first_success=[r["first_success"] for r in res],
           best_inliers=[r["best_inliers"] for r in res], wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)),
           wall_ms_max=float(np.max(wall)), kernels_ms_median=float(np.median(dev)), kernels_ms_min=float(np.min(dev)))
if os.environ.get("SIM3_HOST"):
    host = []
    for it in range(5):
        t0 = time.perf_counter()
        assert M.L.aos2_debug_sim3_host(P, R, len(problems)) == 0
        host.append((time.perf_counter() - t0) * 1e3)
    out["own_host_routine_one_core_ms_median"] = float(np.median(host))
print(json.dumps(out))
