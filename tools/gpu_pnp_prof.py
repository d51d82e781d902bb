"""Stage driver: aos2_pnp_ransac calls of a relocalisation shape -- 5 candidate keyframes, 60-300 correspondences each, 40 % outliers,
SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) as Tracking::Relocalization sets them (35 iterations per candidate), and the same
candidates with epsilon = 0.2 (300 iterations each) -- timed as wall time around the C call and as device time of its five kernels
(HIP events of the handle); one JSON line.  Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python
tools/gpu_pnp_prof.py (a run of its own; tools/kstats.py prints the csv).  PNP_REPS = timed calls; PNP_HOST=1 also times
aos2_debug_pnp_host, this repository's own C++ routine on one core (it stops at returned_at, so its time depends on the draws; it
is not the reference's PnPsolver, which goes through OpenCV)."""
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
K = (517.3, 516.5, 318.6, 255.3)


def candidate(rng, n, epsilon):
    """n map points 3-8 m in front of a planted pose, their projections with 0.5 sigma of pixel noise, 40 % of them a random pixel"""
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    ang = rng.uniform(0.1, 0.6)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    Rm, t = np.eye(3) + math.sin(ang) * Kx + (1 - math.cos(ang)) * (Kx @ Kx), rng.uniform(-0.5, 0.5, 3)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3.0, 8.0, n)], 1)
    Xw = ((Xc - t) @ Rm).astype(np.float32)
    c = Xw.astype(np.float64) @ Rm.T + t
    sigma2 = (np.float32(1.2) ** (2 * rng.integers(0, 8, n))).astype(np.float32)
    uv = np.stack([K[0] * c[:, 0] / c[:, 2] + K[2], K[1] * c[:, 1] / c[:, 2] + K[3]], 1) + 0.5 * np.sqrt(sigma2)[:, None] * rng.normal(size=(n, 2))
    out = rng.permutation(n)[: int(0.4 * n)]
    uv[out] = np.stack([rng.uniform(0, 640, len(out)), rng.uniform(0, 480, len(out))], 1)
    mi, eps, its = capi.pnp_ransac_parameters(n, 0.99, 10, 300, 4, epsilon)
    its = max(its, 5)   # the first iterate(5)
    return dict(P3Dw=Xw, P2D=uv.astype(np.float32), max_err=sigma2 * np.float32(5.991), K=K, min_inliers=mi, min_set=4, n_iterations=its,
                draws=capi.pnp_draws(rng, n, its, 4))


def timed(M, problems, host):
    res = M.PnpRansac(problems)
    P, R, keep, outs = capi._pnp_args(problems)
    wall, dev = [], []
    for it in range(int(os.environ.get("PNP_REPS", "30")) + 5):
        t0 = time.perf_counter()
        st = M.L.aos2_pnp_ransac(M.h, P, R, len(problems))
        t1 = time.perf_counter()
        assert st == 0
        if it >= 5:
            wall.append((t1 - t0) * 1e3)
            dev.append(M.last_device_ms())
    out = dict(n=[len(p["P3Dw"]) for p in problems], n_iterations=[p["n_iterations"] for p in problems],
               hypotheses=int(sum(p["n_iterations"] for p in problems)), returned_at=[r["returned_at"] for r in res],
               n_inliers=[r["n_inliers"] for r in res], wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)),
               wall_ms_max=float(np.max(wall)), kernels_ms_median=float(np.median(dev)), kernels_ms_min=float(np.min(dev)))
    if host:
        t = []
        for it in range(5):
            t0 = time.perf_counter()
            assert M.L.aos2_debug_pnp_host(P, R, len(problems)) == 0
            t.append((time.perf_counter() - t0) * 1e3)
        out["own_host_routine_one_core_ms_median"] = float(np.median(t))
    return out


M = capi.Matcher(0.75, True, device=0)
host = bool(os.environ.get("PNP_HOST"))
out = dict(candidates=5)
for name, eps in (("relocalisation", 0.5), ("epsilon_0.2", 0.2)):
    rng = np.random.default_rng(7)
    out[name] = timed(M, [candidate(rng, n, eps) for n in (60, 120, 180, 240, 300)], host)
print(json.dumps(out))
