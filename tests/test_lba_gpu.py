"""HIP LocalBundleAdjustment vs the oracle.  Floating point (IEEE double inside, float32 at the
boundary like the reference): tolerance 1e-5 absolute on the float32 poses/points written back
(north_star), checked on top of the float32 quantisation of the stored value."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-5


def close(a, b, key=None):
    import parity   # oracle/parity.py: |a - b| <= 1e-5, literally; records the worst difference seen
    ok = parity.close(a, b, TOL, key=key)
    if not ok:
        print("worst |difference|:", parity.worst(a, b))
    return ok


@pytest.mark.parametrize("cfg", [dict(seed=1, n_local=3, n_fixed=2, n_points=60, stereo_frac=0.5),
                                 dict(seed=2, n_local=6, n_fixed=4, n_points=400, stereo_frac=0.0),
                                 dict(seed=4, n_local=5, n_fixed=0, n_points=300, include_kf0=True),
                                 dict(seed=0), dict(seed=3, include_kf0=True, outlier_frac=0.15)])
def test_lba_vs_oracle(pkg, oracle, gpu, cfg):
    prob = pkg.synth.synth_lba_problem(**cfg)
    want = oracle.lba_solve(prob)
    got = pkg.LocalBA().LocalBundleAdjustment(prob)
    assert got["status"] == 0 and got["iters"] == want["iters"]
    assert close(got["pose_Tcw"], want["pose_Tcw"])
    assert close(got["point_xyz"], want["point_xyz"])
    assert (got["edge_outlier"] == want["edge_outlier"]).all()
    assert abs(got["final_chi2"] - want["chi2_trace"][-1]) <= 1e-6 * want["chi2_trace"][-1]
    assert np.allclose(got["edge_chi2"], want["edge_chi2"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name", ["lba_3kf", "lba_14kf"])
def test_lba_golden(pkg, gpu, name):
    g = np.load(os.path.join(GOLD, name + ".npz"))
    prob = {k: g[k] for k in g.files if not k.startswith("out_")}
    for k in ("n_poses", "n_points", "n_edges"):
        prob[k] = int(prob[k])
    got = pkg.LocalBA().LocalBundleAdjustment(prob)
    assert close(got["pose_Tcw"], g["out_pose_Tcw"]) and close(got["point_xyz"], g["out_point_xyz"])
    assert (got["edge_outlier"] == g["out_outlier"]).all()


def test_lba_stop_flag_and_properties(pkg, oracle, gpu):
    prob = pkg.synth.synth_lba_problem(5, n_local=4, n_fixed=3, n_points=200)
    ba = pkg.LocalBA()
    flag = np.ones(1, np.uint8)
    r = ba.LocalBundleAdjustment(prob, stop_flag=flag)
    assert r["status"] == pkg.capi.AOS2_ERR_STOPPED and r["iters"] == (0, 0)
    assert (r["pose_Tcw"] == prob["pose_Tcw"]).all() and (r["point_xyz"] == prob["point_xyz"]).all()
    r = ba.LocalBundleAdjustment(prob)
    fixed = prob["pose_fixed"].astype(bool)
    assert np.abs(r["pose_Tcw"][fixed] - prob["pose_Tcw"][fixed]).max() < 1e-6   # fixed cameras do not move
    # a solved problem stays solved (idempotence up to the LM stop rule)
    p2 = dict(prob)
    p2["pose_Tcw"], p2["point_xyz"] = r["pose_Tcw"], r["point_xyz"]
    r2 = ba.LocalBundleAdjustment(p2)
    assert np.abs(r2["pose_Tcw"] - r["pose_Tcw"]).max() < 5e-2
    # iteration counts: only the first pass
    r3 = ba.LocalBundleAdjustment(prob, iters=(5, 0))
    w3 = oracle.lba_solve(prob, iters1=5, iters2=0)
    assert close(r3["pose_Tcw"], w3["pose_Tcw"]) and close(r3["point_xyz"], w3["point_xyz"])


def test_lba_degenerate_control_flow(pkg, oracle, gpu):
    """corners of the device-side control flow: no first optimisation (iterations 0: the outlier pass then sees zero
    residuals), no second one, and a window whose edges ALL leave at the outlier pass (initializeOptimization(0) finds no
    level-0 edge: the second optimisation never starts) -- same results, iteration counts and polls as the oracle"""
    prob = pkg.synth.synth_lba_problem(6, n_local=5, n_fixed=3, n_points=250)
    for it in ((0, 10), (3, 0), (0, 0), (1, 1)):
        got = pkg.LocalBA().LocalBundleAdjustment(prob, iters=it)
        want = oracle.lba_solve(prob, iters1=it[0], iters2=it[1])
        assert got["status"] == 0 and got["iters"] == want["iters"], it
        assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
        assert (got["edge_outlier"] == want["edge_outlier"]).all() and got["polls"] == want["polls"]
    bad = dict(prob)
    rng = np.random.default_rng(3)
    obs = prob["edge_obs"].copy()
    obs[:, :2] += rng.choice([-1.0, 1.0], (len(obs), 2)).astype(np.float32) * rng.uniform(60, 200, (len(obs), 2)).astype(np.float32)
    bad["edge_obs"] = obs
    got = pkg.LocalBA().LocalBundleAdjustment(bad)
    want = oracle.lba_solve(bad)
    assert got["iters"][0] == want["iters"][0] and (got["edge_outlier"] == want["edge_outlier"]).all()
    if want["chi2_trace"][-1] > 1e-18:   # (two edges left: the second optimisation drives chi2 to 1e-25 and stops on rounding noise)
        assert got["iters"] == want["iters"]
    assert want["edge_outlier"].mean() > 0.9   # (nearly) everything is an outlier
    assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])


# ---- Optimizer::PoseOptimization -----------------------------------------
@pytest.mark.parametrize("cfg", [dict(seed=0), dict(seed=1, stereo_frac=0.0, cfg="tum"), dict(seed=2, n=300, outlier_frac=0.3),
                                 dict(seed=3, n=2000), dict(seed=4, n=8), dict(seed=5, n=2), dict(seed=6, n=40, rot_err=0.05)])
def test_pose_optimization_vs_oracle(pkg, oracle, gpu, cfg):
    prob = pkg.synth.synth_pose_problem(**cfg)
    want = oracle.pose_optimization(prob)
    got = pkg.LocalBA().PoseOptimization(prob)
    assert got["n_inliers"] == want["n_inliers"] and got["n_bad"] == want["n_bad"]
    assert (got["outlier"] == want["outlier"]).all()
    assert close(got["Tcw"].reshape(1, 16), want["Tcw"].reshape(1, 16))


def test_pose_optimization_slot_count_boundaries(pkg, oracle, gpu):
    """The edge passes run a wave's edges K at a time, K = the slots the WAVE uses (pose_opt.h): correspondence counts around every
    change of a wave's slot count -- 64 w and 256 j + 64 w (+- 1) for the 256-thread kernel that keeps <= 4 edges per thread in
    registers, and beyond 1024 the kernel that leaves them in memory -- one call with all of them (problems of different sizes share a launch),
    with mono-only, stereo-only and mixed edges and enough outliers for edges to leave at every round."""
    ns = sorted(set(n for base in (64, 128, 192, 256, 320, 512, 576, 768, 832, 1024) for n in (base - 1, base, base + 1)) | {9, 10, 11, 33, 1025, 1500})
    probs = [pkg.synth.synth_pose_problem(8100 + i, n=n, stereo_frac=(0.0, 1.0, 0.6)[i % 3], outlier_frac=(0.05, 0.3)[i % 2], cfg=("tum", "kitti")[i % 2])
             for i, n in enumerate(ns)]
    small = [p for p in probs if p["n"] <= 1024]
    ba = pkg.LocalBA()
    got = ba.PoseOptimization(small) + [ba.PoseOptimization(p) for p in probs if p["n"] > 1024]
    for p, g in zip(small + [p for p in probs if p["n"] > 1024], got):
        want = oracle.pose_optimization(p)
        assert g["n_inliers"] == want["n_inliers"] and g["n_bad"] == want["n_bad"] and (g["outlier"] == want["outlier"]).all(), p["n"]
        assert close(g["Tcw"].reshape(1, 16), want["Tcw"].reshape(1, 16), key="po_slots"), p["n"]


def test_pose_optimization_fewer_than_three_correspondences(pkg, oracle, gpu):
    """nInitialCorrespondences < 3 (:355-356): pose unchanged, 0 inliers, and mvbOutlier all false -- also right after a
    call on the same handle that left outlier flags in the device arena (found by tools/gpu_fuzz_rest.py)."""
    ba = pkg.LocalBA()
    big = pkg.synth.synth_pose_problem(1, n=900, outlier_frac=0.5)
    assert ba.PoseOptimization(big)["outlier"].any()
    for seed in range(700, 720):
        for n in (1, 2):
            p = pkg.synth.synth_pose_problem(seed, n=n, stereo_frac=0.5)
            got, want = ba.PoseOptimization(p), oracle.pose_optimization(p)
            assert got["n_inliers"] == want["n_inliers"] == 0 and not got["outlier"].any() and not want["outlier"].any()
            assert got["Tcw"].tobytes() == p["Tcw"].astype(np.float32).tobytes()
        ba.PoseOptimization(big)


def test_pose_optimization_three_to_seven_correspondences(pkg, oracle, gpu):
    """The smallest systems PoseOptimization accepts (nInitialCorrespondences >= 3, :355-356), with outliers among them:
    the 6x6 system is close to singular, and still the float32 pose is within 1e-5 of the oracle (fixed-order sums: for
    n <= 32 the workgroup reduction adds the edges in g2o's insertion order)."""
    ba = pkg.LocalBA()
    rng = np.random.default_rng(5)
    for n in (3, 4, 5, 6, 7):
        for seed in range(60):
            p = pkg.synth.synth_pose_problem(3000 + seed, n=n, stereo_frac=float(rng.choice([0.0, 0.5, 1.0])),
                                             outlier_frac=float(rng.choice([0.0, 0.1, 0.4])), cfg=("kitti", "tum")[seed % 2])
            want, got = oracle.pose_optimization(p), ba.PoseOptimization(p)
            assert got["n_inliers"] == want["n_inliers"] and (got["outlier"] == want["outlier"]).all()
            assert close(got["Tcw"].reshape(1, 16), want["Tcw"].reshape(1, 16)), (n, seed)


def test_pose_solver_building_blocks(pkg, oracle, gpu):
    """pose_opt.h's serial path uses its own exp-map update (polynomial small-angle form, a general form beyond
    |omega|^2 = 0.6, the reference's first-order form below 1e-5 rad) and a square-root-free 6x6 solve: every branch against
    the oracle's se3quat restatement / numpy, to 1e-12 (they differ by rounding only)."""
    rng = np.random.default_rng(7)
    n = 4000
    ax = rng.normal(size=(n, 3)); ax /= np.linalg.norm(ax, axis=1, keepdims=True)
    ang = np.concatenate([10.0 ** rng.uniform(-9, -5.3, n // 4), 10.0 ** rng.uniform(-5, -1, n // 4), rng.uniform(0.05, 0.77, n // 4),
                          rng.uniform(0.78, 3.1, n - 3 * (n // 4))])   # tiny / small / moderate / general (all three trace branches)
    upd = np.concatenate([ax * ang[:, None], rng.normal(0, 0.5, (n, 3))], 1)
    q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True); q[q[:, 3] < 0] *= -1
    T = np.concatenate([q, rng.normal(0, 3.0, (n, 3))], 1)
    # SPD systems with a wide range of conditioning, plus a few indefinite ones
    Hb = np.zeros((n, 27)); lam = 10.0 ** rng.uniform(-8, 2, n); xs_want = np.zeros((n, 6)); ok_want = np.ones(n, np.uint8)
    iu = np.triu_indices(6)
    for i in range(n):
        A = rng.normal(size=(6, 6)) * 10.0 ** rng.uniform(-2, 3, 6)[None, :]
        H = A.T @ A
        if i % 97 == 0:
            H -= 2 * (np.trace(H) + lam[i]) * np.eye(6)   # not positive definite
            ok_want[i] = 0
        b = rng.normal(size=6) * np.sqrt(np.diag(np.abs(H)) + 1e-3)
        Hb[i, :21] = H[iu]; Hb[i, 21:] = b
        if ok_want[i]:
            xs_want[i] = np.linalg.solve(H + lam[i] * np.eye(6), b)
    x0 = np.full((n, 6), 7.25)
    To, xs, ok = pkg.capi.debug_pose_blocks_device(upd, T, Hb, lam, x0)
    assert (ok == ok_want).all()
    assert (xs[ok_want == 0] == 7.25).all()   # a failed solve leaves the solver's x alone
    good = ok_want == 1
    for i in np.nonzero(good)[0]:
        H = np.zeros((6, 6)); H[iu] = Hb[i, :21]; H = H + H.T - np.diag(np.diag(H)); H += lam[i] * np.eye(6)
        tol = 1e-13 * np.linalg.cond(H) * (np.abs(xs_want[i]).max() + 1e-300)
        assert np.abs(xs[i] - xs_want[i]).max() <= tol + 1e-300, (i, xs[i], xs_want[i])
    for i in range(n):
        want = oracle.se3_mul(oracle.se3_exp(upd[i]), T[i])
        assert np.abs(To[i] - want).max() < 1e-12 * (1 + np.abs(want).max()), (i, ang[i], To[i], want)


def test_pose_optimization_batch_and_golden(pkg, oracle, gpu):
    probs = [pkg.synth.synth_pose_problem(100 + i, n=600 + 37 * i) for i in range(24)]
    ba = pkg.LocalBA()
    res = ba.PoseOptimization(probs)
    for p, r in zip(probs, res):
        w = oracle.pose_optimization(p)
        assert r["n_inliers"] == w["n_inliers"] and (r["outlier"] == w["outlier"]).all()
        assert close(r["Tcw"].reshape(1, 16), w["Tcw"].reshape(1, 16))
    assert ba.pose_last_device_ms() > 0
    g = np.load(os.path.join(GOLD, "pose_500.npz"))
    prob = {k: g[k] for k in g.files if not k.startswith("out_")}
    prob["n"] = int(prob["n"])
    r = ba.PoseOptimization(prob)
    assert r["n_inliers"] == int(g["out_n_inliers"]) and (r["outlier"] == g["out_outlier"]).all()
    assert close(r["Tcw"].reshape(1, 16), g["out_Tcw"].reshape(1, 16))


def test_lba_concurrent_windows_from_threads(pkg, gpu):
    """Independent windows (one handle + one host thread each, SURVEY 8(e) "replicas only") solved at the same time
    give exactly the results of solving them one after the other: handles share nothing but the device."""
    import threading
    probs = [pkg.synth.synth_lba_problem(30 + i, n_local=4 + i, n_fixed=3, n_points=150 + 40 * i) for i in range(6)]
    serial = [pkg.LocalBA().LocalBundleAdjustment(q) for q in probs]
    handles = [pkg.LocalBA() for _ in probs]
    out = [None] * len(probs)

    def work(i):
        for _ in range(3):
            out[i] = handles[i].LocalBundleAdjustment(probs[i])

    ths = [threading.Thread(target=work, args=(i,)) for i in range(len(probs))]
    [t.start() for t in ths]
    [t.join() for t in ths]
    for a, b in zip(out, serial):
        assert a is not None and a["status"] == 0 and a["iters"] == b["iters"]
        assert (a["pose_Tcw"] == b["pose_Tcw"]).all() and (a["point_xyz"] == b["point_xyz"]).all()
        assert (a["edge_outlier"] == b["edge_outlier"]).all()


def _same(a, b):
    return (a["pose_Tcw"].tobytes() == b["pose_Tcw"].tobytes() and a["point_xyz"].tobytes() == b["point_xyz"].tobytes()
            and (a["edge_outlier"] == b["edge_outlier"]).all() and a["iters"] == b["iters"] and a["trials"] == b["trials"]
            and a["edge_chi2"].tobytes() == b["edge_chi2"].tobytes())


def test_lba_batch_equals_single_windows(pkg, oracle, gpu):
    """aos2_lba_solve_batch: windows of different sizes (reduced systems of 2 to 25 free keyframes, all in the register form
    k_ldlt_reg; a window without free keyframes' worth of points; different iteration needs) solved in one call give bit for bit what each gives
    alone, and match the oracle."""
    cfgs = [dict(seed=21, n_local=4, n_fixed=3, n_points=150), dict(seed=22, n_local=25, n_fixed=5, n_points=700),
            dict(seed=23, n_local=9, n_fixed=0, n_points=400, include_kf0=True, stereo_frac=0.3),
            dict(seed=24, n_local=2, n_fixed=9, n_points=300), dict(seed=0)]
    probs = [pkg.synth.synth_lba_problem(**c) for c in cfgs] + [_hard_problem(pkg, 42, 0.5, 3, 2)]
    batch = pkg.LocalBA().LocalBundleAdjustmentBatch(probs)
    for p, got in zip(probs, batch):
        alone = pkg.LocalBA().LocalBundleAdjustment(p)
        assert got["status"] == 0 and _same(got, alone)
        want = oracle.lba_solve(p)
        assert got["iters"] == want["iters"] and sum(got["trials"]) == want["trials"]
        assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
        assert (got["edge_outlier"] == want["edge_outlier"]).all()


def test_lba_batch_sizes_around_the_window_groups(pkg, gpu, monkeypatch):
    """The Schur kernel maps (window, block) to workgroups in groups of 8 / 16 windows (a window stays on one XCD); the
    linearisation's grid is (window, block).  Batches of 7, 8, 9, 16, 17 and 33 windows of mixed sizes -- partial groups,
    windows without off-diagonal blocks (one free keyframe), both landmark-kernel layouts -- give each window the bits it
    gets alone."""
    cfgs = [dict(seed=61, n_local=1, n_fixed=4, n_points=120), dict(seed=62, n_local=6, n_fixed=2, n_points=260),
            dict(seed=63, n_local=12, n_fixed=3, n_points=330, stereo_frac=0.4), dict(seed=64, n_local=3, n_fixed=0, n_points=90, include_kf0=True)]
    uniq = [pkg.synth.synth_lba_problem(**c) for c in cfgs]
    alone = [pkg.LocalBA().LocalBundleAdjustment(p) for p in uniq]
    for layout in ("slots", "walk"):
        monkeypatch.setenv("AOS2_LBA_LAYOUT", layout)
        ba = pkg.LocalBA()
        for n in (7, 8, 9, 16, 17, 33):
            idx = [(3 * i + n) % len(uniq) for i in range(n)]
            got = ba.LocalBundleAdjustmentBatch([uniq[j] for j in idx])
            assert all(g["status"] == 0 and _same(g, alone[j]) for g, j in zip(got, idx)), (layout, n)
    monkeypatch.delenv("AOS2_LBA_LAYOUT")
    # aos2_lba_set_window_groups: one program for the batch / two staggered groups (the default from 16 windows on) -- the same bits
    idx = [(3 * i + 5) % len(uniq) for i in range(33)]
    for groups in (1, 2, 0):
        ba = pkg.LocalBA()
        ba.set_window_groups(groups)
        for _ in range(2):
            got = ba.LocalBundleAdjustmentBatch([uniq[j] for j in idx])
            assert all(g["status"] == 0 and _same(g, alone[j]) for g, j in zip(got, idx)), groups
    with pytest.raises(Exception):
        ba.set_window_groups(3)


def test_lba_batch_is_deterministic_under_concurrency(pkg, gpu):
    """The LM decision is taken by the workgroup that finishes last from sums the other workgroups hand over (device-scope
    write-through stores, relaxed counter; no L2 write-back): repeated solves of one batch -- alone and while a second handle
    and the extractor keep the device busy -- give the same bits every time (tools/gpu_lba_determinism.py runs thousands)."""
    import threading
    u = [pkg.synth.synth_lba_problem(i, n_points=3000) for i in range(3)] + [pkg.synth.synth_lba_problem(seed=45, n_local=5, n_fixed=2, n_points=300)]
    probs = [u[i % len(u)] for i in range(16)]
    ba = pkg.LocalBA()
    ref = ba.LocalBundleAdjustmentBatch(probs)
    stop = []
    def other_lba():
        b2 = pkg.LocalBA()
        while not stop:
            b2.LocalBundleAdjustmentBatch(probs[:8])
    def extractor():
        ex = pkg.Extractor()
        imgs = pkg.synth.synth_batch(0, 16)
        while not stop:
            ex.extract_batch(imgs)
    th = [threading.Thread(target=other_lba), threading.Thread(target=extractor)]
    [t.start() for t in th]
    try:
        for _ in range(25):
            got = ba.LocalBundleAdjustmentBatch(probs)
            assert all(_same(a, b) for a, b in zip(got, ref))
    finally:
        stop.append(1)
        [t.join() for t in th]


def test_lba_handles_come_and_go(pkg, gpu):
    """A handle keeps worker threads and structure buffers between calls: creating, using (batches that start the pool,
    single windows that do not, a rejected input in between) and destroying many handles leaves nothing behind and
    changes no result."""
    def os_threads():
        return int(next(l for l in open("/proc/self/status") if l.startswith("Threads:")).split()[1])
    probs = [pkg.synth.synth_lba_problem(seed=71 + i, n_local=4 + i, n_fixed=2, n_points=100 + 40 * i) for i in range(3)]
    want = [pkg.LocalBA().LocalBundleAdjustment(p) for p in probs]
    warm = pkg.LocalBA()
    warm.LocalBundleAdjustmentBatch(probs)
    warm.close()
    before = os_threads()
    for rep in range(40):
        ba = pkg.LocalBA()
        if rep % 3 == 0:
            got = ba.LocalBundleAdjustmentBatch(probs * 3)
            assert all(_same(g, want[i % 3]) for i, g in enumerate(got))
        if rep % 5 == 0:
            bad = dict(probs[0])
            bad["edge_point"] = np.array(bad["edge_point"]).copy()
            bad["edge_point"][7] = bad["n_points"] + 5
            with pytest.raises(pkg.capi.AosError):
                ba.LocalBundleAdjustmentBatch([probs[1], bad])
        assert _same(ba.LocalBundleAdjustment(probs[rep % 3]), want[rep % 3])
        ba.close()
    assert os_threads() <= before   # (the pools' threads are joined when their handle goes)


def test_lba_landmark_kernel_layouts_agree(pkg, oracle, gpu, monkeypatch):
    """The landmark kernels have two layouts (8 threads per landmark for a few windows, one thread per landmark for many):
    both give the same bits, for landmarks with 2 .. 30 observations (several rounds of 8) and with rejected trials."""
    probs = [pkg.synth.synth_lba_problem(seed=51, n_local=30, n_fixed=4, n_points=120, obs_per_point=20),
             pkg.synth.synth_lba_problem(seed=0), _hard_problem(pkg, 42, 0.5, 3, 2)]
    assert np.bincount(probs[0]["edge_point"]).max() > 8
    res = {}
    for layout in ("slots", "walk"):
        monkeypatch.setenv("AOS2_LBA_LAYOUT", layout)
        res[layout] = [pkg.LocalBA().LocalBundleAdjustment(p) for p in probs] + pkg.LocalBA().LocalBundleAdjustmentBatch(probs)
    monkeypatch.delenv("AOS2_LBA_LAYOUT")
    for a, b in zip(res["slots"], res["walk"]):
        assert a["status"] == 0 and _same(a, b)
    for p, got in zip(probs, res["slots"]):
        want = oracle.lba_solve(p)
        assert got["iters"] == want["iters"]
        assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
        assert (got["edge_outlier"] == want["edge_outlier"]).all()


def test_lba_many_free_keyframes(pkg, oracle, gpu):
    """More than 42 free keyframes (reduced camera system > 256 rows): EuRoC / KITTI windows reach this size; the
    factorisation then runs in place in device memory (k_ldlt_dev) instead of in registers."""
    for cfg in (dict(seed=31, n_local=48, n_fixed=6, n_points=900), dict(seed=32, n_local=70, n_fixed=10, n_points=1200, stereo_frac=0.5)):
        prob = pkg.synth.synth_lba_problem(**cfg)
        assert int((prob["pose_fixed"] == 0).sum()) > 42
        want = oracle.lba_solve(prob)
        got = pkg.LocalBA().LocalBundleAdjustment(prob)
        assert got["status"] == 0 and got["iters"] == want["iters"]
        assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
        assert (got["edge_outlier"] == want["edge_outlier"]).all()


def test_lba_batch_with_both_reduced_system_forms(pkg, oracle, gpu):
    """A batch with windows on both sides of 40 free keyframes: k_ldlt_reg and k_ldlt_dev run side by side on two streams in every
    trial.  Every window equals the oracle and gives the bits it gives alone."""
    cfgs = [dict(seed=33, n_local=48, n_fixed=6, n_points=900), dict(seed=34, n_local=12, n_fixed=4, n_points=500),
            dict(seed=35, n_local=30, n_fixed=8, n_points=800, stereo_frac=0.5)]
    probs = [pkg.synth.synth_lba_problem(**c) for c in cfgs]
    nfree = [int((p["pose_fixed"] == 0).sum()) for p in probs]
    assert min(nfree) <= 40 < max(nfree)
    batch = pkg.LocalBA().LocalBundleAdjustmentBatch(probs)
    for p, got in zip(probs, batch):
        want = oracle.lba_solve(p)
        alone = pkg.LocalBA().LocalBundleAdjustment(p)
        assert got["status"] == 0 and got["iters"] == want["iters"]
        assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
        assert (got["edge_outlier"] == want["edge_outlier"]).all()
        assert _same(got, alone)


def _check_abort(got, want):
    assert got["stop_poll"] == want["stop_poll"] and got["polls"] == want["polls"]
    assert got["iters"] == want["iters"] and sum(got["trials"]) == want["trials"]
    assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
    assert (got["edge_outlier"] == want["edge_outlier"]).all()
    assert np.allclose(got["edge_chi2"], want["edge_chi2"], rtol=1e-5, atol=1e-6)


def test_lba_abort_at_every_poll(pkg, oracle, gpu):
    """pbStopFlag set while the optimisation runs (LocalMapping::InterruptBA, src/LocalMapping.cc:118-123): g2o reads it
    in the `for` condition of every iteration (sparse_optimizer.cpp:372), in the `while` condition of the trial loop
    after a rejected step (levenberg.cpp:149), and Optimizer.cc:663-666 once between the two optimisations.  The flag
    is made to appear at the k-th evaluation on both sides: same iterations, same trials, same results."""
    ba = pkg.LocalBA()
    for prob in (pkg.synth.synth_lba_problem(5, n_local=4, n_fixed=3, n_points=200), _hard_problem(pkg, 42, 0.5, 3, 2)):
        full = oracle.lba_solve(prob)
        assert full["stop_poll"] == 0
        for k in range(1, full["polls"] + 2):
            ba.debug_stop_at_poll(k)
            got = ba.LocalBundleAdjustment(prob)
            want = oracle.lba_solve(prob, stop_at_poll=k)
            if k == 1:
                assert got["status"] == pkg.capi.AOS2_ERR_STOPPED and want["status"] == 1
                assert (got["pose_Tcw"] == prob["pose_Tcw"]).all()
                continue
            assert got["status"] == 0
            _check_abort(got, want)
            if k <= full["polls"]:
                assert got["stop_poll"] == k
        ba.debug_stop_at_poll(0)
        assert ba.LocalBundleAdjustment(prob)["stop_poll"] == 0


def test_lba_abort_from_another_thread(pkg, oracle, gpu):
    """The real thing: a second host thread sets the flag while aos2_lba_solve waits for the device.  The call reports
    the evaluation that first saw the flag; the oracle replays an abort at that evaluation."""
    import threading
    import time
    prob = pkg.synth.synth_lba_problem(0)
    ba = pkg.LocalBA()
    ba.LocalBundleAdjustment(prob)   # warm-up (allocations)
    seen_mid = 0
    for delay in (0.0, 0.0002, 0.0004, 0.0007, 0.001, 0.0015, 0.002, 0.003):
        flag = np.zeros(1, np.uint8)

        def setter():
            time.sleep(delay)
            flag[0] = 1
        th = threading.Thread(target=setter)
        th.start()
        got = ba.LocalBundleAdjustment(prob, stop_flag=flag)
        th.join()
        if got["status"] == pkg.capi.AOS2_ERR_STOPPED:
            continue
        want = oracle.lba_solve(prob, stop_at_poll=got["stop_poll"]) if got["stop_poll"] else oracle.lba_solve(prob)
        _check_abort(got, want)
        seen_mid += 1 if got["stop_poll"] > 1 else 0
    assert seen_mid >= 1, "no run was interrupted in mid-solve: adjust the delays"


def _hard_problem(pkg, seed, rot_sigma, trans_sigma, point_sigma):
    """a small window whose free keyframes and points start far from the optimum, so that Levenberg-Marquardt rejects
    steps (lambda grows, estimates are restored) and, for some seeds, gives up after ten failed trials"""
    def rot(axis, a):
        axis = axis / np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        return np.eye(3) + np.sin(a) * K + (1 - np.cos(a)) * K @ K
    prob = pkg.synth.synth_lba_problem(seed, n_local=5, n_fixed=3, n_points=250, stereo_frac=0.3)
    rng = np.random.default_rng(seed)
    T = prob["pose_Tcw"].copy().reshape(-1, 4, 4)
    for i in range(len(T)):
        if not prob["pose_fixed"][i]:
            R = rot(rng.normal(size=3), rot_sigma * rng.normal())
            T[i, :3, :3] = (R @ T[i, :3, :3]).astype(np.float32)
            T[i, :3, 3] += rng.normal(size=3).astype(np.float32) * trans_sigma
    prob["pose_Tcw"] = T.reshape(prob["pose_Tcw"].shape).astype(np.float32)
    prob["point_xyz"] = (prob["point_xyz"] + rng.normal(size=prob["point_xyz"].shape) * point_sigma).astype(np.float32)
    return prob


@pytest.mark.parametrize("cfg", [(42, 0.5, 3, 2), (43, 0.5, 3, 2), (43, 1.0, 6, 4), (42, 0.3, 10, 8), (44, 0.5, 3, 2)])
def test_lba_rejected_trials_and_early_termination(pkg, oracle, gpu, cfg):
    """LM trials that fail (rho <= 0): estimates restored from the backup the Schur item kernel made (the system of
    the restored estimates is still in place, the residuals stay those of the rejected step like g2o's _error),
    lambda *= nu; ten failures end the optimisation (levenberg.cpp:118-150).  Same iteration and trial counts, lambda
    and outlier sets as the oracle."""
    prob = _hard_problem(pkg, *cfg)
    want = oracle.lba_solve(prob)
    lt, n1 = want["lambda_trace"], want["iters"][0]
    got = pkg.LocalBA().LocalBundleAdjustment(prob)
    assert got["status"] == 0 and got["iters"][0] == want["iters"][0]
    if want["chi2_trace"][-1] > 1e-18:   # (a pass that drives chi2 to 1e-26 accepts / rejects / stops on rounding noise)
        assert got["iters"] == want["iters"] and sum(got["trials"]) == want["trials"]
    assert (got["edge_outlier"] == want["edge_outlier"]).all()
    assert abs(got["final_chi2"] - want["chi2_trace"][-1]) <= 1e-6 * want["chi2_trace"][-1] + 1e-9   # (one case ends at chi2 ~ 1e-27)
    assert close(got["pose_Tcw"], want["pose_Tcw"]) and close(got["point_xyz"], want["point_xyz"])
    if cfg[0] != 44:   # these problems do contain rejected trials (lambda grows inside a pass)
        grow = [lt[i + 1] > lt[i] for i in range(len(lt) - 1) if i + 1 != n1]
        assert any(grow)


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_lba_bench_windows_vs_oracle(pkg, oracle, gpu, monkeypatch, layout):
    """Exactly what bench.py times: the SURVEY 8(d) windows (`synth_lba_problem(i, n_points=8000)`: 50 keyframes, ~4000
    points, ~24 k stereo edges), each solved alone and all together as bench.py's 32-window batch (4 distinct problems
    tiled), in both landmark-kernel layouts -- poses, points, outlier sets, iteration and trial counts against the oracle
    (1e-5), and the batch bit-identical to the single solves."""
    import sys
    sys.path.insert(0, os.path.dirname(oracle.__file__))
    import parity
    monkeypatch.setenv("AOS2_LBA_LAYOUT", layout)
    uniq = [pkg.synth.synth_lba_problem(i, n_points=8000) for i in range(4)]
    assert all(p["n_edges"] > 20000 and p["n_poses"] == 50 for p in uniq)
    want = [oracle.lba_solve(p) for p in uniq]
    ba = pkg.LocalBA()
    alone = [ba.LocalBundleAdjustment(p) for p in uniq]
    for i, (a, w) in enumerate(zip(alone, want)):
        assert parity.lba_mismatches(a, w, tag=f"window {i} alone ({layout})") == []
    batch = ba.LocalBundleAdjustmentBatch([uniq[i % 4] for i in range(32)])
    for i, got in enumerate(batch):
        assert parity.lba_mismatches(got, want[i % 4], tag=f"window {i} of the batch ({layout})") == []
        assert _same(got, alone[i % 4]), (layout, i)
    # the prepared form bench.py calls (same inputs every step, results in place)
    prep = ba.prepare_batch([uniq[i % 4] for i in range(32)])
    for _ in range(2):
        R = ba.solve_prepared(prep)
    for i in range(32):
        got = pkg.LocalBA._result(R[i], prep["arrs"][i])
        assert parity.lba_mismatches(got, want[i % 4], tag=f"prepared window {i} ({layout})") == []


def test_lba_mixed_window_batch_vs_oracle(pkg, oracle, gpu):
    """A batch of DIFFERENT windows (synth.lba_window_mix: reduced systems of 10 to 40 free keyframes, sparse and dense covisibility) and
    two hand-made extremes -- three keyframes sharing every point (off-diagonal blocks of > 256 items: k_schur's BIG units) and a
    window whose second keyframe pair shares nothing (an empty block still gets its zeros): every window equals the oracle, and
    the batch gives the bits of the windows solved alone (task lists, PACK units).  The two reduced-system kernels side by side:
    test_lba_batch_with_both_reduced_system_forms."""
    mix = pkg.synth.lba_window_mix(3, 6)
    for m in mix:
        m["n_points"] = 1500 + m["n_points"] // 6
    probs = [pkg.synth.synth_lba_problem(**m) for m in mix]
    probs.append(pkg.synth.synth_lba_problem(seed=61, n_local=3, n_fixed=1, n_points=1400, obs_per_point=4))
    nfree = [int((p["pose_fixed"] == 0).sum()) for p in probs]
    assert min(nfree) <= 21 < max(nfree)   # small and large reduced systems
    big = probs[-1]
    free = np.flatnonzero(big["pose_fixed"] == 0)
    both = np.intersect1d(big["edge_point"][big["edge_pose"] == free[0]], big["edge_point"][big["edge_pose"] == free[1]])
    assert len(both) > 256   # a BIG off-diagonal block
    ba = pkg.LocalBA()
    batch = ba.LocalBundleAdjustmentBatch(probs)
    assert ba.last_program()[0] >= 15
    for p, got in zip(probs, batch):
        want = oracle.lba_solve(p)
        alone = pkg.LocalBA().LocalBundleAdjustment(p)
        assert got["status"] == 0 and got["iters"] == want["iters"] and sum(got["trials"]) == want["trials"]
        assert close(got["pose_Tcw"], want["pose_Tcw"], key="mix_pose") and close(got["point_xyz"], want["point_xyz"], key="mix_point")
        assert (got["edge_outlier"] == want["edge_outlier"]).all()
        assert _same(got, alone)


def test_lba_unfinished_windows_continue_compacted(pkg, oracle, gpu):
    """The first round of the device program holds exactly the iterations' trials (5 + 10); windows whose steps get rejected are not
    finished then and continue in further rounds that cover THEM only (descriptors compacted, task lists rebuilt for the subset,
    sized for what they still need), while the others' results already stand.  A batch with such windows among ordinary ones of
    different sizes: every window equals the oracle (iterations, trials, lambda path through the outlier sets, poses), gives the bits
    it gives alone, and the program reports what it enqueued (aos2_lba_last_program / _window_slots)."""
    import sys
    sys.path.insert(0, os.path.dirname(oracle.__file__))
    import parity
    mix = pkg.synth.lba_window_mix(11, 12, hard_every=3)
    for m in mix:
        m["n_points"] = 900 + m["n_points"] // 8
    probs = [pkg.synth._lba_from_kwargs(m) for m in mix] + [_hard_problem(pkg, 42, 0.5, 3, 2), _hard_problem(pkg, 43, 1.0, 6, 4)]
    ba = pkg.LocalBA()
    batch = ba.LocalBundleAdjustmentBatch(probs)
    slots, rounds = ba.last_program()
    need = []
    for p, got, m_ in zip(probs, batch, mix + [dict(hard=1), dict(hard=1)]):
        want = oracle.lba_solve(p)
        assert got["status"] == 0 and got["iters"] == want["iters"] and sum(got["trials"]) == want["trials"], (got["iters"], got["trials"], want["iters"], want["trials"])
        if "hard" in m_:
            # 15 trials from a bad start do not converge; landmarks left with two inlier observations are held by lambda alone, and
            # rounding-level differences grow ~10 x per iteration.  The bar is the resolution the ORACLE has on this very window: its
            # spread against its own re-associated runs (parity.lba_resolution; profiles/r06_lba_sensitivity.txt), times
            # parity.LBA_RESOLUTION_FACTOR, never below 1e-5 -- and every decision has to be the oracle's
            res = parity.lba_resolution(p, want=want)
            assert res["decisions_equal"]
            assert parity.lba_mismatches(got, want, tag="window off the optimum", resolution=res) == []
        else:
            assert close(got["pose_Tcw"], want["pose_Tcw"], key="cont_pose") and close(got["point_xyz"], want["point_xyz"], key="cont_point")
        assert (got["edge_outlier"] == want["edge_outlier"]).all()
        assert _same(got, pkg.LocalBA().LocalBundleAdjustment(p))
        need.append(want["trials"])
    assert max(need) > 15 and rounds >= 2 and slots >= max(need)   # some window needed a continuation
    wslots = ba.last_window_slots()
    assert 15 * len(probs) < wslots < slots * len(probs)           # ... and the continuation rounds did not cover the finished ones
    # the form of rounds 2-4 (a spare trial per optimisation for every window) gives the same results
    os.environ["AOS2_LBA_SPARE_SLOTS"] = "1"
    try:
        ba2 = pkg.LocalBA()
        for got, old in zip(batch, ba2.LocalBundleAdjustmentBatch(probs)):
            assert _same(got, old)
        assert ba2.last_window_slots() >= 17 * len(probs)
    finally:
        del os.environ["AOS2_LBA_SPARE_SLOTS"]


@pytest.mark.parametrize("groups", [2, 1])
def test_lba_continuation_lists_larger_than_the_first_rounds(pkg, gpu, groups):
    """with two window groups and 8-15 windows a group has fewer than 8 windows, so the first round's Schur list is NOT
    padded to 8 queues -- the continuation round on >= 8 unfinished windows is (NX = 8, each queue as long as the longest: one
    40-keyframe window among 10-keyframe ones), i.e. LONGER than anything the first round built.  The continuation region is sized
    for any subset (lba_plan.h "Sized for ANY subset"): the batch solves, every window gives the bits it gives alone.  (Seeds whose
    oracle runs reject steps: more trials than iterations.)"""
    S = pkg.synth
    small = lambda seed, pert: S.perturb_lba_problem(S.synth_lba_problem(seed, n_local=10, n_fixed=4, n_points=260, obs_per_point=4, stereo_frac=0.3), seed, *pert)  # noqa: E731
    probs = [S.perturb_lba_problem(S.synth_lba_problem(880, n_local=40, n_fixed=4, n_points=700, obs_per_point=6, stereo_frac=0.3), 880, 2.0, 3.0, 2.0)]
    probs += [small(sd, (2.0, 3.0, 2.0)) for sd in (900, 906, 907, 913, 915, 919)] + [small(sd, (1.0, 6.0, 4.0)) for sd in (903, 910, 919, 926)]
    probs += [S.synth_lba_problem(950, n_local=8, n_fixed=3, n_points=200)]
    assert len(probs) == 12
    ba = pkg.LocalBA()
    ba.set_window_groups(groups)
    batch = ba.LocalBundleAdjustmentBatch(probs)
    slots, rounds = ba.last_program()
    rejected = [sum(r["trials"]) > sum(r["iters"]) for r in batch]
    assert rounds >= 2 and rejected[0] and sum(rejected) >= 9, (rounds, [(r["iters"], r["trials"]) for r in batch])
    for p, got in zip(probs, batch):
        assert got["status"] == 0 and _same(got, pkg.LocalBA().LocalBundleAdjustment(p))
    if groups == 2:
        # a continuation whose padded list would not fit falls back to ONE unpadded queue (AOS2_LBA_CONT_ONE_QUEUE forces that path: the
        # static is read at the first continuation of the process, so this runs in a child): the same bits
        import subprocess, sys, pickle, tempfile
        with tempfile.TemporaryDirectory() as d:
            pickle.dump(probs, open(os.path.join(d, "p.pkl"), "wb"))
            code = ("import sys, pickle; sys.path.insert(0, %r); import __graft_entry__ as g; pkg = g.load_package(); "
                    "probs = pickle.load(open(%r, 'rb')); ba = pkg.LocalBA(); ba.set_window_groups(2); r = ba.LocalBundleAdjustmentBatch(probs); "
                    "pickle.dump([(x['pose_Tcw'], x['point_xyz'], x['edge_outlier'], x['iters'], x['trials']) for x in r], open(%r, 'wb'))"
                    % (os.path.dirname(os.path.dirname(os.path.abspath(__file__))), os.path.join(d, "p.pkl"), os.path.join(d, "r.pkl")))
            subprocess.check_call([sys.executable, "-c", code], env=dict(os.environ, AOS2_LBA_CONT_ONE_QUEUE="1"))
            forced = pickle.load(open(os.path.join(d, "r.pkl"), "rb"))
        for got, f in zip(batch, forced):
            assert got["pose_Tcw"].tobytes() == f[0].tobytes() and got["point_xyz"].tobytes() == f[1].tobytes() and (got["edge_outlier"] == f[2]).all()
            assert tuple(got["iters"]) == tuple(f[3]) and tuple(got["trials"]) == tuple(f[4])


def test_lba_offopt_rule_over_a_spread_of_windows(pkg, oracle, gpu):
    """The comparison rule for windows that start off the optimum (parity.lba_resolution / lba_mismatches(resolution=)) on 18 more of them,
    three perturbation levels, one device batch: every decision the oracle's, poses / points within max(1e-5, 4 x the oracle's own spread
    on the window) -- the sample of tools/gpu_lba_offopt_sweep.py (profiles/r06_lba_offopt_sweep.txt: 192 windows, worst 1.79 x) that
    stays in the suite.  The oracle and its six re-associated runs per window are computed side by side in a thread pool (the variant
    switch is per thread)."""
    import sys
    from concurrent.futures import ThreadPoolExecutor
    sys.path.insert(0, os.path.dirname(oracle.__file__))
    import parity
    mix = pkg.synth.lba_window_mix(5, 18, hard_every=1)
    levels = [(0.5, 3.0, 2.0), (0.3, 1.0, 0.5), (0.2, 0.5, 0.2)]
    for i, m in enumerate(mix):
        m["hard"] = levels[i % 3]
        m["n_points"] = 800 + m["n_points"] // 6
    probs = [pkg.synth._lba_from_kwargs(m) for m in mix]
    got = pkg.LocalBA().LocalBundleAdjustmentBatch(probs)

    def ref(p):
        w = oracle.lba_solve(p)
        return w, parity.lba_resolution(p, want=w)
    with ThreadPoolExecutor(8) as pool:
        refs = list(pool.map(ref, probs))
    bad = []
    for i, (r, (w, res)) in enumerate(zip(got, refs)):
        assert res["decisions_equal"], i
        bad += parity.lba_mismatches(r, w, tag=f"window {i} {mix[i]['hard']}", resolution=res)
    assert bad == []
    assert any(res["point"] > 1e-5 for _, res in refs)   # (some of these windows do amplify: the rule is exercised, not vacuous)
