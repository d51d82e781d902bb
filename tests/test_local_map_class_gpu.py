"""host/LocalMap.h, the snapshot of the map and UpdateLocalMap at the reference's call site, driven by tests/cpp/local_map_test.cpp on
the GPU the way Tracking drives it: one snapshot, then frame after frame with mvpLocalKeyFrames and mpReferenceKF carried over,
against the restatement (tests/local_map_ref.py).  The C++ side allocates its keyframes so that pointer order is not row order."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import local_map_cases as cases  # noqa: E402
import local_map_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_update_local_map_class_follows_the_restatement(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "local_map_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", "-I" + os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "local_map_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(91)
    g = cases.random_graph(rng, 16, 120)
    frames = cases.random_frames(rng, g, 12, (40, 0, 25, 64, 3))
    bad = [int(p) for p in np.flatnonzero(g["point_bad"])]
    frames[3], frames[6] = [-1] * 7, [bad[0], -1, bad[1 % len(bad)]]   # frames without votes keep the list of the frame before
    n, mp = cases.frames_arrays(frames, cap=64)
    nk, B = g["n_keyframes"], len(frames)
    arrays = {k: np.ascontiguousarray(v, np.int32) for k, v in g.items() if isinstance(v, np.ndarray)}
    arrays.update(n_points=np.array([g["n_points"]], np.int32), n_keyframes=np.array([nk], np.int32), n=n, mp=mp)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    lk, nlk, rk = np.full((1, nk), -1, np.int32), np.zeros(1, np.int32), np.full(1, -1, np.int32)
    kept = 0
    for b in range(B):
        w = ref.update_batch(g, n[b:b + 1], mp[b:b + 1], g["n_points"], nk, lk, nlk, rk)
        kept += (not w["voted"][0]) and w["n_local_kfs"][0] > 0
        assert list(out["mp"][b]) == list(w["mp"][0]), b
        assert list(out["kf_rows"][out["kf_off"][b]:out["kf_off"][b + 1]]) == list(w["local_kfs"][0, :w["n_local_kfs"][0]]), b
        assert list(out["pt_rows"][out["pt_off"][b]:out["pt_off"][b + 1]]) == list(w["local"][0, :w["n_local"][0]]), b
        assert out["ref"][b] == w["ref_kf"][0], b
        lk, nlk, rk = w["local_kfs"], w["n_local_kfs"], w["ref_kf"]
    assert kept >= 2 and (out["mp"] != mp).any() and len(set(out["ref"])) > 1
