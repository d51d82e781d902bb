"""host/StateValidChecker.h, the class at the reference's signatures, driven by tests/cpp/state_valid_checker_test.cpp on the GPU
over the reference's own planner map and obstacles: checkMotionTW, MotionCost, GetShortestPath, myprop, reconstructMotionTW,
MotionCostLength / MotionCostCamera, isValid and check_collisions one at a time (Vector and ob::State* forms) against the
restatement (tests/motion_tw_ref.py), and the batch members checkMotionsTW, MotionCosts, reconstructMotionsTW and isValidBatch equal
to the one-at-a-time members."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import motion_tw_ref as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
NM = 40


def test_state_valid_checker_class_returns_what_the_restatement_returns(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "state_valid_checker_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS",
                           os.path.join(ROOT, "tests", "cpp", "state_valid_checker_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    D = M.golden_draw()
    S, w = D.scene, D.want
    none = M.PLANTED_MOTIONS["none"]                       # a pair without a path among them
    q1, q2 = np.vstack([D.q1[:NM - 1], [none[0]]]), np.vstack([D.q2[:NM - 1], [none[1]]])
    want = S.motions(q1, q2)
    states = w["states"][:60]
    m = S.map
    arrays = dict(xyz=m.xyz.astype(np.float64), ub=m.upper.astype(np.float64), lb=m.lower.astype(np.float64),
                  max_dist=m.max_range.astype(np.float64), min_dist=m.min_range.astype(np.float64), ratio=m.ratio.astype(np.float64),
                  thres=np.array([S.thr], np.int32), obs=S.obs, q1=q1, q2=q2, states=states)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    # one at a time against the restatement
    assert list(out["check"]) == list(want["valid"]) and list(out["check_state"]) == list(want["valid"])
    assert out["len"].tobytes() == want["cost_length"].tobytes() and out["len_state"].tobytes() == want["cost_length"].tobytes()
    assert out["cam"].tobytes() == want["cost_camera"].tobytes()
    assert list(out["path_valid"]) == list(want["path_valid"]) and out["path_t"].tobytes() == want["t"].tobytes()
    dirs = np.array([[M.CANDIDATES[t][2]] * 3 if t >= 0 else [0, 0, 0] for t in want["type"]], np.int32)
    assert (out["path_v"].reshape(-1, 3) == dirs).all()
    ws = np.array([[M.CANDIDATES[t][0] * M.CANDIDATES[t][2] / 0.25, 0, M.CANDIDATES[t][1] * M.CANDIDATES[t][2] / 0.25] if t >= 0 else [0, 0, 0]
                   for t in want["type"]], np.float64)
    assert out["path_w"].tobytes() == ws.tobytes()
    prop = np.array([M.myprop(list(a), float(d[0]), x[0], t[0]) if t0 >= 0 else list(a)
                     for a, d, x, t, t0 in zip(q1, dirs, ws, want["t"], want["type"])], np.float64)
    assert out["prop"].tobytes() == prop.tobytes()
    assert list(out["rec_ok"]) == list(want["path_valid"])
    keep = np.concatenate([np.arange(want["offsets"][k], want["offsets"][k + 1]) for k in range(NM) if want["path_valid"][k]])
    assert out["rec"].tobytes() == want["states"][keep].tobytes()
    assert list(np.diff(out["rec_off"])) == [int(n) if ok else 0 for n, ok in zip(want["n_states"], want["path_valid"])]
    assert out["len_q"].tobytes() == want["cost_length"].tobytes() and out["cam_q"].tobytes() == want["cost_camera"].tobytes()
    v = S.valid(states)
    assert list(out["valid"]) == list(v["valid"]) and list(out["free"]) == list(v["collision_free"])
    assert not out["plain"].any()                          # a checker without a map sees nothing: no state is valid
    # the batch members against the one-at-a-time members
    assert list(out["b_check"]) == list(out["check"]) and list(out["b_valid"]) == list(out["valid"])
    assert out["b_len"].tobytes() == out["len"].tobytes() and out["b_cam"].tobytes() == out["cam"].tobytes()
    assert list(out["b_rec_ok"]) == list(out["rec_ok"]) and list(out["b_rec_off"]) == list(out["rec_off"])
    assert out["b_rec"].tobytes() == out["rec"].tobytes()
    assert 0 < out["check"].sum() < NM and 0 < out["valid"].sum() < len(states) and 0 < out["free"].sum() < len(states)
