"""host/camera.h, the class at the reference's signatures, driven by tests/cpp/camera_test.cpp on the GPU over the reference's own
planner map: countVisible in both overloads, IsStateVisiblilty, and the batch members countVisibleBatch, MotionCostCameraBatch and
AdvanceStepCamera against the restatement (tests/visibility_ref.py), with a second camera object taking the thread's handle in
between."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import visibility_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
THRES = 20


def test_camera_class_returns_what_the_restatement_returns(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "camera_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS",
                           os.path.join(ROOT, "tests", "cpp", "camera_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    case = R.golden_case()
    m = case.map
    single = np.concatenate([np.nonzero(case.count > 40)[0][:4], np.nonzero(case.count == 0)[0][:2],
                             np.nonzero((case.count > 0) & (case.count <= 40))[0][:2]]).astype(np.int32)
    sizes = (1, 2, 3, 40, 100)
    motions, counts = R.motions_of(case, sizes)
    traj = R.trajectories_of(case, THRES)
    traj40 = {k: R.advance_step(case.count[idx], 40) for k, (idx, _) in traj.items()}
    arrays = dict(xyz=m.xyz.astype(np.float64), ub=m.upper.astype(np.float64), lb=m.lower.astype(np.float64),
                  max_dist=m.max_range.astype(np.float64), min_dist=m.min_range.astype(np.float64), ratio=m.ratio.astype(np.float64),
                  thres=np.array([THRES], np.int32), states=case.states.astype(np.float64), single=single,
                  poses=case.poses()[single], mo_off=np.cumsum((0,) + sizes).astype(np.int32),
                  tr_off=np.cumsum([0] + [len(idx) for idx, _ in traj.values()]).astype(np.int32),
                  tr_idx=np.concatenate([idx for idx, _ in traj.values()]).astype(np.int32))
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    assert list(out["one"]) == list(case.count[single]) and list(out["one_pose"]) == list(case.count[single])
    assert list(out["visible"]) == [int(c > THRES) for c in case.count[single]]
    assert list(out["visible_40"]) == [int(c > 40) for c in case.count[single]]
    assert (out["empty"] == 0).all() and len(out["empty"]) == len(single)
    assert (out["batch"] == case.count).all()
    want = np.array([R.motion_cost(c, THRES) for c in counts], np.float64)
    assert out["cost"].tobytes() == want.tobytes() and want[4] > 0
    assert list(out["advance"]) == [w for _, w in traj.values()]
    assert list(out["advance_40"]) == [traj40[k] for k in traj]
    assert len(set(out["visible"])) == 2 and max(out["advance"]) >= 65 and min(out["advance"]) == -1
