"""host/LocalMap.h LocalMapSnapshot::Apply at the reference's call site, driven by tests/cpp/local_map_apply_test.cpp on the GPU the
way one pass of LocalMapping::Run drives it: a snapshot with its culling view, the stub objects changed (a keyframe inserted, points
created, replaced and culled, a keyframe culled, covisibles re-linked), ONE Apply that names what changed.  The program requires the
applied handle and a FRESH snapshot of the changed map to agree array by array; here the lists of Tracking::UpdateLocalMap and the
verdicts of KeyFrameCulling that it got through the applied snapshot are compared with tests/local_map_ref.py and
tests/keyframe_culling_ref.py on the final graph."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import keyframe_culling_cases as kcases  # noqa: E402
import keyframe_culling_ref as kref  # noqa: E402
import local_map_apply_cases as cases  # noqa: E402
import local_map_ref as lref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_snapshot_apply_follows_one_local_mapping_pass(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "local_map_apply_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", "-I" + os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "local_map_apply_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(7)
    m = cases.random_map(rng)
    nk = len(m["kfs"])
    m["kfs"][nk // 2]["flags"] = 0   # (the keyframe the program culls is neither held nor the first one)
    g, v = cases.to_arrays(m)
    assert v["kf_flags"][0] & kcases.FIRST and not (v["kf_flags"][1:] & kcases.FIRST).any() and nk // 2 > 0
    arrays = {k: np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.int32) for k, a in {**g, **v}.items()
              if isinstance(a, np.ndarray)}
    arrays.update(n_points=np.array([g["n_points"]], np.int32), n_keyframes=np.array([nk], np.int32), monocular=np.array([0], np.int32))
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    assert out["agree"][0] == 1, ("the applied and the fresh snapshot differ in arrays", list(out["differ"]))
    assert out["path"][0] == 1                      # the rebuild ran on the device
    touched, relinked, points = (int(x) for x in out["named"])
    assert 1 < touched <= nk and 3 <= relinked <= nk and 10 < points < g["n_points"]   # a delta, not the whole map
    # the final graph as the snapshot holds it
    g1 = dict(n_points=len(out["point_bad"]), n_keyframes=len(out["kf_bad"]))
    for k in ("point_bad", "kf_bad"):
        g1[k] = out[k].astype(np.uint8)
    for k in ("point_nobs", "obs_off", "obs_kf", "kf_mp_off", "kf_mp", "kf_best", "kf_child_off", "kf_child", "kf_parent"):
        g1[k] = out[k].astype(np.int32)
    v1 = dict(obs_idx=out["obs_idx"].astype(np.int32), kf_octave=out["kf_octave"].astype(np.int8), kf_depth=out["kf_depth"].astype(np.float32),
              kf_stereo=out["kf_stereo"].astype(np.uint8), kf_th_depth=out["kf_th_depth"].astype(np.float32), kf_flags=out["kf_flags"].astype(np.uint8))
    assert g1["n_keyframes"] == nk + 1 and g1["n_points"] == g["n_points"] + 4 and g1["kf_bad"][nk // 2] == 1
    assert g1["point_bad"][g["n_points"] + 1] == 1 and np.diff(g1["obs_off"])[g["n_points"] + 1] == 0   # the NULL slot of the table
    assert (np.diff(g1["obs_off"])[[g["n_points"], g["n_points"] + 2, g["n_points"] + 3]] >= 1).all() and g1["kf_parent"][nk] == nk - 1
    # Tracking::UpdateLocalMap of the program's frames
    B = len(out["f_off"]) - 1
    assert B == 4
    voted = 0
    for b in range(B):
        mp = out["f_mp"][out["f_off"][b]:out["f_off"][b + 1]].astype(np.int32)
        w = lref.update_batch(g1, np.array([len(mp)], np.int32), mp.reshape(1, -1), g1["n_points"], g1["n_keyframes"])
        assert list(out["f_mp_out"][out["f_off"][b]:out["f_off"][b + 1]]) == list(w["mp"][0]), b
        assert list(out["kf_rows"][out["kf_off"][b]:out["kf_off"][b + 1]]) == list(w["local_kfs"][0, :w["n_local_kfs"][0]]), b
        assert list(out["pt_rows"][out["pt_off"][b]:out["pt_off"][b + 1]]) == list(w["local"][0, :w["n_local"][0]]), b
        assert out["ref"][b] == w["ref_kf"][0], b
        voted += int(w["voted"][0])
    assert voted >= 3 and nk in out["kf_rows"]      # the new keyframe is a local keyframe of some frame
    # LocalMapping::KeyFrameCulling through the applied snapshot
    w = kref.keyframe_culling(g1, v1, 0, out["cand"])
    assert list(out["status"]) == list(w["status"])
    assert (w["status"] == kcases.CULLED).any() and (w["status"] == kcases.KEPT).any()
    culled = [int(c) for c, s in zip(out["cand"], w["status"]) if s == kcases.CULLED]
    assert all(out["kf_bad_after"][c] == 1 for c in culled)
