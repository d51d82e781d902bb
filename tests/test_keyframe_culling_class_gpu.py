"""host/KeyFrameCulling.h at the reference's call site, driven by tests/cpp/keyframe_culling_test.cpp on the GPU the way
LocalMapping::Run drives it: a snapshot with its culling view, one call, SetBadFlag on the pointer graph -- beside the stand-in's own
serial loop (tests/cpp/refstub/kf_culling_stub.h) on a second copy of the map.  Every keyframe's isBad() and mbToBeErased, every
point's isBad(), Observations() and observation set, and every keyframe's matches must be equal between the two copies."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import keyframe_culling_cases as cases  # noqa: E402
import keyframe_culling_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_keyframe_culling_class_follows_the_serial_loop(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "keyframe_culling_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", "-I" + os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "keyframe_culling_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    (g, v), cand, current = cases.class_map()
    w = ref.keyframe_culling(g, v, 1, cand)
    C, K, D, S = cases.CULLED, cases.KEPT, cases.DEFERRED, cases.SKIPPED
    assert list(w["status"]) == [D, S, C, C, C, C, K, K, K] and list(w["alone"][3:6]) == [K, K, K] and w["n_bad_points"] == 20   # the flips
    arrays = {k: np.ascontiguousarray(a, np.float32 if a.dtype == np.float32 else np.int32) for k, a in {**g, **v}.items()
              if isinstance(a, np.ndarray)}
    arrays.update(n_points=np.array([g["n_points"]], np.int32), n_keyframes=np.array([g["n_keyframes"]], np.int32),
                  cand=np.array(cand, np.int32), current=np.array([current], np.int32), monocular=np.array([1], np.int32))
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    for k in ("kf_bad", "kf_to_be_erased", "kf_mp", "point_bad", "point_nobs", "obs_off", "obs_kf"):
        assert np.array_equal(out["device_" + k], out["serial_" + k]), k
    # ... and both are what the restatement says (the keyframe added after the snapshot comes last and is KEPT)
    assert list(out["status"]) == list(w["status"]) + [K]
    nk = g["n_keyframes"]
    bad, tbe = np.zeros(nk, np.int32), np.zeros(nk, np.int32)
    bad[[c for c, s in zip(cand, w["status"]) if s == C]] = 1
    tbe[[c for c, s in zip(cand, w["status"]) if s == D]] = 1
    assert np.array_equal(out["device_kf_bad"], bad) and np.array_equal(out["device_kf_to_be_erased"], tbe)
    assert list(np.flatnonzero(out["device_point_bad"])) == list(w["bad_points"])
    assert (out["device_kf_mp"] != g["kf_mp"]).any()   # (the bad points left the matches of their observers)
