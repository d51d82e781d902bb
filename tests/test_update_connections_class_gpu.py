"""host/UpdateConnections.h at the reference's call sites, driven by tests/cpp/update_connections_test.cpp on the GPU: a snapshot, a
fusion applied as a delta, the sequence of LoopClosing::CorrectLoop (the current keyframe, then a loop over its connected keyframes)
and a new keyframe that the snapshot does not know -- beside the stand-in's own serial KeyFrame::UpdateConnections
(tests/cpp/refstub/connections_stub.h, the connection members protected) on a second copy of the map.  Every keyframe's weight map,
ordered list, ordered weights, parent, children and mbFirstConnection must be equal between the two copies, and equal to the
restatement tests/update_connections_ref.py where it speaks."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import local_map_cases as lm_cases  # noqa: E402
import update_connections_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
REPORT = ("weight_off", "weight_kf", "weight_w", "ordered_off", "ordered_kf", "ordered_w", "parent", "child_off", "child", "first")


def class_map():
    """8 keyframes of 56 features over 112 points: keyframe k holds the points [12 k, 12 k + 40), so neighbours share 28, 16 and 4
    points (15 lies between); keyframe 7 holds only [84, 94) and ties at 10 with 5 and 6; two bad points.  The fusion gives keyframe
    2 the points [64, 76): its weight with keyframe 5 goes from 3 to exactly 15.  The late keyframe sees [48, 52): 4 each with 1, 2, 3, 4."""
    nk, N = 8, 56
    kf_mp = [list(range(12 * k, 12 * k + 40)) + [-1] * (N - 40) for k in range(7)] + [list(range(84, 94)) + [-1] * (N - 10)]
    bad = [30, 61]
    fuse = [(2, 40 + j, 64 + j) for j in range(12)]
    kf_mp1 = [list(r) for r in kf_mp]
    for k, f, p in fuse:
        kf_mp1[k][f] = p
    late = [48, -1, 49, 50, 51, -1]
    return lm_cases.make_graph(112, kf_mp, point_bad=bad), lm_cases.make_graph(112, kf_mp1, point_bad=bad), fuse, late, 2


def rows_of(out, tag, k):
    """keyframe k of a report -> (weight map, ordered list, parent, children, first)"""
    a, b = out[tag + "weight_off"][k:k + 2]
    c, d = out[tag + "ordered_off"][k:k + 2]
    e, f = out[tag + "child_off"][k:k + 2]
    return (dict(zip(out[tag + "weight_kf"][a:b].tolist(), out[tag + "weight_w"][a:b].tolist())),
            list(zip(out[tag + "ordered_kf"][c:d].tolist(), out[tag + "ordered_w"][c:d].tolist())),
            int(out[tag + "parent"][k]), out[tag + "child"][e:f].tolist(), int(out[tag + "first"][k]))


def test_update_connections_class_follows_the_serial_function(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "update_connections_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", "-I" + os.path.join(ROOT, "tests", "cpp"),
                           os.path.join(ROOT, "tests", "cpp", "update_connections_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    g0, g1, fuse, late, current = class_map()
    nk = g0["n_keyframes"]
    # what the sequence is to show, from the restatement alone
    c0, o0 = ref.update_connections_one(g0, current, ref.resident_matches(g0, current))
    c1, o1 = ref.update_connections_one(g1, current, ref.resident_matches(g1, current))
    assert c0[5] == 3 and c1[5] == 15 and (5, 15) in o1 and len(o1) > len(o0) > 1          # the fusion lifts 5 over the threshold
    _, o7 = ref.update_connections_one(g1, 7, ref.resident_matches(g1, 7))
    assert o7 == [(5, 10)]                                                                 # nothing over 15, a tie: the lowest row
    cl, ol = ref.update_connections_one(g1, -1, late)
    assert cl == {1: 4, 2: 4, 3: 4, 4: 4} and ol == [(1, 4)]
    arrays = dict(n_points=np.array([g0["n_points"]], np.int32), n_keyframes=np.array([nk], np.int32), kf_mp_off=g0["kf_mp_off"],
                  kf_mp=g0["kf_mp"], point_bad=g0["point_bad"].astype(np.int32), current=np.array([current], np.int32),
                  fuse_kf=np.array([f[0] for f in fuse], np.int32), fuse_feature=np.array([f[1] for f in fuse], np.int32),
                  fuse_point=np.array([f[2] for f in fuse], np.int32), late_mp=np.array(late, np.int32))
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    for tag in ("", "at434_"):
        for k in REPORT:
            assert np.array_equal(out["device_" + tag + k], out["serial_" + tag + k]), (tag, k)
    assert np.array_equal(out["device_seen"], out["serial_seen"]) and len(out["device_seen"]) > 40   # the hooks around each keyframe of the loop
    # the sequence changed the graph, and the loop ran over more than the current keyframe
    assert any(not np.array_equal(out["device_" + k], out["before_" + k]) for k in ("weight_w", "ordered_kf"))
    assert len(out["connected"]) == len(o1) + 1 and 5 in out["connected"].tolist()
    # ... and where the restatement speaks: the current keyframe right after :434, the late keyframe at the end, keyframe 7's first link
    weights, ordered, parent, children, first = rows_of(out, "device_at434_", 0)
    assert weights == c1 and ordered == o1 and first == 0
    weights, ordered, parent, children, first = rows_of(out, "device_", nk)
    assert weights == cl and ordered == ol and parent == 1 and first == 0 and children == []
    assert nk in rows_of(out, "device_", 1)[3] and rows_of(out, "device_", 1)[0][nk] == 4      # AddChild and AddConnection on keyframe 1
    assert rows_of(out, "before_", 7)[1][0] == (5, 10) and rows_of(out, "before_", 7)[2] == 5
    assert rows_of(out, "device_", 0)[2] == -1 and rows_of(out, "device_", 0)[4] == 1          # mnId 0: no parent, the flag stays
