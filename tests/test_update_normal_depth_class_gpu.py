"""host/UpdateNormalAndDepth.h at the reference's call sites, driven by tests/cpp/update_normal_depth_test.cpp on the GPU: a snapshot
with its culling view, the batch overload over every point of a map (with a NULL, a point outside the table, a bad point, one without
observations and one whose reference keyframe cannot be read at the observed feature), then moved points, an observation added and
applied as a delta, the one-point overload and the batch again -- beside a literal transcription of src/MapPoint.cc:363-413 written
in that program, on a second copy of the map.  mNormalVector, mfMinDistance, mfMaxDistance, theta_mean, theta_std, mNormalVectors and
theta_sVector of every point must be equal between the two copies BIT FOR BIT, the members of the points that are not updated must be
what they were, and everything must equal the restatement tests/normal_depth_ref.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import normal_depth_cases as cases  # noqa: E402
import normal_depth_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
PRESET = np.array([9, 9, 9, -1, -2, -3, -4], np.float32)   # what the program gives every point's members before the first update
BAD, EMPTY, OUTSIDE, UNREADABLE = 3, 4, 5, 6                # the points that are not to be updated


def class_map():
    """10 keyframes of 4 features (the last one spare) and 8 levels, 12 points seen from 2 .. 5 of them; point 6 is seen by its
    reference keyframe at a feature of octave 9.  -> the bundle's arrays, and graph / view of the points of the table before and
    after point 0 gains an observation"""
    rng = np.random.RandomState(5)
    nk, n_points = 10, 12
    octaves = [[(k + f) % 8 for f in range(4)] for k in range(nk)]
    octaves[2][1] = 9
    obs = [[(k, (p + k) % 3) for k in range(p % 3, nk, 2 + p % 3)] for p in range(n_points)]
    obs[EMPTY] = []
    obs[UNREADABLE] = [(2, 1), (7, 0)]
    refs = [o[len(o) // 2][0] if o else 0 for o in obs]
    refs[1] = next(k for k in range(nk) if k not in [x for x, _ in obs[1]])   # a reference keyframe that does not observe the point
    refs[UNREADABLE] = 2
    gain = (0, next(k for k in range(nk) if k not in [x for x, _ in obs[0]]), 3)
    in_table = np.ones(n_points, np.int32)
    in_table[OUTSIDE] = 0
    readable = np.ones(n_points, np.int32)
    readable[UNREADABLE] = 0
    bad = np.zeros(n_points, np.int32)
    bad[BAD] = 1
    kf_off, octave = cases.csr(octaves)
    obs_off, obs_kf = cases.csr([[k for k, _ in o] for o in obs])
    arrays = dict(n_keyframes=np.array([nk], np.int32), n_points=np.array([n_points], np.int32), kf_off=kf_off, octave=octave,
                  centre=rng.uniform(-5, 5, (nk, 3)).astype(np.float32), scale=cases.SCALE, xyz=rng.uniform(-3, 3, (n_points, 3)).astype(np.float32),
                  xyz2=rng.uniform(-3, 3, (n_points, 3)).astype(np.float32), ref=np.array(refs, np.int32), bad=bad, in_table=in_table,
                  readable=readable, obs_off=obs_off, obs_kf=obs_kf, obs_idx=np.array([f for o in obs for _, f in o], np.int32),
                  gain=np.array(gain, np.int32))
    rows = [p for p in range(n_points) if in_table[p]]   # the table's rows
    obs1 = [list(o) for o in obs]
    obs1[0] = sorted(obs1[0] + [(gain[1], gain[2])])
    graphs = [cases.build(octaves, [o[p] for p in rows], bad=[rows.index(BAD)]) for o in (obs, obs1)]
    return arrays, rows, graphs


def members_of(r, i):
    return np.concatenate([r["normal"][i], [r["min_dist"][i], r["max_dist"][i], r["theta_mean"][i], r["theta_std"][i]]]).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_update_normal_depth_class_follows_the_serial_function(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "update_normal_depth_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", "-DAOS2_HOST_EXCEPTIONS",
                           "-I" + os.path.join(ROOT, "tests", "cpp"), os.path.join(ROOT, "tests", "cpp", "update_normal_depth_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    arrays, rows, graphs = class_map()
    n_points = int(arrays["n_points"][0])
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    idle = (BAD, EMPTY, OUTSIDE, UNREADABLE)
    U, K = ref.UPDATED, ref.UNKNOWN
    want_status = [U, U, U, ref.BAD, ref.NO_OBS, K, ref.REF_UNUSABLE] + [U] * (n_points - 7)
    assert out["status_first"].tolist() == [K] + want_status            # (the NULL in front)
    assert out["status"].tolist() == want_status[1:]                     # (point 0 went through the one-point overload)
    for tag, xyz, (g, v) in (("first_", arrays["xyz"], graphs[0]), ("", arrays["xyz2"], graphs[1])):
        dm, sm = out["device_" + tag + "members"].reshape(n_points, 7), out["serial_" + tag + "members"].reshape(n_points, 7)
        doff, soff = out["device_" + tag + "off"], out["serial_" + tag + "off"]
        r = ref.update_normal_depth(g, v, np.arange(len(rows)), xyz[rows], arrays["ref"][rows], arrays["centre"], cases.SCALE,
                                    term_off=g["obs_off"])
        for p in range(n_points):
            du = out["device_" + tag + "units"][3 * doff[p]:3 * doff[p + 1]]
            dt = out["device_" + tag + "thetas"][doff[p]:doff[p + 1]]
            if p in idle:      # every member as the program preset it
                assert bits(dm[p]).tolist() == bits(PRESET).tolist() and du.tolist() == [8, 8, 8] and dt.tolist() == [-5], (tag, p)
                continue
            su = out["serial_" + tag + "units"][3 * soff[p]:3 * soff[p + 1]]
            st = out["serial_" + tag + "thetas"][soff[p]:soff[p + 1]]
            assert bits(dm[p]).tolist() == bits(sm[p]).tolist(), (tag, p, dm[p], sm[p])
            assert bits(du).tolist() == bits(su).tolist() and bits(dt).tolist() == bits(st).tolist(), (tag, p)
            i = rows.index(p)
            assert r["status"][i] == U and bits(dm[p]).tolist() == bits(members_of(r, i)).tolist(), (tag, p)
            a, b = g["obs_off"][i], g["obs_off"][i + 1]
            assert bits(dt).tolist() == bits(r["term_theta"][a:b]).tolist() and bits(du).tolist() == bits(r["term_unit"][a:b]).reshape(-1).tolist()
        # the serial copy leaves the bad point and the one without observations alone too
        assert bits(sm[BAD]).tolist() == bits(PRESET).tolist() and bits(sm[EMPTY]).tolist() == bits(PRESET).tolist()
    # the second round differs from the first, and point 0 has one observer more
    assert not np.array_equal(out["device_members"], out["device_first_members"])
    assert out["device_off"][1] == out["device_first_off"][1] + 1
