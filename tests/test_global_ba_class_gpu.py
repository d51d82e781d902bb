"""host/GlobalBundleAdjustment.h at the reference's signatures on the GPU: tests/cpp/global_ba_test.cpp builds a pointer graph of
stand-ins (tests/cpp/refstub/global_ba_stub.h) from a generator case -- keyframes with float32 poses and their undistorted keys,
map points with their observation maps -- and calls Optimizer::GlobalBundleAdjustemnt as LoopClosing.cc:652 (nLoopKF != 0, not robust)
and Tracking.cc:781 (nLoopKF == 0, robust) do.  What it writes is compared, bit for bit, with the C call on the arrays the gather of
:71-184 has to form from that map, and the order of the writes with :193-235.

What the map holds beyond the generator's problem, so that every gate of the gather is passed: mnId = 2 index (the vertex index is not
the mnId; keyframe 0 keeps mnId 0 and is the fixed one), keyframes and map points stored in an order that is not the order of their
mnId, a bad keyframe with the largest mnId that observes points, a point that only the bad keyframe observes (no edge: left
untouched), bad map points with observations, and the generator's point without any observation."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import global_ba_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def class_case(name, seed=5):
    """-> (bundle arrays without params, the problem as the class has to form it, per keyframe / map point of the map: the row of the
    problem it becomes or -1)"""
    P = R.problem(name)
    rng = np.random.default_rng([seed, 0xC1A55])
    n, M = P["n_poses"], P["n_points"]
    sf = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(7, np.float32(1.2), np.float32)])).astype(np.float32)
    table = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    octave = np.abs(P["edge_inv_sigma2"][:, None] - table[None]).argmin(1).astype(np.int32)
    assert (table[octave] == P["edge_inv_sigma2"]).all()
    # the map: keyframes in a shuffled storage order, then the bad one; map points shuffled, every seventh bad, then the orphan
    kf_order = rng.permutation(n)
    kf_id = np.concatenate([2 * np.asarray(P["pose_id"])[kf_order], [2 * n + 10]]).astype(np.int32)
    kf_bad = np.array([0] * n + [1], np.uint8)
    Tbad = np.eye(4, dtype=np.float32).reshape(16)
    kf_Tcw = np.concatenate([np.asarray(P["pose_Tcw"], np.float32)[kf_order], Tbad[None]])
    kf_slot = np.empty(n, np.int64)
    kf_slot[kf_order] = np.arange(n)
    mp_order = rng.permutation(M)
    mp_slot = np.empty(M, np.int64)
    mp_slot[mp_order] = np.arange(M)
    mp_id = np.concatenate([rng.permutation(M) * 2 + 1, [2 * M + 9]]).astype(np.int32)
    mp_bad = np.concatenate([(np.arange(M) % 7 == 3), [False]]).astype(np.uint8)
    mp_pos = np.concatenate([np.asarray(P["point_xyz"], np.float32)[mp_order], np.array([[0.5, 0.25, 9.0]], np.float32)])
    e_kf, e_mp = kf_slot[P["edge_pose"]], mp_slot[P["edge_point"]]
    shuffle = rng.permutation(P["n_edges"])   # (the observation maps are keyed by pointer: the order they are filled in must not matter)
    e_kf, e_mp, e_obs, e_oct = e_kf[shuffle], e_mp[shuffle], np.asarray(P["edge_obs"], np.float32)[shuffle], octave[shuffle]
    extra = [(n, int(j)) for j in range(0, M, 11)] + [(n, M)]   # the bad keyframe observes some points and, alone, the orphan
    e_kf = np.concatenate([e_kf, [k for k, _ in extra]]).astype(np.int32)
    e_mp = np.concatenate([e_mp, [j for _, j in extra]]).astype(np.int32)
    e_obs = np.concatenate([e_obs, np.tile(np.array([[100.0, 80.0, 90.0]], np.float32), (len(extra), 1))])
    e_oct = np.concatenate([e_oct, np.zeros(len(extra), np.int32)]).astype(np.int32)
    arrays = dict(cam=np.array([P[k] for k in ("fx", "fy", "cx", "cy", "bf")], np.float32), inv_sigma2=table, kf_id=kf_id, kf_bad=kf_bad, kf_Tcw=kf_Tcw,
                  mp_id=mp_id, mp_bad=mp_bad, mp_pos=mp_pos, e_kf=e_kf, e_mp=e_mp, e_obs=e_obs, e_octave=e_oct)
    # the problem of :71-184: the not-bad keyframes in storage order; the not-bad points with an observation by one of them, in
    # storage order; a point's observations by ascending mnId
    kf_row = np.where(kf_bad == 0, np.cumsum(kf_bad == 0) - 1, -1)
    mp_row = np.full(M + 1, -1, np.int64)
    ep, el, eo, es, ew = [], [], [], [], []
    rows = 0
    for j in range(M + 1):
        if mp_bad[j]:
            continue
        mine = [e for e in np.flatnonzero(e_mp == j) if kf_row[e_kf[e]] >= 0]
        if not mine:
            continue
        mp_row[j] = rows
        for e in sorted(mine, key=lambda e: kf_id[e_kf[e]]):
            ep.append(kf_row[e_kf[e]])
            el.append(rows)
            eo.append(e_obs[e])
            es.append(0 if e_obs[e][2] < 0 else 1)
            ew.append(table[e_oct[e]])
        rows += 1
    keep_k, keep_m = kf_row >= 0, mp_row >= 0
    Q = dict(P, n_poses=int(keep_k.sum()), n_points=rows, n_edges=len(ep), pose_Tcw=kf_Tcw[keep_k], pose_fixed=(kf_id[keep_k] == 0).astype(np.uint8),
             pose_id=kf_id[keep_k].astype(np.int64), point_xyz=mp_pos[keep_m], point_id=mp_id[keep_m].astype(np.int64), edge_pose=np.array(ep, np.int32),
             edge_point=np.array(el, np.int32), edge_obs=np.array(eo, np.float32).reshape(-1, 3), edge_stereo=np.array(es, np.uint8),
             edge_inv_sigma2=np.array(ew, np.float32))
    return arrays, Q, kf_row, mp_row


@pytest.fixture(scope="module")
def exe(pkg, gpu, tmp_path_factory):
    libdir = os.path.dirname(pkg.lib_path())
    out = str(tmp_path_factory.mktemp("gba_class") / "global_ba_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "global_ba_test.cpp"),
                           "-o", out, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("name,iterations,loop_kf,robust", [("mixed", 10, 7, False), ("mixed", 10, 0, False), ("init", 20, 0, True)])
def test_optimizer_class_gathers_calls_and_writes_back_like_the_reference(pkg, exe, tmp_path, name, iterations, loop_kf, robust):
    arrays, Q, kf_row, mp_row = class_case(name)
    want = pkg.capi.LocalBA(device=0).GlobalBundleAdjustment(Q, iterations, robust, R.HUBER_GBA)
    assert want["iterations"] >= 1 and want["point_included"].all() and np.abs(want["pose_Tcw"] - Q["pose_Tcw"]).max() > 1e-4
    bundle_io.save(tmp_path / "in.bundle", dict(arrays, params=np.array([iterations, loop_kf, int(robust)], np.int32)))
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    nk, nm = len(kf_row), len(mp_row)
    kin, min_ = kf_row >= 0, mp_row >= 0
    if loop_kf == 0:   # :200-203, :224-228
        new_T, new_X = out["kf_Tcw"].reshape(nk, 16), out["mp_pos"].reshape(nm, 3)
        assert (out["kf_gba"] == 0).all() and (out["mp_gba"] == 0).all() and not out["kf_TcwGBA"].any() and not out["mp_posGBA"].any()
        assert out["mp_updates"].tolist() == min_.astype(int).tolist()
        expect = [(ord("K"), int(i)) for i in arrays["kf_id"][kin]]
        for j in np.flatnonzero(min_):
            expect += [(ord("P"), int(arrays["mp_id"][j])), (ord("N"), int(arrays["mp_id"][j]))]
        assert [tuple(r) for r in out["log"].reshape(-1, 2).tolist()] == expect
    else:              # :204-209, :229-234: the map itself stays as it was
        new_T, new_X = out["kf_TcwGBA"].reshape(nk, 16), out["mp_posGBA"].reshape(nm, 3)
        assert out["kf_Tcw"].reshape(nk, 16).tobytes() == arrays["kf_Tcw"].tobytes() and out["mp_pos"].reshape(nm, 3).tobytes() == arrays["mp_pos"].tobytes()
        assert out["kf_gba"].tolist() == (kin * loop_kf).tolist() and out["mp_gba"].tolist() == (min_ * loop_kf).tolist()
        assert not out["mp_updates"].any() and out["log"].size == 0
    assert new_T[kin].tobytes() == want["pose_Tcw"][kf_row[kin]].tobytes()
    assert new_X[min_].tobytes() == want["point_xyz"][mp_row[min_]].tobytes()
    # the bad keyframe, the bad points, the orphan and the point without an observation: untouched
    if loop_kf == 0:
        assert new_T[~kin].tobytes() == arrays["kf_Tcw"][~kin].tobytes() and new_X[~min_].tobytes() == arrays["mp_pos"][~min_].tobytes()
    else:
        assert not new_T[~kin].any() and not new_X[~min_].any()
    assert mp_row[-1] == -1 and (mp_row[:-1][arrays["mp_bad"][:-1] == 0] == -1).any()
