"""host/OptimizeEssentialGraph.h at the reference's signature on the GPU: tests/cpp/essential_graph_test.cpp builds a pointer graph of
stand-ins (tests/cpp/refstub/essential_graph_stub.h) from the generator's map -- keyframes with float32 poses, parents and children,
loop edges, ordered covisibility lists with weights, CorrectedSim3 / NonCorrectedSim3, LoopConnections, map points with their reference
keyframes -- and calls Optimizer::OptimizeEssentialGraph as LoopClosing.cc:569 does.  The values written by SetPose / SetWorldPos, the
number of UpdateNormalAndDepth calls and the order of the writes are compared with tests/essential_graph_ref.py run on the problem the
gather of :798-984 has to form from that map (the comparison rule of DESIGN.md section 2 item 14).

What the map holds beyond the generator's edges, so that every gate of the gather is passed at least once: mnId = 2 index + 3 (the
vertex index is not the mnId), a bad keyframe with an mnId in the middle, a LoopConnections pair below minFeat (:864) and the
(pCurKF, pLoopKF) pair below it (kept), covisibility lists that also name the parent, a child, the loop-edge partner, pairs of
sInsertedEdges, later keyframes and a neighbour below weight 100, bad map points, and points corrected by pCurKF (:1022-1025)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import essential_graph_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def class_case(seed, n, fix_scale):
    """-> (bundle arrays, the problem as the class has to form it, per map point: bad)"""
    P = R.problem(seed, n, fix_scale)
    rng = np.random.default_rng([seed, n, 77])
    U, cur_side, loop, cur = P["uncorrected"], P["cur_side"], int(P["fixed"]), n - 1
    Tcw = np.zeros((n + 1, 4, 4), np.float32)
    Tcw[:n, :3, :3] = R.rot_of(U[:, :4] / np.linalg.norm(U[:, :4], axis=1, keepdims=True)).astype(np.float32)
    Tcw[:n, :3, 3] = U[:, 4:7].astype(np.float32)
    Tcw[:, 3, 3] = 1
    Tcw[n, :3, :3] = np.eye(3)   # the bad keyframe, last in storage
    # Sim3(Rcw, tcw, 1.0) of the float32 pose: Quaterniond(R) is not normalised
    Uq = np.stack([np.concatenate([R.S3.quat_from_rot(Tcw[k, :3, :3].astype(np.float64)), Tcw[k, :3, 3].astype(np.float64), [1.0]]) for k in range(n)])
    vScw = Uq.copy()
    vScw[cur_side] = P["Scw"][cur_side]
    v0, v1, kind = P["v0"], P["v1"], P["kind"]
    Sji = np.where((kind == 0)[:, None], R.mul(vScw[v1], R.inverse(vScw)[v0]), R.mul(Uq[v1], R.inverse(Uq)[v0]))
    # map points: every fifth one bad, every third of the rest corrected by pCurKF with another reference
    M = 6 * n
    bad = (np.arange(M) % 5 == 2)
    by_cur = (np.arange(M) % 3 == 1)
    mp_ref, corr_ref = rng.integers(0, n, M).astype(np.int32), rng.integers(0, n, M).astype(np.int32)
    pos = rng.uniform(-5, 5, (M, 3)).astype(np.float32)
    good = ~bad
    Q = dict(P, Scw=vScw, Sji=Sji, Xw=pos[good], ref=np.where(by_cur, corr_ref, mp_ref)[good].astype(np.int32))
    # the pointer graph
    lc = [(int(a), int(b)) for a, b, k in zip(v0, v1, kind) if k == 0]
    weights = [(a, b, 10 if (a, b) == (cur, loop) else 150) for a, b in lc]
    if n >= 9:
        lc.append((cur, 4))          # below minFeat: no edge
        weights.append((cur, 4, 50))
    loop_edges = [(int(a), int(b)) for a, b, k in zip(v0, v1, kind) if k == 2]
    covis_ptr, covis_idx, covis_w = [0], [], []
    for i in range(n):
        row = ([(i + 1, 200)] if i + 1 < n else []) + ([(i - 1, 190)] if i > 0 else [])
        row += [(j, 150) for j in range(i - 2, max(0, i - 2 - (2 + i % 5)), -1) if j >= 1]
        row += [(i + 2, 120)] if i + 2 < n else []            # a later keyframe: the edge belongs to its turn
        row += [(i - 9, 60)] if i - 9 >= 1 else []            # below weight 100
        covis_idx += [j for j, w in row]
        covis_w += [w for j, w in row]
        covis_ptr.append(len(covis_idx))
    covis_ptr.append(len(covis_idx))                          # the bad keyframe: no neighbours
    ids = np.concatenate([2 * np.arange(n) + 3, [2 * (n // 2) + 4]]).astype(np.int32)
    arrays = dict(params=np.array([loop, cur, int(fix_scale)], np.int32), kf_id=ids, kf_bad=np.array([0] * n + [1], np.uint8), kf_Tcw=Tcw.reshape(n + 1, 16),
                  kf_parent=np.concatenate([[-1], np.arange(n - 1), [0]]).astype(np.int32), loop_edges=np.array(loop_edges, np.int32).reshape(-1, 2),
                  covis_ptr=np.array(covis_ptr, np.int32), covis_idx=np.array(covis_idx, np.int32), covis_w=np.array(covis_w, np.int32),
                  weights=np.array(weights, np.int32).reshape(-1, 3), sim3_idx=np.array(cur_side, np.int32), corrected=P["Scw"][cur_side],
                  noncorrected=Uq[cur_side], lc_pairs=np.array(lc, np.int32).reshape(-1, 2), mp_pos=pos, mp_bad=bad.astype(np.uint8), mp_ref=mp_ref,
                  mp_by_cur=by_cur.astype(np.uint8), mp_corr_ref=corr_ref)
    return arrays, Q, bad


@pytest.fixture(scope="module")
def exe(pkg, gpu, tmp_path_factory):
    libdir = os.path.dirname(pkg.lib_path())
    out = str(tmp_path_factory.mktemp("eg_class") / "essential_graph_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "essential_graph_test.cpp"),
                           "-o", out, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    return out


@pytest.mark.parametrize("n,fix_scale", [(17, False), (33, True)])
def test_optimizer_class_gathers_calls_and_writes_back_like_the_reference(exe, tmp_path, n, fix_scale):
    arrays, Q, bad = class_case(4, n, fix_scale)
    want = R.optimize(Q)
    res, same_status = R.resolution(Q, want)
    assert same_status and want["status"] == R.EG_OK and want["chi2_final"] < want["chi2_initial"]
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    tol = R.tolerance(res)
    Tcw = out["kf_Tcw"].reshape(n + 1, 4, 4)
    dT = float(np.abs(Tcw[:n].astype(np.float64) - want["Tiw"]).max())
    dX = float(np.abs(out["mp_pos"].reshape(-1, 3)[~bad].astype(np.float64) - want["Xw"]).max())
    moved = float(np.abs(Tcw[:n] - arrays["kf_Tcw"].reshape(n + 1, 4, 4)[:n]).max())
    print("n", n, "SetPose differs by %.3g, SetWorldPos by %.3g, tolerance %.3g; the poses moved by up to %.3g" % (dT, dX, tol, moved))
    assert dT <= tol and dX <= tol and moved > 1e-3
    # the fixed keyframe: R(q) of its own pose, t / 1; the bad keyframe and the bad points: untouched
    assert np.abs(Tcw[Q["fixed"]] - arrays["kf_Tcw"].reshape(n + 1, 4, 4)[Q["fixed"]]).max() <= 1e-6
    assert Tcw[n].tobytes() == arrays["kf_Tcw"].reshape(n + 1, 4, 4)[n].tobytes()
    assert out["mp_pos"].reshape(-1, 3)[bad].tobytes() == arrays["mp_pos"][bad].tobytes()
    assert out["mp_updates"].tolist() == (~bad).astype(int).tolist()
    # the order of the writes (:993-1044): every keyframe in the order of GetAllKeyFrames, then per point SetWorldPos, UpdateNormalAndDepth
    log = out["log"].reshape(-1, 2)
    ids = arrays["kf_id"][:n]
    expect = [(ord("K"), int(i)) for i in ids]
    for j in np.flatnonzero(~bad):
        expect += [(ord("P"), 100 + int(j)), (ord("N"), 100 + int(j))]
    assert [tuple(r) for r in log.tolist()] == expect
