"""Whole LocalBundleAdjustment solves of small windows built to reach what the landmark kernels' data paths depend on: an edge order
that is a real permutation, landmark degrees around the chunk sizes of the walks' loops, flags the outlier pass rewrites, trials
that are rejected, a window with hundreds of keyframes beside a small one.  Every window is solved in both landmark-kernel layouts,
alone and in one batch: the same bits everywhere, the oracle's result, and the bits recorded in tests/golden/lba_walk_bits.json
(tests/golden/make_lba_walk_bits.py) with the build before the walks read edge records and staged the keyframe state in LDS."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_lba_walk_bits as WB  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "lba_walk_bits.json")) as f:
    GOLDEN = json.load(f)
NAMES = ("permuted", "degrees", "flags", "rejected", "rejected_repeated", "big")


def _same(a, b):
    return (a["pose_Tcw"].tobytes() == b["pose_Tcw"].tobytes() and a["point_xyz"].tobytes() == b["point_xyz"].tobytes()
            and (a["edge_outlier"] == b["edge_outlier"]).all() and a["iters"] == b["iters"] and a["trials"] == b["trials"]
            and a["edge_chi2"].tobytes() == b["edge_chi2"].tobytes())


@pytest.fixture(scope="module")
def wins(pkg):
    return WB.cases(pkg)


@pytest.fixture(scope="module")
def want(wins, oracle):
    return {name: oracle.lba_solve(w) for name, w in wins.items()}


@pytest.fixture(scope="module")
def solved(pkg, gpu, wins):
    """{layout: {name: result}} of every window alone, and of all of them in one call (the big window beside window 1 in one launch)"""
    alone = {layout: dict(zip(wins, WB.solve(pkg, layout, wins.values()))) for layout in WB.LAYOUTS}
    batch = {layout: dict(zip(wins, WB.solve(pkg, layout, wins.values(), batch=True))) for layout in WB.LAYOUTS}
    return alone, batch


def test_the_windows_are_what_they_are_meant_to_be(wins, want):
    assert tuple(wins) == NAMES and sorted(GOLDEN) == sorted(NAMES)
    assert all(sorted(v) == sorted(WB.LAYOUTS) and all(len(h) == 64 for h in v.values()) for v in GOLDEN.values())
    # 1: the edges are not in landmark order (pt_k is a real permutation), mono and stereo mixed
    w = wins["permuted"]
    assert (w["n_poses"], int(w["pose_fixed"].sum()), w["n_points"]) == (5, 2, 60)
    assert (np.diff(w["edge_point"]) < 0).any() and 0 < int(w["edge_stereo"].sum()) < w["n_edges"]
    # 2: every degree, every free-keyframe degree
    w = wins["degrees"]
    free = np.asarray(w["pose_fixed"])[w["edge_pose"]] == 0
    deg = np.bincount(w["edge_point"], minlength=w["n_points"])
    fdeg = np.bincount(w["edge_point"], weights=free, minlength=w["n_points"]).astype(int)
    assert set(WB.DEGREES) <= set(deg.tolist()) and set(WB.FREE_DEGREES) <= set(fdeg.tolist())
    # 3: the outlier pass masks edges of free and of fixed keyframes; the second optimisation runs on what it rewrote
    w, r = wins["flags"], want["flags"]
    free = np.asarray(w["pose_fixed"])[w["edge_pose"]] == 0
    assert (r["edge_level1"][free] != 0).any() and (r["edge_level1"][~free] != 0).any() and r["iters"][1] > 0
    # 4: rejected trials.  In the first window a step is rejected (lambda grows inside an optimisation) but ends its optimisation: its
    # trials equal its iterations.  In the second, rejected trials are repeated: more trials than iterations.
    r = want["rejected"]
    lt, n1 = r["lambda_trace"], r["iters"][0]
    assert any(lt[i + 1] > lt[i] for i in range(len(lt) - 1) if i + 1 != n1)
    r = want["rejected_repeated"]
    assert r["trials"] > sum(r["iters"])
    # 5: more keyframes than the 16 KB LDS copy of a window's keyframe state holds (walk_lds_bytes, lba_window.h): the device-memory path
    w = wins["big"]
    n_free = int((np.asarray(w["pose_fixed"]) == 0).sum())
    assert n_free == 2 and 56 * w["n_poses"] + 120 * n_free > 16 * 1024 and w["n_edges"] < 3000


@pytest.mark.parametrize("name", NAMES)
def test_layouts_and_batches_give_the_same_bits(solved, name):
    alone, batch = solved
    ref = alone["slots"][name]
    assert ref["status"] == 0
    for layout in WB.LAYOUTS:
        assert _same(alone[layout][name], ref), (layout, "alone")
        assert _same(batch[layout][name], ref), (layout, "batch")


@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(oracle, solved, want, name):
    sys.path.insert(0, os.path.dirname(oracle.__file__))
    import parity
    alone, _ = solved
    for layout in WB.LAYOUTS:
        assert parity.lba_mismatches(alone[layout][name], want[name], tag=f"{name} ({layout})") == []


@pytest.mark.parametrize("name", NAMES)
def test_bits_of_the_parent_build(solved, name):
    alone, _ = solved
    got = {layout: WB.result_digest(alone[layout][name]) for layout in WB.LAYOUTS}
    assert got == GOLDEN[name], f"window {name} changed its bits: {[k for k in got if got[k] != GOLDEN[name][k]]}"
