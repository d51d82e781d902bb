"""Writes tests/golden/lba_walk_bits.json: SHA-256 digests of what LocalBundleAdjustment returns (poses, points, outlier flags, chi2 of
every edge, iteration and trial counts) for the windows of cases() below, in both landmark-kernel layouts (AOS2_LBA_LAYOUT = walk,
slots), every window solved alone.  Needs the built library and a device.  The file pins the BITS of whole solves: it was recorded
with the build before the walk layout's kernels read packed edge records and the window's keyframe state from LDS -- changes of where
values are kept, not of how they are formed -- so every later build reproduces it.  Regenerate it only with a build whose results are
meant to differ, and say so.
    python tests/golden/make_lba_walk_bits.py [output path]"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import lba_system_ref as R  # noqa: E402

LAYOUTS = ("walk", "slots")
EDGE_KEYS = ("edge_pose", "edge_point", "edge_obs", "edge_stereo", "edge_inv_sigma2")
# landmark degrees around the chunk sizes of the walks' three loops (4 free-keyframe edges, 4 and 6 edges of any keyframe) ...
DEGREES = (1, 4, 5, 6, 7, 8, 9, 12, 13)
# ... and how many of a landmark's keyframes are free (0: a landmark that only fixed keyframes see)
FREE_DEGREES = (0, 1, 4, 5, 8, 9)
# The big window: the keyframe state a landmark workgroup of the walks stages in LDS is the window's poses (7 doubles each) and, in a
# trial, the update x (6 doubles) and the linearisation's rotation (9 doubles) of every free keyframe: 56 n_poses + 120 n_free bytes
# (walk_lds_bytes, lba_window.h).  With 2 free keyframes that exceeds the 16 KB budget from (16384 - 240) / 56 = 288.3, i.e. 289 keyframes,
# on: such a window reads device memory, beside the small windows of the same launch that read LDS.
BIG_FIXED = 300
_cache = {}


def shuffled(win, seed):
    """the window with its edges in another order (a seeded permutation of every per-edge array) -> (window, permutation)"""
    perm = np.random.default_rng(seed).permutation(win["n_edges"])
    out = dict(win)
    for k in EDGE_KEYS:
        out[k] = np.ascontiguousarray(np.asarray(win[k])[perm])
    return out, perm


def sees_small(rng):
    """3 free + 2 fixed keyframes, 60 landmarks seen by 2 .. 5 of them, at least one free"""
    sees = []
    for l in range(60):
        d = int(rng.integers(2, 6))
        ks = set(int(k) for k in rng.choice(5, d, replace=False))
        if not ks & {0, 1, 2}:
            ks.add(l % 3)
        sees.append(sorted(ks))
    return sees


def window_one(outliers=False):
    """window 1: mono and stereo mixed, edges shuffled; outliers: +-60 .. 200 px planted on edges of free and of fixed keyframes"""
    sees = sees_small(np.random.default_rng(11))
    planted = ()
    if outliers:
        ep = np.array([k for ks in sees for k in ks])
        el = np.array([l for l, ks in enumerate(sees) for _ in ks])
        deg = np.array([len(ks) for ks in sees])
        cand = np.flatnonzero(deg[el] >= 4)
        planted = np.concatenate([cand[ep[cand] < 3][::5], cand[ep[cand] >= 3][::4]])
    win = R.make_window(1101, 3, 2, sees, kinds="mixed", huber_split=False, noise=0.5, perturb=0.03, outliers=planted, depths=(3.0, 40.0))
    return shuffled(win, 1102)[0]


def sees_degrees(n_free=9, n_fixed=6):
    """every degree of DEGREES with every free-keyframe degree of FREE_DEGREES that fits, twice; then landmarks that keep every
    keyframe well observed"""
    rng = np.random.default_rng(12)
    sees, pairs = [], []
    for d in DEGREES:
        for f in FREE_DEGREES:
            if f > d or d - f > n_fixed:
                continue
            for _ in range(2):
                ks = sorted(int(k) for k in rng.choice(n_free, f, replace=False)) + sorted(n_free + int(k) for k in rng.choice(n_fixed, d - f, replace=False))
                sees.append(ks)
                pairs.append((d, f))
    for i in range(n_free):
        for r in range(8):
            sees.append(sorted({i, (i + 1 + r % 3) % n_free, n_free + r % n_fixed}))
    return sees, pairs


def window_degrees():
    sees, pairs = sees_degrees()
    assert {d for d, _ in pairs} == set(DEGREES) and {f for _, f in pairs} == set(FREE_DEGREES)
    # (stereo observations: a landmark seen once is still determined)
    win = R.make_window(1201, 9, 6, sees, kinds="stereo", huber_split=False, noise=0.5, perturb=0.03, depths=(3.0, 40.0))
    return shuffled(win, 1202)[0]


def window_hard(pkg, seed, rot_sigma, trans_sigma, point_sigma):
    """a window that starts far from the optimum: Levenberg-Marquardt rejects steps (lambda grows, the estimates are restored)"""
    prob = pkg.synth.synth_lba_problem(seed, n_local=5, n_fixed=3, n_points=250, stereo_frac=0.3)
    return pkg.synth.perturb_lba_problem(prob, seed, rot_sigma, trans_sigma, point_sigma)


def window_big():
    """2 free keyframes and BIG_FIXED fixed ones that observe 2 landmarks each: 100 landmarks of degree 8, 800 edges"""
    sees = [[0, 1] + [2 + (6 * l + r) // 2 for r in range(6)] for l in range(100)]
    assert max(k for ks in sees for k in ks) == 2 + BIG_FIXED - 1
    win = R.make_window(1501, 2, BIG_FIXED, sees, kinds="mixed", huber_split=False, noise=0.5, perturb=0.03, depths=(3.0, 40.0))
    assert win["n_edges"] < 3000 and all(int((win["edge_pose"] == k).sum()) == 2 for k in range(2, 2 + BIG_FIXED))
    return shuffled(win, 1502)[0]


def cases(pkg):
    """-> {name: window}: an edge order that is a real permutation; degrees around the walks' chunk sizes; flags the outlier pass
    rewrites; a rejected trial that ends its optimisation, and rejected trials that are repeated; hundreds of keyframes"""
    if not _cache:
        _cache.update(permuted=window_one(), degrees=window_degrees(), flags=window_one(outliers=True), rejected=window_hard(pkg, 42, 0.5, 3, 2),
                      rejected_repeated=window_hard(pkg, 43, 1.0, 6, 4), big=window_big())
    return _cache


def result_digest(r):
    h = hashlib.sha256()
    for k, dt in (("pose_Tcw", np.float32), ("point_xyz", np.float32), ("edge_outlier", np.uint8), ("edge_chi2", np.float64),
                  ("iters", np.int64), ("trials", np.int64)):
        h.update(np.ascontiguousarray(r[k], dt).tobytes())
    return h.hexdigest()


def solve(pkg, layout, windows, batch=False):
    """the windows solved by a fresh handle in the given landmark-kernel layout, each alone or all in one call"""
    old = os.environ.get("AOS2_LBA_LAYOUT")
    os.environ["AOS2_LBA_LAYOUT"] = layout
    try:
        ba = pkg.LocalBA()
        out = ba.LocalBundleAdjustmentBatch(list(windows)) if batch else [ba.LocalBundleAdjustment(w) for w in windows]
        ba.close()
    finally:
        if old is None:
            del os.environ["AOS2_LBA_LAYOUT"]
        else:
            os.environ["AOS2_LBA_LAYOUT"] = old
    return out


def digests(pkg):
    wins = cases(pkg)
    return {name: {layout: result_digest(solve(pkg, layout, [w])[0]) for layout in LAYOUTS} for name, w in wins.items()}


def main():
    import __graft_entry__ as entry
    pkg = entry.load_package()
    out = digests(pkg)
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "lba_walk_bits.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(out), "windows")


if __name__ == "__main__":
    main()
