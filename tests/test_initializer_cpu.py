"""aos2_debug_initializer_host (csrc/initializer.h run serially on the CPU) against tests/initializer_ref.py, the independent Python
restatement of src/Initializer.cc under DESIGN.md section 2 item 12: every result byte, parallax within 1 float ulp (glibc's acos
here, ocml's on the device).  Then the pieces of item 12 alone against their definitions, the scene outcomes, and the refusals.

The generator condition.  A seed is discarded when a decision of its run lies closer than 16 float ulps to its threshold (a chi
square against 5.991 / 3.841, RH against 0.40, a reprojection error against 4 sigma^2, cosParallax against 0.99998, the parallax
against 1.0, two iterations that tie for the best score); at most 10 % may be.  CONDITIONED holds such seeds: general scenes with
noise and outliers (1 of 40 candidates measured discarded, by a cosine).  It cannot hold for the other scene types, whatever the
seed, and STRUCTURAL lists them apart: exact scenes and a static camera tie by construction (every iteration reaches the same
score, and the strict `>` keeps the first); planar, pure-rotation and low-parallax scenes evaluate cosParallax on points whose
parallax is below half a degree, where a float cosine takes only ~670 distinct values, so a band of +-16 ulps around 0.99998 is a
twentieth of them (measured: 3 to 12 of 16 seeds).  Both lists are compared byte for byte; the condition is asserted on the first."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import initializer_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = float(np.finfo(np.float32).eps)
CANDIDATES = list(range(12))            # general scenes, noise 0.3 px, 20 % outliers
STRUCTURAL = [("planar", 0, 0.0), ("general", 0, 0.0), ("planar", 3, 0.2), ("rotation", 1, 0.0), ("rotation", 2, 0.2), ("low_parallax", 1, 0.2),
              ("static", 0, 0.0), ("general", 2, 0.5)]


def public(P):
    return {k: v for k, v in P.items() if k not in ("kind", "R21", "t21", "outlier")}


@pytest.fixture(scope="module")
def world(pkg):
    S = pkg.synth
    cand = [S.synth_two_view(s, "general", n_matches=80, iterations=50, outlier_frac=0.2, noise=0.3, n_extra=20) for s in CANDIDATES]
    cand_ref = [R.solve(P) for P in cand]
    struct = [S.synth_two_view(s, kind, n_matches=70, iterations=30, outlier_frac=out, noise=0.3 if out else 0.0, n_extra=15 * (s % 2))
              for kind, s, out in STRUCTURAL]
    struct.append(S.synth_two_view(5, "planar", n_matches=65, iterations=40, opposite=True))
    struct_ref = [R.solve(P) for P in struct]
    keep = [k for k, r in enumerate(cand_ref) if r["margin_ulps"] >= 16]
    problems = [cand[k] for k in keep] + struct
    want = [cand_ref[k] for k in keep] + struct_ref
    return dict(cand_ref=cand_ref, problems=problems, want=want, tap=pkg.capi.debug_initializer_host([public(P) for P in problems]))


def test_generator_condition_holds_for_the_conditioned_seeds(world):
    margins = [r["margin_ulps"] for r in world["cand_ref"]]
    discarded = [(CANDIDATES[k], min(r["margins"], key=r["margins"].get), r["margin_ulps"]) for k, r in enumerate(world["cand_ref"]) if r["margin_ulps"] < 16]
    print("margins in ulps:", [round(m, 1) for m in margins], "discarded:", discarded)
    assert len(discarded) <= 0.10 * len(CANDIDATES)


def test_host_tap_equals_the_reference_in_every_byte(world):
    for k, (t, w) in enumerate(zip(world["tap"], world["want"])):
        assert R.raw(t) == R.raw(w), (k, {x: (t[x], w[x]) for x in ("status", "initialized", "used_homography", "SH", "SF", "n_hypotheses")})
        assert R.parallax_ulps(t["parallax"], w["parallax"]) <= 1, (k, t["parallax"], w["parallax"])
    outcomes = {(w["used_homography"], w["initialized"]) for w in world["want"]}
    assert outcomes == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_batched_alone_and_permuted_give_the_same_bytes(pkg, world):
    probs = [public(P) for P in world["problems"]]
    tap = world["tap"]
    for k in (0, len(probs) - 1):
        assert R.raw(pkg.capi.debug_initializer_host([probs[k]])[0]) == R.raw(tap[k])
    order = list(np.random.default_rng(1).permutation(len(probs)))
    got = pkg.capi.debug_initializer_host([probs[k] for k in order])
    assert [R.raw(a) + a["parallax"].tobytes() for a in got] == [R.raw(tap[k]) + tap[k]["parallax"].tobytes() for k in order]
    assert pkg.capi.debug_initializer_host([]) == []


# ------------------------------------------------------------------------------------------------------ the pieces of item 12 alone
@pytest.mark.parametrize("rows,cols", [(16, 9), (8, 9), (3, 3)])
def test_jacobi_reproduces_the_matrix_from_its_factors(pkg, rows, cols):
    """A = sum_k w[k] u_k v_k^T.  One-sided Jacobi applies at most 30 sweeps of n - 1 rotations to a row, each a float operation that
    perturbs the row by FLT_EPSILON of its norm (two products and a sum per element); the final scale by 1/W adds one more: the
    bound is (30 (n - 1) + 2) FLT_EPSILON ||A||_F per element, derived here, not measured."""
    rng = np.random.default_rng(rows * 16 + cols)
    for trial in range(4):
        A = (rng.normal(0, 1, (rows, cols)) * 10.0 ** rng.integers(-2, 3)).astype(np.float32)
        left, w, right = pkg.capi.debug_initializer_svd(A)
        wide = rows < cols
        n = rows if wide else cols
        rl, rw, rr = (R.svd_wide if wide else R.svd_general)(A)
        assert left.tobytes() == rl.tobytes() and w.tobytes() == rw.astype(np.float32).tobytes() and right.tobytes() == rr.tobytes()
        L, Rt = left.astype(np.float64), right.astype(np.float64)
        if wide:    # the rows of A were rotated: A[i][:] = sum_k right[k][i] w[k] left[k][:]
            back = sum(w[k] * np.outer(Rt[k], L[k]) for k in range(n))
        else:       # the columns of A were: A[:][j] = sum_k left[k][:] w[k] right[k][j]
            back = sum(w[k] * np.outer(L[k], Rt[k]) for k in range(n))
        bound = (30 * (n - 1) + 2) * EPS * np.linalg.norm(A.astype(np.float64))
        err = np.abs(back - A).max()
        print(rows, cols, "error", err, "bound", bound)
        assert err <= bound
        assert (np.diff(w) <= 0).all()


def test_completion_row_of_the_wide_case_is_unit_and_orthogonal(pkg):
    """row 8 of vt for an 8x9 matrix comes from no rotation.  After two passes of subtraction against unit rows its residual along
    each is a rounding error of the pass: 9 products and sums of magnitudes <= 1, each FLT_EPSILON / 2, and the stored floats of
    both rows carry FLT_EPSILON / 2 each: |dot| <= (9 + 2) FLT_EPSILON, and the same for |norm^2 - 1|."""
    rng = np.random.default_rng(7)
    for trial in range(6):
        A = rng.normal(0, 1, (8, 9)).astype(np.float32)
        left, w, right = pkg.capi.debug_initializer_svd(A)
        row = left[8].astype(np.float64)
        dots = np.abs(left[:8].astype(np.float64) @ row)
        print("norm^2 - 1:", row @ row - 1, "largest dot:", dots.max())
        assert abs(row @ row - 1) <= 11 * EPS and dots.max() <= 11 * EPS
        assert np.abs(A.astype(np.float64) @ row).max() <= (30 * 7 + 2) * EPS * np.linalg.norm(A.astype(np.float64))   # the null vector


def test_rng_follows_the_recurrence(pkg):
    state, want = 0x12345678, []
    for _ in range(32):
        state = (state & 0xFFFFFFFF) * 4164903690 + (state >> 32)
        assert state < 2 ** 64
        want.append(state & 0xFFFFFFFF)
    assert [int(v) for v in pkg.capi.debug_initializer_rng(32)] == want == R.rng_values(32)
    assert len({v & 256 for v in want}) == 2


def test_inverse_and_determinant_of_a_3x3(pkg):
    """inv(M) M = I: each entry of the float inverse carries FLT_EPSILON / 2 relative (one rounding of a double), so entry (i, j) of
    the product is off by at most sum_k |inv[i][k]| |M[k][j]| FLT_EPSILON (the double arithmetic behind it is 2^-29 of that)"""
    rng = np.random.default_rng(3)
    for trial in range(8):
        M = rng.normal(0, 1, (3, 3)).astype(np.float32)
        inv, det = pkg.capi.debug_initializer_inv33(M)
        assert inv.tobytes() == R.inv33(M).tobytes() and det == float(R.det33(M))
        assert abs(det - np.linalg.det(M.astype(np.float64))) <= 1e-12 * np.abs(M).max() ** 3 * 6
        bound = (np.abs(inv.astype(np.float64)) @ np.abs(M.astype(np.float64))) * EPS
        assert (np.abs(inv.astype(np.float64) @ M.astype(np.float64) - np.eye(3)) <= bound).all()
    S = np.float32([[1, 2, 3], [2, 4, 6], [0, 1, 5]])
    inv, det = pkg.capi.debug_initializer_inv33(S)
    assert det == 0 and not inv.any() and not R.inv33(S).any()


# ------------------------------------------------------------------------------------------------------------------- scene outcomes
def resolution(P):
    """how far float32 moves R21 and the direction of t21 on this scene: the restatement's result against the generator's motion is
    the float64 truth here (the scene is exact), so the measured distance IS the float32 error; the tolerance is 4 times it"""
    r = R.solve(P)
    dR = float(np.abs(r["R21"].astype(np.float64) - P["R21"]).max())
    dt = float(np.abs(r["t21"].astype(np.float64) - P["t21"]).max())
    return r, dR, dt


def test_exact_scenes_pick_their_model_and_recover_the_motion(pkg):
    """planar -> H, general -> F; R21 and the direction of t21 equal the generator's within 4 x the float32 resolution of the scene,
    measured with the reference and recorded in profiles/initializer_resolution.txt"""
    recorded = {}
    with open(os.path.join(ROOT, "profiles", "initializer_resolution.txt")) as f:
        for line in f:
            if line.startswith(("planar", "general")):
                kind, seed, dR, dt = line.split()[:4]
                recorded[(kind, int(seed))] = (float(dR), float(dt))
    for kind, seed in (("planar", 0), ("planar", 1), ("general", 0), ("general", 3)):
        P = pkg.synth.synth_two_view(seed, kind, n_matches=120, iterations=30)
        t = pkg.capi.debug_initializer_host([public(P)])[0]
        assert t["initialized"] == 1 and t["used_homography"] == (kind == "planar"), (kind, seed)
        dR = np.abs(t["R21"].astype(np.float64) - P["R21"]).max()
        dt = np.abs(t["t21"].astype(np.float64) - P["t21"]).max()
        rR, rt = recorded[(kind, seed)]
        print(kind, seed, "dR", dR, "dt", dt, "recorded resolution", rR, rt)
        assert dR <= 4 * rR and dt <= 4 * rt
        assert int(t["triangulated"].sum()) > 100 and abs(np.linalg.norm(t["t21"].astype(np.float64)) - 1) < 4 * EPS


def test_no_motion_and_too_few_points_do_not_initialise(pkg):
    S = pkg.synth
    rot = pkg.capi.debug_initializer_host([public(S.synth_two_view(1, "rotation", n_matches=120, iterations=30))])[0]
    assert rot["status"] == 0 and rot["initialized"] == 0 and rot["used_homography"] == 1 and rot["n_hypotheses"] == 0   # d1/d2 < 1.00001
    noisy = pkg.capi.debug_initializer_host([public(S.synth_two_view(2, "rotation", n_matches=120, iterations=30, outlier_frac=0.2, noise=0.3))])[0]
    assert noisy["initialized"] == 0 and noisy["n_hypotheses"] == 8 and (noisy["parallax"] < 1).all()                     # no parallax
    static = pkg.capi.debug_initializer_host([public(S.synth_two_view(0, "static", n_matches=120, iterations=30))])[0]
    assert static["status"] == 0 and static["initialized"] == 0 and static["n_hypotheses"] == 0
    assert static["SH"] == static["SF"] == np.float32(R.score_and_pick(np.zeros((1, 120), np.float32), np.zeros((1, 120), np.float32), R.TH_H, R.TH_H)[2])
    few = S.synth_two_view(0, "general", n_matches=40, iterations=30)                                                      # 40 < 50 points
    r = pkg.capi.debug_initializer_host([public(few)])[0]
    assert r["initialized"] == 0 and r["used_homography"] == 0 and r["n_good"].max() == 40 and not r["R21"].any() and not r["P3D"].any()
    assert pkg.capi.debug_initializer_host([dict(public(few), min_triangulated=30)])[0]["initialized"] == 1


def test_sign_of_the_null_vector_changes_nothing_but_the_order_of_the_hypotheses(pkg):
    """CheckHomography and CheckFundamental are exact under negation of the model: same scores, same flags, same winners.  The
    decompositions then return -t for t, which renames the hypotheses (0 <-> 2, 1 <-> 3 of ReconstructF; 0 <-> 3, 1 <-> 2, 4 <-> 7,
    5 <-> 6 of ReconstructH) and leaves every other result byte"""
    for kind, seed, perm in (("general", 0, [2, 3, 0, 1, 4, 5, 6, 7]), ("planar", 0, [3, 2, 1, 0, 7, 6, 5, 4])):
        P = pkg.synth.synth_two_view(seed, kind, n_matches=90, iterations=20, outlier_frac=0.1, noise=0.2)
        a, b = R.solve(P), R.solve(P, flip_null=True)
        keys = tuple(k for k in R.RESULT_KEYS if k not in ("H21", "F21", "n_good"))
        assert a["initialized"] == 1 and R.raw(a, keys) == R.raw(b, keys)
        assert (a["H21"] == -b["H21"]).all() and (a["F21"] == -b["F21"]).all() and a["H21"].any() and a["F21"].any()
        assert (a["n_good"] == b["n_good"][perm]).all() and a["parallax"].tobytes() == b["parallax"][perm].tobytes()
        assert a["scores_h"].tobytes() == b["scores_h"].tobytes() and a["scores_f"].tobytes() == b["scores_f"].tobytes()


def test_collinear_sets_report_no_model(pkg):
    P = R.collinear()
    t = pkg.capi.debug_initializer_host([P])[0]
    w = R.solve(P)
    assert t["status"] == pkg.capi.AOS2_INIT_NO_MODEL == w["status"] and t["initialized"] == 0 and R.raw(t) == R.raw(w)
    assert t["SH"] == 0 and t["SF"] == 0 and t["best_iteration_h"] == -1 and t["best_iteration_f"] == -1
    assert all(np.isnan(s) or s == 0 for s in list(w["scores_h"]) + list(w["scores_f"]))
    rep = dict(P, sets=np.tile(np.int32([0, 0, 1, 1, 2, 2, 3, 3]), (2, 1)))   # a set that repeats its matches is no error either
    assert pkg.capi.debug_initializer_host([rep])[0]["status"] in (0, 1)


def test_argument_errors_are_refused_with_no_byte_written(pkg):
    capi = pkg.capi
    P = public(pkg.synth.synth_two_view(0, "general", n_matches=20, iterations=4))
    good = public(pkg.synth.synth_two_view(1, "general", n_matches=20, iterations=4))
    n = len(P["matches"])
    m_first, m_second, m_neg, s_hi, s_neg = P["matches"].copy(), P["matches"].copy(), P["matches"].copy(), P["sets"].copy(), P["sets"].copy()
    m_first[3, 0], m_second[n - 1, 1], m_neg[0, 0] = len(P["keys1"]), len(P["keys2"]), -1
    s_hi[3, 7], s_neg[0, 0] = n, -1
    bads = [dict(P, matches=m_first), dict(P, matches=m_second), dict(P, matches=m_neg), dict(P, sets=s_hi), dict(P, sets=s_neg),
            dict(P, matches=P["matches"][:7], sets=P["sets"] % 7), dict(P, iterations=0), dict(P, sigma=0.0), dict(P, sigma=-1.0),
            dict(P, sigma=float("nan"))] + [dict(P, null=(name,)) for name in ("keys1", "keys2", "matches", "sets", "inliers_h", "inliers_f", "P3D", "triangulated")]
    for bad in bads:
        with pytest.raises(pkg.AosError) as e:
            capi.debug_initializer_host([good, bad, good], sentinel=0x5A)
        assert e.value.code == capi.AOS2_ERR_ARG
        Rc, outs, before = capi.debug_initializer_host.last
        for k in range(3):
            assert bytes(Rc[k]) == before[k]
            assert all((a.view(np.uint8) == 0x5A).all() for a in outs[k])
    L = capi.lib()
    assert L.aos2_debug_initializer_host(None, None, 1) == capi.AOS2_ERR_ARG and L.aos2_debug_initializer_host(None, None, 0) == 0
    assert L.aos2_debug_initializer_host(None, None, 65) == capi.AOS2_ERR_ARG and L.aos2_initializer_initialize(None, None, None, 0) == capi.AOS2_ERR_ARG


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_class_compiles_and_links_against_the_refstub(pkg, tmp_path, flags):
    """host/Initializer.h compiles (-Wall -Werror, both error conventions) against the stand-ins of tests/cpp/refstub and links
    against libaos2 (the run needs the GPU: tests/test_initializer_class_gpu.py)"""
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "initializer_test.cpp"),
                           "-o", str(tmp_path / "initializer_test"), "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir,
                           "-Wl,-rpath,/opt/rocm/lib"])
