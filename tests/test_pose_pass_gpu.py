"""The edge pass and the outlier pass of pose_optimization_body (csrc/pose_opt.h) alone, in every instantiation -- <4,256>, <8,256>, <9,128>
and <0,256>: the K = 1..4 straight-line block, the K = 2 chunks with an odd tail, the one-by-one loop over global memory -- through the tap
aos2_debug_pose_pass_device, which runs the shipped body itself, against tests/pose_pass_ref.py: the g2o operation in long double with a
scale M per quantity.  The condition on the 21 + 6 + 1 sums and on the stored per-edge chi2:
    omega = |q_dev - q_ref| / (2^-53 M_q) <= 4 x the worst omega of two float64 models of the same pass over the same family of inputs
(the textbook form summed in insertion order; the kernel's form with its per-thread, per-wave, wave-order summation tree); the models run
here on the very inputs (tests/test_pose_pass_cpu.py runs them without a device, holds them to omega <= 16 and shows that the condition
rejects wrong assemblies which the end-to-end criterion -- Tcw within 1e-5, equal flags -- lets pass).  The outlier pass's flags and nBad
are equal to the reference's except where the decision lies within the chi2's allowance of its threshold (at most 1 edge in 1000).

Worst omega per quantity over all families and forms, float64 models on the CPU (textbook / kernel form) and the device:
    quantity     textbook  kernel form  device (measured on the MI355X)
    H diagonal   0.70      0.20         0.20
    H off-diag   0.94      0.17         0.17
    b            0.10      0.096        0.12
    robust chi2  0.0026    0.0011       0.0010
    edge chi2    0.10      0.10         0.094
    edge chi2 recomputed by the outlier pass: quaternion form 0.094, matrix form 0.094, device 0.094; no decision left out
(the robust chi2 and b are sums with heavy cancellation inside every term -- e = obs - proj -- whose M is far above their error.)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_pass_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-5
_taps = {}


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def tap(pkg, cases, mode, key=None):
    """one tap call for all cases (kept per family: several tests look at the same launch)"""
    if key is not None and key in _taps:
        return _taps[key]
    got = pkg.capi.debug_pose_pass_device(cases, mode)
    if key is not None:
        _taps[key] = got
    return got


def check_pass_family(family, form, cases, results):
    """the condition of the module docstring on every case of a family; flags untouched; the stored chi2 of an edge at level 1 stays 0"""
    tol = P.family_tolerance(cases)
    seen, bad = {}, []
    for c, g in zip(cases, results):
        ref = P.reference(c)
        for k, d in (("level1", 0), ("robust", 1), ("outlier", 0)):
            assert bits(g[k]) == bits(P.flags(c, k, d)), (family, form, c["name"], k)
        assert bits(g["pose_out"]) == bits(np.asarray(c["pose"], np.float64)) and g["n_bad"] == 0, (family, form, c["name"])
        assert not g["chi2"][~ref["active"]].any(), (family, form, c["name"])
        for q, v in P.omegas(ref, dict(sums=g["sums"], chi2_edge=g["chi2"])).items():
            if v > seen.get(q, (-1.0,))[0]:
                seen[q] = (v, c["name"])
            if not v <= tol[q]:
                bad.append(f"{q}: omega {v:.3g} > {P.MARGIN:g} x {tol[q] / P.MARGIN:.3g} in frame {family}/{c['name']} (n = {c['n']}), form {form}")
    for q in P.QUANTITIES:
        print(f"worst omega {family:8s} form {form} {q:9s} device {seen[q][0]:9.3g} (frame {seen[q][1]})   models {tol[q] / P.MARGIN:9.3g}")
    assert not bad, "\n".join(bad)


def huber_shares(cases):
    """at least 20 % of the active edges on each side of delta^2 for the reference, every frame with n >= 64 whose edges are all robust"""
    for c in cases:
        if c["n"] >= 64 and P.flags(c, "robust", 1).all():
            ref = P.reference(c)
            share = ref["beyond"][ref["active"]].mean()
            assert 0.2 <= share <= 0.8, (c["name"], share)


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_edge_pass_at_slot_count_boundaries(pkg, gpu, form):
    """correspondence counts around every change of a wave's slot count, per form (pose_pass_ref.SLOT_SIZES: for <8,256> 1279 / 1280 / 1281 are
    five -> six slots, the odd tail of the K = 2 chunks; for <9,128> 1023 / 1024 / 1025 eight -> nine; n = 300 gives the waves of <4,256>
    different counts), mono-only, stereo-only and mixed edges cycling"""
    cases = P.cases("slots", form)
    assert [c["n"] for c in cases] == list(P.SLOT_SIZES[form])
    kinds = [(c["stereo"].any(), c["stereo"].all()) for c in cases if c["n"] > 3]
    assert (False, False) in kinds and (True, True) in kinds and (True, False) in kinds
    huber_shares(cases)
    check_pass_family("slots", form, cases, tap(pkg, cases, 1, key=("slots", form)))


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_edge_pass_level_and_robust_flags(pkg, gpu, form):
    """level1 on a scattered 30 % of the edges, on a whole wave's, on a whole slot's (every e with e / NT = 1), on all but three; robust all on,
    all off and mixed per edge.  Edges at level 1 contribute nothing: other data in them -- another finite point, another observation, a
    weight up to 1e6 -- leaves the 28 sums bit for bit."""
    cases = P.cases("flags", form)
    NT = P.FORMS[form][1]
    assert len(cases) == len(P.LEVEL1_PATTERNS) * len(P.ROBUST_PATTERNS)
    for c in cases:
        lp, rp = c["name"].split("/")
        l1, e = c["level1"].astype(bool), np.arange(c["n"])
        assert {"scatter": 0.25 < l1.mean() < 0.35, "wave": (l1 == ((e % NT) // 64 == 1)).all() and l1.any(), "slot": (l1 == (e // NT == 1)).all() and l1.any(),
                "all_but_three": (~l1).sum() == 3}[lp]
        assert {"on": c["robust"].all(), "off": not c["robust"].any(), "mixed": 0.4 < c["robust"].mean() < 0.6}[rp]
    huber_shares(cases)
    twins = [P.replaced(c) for c in cases]
    got = tap(pkg, cases + twins, 1, key=("flags", form))
    check_pass_family("flags", form, cases, got[:len(cases)])
    for c, a, b in zip(cases, got[:len(cases)], got[len(cases):]):
        assert bits(a["sums"]) == bits(b["sums"]), f"form {form}, {c['name']}: the data of level-1 edges reach the sums"


@pytest.mark.parametrize("form", [0, 3])
def test_edge_pass_geometry(pkg, gpu, form):
    """depths 0.5 .. 50; |t| up to 10 with a rotation near pi; weights of all eight pyramid levels; a fifth of the points behind the camera"""
    cases = P.cases("geometry", form)
    assert [c["name"] for c in cases] == list(P.GEOMETRY)
    check_pass_family("geometry", form, cases, tap(pkg, cases, 1, key=("geometry", form)))


def test_edge_pass_same_bits_alone_in_a_batch_and_again(pkg, gpu):
    """a case alone, the same case inside a batch of mixed sizes and forms, and a second call give the same bits"""
    pick = [c for form in range(4) for c in P.cases("slots", form) if c["n"] in (3, 257, 300, 1025, 1152, 1281, 2500)]
    pick += [P.cases("flags", form)[i] for form in range(4) for i in (0, 10)]
    rng = np.random.default_rng(11)
    pick = [pick[i] for i in rng.permutation(len(pick))]
    base = tap(pkg, pick, 1)
    again = tap(pkg, pick, 1)
    alone = [tap(pkg, [c], 1)[0] for c in pick[::3]]
    for c, a, b in list(zip(pick, base, again)) + list(zip(pick[::3], base[::3], alone)):
        for k in ("sums", "chi2"):
            assert bits(a[k]) == bits(b[k]), f"{k} of {c['family']}/{c['name']}, form {c['form']} differs"


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_outlier_pass(pkg, gpu, form):
    """the reclassification of rounds 0..3 at the boundary sizes of the form.  A scattered third of the edges come in flagged outlier with a
    stale stored chi2 of 1e9: their chi2 is recomputed at the pose (po_edge_error) and meets the condition against the reference, with the
    quaternion-rotate and the matrix form as the float64 models; the other edges keep their stored chi2 bit for bit.  robust is cleared
    exactly in round 2.  Flags and nBad equal the reference's, except edges whose decision changes within the chi2's allowance."""
    cases = P.cases("outlier", form)
    assert len(cases) == 4 * len(P.SLOT_SIZES[form])
    tol = P.recomputed_tolerance(form)
    got = tap(pkg, cases, 2, key=("outlier", form))
    worst, left, total, bad = 0.0, 0, 0, []
    for c, g in zip(cases, got):
        o = P.outlier_reference(c, tol)
        name = f"form {form}, {c['name']}"
        rec, keep = o["recomputed"], ~o["left_out"]
        assert bits(g["robust"]) == bits(o["robust"]) and (g["robust"].any() == (c["it"] < 2)), name
        assert bits(g["chi2"][~rec]) == bits(np.asarray(c["chi2"])[~rec]), f"{name}: a stored chi2 changed"
        om = P.omega(g["chi2"][rec], o["chi2"][0][rec], o["chi2"][1][rec]).max()
        worst = max(worst, om)
        if not om <= tol:
            bad.append(f"{name}: recomputed chi2 omega {om:.3g} > {P.MARGIN:g} x {tol / P.MARGIN:.3g}")
        assert (g["outlier"][keep] == o["outlier"][keep]).all() and (g["level1"] == g["outlier"]).all(), f"{name}: flags"
        assert g["n_bad"] == int(g["outlier"].sum()) and o["n_bad"] <= g["n_bad"] <= o["n_bad"] + int((~keep).sum()), name
        assert g["n_inliers"] == c["n"] - g["n_bad"] and bits(g["pose_out"]) == bits(np.asarray(c["pose"], np.float64)), name
        left += int((~keep).sum())
        total += c["n"]
    print(f"worst omega outlier  form {form} recomputed chi2 device {worst:9.3g}   models {tol / P.MARGIN:9.3g}; {left} of {total} decisions left out")
    assert left * 1000 <= total
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_whole_procedure_in_the_forms_a_single_frame_never_reaches(pkg, oracle, gpu, form):
    """the body unchanged as <8,256>, <9,128> and <0,256> (a frame batch reaches them only with a capacity above 1024, above 256 frames, or a
    capacity above 2048) at the boundary sizes, against the oracle with the criterion of test_pose_optimization_slot_count_boundaries:
    counts and flags equal, Tcw within 1e-5.  n < 3 leaves the pose bit for bit; n < 10 stops after one round (the edges are still robust
    where the form shows them), n >= 10 runs all four."""
    import parity
    cases = P.cases("whole", form)
    assert {2, 9} <= {c["n"] for c in cases}
    got = tap(pkg, cases, 0)
    for c, g in zip(cases, got):
        want = oracle.pose_optimization(c)
        name = f"form {form}, n = {c['n']}"
        assert g["n_inliers"] == want["n_inliers"] and g["n_bad"] == want["n_bad"] and (g["outlier"] == want["outlier"]).all(), name
        ok = parity.close(g["Tcw"].reshape(1, 16), want["Tcw"].reshape(1, 16), TOL)
        assert ok, (name, parity.worst(g["Tcw"].reshape(1, 16), want["Tcw"].reshape(1, 16)))
        if c["n"] < 3:
            assert bits(g["pose_out"]) == bits(np.asarray(c["pose"], np.float64)) and g["n_inliers"] == 0 and not g["outlier"].any(), name
        elif form == 3:
            assert g["robust"].all() if c["n"] < 10 else not g["robust"].any(), name
