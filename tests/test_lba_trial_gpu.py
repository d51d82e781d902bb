"""The landmark half of a LocalBA trial and the Levenberg-Marquardt decision alone -- k_points / k_points_walk (solve = 1) with lm_decide in
its last workgroup, k_lin (init = 0), k_transition and k_final, through the tap aos2_debug_lba_trial_device, which runs the host phase of
aos2_lba_solve_batch, enqueues the shipped kernels through its helpers and copies the arena out between the launches -- against
tests/lba_trial_ref.py.

The condition on x_l, the landmarks' scale terms and the landmarks' chi2 terms: omega = |q_dev - q_ref| / (2^-53 M_q) <= 4 x the worst
omega of two float64 models of the operation on the same family of inputs (tests/test_lba_trial_cpu.py runs the models without a device).
Everything that is a plain float64 operation is checked bit for bit: the landmark update and its push(), the scale terms re-formed from the
device's own x_l, the sums in canonical_sums' order, rho, every member of the state record against lba_trial_ref.decide, the restore swap,
the untouched system after a rejected step.  One exception: lambda behind a good-step factor that is not cropped to [1/3, 2/3] depends on
pow(), which no two C libraries round alike; it is held to lba_trial_ref.LAMBDA_POW_BOUND (the device's t * t * t is one ulp off the cube
rounded once on the window of the `alpha` path).

Worst omega per quantity over the families of lba_trial_ref.FAMILIES, float64 models on the CPU (textbook / records) and the device:
    quantity   textbook  records   device (measured on the MI355X)
    x_l        0.145     0.145     0.142
    scale_l    0.00014   0.00018   0.00020
    chi2_l     0.12      0.12      0.092
    chi2 of an edge behind k_transition / k_final (textbook / one reciprocal per edge): 0.081 / 0.085 at the host's estimates, device 0.062
(M is a bound, not an estimate: chi2_l is a sum with cancellation inside every term -- e = obs - proj --, scale_l carries the whole
bound of x_l as its operand's error.)  On the windows of the decision paths that start far from the optimum (chi2 of 1e7) the device
reaches 0.42 / 0.36 / 1.6 against 0.27 / 0.16 / 0.47 of the models on the same inputs.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_system_ref as S  # noqa: E402
import lba_trial_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 4.0
_taps = {}
# what a snapshot is read for (the other arrays of a snapshot hold whatever the arena holds at that moment)
SNAP_KEYS = dict(A=("est", "bk", "Rl", "tmp", "Hll", "b", "e_level1", "e_robust"), B=("est", "bk", "x", "part"), C=("est", "bk", "Hll", "b"),
                 D=("est", "bk", "e_level1", "e_robust", "err", "lrec", "erec_flags"), E=("out_Tcw", "out_xyz", "out_chi2", "out_outlier"))


@pytest.fixture(scope="module")
def ba(pkg, gpu):
    return pkg.LocalBA()


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def lam_of(case):
    """the lambda a case with a factor passes: the factor times lambda_init at the host's estimates (the reference takes the value that was passed)"""
    if case["lam_factor"] is None:
        return 0.0
    k = ("lambda_init", id(case["win"]))
    if k not in _taps:
        _taps[k] = float(S.linearise(case["win"], S.host_estimates(case["win"]), np.float64)["lambda"][0])
    return _taps[k] * case["lam_factor"]


def tap(ba, cases, layout="slots", key=None, fail=None, stop_at_poll=0, **call):
    """one tap call for all cases (kept per key and layout: several tests look at the same launch)"""
    if key is not None and (key, layout) in _taps:
        return _taps[(key, layout)]
    lam = np.array([lam_of(c) for c in cases])
    ba.debug_stop_at_poll(stop_at_poll)
    try:
        got = ba.debug_trial([c["win"] for c in cases], layout=layout, lam=lam if (lam > 0).any() else None, force_solver_failed=fail, **call)
    finally:
        ba.debug_stop_at_poll(0)
    for g in got:
        g["iters"], g["stop_at_poll"] = call.get("iters", (5, 10)), stop_at_poll
    if key is not None:
        _taps[(key, layout)] = got
    return got


def state_equal(got, want, what):
    for k in T.STATE_KEYS:
        a, b = got[k], want[k]
        if k in ("lam", "final_lambda") and want["pow_used"] and b != 0.0:   # (the one operation that is not reproducible bit for bit: pow)
            assert abs(a - b) <= T.LAMBDA_POW_BOUND * abs(b), f"{what}: LmState::{k} is {a!r}, decide() says {b!r}: further than two 1-ulp pow() apart"
            continue
        assert (bits(a) == bits(b)) if isinstance(a, float) else (a == b), f"{what}: LmState::{k} is {a!r}, decide() says {b!r}"
    for k in ("tr_rho", "tr_temp", "tr_cur", "tr_lambda"):
        assert bits(got[k]) == bits(np.array(want[k], np.float64)), f"{what}: {k} {got[k][-1:]!r} against {want[k][-1:]!r}"


def check_trial(case, g):
    """every check of the module docstring on one window's snapshots A, B, C -> (device omegas, worst model omegas, what happened)"""
    name = f"{case['family']}/{case['name']}"
    win, A, B, C = case["win"], g["A"], g["B"], g["C"]
    hp, hl = S.index_maps(win)
    assert g["np"] == len(hp) and g["nl"] == len(hl) and (g["hpose"] == hp).all() and (g["hpoint"] == hl).all(), name
    assert A["st"]["run"] == 1, f"{name}: the trial under test did not run (phase {A['st']['phase']})"
    n6, nl, lam = 6 * g["np"], g["nl"], A["st"]["lam"]
    ok = A["scal3"] != 0.0
    x_p, x_l, b_l = A["x"][:n6], B["x"][n6:].reshape(nl, 3), A["b"][n6:].reshape(nl, 3)
    rejected = B["st"]["err_at"] == 2
    trial_pose, trial_point = (B["bk_pose"], B["bk_point"]) if rejected else (B["pose"], B["point"])
    kept_pose, kept_point = (B["pose"], B["point"]) if rejected else (B["bk_pose"], B["bk_point"])
    # ---- exact: the landmark update, push(), and the swap of a rejected step
    assert bits(trial_point[hl]) == bits(A["point"][hl] + x_l), f"{name}: point != point + x_l"
    assert bits(kept_point[hl]) == bits(A["point"][hl]), f"{name}: the backup of the landmarks"
    assert bits(trial_pose) == bits(A["pose"]) and bits(kept_pose[hp]) == bits(A["bk_pose"][hp]), f"{name}: the poses and their backup"
    if rejected:
        assert bits(B["pose"]) == bits(A["bk_pose"]) and bits(B["point"]) == bits(A["point"]), f"{name}: the estimates are not restored"
    # ---- exact: the scale terms from the device's own x_l, the sums, rho, the state
    t = x_l * (lam * x_l + b_l)
    assert bits(B["part"][nl:]) == bits(((0.0 + t[:, 0]) + t[:, 1]) + t[:, 2]), f"{name}: scale terms of the landmarks"
    temp = T.canonical_sum(B["part"][:nl])
    scale = T.canonical_sum(B["part"][nl:], A["tmp"])
    want, restored = T.decide(A["st"], temp, scale, ok, False, g["iters"], g["stop_at_poll"])
    assert restored == rejected, name
    assert bits(B["st"]["tr_temp"][-1]) == bits(temp if ok else T.DBL_MAX), f"{name}: tempChi {B['st']['tr_temp'][-1]!r} is not the canonical sum {temp!r}"
    if ok:
        assert bits(B["st"]["tr_rho"][-1]) == bits((A["st"]["currentChi"] - temp) / (scale + 1e-3)), f"{name}: rho"
    state_equal(B["st"], want, name)
    # ---- the system after the trial
    if B["st"]["lin"] == 0:
        assert bits(C["Hll"]) == bits(A["Hll"]) and bits(C["b"]) == bits(A["b"]), f"{name}: the system changed without a new linearisation"
    state_equal(C["st"], dict(want, lin=C["st"]["lin"]), name + " (after k_lin)")
    # ---- omega: x_l, scale terms, chi2 terms
    est_lin = T.lin_estimates(A)
    est_trial = dict(pose=trial_pose, point=trial_point, e_level1=A["e_level1"], e_robust=A["e_robust"])
    worst, _, ref = T.model_omegas(win, est_lin, lam, x_p, est_trial)
    om = dict(x_l=T.omega(x_l, ref["x_l"]), scale_l=T.omega(B["part"][nl:], ref["scale_l"]), chi2_l=T.omega(B["part"][:nl], ref["chi2_l"]))
    if B["st"]["lin"] == 1:   # the assembly test's condition on the landmark side of the new system
        est_new = dict(pose=B["pose"], point=B["point"], e_level1=A["e_level1"], e_robust=A["e_robust"])
        sref = S.reference(win, est_new, B["st"]["lam"])
        sworst, _ = S.model_omegas(win, est_new, B["st"]["lam"], ref=sref)
        so = S.omegas(sref, dict(Hll=C["Hll"], b_l=C["b"][n6:].reshape(nl, 3)))
        for q in ("Hll", "b_l"):
            om[q + " (new)"], worst[q + " (new)"] = so[q], sworst[q]
    return om, worst, dict(rejected=rejected, ok=ok, ref=ref, est_trial=est_trial)


def check_family(family, cases, results):
    tol, seen, bad, measured = {}, {}, [], []
    for c, g in zip(cases, results):
        om, worst, info = check_trial(c, g)
        measured.append((c, om, info))
        for q, v in worst.items():
            tol[q] = max(tol.get(q, 0.0), v)
    for c, om, _ in measured:
        for q, (v, where) in om.items():
            if v > seen.get(q, (-1.0,))[0]:
                seen[q] = (v, c["name"], where)
            if not v <= MARGIN * tol[q]:
                bad.append(f"{q}: omega {v:.3g} > {MARGIN:g} x {tol[q]:.3g} in window {family}/{c['name']} at {where}")
    for q in sorted(seen):
        print(f"worst omega {family:8s} {q:12s} device {seen[q][0]:9.3g} (window {seen[q][1]}, at {seen[q][2]})   models {tol[q]:9.3g}")
    assert not bad, "\n".join(bad)
    return [m[2] for m in measured]


# ------------------------------------------------------------------------------------------ the landmark half, by shape
@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_landmark_counts(ba, layout):
    """nl = 1, 31, 32, 33 (a workgroup of the slots layout), 127, 128, 129 (a workgroup of the walk; a lane's second value in canonical_sums),
    2047, 2048, 2049 of degree 2 (the second round of its 16-deep loop): windows of one workgroup and of up to 65, so the hand-over to
    the workgroup that finishes last runs with one and with many."""
    cases = T.cases("nl")
    got = tap(ba, cases, layout, key="nl")
    per = 128 if layout == "walk" else 32
    assert [g["nl"] for g in got] == list(T.NL + T.NL_BIG)
    assert [g["n_part"] for g in got] == [(n + per - 1) // per for n in T.NL + T.NL_BIG] and got[0]["n_part"] == 1 and got[-1]["n_part"] > 16
    info = check_family("nl", cases, got)
    assert all(not i["rejected"] for i in info)


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_landmark_degrees_and_lambda(ba, layout):
    """free-keyframe degrees 0 (fixed keyframes only: x_l = D^-1 b_l), 1, 3, 4, 5, 8, 9, 17 -- around kWalkChunk = 4 and kLmSlots = 8 -- and total
    degrees 1 (mono, seen once: lambda x 1e-8 puts D at the edge of singularity), 5, 6, 7, 12, 13 -- around kWalkChunkE = 6 --, at
    {1e-8, 1, 1e4} x lambda_init."""
    cases = T.cases("degree")
    deg = cases[0]["degrees"]
    assert set(T.FREE_DEGREES) <= {f for _, f in deg} and set(T.TOTAL_DEGREES) <= {d for d, _ in deg}
    w = cases[0]["win"]
    once = np.nonzero(np.bincount(w["edge_point"], minlength=w["n_points"]) == 1)[0]
    assert len(once) and not w["edge_stereo"][np.isin(w["edge_point"], once)].any()
    got = tap(ba, cases, layout, key="degree")
    for c, g in zip(cases, got):
        assert bits(g["A"]["st"]["lam"]) == bits(lam_of(c)), c["name"]
    check_family("degree", cases, got)


def test_reduced_system_forms(ba):
    """np = 1, 8, 40 (k_ldlt_reg) and 41 (k_ldlt_dev): the landmark half behind both reduced-system kernels"""
    cases = T.cases("sizes")
    got = tap(ba, cases, key="sizes")
    assert [g["np"] for g in got] == [1, 8, 40, 41]
    check_family("sizes", cases, got)


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_big_window_beside_a_small_one(ba, layout):
    """2 free + 300 fixed keyframes -- the keyframe state exceeds the walk's LDS budget: the device-memory body -- beside a small window in
    the same launch (the LDS body)"""
    cases = T.cases("big")
    assert 8 * (7 * cases[0]["win"]["n_poses"] + 15 * 2) > 16 * 1024 > 8 * (7 * cases[1]["win"]["n_poses"] + 15 * 3)
    check_family("big", cases, tap(ba, cases, layout, key="big"))


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_edge_kinds_and_huber_sides(ba, layout):
    """mono, stereo and mixed windows; for the reference at least 20 % of the active edges lie on each side of the Huber delta at the
    trial's estimates"""
    cases = T.cases("kinds")
    got = tap(ba, cases, layout, key="kinds")
    info = check_family("kinds", cases, got)
    for c, g, i in zip(cases, got, info):
        st = c["win"]["edge_stereo"]
        assert {"mono": not st.any(), "stereo": st.all(), "mixed": 0.2 < st.mean() < 0.8}[c["name"]]
        assert g["A"]["e_robust"].all() and not g["A"]["e_level1"].any()
        frac = i["ref"]["edges"]["beyond"].mean()
        assert 0.2 <= frac <= 0.8, (c["name"], frac)


def test_same_bits_across_layouts_batches_and_handles(pkg, ba):
    """everything the tap returns is bit for bit the same between the slots and the walk layout, between a window alone and the same window
    shuffled into a batch of mixed sizes, and between two handles"""
    pick = {"nl": ("nl1", "nl33", "nl129", "nl2049"), "sizes": ("np8", "np41"), "degree": ("degree x1",), "big": ("big", "small")}
    cases = [c for f, names in pick.items() for c in T.cases(f) if c["name"] in names]
    rng = np.random.default_rng(10)
    cases = [cases[i] for i in rng.permutation(len(cases))]
    base = tap(ba, cases, "slots", tail=2)
    other = pkg.LocalBA()
    runs = {"walk layout": tap(ba, cases, "walk", tail=2), "second handle": tap(other, cases, "slots", tail=2),
            "alone": [tap(ba, [c], "slots", tail=2)[0] for c in cases], "alone, walk, second handle": [tap(other, [c], "walk", tail=2)[0] for c in cases]}
    other.close()
    for what, res in runs.items():
        for c, a, b in zip(cases, base, res):
            assert bits(a["A"]["x"][:6 * a["np"]]) == bits(b["A"]["x"][:6 * a["np"]]), f"{what}: x_p of window {c['family']}/{c['name']} differs"
            for sn in "ABCDE":
                for k in SNAP_KEYS[sn]:
                    assert a[sn][k].tobytes() == b[sn][k].tobytes(), f"{what}: {k} of snapshot {sn} of window {c['family']}/{c['name']} differs"
                for k in T.STATE_KEYS + ("tr_rho", "tr_temp", "tr_cur", "tr_lambda"):
                    x, y = a[sn]["st"][k], b[sn]["st"][k]
                    assert (bits(x) == bits(y)) if isinstance(x, (float, np.ndarray)) else (x == y), f"{what}: LmState::{k} of snapshot {sn} of {c['name']}"
                assert bits(a[sn]["scal3"]) == bits(b[sn]["scal3"])


# ------------------------------------------------------------------------------------------ the passes that re-form _error
def errors_at(win, snap, at, dt=T.LD):
    """per-edge chi2 (no robust kernel) where LmState::err_at = `at` points: 1 = the estimates, 2 = the backup -> lba_trial_ref.edge_chi2"""
    pose, point = (snap["pose"], snap["point"]) if at == 1 else (snap["bk_pose"], snap["bk_point"])
    E = win["n_edges"]
    return T.edge_chi2(win, dict(pose=pose, point=point, e_level1=np.zeros(E, np.uint8), e_robust=np.zeros(E, np.uint8)), dt)


def chi2_of_stored(err, win):
    """edge_chi2 of lba_math.h on stored errors: s = 0; s += e_i (w e_i) over 2 (mono) or 3 (stereo) components, float64"""
    w = np.asarray(win["edge_inv_sigma2"], np.float32).astype(np.float64)
    s = (0.0 + err[:, 0] * (w * err[:, 0])) + err[:, 1] * (w * err[:, 1])
    return np.where(np.asarray(win["edge_stereo"]).astype(bool), s + err[:, 2] * (w * err[:, 2]), s)


def check_flags(name, win, flags, chi2_dev, before, at_edge, cur):
    """chi2 and the outlier flags of a pass that re-forms _error from `before` (the snapshot in front of it) where at_edge says (0: the
    stored values, exact): omega on chi2, flags = chi2_ref > threshold or z <= 0 outside the band the models' omega leaves undecided.
    -> (worst omega device, models, the reference's flags, compared mask, chi2_ref)"""
    stereo = np.asarray(win["edge_stereo"]).astype(bool)
    thr = np.where(stereo, T.THRESHOLD[1], T.THRESHOLD[0])
    E = win["n_edges"]
    v, M, mdl, mdl2 = np.zeros(E, T.LD), np.zeros(E, T.LD), np.zeros(E), np.zeros(E)
    stored = chi2_of_stored(before["err"], win)
    for at in (1, 2):
        sel = at_edge == at
        if sel.any():
            ref, m64 = errors_at(win, before, at), errors_at(win, before, at, np.float64)
            pose, point = (before["pose"], before["point"]) if at == 1 else (before["bk_pose"], before["bk_point"])
            v[sel], M[sel], mdl[sel] = ref["chi2"][0][sel], (ref["chi2"][1] + ref["chi2"][2])[sel], m64["chi2"][0][sel]
            mdl2[sel] = T.edge_chi2_records(win, dict(pose=pose, point=point))[sel]
    sel0 = at_edge == 0
    assert bits(chi2_dev[sel0]) == bits(stored[sel0]), f"{name}: the chi2 of an edge that kept its _error is not formed from the stored values"
    v[sel0], M[sel0] = stored[sel0], 1.0
    live = ~sel0
    om_dev = T.omega(chi2_dev[live], (v[live], M[live]))[0]
    om_mdl = max(T.omega(m[live], (v[live], M[live]))[0] for m in (mdl, mdl2))   # (the textbook form and the one-reciprocal form)
    depth = errors_at(win, cur, 1)["depth"]
    want = (v > thr) | ~(depth > 0)
    band = np.where(live, MARGIN * om_mdl * S.U53 * M, 0)
    compared = np.abs(v - thr) > band
    assert (flags[compared] != 0).tolist() == want[compared].tolist(), f"{name}: outlier flags"
    assert (~compared).sum() <= 0.01 * E, name
    return om_dev, om_mdl, want, compared, v.astype(np.float64), depth


def check_transition(case, g):
    """snapshot D against C: k_transition re-forms _error where C's err_at says, stores it, flags, drops the robust kernels, masks the
    linearisation records, keeps the edge records in step, counts, and enters the second optimisation"""
    name = f"{case['family']}/{case['name']}"
    win, C, D = case["win"], g["C"], g["D"]
    E = win["n_edges"]
    assert C["st"]["xmark"] == 1 and C["st"]["phase"] == 1, name
    at = C["st"]["err_at"]
    stereo = np.asarray(win["edge_stereo"]).astype(bool)
    # the stored _error is the residual pass's, bit for bit reproducible only through chi2: compare its chi2 under the omega condition
    om_dev, om_mdl, want, compared, chi2_ref, depth = check_flags(name + " (k_transition)", win, D["e_level1"], chi2_of_stored(D["err"], win), C,
                                                                  np.full(E, at), C)
    assert om_dev <= MARGIN * om_mdl, f"{name}: chi2 of the stored _error: omega {om_dev:.3g} > {MARGIN:g} x {om_mdl:.3g}"
    lv = D["e_level1"].astype(bool)
    assert not D["e_robust"].any(), name
    assert (D["erec_flags"] == (stereo[g["pt_k"]] * 1 + lv[g["pt_k"]] * 4)).all(), f"{name}: EdgeRec flags"
    pp = g["pl_pos"]
    masked = lv & (pp >= 0)
    assert masked.any() and bits(D["lrec"][pp[masked]] + 0.0) == bits(np.zeros((masked.sum(), 4))), f"{name}: the record of a masked edge"
    keep = ~lv & (pp >= 0)
    assert bits(D["lrec"][pp[keep]]) == bits(C["lrec"][pp[keep]]), name
    assert bits(D["est"]) == bits(C["est"]) and bits(D["bk"]) == bits(C["bk"]), name
    want_st = T.transition_state(C["st"], int((~lv).sum()), g["iters"], g["stop_at_poll"])
    for k in T.STATE_KEYS:
        assert D["st"][k] == want_st[k], f"{name}: LmState::{k} behind k_transition is {D['st'][k]!r}, expected {want_st[k]!r}"
    thr = np.where(stereo, T.THRESHOLD[1], T.THRESHOLD[0])
    below = ((chi2_ref > thr / 2) & (chi2_ref <= thr))[compared].mean()
    above = ((chi2_ref > thr) & (chi2_ref < 2 * thr))[compared].mean()
    return dict(om_dev=om_dev, om_mdl=om_mdl, below=below, above=above, want=want, chi2_ref=chi2_ref, depth=depth)


def check_final(case, g):
    """snapshot E against D: k_final's chi2 of every edge (an inactive edge: from the _error it kept), the outlier flags, the write-back"""
    name = f"{case['family']}/{case['name']}"
    win, D, E_ = case["win"], g["D"], g["E"]
    at_edge = np.where(D["e_level1"].astype(bool), 0, D["st"]["err_at"])
    om_dev, om_mdl, _, _, _, _ = check_flags(name + " (k_final)", win, E_["out_outlier"], E_["out_chi2"], D, at_edge, D)
    assert om_dev <= MARGIN * om_mdl, f"{name}: out_chi2: omega {om_dev:.3g} > {MARGIN:g} x {om_mdl:.3g}"
    assert E_["out_xyz"].tobytes() == D["point"].astype(np.float32).tobytes(), f"{name}: out_xyz"
    Tm = T.pose_matrix(D["pose"])
    T32 = np.array(Tm, np.float64).astype(np.float32)   # (long double -> float32 through float64: double rounding stays within the ulp allowed)
    got = E_["out_Tcw"].reshape(-1, 4, 4)
    assert (np.abs(got[:, :3].astype(np.float64) - T32[:, :3]) <= np.spacing(np.abs(T32[:, :3]))).all(), f"{name}: out_Tcw"
    assert got[:, 3].tobytes() == np.tile(np.array([0, 0, 0, 1], np.float32), len(got)).tobytes(), f"{name}: the fourth row"
    for k in T.STATE_KEYS:
        assert E_["st"][k] == D["st"][k], name
    return om_dev, om_mdl


def test_second_optimisation_and_its_last_iteration(ba):
    """the first trial of the second optimisation -- the planted edges masked, no robust kernel --, which with iters_second = 1 is also its
    last: accepted, phase 3; k_final then re-forms _error from the estimates (err_at = 1) and reads the masked edges' stored one"""
    cases = T.cases("stage1")
    got = tap(ba, cases, key="stage1", **T.CALL["stage1"])
    info = check_family("stage1", cases, got)
    for c, g, i in zip(cases, got, info):
        A, B = g["A"]["st"], g["B"]["st"]
        assert A["phase"] == 2 and A["trials"] == (5, 0) and A["iters_done"] == (5, 0) and A["it"] == 0, (c["name"], A)
        assert not g["A"]["e_robust"].any() and np.nonzero(g["A"]["e_level1"])[0].tolist() == c["planted"].tolist(), c["name"]
        assert not i["rejected"] and B["phase"] == 3 and B["run"] == 0 and B["iters_done"] == (5, 1) and B["err_at"] == 1 and B["lin"] == 0, (c["name"], B)
        assert all(g["D"]["st"][k] == g["C"]["st"][k] for k in T.STATE_KEYS), c["name"]   # (no outlier pass here)
        om_dev, om_mdl = check_final(c, g)
        print(f"worst omega stage1   out_chi2     device {om_dev:9.3g} (window {c['name']})   model {om_mdl:9.3g}")


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_outlier_pass_and_final_check(ba, layout):
    """the last trial of the first optimisation (accepted: phase 1, xmark 1), k_transition and k_final on windows with residuals of two
    standard deviations, planted gross outliers and a landmark behind a fixed keyframe"""
    cases = T.cases("tail")
    got = tap(ba, cases, layout, key="tail", **T.CALL["tail"])
    info = check_family("tail", cases, got)
    for c, g, i in zip(cases, got, info):
        B = g["B"]["st"]
        assert not i["rejected"] and B["phase"] == 1 and B["xmark"] == 1 and B["run"] == 0 and B["iters_done"] == (5, 0) and B["trials"] == (5, 0), (c["name"], B)
        t = check_transition(c, g)
        print(f"worst omega tail     chi2 (D)     device {t['om_dev']:9.3g} (window {c['name']})   model {t['om_mdl']:9.3g};  within a factor 2 "
              f"below / above the threshold: {t['below']:.3f} / {t['above']:.3f}")
        assert t["below"] >= 0.05 and t["above"] >= 0.05, c["name"]
        e = c["behind"]
        assert g["D"]["e_level1"][e] == 1 and t["chi2_ref"][e] < 1.0 and t["depth"][e] < 0, f"{c['name']}: the edge behind its keyframe"
        assert g["D"]["e_level1"][c["planted"]].all() and g["D"]["st"]["phase"] == 2 and g["D"]["st"]["initp"] == 1, c["name"]
        om_dev, om_mdl = check_final(c, g)
        print(f"worst omega tail     out_chi2     device {om_dev:9.3g} (window {c['name']})   model {om_mdl:9.3g}")
        assert g["E"]["out_outlier"][e] == 1


def test_a_window_whose_edges_all_leave(ba):
    """every observation a gross outlier, one iteration: the outlier pass leaves no edge and the window ends at phase 3"""
    cases = T.cases("all_leave")
    got = tap(ba, cases, key="all_leave", **T.CALL["all_leave"])
    check_family("all_leave", cases, got)
    g = got[0]
    assert g["B"]["st"]["phase"] == 1 and g["B"]["st"]["xmark"] == 1
    assert g["D"]["e_level1"].all() and g["D"]["st"]["n_active"] == 0 and g["D"]["st"]["phase"] == 3 and g["D"]["st"]["initp"] == 0
    want = T.transition_state(g["C"]["st"], 0, g["iters"])
    assert all(g["D"]["st"][k] == want[k] for k in T.STATE_KEYS)


# ------------------------------------------------------------------------------------------ the decision, path by path
def test_decision_paths(pkg, ba):
    """every way a trial can end, reached on the device and asserted from the returned states (each against lba_trial_ref.decide, with all
    checks of check_trial): accepted in the middle of an optimisation, at the last iteration of the first and of the second one; rejected
    and repeated; the tenth trial of an iteration; nBad reaching 3; the stop flag at the repeat poll after a rejected step and at the
    iteration poll; a failed linear solve"""
    def one(family, g):
        c = dict(name=family, family=family, win=g["win"], lam_factor=None)
        info = check_family(family, [c], [g])[0]
        return g["A"]["st"], g["B"]["st"], info

    # accepted in the middle: lin = 1, qmax = 0, iniChi moved
    g = tap(ba, T.cases("nl"), key="nl")[3]
    A, B = g["A"]["st"], g["B"]["st"]
    assert B["err_at"] == 1 and B["lin"] == 1 and B["qmax"] == 0 and B["run"] == 1 and B["iniChi"] == B["currentChi"] < A["iniChi"] and B["it"] == 1
    # the last iteration of the first / second optimisation
    B = tap(ba, T.cases("tail"), key="tail", **T.CALL["tail"])[0]["B"]["st"]
    assert B["err_at"] == 1 and (B["phase"], B["xmark"], B["run"], B["it"]) == (1, 1, 0, 5)
    B = tap(ba, T.cases("stage1"), key="stage1", **T.CALL["stage1"])[0]["B"]["st"]
    assert B["err_at"] == 1 and (B["phase"], B["run"], B["iters_done"]) == (3, 0, (5, 1))
    # rejected and repeated: lambda x ni, ni x 2, err_at 2 -- the seventh trial of the window's first optimisation of 20 iterations
    hard = dict(win=T.window_rejecting(pkg), lam_factor=None)
    g = dict(tap(ba, [hard], iters=(20, 10), trials_before=6)[0], win=hard["win"])
    A, B, info = one("rejected", g)
    assert info["rejected"] and info["ok"] and B["tr_rho"][-1] < 0 and B["err_at"] == 2 and B["run"] == 1 and B["lin"] == 0
    assert B["lam"] == A["lam"] * A["ni"] and B["ni"] == 2 * A["ni"] and B["qmax"] == A["qmax"] + 1 == 1 and B["it"] == A["it"] and B["polls"] == A["polls"] + 1
    # ... and the stop flag seen at that repeat poll: phase 3, err_at 2; k_final re-forms _error from the backup
    g = dict(tap(ba, [hard], iters=(20, 10), trials_before=6, stop_at_poll=A["polls"] + 1, tail=2)[0], win=hard["win"])
    A, B, info = one("stop_repeat", g)
    assert info["rejected"] and B["stop_poll"] == A["polls"] + 1 and (B["phase"], B["run"], B["err_at"], B["xmark"]) == (3, 0, 2, 0)
    assert g["D"]["st"]["err_at"] == 2
    check_final(dict(name="stop_repeat", family="paths", win=hard["win"]), g)
    # the stop flag seen at the iteration poll after an accepted step
    c33 = T.cases("nl")[3]
    g = dict(tap(ba, [c33], stop_at_poll=3)[0], win=c33["win"])
    A, B, info = one("stop_iteration", g)
    assert not info["rejected"] and B["stop_poll"] == 3 and (B["phase"], B["run"], B["err_at"], B["it"], B["polls"]) == (3, 0, 1, 1, 4)
    # a failed linear solve: tempChi = DBL_MAX, rho = -1, rejected and repeated, the estimates restored
    g = dict(tap(ba, [c33], fail=[1])[0], win=c33["win"])
    A, B, info = one("solver_failed", g)
    assert not info["ok"] and info["rejected"] and B["tr_temp"][-1] == T.DBL_MAX and B["tr_rho"][-1] == -1.0 and B["solver_failed"] == 1 and B["run"] == 1
    # nBad reaching 3: at 1e9 x lambda_init every step is accepted and improves chi2 by less than 0.1 %
    cn = T.cases("nbad")[0]
    g = dict(tap(ba, [cn], **T.CALL["nbad"])[0], win=cn["win"])
    A, B, info = one("nbad", g)
    assert not info["rejected"] and A["nBad"] == 2 and B["nBad"] == 3 and B["tr_rho"][-1] > 0 and (B["phase"], B["run"], B["it"], B["xmark"]) == (1, 0, 3, 1)
    # the tenth rejection: trial 23 of the window, the tenth of the ninth iteration of its second optimisation; k_final re-forms _error from
    # the backup (err_at = 2)
    g = dict(tap(ba, [hard], trials_before=22, tail=2)[0], win=hard["win"])
    A, B, info = one("tenth", g)
    assert info["rejected"] and info["ok"] and A["qmax"] == 9 and A["phase"] == 2 and (B["qmax"], B["phase"], B["run"], B["err_at"]) == (10, 3, 0, 2)
    assert B["iters_done"] == (5, A["it"] + 1) and B["polls"] == A["polls"] + 1   # (no repeat poll: qmax < 10 fails first; the loop condition's)
    check_final(dict(name="tenth", family="paths", win=hard["win"]), g)
    # a good-step factor inside (1/3, 2/3) -- 1 - (2 rho - 1)^3 itself -- and rho == 0 (neither accepted nor repeated: Terminate)
    h46 = dict(win=T.window_rho_zero(pkg), lam_factor=None)
    g = dict(tap(ba, [h46], trials_before=1)[0], win=h46["win"])
    A, B, info = one("alpha", g)
    assert not info["rejected"] and 1. / 3. < B["lam"] / A["lam"] < 2. / 3.
    g = dict(tap(ba, [h46], trials_before=8)[0], win=h46["win"])
    A, B, info = one("rho_zero", g)
    assert info["rejected"] and B["tr_rho"][-1] == 0.0 and (B["phase"], B["run"], B["err_at"], B["qmax"]) == (3, 0, 2, 1) and B["polls"] == A["polls"] + 1


def test_outlier_pass_after_a_step_that_was_not_accepted(ba):
    """lambda = 1e30 x lambda_init: the step changes no estimate, tempChi == currentChi, rho == 0 -- the first optimisation ends with pop()
    (err_at = 2) by the third way an iteration can end; the backup equals the estimates here (a backup that differs:
    test_tenth_rejection_ends_the_first_optimisation)"""
    c = dict(T.cases("tail")[0], lam_factor=1e30)
    g = tap(ba, [c], tail=2)[0]
    check_family("rho0", [c], [g])
    B = g["B"]["st"]
    assert B["tr_rho"][-1] == 0.0 and (B["phase"], B["xmark"], B["run"], B["err_at"], B["it"]) == (1, 1, 0, 2, 1)
    assert g["C"]["st"]["err_at"] == 2
    check_transition(c, g)
    assert g["D"]["st"]["phase"] == 2
    check_final(c, g)


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_tenth_rejection_ends_the_first_optimisation(pkg, ba, layout):
    """lambda = 1e-24 x lambda_init on a window far from the optimum: the ten trials of the first iteration are all rejected (rho = -0.57
    in float64: tests/test_lba_trial_cpu.py), the tenth ends the first optimisation with pop() -- phase 1, xmark 1, err_at 2 and a backup
    that differs from the estimates --, k_transition re-forms _error from that backup, k_final reads what it stored"""
    c = dict(name="tenth_first", family="tenth_first", win=T.window_rejecting(pkg), lam_factor=T.TENTH_LAMBDA_FACTOR)
    g = tap(ba, [c], layout, key="tenth_first", trials_before=9, tail=2)[0]
    info = check_family("tenth_first", [c], [g])[0]
    A, B, C = g["A"]["st"], g["B"]["st"], g["C"]
    assert (A["phase"], A["it"], A["qmax"], A["trials"]) == (0, 0, 9, (9, 0)) and (A["tr_rho"] < 0).all() and bits(A["lam"]) == bits(lam_of(c) * 2.0 ** 45)
    assert info["rejected"] and B["tr_rho"][-1] < 0 and (B["phase"], B["xmark"], B["run"], B["err_at"], B["qmax"]) == (1, 1, 0, 2, 10)
    assert B["iters_done"] == (1, 0) and B["trials"] == (10, 0)
    hp, hl = g["hpose"], g["hpoint"]
    assert C["st"]["err_at"] == 2 and (C["bk_pose"][hp] != C["pose"][hp]).any(axis=1).all() and (C["bk_point"][hl] != C["point"][hl]).any(axis=1).mean() > 0.9
    t = check_transition(c, g)
    # the errors came from the backup: at the estimates the same edges give another chi2
    at_est = errors_at(c["win"], C, 1, np.float64)["chi2"][0]
    assert np.abs(at_est - t["chi2_ref"]).max() > 1e-3 * np.abs(t["chi2_ref"]).max()
    assert g["D"]["st"]["phase"] == 2 and g["D"]["st"]["initp"] == 1
    check_final(c, g)
