"""tests/lba_trial_ref.py without a device: the two float64 models of the landmark half of a trial against the long-double reference on every
family of windows of tests/test_lba_trial_gpu.py (x_p = numpy.linalg.solve of the reference's reduced system in float64, the trial's
estimates = the float64 update), `decide` on hand-worked states for every way a trial can end, `canonical_sum` against math.fsum, and
that the chosen windows reach what the device test asserts.

Worst omega of the models per quantity, measured here (textbook / records), and the bound they are held to (the measured worst rounded
up to the next power of two):
    x_l       0.145    / 0.145      0.25
    scale_l   0.000139 / 0.000179   2^-12
    chi2_l    0.120    / 0.120      0.125
"""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_system_ref as S  # noqa: E402
import lba_trial_ref as T  # noqa: E402

BOUND = dict(x_l=0.25, scale_l=2.0 ** -12, chi2_l=0.125)
_trials = {}


def host_trial(case):
    """the float64 model trial of a case from the host's estimates (stage1 / tail: the planted edges masked, no robust kernel)"""
    k = (case["family"], case["name"])
    if k not in _trials:
        kw = dict(masked=case["planted"], robust=False) if case["family"] == "stage1" else {}
        _trials[k] = T.model_trial(case["win"], S.host_estimates(case["win"], **kw), lam_factor=case["lam_factor"])
    return _trials[k]


@pytest.mark.parametrize("family", T.FAMILIES)
def test_models_meet_the_reference(family):
    seen = {}
    for c in T.cases(family):
        mt = host_trial(c)
        _, per, _ = T.model_omegas(c["win"], mt["est_lin"], mt["lam"], mt["x_p"], mt["est_trial"])
        for name, om in per.items():
            for q, v in om.items():
                seen[(q, name)] = max(seen.get((q, name), 0.0), v)
                assert v <= BOUND[q], f"{family}/{c['name']}: {name} model, {q}: omega {v:.3g} > {BOUND[q]:.3g}"
    for q in T.QUANTITIES:
        print(f"worst omega {family:8s} {q:8s} textbook {seen[(q, 'textbook')]:9.3g}  records {seen[(q, 'records')]:9.3g}")


def test_the_windows_reach_what_the_device_test_asserts():
    """every window's first float64 trial is accepted (the device test's families run their trial under test on an accepting window; the
    decision paths that need a rejected step are forced or read from the returned states there); the Huber sides, the degrees, the
    walk's device-memory body, the landmark behind its keyframe"""
    for family in T.FAMILIES:
        for c in T.cases(family):
            mt = host_trial(c)
            assert mt["rho"] > 0 and math.isfinite(mt["tempChi"]), (family, c["name"], mt["rho"])
    for c in T.cases("kinds"):
        ed = T.edge_chi2(c["win"], host_trial(c)["est_trial"], np.float64)
        assert 0.2 <= ed["beyond"].mean() <= 0.8, c["name"]
    deg = T.cases("degree")[0]["degrees"]
    assert set(T.FREE_DEGREES) <= {f for _, f in deg} and set(T.TOTAL_DEGREES) <= {d for d, _ in deg}
    big, small = (c["win"] for c in T.cases("big"))
    assert 8 * (7 * big["n_poses"] + 15 * 2) > 16 * 1024 > 8 * (7 * small["n_poses"] + 15 * 3)
    for c in T.cases("tail"):
        ed = T.edge_chi2(c["win"], S.host_estimates(c["win"]), np.float64)
        e = c["behind"]
        assert ed["depth"][e] < 0 and ed["chi2"][0][e] < 1e-3 and ed["depth"][e - 1] > 0, c["name"]


def test_the_windows_reach_the_decision_paths(pkg, oracle):
    """the paths that need more than one trial, from the oracle's iteration and trial counts and its lambda per iteration, and from
    float64 model trials: a rejected and repeated step, an iteration of ten trials, rho == 0, three improvements below 0.1 %"""
    w = T.window_rejecting(pkg)
    r = oracle.lba_solve(w)
    assert r["iters"] == (5, 9) and r["trials"] == 5 + 8 + 10   # (the ninth iteration of the second optimisation: ten trials)
    lt = r["lambda_trace"]
    assert lt[-1] / lt[-2] > 2.0 ** 44                          # (nine rejections at least: lambda x 2, x 4, ... x 512; the tenth is decided at rounding level)
    r = oracle.lba_solve(w, iters1=20)
    lt = r["lambda_trace"]
    assert r["iters"] == (20, 10) and r["trials"] == 31        # (one step of the whole solve is repeated: the device test reads which from the
    assert math.isclose(lt[6] / lt[5], 2. / 3.)                # returned trace -- the seventh trial, lambda x 2 and then x 1/3)
    est, lam, ni = S.host_estimates(w), None, 2.0   # ten rejections in the first iteration of the first optimisation
    for k in range(10):
        mt = T.model_trial(w, est, lam=lam, lam_factor=T.TENTH_LAMBDA_FACTOR if lam is None else None)
        assert -0.6 < mt["rho"] < -0.5 and math.isfinite(mt["tempChi"]), (k, mt["rho"])
        lam, ni = mt["lam"] * ni, ni * 2
    r = oracle.lba_solve(T.window_rho_zero(pkg))
    lt = r["lambda_trace"]
    assert r["iters"] == (5, 4) and r["trials"] == 9 and r["chi2_trace"][-1] == 0.0 and lt[-1] / lt[-2] == 2.0
    assert 1. / 3. < lt[1] / lt[0] < 2. / 3.                    # (a good-step factor that is not cropped)
    c = T.cases("nbad")[0]
    est, lam = S.host_estimates(c["win"]), None
    for _ in range(3):
        mt = T.model_trial(c["win"], est, lam=lam, lam_factor=c["lam_factor"] if lam is None else None)
        assert mt["rho"] > 0 and 0 < (mt["currentChi"] - mt["tempChi"]) * 1e3 < mt["currentChi"]
        est, lam = mt["est_trial"], mt["lam"] * max(1. / 3., min(2. / 3., 1 - (2 * mt["rho"] - 1) ** 3))
    c = T.cases("tail")[0]
    mt = T.model_trial(c["win"], S.host_estimates(c["win"]), lam_factor=1e30)
    assert mt["tempChi"] == mt["currentChi"] and mt["rho"] == 0.0


def state(**kw):
    s = dict(lam=1.0, ni=2.0, currentChi=100.0, iniChi=100.0, final_chi2=0.0, final_lambda=0.0, phase=0, run=1, lin=0, initp=0, xmark=0, it=0,
             qmax=0, nBad=0, iters_done=(0, 0), trials=(0, 0), polls=2, stop_poll=0, n_active=77, solver_failed=0, err_at=1, ntr=0,
             tr_rho=[], tr_temp=[], tr_cur=[], tr_lambda=[])
    s.update(kw)
    return s


def changed(before, after):
    return {k: after[k] for k in T.STATE_KEYS if after[k] != before[k]}


def test_decide_on_hand_worked_states():
    # accepted in the middle of the first optimisation: rho = 50 / 60, alpha = 1 - (2/3)^3 = 0.70 -> 2/3
    s = state()
    a, restored = T.decide(s, 50.0, 60.0 - 1e-3, True, False)
    assert not restored and changed(s, a) == dict(lam=2. / 3., currentChi=50.0, iniChi=50.0, lin=1, it=1, trials=(1, 0), polls=3, ntr=1)
    assert a["tr_temp"] == [50.0] and a["tr_cur"] == [100.0] and a["tr_lambda"] == [1.0] and math.isclose(a["tr_rho"][0], 50. / 60.)
    # ... alpha inside (1/3, 2/3): rho = 0.9 -> 1 - 0.8^3 = 0.488;  rho = 1 -> alpha = 0 -> 1/3
    a, _ = T.decide(s, 10.0, 100.0 - 1e-3, True, False)
    assert math.isclose(a["lam"], 0.488, rel_tol=1e-12)
    a, _ = T.decide(s, 0.0, 100.0 - 1e-3, True, False)
    assert a["lam"] == 1. / 3.
    # accepted at the last iteration of the first optimisation: the loop condition fails at i < iterations, Optimizer.cc:663 reads the flag
    s = state(it=4, trials=(4, 0), nBad=1)
    a, restored = T.decide(s, 50.0, 60.0, True, False)
    assert not restored and changed(s, a) == dict(lam=2. / 3., currentChi=50.0, final_chi2=50.0, final_lambda=2. / 3., phase=1, run=0, xmark=1, it=5,
                                                  qmax=1, nBad=0, iters_done=(5, 0), trials=(5, 0), polls=3, n_active=0, ntr=1)
    # accepted at the last iteration of the second optimisation
    s = state(phase=2, it=9, iters_done=(5, 0), trials=(5, 9))
    a, _ = T.decide(s, 50.0, 60.0, True, False)
    assert changed(s, a) == dict(lam=2. / 3., currentChi=50.0, final_chi2=50.0, final_lambda=2. / 3., phase=3, run=0, it=10, qmax=1,
                                 iters_done=(5, 10), trials=(5, 10), ntr=1)
    # rejected and repeated: lambda x ni, ni x 2, the errors are the trial's, terminate() evaluated once
    s = state(ni=4.0, qmax=1, it=2)
    a, restored = T.decide(s, 150.0, 60.0, True, False)
    assert restored and changed(s, a) == dict(lam=4.0, ni=8.0, qmax=2, trials=(1, 0), polls=3, err_at=2, ntr=1)
    # the tenth rejection: no repeat poll (qmax < 10 fails first), Terminate; terminate() of the loop condition is evaluated before `ok`
    s = state(ni=1024.0, qmax=9, it=2)
    a, restored = T.decide(s, 150.0, 60.0, True, False)
    assert restored and changed(s, a) == dict(lam=1024.0, ni=2048.0, final_chi2=100.0, final_lambda=1024.0, phase=1, run=0, xmark=1, it=3, qmax=10,
                                              iters_done=(3, 0), trials=(1, 0), polls=4, n_active=0, err_at=2, ntr=1)
    # nBad reaches 3: an improvement below 0.1 % for the third time (rho = 0.05 / 60: alpha = 1 - (-1)^3 -> 2/3)
    s = state(nBad=2, it=2)
    a, _ = T.decide(s, 99.95, 60.0, True, False)
    assert changed(s, a) == dict(lam=2. / 3., currentChi=99.95, final_chi2=99.95, final_lambda=2. / 3., phase=1, run=0, xmark=1, it=3, qmax=1, nBad=3,
                                 iters_done=(3, 0), trials=(1, 0), polls=4, n_active=0, ntr=1)
    a, _ = T.decide(state(nBad=1, it=2), 99.95, 60.0, True, False)
    assert a["nBad"] == 2 and a["run"] == 1 and a["lin"] == 1
    # the stop flag at the repeat poll after a rejected step (the test hook and the flag itself): the loop ends, the stop criterion counts
    # the step as bad, the loop condition and Optimizer.cc:663 see the latched flag
    for kw in (dict(stop_at_poll=3), dict(flag_seen=True)):
        s = state(it=1)
        a, restored = T.decide(s, 150.0, 60.0, True, kw.get("flag_seen", False), stop_at_poll=kw.get("stop_at_poll", 0))
        assert restored and changed(s, a) == dict(lam=2.0, ni=4.0, final_chi2=100.0, final_lambda=2.0, phase=3, run=0, it=2, qmax=1, nBad=1,
                                                  iters_done=(2, 0), trials=(1, 0), polls=5, stop_poll=3, err_at=2, ntr=1)
    # the stop flag at the iteration poll after an accepted step
    s = state(it=1)
    a, restored = T.decide(s, 50.0, 60.0, True, False, stop_at_poll=3)
    assert not restored and changed(s, a) == dict(lam=2. / 3., currentChi=50.0, final_chi2=50.0, final_lambda=2. / 3., phase=3, run=0, it=2, qmax=1,
                                                  iters_done=(2, 0), trials=(1, 0), polls=4, stop_poll=3, ntr=1)
    # the linear solve failed: tempChi = DBL_MAX, rejected and repeated
    s = state()
    a, restored = T.decide(s, 50.0, 60.0, False, False)
    assert restored and changed(s, a) == dict(lam=2.0, ni=4.0, qmax=1, trials=(1, 0), polls=3, solver_failed=1, err_at=2, ntr=1)
    assert a["tr_temp"] == [T.DBL_MAX] and a["tr_rho"] == [-1.0]
    # rho == 0: neither accepted nor repeated, Terminate
    s = state(phase=2, it=3, iters_done=(5, 0))
    a, restored = T.decide(s, 100.0, 60.0, True, False)
    assert restored and changed(s, a) == dict(lam=2.0, ni=4.0, final_chi2=100.0, final_lambda=2.0, phase=3, run=0, it=4, qmax=1, iters_done=(5, 4),
                                              trials=(0, 1), polls=3, err_at=2, ntr=1)


def lanes_one_by_one(values, tail):
    """canonical_sums as a loop over the values (the order stated in lba.hip, not vectorised)"""
    lanes = [0.0] * 128
    for i, v in enumerate(values):
        lanes[i % 128] += float(v)
    for t, v in enumerate(tail):
        lanes[t % 128] += float(v)
    h = 64
    while h:
        for k in range(h):
            lanes[k] += lanes[k + h]
        h //= 2
    return lanes[0]


@pytest.mark.parametrize("n", [1, 127, 128, 129, 2048, 2049])
def test_canonical_sum(n):
    rng = np.random.default_rng(n)
    v = rng.normal(size=n) * 10.0 ** rng.uniform(-6, 6, n)
    tail = rng.normal(size=6 * 41) * 10.0 ** rng.uniform(-6, 6, 6 * 41)
    for tl in ((), tail):
        got = T.canonical_sum(v, tl)
        assert got == lanes_one_by_one(v, tl)
        allv = np.r_[v, np.asarray(tl, np.float64)]
        depth = (n + 127) // 128 + (len(tl) + 127) // 128 + 7   # additions on the longest path
        assert abs(got - math.fsum(allv)) <= depth * 2.0 ** -53 * math.fsum(np.abs(allv)) * (1 + 1e-12)
    # the order is the stated one: a value that is lost unless it meets its lane's partner first
    if n > 128:
        w = np.zeros(n)
        w[0], w[128], w[1] = 1e16, -1e16, 1.0
        assert T.canonical_sum(w) == 1.0
