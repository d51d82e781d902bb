"""One k_eg_trial alone (aos2_debug_essential_graph_trial_device) on the inputs of tests/essential_graph_cases.py: the solver's vector x
is given (R.dense_solve on the device's own H and b at lambda = 1e-16 and 1e-3), the control words are seeded, and what the kernel
leaves is compared piece by piece.

est_try against mul(exp1(u), est) of the restatement.  The sim3_opt tests have no bound for oplus alone, so it is derived here: both
sides evaluate the lines of Sim3(Vector7d) and operator* in float64 and differ where libm does (sin, cos, exp, sqrt within an ulp) and
by the rounding of about twenty operations each.  The entries of exp(u)'s rotation carry at most 6 DBL_EPSILON (1 - cos theta and
theta - sin theta cancel, but what they multiply is theta^2 and theta^3 times smaller), its quaternion 8; the product of two
quaternions of norm 1 adds 4 roundings and passes the 8 on twice; t = s_E (q_E * t) + t_E is a dozen operations on numbers up to
M = max(1, |t_E|, s_E |t|).  Allowed, both sides together: 64 DBL_EPSILON M per component of q and t, 4 DBL_EPSILON relative on s.
tempChi against the long double sum of the restatement's residuals at the DEVICE's est_try: (ne + 8) 2^-53 chi for the sum and
2 sum |e| 128 DBL_EPSILON M for the residuals (the bound of test_header_residual_agrees_with_the_restatement on each).
scale against long double: 2 (7 nf) 2^-53 sum |x (lambda x + b)|.
The control words are scalar IEEE operations on tempChi and scale: a Python restatement of SoLm::decide_scaled / eg_trial_decide on
the device's own two sums must give the same words bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_graph_cases as K  # noqa: E402
import essential_graph_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DBL_EPSILON = 2.0 ** -52
LAMBDAS = (1e-16, 1e-3)
COMPARED = ("lambda", "ni", "currentChi", "rho", "qmax", "trials", "rejected", "accepted_first", "open", "running", "iterations", "nBad")


def decide(c, tempChi, scale):
    """SoLm::decide_scaled, eg_trial_decide and SoLm::end as the lines read, in float64 scalars -> (the words afterwards, accepted)"""
    f = np.float64
    c = dict(c)
    with np.errstate(all="ignore"):
        tempChi = f(tempChi) if c["solved"] else f(R.DBL_MAX)
        rho = (f(c["currentChi"]) - tempChi) / (f(scale) + f(1e-3))
        accepted = bool(rho > 0 and abs(tempChi) <= R.DBL_MAX)
        if accepted:
            t = f(2) * rho - f(1)
            alpha = f(1) - t * t * t
            alpha = alpha if alpha < f(2) / f(3) else f(2) / f(3)
            factor = f(1) / f(3) if f(1) / f(3) > alpha else alpha
            c["lambda"], c["ni"], c["currentChi"] = f(c["lambda"]) * factor, f(2), tempChi
        else:
            c["lambda"], c["ni"] = f(c["lambda"]) * f(c["ni"]), f(c["ni"]) * f(2)
        c["rho"] = rho
        c["qmax"] += 1
        c["trials"] += 1
        if not accepted:
            c["rejected"] += 1
        elif c["iterations"] == 0:
            c["accepted_first"] += 1
        if not (rho < 0 and c["qmax"] < 10):
            c["open"] = 0
            c["iterations"] += 1
            ok = not (c["qmax"] == 10 or rho == 0)
            if ok:
                c["nBad"] = c["nBad"] + 1 if (f(c["iniChi"]) - f(c["currentChi"])) * f(1e3) < f(c["iniChi"]) else 0
                ok = c["nBad"] < 3
            if not ok or c["iterations"] >= c["max_iterations"]:
                c["running"] = 0
    return c, accepted


@pytest.fixture(scope="module")
def handle(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


def check_trial(handle, name, P, lin, x, lam, what, **seed):
    """one trial with the seeds of `what` -> (accepted, the words afterwards, the worst difference / bound of each comparison)"""
    est = np.asarray(P["Scw"], np.float64)
    nv, ne, fixed, fix = len(est), len(P["v0"]), P["fixed"], bool(P["fix_scale"])
    free = np.flatnonzero(np.arange(nv) != fixed)
    seed = dict(dict(current_chi=lin["chi2"], ni=2.0, solved=1, iterations=0, qmax=0), **seed)
    got = handle.debug_essential_graph_trial(P, x, lam, **seed)
    ctl, try_, after = got["control"], got["est_try"], got["est"]

    # est_try
    want = est.copy()
    M = np.ones(nv)
    for h, v in enumerate(free):
        u = np.array(x[7 * h:7 * h + 7])
        if fix:
            u[6] = 0
        Eu = R.exp1(u)
        want[v] = R.mul(Eu[None], est[v:v + 1])[0]
        M[v] = max(1.0, np.abs(Eu[4:7]).max(), Eu[7] * np.abs(est[v, 4:7]).max())
    r_qt = (np.abs(try_ - want)[:, :7].max(axis=1) / (64 * DBL_EPSILON * M)).max()
    r_s = (np.abs(try_[:, 7] - want[:, 7]) / (4 * DBL_EPSILON * np.abs(want[:, 7]))).max()
    assert try_[fixed].tobytes() == est[fixed].tobytes()
    if fix:
        assert try_[:, 7].tobytes() == est[:, 7].tobytes()

    # tempChi at the device's own est_try, scale
    e = R.residuals(P["Sji"], try_, P["v0"], P["v1"]).astype(np.longdouble)
    chi = float((e * e).sum())
    Mr = K.residual_bound(P, try_)
    b_chi = (ne + 8) * 2.0 ** -53 * chi + 2 * float(np.abs(e).sum()) * Mr
    r_chi = abs(got["tempChi"] - chi) / b_chi
    xl, bl = np.asarray(x, np.longdouble), lin["b"].astype(np.longdouble)
    terms = xl * (np.longdouble(lam) * xl + bl)
    b_scale = 2 * (7 * len(free)) * 2.0 ** -53 * float(np.abs(terms).sum())
    r_scale = abs(got["scale"] - float(terms.sum())) / b_scale if b_scale else float(got["scale"] != 0)

    # the control words: the restatement on the device's own sums
    start = {"lambda": lam, "ni": seed["ni"], "currentChi": seed["current_chi"], "iniChi": lin["chi2"], "nBad": 0, "solved": seed["solved"],
             "iterations": seed["iterations"], "qmax": seed["qmax"], "trials": 0, "rejected": 0, "accepted_first": 0, "open": 1, "running": 1,
             "max_iterations": int(P.get("iterations", 20))}
    words, accepted = decide(start, got["tempChi"], got["scale"])
    for k in COMPARED:
        assert np.float64(ctl[k]).tobytes() == np.float64(words[k]).tobytes(), (name, what, k, ctl[k], words[k])
    assert ctl["solved"] == seed["solved"] and ctl["max_iterations"] == start["max_iterations"] and ctl["iniChi"] == lin["chi2"]
    assert ctl["chi2_initial"] == lin["chi2_initial"]
    assert after.tobytes() == (try_ if accepted else est).tobytes()
    print(name, what, "lambda %.0e" % lam, "accepted" if accepted else "rejected", "rho %.3g" % ctl["rho"],
          "difference / bound: q, t %.3g, s %.3g, tempChi %.3g, scale %.3g" % (r_qt, r_s, r_chi, r_scale))
    assert r_qt <= 1 and r_s <= 1 and r_chi <= 1 and r_scale <= 1
    return accepted, ctl, (r_qt, r_s, r_chi, r_scale)


def trials_of(handle, name):
    """the seven trials of a case: the solved step and 1e3 times it at both lambdas, then at lambda = 1e-3 a failed solve, a tenth
    trial and a trial of the last iteration -> what -> (accepted, the words afterwards); every comparison of check_trial on each"""
    P = K.cases()[name]
    nf = len(P["Scw"]) - 1
    lin = handle.debug_essential_graph_linearised(P)
    worst, out = np.zeros(4), {}

    def run(x, lam, what, **seed):
        nonlocal worst
        accepted, ctl, r = check_trial(handle, name, P, lin, x, lam, what, **seed)
        worst = np.maximum(worst, r)
        out[(what, lam)] = (accepted, ctl)
        return accepted, ctl

    for lam in LAMBDAS:
        x = R.dense_solve(lin["H"], lin["b"], lam, np.arange(7 * nf), np.arange(7 * nf))
        assert x is not None
        run(x, lam, "the step")
        run(1e3 * x, lam, "1e3 x the step")
    lam, last = LAMBDAS[1], int(P.get("iterations", 20)) - 1
    accepted, ctl = run(x, lam, "solved = 0", solved=0)
    assert not accepted and ctl["rho"] < 0 and ctl["open"] == 1 and ctl["lambda"] == lam * 2 and ctl["ni"] == 4
    accepted, ctl = run(1e3 * x, lam, "the tenth trial", qmax=9, ni=512.0)
    assert (ctl["qmax"], ctl["open"], ctl["iterations"], ctl["running"]) == (10, 0, 1, 0)
    accepted, ctl = run(x, lam, "the last iteration", iterations=last)
    assert ctl["accepted_first"] == 0 and (ctl["open"], ctl["iterations"], ctl["running"]) in ((0, last + 1, 0), (1, last, 1))
    K.record("trial " + name, "est_try q, t %.3g s %.3g tempChi %.3g scale %.3g; the control words equal their restatement" % tuple(worst))
    return out


@pytest.mark.parametrize("name", list(K.cases())[1:])
def test_one_trial_piece_by_piece(handle, name):
    trials_of(handle, name)


def test_every_outcome_of_a_trial_is_reached(handle):
    """on the first case, beside the comparisons: the step is accepted and closes the iteration, 1e3 times it is rejected with rho < 0
    and leaves it open, the tenth trial ends the call rejected, an accepted trial of the last iteration ends the call"""
    out = trials_of(handle, list(K.cases())[0])
    for lam in LAMBDAS:
        accepted, ctl = out[("the step", lam)]
        assert accepted and (ctl["accepted_first"], ctl["open"], ctl["iterations"], ctl["running"], ctl["rejected"]) == (1, 0, 1, 1, 0)
        accepted, ctl = out[("1e3 x the step", lam)]
        assert not accepted and ctl["rho"] < 0 and (ctl["open"], ctl["rejected"], ctl["iterations"], ctl["running"]) == (1, 1, 0, 1)
    accepted, ctl = out[("the tenth trial", LAMBDAS[1])]
    assert not accepted and ctl["rejected"] == 1
    accepted, ctl = out[("the last iteration", LAMBDAS[1])]
    assert accepted and (ctl["open"], ctl["running"]) == (0, 0)
