"""SoDevEdges::linearise, trial and reject of csrc/sim3_opt.hip alone (aos2_debug_sim3_opt_steps_device: a kernel of sim3_opt_kernel's
launch shape and LDS objects that calls the three members on act / chi / outlier the test plants), which the end-to-end rule of
tests/test_sim3_opt_gpu.py cannot see into: Levenberg-Marquardt corrects a wrong term of the normal equations by itself.

The cases, references, bounds (derived in its docstring) and comparisons are tests/sim3_opt_step_cases.py; tests/test_sim3_opt_steps_cpu.py
shows on the host form and the float64 restatement that a correct implementation meets each bound, and on wrong replays that each
comparison can fail.  Here, per case:
  the 28 transforms that threads 0..13 left in LDS against R.oplus / R.sim3_inverse in long double (bound measured from the restatement);
  with a single-edge mask Hb is that edge's own 36 terms (the running sums start from 0, every other operand of the tree is 0):
  against the terms formed in long double from the residual and the closed-form Jacobian;
  for n in {1, 9, 33} Hb and the trial sum of every mask equal the DEVICE's own per-edge terms added as SoDevEdges::block_sum adds
  them -- per thread over e = tid, tid + 256, ..., the tree of row_sum_f64 over each row of 16, the 16 partials in row order --
  byte for byte; for every n against the long double sum of the reference's terms within the order-free bound;
  chi after linearise and after trial against the long double chi2, inactive edges keeping what was planted byte for byte;
  S_trial = S_lin: chi and the trial sum are linearise's chi and Hb[35] byte for byte;
  reject alone on planted chi: the count, the flags, act and what it must not touch.
One line per case goes to profiles/sim3_opt_taps.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_opt_step_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = list(K.cases())


@pytest.fixture(scope="module")
def handle(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


@pytest.fixture(scope="module")
def runs(handle):
    """every item of every case in six calls: name -> (step outputs in the order of K.step_items, single-edge outputs or None)"""
    cs = K.cases()
    steps = [(name, it) for name, c in cs.items() for _, it in K.step_items(c)]
    singles = [(name, it) for name, c in cs.items() if c["n"] in K.SINGLES for it in K.single_items(c)]
    out = {name: ([], []) for name in cs}
    for k, group in enumerate((steps, singles)):
        for batch in K.batches(group):
            for (name, _), o in zip(batch, handle.debug_sim3_opt_steps([it for _, it in batch], sentinel=K.SENTINEL)):
                out[name][k].append(o)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_linearise_and_trial_against_long_double_and_the_sum_against_its_own_terms(runs, name):
    c = K.cases()[name]
    n, ref = c["n"], K.reference(c)
    outs, single = runs[name]
    items = K.step_items(c)
    assert len(outs) == len(items) and len(single) == (2 * n if n in K.SINGLES else 0)
    worst = {}

    def keep(what, r):
        worst[what] = max(worst.get(what, 0.0), r)

    for (tag, it), o in zip(items, outs):
        act, same = it["act_in"], tag.endswith("_same")
        keep("pert", K.ratio_pert(c, o["pert"]))
        keep("sum", K.ratio_sum(c, act, o["Hb"]))
        keep("chi_lin", K.ratio_chi(c, act, it["chi_in"], o["chi_lin"], "lin"))
        if not same:
            keep("chi_trial", K.ratio_chi(c, act, it["chi_in"], o["chi_trial"], "trial"))
            keep("trial_sum", K.ratio_trial_sum(c, act, o["trial_sum"]))
        else:   # the same values through the same tree
            assert K.bits(o["chi_trial"]) == K.bits(o["chi_lin"]) and K.bits(o["trial_sum"]) == K.bits(o["Hb"][35]), tag
        assert K.fix_scale_exact(c, o), tag
        assert K.bits(o["pert"]) == K.bits(outs[0]["pert"]), tag   # the transforms do not depend on the mask
        if not act.any():
            assert K.bits(o["Hb"]) == K.bits(np.zeros(36)) and K.bits(o["trial_sum"]) == K.bits(0.0), tag
            assert K.bits(o["chi_lin"]) == K.bits(it["chi_in"]) == K.bits(o["chi_trial"]), tag
        # what linearise and trial leave alone
        assert K.untouched(o, ("flagged",)) and K.tails_kept(o, n), tag
        assert np.array_equal(o["act"][:2 * n], act) and not o["outlier"][:n].any() and K.bits(o["chi"][:2 * n]) == K.bits(o["chi_trial"]), tag
    text = ""
    if single:
        eye = np.eye(2 * n, dtype=np.uint8)
        terms = np.stack([o["Hb"] for o in single])
        trial_terms = np.stack([o["trial_sum"] for o in single])
        for e, o in enumerate(single):
            keep("terms", K.ratio_single(c, e, o["Hb"]))
            keep("chi_lin", K.ratio_chi(c, eye[e], K.chi_planted(c), o["chi_lin"], "lin"))
            keep("chi_trial", K.ratio_chi(c, eye[e], K.chi_planted(c), o["chi_trial"], "trial"))
            keep("trial_sum", K.ratio_trial_sum(c, eye[e], o["trial_sum"]))
            assert K.fix_scale_exact(c, o) and K.tails_kept(o, n) and K.bits(o["pert"]) == K.bits(outs[0]["pert"]), e
        for (tag, it), o in zip(items, outs):
            assert K.bits(o["Hb"]) == K.bits(K.block_sum(terms, it["act_in"])), tag
            if not tag.endswith("_same"):
                assert K.bits(o["trial_sum"]) == K.bits(K.block_sum(trial_terms, it["act_in"])), tag
        text = "; Hb and the trial sum equal the tree of the device's own per-edge terms bit for bit"
    print(name, worst)
    K.record("device " + name, " ".join("%s %.3g" % kv for kv in sorted(worst.items())) + text +
             "; S_trial = S_lin: chi and the trial sum equal linearise's bit for bit")
    assert all(r <= 1 for r in worst.values()), worst


@pytest.mark.parametrize("remove", [0, 1])
def test_reject_on_planted_chi(handle, remove):
    made = [K.reject_item(c, remove) for c in K.cases().values()]
    outs = handle.debug_sim3_opt_steps([item for item, _ in made], sentinel=K.SENTINEL)
    for c, (item, want), out in zip(K.cases().values(), made, outs):
        assert K.reject_failures(c, item, want, out) == [], c["name"]


def test_a_refused_call_leaves_every_sentinel_and_the_handle_works_afterwards(pkg, handle, runs):
    name = NAMES[2]
    good = [it for _, it in K.step_items(K.cases()[name])[:2]]
    for change in (lambda it: setattr(it, "chi_trial", None), lambda it: setattr(it.problem, "th2", 0.0), lambda it: setattr(it.problem, "th2", -2.0)):
        I, keep, outs = pkg.capi._sim3_opt_steps_args(good, sentinel=K.SENTINEL)
        change(I[1])
        assert handle.L.aos2_debug_sim3_opt_steps_device(handle.h, I, 2) == pkg.capi.AOS2_ERR_ARG
        assert all(K.untouched(o, o.keys()) for o in outs)
    assert handle.L.aos2_debug_sim3_opt_steps_device(None, I, 2) == pkg.capi.AOS2_ERR_ARG
    again = handle.debug_sim3_opt_steps(good, sentinel=K.SENTINEL)
    for a, b in zip(again, runs[name][0][:2]):   # alone or in a batch of 64, now or before: the same bytes
        assert all(K.bits(a[k], a[k].dtype) == K.bits(b[k], b[k].dtype) for k in a)
