"""linearise, trial and reject of OptimizeSim3's edge backends alone, without a GPU: every comparison of
tests/test_sim3_opt_steps_gpu.py run on the host form of the tap (aos2_debug_sim3_opt_steps_host: SoHostEdges of csrc/sim3_opt.hip, the
header the device runs, sums in edge order) and on the float64 restatement R.Graph, which shows that a correct implementation meets
each bound; and on three wrong replays, which shows that each comparison can fail.  The cases, references, bounds (derived in its
docstring) and comparisons are tests/sim3_opt_step_cases.py.  The bound of the perturbed transforms is measured here, from the
restatement alone: 4 x the largest difference of R.oplus / R.sim3_inverse between float64 and long double over the 14 updates of the
case (floor 8 DBL_EPSILON max(1, |S_lin|)); it is written, with every ratio, to profiles/sim3_opt_taps.txt."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_opt_ref as R  # noqa: E402
import sim3_opt_step_cases as K  # noqa: E402

NAMES = list(K.cases())
LARGE = [k for k in NAMES if K.cases()[k]["n"] >= 9]


def test_cases_meet_their_conditions():
    cs = K.cases()
    assert tuple(sorted({c["n"] for c in cs.values()})) == K.NS and len(cs) == 2 * len(K.NS)
    assert {(c["n"], c["fix"]) for c in cs.values()} == {(n, f) for n in K.NS for f in (False, True)}
    assert {c["far"] for c in cs.values()} == {False, True}
    dropped, drawn = K.draw_counts()
    print("dropped", dropped, "of", drawn, "margins", ["%.1e" % c["margin"] for c in cs.values()])
    # no branch of Huber's kernel hangs on rounding: every chi2 at S_lin and S_trial keeps a relative R.MARGIN from delta_H^2
    assert min(c["margin"] for c in cs.values()) >= R.MARGIN
    assert 2 * dropped <= drawn
    # both branches of Huber's kernel: in the cases together, and side by side in most of them
    assert sum(0 < c["n_above"] < 2 * c["n"] for c in cs.values()) >= len(cs) // 2
    for c in cs.values():
        n, m = c["n"], c["masks"]
        for a in m.values():
            assert a.shape == (2 * n,) and (a[0::2] == a[1::2]).all()   # pair-consistent
        assert m["all"].all() and not m["none"].any()
        col = 2 * ((n - 1) % (K.THREADS // 2))
        owner = np.arange(2 * n) % K.THREADS
        assert not m["column"][(owner == col) | (owner == col + 1)].any() and m["column"][(owner != col) & (owner != col + 1)].all()
        if n > 1:
            assert m["half"].any() and not m["half"].all() and not np.array_equal(c["S_lin"][1], c["S_trial"][1])
        if c["fix"]:
            assert c["S_trial"][2] == c["S_lin"][2]
    assert sum(2 * n for n in K.SINGLES) == 86


@pytest.mark.parametrize("name", NAMES)
def test_host_tap_and_restatement_meet_every_bound(pkg, name):
    c = K.cases()[name]
    n, ref = c["n"], K.reference(c)
    items = K.step_items(c)
    outs = pkg.capi.debug_sim3_opt_steps_host([it for _, it in items], sentinel=K.SENTINEL)
    worst = {"host": {}, "restatement": {}}

    def keep(who, what, r):
        worst[who][what] = max(worst[who].get(what, 0.0), r)

    for (tag, it), out in zip(items, outs):
        act, same = it["act_in"], tag.endswith("_same")
        for who, o in (("host", out), ("restatement", K.graph_outputs(c, act, same))):
            keep(who, "pert", K.ratio_pert(c, o["pert"]))
            keep(who, "sum", K.ratio_sum(c, act, o["Hb"]))
            keep(who, "chi_lin", K.ratio_chi(c, act, it["chi_in"], o["chi_lin"][:2 * n], "lin"))
            if not same:
                keep(who, "chi_trial", K.ratio_chi(c, act, it["chi_in"], o["chi_trial"][:2 * n], "trial"))
                keep(who, "trial_sum", K.ratio_trial_sum(c, act, o["trial_sum"]))
            else:   # the same values through the same sum
                assert K.bits(o["chi_trial"]) == K.bits(o["chi_lin"]) and K.bits(o["trial_sum"]) == K.bits(o["Hb"][35]), (who, tag)
            assert K.fix_scale_exact(c, o), (who, tag)
            if not act.any():
                assert K.bits(o["Hb"]) == K.bits(np.zeros(36)) and K.bits(o["trial_sum"]) == K.bits(0.0), (who, tag)
                assert K.bits(o["chi_lin"]) == K.bits(it["chi_in"]) == K.bits(o["chi_trial"]), (who, tag)
        # what linearise and trial leave alone
        assert K.untouched(out, ("flagged",)) and K.tails_kept(out, n), tag
        assert np.array_equal(out["act"][:2 * n], act) and not out["outlier"][:n].any() and K.bits(out["chi"][:2 * n]) == K.bits(out["chi_trial"]), tag
    if n in K.SINGLES:   # Hb of a single-edge mask is that edge's terms
        single = [o for b in K.batches(K.single_items(c)) for o in pkg.capi.debug_sim3_opt_steps_host(b)]
        full, restated = outs[0], K.graph_outputs(c, c["masks"]["all"], False)
        total = np.zeros(36)
        for e, o in enumerate(single):
            keep("host", "terms", K.ratio_single(c, e, o["Hb"]))
            keep("restatement", "terms", K.ratio_single(c, e, restated["terms"][e]))
            assert K.ratio_chi(c, K.single_items(c)[e]["act_in"], K.chi_planted(c), o["chi_lin"], "lin") <= 1
            total = total + o["Hb"]
        assert K.bits(total) == K.bits(full["Hb"])   # the host form adds in edge order, from 0
    print(name, "M %.1f b_J %.3g b_E %.3g" % (ref["M"], ref["b_J"], ref["b_E"]), worst)
    fmt = lambda w: " ".join("%s %.3g" % kv for kv in sorted(w.items()))   # noqa: E731
    K.record("reference " + name, "n %d fix_scale %d above delta_H^2 %d of %d: pert measured %.3g floor %.3g; restatement / bound: %s" %
             (n, c["fix"], c["n_above"], 2 * n, ref["pert_measured"], ref["pert_floor"], fmt(worst["restatement"])))
    K.record("host " + name, fmt(worst["host"]) + "; S_trial = S_lin: chi and the trial sum equal linearise's bit for bit")
    assert ref["pert_measured"] < 1e-14   # (a reference that determined the transforms no better would make the bound empty)
    for who in worst:
        assert all(r <= 1 for r in worst[who].values()), (who, worst[who])


@pytest.mark.parametrize("name", LARGE)
def test_each_comparison_fails_on_the_mutant_it_targets(name):
    """the test's own replay (K.replay_terms: the terms from the 28 transforms; K.block_sum: the device's order of additions) is the
    restatement when nothing is wrong, and breaches the comparison that should see it when something is"""
    c = K.cases()[name]
    n, fix, act = c["n"], c["fix"], c["masks"]["all"]
    G, S = R.Graph(c["P"], np.float64), K.sim3(c["S_lin"], np.float64)
    good = K.replay_terms(G, S, fix)
    assert K.bits(good) == K.bits(G.edge_terms(S, fix))
    per_edge = lambda t: np.array([K.ratio_single(c, e, t[e]) for e in range(2 * n)])   # noqa: E731
    assert per_edge(good).max() <= 1
    forward = per_edge(K.replay_terms(G, S, fix, "forward"))
    assert (forward[1::2] > 1).all() and (forward[0::2] <= 1).all()   # every e21 edge, no e12 edge
    columns = per_edge(K.replay_terms(G, S, fix, "columns"))
    assert (columns > 1).all()
    whole, short = K.block_sum(good, act), K.block_sum(good, act, skip_row=1)
    r_whole, r_short = K.ratio_sum(c, act, whole), K.ratio_sum(c, act, short)
    print(name, "forward %.3g columns %.3g without row 1 %.3g (the whole sum %.3g)" % (forward[1::2].min(), columns.min(), r_short, r_whole))
    assert r_whole <= 1 < r_short and K.bits(whole) != K.bits(short)
    # a term in the mutants' sums shows in the sum comparison as well
    assert K.ratio_sum(c, act, K.block_sum(K.replay_terms(G, S, fix, "forward"), act)) > 1
    assert K.ratio_sum(c, act, K.block_sum(K.replay_terms(G, S, fix, "columns"), act)) > 1


@pytest.mark.parametrize("remove", [0, 1])
def test_reject_on_planted_chi(pkg, remove):
    made = [K.reject_item(c, remove) for c in K.cases().values()]
    kinds = set()
    for c, (item, want) in zip(K.cases().values(), made):
        kinds |= want["kinds"]
        n, bad = c["n"], want["bad"]
        assert bad[n - 1] and all(bad[e0 // 2] for e0, _ in K.PAIRS if e0 // 2 < n)
        if n >= 9:   # one of every kind, and a flag that was planted and stays
            assert bad[:8].tolist() == [False, True, True, True, False, False, False, False] and item["outlier_in"][7] == 1
            assert np.isnan(item["chi_in"][10:12]).any() and item["chi_in"][12] == 1e300 and not item["act_in"][12]
            assert (item["chi_in"][8:10] == np.float32(R.TH2)).all()
    assert kinds == set(range(8))
    outs = pkg.capi.debug_sim3_opt_steps_host([item for item, _ in made], sentinel=K.SENTINEL)
    for c, (item, want), out in zip(K.cases().values(), made, outs):
        assert K.reject_failures(c, item, want, out) == [], c["name"]


def test_bad_arguments_are_refused_and_leave_every_sentinel(pkg):
    cs = list(K.cases().values())
    good = [it for _, it in K.step_items(cs[2])[:2]]
    L = pkg.capi.lib()
    assert L.aos2_debug_sim3_opt_steps_host(None, 0) == 0 and L.aos2_debug_sim3_opt_steps_host(None, 1) == pkg.capi.AOS2_ERR_ARG
    I, keep, outs = pkg.capi._sim3_opt_steps_args(good * 33)
    assert L.aos2_debug_sim3_opt_steps_host(I, 66) == pkg.capi.AOS2_ERR_ARG

    def refused(change):
        I, keep, outs = pkg.capi._sim3_opt_steps_args(good, sentinel=K.SENTINEL)
        change(I[1])
        assert L.aos2_debug_sim3_opt_steps_host(I, 2) == pkg.capi.AOS2_ERR_ARG
        assert all(K.untouched(o, o.keys()) for o in outs)

    for field in ("act_in", "chi_in", "outlier_in", "Hb", "pert", "chi_lin", "trial_sum", "chi_trial", "flagged", "chi", "act", "outlier"):
        refused(lambda it, f=field: setattr(it, f, None))
    for th2 in (0.0, -1.0, float("nan")):
        refused(lambda it, v=th2: setattr(it.problem, "th2", v))
    refused(lambda it: setattr(it.problem, "n", 0))
    refused(lambda it: setattr(it.problem, "obs2", None))
    refused(lambda it: setattr(it, "mask", 8))
    refused(lambda it: setattr(it, "tail", -1))
    I, keep, outs = pkg.capi._sim3_opt_steps_args(good, sentinel=K.SENTINEL)   # a mask of nothing: the planted state comes back
    I[0].mask = 0
    assert L.aos2_debug_sim3_opt_steps_host(I, 2) == 0
    assert K.untouched(outs[0], ("Hb", "pert", "chi_lin", "trial_sum", "chi_trial", "flagged")) and K.bits(outs[0]["chi"][:4]) == K.bits(good[0]["chi_in"][:4])
    assert not K.untouched(outs[1], ("Hb",))
