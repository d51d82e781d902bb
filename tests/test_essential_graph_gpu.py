"""aos2_optimize_essential_graph on the GPU against tests/essential_graph_ref.py under the comparison rule (status exact, the fixed
vertex and -- with fix_scale -- every scale bit-identical, R(q), t, s, Tiw and Xw within max(1e-5, 4 x the problem's measured
resolution); iterations / trials not compared), against the host tap, and against itself byte for byte: alone or in a batch, from
call to call.  The workload is the generator's (tests/test_essential_graph_cpu.py asserts what it covers)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_graph_cases as K  # noqa: E402
import essential_graph_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 3
SENTINEL = 0x5A


def raw(res):
    """every byte of a result"""
    return b"".join([np.ascontiguousarray(res[k]).tobytes() for k in ("Scw", "Tiw", "Xw")] +
                    [np.array([res["chi2_initial"], res["chi2_final"]], np.float64).tobytes(),
                     np.array([res[k] for k in ("iterations", "trials", "rejected", "l_blocks", "status")], np.int32).tobytes()])


@pytest.fixture(scope="module")
def world(pkg, gpu):
    c = R.generator_case(SEED)
    L = pkg.capi.LocalBA(device=0)
    return c, L, L.optimize_essential_graph(c["problems"])


def test_device_equals_the_reference_at_every_size(world):
    c, L, batch = world
    assert tuple(len(P["Scw"]) for P in c["problems"]) == (1, 2, 3, 9, 17, 64, 65, 130, 300)
    for k, (g, w, P, r) in enumerate(zip(batch, c["want"], c["problems"], c["resolution"])):
        ok, msg = R.same(g, w, P, r)
        print("n", len(P["Scw"]), msg, "iterations", g["iterations"], w["iterations"], "trials", g["trials"], w["trials"], "rejected", g["rejected"],
              "chi2 %.3e -> %.3e" % (g["chi2_initial"], g["chi2_final"]), "l_blocks", g["l_blocks"])
        assert ok, (k, msg)
        assert g["chi2_final"] <= g["chi2_initial"]
    assert L.optimize_essential_graph([]) == []


def test_device_equals_the_host_tap(pkg, world):
    c, L, batch = world
    taps = pkg.capi.debug_essential_graph_host(c["problems"])
    for k, (g, t, P, r) in enumerate(zip(batch, taps, c["problems"], c["resolution"])):
        ok, msg = R.same(g, t, P, r)
        print("n", len(P["Scw"]), msg)
        assert ok, (k, msg)
        assert g["l_blocks"] == t["l_blocks"]


def test_a_batch_of_sixteen_equals_sixteen_single_calls(world):
    c, L, batch = world
    P = c["problems"]
    more = [dict(P[3], fix_scale=False), dict(P[4], fix_scale=True, Scw=np.concatenate([P[4]["Scw"][:, :7], np.ones((17, 1))], axis=1)), dict(P[5], iterations=3),
            dict(P[4], v0=P[4]["v0"][:0], v1=P[4]["v1"][:0], Sji=P[4]["Sji"][:0]), R.problem(9, 33, False), R.problem(9, 64, False, planted=True), P[2]]
    sixteen = [P[k] for k in (8, 0, 7, 1, 6, 2, 5, 3, 4)] + more
    assert len(sixteen) == 16
    together = L.optimize_essential_graph(sixteen)
    for k, Q in enumerate(sixteen):
        assert raw(L.optimize_essential_graph([Q])[0]) == raw(together[k]), k
    assert [raw(together[i]) for i, k in enumerate((8, 0, 7, 1, 6, 2, 5, 3, 4))] == [raw(batch[k]) for k in (8, 0, 7, 1, 6, 2, 5, 3, 4)]
    assert together[11]["iterations"] <= 3


def test_two_consecutive_calls_give_identical_bytes(world):
    c, L, batch = world
    again = L.optimize_essential_graph(c["problems"])
    assert [raw(a) for a in again] == [raw(b) for b in batch]


def test_degenerate_graphs_come_back_through_the_recovery_arithmetic(world):
    """no edges, and n_vertices == 1: no LM runs, Scw out = Scw in, poses and points still go through :992-1044"""
    c, L, batch = world
    P = c["problems"][4]
    none = dict(P, v0=P["v0"][:0], v1=P["v1"][:0], Sji=P["Sji"][:0])
    for Q, g in ((none, L.optimize_essential_graph([none])[0]), (c["problems"][0], batch[0])):
        w = R.optimize(Q)
        assert g["Scw"].tobytes() == np.asarray(Q["Scw"], np.float64).tobytes()
        assert (g["iterations"], g["trials"], g["rejected"], g["status"], g["l_blocks"], g["chi2_initial"], g["chi2_final"]) == (0, 0, 0, 0, 0, 0.0, 0.0)
        assert np.abs(g["Tiw"] - w["Tiw"]).max() <= 1e-6 and np.abs(g["Xw"] - w["Xw"]).max() <= 1e-5


def test_noise_free_measurements_give_the_planted_poses_back(world):
    c, L, batch = world
    P = R.problem(5, 130, False, planted=True)
    g = L.optimize_essential_graph([P])[0]
    S, T = g["Scw"], P["truth"]
    dR, dt, ds = np.abs(R.rot_of(S[:, :4]) - R.rot_of(T[:, :4])).max(), np.abs(S[:, 4:7] - T[:, 4:7]).max(), np.abs(S[:, 7] - T[:, 7]).max()
    print("dR %.2e dt %.2e ds %.2e" % (dR, dt, ds), "chi2 %.3e -> %.3e" % (g["chi2_initial"], g["chi2_final"]), "iterations", g["iterations"], "trials", g["trials"])
    assert g["status"] == R.EG_OK and g["chi2_final"] < g["chi2_initial"]
    assert dR <= 1e-6 and ds <= 1e-6 and dt <= 1e-5


def test_points_of_a_graph_at_its_optimum_come_back_within_one_ulp(world):
    """measurements formed from the estimates themselves (chi2 = 1e-30: the rounding of Sjw * Swi, so a trial may still move an
    estimate in its last bits), and the same graph without edges (the estimates stay bit for bit): correctedSwr.map(Srw.map(P)) is P
    but for the rounding of two double maps, 1e-15 relative and far below half a float32 ulp"""
    c, L, batch = world
    P = c["problems"][6]
    Q = dict(P, Sji=R.mul(P["Scw"][P["v1"]], R.inverse(P["Scw"])[P["v0"]]), Xw=np.random.default_rng(1).uniform(-30, 30, (100000, 3)).astype(np.float32),
             ref=np.random.default_rng(2).integers(0, len(P["Scw"]), 100000).astype(np.int32))
    g = L.optimize_essential_graph([Q])[0]
    print("chi2 %.3e -> %.3e" % (g["chi2_initial"], g["chi2_final"]), "largest change of an estimate %.2e" % np.abs(g["Scw"] - Q["Scw"]).max())
    assert g["chi2_initial"] < 1e-24 and np.abs(g["Scw"] - Q["Scw"]).max() <= 1e-12
    assert (np.abs(g["Xw"] - Q["Xw"]) <= np.spacing(np.abs(Q["Xw"]))).all()
    g = L.optimize_essential_graph([dict(Q, v0=Q["v0"][:0], v1=Q["v1"][:0], Sji=Q["Sji"][:0])])[0]
    assert g["Scw"].tobytes() == np.asarray(Q["Scw"], np.float64).tobytes()
    assert (np.abs(g["Xw"] - Q["Xw"]) <= np.spacing(np.abs(Q["Xw"]))).all()


def test_a_refused_call_leaves_the_sentinel_and_the_handle_works_afterwards(pkg, world):
    c, L, batch = world
    P = c["problems"]
    bad_v1 = np.array(P[4]["v1"])
    bad_v1[5] = 17
    for bad in (dict(P[4], iterations=0), dict(P[4], v1=bad_v1), dict(P[4], fixed=17)):
        with pytest.raises(pkg.AosError) as e:
            L.optimize_essential_graph([P[3], bad, P[5]], sentinel=SENTINEL)
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
        Rc, outs = L.essential_graph_last
        for k in range(3):
            assert all((a.view(np.uint8) == SENTINEL).all() for a in outs[k].values()) and Rc[k].status == 0x5A5A5A5A and Rc[k].iterations == 0x5A5A5A5A
    assert raw(L.optimize_essential_graph([P[4]])[0]) == raw(batch[4])   # the handle is as good as before


# ---------------------------------------------------------------------------------------------- inputs the generator does not produce
@pytest.fixture(scope="module")
def turned(world):
    """tests/essential_graph_cases.py: edges in both orientations between free vertices, a free pair named twice, the fixed vertex
    first, last and in the middle -> the cases, the restatement's results, the batch of the five"""
    c, L, batch = world
    t = K.optimised()
    return t, L.optimize_essential_graph(t["problems"])


def test_turned_inputs_equal_the_reference_and_the_host_tap(pkg, world, turned):
    t, together = turned
    taps = pkg.capi.debug_essential_graph_host(t["problems"])
    assert max(t["resolution"]) < 1e-4
    for k, (g, w, tap, P, r) in enumerate(zip(together, t["want"], taps, t["problems"], t["resolution"])):
        for other, name in ((w, "restatement"), (tap, "host tap")):
            ok, msg = R.same(g, other, P, r)
            print(t["names"][k], name, msg, "iterations", g["iterations"], other["iterations"], "trials", g["trials"], other["trials"])
            assert ok, (k, name, msg)
        assert g["l_blocks"] == tap["l_blocks"] and g["chi2_final"] < g["chi2_initial"]


def test_each_turned_case_alone_equals_the_same_case_in_a_batch(world, turned):
    c, L, batch = world
    t, together = turned
    for k, P in enumerate(t["problems"]):
        assert raw(L.optimize_essential_graph([P])[0]) == raw(together[k]), t["names"][k]


def test_a_measurement_that_is_not_a_number_stays_with_its_problem(world, turned):
    """a NaN in one Sji of the problem between two good ones: no step of its own (tests/test_essential_graph_cpu.py: 20 iterations of
    one rejected trial each, the estimates bit for bit the input's), the neighbours as they are alone, the handle as good as before"""
    c, L, batch = world
    t, together = turned
    bad = K.with_nan(t["problems"][2])
    got = L.optimize_essential_graph([t["problems"][0], bad, t["problems"][3]])
    g = got[1]
    assert (g["status"], g["iterations"], g["trials"], g["rejected"]) == (R.EG_NO_STEP, 20, 20, 20)
    assert g["Scw"].tobytes() == np.asarray(bad["Scw"], np.float64).tobytes()
    assert raw(got[0]) == raw(together[0]) and raw(got[2]) == raw(together[3])
    assert raw(L.optimize_essential_graph([t["problems"][2]])[0]) == raw(together[2])
