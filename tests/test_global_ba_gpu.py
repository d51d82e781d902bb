"""aos2_global_bundle_adjustment on the GPU: Optimizer::BundleAdjustment (src/Optimizer.cc:41-237) for one map, against
  * the oracle (oracle.lba_solve(prob, iters1=n, iters2=0)) on the form it can express -- robust, LocalBA's Huber deltas,
  * tests/global_ba_ref.py on what it cannot -- bRobust = false (LoopClosing's form) and thHuber2D = sqrt(5.99),
  * the library's host tap (the same header and per-item functions on the CPU),
under the project's rule (tests/global_ba_ref.py mismatches): iterations and trials exact, poses and points within
max(1e-5, 4 x resolution), chi2_final within the same factor of 1e-6.  The resolutions of the three small cases are measured here; the
three large ones are compared at the floor of the rule (resolution 0: never wider than the rule; tests/test_global_ba_cpu.py measures
theirs and writes them to profiles/global_ba_resolution.txt)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import global_ba_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = list(R.CASES)
SMALL = ("init", "pair", "mixed")
FLOOR = dict(pose=0.0, point=0.0)
_problems, _oracle = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = R.problem(name)
    return _problems[name]


def oracle_case(oracle, name):
    """the oracle's result and its own spread, once per session"""
    if name not in _oracle:
        import parity
        prob, n = problem(name), R.iterations_of(name)
        want = oracle.lba_solve(prob, iters1=n, iters2=0)
        res = parity.lba_resolution(prob, want=want, iters=(n, 0)) if name in SMALL else FLOOR
        _oracle[name] = (R.from_oracle(want), res)
    return _oracle[name]


@pytest.fixture(scope="module")
def ba(pkg, gpu):
    return pkg.capi.LocalBA(device=0)


@pytest.mark.parametrize("name", CASES)
def test_device_agrees_with_the_oracle_on_the_robust_form(ba, oracle, name):
    want, res = oracle_case(oracle, name)
    got = ba.GlobalBundleAdjustment(problem(name), R.iterations_of(name), True, R.HUBER_LOCAL_BA)
    assert got["status"] == 0 and not R.mismatches(got, want, res, name)
    assert got["polls"] == want["polls"] - 2 and got["stop_poll"] == 0   # no entry check, none after optimize()
    assert got["chi2_final"] < got["chi2_initial"] and got["ms_device"] > 0


@pytest.mark.parametrize("robust,huber", [(False, R.HUBER_GBA), (True, R.HUBER_GBA)])
@pytest.mark.parametrize("name", CASES)
def test_device_agrees_with_the_reference_where_the_oracle_has_no_form(ba, name, robust, huber):
    prob, n = problem(name), R.iterations_of(name)
    if name in SMALL:
        res, want = R.resolution_by_reference(prob, n, robust, huber)
        assert res["decisions_equal"]
    else:
        res, want = FLOOR, R.solve(prob, n, robust, huber)
    got = ba.GlobalBundleAdjustment(prob, n, robust, huber)
    assert not R.mismatches(got, want, res, "%s robust %d" % (name, robust))
    assert (got["polls"], got["h_blocks"]) == (want["polls"], want["h_blocks"])


@pytest.mark.parametrize("name", CASES)
def test_device_agrees_with_the_host_tap(pkg, ba, name):
    prob, n = problem(name), R.iterations_of(name)
    got = ba.GlobalBundleAdjustment(prob, n)
    host = pkg.capi.debug_global_ba_host(prob, n)
    assert not R.mismatches(got, host, FLOOR, name)
    for k in ("polls", "stop_poll", "h_blocks", "l_blocks"):
        assert got[k] == host[k], k
    assert got["point_included"].tobytes() == host["point_included"].tobytes()


def test_abort_at_every_poll(ba, oracle):
    """the device stopped at its poll k against the oracle stopped at its poll k + 1 (the oracle's LocalBA has the entry check in front):
    the same iterations, trials and estimates; stop_poll is reported"""
    name = "mixed"
    prob, n = problem(name), R.iterations_of(name)
    _, res = oracle_case(oracle, name)
    try:
        free = ba.GlobalBundleAdjustment(prob, n, True, R.HUBER_LOCAL_BA)
        assert free["stop_poll"] == 0 and free["polls"] >= n
        for k in range(1, free["polls"] + 1):
            ba.debug_stop_at_poll(k)
            got = ba.GlobalBundleAdjustment(prob, n, True, R.HUBER_LOCAL_BA)
            w = oracle.lba_solve(prob, iters1=n, iters2=0, stop_at_poll=k + 1)
            want = R.from_oracle(w)
            assert got["status"] == 0 and got["stop_poll"] == k and w["stop_poll"] == k + 1, k
            assert (got["iterations"], got["trials"]) == (want["iterations"], want["trials"]), k
            assert R.worst(got["pose_Tcw"], want["pose_Tcw"]) <= max(R.TOL, 4 * res["pose"]), k
            assert R.worst(got["point_xyz"], want["point_xyz"]) <= max(R.TOL, 4 * res["point"]), k
    finally:
        ba.debug_stop_at_poll(0)
    # a flag that is set when the call begins: the head of optimize()'s loop sees it, nothing runs, AOS2_OK
    flag = np.ones(1, np.uint8)
    got = ba.GlobalBundleAdjustment(prob, n, stop_flag=flag)
    assert (got["status"], got["stop_poll"], got["iterations"], got["trials"]) == (0, 1, 0, 0)
    assert got["point_xyz"].tobytes() == np.ascontiguousarray(prob["point_xyz"], np.float32).tobytes()


@pytest.mark.parametrize("name", ["mixed", "loop"])
def test_two_consecutive_calls_are_byte_identical(ba, name):
    prob, n = problem(name), R.iterations_of(name)
    a, b = ba.GlobalBundleAdjustment(prob, n), ba.GlobalBundleAdjustment(prob, n)
    for k in ("pose_Tcw", "point_xyz", "point_included"):
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in ("iterations", "trials", "chi2_initial", "chi2_final", "final_lambda", "polls", "h_blocks", "l_blocks"):
        assert a[k] == b[k], k


@pytest.mark.parametrize("name", CASES)
def test_points_without_an_edge_stay_untouched(ba, name):
    prob, n = problem(name), R.iterations_of(name)
    got = ba.GlobalBundleAdjustment(prob, n)
    deg = np.bincount(prob["edge_point"], minlength=prob["n_points"])
    assert got["point_included"].tolist() == (deg > 0).astype(int).tolist() and (deg == 0).any()
    src = np.ascontiguousarray(prob["point_xyz"], np.float32)
    assert got["point_xyz"][deg == 0].tobytes() == src[deg == 0].tobytes()
    # the point that keyframe 0 alone sees is optimised all the same
    kf0 = int(np.flatnonzero(np.asarray(prob["pose_id"]) == 0)[0])
    only0 = [j for j in np.flatnonzero(deg > 0) if set(prob["edge_pose"][prob["edge_point"] == j]) == {kf0}]
    assert only0 and all(np.abs(got["point_xyz"][j] - src[j]).max() > 0 for j in only0)
    # the fixed keyframe: through toSE3Quat and back
    assert np.abs(got["pose_Tcw"][kf0] - prob["pose_Tcw"][kf0]).max() <= 1e-6


def test_past_local_bas_limit(pkg, ba):
    """159 free keyframes: LocalBundleAdjustment refuses (existing behaviour), GlobalBundleAdjustment solves, and the handle goes on"""
    prob = problem("past_lba")
    assert R.free_keyframes(prob) == 159
    with pytest.raises(pkg.capi.AosError) as e:
        ba.LocalBundleAdjustment(prob)
    assert e.value.code == pkg.capi.AOS2_ERR_ARG
    got = ba.GlobalBundleAdjustment(prob, 10)
    assert got["status"] == 0 and got["iterations"] >= 1 and got["chi2_final"] < got["chi2_initial"] and got["l_blocks"] > got["h_blocks"]


def test_a_refused_call_leaves_the_sentinel_and_the_handle_works(pkg, ba, oracle):
    capi = pkg.capi
    prob = problem("pair")
    bad = prob["edge_pose"].copy()
    bad[1] = -2
    for kw in (dict(iterations=0), dict(prob=dict(prob, edge_pose=bad)), dict(prob=dict(prob, pose_id=None))):
        with pytest.raises(capi.AosError) as e:
            ba.GlobalBundleAdjustment(kw.get("prob", prob), kw.get("iterations", 10), sentinel=0x5A)
        assert e.value.code == capi.AOS2_ERR_ARG
        r, (Tout, Pout, inc) = ba.global_ba_last
        assert (Tout == 0x5A).all() and (Pout == 0x5A).all() and (inc == 77).all()
        assert r.iterations == r.trials == r.status == capi._GBA_SENTINEL_INT
    want, res = oracle_case(oracle, "pair")
    got = ba.GlobalBundleAdjustment(prob, R.iterations_of("pair"), True, R.HUBER_LOCAL_BA)
    assert not R.mismatches(got, want, res, "after the refusals")
    small = pkg.synth.synth_lba_problem(1, n_local=3, n_fixed=2, n_points=60, stereo_frac=0.5)
    lba, owant = ba.LocalBundleAdjustment(small), oracle.lba_solve(small)
    assert np.abs(lba["pose_Tcw"] - owant["pose_Tcw"]).max() < 1e-5 and (lba["edge_outlier"] == owant["edge_outlier"]).all()
