"""aos2_pnp_ransac on the GPU against the library's host tap (every byte of every result) and against tests/pnp_ref.py (returned_at,
the best state, the counts and both flag arrays exactly, both poses bit for bit).  The workload is the generator's batch
(tests/test_pnp_cpu.py asserts what it covers); nothing larger runs."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import pnp_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
SEED = 3
SENTINEL = 0x5A


def raw(res):
    """every byte of a result"""
    return b"".join([np.array([res[k] for k in ("returned_at", "n_inliers", "best_iteration", "best_inliers")], np.int32).tobytes()] +
                    [np.ascontiguousarray(res[k]).tobytes() for k in ("Tcw", "best_Tcw", "inliers", "best")] +
                    ([np.ascontiguousarray(res["counts"]).tobytes()] if res["counts"] is not None else []))


def public(P):
    """the fields the binding reads"""
    return {k: v for k, v in P.items() if k not in ("member", "structures", "ransac_max_its", "octave")}


@pytest.fixture(scope="module")
def world(pkg, gpu):
    c = R.generator_case(SEED)
    problems = [public(P) for P in c["problems"]]
    M = pkg.capi.Matcher(0.75, True, device=0)
    return c, problems, M, M.PnpRansac(problems)


def test_batch_equals_the_host_tap_byte_for_byte_and_the_reference(pkg, world):
    c, problems, M, batch = world
    tap = pkg.capi.debug_pnp_host(problems)
    for k, (g, t, w) in enumerate(zip(batch, tap, c["want"])):
        brief = {x: (g[x], t[x]) for x in ("returned_at", "n_inliers", "best_iteration", "best_inliers")}
        assert raw(g) == raw(t), (k, brief, g["counts"][:12], t["counts"][:12])
        assert R.same(g, w), (k, brief)
    assert M.PnpRansac([]) == []


def test_one_problem_at_a_time_any_order_and_a_second_call_give_the_same_bytes(world):
    c, problems, M, batch = world
    for k, P in enumerate(problems):
        assert raw(M.PnpRansac([P])[0]) == raw(batch[k]), k
    order = [3, 0, 5, 0, 7, 5]   # the problem nothing runs for in the middle of a batch, and twice
    assert [raw(a) for a in M.PnpRansac([problems[k] for k in order])] == [raw(batch[k]) for k in order]
    assert [raw(a) for a in M.PnpRansac(problems)] == [raw(b) for b in batch]
    without = M.PnpRansac(problems, with_counts=False)
    assert all(a["counts"] is None for a in without)
    assert [raw(dict(a, counts=b["counts"])) for a, b in zip(without, batch)] == [raw(b) for b in batch]


def test_resumed_calls_equal_the_uninterrupted_loop(pkg, world):
    """every problem of the batch that returned: a second call from returned_at + 1 with the state carried in, against the host tap
    byte for byte and against the reference's second return (or its exhaustion) in ONE loop that ignores the first return"""
    c, problems, M, batch = world
    resumed, whole = [], []
    for P, b in zip(problems, batch):
        if b["returned_at"] < 0:
            continue
        resumed.append(dict(P, first_iteration=b["returned_at"] + 1, best_inliers_in=b["best_inliers"], best_in=b["best"]))
        whole.append(R.solve(P, ignore_returns=True))
    assert len(resumed) >= 4
    got, tap = M.PnpRansac(resumed), pkg.capi.debug_pnp_host(resumed)
    second_returns = carried_stands = 0
    for g, t, P, w in zip(got, tap, resumed, whole):
        assert raw(g) == raw(t)
        assert (g["counts"][: P["first_iteration"]] == -1).all()
        if len(w["events"]) > 1:
            ev = w["events"][1]
            second_returns += 1
            assert g["returned_at"] == ev["returned_at"] and g["n_inliers"] == ev["n_inliers"] and (g["inliers"] == ev["inliers"]).all()
            assert g["Tcw"].tobytes() == ev["Tcw"].tobytes() and g["best_inliers"] == ev["best_inliers"] and (g["best"] == ev["best"]).all()
            if ev["best_iteration"] >= P["first_iteration"]:
                assert g["best_iteration"] == ev["best_iteration"] and g["best_Tcw"].tobytes() == ev["best_Tcw"].tobytes()
            else:   # the second return refined the carried set
                carried_stands += 1
                assert g["best_iteration"] == -1 and not g["best_Tcw"].any()
            stop = ev["returned_at"] + 1
        else:
            assert g["returned_at"] == -1 and g["best_inliers"] == w["best_inliers"] and (g["best"] == w["best"]).all()
            stop = P["n_iterations"]
        assert (g["counts"][P["first_iteration"]:stop] == w["counts"][P["first_iteration"]:stop]).all() and (g["counts"][stop:] == -1).all()
    print("resumed problems:", len(resumed), "second returns:", second_returns, "of them on the carried set:", carried_stands)
    assert second_returns >= 1 and carried_stands >= 1


def test_bad_draws_are_refused_and_the_result_buffers_keep_their_sentinel(pkg, world):
    c, problems, M, batch = world
    n = len(problems[4]["P3Dw"])
    for it, i, bad in ((0, 0, n), (34, 3, n - 3), (17, 1, -1)):
        d = problems[4]["draws"].copy()
        d[it, i] = bad
        with pytest.raises(pkg.AosError) as e:
            M.PnpRansac([problems[3], dict(problems[4], draws=d), problems[5]], sentinel=SENTINEL)
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
        Rc, outs = M.pnp_last
        for k in range(3):
            assert all((a == SENTINEL).all() for a in outs[k])
            assert bytes(Rc[k])[: pkg.capi._PnpResult.inliers.offset] == bytes([SENTINEL]) * pkg.capi._PnpResult.inliers.offset
            assert Rc[k].best_inliers == int.from_bytes(bytes([SENTINEL]) * 4, "little")
    assert [raw(a) for a in M.PnpRansac(problems)] == [raw(b) for b in batch]   # the handle is as good as before


# ---------------------------------------------------------------------------------------------- the class at the reference's signature
PER_CALL, CALLS = 5, 2


def solver_case(rng, P):
    """a frame and matches whose PnPsolver has the correspondences of problem P (in order) after the gates of :79-101, two features
    without a map point and one with a bad one; the draws of P continued for a second call; the rand() values that make
    DUtils::Random::RandomInt return them; and what each of CALLS calls of iterate(PER_CALL) returns, from the reference"""
    n, ms = len(P["P3Dw"]), P["min_set"]
    nF = n + 3
    kept = np.array([i for i in range(nF) if i not in (0, 2, nF - 1)])
    key, octave, pos, state = np.zeros((nF, 2), np.float32), np.zeros(nF, np.int32), np.zeros((nF, 3), np.float32), np.zeros(nF, np.int32)
    key[kept], octave[kept], pos[kept], state[kept] = P["P2D"], P["octave"], P["P3Dw"], 1
    state[2] = 2
    draws = np.concatenate([P["draws"], R.draws_for(rng, n, 2 * PER_CALL, ms)])
    arrays = dict(ransac=np.array([R.PARAMS["min_inliers"], R.PARAMS["max_iterations"], ms, PER_CALL, CALLS], np.int32),
                  prob=np.array([R.PARAMS["probability"]], np.float64), eps_th2=np.array([R.PARAMS["epsilon"], R.TH2], np.float32),
                  key=key, octave=octave, mp_state=state, mp_pos=pos)
    # the replay of host/PnPsolver.h with the reference in place of the library
    max_its, done, best_n, best_flags, best_T = P["ransac_max_its"], 0, 0, None, None
    calls, drawn = [], 0
    for _ in range(CALLS):
        want = dict(found=0, no_more=0, n_inliers=0, inliers=np.zeros(0, np.uint8), Tcw=np.zeros((4, 4), np.float32))
        if n < P["min_inliers"]:
            calls.append(dict(want, no_more=1))
            continue
        end = done + max(max_its - done, PER_CALL, 0)
        drawn = max(drawn, end)
        Q = dict(P, draws=draws[:end], first_iteration=done, n_iterations=end, best_inliers_in=best_n, best_in=best_flags)
        w = R.solve(Q)
        if w["best_iteration"] >= 0:
            best_n, best_flags, best_T = w["best_inliers"], w["best"], w["best_Tcw"]
        flags = None
        if w["returned_at"] >= 0:
            done = w["returned_at"] + 1
            want.update(found=1, n_inliers=w["n_inliers"], Tcw=w["Tcw"])
            flags = w["inliers"]
        else:
            done = end
            if done >= max_its:
                want["no_more"] = 1
                if best_n >= P["min_inliers"]:
                    want.update(found=1, n_inliers=best_n, Tcw=best_T)
                    flags = best_flags
        if flags is not None:
            vb = np.zeros(nF, np.uint8)
            vb[kept] = flags
            want["inliers"] = vb
        calls.append(dict(want, margin_ulps=w["margin_ulps"], returned_at=w["returned_at"], first=Q["first_iteration"]))
    rand = [int((float(v) + 0.5) * 2.0 ** 31 / (n - i)) for row in draws[:drawn] for i, v in enumerate(row)]
    return arrays, rand, calls


def solver_cases(seed):
    c = R.generator_case(seed)
    rng = np.random.default_rng(seed + 100)
    arrays, rand, expect = dict(cam=np.array(R.CAMERA, np.float32), sigma2=np.array(R.level_sigma2(), np.float32)), [], []
    for k, P in enumerate(c["problems"][i] for i in (4, 6, 1, 3, 0)):
        a, r, calls = solver_case(rng, P)
        arrays.update({"c%d_%s" % (k, name): v for name, v in a.items()})
        rand += r
        expect.append((calls, len(r)))
    arrays["rand"] = np.array(rand, np.int32)
    return arrays, expect


def test_solver_cases_cover_the_paths_of_iterate():
    """(needs no device) what the next test relies on: a return in the first call of a solver that is then called again and returns
    again, an exhaustion with nothing, an exhaustion that returns the unrefined best, min_set = 5, and a solver below its minimum"""
    _, expect = solver_cases(SEED)
    brief = [[(c["found"], c["no_more"], c["n_inliers"], c.get("returned_at"), c.get("first")) for c in calls] for calls, _ in expect]
    print("(found, no_more, n_inliers, returned_at, first_iteration) per call:", brief)
    assert brief[0][0][:2] == (1, 0) and brief[0][0][3] >= PER_CALL and brief[0][1][0] == 1 and brief[0][1][4] == brief[0][0][3] + 1
    assert brief[1][0][:3] == (0, 1, 0) and brief[1][1][:3] == (0, 1, 0) and expect[1][1] == 4 * (35 + PER_CALL)
    assert brief[2][0][:4] == (1, 1, 10, -1) and brief[2][1][4] == 5
    assert brief[3][0][:2] == (1, 0) and expect[3][1] % 5 == 0
    assert brief[4] == [(0, 1, 0, None, None)] * 2 and expect[4][1] == 0
    assert min(c.get("margin_ulps", 1e9) for calls, _ in expect for c in calls) >= 16


def test_pnpsolver_class_replays_the_reference_loop(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "pnp_solver_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "pnp_solver_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    arrays, expect = solver_cases(SEED)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    for c, (calls, rand_used) in enumerate(expect):
        assert int(out["c%d_rand_used" % c][0]) == rand_used, c
        for k, want in enumerate(calls):
            q = "c%d_k%d_" % (c, k)
            got = (int(out[q + "found"][0]), int(out[q + "no_more"][0]), int(out[q + "n_inliers"][0]))
            assert got == (want["found"], want["no_more"], want["n_inliers"]), (c, k, got)
            assert out[q + "inliers"].tobytes() == want["inliers"].tobytes(), (c, k)
            assert np.ascontiguousarray(out[q + "Tcw"], np.float32).tobytes() == np.ascontiguousarray(want["Tcw"], np.float32).tobytes(), (c, k)
