"""aos2_initializer_initialize on the GPU against the library's host tap: every byte of every result, parallax within 1 float ulp
(ocml's and glibc's acos may differ in the last place).  The shapes are the smallest at which each kernel can go wrong: 8 matches
(every set a permutation of all of them), 9, 63 / 64 / 65 (the 64-match chunks of the score chain), 257 (more than one pass of a
256-thread workgroup); 1, 2 and 200 iterations (the models kernel's waves: one lane, H and F in one wave, 7 waves with a straddling
one); frames with and without 300 unmatched keys between the matched ones.  tests/test_initializer_cpu.py compares the same host tap
with the Python restatement."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import initializer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A

# (kind, n_matches, iterations, seed, outlier share, opposite): found with the generator so that together they cover what
# test_the_cases_cover_the_paths asserts; n_extra = 300 for odd seeds
CASES = [("planar", 257, 200, 0, 0.0, False), ("planar", 257, 200, 2, 0.0, False), ("planar", 257, 200, 6, 0.0, False),
         ("planar", 257, 200, 1, 0.0, False), ("planar", 65, 200, 0, 0.0, True), ("planar", 65, 200, 2, 0.0, True),
         ("planar", 65, 200, 5, 0.0, True), ("planar", 65, 200, 8, 0.0, True), ("rotation", 65, 200, 1, 0.2, False),
         ("low_parallax", 65, 2, 0, 0.2, False), ("general", 257, 200, 3, 0.2, False), ("general", 64, 200, 1, 0.2, False),
         ("general", 63, 2, 4, 0.0, False), ("general", 9, 200, 1, 0.0, False), ("general", 8, 1, 0, 0.0, False),
         ("general", 8, 2, 1, 0.0, False), ("planar", 8, 200, 2, 0.0, False), ("static", 64, 1, 1, 0.0, False),
         ("planar", 9, 1, 3, 0.0, False), ("general", 65, 1, 2, 0.5, False), ("rotation", 63, 200, 3, 0.2, False)]


def public(P):
    """the fields the binding reads"""
    return {k: v for k, v in P.items() if k not in ("kind", "R21", "t21", "outlier")}


def build_problems(synth):
    probs = []
    for kind, n, its, seed, out, opp in CASES:
        probs.append(public(synth.synth_two_view(seed, kind, n_matches=n, iterations=its, outlier_frac=out, noise=0.3 if out else 0.0,
                                                 n_extra=300 if seed % 2 else 0, opposite=opp)))
    probs.insert(len(probs) // 2, R.collinear())
    k = 0
    while len(probs) < 64:   # the batch of 64: small problems of every kind
        kind = synth.TWO_VIEW_KINDS[k % 4]
        probs.append(public(synth.synth_two_view(100 + k, kind, n_matches=(8, 9, 63, 64, 65)[k % 5], iterations=(1, 2, 200)[k % 3],
                                                 outlier_frac=0.2 * (k % 2), noise=0.3 * (k % 2), n_extra=300 * (k % 2))))
        k += 1
    return probs


@pytest.fixture(scope="module")
def world(pkg, gpu):
    problems = build_problems(pkg.synth)
    M = pkg.capi.Matcher(0.9, True, device=0)
    return problems, M, M.InitializerInitialize(problems), pkg.capi.debug_initializer_host(problems)


def brief(r):
    return {k: r[k] for k in ("status", "initialized", "used_homography", "SH", "SF", "best_iteration_h", "best_iteration_f", "n_hypotheses")}, r["n_good"]


def test_batch_of_64_equals_the_host_tap_byte_for_byte(pkg, world):
    problems, M, batch, tap = world
    assert len(problems) == 64
    for k, (g, t) in enumerate(zip(batch, tap)):
        assert R.raw(g) == R.raw(t), (k, brief(g), brief(t))
        assert R.parallax_ulps(g["parallax"], t["parallax"]) <= 1, (k, g["parallax"], t["parallax"])
    assert M.InitializerInitialize([]) == []


def test_the_cases_cover_the_paths(world):
    """what the byte comparison relies on: both H and F winners, every hypothesis of ReconstructH as the best one, nGood below, at
    and above 51 (both arms of min(50, size - 1)), initialised and rejected problems, the d1/d2 exit, a problem without a model"""
    problems, M, batch, tap = world
    best_h = {int(np.argmax(r["n_good"])) for r in batch if r["used_homography"] and r["n_hypotheses"] == 8 and r["n_good"].max() > 0}
    print("best hypotheses of ReconstructH:", sorted(best_h))
    assert best_h == set(range(8))
    chosen = {int(np.argmax(r["n_good"])) for r in batch if r["used_homography"] and r["initialized"]}
    print("hypotheses ReconstructH initialised with:", sorted(chosen))
    assert len(chosen) >= 6
    good = np.concatenate([r["n_good"][: r["n_hypotheses"]] for r in batch])
    assert ((good > 0) & (good < 51)).any() and (good == 51).any() and (good > 51).any()
    assert {r["used_homography"] for r in batch if r["initialized"]} == {0, 1}
    assert any(r["used_homography"] and r["n_hypotheses"] == 0 and r["status"] == 0 for r in batch)
    assert any(not r["used_homography"] and r["n_hypotheses"] == 4 and not r["initialized"] for r in batch)
    assert sum(r["status"] == 1 for r in batch) == 1   # AOS2_INIT_NO_MODEL
    assert {len(p["matches"]) for p in problems} >= {8, 9, 63, 64, 65, 257}
    assert {len(p["sets"]) for p in problems} == {1, 2, 3, 200}
    assert any(len(p["keys1"]) == len(p["matches"]) for p in problems) and any(len(p["keys1"]) == len(p["matches"]) + 300 for p in problems)


def test_one_problem_at_a_time_reversed_and_in_threes(world):
    problems, M, batch, tap = world
    for k, P in enumerate(problems[:24]):
        g = M.InitializerInitialize([P])[0]
        assert R.raw(g) + g["parallax"].tobytes() == R.raw(batch[k]) + batch[k]["parallax"].tobytes(), k
    rev = M.InitializerInitialize(problems[::-1])[::-1]
    assert [R.raw(a) + a["parallax"].tobytes() for a in rev] == [R.raw(b) + b["parallax"].tobytes() for b in batch]
    for lo in (0, 9, 20):
        three = M.InitializerInitialize(problems[lo:lo + 3])
        assert [R.raw(a) for a in three] == [R.raw(b) for b in batch[lo:lo + 3]]


def test_a_problem_without_a_model_leaves_its_neighbours_alone(pkg, world):
    problems, M, batch, tap = world
    k = next(i for i, r in enumerate(batch) if r["status"] == pkg.capi.AOS2_INIT_NO_MODEL)
    assert 0 < k < len(problems) - 1
    r = batch[k]
    assert r["initialized"] == 0 and r["SH"] == 0 and r["SF"] == 0 and r["best_iteration_h"] == -1 and r["best_iteration_f"] == -1
    assert not r["inliers_h"].any() and not r["inliers_f"].any() and not r["P3D"].any() and not r["H21"].any() and not r["F21"].any()
    without = M.InitializerInitialize(problems[k - 2:k] + problems[k + 1:k + 3])
    assert [R.raw(a) for a in without] == [R.raw(b) for b in batch[k - 2:k] + batch[k + 1:k + 3]]


def test_argument_errors_are_refused_and_the_result_buffers_keep_their_sentinel(pkg, world):
    problems, M, batch, tap = world
    P = problems[13]
    n = len(P["matches"])
    bad_match, bad_set = P["matches"].copy(), P["sets"].copy()
    bad_match[n // 2, 1] = len(P["keys2"])
    bad_set[-1, 7] = n
    for bad in (dict(P, matches=bad_match), dict(P, sets=bad_set), dict(P, sigma=0.0), dict(P, matches=P["matches"][:7], sets=P["sets"] % 7),
                dict(P, iterations=0), dict(P, null=("keys2",)), dict(P, null=("P3D",))):
        with pytest.raises(pkg.AosError) as e:
            M.InitializerInitialize([problems[12], bad, problems[14]], sentinel=SENTINEL)
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
        Rc, outs, before = M.init_last
        for k in range(3):
            assert bytes(Rc[k]) == before[k]
            assert all((a.view(np.uint8) == SENTINEL).all() for a in outs[k])
    assert [R.raw(a) for a in M.InitializerInitialize(problems[12:15])] == [R.raw(b) for b in batch[12:15]]   # the handle is as good as before
