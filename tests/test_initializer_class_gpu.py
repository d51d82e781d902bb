"""host/Initializer.h, the class at the reference's signature, driven by tests/cpp/initializer_test.cpp on the GPU: what
Tracking::MonocularInitialization gets back (the return value, R21, t21, vP3D, vbTriangulated) against aos2_initializer_initialize on
the same arrays and against tests/initializer_ref.py, with the rand() values that make DUtils::Random::RandomInt draw the sets."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import initializer_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

# (kind, n_matches, n_extra, seed, iterations): an F and an H initialisation, a rejected one, one that ends at the d1/d2 exit
CASES = [("general", 120, 40, 0, 200), ("planar", 120, 0, 0, 200), ("low_parallax", 90, 10, 2, 50), ("static", 64, 5, 1, 20)]


def draw_positions(sets, n):
    """the RandomInt results that make the swap-with-back removal of :82-97 produce `sets`"""
    out = []
    for row in sets:
        avail = list(range(n))
        for v in row:
            r = avail.index(int(v))
            out.append((r, len(avail)))
            avail[r] = avail[-1]
            avail.pop()
    return out


def class_cases(synth):
    arrays, problems, rand = dict(cam=np.array(synth.TWO_VIEW_K, np.float32)), [], []
    for c, (kind, n, extra, seed, its) in enumerate(CASES):
        P = synth.synth_two_view(seed, kind, n_matches=n, n_extra=extra, iterations=its, outlier_frac=0.1 if kind == "general" else 0.0,
                                 noise=0.2 if kind == "general" else 0.0)
        m12 = np.full(len(P["keys1"]), -1, np.int32)
        m12[P["matches"][:, 0]] = P["matches"][:, 1]
        arrays.update({"c%d_params" % c: np.array([P["sigma"], its], np.float32), "c%d_key1" % c: P["keys1"], "c%d_key2" % c: P["keys2"],
                       "c%d_matches12" % c: m12})
        rand += [int((r + 0.5) * 2.0 ** 31 / d) for r, d in draw_positions(P["sets"], n)]
        problems.append({k: v for k, v in P.items() if k not in ("kind", "R21", "t21", "outlier")})
    arrays["rand"] = np.array(rand, np.int32)
    return arrays, problems


def test_initializer_class_returns_what_the_call_returns(pkg, gpu, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "initializer_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "initializer_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    arrays, problems = class_cases(pkg.synth)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    want = pkg.capi.Matcher(0.9, True, device=0).InitializerInitialize(problems)
    oks = []
    for c, (P, w) in enumerate(zip(problems, want)):
        q = "c%d_" % c
        assert R.same(w, R.solve(P)), c
        assert int(out[q + "rand_used"][0]) == 8 * len(P["sets"]) and int(out[q + "seeded"][0]) == 1, c
        ok = int(out[q + "ok"][0])
        oks.append((ok, w["used_homography"], w["n_hypotheses"]))
        assert ok == w["initialized"], c
        assert list(out[q + "empty"]) == [1 - ok, 1 - ok], c
        assert np.ascontiguousarray(out[q + "R21"], np.float32).tobytes() == w["R21"].tobytes(), c
        assert np.ascontiguousarray(out[q + "t21"], np.float32).tobytes() == w["t21"].tobytes(), c
        if ok:
            assert np.ascontiguousarray(out[q + "P3D"], np.float32).tobytes() == w["P3D"].tobytes(), c
            assert out[q + "tri"].tobytes() == w["triangulated"].tobytes(), c
        else:   # the reference leaves vP3D and vbTriangulated as they came
            assert out[q + "P3D"].size == 0 and out[q + "tri"].size == 0, c
    print("(ok, used_homography, n_hypotheses) per case:", oks)
    assert oks[0][:2] == (1, 0) and oks[1][:2] == (1, 1) and oks[2][0] == 0 and oks[3] == (0, 1, 0)
