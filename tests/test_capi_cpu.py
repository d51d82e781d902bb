"""Host-side checks of the product that need no GPU: the C-ABI library loads and exports every
symbol include/aos2.h declares, host tables equal the oracle's, the shared octree routine (host
execution) equals the oracle's DistributeOctTree, error behaviour without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    src = open(os.path.join(ROOT, "include", "aos2.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(aos2_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(pkg):
    L = pkg.capi.lib()
    names = declared_symbols()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing
    assert b"gfx950" in L.aos2_version()


def test_library_contains_gfx950_code_object(pkg):
    data = open(pkg.lib_path(), "rb").read()
    assert b"gfx950" in data and b"fast_cells_kernel" in data and b"describe_kernel" in data


def test_host_tables_match_oracle(pkg, oracle):
    for nf, sf, nl in ((1000, 1.2, 8), (2000, 1.2, 8), (1200, 1.2, 8), (500, 1.5, 4), (3000, 1.1, 12)):
        a = pkg.Extractor(nfeatures=nf, scale_factor=sf, nlevels=nl)
        b = oracle.Extractor(nfeatures=nf, scale_factor=sf, nlevels=nl)
        assert a.GetLevels() == nl and a.GetScaleFactor() == np.float32(sf)
        assert (a.GetScaleFactors() == b.scale_factors).all()
        assert (a.GetInverseScaleFactors() == b.inv_scale_factors).all()
        assert (a.GetScaleSigmaSquares() == b.sigma2).all()
        assert (a.GetInverseScaleSigmaSquares() == b.inv_sigma2).all()
        assert (a.features_per_level == b.features_per_level).all()
        assert (a.umax == b.umax).all()
        assert a.max_keypoints >= nf


def test_keypoint_capacity_bound_covers_the_octree(pkg, oracle):
    """aos2_extractor_max_keypoints_for(w, h) (host arithmetic, no device): per level max(N + 3, 4 * round(W / H)) --
    DistributeOctTree's first pass divides all round(W / H) root nodes unconditionally (src/ORBextractor.cc:549-590).
    Checked against the formula and against what the oracle's octree actually returns on crowded wide levels."""
    rng = np.random.default_rng(5)
    for _ in range(40):
        w, h = int(rng.integers(120, 2000)), int(rng.integers(100, 700))
        nf, sf, nl = int(rng.choice([50, 100, 1000])), float(rng.choice([1.1, 1.2, 1.5])), int(rng.integers(1, 9))
        ex = pkg.Extractor(nfeatures=nf, scale_factor=sf, nlevels=nl)
        inv = ex.GetInverseScaleFactors()
        want = 0
        for l, n_l in enumerate(ex.features_per_level):
            lw, lh = int(np.rint(np.float32(w) * inv[l])), int(np.rint(np.float32(h) * inv[l]))
            b = int(n_l) + 3
            if lw > 32 and lh > 32:
                r = np.float32(lw - 32) / np.float32(lh - 32)
                b = max(b, 4 * int(np.floor(r + np.float32(0.5))))      # round(): half away from zero
            want += b
        assert ex.max_keypoints_for(w, h) == want >= ex.max_keypoints
    # the bound is reached: 7 root nodes, every one crowded, N = 20 -> 28 leaves
    W, H = 7 * 60, 60
    xs, ys = np.meshgrid(np.arange(2, W - 2, 3, dtype=np.float32), np.arange(2, H - 2, 3, dtype=np.float32))
    xs, ys = xs.ravel(), ys.ravel()
    sel = oracle.distribute_octree(xs, ys, np.ones(len(xs), np.float32), 0, W, 0, H, 20)
    assert len(sel) == 28 > 20 + 3


def _check_plan(P, levels, level_sizes):
    """the properties of an extractor plan (Extractor.debug_plan) that hold for every geometry"""
    lv, cells = P["levels"], P["cells"]
    assert len(lv) == levels and (np.diff(cells[:, 0]) >= 0).all() and set(cells[:, 0]) == set(range(levels))
    end = 0
    for l in range(levels):
        lw, lh, pitch, off = (int(v) for v in lv[l])
        assert (lw, lh) == level_sizes[l]
        # planes: pitch a multiple of 16 with room for a 32-bit load past the row end, 256-byte aligned, ascending, disjoint
        assert pitch % 16 == 0 and pitch >= lw + 4 and off % 256 == 0 and off >= end
        end = off + pitch * (lh + 1)
        # the cells tile [19, w - 19) x [19, h - 19) exactly once (src/ORBextractor.cc:768-806), none wider than a FAST tile
        cover = np.zeros((lh, lw), np.int32)
        for _, x0, y0, cw, ch, _ in cells[cells[:, 0] == l]:
            assert 0 < cw <= 64 and ch > 0 and x0 >= 19 and y0 >= 19 and x0 + cw <= lw - 19 and y0 + ch <= lh - 19
            cover[y0:y0 + ch, x0:x0 + cw] += 1
        want = np.zeros((lh, lw), np.int32)
        want[19:lh - 19, 19:lw - 19] = 1
        assert (cover == want).all()
    assert end <= P["pyr_bytes"]
    slots = ((cells[:, 3] + 1) // 2).astype(np.int64) * ((cells[:, 4] + 1) // 2)
    assert (cells[:, 5] == np.concatenate([[0], np.cumsum(slots)[:-1]])).all()
    assert P["slot_total"] == (int(slots.sum()) + 63) // 64 * 64


@pytest.mark.parametrize("w,h,scale,levels,nfeatures", [
    (640, 480, 1.2, 8, 1000), (1241, 376, 1.2, 8, 2000), (752, 480, 1.2, 8, 1200), (401, 323, 1.3, 5, 500),
    (200, 180, 1.1, 8, 300), (517, 333, 1.2, 8, 700), (838, 118, 1.2, 2, 100), (640, 480, 2.0, 3, 500)])
def test_extractor_plan_without_a_device(pkg, oracle, w, h, scale, levels, nfeatures):
    """aos2_debug_extractor_plan: level planes, grid cells and slot offsets are host arithmetic, checked here without a GPU -- level
    sizes against the oracle's pyramid, the cells against the reference's grid rule, the layout against what the kernels assume."""
    ref = oracle.Extractor(nfeatures=nfeatures, scale_factor=scale, nlevels=levels)
    ref.extract(pkg.synth.synth_image(1, w, h))
    sizes = [ref.level_size(l)[:2] for l in range(levels)]
    _check_plan(pkg.Extractor(nfeatures=nfeatures, scale_factor=scale, nlevels=levels).debug_plan(w, h), levels, sizes)
    # the two refusals, and the tap still answers afterwards (it plans aside and never touches the handle's own plan: the commit
    # point of an extract call, which needs a device, is not what this checks)
    ex, fresh = pkg.Extractor(), pkg.Extractor().debug_plan(640, 480)
    for (bw, bh), code in (((100, 100), pkg.capi.AOS2_ERR_TOO_SMALL), ((4001, 480), pkg.capi.AOS2_ERR_ARG)):
        with pytest.raises(pkg.capi.AosError) as err:
            ex.debug_plan(bw, bh)
        assert err.value.code == code
        again = ex.debug_plan(640, 480)
        assert all(np.array_equal(again[k], fresh[k]) for k in fresh)
    if (w, h, scale, levels) == (640, 480, 1.2, 8):
        _check_plan(again, levels, sizes)


def test_bad_arguments_and_missing_device(pkg):
    capi = pkg.capi
    with pytest.raises(capi.AosError) as e:
        pkg.Extractor(nfeatures=0)
    assert e.value.code == capi.AOS2_ERR_ARG
    with pytest.raises(capi.AosError):
        pkg.Extractor(nlevels=40)
    ex = pkg.Extractor()
    # empty image: silent return like src/ORBextractor.cc:1046 (no device needed)
    k, d = ex(np.zeros((0, 0), np.uint8))
    assert len(k) == 0 and d.shape == (0, 32)
    with pytest.raises(AssertionError):
        ex(np.zeros((480, 640), np.float32))
    # aos2_device_local_cpus: argument checks need no device; without one the call says so and bind_to_device_node changes nothing
    L = capi.lib()
    assert L.aos2_device_local_cpus(0, None, 16) == capi.AOS2_ERR_ARG
    if pkg.device_count() == 0:
        import os
        before = os.sched_getaffinity(0)
        with pytest.raises(capi.AosError) as e:
            pkg.device_local_cpus(0)
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE
        assert pkg.bind_to_device_node(0) == 0 and os.sched_getaffinity(0) == before
        with pytest.raises(capi.AosError) as e:
            ex(np.zeros((480, 640), np.uint8))
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE  # loud failure, no CPU fallback
        # the keyframe entry points on batches that were never built: an argument error, nothing is touched
        fa, fb = pkg.capi.Frames(2, 64), pkg.capi.Frames(2, 64)
        z = np.zeros(1, np.int32)
        with pytest.raises(capi.AosError) as e:
            fa.SearchForTriangulation(fb, z, z, np.zeros((1, 9), np.float32), np.zeros((1, 2), np.float32), 8, [8] * 4, [8] * 4, 8, 8)
        assert e.value.code == capi.AOS2_ERR_ARG
        with pytest.raises(capi.AosError) as e:
            pkg.Matcher().hamming_best2(np.zeros((4, 32), np.uint8), np.zeros((4, 32), np.uint8))
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE
        prob = pkg.synth.synth_lba_problem(1, n_local=2, n_fixed=1, n_points=20)
        with pytest.raises(capi.AosError) as e:
            pkg.LocalBA().LocalBundleAdjustment(prob)
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE


def test_matcher_rejects_inconsistent_inputs_before_any_upload(pkg):
    """the arrays that become device-side indices (mGrid as CSR, pyramid levels) are validated on the host: a bad one is
    AOS2_ERR_ARG with a message, on a machine without a GPU too (nothing has been uploaded yet)"""
    capi = pkg.capi
    f, mp = pkg.synth.synth_proj_mp_problem(3, n_f=300, n_mp=200)
    m = pkg.Matcher()

    def bad(frame, points, what):
        with pytest.raises(capi.AosError) as e:
            m.SearchByProjection(frame, points)
        assert e.value.code == capi.AOS2_ERR_ARG and what in str(e.value), str(e.value)

    g = dict(f); g["grid_off"] = f["grid_off"].copy(); g["grid_off"][100] = g["grid_off"][99] - 1 if g["grid_off"][99] > 0 else -1
    bad(g, mp, "grid_off")
    g = dict(f); g["grid_idx"] = f["grid_idx"].copy(); g["grid_idx"][0] = f["n_f"]
    bad(g, mp, "grid_idx")
    g = dict(f); g["kp_octave"] = f["kp_octave"].copy(); g["kp_octave"][5] = f["n_levels"]
    bad(g, mp, "kp_octave")
    iv, nv = int(np.flatnonzero(mp["track_in_view"])[3]), int(np.flatnonzero(mp["track_in_view"] == 0)[0])
    q = dict(mp); q["pred_level"] = mp["pred_level"].copy(); q["pred_level"][iv] = -1
    bad(f, q, "pred_level")
    # mnTrackScaleLevel of a point that is NOT in view is never read by the reference (src/ORBmatcher.cc:55-61): a stale value
    # there is legal -- the call passes validation (and, on this machine without a GPU, stops at the device)
    q = dict(mp); q["pred_level"] = mp["pred_level"].copy(); q["pred_level"][nv] = -12345
    if pkg.device_count() < 1:
        with pytest.raises(capi.AosError) as e:
            m.SearchByProjection(f, q)
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE
    cur, last = pkg.synth.synth_proj_last_problem(4, n=200)
    lv, ln = int(np.flatnonzero(last["last_valid"])[3]), int(np.flatnonzero(last["last_valid"] == 0)[0])
    l2 = dict(last); l2["last_octave"] = last["last_octave"].copy(); l2["last_octave"][lv] = 99
    with pytest.raises(capi.AosError) as e:
        m.SearchByProjectionLast(cur, l2, 7.0, False)
    assert e.value.code == capi.AOS2_ERR_ARG and "last_octave" in str(e.value)
    l2 = dict(last); l2["last_octave"] = last["last_octave"].copy(); l2["last_octave"][ln] = 99   # no usable map point: never read
    if pkg.device_count() < 1:
        with pytest.raises(capi.AosError) as e:
            m.SearchByProjectionLast(cur, l2, 7.0, False)
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE


def test_image_bounds_host_equals_oracle(pkg, oracle):
    """Frame::ComputeImageBounds: the library's host routine (the function the device also runs on the keypoints) against
    the oracle's cv::undistortPoints restatement, bit for bit; zero distortion = the image"""
    fx, fy, cx, cy = 517.306408, 516.469215, 318.643040, 255.313989
    for dist in ([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], [0.05, 0.0, 0.0, 0.0, 0.0], [-0.28, 0.07, 0.0002, 1e-5, 0.0]):
        c = oracle.undistort_points(np.array([[0, 0], [640, 0], [0, 480], [640, 480]], np.float32), fx, fy, cx, cy, dist)
        want = np.array([min(c[0, 0], c[2, 0]), max(c[1, 0], c[3, 0]), min(c[0, 1], c[1, 1]), max(c[2, 1], c[3, 1])], np.float32)
        assert pkg.capi.frame_image_bounds(640, 480, fx, fy, cx, cy, dist).tobytes() == want.tobytes()
    assert (pkg.capi.frame_image_bounds(640, 480, fx, fy, cx, cy, [0, 0.1, 0, 0, 0]) == np.array([0, 640, 0, 480], np.float32)).all()


def test_descriptor_distance_host(pkg, oracle):
    rng = np.random.default_rng(0)
    for _ in range(100):
        a = rng.integers(0, 256, 32, dtype=np.uint8)
        b = rng.integers(0, 256, 32, dtype=np.uint8)
        assert pkg.Matcher.DescriptorDistance(a, b) == oracle.descriptor_distance(a, b)
    assert pkg.Matcher.TH_LOW == 50 and pkg.Matcher.TH_HIGH == 100 and pkg.Matcher.HISTO_LENGTH == 30


def test_octree_routine_matches_oracle_on_extractor_candidates(pkg, oracle):
    for seed, (w, h, nf) in enumerate([(640, 480, 1000), (1241, 376, 2000), (752, 480, 1200)]):
        img = pkg.synth.synth_image(20 + seed, w, h)
        oe = oracle.Extractor(nfeatures=nf)
        oe.extract(img)
        for l in range(8):
            x, y, s = oe.level_candidates(l)
            lw, lh, _ = oe.level_size(l)
            N = int(oe.features_per_level[l])
            a = oracle.distribute_octree(x, y, s, 16, lw - 16, 16, lh - 16, N)
            b = pkg.capi.debug_octree_host(x, y, s, 16, lw - 16, 16, lh - 16, N)
            assert len(a) == len(b) == oe.level_nkeys(l) and (a == b).all()


def test_octree_routine_ties_and_degenerate_inputs(pkg, oracle):
    rng = np.random.default_rng(3)
    for case in range(60):
        W, H = int(rng.integers(40, 1300)), int(rng.integers(40, 500))
        if W < H * 0.5:
            W = H  # nIni would be 0 (the reference divides by zero on tall boxes)
        n = int(rng.integers(1, 3000))
        N = int(rng.integers(1, 500))
        pts = np.unique(np.stack([rng.integers(3, W - 3, n), rng.integers(3, H - 3, n)], 1), axis=0)
        rng.shuffle(pts)
        x, y = pts[:, 0].astype(np.int16), pts[:, 1].astype(np.int16)
        if case % 3 == 0:
            s = np.full(len(x), 50, np.uint8)            # all responses tie
        elif case % 3 == 1:
            s = rng.integers(7, 12, len(x)).astype(np.uint8)  # many ties
        else:
            s = rng.integers(7, 255, len(x)).astype(np.uint8)
        if case % 5 == 0:  # clustered points: deep, degenerate splits
            x = (x // 8 + 5).astype(np.int16)
            y = (y // 8 + 5).astype(np.int16)
            u = np.unique(np.stack([x, y], 1), axis=0)
            x, y, s = u[:, 0].astype(np.int16), u[:, 1].astype(np.int16), s[: len(u)]
        a = oracle.distribute_octree(x, y, s, 0, W, 0, H, N)
        b = pkg.capi.debug_octree_host(x, y, s, 0, W, 0, H, N)
        assert len(a) == len(b) and (a == b).all(), case
        assert len(set(a.tolist())) == len(a)
        assert len(a) <= min(len(x), N + 3)


def test_sincos_host_tap_equals_oracle(pkg, oracle):
    L = oracle.lib()
    L.orc_sincos_exact.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    for a in np.linspace(0, 6.2832, 5000).astype(np.float32):
        s, c = C.c_float(), C.c_float()
        L.orc_sincos_exact(float(a), C.byref(s), C.byref(c))
        assert pkg.capi.debug_sincos_host(a) == (s.value, c.value)


def test_synth_is_seeded(pkg):
    a, b = pkg.synth.synth_image(3), pkg.synth.synth_image(3)
    assert (a == b).all() and a.dtype == np.uint8 and a.shape == (480, 640)
    assert (pkg.synth.synth_image(4) != a).any()
    off, idx, gwi, ghi = pkg.synth.build_grid(np.array([0.0, 639.9, 320.0], np.float32), np.array([0.0, 479.9, 240.0], np.float32), 0, 0, 640, 480)
    assert off[-1] == 2 and len(off) == 64 * 48 + 1  # the point at the max border falls outside (posX == 64)


def test_vocabulary_host_side_without_gpu(pkg, oracle, tmp_path):
    """Loaders, getters, saveToBinaryFile and score() are host code: same results as the oracle, no device."""
    S = pkg.synth
    voc = S.synth_vocabulary(5, 10, 3)
    V, O = pkg.Vocabulary(), oracle.Vocabulary()
    assert V.empty() and V.info()["nodes"] == 0
    V.set_nodes(10, 3, 0, 0, voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
    O.set_nodes(10, 3, 0, 0, voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
    assert V.info() == O.info() == dict(k=10, L=3, scoring=0, weighting=0, nodes=1111, words=1000)
    a, b = tmp_path / "a.bin", tmp_path / "b.bin"
    V.saveToBinaryFile(a)
    assert O.save_binary(b) and a.read_bytes() == b.read_bytes()
    V2 = pkg.Vocabulary()
    assert V2.loadFromBinaryFile(a) and V2.info()["nodes"] == 1112 and V2.info()["words"] == 1001   # eof quirk
    assert not V2.loadFromBinaryFile(tmp_path / "missing.bin") and not V2.loadFromTextFile(tmp_path / "missing.txt")
    bad = tmp_path / "bad.txt"
    bad.write_text("99 3 0 0\n")
    assert not V2.loadFromTextFile(bad)
    with pytest.raises(pkg.AosError):
        V2.set_nodes(10, 3, 0, 0, [0, 5], voc["desc"][:2], voc["weight"][:2], voc["is_leaf"][:2])  # parent after child
    assert V2.empty()
    rng = np.random.default_rng(1)
    r1, r2 = O.transform(S.vocab_descriptors(rng, voc, 400), 2), O.transform(S.vocab_descriptors(rng, voc, 400), 2)
    assert V.score(r1, r2) == oracle.vocab_score_l1(r1, r2) and abs(V.score(r1, r1) - 1.0) < 1e-12
    if pkg.device_count() == 0:  # transform needs the device: loud failure, no CPU fallback
        with pytest.raises(pkg.AosError):
            V.transform(voc["desc"][:10], 2)


def test_host_alloc_needs_the_gpu_runtime(pkg):
    """aos2_host_alloc is page-locked memory from the HIP runtime: without a device it must say so, not hand out malloc"""
    import ctypes as C
    L = pkg.capi.lib()
    p = C.c_void_p(123)
    if pkg.device_count() > 0:
        pytest.skip("GPU present")
    assert L.aos2_host_alloc(C.byref(p), 4096) == -5 and not p.value
    assert L.aos2_host_free(None) == 0
    with pytest.raises(pkg.AosError):
        pkg.host_empty((4, 4))


def test_replay_entry_points_validate_their_arguments(pkg):
    """include/aos2.h "Replay of a fixed call sequence": the argument checks that need no device -- a recording needs a handle's
    stream (not the null stream), a launch needs a graph; destroying nothing is allowed."""
    L = pkg.capi.lib()
    assert L.aos2_capture_begin(None) == pkg.capi.AOS2_ERR_ARG
    assert b"stream" in L.aos2_last_error()
    h = C.c_void_p()
    assert L.aos2_capture_end(None, C.byref(h)) == pkg.capi.AOS2_ERR_ARG and not h.value
    assert L.aos2_graph_launch(None, None) == pkg.capi.AOS2_ERR_ARG
    assert L.aos2_graph_nodes(None) == 0
    L.aos2_graph_destroy(None)


@pytest.mark.parametrize("flags", [["-DAOS2_HOST_EXCEPTIONS"], []])
def test_reference_signature_classes_compile_and_link(pkg, tmp_path, flags):
    """host/*.h at the reference's signatures compile (-Wall -Werror, both error conventions) against the stand-in declarations of
    tests/cpp/refstub -- whose MapPoint keeps mfMinDistance / mfMaxDistance / mMutexPos PROTECTED like include/MapPoint.h:123-154: the
    shim reads them through aos2::MapPointDistances, no accessor added to the reference's class -- and link against libaos2 (the run
    needs the GPU: tests/test_ref_signature_gpu.py)."""
    import subprocess
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "ref_signature_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "cpp", "ref_signature_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    stub = open(os.path.join(ROOT, "tests", "cpp", "refstub", "slam_stub.h")).read()
    assert "GetMaxDistance()" not in stub and "GetMinDistance()" not in stub
    assert re.search(r"protected:[^}]*mfMinDistance[^}]*mMutexPos", stub, flags=re.S)


def test_refcheck_project_configures_and_says_what_it_cannot_build(tmp_path):
    """tools/refcheck (the reference's own g2o + ORBextractor.cc + ORBmatcher.cc compiled untouched next to the oracle: the route to a
    PINNED oracle) is a one-command affair on a machine that has OpenCV and Eigen3.  Here it must configure
    cleanly and say what is missing -- this image has neither library (/root/reference/CMakeLists.txt:33-41 asks for both), so no
    target is generated and nothing of the reference is built or stood in for."""
    import shutil
    import subprocess
    if shutil.which("cmake") is None:
        pytest.skip("no cmake on this box")
    r = subprocess.run(["cmake", "-S", os.path.join(ROOT, "tools", "refcheck"), "-B", str(tmp_path / "b"), "-DAOS2_REFERENCE_DIR=" + str(tmp_path / "no_checkout")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout + r.stderr
    have_cv = "OpenCV not found" not in out
    have_eigen = "refcheck_lba is not built" not in out
    assert "Configuring done" in out
    if not have_cv:
        assert "refcheck: OpenCV not found" in out
    if not have_eigen:
        assert "refcheck: Eigen3 or" in out
    # the sources the project would compile exist and name the switches a pinned run reports per convention
    src = open(os.path.join(ROOT, "tools", "refcheck", "refcheck_extractor.cpp")).read()
    assert "orc_set_tiebreak_mode" in src and "orc_set_trig_mode" in src
    assert "resolution" in open(os.path.join(ROOT, "tools", "refcheck", "refcheck_lba.cpp")).read()
    assert "lba_resolution" in open(os.path.join(ROOT, "tools", "refcheck", "dump_cases.py")).read()


def test_lba_window_builder_on_a_hand_made_graph(tmp_path):
    """aos2::LbaWindow (host/LbaWindow.h) without a GPU: optimised keyframes / map points / constant cameras / edges of a hand-made pointer
    graph with bad keyframes, a bad point, the map's first keyframe, a stereo observation and observers outside the window come out as
    src/Optimizer.cc:457-654 prescribes (edges by ascending KeyFrame::mnId: parity convention 2), and the reference's mnBA...ForKF
    stamps are not touched (tests/cpp/lba_window_test.cpp)."""
    import subprocess
    exe = str(tmp_path / "lba_window_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "lba_window_test.cpp"),
                           "-I", os.path.join(ROOT, "tests", "cpp", "refstub"), "-I", os.path.join(ROOT, "active-orb-slam2_amd", "host"),
                           "-I", os.path.join(ROOT, "include"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert "lba_window_test ok: 5 keyframes (3 optimised), 3 points, 8 edges" in out


def test_region_list_offsets_and_binding(tmp_path):
    """aos2::Regions (csrc/regions.h), the typed region list of the frame batch's buffers, as a stand-alone program under the address
    and undefined-behaviour sanitizers: 256-byte offsets, disjoint regions in order of registration (one of them empty), bytes(),
    what bind() writes into the fields, the same layout from the same calls.  And aos2::HostArena, the arena of the loop-closing
    optimisers with its staged prefix: an empty region first and last, a null source among the inputs, an element 20 bytes wide, a
    field set with at() inside an array, bind() to two bases, and a caller's buffer that the last push fills exactly or misses by a
    byte (tests/cpp/regions_test.cpp)."""
    import subprocess
    exe = str(tmp_path / "regions_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "regions_test.cpp"), "-I", os.path.join(ROOT, "active-orb-slam2_amd", "csrc"),
                           "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert "regions_test ok: 7 regions, 1536 bytes; host arena ok: 7 fields, 612 of 1280 bytes staged" in out


def test_local_map_array_list_layouts_and_round_trip(tmp_path):
    """The one list of the resident local map's arrays (csrc/local_map_arrays.h), as a stand-alone program under the address and
    undefined-behaviour sanitizers: lm_each visits 11 arrays without the view and 17 with it, each once; the graph block of a planted
    graph (3 points, one of them unobserved, 2 keyframes) is 2568 bytes, 4098 with the view, every array on the 256-byte boundary it
    has always had, and the empty map's block 768; the mirror survives a block of exactly that size and back, zero-length arrays
    included; a delta's block follows the order of aos2_local_map_apply's upload; an appended row reads 1, 0, 1, -1, -1, 0.f, 0
    (tests/cpp/local_map_arrays_test.cpp)."""
    import subprocess
    exe = str(tmp_path / "local_map_arrays_test")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "cpp", "local_map_arrays_test.cpp"), "-I", os.path.join(ROOT, "active-orb-slam2_amd", "csrc"),
                           "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert "local_map_arrays_test ok: 11 + 6 arrays; graph block 2568 / 4098 bytes, empty map 768; delta block 3332 / 4865 bytes" in out


def test_frame_members_of_a_batch_that_was_never_built(pkg):
    """aos2_frames_get / aos2_frames_device_ptr on a batch without a build: whatever the id -- the gettable 0-8, the device-pointer-only
    9 and 10, ids the header does not define -- the one answers with an argument error and the other with NULL, and no device is looked
    for.  (Both return before they consult the member table: that is test_every_member_by_copy_and_by_device_pointer's, on a GPU.)"""
    capi = pkg.capi
    f = capi.Frames(2, 64)
    for what in [-1] + list(range(12)) + [9999]:
        with pytest.raises(capi.AosError) as e:
            f.get(what)
        assert e.value.code == capi.AOS2_ERR_ARG, what
        assert f.device_ptr(what) == 0, what
        assert f.L.aos2_frames_device_ptr(f.h, what) is None, what


def test_reduced_solve_tap_and_lba_size_limit_refuse_on_the_host(pkg):
    """aos2_debug_lba_reduced_solve_device checks its arguments before it looks for a device: a NULL, no cases, np < 1, the register
    form beyond 40 free keyframes, the device-memory form beyond the 154 whose LDS a compute unit holds, an unknown form.  The same
    limit refuses a LocalBA window in the host phase that aos2_lba_solve_batch runs before it enqueues anything."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ldlt_ref
    capi = pkg.capi
    L = capi.lib()
    H, b = np.eye(6), np.ones(6)
    T = np.array([[0, 0, 0, 1.0, 0, 0, 0]])

    def one(form, q, **kw):
        c = dict(form=form, H=np.eye(6 * q), bs=np.ones(6 * q), b_pose=np.ones(6 * q), x0=np.zeros(6 * q), scale0=np.zeros(6 * q), lam=1.0,
                 T=np.tile(T, (q, 1)))
        c.update(kw)
        return c

    for bad in (one(2, 41), one(0, 155), one(1, 1), one(3, 1), one(-1, 1)):
        with pytest.raises(capi.AosError) as e:
            capi.debug_lba_reduced_solve_device([bad])
        assert e.value.code == capi.AOS2_ERR_ARG, bad["form"]
    f = L.aos2_debug_lba_reduced_solve_device
    q1, f2 = np.array([1], np.int32), np.array([2], np.int32)
    lam, x, To, Tb, sc, ok = np.ones(1), np.zeros(6), np.zeros(7), np.zeros(7), np.zeros(6), np.zeros(1, np.uint8)
    args = [q1, f2, H, b, b, lam, T, x, To, Tb, sc, ok]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    for k in range(len(args)):   # every pointer in turn
        a = list(args)
        a[k] = None
        assert f(1, *[p(v) for v in a], 0) == capi.AOS2_ERR_ARG, k
    assert f(0, *[p(v) for v in args], 0) == capi.AOS2_ERR_ARG
    z = np.zeros(1, np.int32)
    assert f(1, p(z), *[p(v) for v in args[1:]], 0) == capi.AOS2_ERR_ARG   # np = 0
    if pkg.device_count() == 0:   # good arguments get as far as the device
        with pytest.raises(capi.AosError) as e:
            capi.debug_lba_reduced_solve_device([one(2, 40), one(0, 154)])
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE
    # a LocalBA window: 154 free keyframes pass the host phase, 155 do not
    capi.lba_host_phase([ldlt_ref.lba_star_window(154)], 1)
    with pytest.raises(capi.AosError) as e:
        capi.lba_host_phase([ldlt_ref.lba_star_window(155)], 1)
    assert e.value.code == capi.AOS2_ERR_ARG and "155 free keyframes" in str(e.value)


def test_assembly_tap_refuses_on_the_host(pkg):
    """aos2_debug_lba_assemble_device checks its arguments before it looks for a device: a NULL, no problems, another layout or stage,
    iterations < 1, a window the host phase of the solve refuses (an edge out of range, two edges between one keyframe and one landmark,
    155 free keyframes) or one without a free keyframe."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ldlt_ref
    import lba_system_ref as S
    capi = pkg.capi
    ba = capi.LocalBA()
    win = S.make_window(1, 2, 2, S.sees_counts(3))

    def refused(w, text=None, **kw):
        with pytest.raises(capi.AosError) as e:
            ba.debug_assemble([win, w], **kw)
        assert e.value.code == capi.AOS2_ERR_ARG, (kw, str(e.value))
        assert text is None or text in str(e.value), str(e.value)

    for kw in (dict(layout=2), dict(layout=-1), dict(stage=2), dict(stage=-1), dict(iters=(0, 10)), dict(stage=1, iters=(5, 0))):
        refused(win, **kw)
    ep = win["edge_pose"].copy()
    ep[3] = win["n_poses"]
    refused(dict(win, edge_pose=ep), "out of range")
    dup = dict(win, edge_pose=np.r_[win["edge_pose"], win["edge_pose"][:1]], edge_point=np.r_[win["edge_point"], win["edge_point"][:1]],
               edge_obs=np.r_[win["edge_obs"], win["edge_obs"][:1]], edge_stereo=np.r_[win["edge_stereo"], win["edge_stereo"][:1]],
               edge_inv_sigma2=np.r_[win["edge_inv_sigma2"], win["edge_inv_sigma2"][:1]], n_edges=win["n_edges"] + 1)
    refused(dup, "same keyframe and map point")
    refused(ldlt_ref.lba_star_window(155), "155 free keyframes")
    refused(dict(win, pose_fixed=np.ones(win["n_poses"], np.uint8)), "no free keyframe")
    f = capi.lib().aos2_debug_lba_assemble_device
    S_, R_, O_ = (capi._LbaProblem * 1)(), (capi._LbaResult * 1)(), (capi._LbaSystem * 1)()
    keep = []
    ba._fill(S_[0], R_[0], win, None, (5, 10), keep)
    bufs = {k: np.zeros(4096, np.float64) for k, _ in capi._LbaSystem._fields_[9:]}
    for k, a in bufs.items():
        setattr(O_[0], k, a.ctypes.data)
    assert f(None, C.byref(S_), 1, 0, 0, None, C.byref(O_)) == capi.AOS2_ERR_ARG
    assert f(ba.h, None, 1, 0, 0, None, C.byref(O_)) == capi.AOS2_ERR_ARG
    assert f(ba.h, C.byref(S_), 1, 0, 0, None, None) == capi.AOS2_ERR_ARG
    assert f(ba.h, C.byref(S_), 0, 0, 0, None, C.byref(O_)) == capi.AOS2_ERR_ARG
    for k in bufs:   # every output array in turn
        setattr(O_[0], k, None)
        assert f(ba.h, C.byref(S_), 1, 0, 0, None, C.byref(O_)) == capi.AOS2_ERR_ARG, k
        setattr(O_[0], k, bufs[k].ctypes.data)
    for k in ("pose_Tcw", "edge_obs", "point_id"):   # ... and inputs of the problem
        old = getattr(S_[0], k)
        setattr(S_[0], k, None)
        assert f(ba.h, C.byref(S_), 1, 0, 0, None, C.byref(O_)) == capi.AOS2_ERR_ARG, k
        setattr(S_[0], k, old)
    if pkg.device_count() == 0:   # good arguments get as far as the device
        with pytest.raises(capi.AosError) as e:
            ba.debug_assemble([win])
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE


def test_trial_tap_refuses_on_the_host(pkg):
    """aos2_debug_lba_trial_device checks its arguments before it looks for a device: a NULL (the handle, the problems, the outputs, every
    index array of a window, inputs of the problem), no problems, another layout or tail, a negative trials_before, iterations < 1, a
    window the host phase refuses or one without a free keyframe."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import lba_system_ref as S
    capi = pkg.capi
    ba = capi.LocalBA()
    win = S.make_window(1, 2, 2, S.sees_counts(3))

    def refused(w, text=None, **kw):
        with pytest.raises(capi.AosError) as e:
            ba.debug_trial([win, w], **kw)
        assert e.value.code == capi.AOS2_ERR_ARG, (kw, str(e.value))
        assert text is None or text in str(e.value), str(e.value)

    for kw in (dict(layout=2), dict(layout=-1), dict(tail=3), dict(tail=-1), dict(trials_before=-1), dict(iters=(0, 10))):
        refused(win, **kw)
    ep = win["edge_pose"].copy()
    ep[3] = win["n_poses"]
    refused(dict(win, edge_pose=ep), "out of range")
    refused(dict(win, pose_fixed=np.ones(win["n_poses"], np.uint8)), "no free keyframe")
    f = capi.lib().aos2_debug_lba_trial_device
    S_, R_, O_ = (capi._LbaProblem * 1)(), (capi._LbaResult * 1)(), (capi._LbaTrial * 1)()
    keep = []
    ba._fill(S_[0], R_[0], win, None, (5, 10), keep)
    bufs = {k: np.zeros(4096, np.int32) for k in ("hpose", "hpoint", "pt_off", "pt_k", "pl_pos")}
    for k, a in bufs.items():
        setattr(O_[0], k, a.ctypes.data)
    assert f(None, C.byref(S_), 1, 0, 0, None, None, 0, C.byref(O_)) == capi.AOS2_ERR_ARG
    assert f(ba.h, None, 1, 0, 0, None, None, 0, C.byref(O_)) == capi.AOS2_ERR_ARG
    assert f(ba.h, C.byref(S_), 1, 0, 0, None, None, 0, None) == capi.AOS2_ERR_ARG
    assert f(ba.h, C.byref(S_), 0, 0, 0, None, None, 0, C.byref(O_)) == capi.AOS2_ERR_ARG
    for k in bufs:
        setattr(O_[0], k, None)
        assert f(ba.h, C.byref(S_), 1, 0, 0, None, None, 0, C.byref(O_)) == capi.AOS2_ERR_ARG, k
        setattr(O_[0], k, bufs[k].ctypes.data)
    for k in ("pose_Tcw", "edge_obs", "point_id"):
        old = getattr(S_[0], k)
        setattr(S_[0], k, None)
        assert f(ba.h, C.byref(S_), 1, 0, 0, None, None, 0, C.byref(O_)) == capi.AOS2_ERR_ARG, k
        setattr(S_[0], k, old)
    if pkg.device_count() == 0:   # good arguments get as far as the device (no snapshot array is required)
        with pytest.raises(capi.AosError) as e:
            ba.debug_trial([win], tail=2)
        assert e.value.code == capi.AOS2_ERR_NO_DEVICE


def test_pose_pass_tap_refuses_on_the_host(pkg):
    """aos2_debug_pose_pass_device checks its arguments before it looks for a device: a NULL (the case list, every array of a case), no
    cases, an unknown form or mode, n above the form's limit (1024, 2048, 1152; none for the form that leaves the edges in memory) or
    below 0, a round outside 0..3."""
    capi = pkg.capi
    p = pkg.synth.synth_pose_problem(1, n=40)
    good = dict(p, form=0, pose=pkg.synth.tcw_to_qt(p["Tcw"]))

    def refused(case, mode=1):
        with pytest.raises(capi.AosError) as e:
            capi.debug_pose_pass_device([good, case], mode)
        assert e.value.code == capi.AOS2_ERR_ARG, (mode, str(e.value))

    for mode in (-1, 3):
        refused(good, mode)
    for kw in (dict(form=-1), dict(form=4), dict(it=-1), dict(it=4)):
        refused(dict(good, **kw))
    for form, limit in ((0, 1024), (1, 2048), (2, 1152)):
        big = pkg.synth.synth_pose_problem(2, n=limit + 1)
        refused(dict(big, form=form, pose=good["pose"]))
    f = capi.lib().aos2_debug_pose_pass_device
    assert f(None, 1, 1, 0) == capi.AOS2_ERR_ARG
    S_ = (capi._PosePassCase * 1)()
    bufs = {k: np.zeros(256, np.float64) for k in ("Xw", "obs", "inv_sigma2", "stereo", "level1", "robust", "outlier", "chi2")}
    S_[0].n, S_[0].form, S_[0].it = 40, 0, 0
    S_[0].pose = (C.c_double * 7)(0, 0, 0, 1, 0, 0, 0)
    for k, a in bufs.items():
        setattr(S_[0], k, a.ctypes.data)
    assert f(C.byref(S_), 0, 1, 0) == capi.AOS2_ERR_ARG and f(C.byref(S_), -1, 1, 0) == capi.AOS2_ERR_ARG
    S_[0].n = -1
    assert f(C.byref(S_), 1, 1, 0) == capi.AOS2_ERR_ARG
    S_[0].n = 40
    for k in bufs:   # every array in turn
        setattr(S_[0], k, None)
        assert f(C.byref(S_), 1, 1, 0) == capi.AOS2_ERR_ARG, k
        setattr(S_[0], k, bufs[k].ctypes.data)
    if pkg.device_count() == 0:   # good arguments get as far as the device
        for form, n in ((0, 1024), (1, 2048), (2, 1152), (3, 5000)):
            big = pkg.synth.synth_pose_problem(2, n=n)
            with pytest.raises(capi.AosError) as e:
                capi.debug_pose_pass_device([dict(big, form=form, pose=good["pose"])], 1)
            assert e.value.code == capi.AOS2_ERR_NO_DEVICE
        assert f(C.byref(S_), 1, 1, 0) == capi.AOS2_ERR_NO_DEVICE
