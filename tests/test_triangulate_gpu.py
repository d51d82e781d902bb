"""aos2_frames_triangulate_matches / aos2_triangulate_matches / host/NewMapPoints.h on the GPU against tests/triangulation_ref.py:
status equal, x3D bit for bit wherever it is defined.  The frames are built with aos2_frames_build_stereo from crafted keypoint
records, mvuRight and mvDepth, so the geometry is the generator's (tests/test_triangulate_cpu.py asserts what its seeds cover)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import triangulation_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 2


class Batch:
    """a keyframe batch on the device built from OBS records: frames `which` of a scene, all with camera `cam`"""

    def __init__(self, pkg, S, which, cam, cap, n=None):
        import torch
        self.t, dev = torch, torch.device("cuda", 0)
        B = len(which)
        self.kfs = [S["kfs"][f] for f in which]
        self.obs = np.zeros((B, cap), R.OBS)
        self.n = np.array([S["n"][f] for f in which] if n is None else n, np.int32)
        kps = np.zeros((B, cap, 7), np.float32)
        for j, f in enumerate(which):
            nf = len(S["obs"][f])
            self.obs[j, :nf] = S["obs"][f]
            kps[j, :nf, 0], kps[j, :nf, 1] = S["obs"][f]["kx"], S["obs"][f]["ky"]
            kps[j, :nf, 5] = S["obs"][f]["octave"].astype(np.int32).view(np.float32)
        self.ex = pkg.capi.Extractor(nfeatures=1000, device=0)
        assert (self.ex.GetScaleFactors() == S["sf"]).all()
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
        self.d = [up(kps), torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev), up(self.n), up(self.obs["u_right"]), up(self.obs["depth"]),
                  up(np.stack([k["Tcw"].reshape(16) for k in self.kfs]))]
        torch.cuda.synchronize()
        self.fr = pkg.capi.Frames(B, cap, 0)
        self.fr.build_stereo(self.ex, self.d[0].data_ptr(), self.d[1].data_ptr(), self.d[2].data_ptr(), cam["w"], cam["h"], self.d[3].data_ptr(),
                             self.d[4].data_ptr(), cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"])
        self.fr.set_pose(self.d[5].data_ptr())
        self.fr.wait()
        self.B, self.cap = B, cap

    def triangulate(self, other, kf1, kf2, match12, first_wins):
        torch = self.t
        P = len(kf1)
        m = np.full((P, self.cap), -1, np.int32)
        m[:, : match12.shape[1]] = match12
        d_m = torch.from_numpy(m).to("cuda:0")
        x = torch.full((P, self.cap, 3), 7.0, dtype=torch.float32, device="cuda:0")
        st = torch.full((P, self.cap), 99, dtype=torch.uint8, device="cuda:0")
        nn = torch.full((P,), -5, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        self.fr.TriangulateMatches(other.fr, kf1, kf2, d_m.data_ptr(), x.data_ptr(), st.data_ptr(), nn.data_ptr(), first_wins=first_wins)
        self.fr.wait()
        return st.cpu().numpy(), x.cpu().numpy(), nn.cpu().numpy(), m


def reference(a, b, kf1, kf2, m, first_wins):
    return R.triangulate_frames(a.kfs, a.obs, a.n, b.kfs, b.obs, b.n, kf1, kf2, m, first_wins)


def same(got, want):
    """status and the count exactly; x3D bit for bit (zeros where it is undefined, on both sides)"""
    return (got[0] == want[0]).all() and (got[1].view(np.uint32) == want[1].view(np.uint32)).all() and (got[2] == want[2]).all()


@pytest.fixture(scope="module")
def world(pkg, gpu):
    """the generator's scene of SEED as one batch of 4 frames, cap = 100 (a partial wave: 96 features)"""
    c = R.generator_case(SEED)
    return c, Batch(pkg, c["scene"], (0, 1, 2, 3), R.CAM_A, cap=100)


def test_generator_pairs_with_and_without_first_wins(world):
    c, a = world
    pad = lambda s: np.pad(s, [(0, 0), (0, a.cap - s.shape[1])] + [(0, 0)] * (s.ndim - 2))   # noqa: E731
    got = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], True)
    assert same(got, (pad(c["status"]), pad(c["x3D"]), c["nnew"]))
    assert (got[0] == R.SUPERSEDED).sum() >= 3 and (got[2] > 0).all()
    got = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], False)
    assert same(got, (pad(c["status_all"]), pad(c["x3D"]), c["nnew_all"]))
    # the groups follow kf1, not the position in the call: the same pairs interleaved
    order = np.array([3, 0, 4, 1, 5, 2])
    got = a.triangulate(a, c["kf1"][order], c["kf2"][order], c["match12"][order], True)
    assert same(got, (pad(c["status"])[order], pad(c["x3D"])[order], c["nnew"][order]))


def test_two_batches_with_different_cameras(pkg, gpu):
    c = R.generator_case(SEED, "mixed")
    S = c["scene"]
    a, b = Batch(pkg, S, (0, 2), R.CAM_A, cap=100), Batch(pkg, S, (1, 3), R.CAM_B, cap=128)
    kf1, kf2 = np.array([0, 0, 1, 1], np.int32), np.array([0, 1, 0, 1], np.int32)
    m = R.matches(SEED + 50, 96, range(4))
    got = a.triangulate(b, kf1, kf2, m, True)
    want = reference(a, b, kf1, kf2, got[3], True)
    assert same(got, want)
    assert (want[0] == R.ACCEPTED).sum() >= 10 and (want[0] == R.REPROJ2).sum() >= 3


def test_shapes_that_stress_the_compaction_and_the_grid(pkg, gpu):
    S = R.scene(SEED + 1, n_feat=280)
    n = np.array([280, 280, 0, 257], np.int32)   # a frame without features; one that ends one lane into the second workgroup
    a = Batch(pkg, S, (0, 1, 2, 3), R.CAM_A, cap=300, n=n)
    kf1 = np.array([0, 0, 1, 2, 0, 3], np.int32)
    kf2 = np.array([1, 3, 0, 1, 2, 1], np.int32)
    m = R.matches(SEED + 1, 280, range(6))
    m[0] = np.arange(280)   # every feature matched: each workgroup's list is as long as it gets
    m[2] = -1               # no match at all
    got = a.triangulate(a, kf1, kf2, m, True)
    want = reference(a, a, kf1, kf2, got[3], True)
    assert same(got, want)
    assert (want[0][0, :280] != R.NO_MATCH).all() and (want[0][0] == R.ACCEPTED).sum() > 64
    assert (want[0][2:5] == R.NO_MATCH).all() and (want[2][2:5] == 0).all()      # all -1; keyframe 1 empty; keyframe 2 empty
    assert (want[0][1, :280] == R.NO_MATCH).sum() > (m[1] < 0).sum()              # partners beyond keyframe 2's 257 features
    assert (want[0][5, 257:] == R.NO_MATCH).all()
    # one pair
    got1 = a.triangulate(a, kf1[:1], kf2[:1], m[:1], False)
    assert same(got1, reference(a, a, kf1[:1], kf2[:1], got1[3], False))


def test_host_pointer_call_and_shim_equal_the_device_resident_call(pkg, world, tmp_path):
    c, a = world
    S = c["scene"]
    dev = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], False)
    M = pkg.capi.Matcher(0.6, False, device=0)
    for p, (f1, f2) in enumerate(R.PAIRS6):
        idx = np.flatnonzero(c["match12"][p] >= 0)
        st, x = M.TriangulateMatches(S["kfs"][f1], S["kfs"][f2], S["obs"][f1][idx], S["obs"][f2][c["match12"][p][idx]])
        assert (st == dev[0][p][idx]).all() and (x.view(np.uint32) == dev[1][p][idx].view(np.uint32)).all()
    # more than one workgroup, mvKeys != mvKeysUn
    S2 = R.scene(SEED, n_feat=300, distort_keys=True)
    st, x = M.TriangulateMatches(S2["kfs"][0], S2["kfs"][3], S2["obs"][0], S2["obs"][3])
    want = R.triangulate_matches(S2["kfs"][0], S2["kfs"][3], S2["obs"][0], S2["obs"][3])
    assert (st == want[0]).all() and (x.view(np.uint32) == want[1].view(np.uint32)).all()
    assert (st == R.ACCEPTED).sum() > 20 and len(np.unique(st)) >= 5
    # the shim at the reference's call site
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "new_map_points_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS", os.path.join(ROOT, "tests", "cpp", "new_map_points_test.cpp"),
                           "-o", exe, "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    p, (f1, f2) = 2, R.PAIRS6[2]
    idx = np.flatnonzero(c["match12"][p] >= 0)
    arrays = {"matches": np.stack([idx, c["match12"][p][idx]], 1).astype(np.int32)}
    for tag, f in (("kf1_", f1), ("kf2_", f2)):
        K, o = S["kfs"][f], S["obs"][f]
        arrays[tag + "Tcw"] = K["Tcw"].reshape(16)
        arrays[tag + "cam"] = np.array([K[k] for k in ("fx", "fy", "cx", "cy", "mb", "mbf")], np.float32)
        arrays[tag + "sf"] = K["scale_factors"]
        arrays[tag + "obs"] = np.stack([o[k] for k in ("ux", "uy", "kx", "ky", "u_right", "depth")], 1).astype(np.float32)
        arrays[tag + "octave"] = o["octave"].astype(np.int32)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    assert (out["status"] == dev[0][p][idx]).all() and (out["x3D"].view(np.uint32) == dev[1][p][idx].view(np.uint32)).all()
    defined = ~np.isin(out["status"], (R.NO_MATCH, R.LOW_PARALLAX, R.W_ZERO))
    assert (out["has_x3D"].astype(bool) == defined).all() and defined.sum() > 10 and (~defined).sum() >= 3


def test_repeatable_and_the_asynchronous_form_equals_the_synchronous(world):
    c, a = world
    first = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], True)
    again = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], True)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first[:3], again[:3]))
    a.fr.set_async_keyframe_calls(True)
    try:
        for _ in range(2):   # (the second call finds the staging buffer of the first in use)
            asy = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], True)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first[:3], asy[:3]))
    finally:
        a.fr.set_async_keyframe_calls(False)


def test_asynchronous_staging_grows_behind_a_call_in_flight(pkg, world):
    """Asynchronous keyframe calls on a handle whose staging holds nothing yet: 2 pairs, then all 6 without a wait in between -- the
    second call has to grow the page-locked and the device staging buffer while the upload and the kernels of the first may still be
    in flight -- then one wait.  Both calls give the synchronous call's bytes."""
    c, a = world
    want6 = a.triangulate(a, c["kf1"], c["kf2"], c["match12"], True)
    want2 = a.triangulate(a, c["kf1"][:2], c["kf2"][:2], c["match12"][:2], True)
    b = Batch(pkg, c["scene"], (0, 1, 2, 3), R.CAM_A, cap=100)   # (the world's own handle has staged 6 pairs before)
    torch = b.t

    def buffers(P):
        m = np.full((P, b.cap), -1, np.int32)
        m[:, : c["match12"].shape[1]] = c["match12"][:P]
        return (torch.from_numpy(m).to("cuda:0"), torch.full((P, b.cap, 3), 7.0, dtype=torch.float32, device="cuda:0"),
                torch.full((P, b.cap), 99, dtype=torch.uint8, device="cuda:0"), torch.full((P,), -5, dtype=torch.int32, device="cuda:0"))

    o2, o6 = buffers(2), buffers(6)
    torch.cuda.synchronize()
    b.fr.set_async_keyframe_calls(True)
    for P, (d_m, x, st, nn) in ((2, o2), (6, o6)):
        b.fr.TriangulateMatches(b.fr, c["kf1"][:P], c["kf2"][:P], d_m.data_ptr(), x.data_ptr(), st.data_ptr(), nn.data_ptr(), first_wins=True)
    b.fr.wait()
    for want, (d_m, x, st, nn) in ((want2, o2), (want6, o6)):
        got = (st.cpu().numpy(), x.cpu().numpy(), nn.cpu().numpy())
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want[:3]))
    assert (want6[0] == R.ACCEPTED).sum() > (want2[0] == R.ACCEPTED).sum() > 0


def test_bad_pairs_are_rejected_before_anything_runs(pkg, world):
    c, a = world
    torch = a.t
    st = torch.full((1, a.cap), 99, dtype=torch.uint8, device="cuda:0")
    x = torch.zeros((1, a.cap, 3), dtype=torch.float32, device="cuda:0")
    nn = torch.full((1,), -5, dtype=torch.int32, device="cuda:0")
    m = torch.full((1, a.cap), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for kf1, kf2 in (([0], [4]), ([-1], [0]), ([10 ** 6], [0]), ([], [])):
        with pytest.raises(pkg.AosError) as e:
            a.fr.TriangulateMatches(a.fr, kf1, kf2, m.data_ptr(), x.data_ptr(), st.data_ptr(), nn.data_ptr())
        assert e.value.code == pkg.capi.AOS2_ERR_ARG
    with pytest.raises(pkg.AosError):
        a.fr.TriangulateMatches(a.fr, [0], [1], 0, x.data_ptr(), st.data_ptr(), nn.data_ptr())
    a.fr.wait()
    assert (st.cpu().numpy() == 99).all() and int(nn.cpu()[0]) == -5


def test_on_the_real_chain_after_the_keyframe_work(pkg, gpu):
    """KeyFrameWork.triangulate() after run(): the matches SearchForTriangulation left on the device, triangulated there, equal the
    reference evaluated on the members read back from the device; map points are born"""
    F = pkg.capi.Frames
    scen = pkg.scenario.tracking_scenario(31, 6, n_unique=3)
    tc = pkg.chain.TrackingChain(scen, n_local=800)
    voc = pkg.synth.synth_vocabulary(402, 10, 4)
    kw = pkg.chain.KeyFrameWork(tc, voc, n_kf=5, n_nb=4).run()
    kw.triangulate()
    sf = tc.ex.GetScaleFactors()

    def members(fr, d_kps, d_n):
        kps, n = d_kps.cpu().numpy(), d_n.cpu().numpy()
        T = fr.get(F.TCW)
        obs = np.zeros(kps.shape[:2], R.OBS)
        obs["ux"], obs["uy"], obs["u_right"], obs["depth"] = fr.get(F.KEYS_UN_X), fr.get(F.KEYS_UN_Y), fr.get(F.U_RIGHT), fr.get(F.DEPTH)
        obs["kx"], obs["ky"] = kps[:, :, 0], kps[:, :, 1]
        obs["octave"] = np.ascontiguousarray(kps[:, :, 5]).view(np.int32)
        kfs = [R.keyframe(T[b], scen["fx"], scen["fy"], scen["cx"], scen["cy"], scen["mbf"], sf) for b in range(len(T))]
        return kfs, obs, n

    k1, o1, n1 = members(tc.last, tc.dl_kps, tc.dl_n)
    k2, o2, n2 = members(kw.kfs, kw.n_kps, kw.n_n)
    want = R.triangulate_frames(k1, o1, n1, k2, o2, n2, kw.t_kf1, kw.t_kf2, kw.match12, True)
    assert same((kw.tri_status, kw.x3D, kw.nnew), want)
    assert (kw.nnew > 0).any() and ((kw.match12 >= 0) == (kw.tri_status != R.NO_MATCH)).all()
    print("nnew per pair", kw.nnew.tolist(), "statuses", np.bincount(kw.tri_status.ravel(), minlength=11).tolist())
