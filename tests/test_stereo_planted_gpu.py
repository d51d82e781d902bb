"""The stereo kernels of csrc/stereo.hip alone, on planted worlds (tests/stereo_ref.py): hand-built keypoints that sit on
every decision of Frame::ComputeStereoMatches (src/Frame.cc:495-669), through every form of the call, byte for byte
against the numpy restatement run on the device's own pyramid planes and against the oracle; and the refusal of keypoint
records whose windows would leave the planes.  test_stereo_cpu.py shows that the worlds hold what they claim."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SENTINEL = np.float32(-77.0)
_CACHE = {}

SMALL = ("gates16", "median_odd", "maxd", "median_even", "nomatch", "median_zeros", "nright1", "median_tied", "median_two",
         "median_one")                      # the 320 x 240 worlds; gates16 (16 left, 16 right) sets the capacity of a batch


def _world(name):
    if "worlds" not in _CACHE:
        _CACHE["worlds"] = R.build_worlds()
    return _CACHE["worlds"][name]


def _want(oracle, name):
    """the world's arrays and the oracle's outputs, computed once"""
    if name not in _CACHE:
        W = _world(name)
        eL, eR, _, _, nat = R.oracle_side(oracle, W)
        arrays = nat if name == "levels" else W.arrays()
        assert R.in_domain(arrays[0], arrays[2], W.sizes(), R.INV_SCALE) == (True, ""), name
        _CACHE[name] = (arrays, oracle.compute_stereo_matches(eL, eR, *arrays, W.mb, W.mbf)[:2], (eL, eR))
    return _CACHE[name]


def _planes(x, image=0):
    return [x.pyramid_level(l, image=image) for l in range(R.NLEVELS)]


def _restated(W, arrays, xl, xr, image=0):
    assert R.in_domain(arrays[0], arrays[2], W.sizes(), R.INV_SCALE) == (True, "")
    return R.compute(*arrays, W.mb, W.mbf, xl.GetScaleFactors(), xl.GetInverseScaleFactors(), _planes(xl, image), _planes(xr, image))


def _same(got, want, what):
    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), what


@pytest.mark.parametrize("name", sorted(R.build_worlds()))
def test_planted_world_host_form(pkg, oracle, gpu, name):
    W = _world(name)
    arrays, want_oracle, _ = _want(oracle, name)
    xl, xr = pkg.Extractor(nfeatures=W.nfeatures), pkg.Extractor(nfeatures=W.nfeatures)
    gkl, gdl = xl(W.left)
    gkr, gdr = xr(W.right)
    if name == "levels":                     # the extractor's own keypoints: the device's are the oracle's
        assert gkl.tobytes() == arrays[0].tobytes() and gdr.tobytes() == arrays[3].tobytes()
    assert np.array_equal(xl.pyramid_level(0), W.left) and np.array_equal(xr.pyramid_level(0), W.right)
    ur, dp, tr = _restated(W, arrays, xl, xr)
    R.check_expectations(W, tr)
    got = pkg.ComputeStereoMatches(xl, xr, *arrays, W.mb, W.mbf)
    bad = np.flatnonzero(got[0] != ur)
    assert got[0].tobytes() == ur.tobytes() and got[1].tobytes() == dp.tobytes(), \
        (name, [(W.tags[i] if W.tags else i, R.REASONS[tr["reason"][i]], float(got[0][i]), float(ur[i])) for i in bad[:8]])
    _same(got, want_oracle, name)


def test_prefixes_of_the_pixels_world(pkg, oracle, gpu):
    """n_left on both sides of the 4 left keypoints of a workgroup and of the 256 threads the cull strides by"""
    W = _world("pixels")
    (kl, dl, kr, dr), _, (eL, eR) = _want(oracle, "pixels")
    xl, xr = pkg.Extractor(nfeatures=W.nfeatures), pkg.Extractor(nfeatures=W.nfeatures)
    xl(W.left)
    xr(W.right)
    pl, pr = _planes(xl), _planes(xr)
    for n in R.N_LEFT_PREFIXES:
        ur, dp, tr = R.compute(kl[:n], dl[:n], kr, dr, W.mb, W.mbf, R.SCALE, R.INV_SCALE, pl, pr)
        assert tr["n_before_cull"] == n
        got = pkg.ComputeStereoMatches(xl, xr, kl[:n], dl[:n], kr, dr, W.mb, W.mbf)
        _same(got, (ur, dp), n)
        _same(got, oracle.compute_stereo_matches(eL, eR, kl[:n], dl[:n], kr, dr, W.mb, W.mbf), n)


def _batch_case(B):
    """B small worlds, a different one per image, as [B][cap] arrays: image 0 has n_left = cap; with B >= 3 image 1 has
    n_left = 0 and image 2 has n_right = 0"""
    names = SMALL[:B]
    cases = []
    for b, name in enumerate(names):
        W = _world(name)
        kl, dl, kr, dr = W.arrays()
        if B >= 3 and b == 1:
            kl, dl = kl[:0], dl[:0]
        if B >= 3 and b == 2:
            kr, dr = kr[:0], dr[:0]
        cases.append((W, (kl, dl, kr, dr)))
    cap = 16
    assert len(cases[0][1][0]) == cap and all(len(a[0]) <= cap and len(a[2]) <= cap for _, a in cases)
    assert len({W.mbf for W, _ in cases}) > 1 or B == 1          # mb / mbf are per call: the batch is run once per value
    return cases, cap


def _run_batch(pkg, torch, cases, cap, form):
    """-> per image (u_right[:cap], depth[:cap]) from the device-resident form, planes read back for the restatement"""
    B, dev = len(cases), torch.device("cuda:0")
    h, w = cases[0][0].left.shape
    L = torch.from_numpy(np.stack([W.left for W, _ in cases])).to(dev)
    Rt = torch.from_numpy(np.stack([W.right for W, _ in cases])).to(dev)
    xl, xr = pkg.Extractor(nfeatures=500), pkg.Extractor(nfeatures=500)
    xcap = xl.max_keypoints_for(w, h)
    scratch = [(torch.zeros((B, xcap, 28), dtype=torch.uint8, device=dev), torch.zeros((B, xcap, 32), dtype=torch.uint8, device=dev),
                torch.zeros(B, dtype=torch.int32, device=dev)) for _ in range(2)]
    kp = [np.zeros((B, cap), R.KP_DTYPE) for _ in range(2)]
    ds = [np.zeros((B, cap, 32), np.uint8) for _ in range(2)]
    n = [np.zeros(B, np.int32) for _ in range(2)]
    for b, (W, (kl, dl, kr, dr)) in enumerate(cases):
        assert R.in_domain(kl, kr, W.sizes(), R.INV_SCALE) == (True, "")      # nothing else may reach a device-resident form
        kp[0][b, :len(kl)], ds[0][b, :len(kl)], n[0][b] = kl, dl, len(kl)
        kp[1][b, :len(kr)], ds[1][b, :len(kr)], n[1][b] = kr, dr, len(kr)
    dkp = [torch.from_numpy(a.view(np.uint8).reshape(B, cap, 28)).to(dev) for a in kp]
    dds = [torch.from_numpy(a).to(dev) for a in ds]
    dn = [torch.from_numpy(a).to(dev) for a in n]
    torch.cuda.synchronize()
    out = {}
    extract = "extract_batch_device_async" if form == "async" else "extract_batch_device"
    for x, imgs, (k, d, c) in ((xl, L, scratch[0]), (xr, Rt, scratch[1])):
        getattr(x, extract)(imgs.data_ptr(), B, w, h, w, w * h, k.data_ptr(), d.data_ptr(), xcap, c.data_ptr())
    for mbf in sorted({float(W.mbf) for W, _ in cases}):
        ur = torch.full((B, cap), float(SENTINEL), dtype=torch.float32, device=dev)
        dp = torch.full((B, cap), float(SENTINEL), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        args = (xl, xr, B, dkp[0].data_ptr(), dds[0].data_ptr(), dn[0].data_ptr(), dkp[1].data_ptr(), dds[1].data_ptr(),
                dn[1].data_ptr(), cap, np.float32(0.5), np.float32(mbf), ur.data_ptr(), dp.data_ptr())
        if form == "async":
            pkg.capi.compute_stereo_matches_device_async(*args)
            xl.wait()
        else:
            assert pkg.capi.compute_stereo_matches_device(*args) > 0
        torch.cuda.synchronize()
        out[mbf] = (ur.cpu().numpy(), dp.cpu().numpy())
    xr.wait()
    return out, xl, xr


@pytest.mark.parametrize("B", [1, 3, 9])
def test_device_batch(pkg, oracle, gpu, B):
    """[batch][cap] device arrays through compute_stereo_matches_device (the grid is padded to 8 images), each image compared
    with the restatement on that image's planes and with the oracle; the asynchronous form, enqueued behind two extractions
    still in flight, gives the same bytes"""
    import torch
    cases, cap = _batch_case(B)
    out, xl, xr = _run_batch(pkg, torch, cases, cap, "sync")
    for b, (W, arrays) in enumerate(cases):
        assert W.mb == np.float32(0.5)
        ur, dp = out[float(W.mbf)]
        nl = len(arrays[0])
        want = _restated(W, arrays, xl, xr, image=b)
        _same((ur[b, :nl], dp[b, :nl]), want[:2], (B, b, W.name))
        assert (ur[b, nl:] == SENTINEL).all() and (dp[b, nl:] == SENTINEL).all()      # nothing written past n_left
        eL, eR = _want(oracle, W.name)[2]
        _same((ur[b, :nl], dp[b, :nl]), oracle.compute_stereo_matches(eL, eR, *arrays, W.mb, W.mbf)[:2], (B, b, W.name))
        if nl and len(arrays[2]) == 0:
            assert (ur[b, :nl] == -1).all()
    if B == 3:
        out2, xl2, xr2 = _run_batch(pkg, torch, cases, cap, "async")
        for k in out:
            assert out2[k][0].tobytes() == out[k][0].tobytes() and out2[k][1].tobytes() == out[k][1].tobytes()


def test_host_form_on_image_2_of_3(pkg, oracle, gpu):
    names = ("median_odd", "nomatch", "gates16")
    xl, xr = pkg.Extractor(nfeatures=500), pkg.Extractor(nfeatures=500)
    xl.extract_batch(np.stack([_world(n).left for n in names]))
    xr.extract_batch(np.stack([_world(n).right for n in names]))
    W = _world(names[2])
    arrays, want_oracle, _ = _want(oracle, names[2])
    assert np.array_equal(xl.pyramid_level(0, image=2), W.left)
    got = pkg.ComputeStereoMatches(xl, xr, *arrays, W.mb, W.mbf, image=2)
    _same(got, _restated(W, arrays, xl, xr, image=2)[:2], "image 2")
    _same(got, want_oracle, "image 2")
    assert got[0].tobytes() != pkg.ComputeStereoMatches(xl, xr, *arrays, W.mb, W.mbf, image=0)[0].tobytes()


def _raw_call(pkg, xl, xr, kl, dl, kr, dr, mb, mbf):
    """aos2_compute_stereo_matches with outputs this test owns -> (status, u_right, depth)"""
    kl, kr = np.ascontiguousarray(kl, pkg.capi.KP_DTYPE), np.ascontiguousarray(kr, pkg.capi.KP_DTYPE)
    dl, dr = np.ascontiguousarray(dl, np.uint8), np.ascontiguousarray(dr, np.uint8)
    ur, dp = np.full(len(kl), SENTINEL, np.float32), np.full(len(kl), SENTINEL, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    st = xl.L.aos2_compute_stereo_matches(xl.h, xr.h, 0, p(kl), p(dl), len(kl), p(kr), p(dr), len(kr), np.float32(mb),
                                          np.float32(mbf), p(ur), p(dp))
    return st, ur, dp


OUTSIDE = [  # (side, field, value): one record of the world moved out of the domain
    ("left", "x", 4.4), ("left", "x", 320 - 5.4), ("left", "y", 4.4), ("left", "y", 240 - 5.4), ("left", "x", -20.0),
    ("left", "octave", 8), ("left", "octave", -1), ("left", "octave", 1 << 20), ("left", "x", np.nan), ("left", "y", np.inf),
    ("left", "x", 1e30), ("right", "x", 9.4), ("right", "x", 0.0), ("right", "x", 11.3), ("right", "octave", 8),
    ("right", "octave", -1), ("right", "y", np.nan), ("right", "y", -np.inf),
]


def test_out_of_domain_records_are_refused(pkg, oracle, gpu):
    """the host-pointer form returns AOS2_ERR_ARG before anything is uploaded: outputs untouched, the handle as good as before.
    (Only this form is given such records: it returns before any GPU work.)"""
    W = _world("gates16")
    (kl, dl, kr, dr), want, _ = _want(oracle, "gates16")
    xl, xr = pkg.Extractor(nfeatures=500), pkg.Extractor(nfeatures=500)
    xl(W.left)
    xr(W.right)
    for side, field, value in OUTSIDE:
        for at in (0, len(kl) - 1):
            a, b = kl.copy(), kr.copy()
            (a if side == "left" else b)[field][at] = value
            assert not R.in_domain(a, b, W.sizes(), R.INV_SCALE)[0], (side, field, value)
            st, ur, dp = _raw_call(pkg, xl, xr, a, dl, b, dr, W.mb, W.mbf)
            assert st == pkg.capi.AOS2_ERR_ARG, (side, field, value, st)
            assert (ur == SENTINEL).all() and (dp == SENTINEL).all()
            assert b"keypoint" in xl.L.aos2_last_error()
    # a bad right record is refused even when there is no left keypoint to match
    b = kr.copy()
    b["octave"][0] = 99
    assert _raw_call(pkg, xl, xr, kl[:0], dl[:0], b, dr, W.mb, W.mbf)[0] == pkg.capi.AOS2_ERR_ARG
    # records on the edge of the domain pass, and the handles still give the world's bytes
    st, ur, dp = _raw_call(pkg, xl, xr, kl, dl, kr, dr, W.mb, W.mbf)
    assert st == 0 and ur.tobytes() == want[0].tobytes() and dp.tobytes() == want[1].tobytes()


def test_capacity_refusal_leaves_the_handle_usable(pkg, oracle, gpu):
    """15361 left keypoints (the cull keeps one int per left keypoint in LDS, 15360 fit) -> AOS2_ERR_CAPACITY before a launch.
    (The other capacity refusal of launch_stereo, more than 12000 rows, cannot be reached: the extractor takes no image
    taller than 4000.)"""
    W = _world("median_odd")
    (kl, dl, kr, dr), want, _ = _want(oracle, "median_odd")
    xl, xr = pkg.Extractor(nfeatures=500), pkg.Extractor(nfeatures=500)
    xl(W.left)
    xr(W.right)
    n = 15361
    big_k, big_d = np.resize(kl, n), np.resize(dl, (n, 32))
    assert R.in_domain(big_k, kr, W.sizes(), R.INV_SCALE)[0]
    st, ur, dp = _raw_call(pkg, xl, xr, big_k, big_d, kr, dr, W.mb, W.mbf)
    assert st == pkg.capi.AOS2_ERR_CAPACITY and (ur == SENTINEL).all() and (dp == SENTINEL).all()
    _same(pkg.ComputeStereoMatches(xl, xr, kl, dl, kr, dr, W.mb, W.mbf), want, "after the refusal")
