"""Frame::ComputeStereoMatches (src/Frame.cc:495-669) without a GPU: the numpy restatement of tests/stereo_ref.py against
independent knowledge and against the oracle's C restatement, byte for byte, on every planted world and on natural pairs;
the floors that keep the planted GPU tests from being vacuous; the domain rule of include/aos2.h."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stereo_ref as R  # noqa: E402

_CACHE = {}


def _worlds():
    if "worlds" not in _CACHE:
        _CACHE["worlds"] = R.build_worlds()
    return _CACHE["worlds"]


def _run(oracle, name, natural=False):
    """(world, arrays, trace, restatement outputs, oracle outputs, planes) of one world, computed once"""
    key = (name, natural)
    if key not in _CACHE:
        W = _worlds()[name]
        eL, eR, pl, pr, nat = R.oracle_side(oracle, W)
        kl, dl, kr, dr = nat if natural else W.arrays()
        ok, why = R.in_domain(kl, kr, W.sizes(), R.INV_SCALE)
        assert ok, (name, why)                      # before anything reads a plane
        ur, dp, tr = R.compute(kl, dl, kr, dr, W.mb, W.mbf, R.SCALE, R.INV_SCALE, pl, pr)
        our, odp, on = oracle.compute_stereo_matches(eL, eR, kl, dl, kr, dr, W.mb, W.mbf)
        _CACHE[key] = dict(W=W, kl=kl, dl=dl, kr=kr, dr=dr, tr=tr, ur=ur, dp=dp, our=our, odp=odp, on=on, pl=pl, pr=pr)
    return _CACHE[key]


WORLD_NAMES = sorted(R.build_worlds())
PLANTED = [n for n in WORLD_NAMES if n != "levels"]


def test_worlds_are_reproducible_and_level0_is_the_image(oracle):
    a, b = R.build_worlds(), R.build_worlds()
    for name in WORLD_NAMES:
        assert a[name].right.tobytes() == b[name].right.tobytes() and a[name].left.max() <= 234
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a[name].arrays(), b[name].arrays()))
    r = _run(oracle, "median_odd")
    assert np.array_equal(r["pl"][0], r["W"].left) and np.array_equal(r["pr"][0], r["W"].right)


@pytest.mark.parametrize("name", WORLD_NAMES)
def test_restatement_equals_oracle_on_worlds(oracle, name):
    for natural in (False, True):
        r = _run(oracle, name, natural)
        assert r["ur"].tobytes() == r["our"].tobytes() and r["dp"].tobytes() == r["odp"].tobytes()
        assert r["on"] == r["tr"]["n_before_cull"]
        if not natural:
            R.check_expectations(r["W"], r["tr"])


@pytest.mark.parametrize("w,h,nf,seed", [(320, 240, 500, 3), (1241, 376, 2000, 4)])
def test_restatement_equals_oracle_on_natural_pairs(pkg, oracle, w, h, nf, seed):
    left, right, _ = pkg.synth.synth_stereo_pair(seed, w, h, max_disp=48)
    eL, eR = oracle.Extractor(nfeatures=nf), oracle.Extractor(nfeatures=nf)
    kl, dl = eL.extract(left)
    kr, dr = eR.extract(right)
    sizes = [eL.level_size(l)[:2] for l in range(R.NLEVELS)]
    assert sizes == R.level_sizes(w, h) and R.in_domain(kl, kr, sizes, R.INV_SCALE)[0]
    pl, pr = [eL.level_plane(l) for l in range(R.NLEVELS)], [eR.level_plane(l) for l in range(R.NLEVELS)]
    mb, mbf = np.float32(0.5), np.float32(40.0)
    ur, dp, tr = R.compute(kl, dl, kr, dr, mb, mbf, eL.scale_factors, eL.inv_scale_factors, pl, pr)
    our, odp, on = oracle.compute_stereo_matches(eL, eR, kl, dl, kr, dr, mb, mbf)
    assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes() and on == tr["n_before_cull"]
    acc = np.isin(tr["reason"], (R.ACCEPTED, R.ACCEPTED_ZERO_DISPARITY))
    print(f"{w}x{h}: {R.reason_counts(tr)}; accepted per level {[int((acc & (kl['octave'] == l)).sum()) for l in range(8)]}")
    assert acc.sum() > 100 and all((acc & (kl["octave"] == l)).any() for l in range(R.NLEVELS))


@pytest.mark.parametrize("name,natural", [("hamming", False), ("gates80", False), ("pixels", False), ("levels", True)])
def test_restatement_against_independent_knowledge(oracle, name, natural):
    """np.unpackbits for the Hamming distance, an int64 abs().sum() per offset, np.sort for the median, the vertex of
    np.polyfit through the three sums, and the outputs recomputed from those in double"""
    r = _run(oracle, name, natural)
    W, tr, kl, kr = r["W"], r["tr"], r["kl"], r["kr"]
    reached = np.flatnonzero(tr["best_idx"] >= 0)
    assert len(reached) > 20
    sad = []
    for i in reached:
        j = tr["best_idx"][i]
        assert tr["hamming"][i] == int((np.unpackbits(r["dl"][i]) != np.unpackbits(r["dr"][j])).sum()) < 75
        if tr["reason"][i] == R.WINDOW_OUT:
            continue
        lv = int(kl["octave"][i])
        s = float(R.SCALE[lv])
        # the window centres take the float product as it is: a level-0 x of 3 mod 6 is k + 0.5 at level 1 in exact arithmetic,
        # and which way it goes is decided by the rounding of x * (1 / 1.2f) to float, so a double cannot second-guess it
        cu, cv, cr = (int(np.trunc(float(np.float32(v) * R.INV_SCALE[lv]) + 0.5))
                      for v in (kl["x"][i], kl["y"][i], kr["x"][j]))
        PL, PR = r["pl"][lv].astype(np.int64), r["pr"][lv].astype(np.int64)
        a = PL[cv - 5:cv + 6, cu - 5:cu + 6] - PL[cv, cu]
        sums = [int(np.abs(a - (PR[cv - 5:cv + 6, cr + o - 5:cr + o + 6] - PR[cv, cr + o])).sum()) for o in range(-5, 6)]
        assert sums == tr["sums"][i].tolist()
        b = int(np.argmin(sums))                                  # first minimum
        assert b - 5 == tr["best_inc"][i] and sums[b] == tr["best_sum"][i]
        if 0 < b < 10:
            c2, c1, _ = np.polyfit([-1.0, 0.0, 1.0], sums[b - 1:b + 2], 2)
            vertex = -c1 / (2 * c2)
            assert abs(vertex) <= 0.5 and abs(vertex - float(tr["delta"][i])) < 1e-6
            if tr["reason"][i] in (R.ACCEPTED, R.CULLED):
                sad.append(sums[b])
                u = s * (cr + b - 5 + vertex)
                if tr["reason"][i] == R.ACCEPTED:
                    # float: (cr + inc) + deltaR, the product with the scale and bestuR itself each round once, by at most
                    # half a step of a value no larger than u: 3 * 2^-23 u bounds the error of bestuR and of the disparity
                    err, disp = 3 * 2.0 ** -23 * u, float(kl["x"][i]) - u
                    assert abs(u - float(r["ur"][i])) <= err
                    if disp > 8 * err:       # (below that the float disparity has no digit a double could confirm)
                        assert abs(float(W.mbf) / disp - float(r["dp"][i])) <= (err / (disp - err) + 1e-6) * float(r["dp"][i])
    if sad:
        median = np.sort(np.array(sad))[len(sad) // 2]
        assert median == tr["median"] and len(sad) == tr["n_before_cull"] - (tr["reason"] == R.ACCEPTED_ZERO_DISPARITY).sum()
        th = 1.5 * 1.4 * float(median)
        far = np.abs(np.array(sad) - th) > 1e-3                  # away from the float rounding of thDist
        culled = np.array([tr["reason"][i] == R.CULLED for i in reached if tr["reason"][i] in (R.ACCEPTED, R.CULLED)])
        assert ((np.array(sad) >= th) == culled)[far].all()


def test_thdist_is_exact_where_the_worlds_need_it(oracle):
    """median 10 -> thDist = 1.5f * 1.4f * 10 = 21.0 exactly, read from the trace: a sum of 20 is kept, 21 is culled"""
    for name in ("pixels", "median_odd", "median_tied", "hamming", "gates16", "gates80", "maxd"):
        tr = _run(oracle, name)["tr"]
        assert tr["median"] == 10 and tr["th_dist"] == np.float32(21.0) and tr["th_dist"].dtype == np.float32, name
    assert _run(oracle, "median_even")["tr"]["th_dist"] == np.float32(42.0)
    assert _run(oracle, "median_zeros")["tr"]["th_dist"] == 0.0
    assert _run(oracle, "nomatch")["tr"]["median"] is None


def test_floors_of_the_planted_worlds(oracle):
    """every reason code and every shape the planted GPU tests rely on is present, in the planted worlds alone"""
    total = {n: 0 for n in R.REASONS}
    for name in PLANTED:
        c = R.reason_counts(_run(oracle, name)["tr"])
        print(f"{name:14s} n_left {len(_run(oracle, name)['kl']):4d} n_right {len(_run(oracle, name)['kr']):4d}  "
              + "  ".join(f"{k}={v}" for k, v in c.items() if v))
        for k, v in c.items():
            total[k] += v
        shapes = [t.split(":")[0] for t in _run(oracle, name)["W"].tags]
        print(" " * 15 + "planted for: " + "  ".join(f"{s}={shapes.count(s)}" for s in dict.fromkeys(shapes)))
    print("planted total  " + "  ".join(f"{k}={v}" for k, v in total.items()))
    floors = dict(NO_CANDIDATES=2, NO_DESCRIPTOR_MATCH=10, WINDOW_OUT=3, BEST_AT_END=2, DISPARITY_OUT=2, ACCEPTED=600,
                  ACCEPTED_ZERO_DISPARITY=1, CULLED=120 + 1 + 4 + 2)
    assert all(total[k] >= v for k, v in floors.items()), total

    # every pixel counts once
    r = _run(oracle, "pixels")
    W, tr = r["W"], r["tr"]
    for k in range(121):
        if k == 60:
            continue
        (i21,), (i20,) = W.which(f"pix21:{k}"), W.which(f"pix20:{k}")
        assert tr["best_sum"][i21] == 21 and tr["reason"][i21] == R.CULLED and r["ur"][i21] == -1
        assert tr["best_sum"][i20] == 20 and tr["reason"][i20] == R.ACCEPTED and r["ur"][i20] > 0
    tens = W.which("ten")
    assert len(tens) == 260 and (tr["best_sum"][tens] == 10).all() and (tr["best_inc"] == 0).all()

    # median index and cull comparison
    for name, (sums, _, culled) in R.MEDIAN_WORLDS.items():
        r = _run(oracle, "median_" + name)
        assert sorted(r["tr"]["best_sum"].tolist()) == sorted(sums)
        assert sorted(r["tr"]["best_sum"][r["ur"] == -1].tolist()) == sorted(culled)
    assert (_run(oracle, "nomatch")["ur"] == -1).all() and _run(oracle, "nomatch")["tr"]["n_before_cull"] == 0

    # the descriptor stage
    r = _run(oracle, "hamming")
    W, tr, kr = r["W"], r["tr"], r["kr"]
    (i74,), (i75,) = W.which("ham74"), W.which("ham75")
    assert tr["hamming"][i74] == 74 and r["ur"][i74] > 0 and tr["hamming"][i75] == 75 and r["ur"][i75] == -1
    rows = {}
    for y in kr["y"]:
        rows[float(y)] = rows.get(float(y), 0) + 1
    assert {1, 2, 63, 64, 65, 129} <= set(rows.values())
    for n in (1, 63, 64, 65, 129):
        idx = W.which(f"row{n}")
        assert len(idx) == {1: 1, 63: 1, 64: 1, 65: 65, 129: 3}[n] and (r["ur"][idx] > 0).all()
        y = float(r["kl"]["y"][idx[0]])
        last = max(j for j in range(len(kr)) if kr["y"][j] == y)
        assert last in tr["best_idx"][idx]                   # the best candidate of a row is its last one
    for n, first in ((2, "true"), (2, "decoy"), (65, "true"), (129, "decoy")):
        (i,) = W.which(f"tie{n}:{first}_first")
        y = float(r["kl"]["y"][i])
        twins = [j for j in range(len(kr)) if kr["y"][j] == y and (r["dr"][j] == r["dr"][tr["best_idx"][i]]).all()]
        assert len(twins) == 2 and twins[1] - twins[0] == n - 1 and tr["best_idx"][i] == twins[0]
        assert kr["x"][twins[0]] != kr["x"][twins[1]] and (r["ur"][i] > 0) == (first == "true")

    # the gates
    r = _run(oracle, "gates16")
    W, tr, kl, kr = r["W"], r["tr"], r["kl"], r["kr"]
    maxD = W.mbf / W.mb
    (on,), (below,) = W.which("minU:on"), W.which("minU:below")
    assert kr["x"][tr["best_idx"][on]] == kl["x"][on] - maxD and tr["best_inc"][on] == 4 and r["ur"][on] > 0
    assert r["ur"][below] == -1 and 0 < (kl["x"][below] - maxD) - kr["x"][below] < 1e-5
    (on,), (above,) = W.which("maxU:on"), W.which("maxU:above")
    assert tr["reason"][on] == R.ACCEPTED_ZERO_DISPARITY and tr["delta"][on] == 0 and tr["best_sum"][on] == 0
    assert r["ur"][on] == kl["x"][on] - np.float32(0.01) and r["dp"][on] == W.mbf / np.float32(0.01)
    assert r["ur"][above] == -1 and 0 < kr["x"][above] - kl["x"][above] < 1e-5
    r = _run(oracle, "maxd")
    W, tr, kl = r["W"], r["tr"], r["kl"]
    maxD = W.mbf / W.mb
    (below,), (on,), (above,) = W.which("maxD:below"), W.which("maxD:on"), W.which("maxD:above")
    assert (tr["delta"][[below, on, above]] == 0).all() and (tr["best_inc"][[below, on, above]] == -4).all()
    assert kl["x"][below] - r["ur"][below] == np.nextafter(maxD, np.float32(0)) and kl["x"][on] - np.float32(8) == maxD
    assert r["ur"][on] == -1 and r["ur"][above] == -1 and tr["reason"][on] == R.DISPARITY_OUT
    r = _run(oracle, "gates80")
    W, tr, kl, kr = r["W"], r["tr"], r["kl"], r["kr"]
    assert r["pl"][0].shape[0] == 300
    for tag, reason in (("octR:+1", R.ACCEPTED), ("octR:+2", R.NO_DESCRIPTOR_MATCH), ("octL7:-2", R.NO_DESCRIPTOR_MATCH),
                        ("octL7:-1", R.ACCEPTED), ("octL7:+0", R.ACCEPTED), ("inc:-5", R.BEST_AT_END), ("inc:-4", R.ACCEPTED),
                        ("inc:+4", R.ACCEPTED), ("inc:+5", R.BEST_AT_END), ("iniu<0", R.WINDOW_OUT),
                        ("endu0:cols-1", R.ACCEPTED), ("endu0:cols", R.WINDOW_OUT), ("endu1:cols", R.WINDOW_OUT),
                        ("band_bottom", R.ACCEPTED)):
        (i,) = W.which(tag)
        assert tr["reason"][i] == reason, tag
    (i,) = W.which("endu1:cols-1")
    assert tr["reason"][i] not in (R.WINDOW_OUT, R.NO_DESCRIPTOR_MATCH, R.NO_CANDIDATES)      # it got past the column test
    for tag, inc in (("inc:-4", -4), ("inc:+4", 4), ("inc:-5", -5), ("inc:+5", 5)):
        assert tr["best_inc"][W.which(tag)[0]] == inc
    assert kr["x"][tr["best_idx"][W.which("iniu<0")[0]]] < 0
    (i,) = W.which("sadtie")
    assert tr["sums"][i][[2, 5, 8]].tolist() == [0, 0, 0] and tr["best_inc"][i] == -3 and tr["sums"][i].min() == 0
    assert r["ur"][i] == np.float32(kr["x"][tr["best_idx"][i]] - 3 + tr["delta"][i])
    yr, rr = kr["y"], 2 * R.SCALE[kr["octave"]]
    assert (np.floor(yr - rr) < 0).sum() >= 2 and (np.ceil(yr + rr) > 299).sum() >= 2       # bands cut by both borders
    assert np.ceil(yr + rr)[tr["best_idx"][W.which("band_bottom")[0]]] > 299

    # counts
    r = _run(oracle, "nright1")
    assert len(r["kr"]) == 1 and (r["ur"] > 0).sum() == 1
    assert len(_run(oracle, "pixels")["kl"]) >= max(R.N_LEFT_PREFIXES)

    # the levels nobody can plant
    r = _run(oracle, "levels", natural=True)
    acc = np.isin(r["tr"]["reason"], (R.ACCEPTED, R.ACCEPTED_ZERO_DISPARITY))
    per_level = [int((acc & (r["kl"]["octave"] == l)).sum()) for l in range(R.NLEVELS)]
    print(f"levels (the extractor's keypoints): {R.reason_counts(r['tr'])}; accepted per level {per_level}")
    assert min(per_level) >= 1


@pytest.mark.parametrize("n", R.N_LEFT_PREFIXES)
def test_prefixes_of_the_pixels_world(oracle, n):
    r = _run(oracle, "pixels")
    W = r["W"]
    eL, eR, pl, pr, _ = R.oracle_side(oracle, W)
    ur, dp, tr = R.compute(r["kl"][:n], r["dl"][:n], r["kr"], r["dr"], W.mb, W.mbf, R.SCALE, R.INV_SCALE, pl, pr)
    our, odp, _ = oracle.compute_stereo_matches(eL, eR, r["kl"][:n], r["dl"][:n], r["kr"], r["dr"], W.mb, W.mbf)
    assert ur.tobytes() == our.tobytes() and dp.tobytes() == odp.tobytes() and tr["n_before_cull"] == n


def test_domain_holds_for_every_world_and_every_extractor_keypoint(pkg, oracle):
    """in_domain() is the rule the host-pointer entry enforces: the planted worlds are inside it, and so is everything the
    extractor produces, so the check never refuses the product path"""
    for name in WORLD_NAMES:
        W = _worlds()[name]
        kl, dl, kr, dr = W.arrays()
        assert R.in_domain(kl, kr, W.sizes(), R.INV_SCALE) == (True, ""), name
        r = _run(oracle, name, natural=True)
        assert len(r["kl"]) > 300 and R.in_domain(r["kr"], r["kl"], W.sizes(), R.INV_SCALE)[0]   # (and the eyes swapped)
    S = pkg.synth
    for cfg in ("tum", "kitti", "euroc"):
        c = S.CONFIGS[cfg]
        left, right, _ = S.synth_stereo_pair(11, c["w"], c["h"], max_disp=48 if cfg != "kitti" else 96)
        e = oracle.Extractor(nfeatures=c["nfeatures"])
        sizes = None
        for img in (left, right, S.synth_image(12, c["w"], c["h"])):
            k, _ = e.extract(img)
            sizes = [e.level_size(l)[:2] for l in range(R.NLEVELS)]
            assert len(k) > 500 and R.in_domain(k, k, sizes, e.inv_scale_factors)[0], cfg
            assert k["x"].min() >= 16 and (k["x"] * e.inv_scale_factors[np.minimum(k["octave"] + 1, 7)]).min() >= 13
    # and the rule does refuse what leaves a plane
    W = _worlds()["median_odd"]
    kl, dl, kr, dr = W.arrays()
    for field, value, side in (("x", 4.4, 0), ("x", W.w - 5.4, 0), ("y", 4.4, 0), ("y", W.h - 5.4, 0), ("octave", 8, 0),
                               ("octave", -1, 0), ("x", np.nan, 0), ("y", np.inf, 0), ("x", 9.4, 1), ("x", 0.0, 1),
                               ("x", 11.3, 1), ("octave", 8, 1), ("y", np.nan, 1)):
        a, b = kl.copy(), kr.copy()
        (a, b)[side][field][2] = value
        assert not R.in_domain(a, b, W.sizes(), R.INV_SCALE)[0], (field, value, side)
    for field, value, side in (("x", 4.6, 0), ("x", W.w - 5.6, 0), ("x", -3.0, 1), ("x", 11.5, 1), ("x", np.nan, 1)):
        a, b = kl.copy(), kr.copy()
        (a, b)[side][field][2] = value
        assert R.in_domain(a, b, W.sizes(), R.INV_SCALE)[0], (field, value, side)
