"""Cases for the UpdateNormalAndDepth tests (test_update_normal_depth_cpu.py, test_update_normal_depth_gpu.py): planted batches over
one graph of 300 keyframes with a few features each, every one with a `prove` that asserts ON THE REFERENCE RESTATEMENT's result what it
was planted for, and seeded random cases.  A case is a dict: g, v (graph and culling view), point, xyz, ref_kf, kf_center, scale,
rows_form, term_off (or None)."""
import numpy as np

import normal_depth_ref as ref

NK = 300
LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 257)   # the seams of a lane group, of a wave, of the LDS form (and what a hook sets)
BATCHES = (1, 63, 64, 65, 257)
SCALE = np.array([1.2 ** i for i in range(8)], np.float32)
NO_FEATURES, ODD_OCTAVES = 299, 298   # a keyframe without a feature; one whose octaves are 9 and -1
LEFT, RIGHT = 290, 291                # the two cameras the interval points look from


def csr(lists):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    return off, np.array([v for x in lists for v in x], np.int32)


def build(octaves, obs, bad=()):
    """octaves: one list of feature octaves per keyframe; obs: one list of (keyframe, feature) per point, in the stored order ->
    graph and view.  The match lists are as long as the feature lists and name the points that observe them."""
    nk, n_points = len(octaves), len(obs)
    kf_mp = [[-1] * len(o) for o in octaves]
    for p, lst in enumerate(obs):
        for k, f in lst:
            kf_mp[k][f] = p
    pb = np.zeros(n_points, np.uint8)
    pb[list(bad)] = 1
    g = dict(n_points=n_points, n_keyframes=nk, point_bad=pb, point_nobs=np.array([len(x) for x in obs], np.int32),
             kf_bad=np.zeros(nk, np.uint8), kf_best=np.full(nk * 10, -1, np.int32), kf_parent=np.full(nk, -1, np.int32))
    g["obs_off"], g["obs_kf"] = csr([[k for k, _ in x] for x in obs])
    g["kf_mp_off"], g["kf_mp"] = csr(kf_mp)
    g["kf_child_off"], g["kf_child"] = csr([[] for _ in range(nk)])
    n_mp = len(g["kf_mp"])
    v = dict(obs_idx=np.array([f for x in obs for _, f in x], np.int32), kf_octave=np.array([o for x in octaves for o in x], np.int8),
             kf_depth=np.ones(n_mp, np.float32), kf_stereo=np.zeros(n_mp, np.uint8), kf_th_depth=np.full(nk, 40, np.float32),
             kf_flags=np.zeros(nk, np.uint8))
    return g, v


_WORLD = {}


def world():
    """the planted graph, built once: points 0 .. 12 have the lists of LENGTHS, the others are named in `at`"""
    if _WORLD:
        return _WORLD
    rng = np.random.RandomState(2024)
    octaves = [[(k + f) % 8 for f in range(3 + k % 3)] for k in range(NK)]
    octaves[NO_FEATURES] = []
    octaves[ODD_OCTAVES] = [9, -1, 3]
    centre = rng.uniform(-5, 5, (NK, 3)).astype(np.float32)
    centre[LEFT], centre[RIGHT] = (-1, 0, 0), (1, 0, 0)
    observers = list(range(0, 280))   # the lists come from here; 280 .. 299 observe only what is planted below
    obs, xyz, at = [], [], {}
    for L in LENGTHS:
        ks = sorted(rng.choice(observers, L, replace=False).tolist())
        obs.append([(k, (len(obs) + k) % len(octaves[k])) for k in ks])
        xyz.append(rng.uniform(-3, 3, 3))

    def plant(name, lst, P, **kw):
        at[name] = len(obs)
        obs.append(lst)
        xyz.append(P)

    plant("bad", [(3, 0), (7, 1)], (0.5, 0.25, 2))
    plant("d0_d2_zero", [(4, 1), (9, 2)], centre[4] + np.float32([0, 1.5, 0]))       # straight above camera 4: atan2(0, 0)
    plant("on_centre", [(5, 0), (11, 1), (12, 2)], centre[11])                         # cv::norm == 0: inf and NaN, as there
    plant("odd_octave_9", [(20, 1), (ODD_OCTAVES, 0)], (1, 1, 1))
    plant("odd_octave_neg", [(21, 1), (ODD_OCTAVES, 1)], (1, 2, 1))
    plant("odd_octave_ok", [(22, 1), (ODD_OCTAVES, 2)], (1, 2, 3))
    # two cameras at x = -1 and +1, the point in front of their middle at depth z: theta = -+atan(1 / z), mean 0, std atan(1 / z)
    plant("far", [(LEFT, 0), (RIGHT, 0)], (0, 0, 100))                                 # 2.5 std below both floors
    plant("between", [(LEFT, 1), (RIGHT, 1)], (0, 0, 1 / np.tan(0.1)))                 # above 10 / 57.3, below 30 / 57.3
    plant("near", [(LEFT, 2), (RIGHT, 2)], (0, 0, 1))                                  # above both
    g, v = build(octaves, obs, bad=[at["bad"]])
    _WORLD.update(g=g, v=v, centre=centre, xyz=np.array(xyz, np.float32), obs=obs, at=at)
    return _WORLD


def case(name, entries, rows_form=ref.ROWS_PLANNING, term_off=None, prove=None):
    """entries: (point row, reference keyframe) pairs over the planted world; a row the table does not know sits at the origin"""
    w = world()
    point = np.array([p for p, _ in entries], np.int32)
    xyz = np.array([w["xyz"][p] if p < len(w["xyz"]) else (0, 0, 0) for p, _ in entries], np.float32).reshape(-1, 3)
    return dict(name=name, g=w["g"], v=w["v"], point=point, xyz=xyz, ref_kf=np.array([r for _, r in entries], np.int32),
                kf_center=w["centre"], scale=SCALE, rows_form=rows_form, term_off=term_off, prove=prove)


def non_observer(p):
    w = world()
    seen = {k for k, _ in w["obs"][p]}
    return next(k for k in range(NK - 20) if k not in seen)


def length_entries():
    """every list length with the reference keyframe as first observer, as last observer and as a non-observer"""
    w = world()
    out = []
    for p, L in enumerate(LENGTHS):
        ks = [k for k, _ in w["obs"][p]]
        out += [(p, ks[0] if L else 0), (p, ks[-1] if L else 1), (p, non_observer(p))]
    return out


def term_offsets(entries, mismatch=()):
    """CSR room of exactly each list's length, except for the listed entries of `mismatch`: one too many"""
    w = world()
    lens = [(len(w["obs"][p]) if p < len(w["obs"]) else 0) + (1 if i in mismatch else 0) for i, (p, _) in enumerate(entries)]
    return np.cumsum([0] + lens).astype(np.int32)


def planted():
    w, at = world(), world()["at"]
    S = ref
    out = []
    le = length_entries()

    def prove_lengths(r, c):
        assert list(r["status"][:3]) == [S.NO_OBS] * 3 and (r["status"][3:] == S.UPDATED).all()
        assert list(r["n_terms"][3::3]) == list(LENGTHS[1:])
        # first, last and no observer read different features: somewhere the distances differ
        assert any(r["max_dist"][i] != r["max_dist"][i + 2] for i in range(3, len(le), 3))

    for form, tag in ((S.ROWS_PLANNING, "planning"), (S.ROWS_TRACKING, "tracking")):
        out.append(case("lengths/" + tag, le, form, prove=prove_lengths))

    sp = [(at["bad"], 3), (1, w["obs"][1][0][0]), (1, w["obs"][1][0][0]), (w["g"]["n_points"], 0), (w["g"]["n_points"] + 1000, 5),
          (at["d0_d2_zero"], 4), (at["on_centre"], 11), (at["on_centre"], 5), (3, NO_FEATURES), (at["odd_octave_9"], ODD_OCTAVES),
          (at["odd_octave_neg"], ODD_OCTAVES), (at["odd_octave_ok"], ODD_OCTAVES), (at["far"], LEFT), (at["between"], LEFT),
          (at["near"], RIGHT)]

    def prove_specials(r, c):
        U = S.UPDATED
        assert list(r["status"]) == [S.BAD, U, U, S.UNKNOWN, S.UNKNOWN, U, U, U, S.REF_UNUSABLE, S.REF_UNUSABLE, S.REF_UNUSABLE, U, U, U, U]
        assert r["normal"][1].tobytes() == r["normal"][2].tobytes()                   # a repeated row
        assert r["normal"][0].tolist() == [-7, -7, -7] and r["upper"][8] == -7        # untouched
        assert np.isnan(r["normal"][6]).all() and r["max_dist"][6] == 0 and r["max_dist"][7] > 0   # on a camera centre
        assert np.isfinite(r["theta_mean"][5])                                        # atan2(0, 0) = 0
        wide = r["theta_std"][12:15].astype(np.float64) * 2.5
        assert wide[0] < 10 / 57.3 < wide[1] < 30 / 57.3 < wide[2]
        floor = np.float32((30 if c["rows_form"] == S.ROWS_PLANNING else 10) / 57.3)
        assert r["upper"][12] == r["theta_mean"][12] + floor and r["upper"][14] > r["theta_mean"][14] + floor
        assert (r["upper"][13] == r["theta_mean"][13] + floor) == (c["rows_form"] == S.ROWS_PLANNING)

    for form, tag in ((S.ROWS_PLANNING, "planning"), (S.ROWS_TRACKING, "tracking")):
        out.append(case("specials/" + tag, sp, form, prove=prove_specials))

    mismatch = set(range(4, len(le), 2)) | {0}
    def prove_terms(r, c):
        off = c["term_off"]
        for i in range(len(le)):
            a, b = int(off[i]), int(off[i + 1])
            written = (r["term_theta"][a:b] != -7).any()
            assert written == (i not in mismatch and r["status"][i] == S.UPDATED), i
    out.append(case("term_off/matching_and_not", le, term_off=term_offsets(le, mismatch), prove=prove_terms))
    out.append(case("term_off/specials", sp, S.ROWS_TRACKING, term_off=term_offsets(sp),
                    prove=lambda r, c: (r["term_theta"][c["term_off"][0]:c["term_off"][1]] == -7).all()))
    out.append(case("empty", [], prove=lambda r, c: len(r["status"]) == 0))
    pool = le[3:] + sp
    for B in BATCHES:
        out.append(case("batch/%d" % B, [pool[(7 * i) % len(pool)] for i in range(B)], S.ROWS_TRACKING if B & 1 else S.ROWS_PLANNING,
                        prove=lambda r, c: len(r["status"]) == len(c["point"])))
    return out


def random_case(seed):
    """a small random world of its own: lists of 0 .. 20 observers (now and then 70), bad points, unknown and repeated rows, reference
    keyframes among the observers and outside, with and without room for the per-observation outputs"""
    rng = np.random.RandomState(1000 + seed)
    nk, n_points = int(rng.randint(72, 90)), int(rng.randint(10, 40))
    octaves = [[int(o) for o in rng.randint(0, 8, rng.randint(1, 6))] for _ in range(nk)]
    obs = []
    for p in range(n_points):
        L = 70 if rng.rand() < 0.05 else int(rng.randint(0, 21))
        ks = sorted(rng.choice(nk, L, replace=False).tolist())
        obs.append([(k, int(rng.randint(len(octaves[k])))) for k in ks])
    bad = [p for p in range(n_points) if rng.rand() < 0.1]
    g, v = build(octaves, obs, bad)
    B = int(rng.randint(1, 80))
    point = rng.randint(0, n_points + 2, B).astype(np.int32)
    ref_kf = np.array([obs[p][rng.randint(len(obs[p]))][0] if p < n_points and obs[p] and rng.rand() < 0.7 else rng.randint(nk)
                       for p in point], np.int32)
    term_off = None
    if seed % 2:
        lens = [(len(obs[p]) if p < n_points else 0) + int(rng.rand() < 0.2) for p in point]
        term_off = np.cumsum([0] + lens).astype(np.int32)
    return dict(name="random/%d" % seed, g=g, v=v, point=point, xyz=rng.uniform(-4, 4, (B, 3)).astype(np.float32), ref_kf=ref_kf,
                kf_center=rng.uniform(-5, 5, (nk, 3)).astype(np.float32), scale=SCALE, rows_form=seed // 2 % 2, term_off=term_off,
                prove=None)


def want(c):
    """the reference restatement's result for a case, proved to hold what the case was planted for"""
    r = ref.update_normal_depth(c["g"], c["v"], c["point"], c["xyz"], c["ref_kf"], c["kf_center"], c["scale"], c["rows_form"], c["term_off"])
    if c["prove"] is not None:
        assert c["prove"](r, c) is not False, c["name"]
    return r
