"""Maps for the KeyFrameCulling tests (test_keyframe_culling_cpu.py, test_keyframe_culling_gpu.py): the planted cases, each with a
`prove` that asserts ON THE PYTHON REFERENCE's result the property the case exists for, and the seeded generator of the sweep.
A case is dict(name, g, v, cand, monocular, prove[, bad_cap]); g has the fields of aos2_local_map_graph_t, v those of
aos2_kf_culling_view_t."""
import numpy as np

import keyframe_culling_ref as ref

KEPT, CULLED, DEFERRED, SKIPPED = ref.KEPT, ref.CULLED, ref.DEFERRED, ref.SKIPPED
FIRST, NOT_ERASE = 1, 2   # kf_flags


def F(p, octave=0, depth=1.0, stereo=0):
    """a feature: point row (-1 = NULL), mvKeysUn[i].octave, mvDepth[i], mvuRight[i] >= 0"""
    return (p, octave, depth, stereo)


def make_map(n_points, kfs, obs=None, point_nobs=None, point_bad=(), th=2.0, flags=None):
    """kfs: one list of features per keyframe (F(...) or a bare point row).  The observations of a point default to the keyframes
    that hold it, at the FIRST feature that does; obs = {point: [(kf, idx), ...]} replaces them.  nObs defaults to 2 per stereo
    observation and 1 per other; point_nobs = {point: n} replaces it.  th: mThDepth of all, or {kf: th}; flags: {kf: bits}."""
    kfs = [[f if isinstance(f, tuple) else F(f) for f in k] for k in kfs]
    nk = len(kfs)
    derived = {p: [] for p in range(n_points)}
    for k, feats in enumerate(kfs):
        seen = set()
        for i, f in enumerate(feats):
            if f[0] >= 0 and f[0] not in seen:
                seen.add(f[0])
                derived[f[0]].append((k, i))
    o = [list((obs or {}).get(p, derived[p])) for p in range(n_points)]
    nobs = np.array([sum(2 if kfs[k][i][3] else 1 for k, i in x) for x in o], np.int32)
    for p, n in (point_nobs or {}).items():
        nobs[p] = n
    pb = np.zeros(n_points, np.uint8)
    pb[list(point_bad)] = 1
    g = dict(n_points=n_points, n_keyframes=nk, point_bad=pb, point_nobs=nobs, kf_bad=np.zeros(nk, np.uint8),
             kf_best=np.full(nk * 10, -1, np.int32), kf_parent=np.full(nk, -1, np.int32), kf_child_off=np.zeros(nk + 1, np.int32),
             kf_child=np.zeros(0, np.int32))
    g["obs_off"] = np.cumsum([0] + [len(x) for x in o]).astype(np.int32)
    g["obs_kf"] = np.array([k for x in o for k, _ in x], np.int32)
    g["kf_mp_off"] = np.cumsum([0] + [len(k) for k in kfs]).astype(np.int32)
    flat = [f for k in kfs for f in k]
    g["kf_mp"] = np.array([f[0] for f in flat], np.int32)
    fl = np.zeros(nk, np.uint8)
    for k, b in (flags or {}).items():
        fl[k] = b
    v = dict(obs_idx=np.array([i for x in o for _, i in x], np.int32), kf_octave=np.array([f[1] for f in flat], np.int8),
             kf_depth=np.array([f[2] for f in flat], np.float32), kf_stereo=np.array([f[3] for f in flat], np.uint8),
             kf_th_depth=np.array([th[k] if isinstance(th, dict) else th for k in range(nk)], np.float32), kf_flags=fl)
    return g, v


def case(name, gv, cand, prove, monocular=1, bad_cap=None):
    return dict(name=name, g=gv[0], v=gv[1], cand=np.array(cand, np.int32), monocular=monocular, prove=prove, bad_cap=bad_cap)


def want(c):
    """the reference's result for a case, proved to show what the case was planted for"""
    r = ref.keyframe_culling(c["g"], c["v"], c["monocular"], c["cand"])
    c["prove"](r)
    return r


class _Rows:
    """hands out fresh point rows"""

    def __init__(self):
        self.n = 0

    def take(self, k):
        self.n += k
        return list(range(self.n - k, self.n))


def _flip_to_kept(flags=None):
    # keyframes A=0, B=1 (candidates), C=2, D=3: ten points seen by all four.  A is redundant; without A the points have nObs 3
    return make_map(10, [list(range(10))] * 4, flags=flags)


def _flip_to_culled(flags=None):
    # A=0, B=1 (candidates), C, D, E = 2..4.  A: 60 points of {A,C,D,E} (redundant) + 5 of {A,B,C} (nObs 3) -> 60 > 0.9 * 65.
    # B: 10 points of {B,C,D,E} + the same 5 -> 10 > 13.5 is false.  A's cull takes the 5 to nObs 2: bad, B has 10 of 10.
    R = _Rows()
    ra, s, rb = R.take(60), R.take(5), R.take(10)
    return make_map(R.n, [ra + s, rb + s, ra + s + rb, ra + rb, ra + rb], flags=flags)


def _chain(flags=None, more=None):
    # K0..K3 (candidates 0..3), K4 = 4 (kept), helpers H1..H3 = 5..7.  R_j: 60 points of {K_j,H1,H2,H3}; S_j (j >= 1): 5 points of
    # {K_j-1,K_j,H1}, nObs 3; T: 5 points of {K3,H1,H2}.  K0 has 60 of 65 alone; K1..K3 have 60 of 70 until the keyframe before them
    # is culled and their S goes bad.
    R = _Rows()
    Rj = [R.take(60) for _ in range(4)]
    Sj = [None] + [R.take(5) for _ in range(3)]
    T, U = R.take(5), R.take(8)
    k = [Rj[0] + Sj[1], Rj[1] + Sj[1] + Sj[2], Rj[2] + Sj[2] + Sj[3], Rj[3] + Sj[3] + T, U]
    allr = [p for r in Rj for p in r]
    h1 = allr + Sj[1] + Sj[2] + Sj[3] + T + U
    return make_map(R.n, k + [h1, allr + T, allr] + list(more(U) if more else []), flags=flags)


def class_map():
    """the map of tests/test_keyframe_culling_class_gpu.py: the chain with H2 = 6 held by mbNotErase (redundant: DEFERRED) and H3 = 7
    as the mnId == 0 keyframe, the current keyframe 8 (it sees K4's points), two keyframes without points -> (g, v), the current
    keyframe's covisibles in their order, the current keyframe"""
    return _chain({6: NOT_ERASE, 7: FIRST}, lambda U: [U, [], []]), [6, 7, 0, 1, 2, 3, 4, 9, 10], 8


def planted():
    out = []

    # 1. nothing is redundant: every point has two observers
    def p1(r):
        assert (r["status"] == KEPT).all() and (r["n_redundant"] == 0).all() and (r["n_mps"] == 20).all() and r["n_bad_points"] == 0
    out.append(case("none_redundant", make_map(50, [list(range(10 * k, 10 * k + 10)) + list(range(10 * ((k + 1) % 5), 10 * ((k + 1) % 5) + 10))
                                                    for k in range(5)]), [3, 0, 4, 1, 2], p1))

    # 2. a cull turns "would be culled" into KEPT
    def p2(r):
        assert list(r["status"]) == [CULLED, KEPT] and r["alone"][1] == CULLED and list(r["n_redundant"]) == [10, 0]
        assert r["n_bad_points"] == 0
    out.append(case("flip_to_kept", _flip_to_kept(), [0, 1], p2))

    # 3. a cull turns "would be kept" into CULLED: the later candidate's other points go bad and nMPs shrinks
    def p3(r):
        assert list(r["status"]) == [CULLED, CULLED] and r["alone"][1] == KEPT and list(r["n_mps"]) == [65, 10]
        assert r["n_bad_points"] == 5 and list(r["bad_points"]) == [60, 61, 62, 63, 64]
    out.append(case("flip_to_culled", _flip_to_culled(), [0, 1], p3))

    # 4. a chain: every cull flips the next candidate
    def p4(r):
        assert list(r["status"]) == [CULLED] * 4 + [KEPT] and list(r["alone"]) == [CULLED, KEPT, KEPT, KEPT, KEPT]
        assert list(r["n_mps"][:4]) == [65] * 4 and r["n_bad_points"] == 20   # (S_1..S_3, and T when K3 goes)
    out.append(case("chain", _chain(), [0, 1, 2, 3, 4], p4))

    # 5. not monocular.  A = 0 (stereo features, mThDepth 2), B = 1, C..E = 2..4.
    #    P: 60 of {A,C,D,E}, nObs 5; Q: 10 of {A,B,C,D,E}, nObs 6; W: 5 of {A,B,C}, nObs 4: A's cull subtracts 2 -> bad
    #    A also holds 3 far points (depth 5), 2 with depth -1 and one AT the threshold, none of them redundant
    R = _Rows()
    P, Q, W, far, neg, at = R.take(60), R.take(10), R.take(5), R.take(3), R.take(2), R.take(1)
    A = [F(p, stereo=1) for p in P + Q + W] + [F(p, depth=5.0, stereo=1) for p in far] + [F(p, depth=-1.0) for p in neg] + \
        [F(at[0], depth=2.0, stereo=1)]
    up = [F(x, 9) for x in far + neg + at]   # (seen from C, D, E too, nine levels up: they never count and never go bad)
    gv5 = make_map(R.n, [A, Q + W, P + Q + W + up, P + Q + up, P + Q + up])

    def p5(r):
        assert list(r["status"]) == [CULLED, CULLED] and list(r["n_mps"]) == [76, 10] and list(r["n_redundant"]) == [70, 10]
        assert r["alone"][1] == KEPT and list(r["bad_points"]) == W   # (a subtraction of 1 would leave W at nObs 3)
        assert gv5[0]["point_nobs"][P[0]] == 5 and gv5[0]["obs_off"][P[0] + 1] - gv5[0]["obs_off"][P[0]] == 4
        m = ref.keyframe_culling(gv5[0], gv5[1], 1, [0, 1])
        assert list(m["n_mps"]) == [81, 15] and list(m["status"]) == [KEPT, KEPT]   # monocular: the far points count
    out.append(case("stereo", gv5, [0, 1], p5, monocular=0))
    out.append(case("stereo_as_monocular", gv5, [0, 1], lambda r: None, monocular=1))

    # 6. a redundant candidate with mbNotErase is DEFERRED: the later ones get the verdict they would get alone
    def p6a(r):
        assert list(r["status"]) == [DEFERRED, CULLED] and list(r["status"][1:]) == list(r["alone"][1:]) and r["n_bad_points"] == 0
        assert list(r["n_redundant"]) == [10, 10]
    out.append(case("deferred_then_culled", _flip_to_kept({0: NOT_ERASE}), [0, 1], p6a))

    def p6b(r):
        assert list(r["status"]) == [DEFERRED, KEPT] and list(r["status"][1:]) == list(r["alone"][1:]) and r["n_bad_points"] == 0
        assert list(r["n_mps"]) == [65, 15]
    out.append(case("deferred_then_kept", _flip_to_culled({0: NOT_ERASE}), [0, 1], p6b))

    # 7. the mnId == 0 keyframe is skipped, redundant as it is
    def p7(r):
        assert list(r["status"]) == [SKIPPED, CULLED] and r["n_mps"][0] == 0 and r["n_redundant"][0] == 0 and r["n_redundant"][1] == 10
    out.append(case("first_keyframe", _flip_to_kept({0: FIRST | NOT_ERASE}), [0, 1], p7))

    # 8. A = 0 holds each of p (10 points of {A,B,C,D,E}, nObs 5) at TWO features: nObs falls once, to 4, and B = 1 still finds them
    #    redundant.  A also matches q (10 points of {B,C,D,E}, nObs 4) which do not list A: nObs stays 4.
    R = _Rows()
    p, q = R.take(10), R.take(10)
    obs = {x: [(1, 10 + j), (2, 10 + j), (3, 10 + j), (4, 10 + j)] for j, x in enumerate(q)}
    gv8 = make_map(R.n, [p + q + p, p + q, p + q, p + q, p + q], obs=obs)

    def p8(r):
        assert list(r["status"]) == [CULLED, CULLED] and list(r["n_mps"]) == [30, 20] and list(r["n_redundant"]) == [30, 20]
        assert r["n_bad_points"] == 0
    out.append(case("twice_in_one_keyframe_and_not_listed", gv8, [0, 1], p8))

    # 9. the scale gate, candidate features at level 2
    def scale(others, extra=None):
        k = [[F(x, 2) for x in range(10)]] + [[F(x, o) for x in range(10)] for o in others]
        return make_map(10, k, point_nobs=extra)

    def p9a(r):
        assert list(r["status"]) == [CULLED] and r["n_redundant"][0] == 10
    out.append(case("scale_level_plus_1", scale([3, 3, 3]), [0], p9a))

    def p9b(r):
        assert list(r["status"]) == [KEPT] and r["n_redundant"][0] == 0 and r["n_mps"][0] == 10
    out.append(case("scale_level_plus_2", scale([4, 4, 4]), [0], p9b))
    # three qualifying observers of which one is the candidate, a fourth two levels up: nObs 4 > 3, but only two count
    out.append(case("scale_candidate_is_the_third", scale([3, 0, 4]), [0], p9b))

    # 10. the 0.9 boundary.  N = 0: 9 redundant + 1; Z = 1: no features with points; T = 2: 10 redundant; helpers 3..5
    R = _Rows()
    n9, n1, t10 = R.take(9), R.take(1), R.take(10)
    gv10 = make_map(R.n, [n9 + n1, [-1, -1], t10, n9 + n1 + t10, n9 + t10, n9 + t10])

    def p10(r):
        assert list(r["status"]) == [KEPT, KEPT, CULLED] and list(r["n_mps"]) == [10, 0, 10] and list(r["n_redundant"]) == [9, 0, 10]
    out.append(case("boundary_0_9", gv10, [0, 1, 2], p10))

    # 11. sizes that cross the strides: A = 0 with 2 * 1024 + 1 features (the count and apply kernels run 1024 lanes); B = 1
    #     holds 10 points with 70 observers each of which only the LAST three pass the scale gate; E = 2 has no features
    R = _Rows()
    big, z = R.take(2049), R.take(10)
    k = [big, z, []] + [big + [F(x, 9) for x in z]] * 3 + [[F(x, 9) for x in z]] * 64 + [z] * 3
    gv11 = make_map(R.n, k)

    def p11(r):
        assert list(r["status"]) == [CULLED, CULLED, KEPT] and list(r["n_mps"]) == [2049, 10, 0] and list(r["n_redundant"]) == [2049, 10, 0]
        off = gv11[0]["obs_off"]
        assert off[z[0] + 1] - off[z[0]] == 71
    out.append(case("strides", gv11, [0, 1, 2], p11))
    out.append(case("no_candidates", gv11, [], lambda r: None))

    # 12. bad_cap below the count
    def p12(r):
        assert r["n_bad_points"] == 5
    out.append(case("small_bad_cap", _flip_to_culled(), [0, 1], p12, bad_cap=2))
    return out


SWEEP_SEEDS = tuple(range(101, 125))


def random_case(seed):
    """a map of 12-40 keyframes and up to ~400 points as a camera moving along a line leaves it: a point is seen from a run of
    consecutive keyframes, at octaves that drift; with NULL features, bad points, stereo and far features, points held twice, matches
    that the point does not list and entries that the keyframe does not hold, mbNotErase keyframes and the mnId == 0 keyframe"""
    rng = np.random.default_rng(seed)
    nk = int(rng.integers(12, 41))
    npnt = int(rng.integers(150, 401))
    dense = rng.random() < 0.7   # long runs: many redundant keyframes
    monocular = int(rng.random() < 0.5)
    kfs = [[] for _ in range(nk)]
    obs = {}
    for p in range(npnt):
        run = int(rng.integers(5, 11)) if (dense and rng.random() < 0.96) else int(rng.integers(1, 5))
        k0 = int(rng.integers(0, max(1, nk - run + 1)))
        lvl = int(rng.integers(0, 4))
        o = []
        for k in range(k0, min(nk, k0 + run)):
            if rng.random() < 0.05:
                continue
            u = rng.random()
            depth = 5.0 if u < 0.04 else (-1.0 if u < 0.08 else (2.0 if u < 0.1 else 1.0))
            drift = int(rng.integers(-1, 3)) if rng.random() < 0.2 else 0
            kfs[k].append(F(p, max(0, lvl + drift), depth, int(rng.random() < 0.3)))
            o.append(k)
        obs[p] = o
    pairs = {}
    for k in range(nk):
        for _ in range(int(rng.integers(0, 4))):
            kfs[k].append(F(-1))
        if kfs[k] and rng.random() < 0.3:   # a point at two features
            kfs[k].append(kfs[k][int(rng.integers(0, len(kfs[k])))])
        kfs[k] = [kfs[k][i] for i in rng.permutation(len(kfs[k]))]
        first = {}
        for i, f in enumerate(kfs[k]):
            if f[0] >= 0:
                first.setdefault(f[0], i)
        pairs[k] = first
    full = {}
    for p in range(npnt):
        o = [(k, pairs[k][p]) for k in obs[p]]
        if o and rng.random() < 0.05:      # a match that the point does not list
            o.pop(int(rng.integers(0, len(o))))
        if rng.random() < 0.03:            # an entry whose keyframe does not hold the point
            k = int(rng.integers(0, nk))
            if kfs[k] and k not in [x for x, _ in o]:
                o.append((k, int(rng.integers(0, len(kfs[k])))))
        full[p] = [o[i] for i in rng.permutation(len(o))]
    flags = {0: FIRST}
    for k in range(1, nk):
        if rng.random() < 0.08:
            flags[k] = NOT_ERASE
    g, v = make_map(npnt, kfs, obs=full, point_bad=np.flatnonzero(rng.random(npnt) < 0.03), flags=flags)
    noise = rng.random(npnt) < 0.05
    g["point_nobs"] = (g["point_nobs"] + noise * rng.integers(-1, 2, npnt)).astype(np.int32)
    cand = rng.permutation(nk)[:int(rng.integers(nk // 2, nk + 1))]
    return case(f"seed_{seed}", (g, v), cand, lambda r: None, monocular=monocular)
