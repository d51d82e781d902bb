"""Deltas for the aos2_local_map_apply tests (test_local_map_apply_cpu.py, test_local_map_apply_gpu.py): planted deltas on a small
map, each with a `prove` that asserts ON THE PYTHON REFERENCE's result what the case exists for, and random_delta, which changes a
map the way one pass of LocalMapping::Run does.  A map is edited as a MODEL (lists of points and keyframes); the delta is the
difference of two models, the rows that changed."""
import copy

import numpy as np

import keyframe_culling_cases as kcases
import local_map_apply_ref as ref

NB = ref.NB


# ---- the model: pts[p] = dict(bad, nobs, obs=[(kf, idx)]); kfs[k] = dict(bad, feats=[(point, octave, depth, stereo)], best, children,
# parent, th, flags)
def to_model(g, v):
    pts, kfs = [], []
    for p in range(g["n_points"]):
        a, b = g["obs_off"][p], g["obs_off"][p + 1]
        pts.append(dict(bad=int(g["point_bad"][p]), nobs=int(g["point_nobs"][p]),
                        obs=[(int(g["obs_kf"][e]), int(v["obs_idx"][e])) for e in range(a, b)]))
    for k in range(g["n_keyframes"]):
        a, b = g["kf_mp_off"][k], g["kf_mp_off"][k + 1]
        c0, c1 = g["kf_child_off"][k], g["kf_child_off"][k + 1]
        kfs.append(dict(bad=int(g["kf_bad"][k]),
                        feats=[(int(g["kf_mp"][f]), int(v["kf_octave"][f]), float(v["kf_depth"][f]), int(v["kf_stereo"][f])) for f in range(a, b)],
                        best=[int(x) for x in g["kf_best"][k * NB:(k + 1) * NB] if x >= 0], children=[int(x) for x in g["kf_child"][c0:c1]],
                        parent=int(g["kf_parent"][k]), th=float(v["kf_th_depth"][k]), flags=int(v["kf_flags"][k])))
    return dict(pts=pts, kfs=kfs)


def _off(rows):
    return np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)


def _best(b):
    return list(b[:NB]) + [-1] * (NB - len(b[:NB]))


def to_arrays(m):
    pts, kfs = m["pts"], m["kfs"]
    g = dict(n_points=len(pts), n_keyframes=len(kfs), point_bad=np.array([p["bad"] for p in pts], np.uint8),
             point_nobs=np.array([p["nobs"] for p in pts], np.int32), obs_off=_off([p["obs"] for p in pts]),
             obs_kf=np.array([k for p in pts for k, _ in p["obs"]], np.int32), kf_bad=np.array([k["bad"] for k in kfs], np.uint8),
             kf_mp_off=_off([k["feats"] for k in kfs]), kf_mp=np.array([f[0] for k in kfs for f in k["feats"]], np.int32),
             kf_best=np.array([_best(k["best"]) for k in kfs], np.int32).reshape(-1), kf_child_off=_off([k["children"] for k in kfs]),
             kf_child=np.array([c for k in kfs for c in k["children"]], np.int32), kf_parent=np.array([k["parent"] for k in kfs], np.int32))
    v = dict(obs_idx=np.array([i for p in pts for _, i in p["obs"]], np.int32),
             kf_octave=np.array([f[1] for k in kfs for f in k["feats"]], np.int8),
             kf_depth=np.array([f[2] for k in kfs for f in k["feats"]], np.float32),
             kf_stereo=np.array([f[3] for k in kfs for f in k["feats"]], np.uint8),
             kf_th_depth=np.array([k["th"] for k in kfs], np.float32), kf_flags=np.array([k["flags"] for k in kfs], np.uint8))
    return g, v


EMPTY_POINT = dict(bad=1, nobs=0, obs=[])


def delta_between(m0, m1, with_view=True, name_points=(), name_mp=(), name_links=()):
    """the delta that turns model m0 into m1: the rows that differ, every appended keyframe, every appended point that is not the
    empty slot, and the rows the caller wants named on top"""
    p0, k0, p1, k1 = m0["pts"], m0["kfs"], m1["pts"], m1["kfs"]
    prow = [r for r in range(len(p1)) if r in name_points or (p1[r] != p0[r] if r < len(p0) else p1[r] != EMPTY_POINT)]
    mrow = [r for r in range(len(k1)) if r in name_mp or r >= len(k0) or k1[r]["feats"] != k0[r]["feats"]]
    link = ("bad", "best", "children", "parent", "th", "flags")
    lrow = [r for r in range(len(k1)) if r in name_links or r >= len(k0) or any(k1[r][x] != k0[r][x] for x in link)]
    d = dict(n_points=len(p1), n_keyframes=len(k1), point_row=np.array(prow, np.int32),
             point_bad=np.array([p1[r]["bad"] for r in prow], np.uint8), point_nobs=np.array([p1[r]["nobs"] for r in prow], np.int32),
             obs_off=_off([p1[r]["obs"] for r in prow]), obs_kf=np.array([k for r in prow for k, _ in p1[r]["obs"]], np.int32),
             kf_mp_row=np.array(mrow, np.int32), kf_mp_off=_off([k1[r]["feats"] for r in mrow]),
             kf_mp=np.array([f[0] for r in mrow for f in k1[r]["feats"]], np.int32),
             kf_link_row=np.array(lrow, np.int32), kf_bad=np.array([k1[r]["bad"] for r in lrow], np.uint8),
             kf_best=np.array([_best(k1[r]["best"]) for r in lrow], np.int32).reshape(-1), kf_child_off=_off([k1[r]["children"] for r in lrow]),
             kf_child=np.array([c for r in lrow for c in k1[r]["children"]], np.int32),
             kf_parent=np.array([k1[r]["parent"] for r in lrow], np.int32), view=None)
    if with_view:
        d["view"] = dict(obs_idx=np.array([i for r in prow for _, i in p1[r]["obs"]], np.int32),
                         kf_octave=np.array([f[1] for r in mrow for f in k1[r]["feats"]], np.int8),
                         kf_depth=np.array([f[2] for r in mrow for f in k1[r]["feats"]], np.float32),
                         kf_stereo=np.array([f[3] for r in mrow for f in k1[r]["feats"]], np.uint8),
                         kf_th_depth=np.array([k1[r]["th"] for r in lrow], np.float32),
                         kf_flags=np.array([k1[r]["flags"] for r in lrow], np.uint8))
    return d


def base_model():
    """6 keyframes of 4 levels, 20 points, each seen from a run of keyframes; a spanning tree 0 <- 1 <- 2 ..., covisibles both ways"""
    F = kcases.F
    kfs = [[F(p, (p + k) % 4, 1.0 + 0.25 * k, (p + k) % 3 == 0) for p in range(20) if k <= p // 3 + 1 and p // 3 - 2 <= k] + [F(-1)] for k in range(6)]
    g, v = kcases.make_map(20, kfs, point_bad=[7], th=3.0, flags={0: kcases.FIRST, 3: kcases.NOT_ERASE})
    m = to_model(g, v)
    for k in range(6):
        m["kfs"][k]["best"] = [j for j in (k - 1, k + 1, k - 2, k + 2) if 0 <= j < 6]
        m["kfs"][k]["parent"] = k - 1
        m["kfs"][k]["children"] = [k + 1] if k < 5 else []
    m["kfs"][0]["children"] = [1, 4]   # (an extra child, listed out of order below)
    m["kfs"][4]["parent"] = 0
    m["kfs"][3]["children"] = []
    return m


def _lens(g, key):
    return np.diff(g[key])


def case(name, m0, m1, prove, with_view=True, **named):
    g0, v0 = to_arrays(m0)
    g1, v1 = to_arrays(m1)
    return dict(name=name, g=g0, v=v0 if with_view else None, delta=delta_between(m0, m1, with_view, **named), g1=ref.stored(g1),
                v1=v1 if with_view else None, prove=prove)


def want(c):
    """the reference's result for a case: proved to show what the case was planted for, and equal to the edited model"""
    g, v = ref.apply(c["g"], c["v"], c["delta"])
    assert ref.same_graph(g, c["g1"]) is None and ref.same_view(v, c["v1"]) is None, c["name"]
    c["prove"](c["g"], g, c["delta"])
    return g, v


def planted():
    out = []
    m0 = base_model()

    # 1. a keyframe inserted: matches to existing points (which gain an observation) and to two appended points
    m = copy.deepcopy(m0)
    m["pts"] += [dict(bad=0, nobs=1, obs=[(6, 3)]), dict(bad=0, nobs=2, obs=[(6, 4)])]
    m["kfs"].append(dict(bad=0, feats=[(15, 1, 1.5, 0), (16, 2, 2.5, 1), (-1, 0, 1.0, 0), (20, 0, 0.5, 0), (21, 3, -1.0, 1), (19, 1, 1.0, 0)],
                         best=[5, 4], children=[], parent=5, th=3.5, flags=0))
    for p, i in ((15, 0), (16, 1), (19, 5)):
        m["pts"][p]["obs"].append((6, i))
        m["pts"][p]["nobs"] += 1
    m["kfs"][5]["children"] = [6]
    m["kfs"][5]["best"] = [6, 4, 3]

    def p1(g0, g, d):
        assert g["n_keyframes"] == 7 and g["n_points"] == 22 and list(d["kf_mp_row"]) == [6] and list(d["kf_link_row"]) == [5, 6]
        assert _lens(g, "obs_off")[15] == _lens(g0, "obs_off")[15] + 1 and list(d["point_row"]) == [15, 16, 19, 20, 21]
    out.append(case("append_keyframe", m0, m, p1))

    # 2. rows that shrink: an observation erased, a point going bad (its list cleared), a keyframe going bad
    m = copy.deepcopy(m0)
    m["pts"][4]["obs"].pop(0)
    m["pts"][4]["nobs"] -= 1
    m["pts"][9] = dict(bad=1, nobs=0, obs=[])
    m["kfs"][2]["bad"] = 1
    m["kfs"][2]["children"] = []

    def p2(g0, g, d):
        a, b = _lens(g0, "obs_off"), _lens(g, "obs_off")
        assert b[4] == a[4] - 1 and a[9] > 0 and b[9] == 0 and g["point_bad"][9] == 1 and g["kf_bad"][2] == 1
        assert _lens(g, "kf_child_off")[2] == 0 and len(d["kf_mp_row"]) == 0 and list(d["kf_link_row"]) == [2]
    out.append(case("shrink", m0, m, p2))

    # 3. a row that becomes empty while it stays good, between rows that keep theirs
    m = copy.deepcopy(m0)
    m["pts"][10]["obs"] = []

    def p3(g0, g, d):
        assert _lens(g, "obs_off")[10] == 0 and _lens(g0, "obs_off")[10] > 0 and g["point_bad"][10] == 0 and list(d["point_row"]) == [10]
        assert g["obs_off"][-1] == g0["obs_off"][-1] - _lens(g0, "obs_off")[10]
    out.append(case("row_becomes_empty", m0, m, p3))

    # 4. the first row, the last row, two adjacent rows, ALL rows named (most with the content they have)
    def grow(rows):
        m = copy.deepcopy(m0)
        for p in rows:
            k = next(k for k in range(6) if k not in [o[0] for o in m["pts"][p]["obs"]])
            m["pts"][p]["obs"].append((k, 0))
            m["pts"][p]["nobs"] += 2
        return m

    def p4(rows):
        def prove(g0, g, d):
            a, b = _lens(g0, "obs_off"), _lens(g, "obs_off")
            assert [p for p in range(20) if a[p] != b[p]] == rows and g["point_nobs"][rows[0]] == g0["point_nobs"][rows[0]] + 2
        return prove
    out.append(case("first_row", m0, grow([0]), p4([0])))
    out.append(case("last_row", m0, grow([19]), p4([19])))
    out.append(case("adjacent_rows", m0, grow([11, 12]), p4([11, 12])))
    m = grow([3, 12])
    m["kfs"][1]["feats"][0] = (-1, 0, 9.0, 1)
    m["kfs"][5]["best"] = [0]

    def p4all(g0, g, d):
        assert list(d["point_row"]) == list(range(20)) and list(d["kf_mp_row"]) == list(range(6)) and list(d["kf_link_row"]) == list(range(6))
        assert g["obs_off"][-1] == g0["obs_off"][-1] + 2 and g["kf_mp"][g["kf_mp_off"][1]] == -1
    out.append(case("all_rows_named", m0, m, p4all, name_points=range(20), name_mp=range(6), name_links=range(6)))

    # 5. appended point rows that the delta does not name: empty slots, bad, without observations
    m = copy.deepcopy(m0)
    m["pts"] += [dict(EMPTY_POINT), dict(EMPTY_POINT), dict(bad=0, nobs=1, obs=[(2, 1)]), dict(EMPTY_POINT)]

    def p5(g0, g, d):
        assert g["n_points"] == 24 and list(d["point_row"]) == [22] and list(g["point_bad"][20:]) == [1, 1, 0, 1]
        assert list(_lens(g, "obs_off")[20:]) == [0, 0, 1, 0] and list(g["point_nobs"][20:]) == [0, 0, 1, 0]
    out.append(case("appended_unnamed", m0, m, p5))

    # 6. link rows only: a covisibility list, the children (given out of order) and a parent change, no match row
    m = copy.deepcopy(m0)
    m["kfs"][1]["best"] = [5, 4, 3, 2, 0]
    m["kfs"][0]["children"] = [4, 3, 1]
    m["kfs"][3]["parent"] = 0
    m["kfs"][2]["children"] = []
    m["kfs"][4]["th"] = 7.0
    m["kfs"][5]["flags"] = kcases.NOT_ERASE

    def p6(g0, g, d):
        assert len(d["kf_mp_row"]) == 0 and len(d["point_row"]) == 0 and list(d["kf_link_row"]) == [0, 1, 2, 3, 4, 5]
        assert list(g["kf_child"][g["kf_child_off"][0]:g["kf_child_off"][1]]) == [1, 3, 4]   # stored in ascending row
        assert list(d["kf_child"][:3]) == [4, 3, 1] and np.array_equal(g["kf_mp"], g0["kf_mp"]) and np.array_equal(g["obs_kf"], g0["obs_kf"])
    out.append(case("links_only", m0, m, p6, name_links=range(6)))

    # 7. the empty delta
    def p7(g0, g, d):
        assert len(d["point_row"]) == 0 and len(d["kf_mp_row"]) == 0 and len(d["kf_link_row"]) == 0
        assert ref.same_graph(g, ref.stored(g0)) is None
    out.append(case("empty_delta", m0, copy.deepcopy(m0), p7))

    # 8. a delta onto the empty map (a handle that holds no view)
    def p8(g0, g, d):
        assert g0["n_points"] == 0 and g0["n_keyframes"] == 0 and g["n_keyframes"] == 6 and d["view"] is None
    out.append(case("onto_empty_map", dict(pts=[], kfs=[]), m0, p8, with_view=False))
    return out


def empty_map():
    return to_arrays(dict(pts=[], kfs=[]))


def random_map(rng):
    """a map of tests/keyframe_culling_cases.py's generator with a spanning tree and covisibility lists -> model"""
    c = kcases.random_case(int(rng.integers(1, 1 << 30)))
    m = to_model(c["g"], c["v"])
    nk = len(m["kfs"])
    for k in range(nk):
        m["kfs"][k]["best"] = [j for j in (k - 1, k + 1, k - 2, k + 2, k + 3) if 0 <= j < nk]
        m["kfs"][k]["parent"] = k - 1 if k else -1
        m["kfs"][k]["children"] = [k + 1] if k + 1 < nk else []
    return m


def random_delta(rng, g, v):
    """one pass of LocalMapping::Run on the map (g, v): a keyframe inserted (ProcessNewKeyFrame, CreateNewMapPoints), points culled
    (MapPointCulling), points fused into others (SearchInNeighbors), one keyframe culled (KeyFrameCulling) -> (delta, graph after,
    view after)"""
    m0 = to_model(g, v)
    m = copy.deepcopy(m0)
    pts, kfs = m["pts"], m["kfs"]
    nk, npnt = len(kfs), len(pts)
    good = [p for p in range(npnt) if not pts[p]["bad"]]

    def erase(p, k):   # MapPoint::EraseObservation
        for j, (kf, i) in enumerate(pts[p]["obs"]):
            if kf == k:
                pts[p]["nobs"] -= 2 if kfs[k]["feats"][i][3] else 1
                pts[p]["obs"].pop(j)
                return

    def unmatch(p):   # the point leaves the features of every keyframe that lists it
        for kf, i in pts[p]["obs"]:
            if kfs[kf]["feats"][i][0] == p:
                kfs[kf]["feats"][i] = (-1,) + kfs[kf]["feats"][i][1:]

    # insert: a keyframe of 12-40 features, two thirds matched to points of the last keyframes, a few new points, two empty slots
    nf = int(rng.integers(12, 41))
    near = [p for p in good if any(kf >= nk - 3 for kf, _ in pts[p]["obs"])] or good
    feats = []
    seen = set()
    n_new = int(rng.integers(1, 6))
    pts += [dict(EMPTY_POINT) for _ in range(n_new + 2)]
    for i in range(nf):
        u = rng.random()
        p = -1
        if u < 0.65 and near:
            p = int(near[int(rng.integers(0, len(near)))])
        elif u < 0.8:
            p = npnt + int(rng.integers(0, n_new))
        st = int(rng.random() < 0.3)
        feats.append((p, int(rng.integers(0, 4)), float(np.float32(rng.random() * 4)), st))
        if p >= 0 and p not in seen:
            seen.add(p)
            if p >= npnt and pts[p]["bad"]:
                pts[p] = dict(bad=0, nobs=0, obs=[])
            pts[p]["obs"].append((nk, i))
            pts[p]["nobs"] += 2 if st else 1
    parent = int(rng.integers(max(0, nk - 3), nk)) if nk else -1
    neigh = sorted({int(x) for x in rng.integers(max(0, nk - 8), nk, 5)}) if nk else []
    kfs.append(dict(bad=0, feats=feats, best=neigh[::-1], children=[], parent=parent, th=float(np.float32(2 + rng.random())), flags=0))
    if nk:
        kfs[parent]["children"] = kfs[parent]["children"] + [nk]
    for j in neigh:   # UpdateConnections: the new keyframe enters its neighbours' lists
        kfs[j]["best"] = ([nk] + [b for b in kfs[j]["best"] if b != nk])[:NB]
    # point culling: the point goes bad, its observations are erased, its features are freed
    for p in rng.permutation(good)[:int(rng.integers(2, 6))]:
        p = int(p)
        unmatch(p)
        pts[p] = dict(bad=1, nobs=0, obs=[])
    # fuse: b takes a's place in every keyframe that does not see b yet, a goes bad (MapPoint::Replace)
    live = [p for p in good if not pts[p]["bad"] and pts[p]["obs"]]
    for _ in range(int(rng.integers(1, 4))):
        if len(live) < 2:
            break
        a, b = (int(x) for x in rng.permutation(live)[:2])
        if pts[a]["bad"] or pts[b]["bad"]:
            continue
        have = {kf for kf, _ in pts[b]["obs"]}
        for kf, i in pts[a]["obs"]:
            if kfs[kf]["feats"][i][0] != a:
                continue
            if kf in have:
                kfs[kf]["feats"][i] = (-1,) + kfs[kf]["feats"][i][1:]
            else:
                kfs[kf]["feats"][i] = (b,) + kfs[kf]["feats"][i][1:]
                pts[b]["obs"].append((kf, i))
                pts[b]["nobs"] += 2 if kfs[kf]["feats"][i][3] else 1
                have.add(kf)
        pts[a] = dict(bad=1, nobs=0, obs=[])
    # one keyframe culled (KeyFrame::SetBadFlag): its observations erased, its children handed to its parent
    cand = [k for k in range(1, nk) if not kfs[k]["bad"] and not kfs[k]["flags"] & 2]
    if cand:
        k = int(cand[int(rng.integers(0, len(cand)))])
        for p in {f[0] for f in kfs[k]["feats"] if f[0] >= 0}:
            erase(p, k)
        par = kfs[k]["parent"]
        for c in kfs[k]["children"]:
            kfs[c]["parent"] = par
            if par >= 0:
                kfs[par]["children"] = kfs[par]["children"] + [c]
        if par >= 0:
            kfs[par]["children"] = [c for c in kfs[par]["children"] if c != k]
        kfs[k].update(bad=1, children=[], best=[])
        for j in range(len(kfs)):
            if k in kfs[j]["best"]:
                kfs[j]["best"] = [b for b in kfs[j]["best"] if b != k]
    d = delta_between(m0, m)
    g1, v1 = to_arrays(m)
    return d, ref.stored(g1), v1


SEQUENCE_SEEDS = (11, 12, 13)   # the sequences of the CPU and the GPU tests
SEQUENCE_LENGTH = 5


def sequence(seed):
    """-> the map (g, v) and SEQUENCE_LENGTH steps (delta, graph after, view after)"""
    rng = np.random.default_rng(seed)
    g, v = to_arrays(random_map(rng))
    g = ref.stored(g)
    steps, g0, v0 = [], g, v
    for _ in range(SEQUENCE_LENGTH):
        d, g1, v1 = random_delta(rng, g0, v0)
        steps.append((d, g1, v1))
        g0, v0 = g1, v1
    return g, v, steps


def row_changes(g0, g1):
    """what a delta did to the rows of the three CSR arrays: dict(grew, shrank, appended, stayed) of counts"""
    out = dict(grew=0, shrank=0, appended=0, stayed=0)
    for key in ("obs_off", "kf_mp_off", "kf_child_off"):
        a, b = np.diff(g0[key]), np.diff(g1[key])
        out["appended"] += len(b) - len(a)
        out["grew"] += int((b[:len(a)] > a).sum())
        out["shrank"] += int((b[:len(a)] < a).sum())
        out["stayed"] += int((b[:len(a)] == a).sum())
    return out


def seam_model(n_points, n_kfs, rng):
    """a map of exactly n_points points and n_kfs keyframes for the scan seams: keyframe k holds the points p with p % n_kfs == k (up
    to 16 of them, or all of them where the points are many) and one more feature without a point; every seventh point has no
    observation"""
    per_kf = max(16, n_points // max(n_kfs, 1) + 1)
    kfs = [dict(bad=0, feats=[], best=[j for j in (k - 1, k + 1) if 0 <= j < n_kfs], children=[k + 1] if k + 1 < n_kfs else [],
                parent=k - 1, th=2.0, flags=1 if k == 0 else 0) for k in range(n_kfs)]
    pts = []
    for p in range(n_points):
        k = p % max(n_kfs, 1)
        if n_kfs and p % 7 != 6 and len(kfs[k]["feats"]) < per_kf:
            kfs[k]["feats"].append((p, int(rng.integers(0, 4)), 1.0, int(rng.integers(0, 2))))
            pts.append(dict(bad=0, nobs=1, obs=[(k, len(kfs[k]["feats"]) - 1)]))
        else:
            pts.append(dict(bad=0, nobs=0, obs=[]))
    for k in kfs:
        k["feats"].append((-1, 0, -1.0, 0))
    return dict(pts=pts, kfs=kfs)


def seam_delta(m0, tile, rng):
    """names rows on both sides of every tile seam of both tables: point rows lose or gain an observation, keyframe link rows lose
    or gain children; appends two points and one keyframe"""
    m = copy.deepcopy(m0)
    pts, kfs = m["pts"], m["kfs"]
    npnt, nk = len(pts), len(kfs)

    def around(n):
        rows = {0, n - 1}
        for s in range(tile, n + tile, tile):
            rows |= {s - 1, s, s + 1}
        rows = sorted(r for r in rows if 0 <= r < n)
        if len(rows) > 48:   # (T * T + 1 rows: the first, the last and a spread of the seams)
            rows = rows[:16] + [rows[i] for i in sorted(rng.choice(np.arange(16, len(rows) - 16), 16, replace=False))] + rows[-16:]
        return rows
    feats = [(-1, 0, 1.0, 0)] * 4
    kfs.append(dict(bad=0, feats=feats, best=[nk - 1] if nk else [], children=[], parent=nk - 1, th=2.5, flags=0))
    for j, p in enumerate(around(npnt)):
        if pts[p]["obs"] and j % 2:
            pts[p]["obs"], pts[p]["nobs"] = [], 0
        else:
            pts[p]["obs"] = pts[p]["obs"] + [(nk, j % 4)]
            pts[p]["nobs"] += 1
    for j, k in enumerate(around(nk)):
        kfs[k]["children"] = [] if (kfs[k]["children"] and j % 2) else kfs[k]["children"] + [nk, 0]
        kfs[k]["best"] = [nk] + kfs[k]["best"]
    pts += [dict(bad=0, nobs=1, obs=[(nk, 1)]), dict(EMPTY_POINT)]
    return m
