"""Graphs and frames for the UpdateLocalMap tests (test_local_map_cpu.py, test_local_map_gpu.py): the planted cases, each with a
`prove` that asserts ON THE REFERENCE RESTATEMENT's result that its branch was taken, and seeded random graphs."""
import numpy as np

import local_map_ref as ref


def csr(lists):
    off = np.cumsum([0] + [len(x) for x in lists]).astype(np.int32)
    flat = np.array([v for x in lists for v in x], np.int32)
    return off, flat


def make_graph(n_points, kf_mp, obs=None, point_bad=(), point_nobs=None, kf_bad=(), best=None, children=None, parent=None):
    """kf_mp: one list of point rows (-1 = NULL) per keyframe.  obs: {point: [keyframes]}, default = the keyframes that list the
    point; point_nobs: {point: n}, default = the number of observations; best / children: {keyframe: [rows]}; parent: {kf: row}"""
    nk = len(kf_mp)
    derived = [[k for k in range(nk) if p in kf_mp[k]] for p in range(n_points)]
    o = [list((obs or {}).get(p, derived[p])) for p in range(n_points)]
    nobs = np.array([len(x) for x in o], np.int32)
    for p, v in (point_nobs or {}).items():
        nobs[p] = v
    pb, kb = np.zeros(n_points, np.uint8), np.zeros(nk, np.uint8)
    pb[list(point_bad)] = 1
    kb[list(kf_bad)] = 1
    bst = np.full((nk, 10), -1, np.int32)
    for k, v in (best or {}).items():
        bst[k, :len(v)] = v
    par = np.full(nk, -1, np.int32)
    for k, v in (parent or {}).items():
        par[k] = v
    g = dict(n_points=n_points, n_keyframes=nk, point_bad=pb, point_nobs=nobs, kf_bad=kb, kf_best=bst.reshape(-1), kf_parent=par)
    g["obs_off"], g["obs_kf"] = csr(o)
    g["kf_mp_off"], g["kf_mp"] = csr(kf_mp)
    g["kf_child_off"], g["kf_child"] = csr([list((children or {}).get(k, [])) for k in range(nk)])
    return g


def frames_arrays(frames, cap=None):
    """lists of point rows -> n [B], mp [B][cap] (-1 behind a frame's features)"""
    cap = cap or max(1, max(len(f) for f in frames))
    mp = np.full((len(frames), cap), -1, np.int32)
    for b, f in enumerate(frames):
        mp[b, :len(f)] = f
    return np.array([len(f) for f in frames], np.int32), mp


def case(name, g, frames, prove, local_cap=64, kf_cap=16, prev=None, cap=None):
    """prev: per frame (previous list, reference keyframe) or None"""
    n, mp = frames_arrays(frames, cap)
    B = len(frames)
    lk, nlk, rk = np.full((B, kf_cap), -1, np.int32), np.zeros(B, np.int32), np.full(B, -1, np.int32)
    for b, p in enumerate(prev or []):
        if p is not None:
            lk[b, :len(p[0])], nlk[b], rk[b] = p[0], len(p[0]), p[1]
    return dict(name=name, g=g, n=n, mp=mp, local_cap=local_cap, kf_cap=kf_cap, local_kfs=lk, n_local_kfs=nlk, ref_kf=rk, prove=prove)


def want(c):
    """the reference restatement's result for a case, proved to take the case's branch"""
    r = ref.update_batch(c["g"], c["n"], c["mp"], c["local_cap"], c["kf_cap"], c["local_kfs"], c["n_local_kfs"], c["ref_kf"])
    c["prove"](r)
    return r


def rows(r, b, what="local_kfs"):
    k = "n_local" if what == "local" else "n_local_kfs"
    return list(r[what][b, :r[k][b]])


def planted():
    out = []

    # 1. a bad point in the frame is nulled and does not vote: keyframe 2 is seen through the bad point 2 only
    g = make_graph(6, [[0, 1], [1, 3], [2, 4]], point_bad=[2])

    def p1(r):
        assert list(r["mp"][0]) == [0, -1, -1, 1] and rows(r, 0) == [0, 1] and r["voted"][0]
    out.append(case("bad_point", g, [[0, 2, -1, 1]], p1))

    # 2. no votes: all features NULL, all points bad, a point without observations, each with and without a previous list
    g = make_graph(8, [[0, 1, 6], [2, 3, 0], [4, 5]], point_bad=[4, 5], obs={6: []})

    def p2(r):
        assert not r["voted"].any()
        for b in (0, 2, 4):   # the previous list [1, 0] and its reference keyframe stand; the points come from it
            assert rows(r, b) == [1, 0] and r["ref_kf"][b] == 1 and rows(r, b, "local") == [2, 3, 0, 1, 6]
        for b in (1, 3, 5):
            assert r["n_local_kfs"][b] == 0 and r["n_local"][b] == 0 and (r["local"][b] == -1).all() and r["ref_kf"][b] == -1
        assert (r["mp"][2:4] == -1).all()
    fr = [[-1, -1, -1], [-1, -1, -1], [4, 5, 4], [5, 4, -1], [6], [6, -1]]
    out.append(case("no_votes", g, fr, p2, prev=[([1, 0], 1), None, ([1, 0], 1), None, ([1, 0], 1), None]))

    # 3. the bad keyframe 1 holds the most votes; 0 and 2 tie for the rest: the lower row is the reference keyframe
    g = make_graph(7, [[0, 1], [0, 1, 2, 3], [2, 3], [4]], kf_bad=[1])

    def p3(r):
        assert rows(r, 0) == [0, 2] and r["ref_kf"][0] == 0
    out.append(case("bad_kf_most_votes_and_tie", g, [[0, 1, 2, 3]], p3))
    g = make_graph(7, [[0, 1], [1, 2], [5, 6]], kf_bad=[0, 1])

    def p3b(r):   # every voted keyframe is bad: the list is emptied, the reference keyframe stays
        assert r["voted"][0] and r["n_local_kfs"][0] == 0 and (r["local_kfs"][0] == -1).all() and r["ref_kf"][0] == 2 and r["n_local"][0] == 0
    out.append(case("all_voted_kfs_bad", g, [[0, 1, 2]], p3b, prev=[([2], 2)]))

    # 4. neighbours: 0 skips 1 (in the list) and 3 (bad), takes 4 and not 5; 1 has two neighbours, 4 is in by now, takes 5
    g = make_graph(12, [[0], [1], [2], [3], [4], [5], [6]], kf_bad=[3], best={0: [1, 3, 4, 5, 6, 2, 1, 0, 3, 4], 1: [4, 5]})

    def p4(r):
        assert rows(r, 0) == [0, 1, 4, 5] and rows(r, 0, "local") == [0, 1, 4, 5]
    out.append(case("neighbours", g, [[0, 1]], p4))

    # 5. children of 0 = {3 (bad), 5, 6}: 5; its parent 7 is bad and is added; that ends the loop: 1's fresh neighbour 8 stays out
    g = make_graph(12, [[0], [1], [2], [3], [4], [5], [6], [7], [8]], kf_bad=[3, 7], children={0: [6, 3, 5]}, parent={0: 7}, best={1: [8]})

    def p5(r):
        assert rows(r, 0) == [0, 1, 5, 7] and rows(r, 0, "local") == [0, 1, 5, 7]
    out.append(case("child_parent", g, [[0, 1]], p5))
    # ... an added keyframe is not expanded: 2 joins as 0's neighbour, 2's neighbour 3, child 4 and parent 5 do not
    g = make_graph(8, [[0], [1], [2], [3], [4], [5]], best={0: [2], 2: [3]}, children={2: [4]}, parent={2: 5})

    def p5b(r):
        assert rows(r, 0) == [0, 2]
    out.append(case("added_not_expanded", g, [[0]], p5b))

    # 6. the limit of 80: V voted keyframes 0..V-1 observing point k each; keyframe k has the fresh neighbour 100 + k, the
    # child 200 + k and the parent 300 + k where asked for
    def chain(V, child, par):
        nk = 400
        kf_mp = [[k] if k < V else [] for k in range(nk)]
        return make_graph(V, kf_mp, best={k: [100 + k] for k in range(V)}, children={k: [200 + k] for k in range(V)} if child else None,
                          parent={k: 300 + k for k in range(V)} if par else None), [list(range(V))]

    def p6(nwant, tail):
        def prove(r):
            assert r["n_local_kfs"][0] == nwant and rows(r, 0)[-len(tail):] == tail, rows(r, 0)
        return prove
    for name, V, child, par, nwant, tail in (("limit_81_voted", 81, True, True, 81, [78, 79, 80]),
                                             ("limit_79_neighbours", 79, False, False, 81, [78, 100, 101]),
                                             ("limit_79_two_per_step", 79, True, False, 81, [78, 100, 200]),
                                             ("limit_80_overshoot", 80, True, True, 83, [79, 100, 200, 300])):
        g, fr = chain(V, child, par)
        out.append(case(name, g, fr, p6(nwant, tail), local_cap=128, kf_cap=96))

    # 7. local points: NULL slots, the bad point 5, point 7 in three keyframes, keyframe 1 without matches, point 9 without
    # observations, point 4 held by the frame, and the order of the list
    g = make_graph(10, [[-1, 4, 5, 7], [], [7, 4, 9, -1, 3], [7, 1]], point_bad=[5], obs={4: [0, 1, 2], 9: []}, point_nobs={9: 0},
                   best={0: [3]})

    def p7(r):
        assert rows(r, 0) == [0, 1, 2, 3] and rows(r, 0, "local") == [4, 7, 9, 3, 1] and 4 in r["mp"][0]
    out.append(case("local_points", g, [[4, -1]], p7))

    # 8. capacities below the counts (the planted graph of case 4 and a chain): true counts, the first rows
    g = make_graph(12, [[0], [1], [2], [3], [4], [5], [6]], kf_bad=[3], best={0: [1, 3, 4, 5, 6, 2, 1, 0, 3, 4], 1: [4, 5]})

    def p8(r):   # the fourth local point comes from the fourth keyframe, which kf_cap cuts off: the whole list was walked
        assert r["n_local_kfs"][0] == 4 and r["n_local"][0] == 4 and list(r["local_kfs"][0]) == [0, 1] and list(r["local"][0]) == [0, 1, 4]
        assert r["full_kfs"][0] == [0, 1, 4, 5]
    out.append(case("capacities", g, [[0, 1]], p8, local_cap=3, kf_cap=2))
    return out


def random_graph(rng, nk, n_points, feats=(0, 24)):
    kf_mp = []
    for k in range(nk):
        nf = int(rng.integers(feats[0], feats[1] + 1))
        rws = rng.integers(0, n_points, nf) if n_points else np.full(nf, -1, np.int64)
        rws = np.where(rng.random(nf) < 0.2, -1, rws)
        kf_mp.append([int(v) for v in rws])
    obs = {}
    for p in range(n_points):
        s = {k for k in range(nk) if p in kf_mp[k]} if nk <= 64 else set()
        obs[p] = s
    if nk > 64:   # (the inverse of kf_mp without the quadratic scan)
        for k, lst in enumerate(kf_mp):
            for p in lst:
                if p >= 0:
                    obs[p].add(k)
    for p in range(n_points):   # the observations need not mirror the matches: drop and add a few
        s = obs[p]
        if s and rng.random() < 0.1:
            s.discard(next(iter(s)))
        if nk and rng.random() < 0.1:
            s.add(int(rng.integers(0, nk)))
        obs[p] = sorted(s) if rng.random() < 0.5 else [int(v) for v in rng.permutation(sorted(s))]
    nobs = {p: (0 if rng.random() < 0.05 else len(obs[p]) + int(rng.integers(0, 3))) for p in range(n_points)}
    best, children, parent = {}, {k: [] for k in range(nk)}, {}
    for k in range(nk):
        others = [int(v) for v in rng.permutation(nk)[:int(rng.integers(0, 11))] if v != k]
        best[k] = others
        if k and rng.random() < 0.8:
            parent[k] = int(rng.integers(0, k)) if rng.random() < 0.9 else int(rng.integers(0, nk))
            children[parent[k]].append(k)
    children = {k: [int(v) for v in rng.permutation(v)] for k, v in children.items()}
    return make_graph(n_points, kf_mp, obs=obs, point_nobs=nobs, point_bad=np.flatnonzero(rng.random(n_points) < 0.1),
                      kf_bad=np.flatnonzero(rng.random(nk) < 0.1), best=best, children=children, parent=parent)


def random_frames(rng, g, B, sizes):
    """frames that look at the map around a few keyframes, with NULL features, bad points and strays"""
    frames = []
    mo, mm, nk, npnt = g["kf_mp_off"], g["kf_mp"], g["n_keyframes"], g["n_points"]
    for b in range(B):
        N = int(sizes[b % len(sizes)])
        pool = []
        for k in (rng.integers(0, nk, int(rng.integers(1, 4))) if nk else []):
            pool += [int(v) for v in mm[mo[k]:mo[k + 1]] if v >= 0]
        f = []
        for i in range(N):
            u = rng.random()
            f.append(-1 if (u < 0.3 or not npnt) else (int(pool[int(rng.integers(0, len(pool)))]) if (pool and u < 0.9) else int(rng.integers(0, npnt))))
        frames.append(f)
    return frames


def random_case(seed, nk, n_points, B, sizes, local_cap=None, kf_cap=None, feats=(0, 24)):
    rng = np.random.default_rng(seed)
    g = random_graph(rng, nk, n_points, feats)
    frames = random_frames(rng, g, B, sizes)
    c = case(f"random_{seed}", g, frames, lambda r: None, local_cap=local_cap or max(1, min(n_points, 4096)), kf_cap=kf_cap or max(1, nk))
    # a previous list for the frames that will not vote
    for b in range(B):
        k = int(rng.integers(0, min(c["kf_cap"], nk) + 1)) if nk else 0
        c["local_kfs"][b, :k] = rng.integers(0, nk, k) if nk else 0
        c["n_local_kfs"][b] = k
        c["ref_kf"][b] = int(rng.integers(-1, nk)) if nk else -1
    return c
