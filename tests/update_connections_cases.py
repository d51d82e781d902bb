"""Graphs and batches for the KeyFrame::UpdateConnections tests (test_update_connections_cpu.py, test_update_connections_gpu.py): the
planted cases, each with a `prove` that asserts ON THE REFERENCE RESTATEMENT's result that its branch was taken, the graphs of 300
keyframes with ordered lists of chosen lengths, and seeded random cases.  A case is a dict: g, kf, mp (None = the resident matches,
or one list per keyframe), th, conn_cap, ordered_cap."""
import numpy as np

import local_map_cases as lm
import update_connections_ref as ref


def stars(nk, centres, point_bad=(), kf_bad=(), own=True, twice=()):
    """Keyframe c (the index in `centres`) is to see keyframe r with weight centres[c][r]: it holds max-weight points, point j of
    which is observed by every r with weight > j (and by c itself, with own).  twice: centres that list their first point twice."""
    kf_mp = [[] for _ in range(nk)]
    obs, p = {}, 0
    for c, weights in enumerate(centres):
        for j in range(max(weights.values(), default=0)):
            seen = [r for r, w in sorted(weights.items()) if w > j]
            obs[p] = ([c] if own else []) + seen
            kf_mp[c].append(p)
            for r in seen:
                kf_mp[r].append(p)
            p += 1
        if c in twice and kf_mp[c]:
            kf_mp[c].append(kf_mp[c][0])
    return lm.make_graph(p, kf_mp, obs=obs, point_bad=point_bad, kf_bad=kf_bad)


def case(name, g, kf, prove, mp=None, th=3, conn_cap=16, ordered_cap=16):
    return dict(name=name, g=g, kf=list(kf), mp=mp, th=th, conn_cap=conn_cap, ordered_cap=ordered_cap, prove=prove)


def want(c):
    """the reference restatement's result for a case, proved to take the case's branch"""
    r = ref.update_connections(c["g"], c["kf"], c["mp"], c["th"], c["conn_cap"], c["ordered_cap"])
    c["prove"](r)
    return r


def planted():
    out = []

    # 1. the empty counter, three ways: no matches; only bad points; only observed by itself.  (Keyframe 3 sees 0 through point 4:
    # the observations need not mirror the matches.)
    g = lm.make_graph(5, [[], [0, 1, -1], [2, 3], [0, 4]], point_bad=[0, 1], obs={2: [2], 3: [2], 4: [0, 3]})

    def p1(r):
        assert r["counters"][:3] == [{}, {}, {}] and list(r["n_conn"]) == [0, 0, 0, 1] and list(r["n_ordered"]) == [0, 0, 0, 1]
        assert (r["conn_kf"][:3] == -1).all() and (r["ordered_w"][:3] == 0).all()
    out.append(case("empty_counter", g, [0, 1, 2, 3], p1))

    # 2. nothing >= th and a tie at the maximum: the LOWEST row is the single entry
    g = stars(5, [{1: 1, 2: 2, 3: 2, 4: 1}])

    def p2(r):
        assert r["counters"][0] == {1: 1, 2: 2, 3: 2, 4: 1} and r["ordered"][0] == [(2, 2)]
    out.append(case("tie_at_the_maximum_below_th", g, [0], p2, th=5))

    # 3. the same weights with th = 2: both tied keyframes are listed, the HIGHER row first
    def p3(r):
        assert r["ordered"][0] == [(3, 2), (2, 2)] and r["n_conn"][0] == 4
    out.append(case("ties_above_th", g, [0], p3, th=2))
    g3 = stars(9, [{8: 4, 2: 4, 5: 4, 3: 6, 7: 3, 6: 2}])

    def p3b(r):
        assert r["ordered"][0] == [(3, 6), (8, 4), (5, 4), (2, 4), (7, 3)]
    out.append(case("ties_above_th_three", g3, [0], p3b, th=3))

    # 4. weights exactly th and th - 1
    g = stars(4, [{1: 3, 2: 2, 3: 4}])

    def p4(r):
        assert r["ordered"][0] == [(3, 4), (1, 3)] and r["counters"][0][2] == 2 and list(r["conn_kf"][0][:3]) == [1, 2, 3]
    out.append(case("th_and_th_minus_1", g, [0], p4, th=3))

    # 5. the keyframe's own row among the observations is not counted; as a keyframe the graph does not know (-1) it is
    def p5(r):
        assert 0 not in r["counters"][0] and r["counters"][1][0] == 4 and r["ordered"][1][0] == (3, 4) and r["ordered"][1][1] == (0, 4)
    out.append(case("own_row_and_unknown_keyframe", g, [0, -1], p5, mp=[ref.resident_matches(g, 0)] * 2, th=3))

    # 6. a point listed twice counts twice and lifts keyframe 1 over th
    g = stars(3, [{1: 2, 2: 2}], twice=[0])

    def p6(r, g=g):
        assert r["counters"][0] == {1: 3, 2: 3} and r["ordered"][0] == [(2, 3), (1, 3)]
        once = ref.update_connections_one(g, 0, ref.resident_matches(g, 0)[:-1], 3)
        assert once[1] == [(1, 2)]   # (without the second listing nothing reaches th)
    out.append(case("point_listed_twice", g, [0], p6, th=3))

    # 7. -1, bad and >= n_points entries are skipped (explicit matches)
    g = stars(4, [{1: 2, 2: 1}, {3: 1}], point_bad=[1])

    def p7(r):
        assert r["counters"][0] == {1: 1, 2: 1, 0: 1} and r["counters"][1] == {1: 1, 2: 1}
    out.append(case("skipped_entries", g, [3, 0], p7, mp=[[-1, 1, 0, g["n_points"], g["n_points"] + 7], [0, -1, 1, 1 << 30]], th=1))

    # 8. a bad observer is counted, and a bad keyframe gets its connections
    g = stars(4, [{1: 3, 2: 1}, {0: 3}], kf_bad=[1])

    def p8(r):
        assert r["ordered"][0] == [(1, 6)] and r["ordered"][1] == [(0, 6)] and r["counters"][0][2] == 1
    out.append(case("bad_observer_and_bad_keyframe", g, [0, 1], p8, th=3))

    # 9. capacities below the counts, and 0 / NULL
    g = stars(8, [{1: 3, 2: 5, 3: 1, 4: 4, 5: 3, 6: 2, 7: 3}])

    def p9(r):
        assert r["n_conn"][0] == 7 and r["n_ordered"][0] == 5 and list(r["conn_kf"][0]) == [1, 2] and list(r["ordered_kf"][0]) == [2, 4, 7]
    out.append(case("small_capacities", g, [0], p9, th=3, conn_cap=2, ordered_cap=3))

    def p9b(r):
        assert r["n_conn"][0] == 7 and r["n_ordered"][0] == 5 and r["conn_kf"].size == 0 and r["ordered_kf"].size == 0
    out.append(case("zero_capacities", g, [0], p9b, th=3, conn_cap=0, ordered_cap=0))

    def p9c(r):   # one capacity exact, the other with room: the tail is -1 / 0
        assert list(r["ordered_kf"][0]) == [2, 4, 7, 5, 1] and list(r["conn_w"][0]) == [3, 5, 1, 4, 3, 2, 3, 0, 0]
    out.append(case("exact_and_roomy_capacities", g, [0], p9c, th=3, conn_cap=9, ordered_cap=5))

    # 10. the same row twice in a batch
    def p10(r):
        assert r["ordered"][0] == r["ordered"][2] and r["counters"][0] == r["counters"][2] and r["n_ordered"][0] == 5
        assert r["counters"][1][0] == 5
    out.append(case("same_row_twice", g, [0, 2, 0], p10, th=3))

    # 11. n == 0
    def p11(r):
        assert len(r["n_conn"]) == 0
    out.append(case("empty_batch", g, [], p11))
    return out


LIST_LENGTHS = (1, 2, 63, 64, 65, 257)


def long_lists(th=4, nk=300):
    """300 keyframes (the scan's tile of 256 is crossed); keyframe c < 6 has an ordered list of LIST_LENGTHS[c] entries over rows on
    both sides of row 256, weights th .. th + 2 (so every list holds ties); a seventh has one keyframe below th on each side"""
    rng = np.random.default_rng(300)
    centres = []
    for L in LIST_LENGTHS:
        rows = sorted(int(v) for v in rng.permutation(np.arange(8, nk))[:L])
        if L >= 2:
            rows[0], rows[-1] = 8, nk - 1
        w = {r: th + (i * 7 + r) % 3 for i, r in enumerate(rows)}
        for r in (9, 270):   # connected but not listed
            if r not in w:
                w[r] = th - 1
        centres.append(w)
    centres.append({40: th - 1, 280: th - 1, 290: 1})
    g = stars(nk, centres)

    def prove(r):
        assert list(r["n_ordered"]) == list(LIST_LENGTHS) + [1] and r["ordered"][6] == [(40, th - 1)]
        for c, L in enumerate(LIST_LENGTHS):
            rows = [row for row, _ in r["ordered"][c]]
            ws = [w for _, w in r["ordered"][c]]
            assert ws == sorted(ws, reverse=True) and r["n_conn"][c] >= L
            if L >= 2:
                assert min(rows) < 256 < max(rows)
            if L >= 63:
                assert any(a == b for a, b in zip(ws, ws[1:]))
        assert sum(int(r["n_conn"][c]) > L for c, L in enumerate(LIST_LENGTHS)) >= 4
    return case("long_lists", g, list(range(7)), prove, th=th, conn_cap=300, ordered_cap=260)


def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    nk = int(rng.integers(1, 40))
    n_points = int(rng.integers(0, 120))
    g = lm.random_graph(rng, nk, n_points, feats=(0, int(rng.integers(1, 60))))
    n = int(rng.integers(0, 9))
    explicit = bool(rng.integers(0, 2))
    kf = [int(v) for v in rng.integers(-1 if explicit else 0, nk, n)]
    mp = None
    if explicit:
        mp = []
        for k in range(n):
            m = int(rng.integers(0, 50))
            rows = rng.integers(-1, n_points + 3, m)
            if kf[k] >= 0 and rng.random() < 0.5:
                rows = np.concatenate([rows, ref.resident_matches(g, kf[k])]).astype(np.int64)
            mp.append([int(v) for v in rows])
    caps = [int(rng.integers(0, 4)) if rng.random() < 0.3 else nk + 2 for _ in range(2)]
    return case(f"random_{seed}", g, kf, lambda r: None, mp=mp, th=int(rng.integers(1, 7)), conn_cap=caps[0], ordered_cap=caps[1])
