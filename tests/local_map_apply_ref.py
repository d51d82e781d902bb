"""aos2_local_map_apply (include/aos2.h) restated in plain Python from its semantics: the graph after the call is the graph before it
with every named row replaced by the delta's content and the tables extended to the new counts.  Works on the dicts of
tests/local_map_cases.py (graph) and tests/keyframe_culling_cases.py (view); written from the header's text, not from the C++."""
import numpy as np

NB = 10   # AOS2_LOCAL_MAP_NEIGHBOURS

GRAPH_KEYS = ("n_points", "n_keyframes", "point_bad", "point_nobs", "obs_off", "obs_kf", "kf_bad", "kf_mp_off", "kf_mp", "kf_best",
              "kf_child_off", "kf_child", "kf_parent")
VIEW_KEYS = ("obs_idx", "kf_octave", "kf_depth", "kf_stereo", "kf_th_depth", "kf_flags")
VIEW_DTYPES = dict(obs_idx=np.int32, kf_octave=np.int8, kf_depth=np.float32, kf_stereo=np.uint8, kf_th_depth=np.float32, kf_flags=np.uint8)


def _split(off, flat):
    return [list(flat[off[i]:off[i + 1]]) for i in range(len(off) - 1)]


def _join(rows, dtype=np.int32):
    off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    return off, np.array([x for r in rows for x in r], dtype)


def _d(delta, key, n=None):
    a = delta.get(key)
    return [] if a is None else list(np.asarray(a).reshape(-1))


def apply(g, v, d):
    """(graph, view or None, delta) -> (graph, view or None); the inputs are left alone"""
    np0, nk0, np1, nk1 = int(g["n_points"]), int(g["n_keyframes"]), int(d["n_points"]), int(d["n_keyframes"])
    assert np1 >= np0 and nk1 >= nk0
    dv = d.get("view")
    assert (v is None) == (dv is None)
    # the tables as lists of rows, extended: an appended point row is the empty slot until the delta names it
    obs = _split(g["obs_off"], g["obs_kf"]) + [[] for _ in range(np1 - np0)]
    bad = list(g["point_bad"]) + [1] * (np1 - np0)
    nobs = list(g["point_nobs"]) + [0] * (np1 - np0)
    mp = _split(g["kf_mp_off"], g["kf_mp"]) + [None] * (nk1 - nk0)
    child = _split(g["kf_child_off"], g["kf_child"]) + [None] * (nk1 - nk0)
    kbad = list(g["kf_bad"]) + [None] * (nk1 - nk0)
    best = [list(r) for r in np.asarray(g["kf_best"]).reshape(nk0, NB)] + [None] * (nk1 - nk0)
    parent = list(g["kf_parent"]) + [None] * (nk1 - nk0)
    if v is not None:
        idx = _split(g["obs_off"], v["obs_idx"]) + [[] for _ in range(np1 - np0)]
        octave, depth, stereo = (_split(g["kf_mp_off"], v[k]) + [None] * (nk1 - nk0) for k in ("kf_octave", "kf_depth", "kf_stereo"))
        th, flags = list(v["kf_th_depth"]) + [None] * (nk1 - nk0), list(v["kf_flags"]) + [None] * (nk1 - nk0)

    rows = _d(d, "point_row")
    d_obs = _split(d["obs_off"], d["obs_kf"]) if rows else []
    d_idx = _split(d["obs_off"], dv["obs_idx"]) if rows and dv is not None else []
    for s, r in enumerate(rows):
        obs[r], bad[r], nobs[r] = d_obs[s], d["point_bad"][s], d["point_nobs"][s]
        if dv is not None:
            idx[r] = d_idx[s]

    rows = _d(d, "kf_mp_row")
    d_mp = _split(d["kf_mp_off"], d["kf_mp"]) if rows else []
    for s, r in enumerate(rows):
        assert mp[r] is None or len(mp[r]) == len(d_mp[s])   # a keyframe's N never changes
        mp[r] = d_mp[s]
        if dv is not None:
            a, b = d["kf_mp_off"][s], d["kf_mp_off"][s + 1]
            octave[r], depth[r], stereo[r] = list(dv["kf_octave"][a:b]), list(dv["kf_depth"][a:b]), list(dv["kf_stereo"][a:b])

    rows = _d(d, "kf_link_row")
    d_child = _split(d["kf_child_off"], d["kf_child"]) if rows else []
    d_best = np.asarray(d["kf_best"]).reshape(-1, NB) if rows else []
    for s, r in enumerate(rows):
        kbad[r], best[r], child[r], parent[r] = d["kf_bad"][s], list(d_best[s]), d_child[s], d["kf_parent"][s]
        if dv is not None:
            th[r], flags[r] = dv["kf_th_depth"][s], dv["kf_flags"][s]
    assert all(x is not None for x in mp) and all(x is not None for x in child), "an appended keyframe is in both row sets"

    out = dict(n_points=np1, n_keyframes=nk1, point_bad=np.array(bad, np.uint8), point_nobs=np.array(nobs, np.int32),
               kf_bad=np.array(kbad, np.uint8), kf_best=np.array(best, np.int32).reshape(-1), kf_parent=np.array(parent, np.int32))
    out["obs_off"], out["obs_kf"] = _join(obs)
    out["kf_mp_off"], out["kf_mp"] = _join(mp)
    out["kf_child_off"], out["kf_child"] = _join([sorted(c) for c in child])   # stored in ascending row, as set stores them
    if v is None:
        return out, None
    view = dict(obs_idx=_join(idx)[1], kf_octave=_join(octave, np.int8)[1], kf_depth=_join(depth, np.float32)[1],
                kf_stereo=_join(stereo, np.uint8)[1], kf_th_depth=np.array(th, np.float32), kf_flags=np.array(flags, np.uint8))
    return out, view


def stored(g):
    """a graph as aos2_local_map_set stores it: the children of every keyframe in ascending row"""
    out = {k: (np.array(g[k]).copy() if k not in ("n_points", "n_keyframes") else int(g[k])) for k in GRAPH_KEYS}
    out["kf_child_off"], out["kf_child"] = _join([sorted(c) for c in _split(g["kf_child_off"], g["kf_child"])])
    return out


def same_graph(a, b):
    """the first key at which two graphs differ, None if none (exact equality, dtypes of the C arrays)"""
    for k in GRAPH_KEYS:
        if k in ("n_points", "n_keyframes"):
            if int(a[k]) != int(b[k]):
                return k
        elif not np.array_equal(np.asarray(a[k]), np.asarray(b[k])):
            return k
    return None


def same_view(a, b):
    if (a is None) != (b is None):
        return "view"
    if a is None:
        return None
    for k in VIEW_KEYS:   # bit for bit: the floats are moved, never computed
        x, y = np.ascontiguousarray(a[k], VIEW_DTYPES[k]), np.ascontiguousarray(b[k], VIEW_DTYPES[k])
        if x.shape != y.shape or x.tobytes() != y.tobytes():
            return k
    return None
