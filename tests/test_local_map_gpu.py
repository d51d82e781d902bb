"""Tracking::UpdateLocalMap on the device (aos2_frames_update_local_map, aos2_frames_track_local_map_stats; csrc/local_map.hip)
against the line-by-line restatement tests/local_map_ref.py: every output equal as integers.  The planted cases of
tests/local_map_cases.py (each proves on the restatement's result that its branch was taken), the shapes at the kernels' seams,
both counter forms, grouped batches, the hand-over to aos2_frames_search_local_points, the statistics, a random sweep."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import local_map_cases as cases   # noqa: E402
import local_map_ref as ref       # noqa: E402

pytestmark = pytest.mark.gpu
KEYS = ("mp", "local", "n_local", "local_kfs", "n_local_kfs", "ref_kf")
PLANTED = cases.planted()
GUARD, NG = 0x5A5A5A5A, 64


@pytest.fixture(scope="module")
def rig(pkg, gpu):
    import torch

    class Rig:
        capi = pkg.capi
        t = torch
        dev = torch.device("cuda", gpu)
        ex = pkg.capi.Extractor(nfeatures=500)

        def batch(self, n, mp, outlier=None, n_points=1):
            """a frame batch whose frames have n [B] features and the map points mp [B][cap]"""
            B, cap = mp.shape
            t, capi = self.t, self.capi
            n_points = max(n_points, int(mp.max()) + 1)   # (Observations() > 0 of every row the frames name)
            f = capi.Frames(B, cap)
            f.keep = (t.zeros((B, cap, 7), dtype=t.float32, device=self.dev), t.zeros((B, cap, 32), dtype=t.uint8, device=self.dev),
                      t.from_numpy(np.ascontiguousarray(n, np.int32)).to(self.dev), t.ones(max(n_points, 1), dtype=t.uint8, device=self.dev))
            f.build(self.ex, f.keep[0].data_ptr(), f.keep[1].data_ptr(), f.keep[2].data_ptr(), 640, 480, 0, 500.0, 500.0, 320.0, 240.0, 40.0)
            f.table = capi.map_points_dev(max(n_points, 1), 0, 0, f.keep[3].data_ptr())
            f.set_map_points(mp, f.table, outlier)
            return f

        def dev_i32(self, a, guard=True):
            """a device copy of an int32 array with guard words behind it"""
            a = np.ascontiguousarray(a, np.int32).reshape(-1)
            h = np.concatenate([a, np.full(NG if guard else 0, GUARD, np.int32)])
            return self.t.from_numpy(h).to(self.dev)

        def update(self, c, lm=None, frames=None):
            """aos2_frames_update_local_map of a case -> the arrays it leaves (and the guard words checked)"""
            capi = self.capi
            own = lm is None
            if own:
                lm = capi.LocalMap()
                lm.set(c["g"])
            f = frames or self.batch(c["n"], c["mp"], n_points=c["g"]["n_points"])
            B = len(c["n"])
            d = dict(local=self.dev_i32(np.full((B, c["local_cap"]), -9)), n_local=self.dev_i32(np.full(B, -9)),
                     local_kfs=self.dev_i32(c["local_kfs"]), n_local_kfs=self.dev_i32(c["n_local_kfs"]), ref_kf=self.dev_i32(c["ref_kf"]))
            lm.update(f, d["local"].data_ptr(), c["local_cap"], d["n_local"].data_ptr(), d["local_kfs"].data_ptr(), c["kf_cap"],
                      d["n_local_kfs"].data_ptr(), d["ref_kf"].data_ptr())
            f.wait()
            out = {}
            for k, v in d.items():
                h = v.cpu().numpy()
                assert (h[-NG:] == GUARD).all(), k   # nothing behind an array is touched
                out[k] = h[:-NG].reshape(B, -1) if k in ("local", "local_kfs") else h[:-NG]
            out["mp"] = f.get(capi.Frames.MAP_POINTS)
            out["groups"] = lm.last_groups()
            if own:
                lm.close()
            if frames is None:
                f.close()
            return out

    return Rig()


def same(got, want, name=""):
    for k in KEYS:
        assert np.array_equal(got[k], want[k]), (name, k, got[k], want[k])


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_case(rig, c):
    same(rig.update(c), cases.want(c), c["name"])


def test_small_capacities_on_a_random_graph(rig):
    c = cases.random_case(21, 14, 60, 9, sizes=(8, 33, 64), local_cap=4, kf_cap=3)
    want = cases.want(c)
    assert (want["n_local"] > 4).any() and (want["n_local_kfs"] > 3).any()
    # the points behind the cut-off keyframes are counted: the first kf_cap keyframes alone hold fewer points
    g = c["g"]
    first3 = [{int(p) for k in kfs[:3] for p in g["kf_mp"][g["kf_mp_off"][k]:g["kf_mp_off"][k + 1]] if p >= 0 and not g["point_bad"][p]}
              for kfs in want["full_kfs"]]
    assert any(len(s) < want["n_local"][b] for b, s in enumerate(first3))
    same(rig.update(c), want)


def test_shapes_at_the_seams(rig):
    """frames of 0, 1, 63, 64, 65 and 257 features; batches of 1, 3 and 65; a frame alone and inside a mixed batch; two calls"""
    sizes = (0, 1, 63, 64, 65, 257)
    c = cases.random_case(31, 13, 80, 6, sizes=sizes, feats=(0, 40))
    assert tuple(c["n"]) == sizes
    want = cases.want(c)
    assert want["voted"].sum() >= 4 and not want["voted"][0]
    got = rig.update(c)
    same(got, want)
    again = rig.update(c)
    assert all(got[k].tobytes() == again[k].tobytes() for k in KEYS)   # two calls: identical bytes
    for b in range(6):   # alone = inside the mixed batch
        one = dict(c, n=c["n"][b:b + 1], mp=c["mp"][b:b + 1], local_kfs=c["local_kfs"][b:b + 1], n_local_kfs=c["n_local_kfs"][b:b + 1],
                   ref_kf=c["ref_kf"][b:b + 1])
        g1 = rig.update(one)
        assert all(g1[k][0].tobytes() == got[k][b].tobytes() for k in KEYS), b
    for B in (3, 65):
        cb = cases.random_case(32 + B, 13, 80, B, sizes=(5, 17, 64, 0, 33))
        same(rig.update(cb), cases.want(cb), f"batch {B}")


def test_counters_in_lds_and_in_global_memory(rig):
    """n_keyframes on both sides of the switch (moved down to 14 keyframes through the test hook), and the largest LDS form"""
    c = cases.random_case(41, 14, 90, 7, sizes=(9, 40, 64))
    want = cases.want(c)
    assert want["voted"].any() and (want["n_local_kfs"] > 0).any()
    for lds_kfs in (14, 13, 0):
        lm = rig.capi.LocalMap()
        lm.set(c["g"])
        lm.debug_limits(0, lds_kfs)
        same(rig.update(c, lm=lm), want, f"lds_keyframes {lds_kfs}")
        lm.close()
    for name in ("child_parent", "neighbours", "limit_80_overshoot", "no_votes", "all_voted_kfs_bad"):   # the expansion through global marks
        p = next(x for x in PLANTED if x["name"] == name)
        lm = rig.capi.LocalMap()
        lm.set(p["g"])
        lm.debug_limits(0, 0)
        same(rig.update(p, lm=lm), cases.want(p), name)
        lm.close()


def test_batch_in_groups_and_the_scratch_bound(rig):
    c = cases.random_case(51, 12, 70, 11, sizes=(12, 64, 30))
    want = cases.want(c)
    per_frame = 4 * (70 + 2 * 12) + 4
    lm = rig.capi.LocalMap()
    lm.set(c["g"])
    lm.debug_limits(3 * per_frame + 7, -1)   # three frames per group: 11 frames in 4 groups
    got = rig.update(c, lm=lm)
    assert got["groups"] == 4
    same(got, want)
    lm.debug_limits(per_frame, -1)
    got = rig.update(c, lm=lm)
    assert got["groups"] == 11
    same(got, want)
    lm.debug_limits(per_frame - 1, -1)   # one frame does not fit: refused before anything is enqueued
    with pytest.raises(rig.capi.AosError) as e:
        rig.update(c, lm=lm)
    assert e.value.code == rig.capi.AOS2_ERR_ARG
    lm.debug_limits(0, -1)
    got = rig.update(c, lm=lm)
    assert got["groups"] == 1
    same(got, want)
    lm.close()


def test_graph_replaced_and_empty_map(rig):
    a, b = cases.random_case(61, 9, 50, 4, sizes=(20,)), cases.random_case(62, 15, 30, 4, sizes=(20,))
    lm = rig.capi.LocalMap()
    for c in (a, b, a):
        lm.set(c["g"])
        same(rig.update(c, lm=lm), cases.want(c))
    e = cases.case("empty", cases.make_graph(0, []), [[0, -1, 3]], lambda r: None)
    lm.set(e["g"])
    same(rig.update(e, lm=lm), cases.want(e))
    lm.close()


def test_host_array_form(rig):
    """aos2_local_map_update: the same kernels on host arrays (the route of host/LocalMap.h)"""
    c = cases.random_case(95, 12, 60, 7, sizes=(0, 20, 64))
    want = cases.want(c)
    lm = rig.capi.LocalMap()
    lm.set(c["g"])
    same(lm.update_host(c["n"], c["mp"], c["local_cap"], c["kf_cap"], c["local_kfs"], c["n_local_kfs"], c["ref_kf"]), want)
    lm.close()


def test_track_local_map_stats(rig):
    rng = np.random.default_rng(71)
    g = cases.random_graph(rng, 10, 60)
    n, mp = cases.frames_arrays(cases.random_frames(rng, g, 9, (0, 5, 63, 64, 65, 257)), cap=257)
    outlier = (rng.random(mp.shape) < 0.3).astype(np.uint8)
    lm = rig.capi.LocalMap()
    lm.set(g)
    for stereo in (False, True):
        for only_tracking in (False, True):
            want = ref.stats_batch(g, n, mp, outlier, stereo, only_tracking)
            assert (want["mp"] != mp).any() == stereo and (want["stats"][:, 2] == 0).all() == only_tracking
            f = rig.batch(n, mp, outlier, n_points=60)
            stats, inc = rig.dev_i32(np.full((9, 3), -9)), rig.dev_i32(np.zeros(60))
            lm.stats(f, stats.data_ptr(), inc.data_ptr(), stereo, only_tracking)
            f.wait()
            hs, hi = stats.cpu().numpy(), inc.cpu().numpy()
            assert (hs[-NG:] == GUARD).all() and (hi[-NG:] == GUARD).all()
            assert np.array_equal(hs[:-NG].reshape(9, 3), want["stats"]) and np.array_equal(hi[:-NG], want["found_inc"])
            assert np.array_equal(f.get(rig.capi.Frames.MAP_POINTS), want["mp"])
            assert np.array_equal(f.get(rig.capi.Frames.OUTLIER), outlier)
            lm.stats(f, stats.data_ptr(), 0, stereo, only_tracking)   # without found_inc; the stereo discard has been made
            f.wait()
            again = ref.stats_batch(g, n, want["mp"], outlier, stereo, only_tracking)
            assert np.array_equal(stats.cpu().numpy()[:-NG].reshape(9, 3), again["stats"])
            f.close()
    lm.close()


@pytest.mark.parametrize("seed,nk,npnt,B,feats", [(81, 200, 5000, 128, (20, 120)), (82, 50, 800, 100, (0, 60)), (83, 12, 40, 65, (0, 24))])
def test_random_sweep(rig, seed, nk, npnt, B, feats):
    c = cases.random_case(seed, nk, npnt, B, sizes=(0, 3, 20, 64, 50, 31), feats=feats)
    want = cases.want(c)
    assert want["voted"].any() and (want["n_local"] > 0).any()
    same(rig.update(c), want)


def test_into_search_local_points_without_a_host_wait(pkg, rig):
    """aos2_frames_set_map_points, aos2_frames_update_local_map, then aos2_frames_search_local_points on the device-written list
    with nothing in between: the frames end with the bytes that uploading the restatement's list, padded with -1, gives."""
    capi, t, F = rig.capi, rig.t, rig.capi.Frames
    scen = pkg.scenario.tracking_scenario(3, 2, n_unique=2)
    tc = pkg.chain.TrackingChain(scen, n_local=600)
    B, cap, c, s = tc.B, tc.cap, tc.cur, scen
    tc.ex.extract_batch_device(tc.d_cur.data_ptr(), B, tc.W, tc.H, tc.W, tc.W * tc.H, tc.d_kps.data_ptr(), tc.d_desc.data_ptr(), cap, tc.d_n.data_ptr())
    c.build(tc.ex, tc.d_kps.data_ptr(), tc.d_desc.data_ptr(), tc.d_n.data_ptr(), tc.W, tc.H, tc.d_depth.data_ptr(),
            float(s["fx"]), float(s["fy"]), float(s["cx"]), float(s["cy"]), float(s["mbf"]))
    c.set_pose(tc.d_guess.data_ptr())
    c.SearchByProjectionLast(tc.last, tc.table, tc.th_last, mono=False, check_orientation=True)
    c.PoseOptimization(tc.table)
    c.discard_outliers()
    mp0, n = c.get(F.MAP_POINTS), tc.d_n.cpu().numpy()
    # a covisibility graph over the scenario's table: the local points of all frames dealt out to 8 keyframes in runs of 40
    n_points = int(tc.map["table"]["n"])
    loc = np.unique(np.concatenate([np.asarray(x).reshape(-1) for x in tc.map["local"]]))
    loc = loc[loc >= 0]
    kf_mp = [[] for _ in range(8)]
    for i, r in enumerate(loc):
        kf_mp[(i // 40) % 8].append(int(r))
    g = cases.make_graph(n_points, kf_mp, best={k: [(k + 1) % 8] for k in range(8)})
    local_cap = int(ref.update_batch(g, n, mp0, 1, 8)["n_local"].max()) + 17
    want = ref.update_batch(g, n, mp0, local_cap, 8)
    assert want["voted"].all() and (want["n_local"] > 100).all() and (want["n_local"] < local_cap).all()
    lm = capi.LocalMap()
    lm.set(g)
    d = dict(local=rig.dev_i32(np.full((B, local_cap), -9)), n_local=rig.dev_i32(np.zeros(B)), local_kfs=rig.dev_i32(np.full((B, 8), -1)),
             n_local_kfs=rig.dev_i32(np.zeros(B)), ref_kf=rig.dev_i32(np.full(B, -1)))
    c.set_map_points(mp0, tc.table)
    lm.update(c, d["local"].data_ptr(), local_cap, d["n_local"].data_ptr(), d["local_kfs"].data_ptr(), 8, d["n_local_kfs"].data_ptr(),
              d["ref_kf"].data_ptr())
    c.SearchLocalPoints(tc.table, d["local"].data_ptr(), local_cap, tc.th_local, tc.nnratio_local)
    c.wait()
    got = c.get(F.MAP_POINTS)
    assert np.array_equal(d["local"].cpu().numpy()[:-NG].reshape(B, local_cap), want["local"])
    up = rig.dev_i32(want["local"])
    c.set_map_points(want["mp"], tc.table)
    c.SearchLocalPoints(tc.table, up.data_ptr(), local_cap, tc.th_local, tc.nnratio_local)
    c.wait()
    by_upload = c.get(F.MAP_POINTS)
    assert got.tobytes() == by_upload.tobytes()
    assert (by_upload != want["mp"]).any()   # the list changed a feature's match
    lm.close()
