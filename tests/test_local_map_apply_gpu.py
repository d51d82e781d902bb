"""aos2_local_map_apply on a resident graph (the rebuild on the device, csrc/local_map_apply.hip): the handle's snapshot and view,
downloaded, against tests/local_map_apply_ref.py, exactly; the applied handle against a NEW handle that was set to the reference's
graph, through the three consumers of the graph (aos2_local_map_update, the statistics, keyframe culling), byte for byte; the seams
of the multi-workgroup scan through the tile hook; the forced host path; the ordering contract; a refused delta."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import keyframe_culling_cases as kcases      # noqa: E402
import local_map_apply_cases as cases        # noqa: E402
import local_map_apply_ref as ref            # noqa: E402
import local_map_cases as lcases             # noqa: E402

PLANTED = cases.planted()
SEQUENCE_SEEDS, sequence = cases.SEQUENCE_SEEDS, cases.sequence

pytestmark = pytest.mark.gpu
GUARD, NG = 0x5A5A5A5A, 64
TILE = 64


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
            n_points = max(n_points, int(mp.max()) + 1)
            f = capi.Frames(B, cap)
            f.keep = (t.zeros((B, cap, 7), dtype=t.float32, device=self.dev), t.zeros((B, cap, 32), dtype=t.uint8, device=self.dev),
                      t.from_numpy(np.ascontiguousarray(n, np.int32)).to(self.dev), t.ones(max(n_points, 1), dtype=t.uint8, device=self.dev))
            f.build(self.ex, f.keep[0].data_ptr(), f.keep[1].data_ptr(), f.keep[2].data_ptr(), 640, 480, 0, 500.0, 500.0, 320.0, 240.0, 40.0)
            f.table = capi.map_points_dev(max(n_points, 1), 0, 0, f.keep[3].data_ptr())
            f.set_map_points(mp, f.table, outlier)
            return f

        def dev_i32(self, a):
            a = np.ascontiguousarray(a, np.int32).reshape(-1)
            return self.t.from_numpy(np.concatenate([a, np.full(NG, GUARD, np.int32)])).to(self.dev)

        def lists(self, B, local_cap, kf_cap):
            """the five device arrays of aos2_frames_update_local_map, no previous list"""
            return dict(local=self.dev_i32(np.full((B, local_cap), -9)), n_local=self.dev_i32(np.full(B, -9)),
                        local_kfs=self.dev_i32(np.full((B, kf_cap), -1)), n_local_kfs=self.dev_i32(np.zeros(B)), ref_kf=self.dev_i32(np.full(B, -1)))

        def enqueue(self, lm, f, d, local_cap, kf_cap):
            lm.update(f, d["local"].data_ptr(), local_cap, d["n_local"].data_ptr(), d["local_kfs"].data_ptr(), kf_cap,
                      d["n_local_kfs"].data_ptr(), d["ref_kf"].data_ptr())

        def read(self, d):
            out = {}
            for k, v in d.items():
                h = v.cpu().numpy()
                assert (h[-NG:] == GUARD).all(), k
                out[k] = h[:-NG]
            return out

        def resident(self, g, v):
            lm = self.capi.LocalMap()
            lm.set(g)
            if v is not None:
                lm.set_culling_view(v)
            return lm

        def consumers(self, lm, g, probe):
            """what the three readers of the resident graph give for the frames and candidates of `probe` -> dict of arrays"""
            n, mp, outlier, cand, monocular = probe
            local_cap, kf_cap = max(1, g["n_points"]), max(1, g["n_keyframes"])
            out = {"update/" + k: a for k, a in lm.update_host(n, mp, local_cap, kf_cap).items()}
            f = self.batch(n, mp, outlier, n_points=g["n_points"])
            stats, inc = self.dev_i32(np.full((len(n), 3), -9)), self.dev_i32(np.zeros(max(1, g["n_points"])))
            lm.stats(f, stats.data_ptr(), inc.data_ptr(), True, False)
            f.wait()
            out["stats"], out["found_inc"], out["stats/mp"] = stats.cpu().numpy(), inc.cpu().numpy(), f.get(self.capi.Frames.MAP_POINTS)
            f.close()
            if cand is not None:
                for k, a in lm.keyframe_culling(cand, monocular=monocular).items():
                    out["culling/" + k] = np.asarray(a)
            return out

    return Rig()


def probe_for(rng, g, view=True):
    """frames that look at the map, outlier flags, and the candidates of a culling call (every keyframe, in a random order)"""
    frames = lcases.random_frames(rng, g, 6, (0, 9, 40, 64, 65, 130))
    n, mp = lcases.frames_arrays(frames, cap=130)
    outlier = (rng.random(mp.shape) < 0.3).astype(np.uint8)
    cand = rng.permutation(g["n_keyframes"]).astype(np.int32) if view else None
    return n, mp, outlier, cand, int(rng.random() < 0.5)


def same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


def check(lm, g, v, what):
    got_g, got_v = lm.graph(), lm.view()
    assert ref.same_graph(got_g, g) is None, (what, ref.same_graph(got_g, g))
    assert ref.same_view(got_v, v) is None, (what, ref.same_view(got_v, v))


@pytest.mark.parametrize("c", PLANTED, ids=[c["name"] for c in PLANTED])
def test_planted_delta_on_the_device(rig, c):
    g, v = cases.want(c)
    lm = rig.resident(c["g"], c["v"])
    lm.apply(c["delta"])
    la = lm.last_apply()
    assert la["path"] == 1 and la["device_ms"] >= 0 and la["bytes"] > 0
    check(lm, g, v, c["name"])
    # ... and the graph that was downloaded is the one the kernels read
    rng = np.random.default_rng(3)
    probe = probe_for(rng, g, v is not None)
    fresh = rig.resident(g, v)
    same_bytes(rig.consumers(lm, g, probe), rig.consumers(fresh, g, probe), c["name"])
    fresh.close()
    lm.close()


def delta_block_bytes(d):
    """the block a device rebuild uploads: every array at the next 256-byte boundary -- per row set its row
    list and then its arrays, the graph's part first, the view's behind it"""
    npr, nmr, nlr = len(d["point_row"]), len(d["kf_mp_row"]), len(d["kf_link_row"])
    n_obs, n_mp, n_child = (int(d[k][-1]) if len(d[k]) else 0 for k in ("obs_off", "kf_mp_off", "kf_child_off"))
    sizes = [4 * npr, npr, 4 * npr, 4 * (npr + 1), 4 * n_obs,                        # point_row, point_bad, point_nobs, obs_off, obs_kf
             4 * nmr, 4 * (nmr + 1), 4 * n_mp,                                       # kf_mp_row, kf_mp_off, kf_mp
             4 * nlr, nlr, 40 * nlr, 4 * (nlr + 1), 4 * n_child, 4 * nlr]            # kf_link_row, kf_bad, kf_best, kf_child_off, kf_child, kf_parent
    if d.get("view") is not None:
        sizes += [4 * n_obs, n_mp, 4 * n_mp, n_mp, 4 * nlr, nlr]                     # obs_idx, kf_octave, kf_depth, kf_stereo, kf_th_depth, kf_flags
    size = 0
    for b in sizes:
        size = ((size + 255) & ~255) + b
    return size


def test_uploaded_bytes_are_the_delta_block(rig):
    """aos2_local_map_last_apply_bytes pins the layout of the delta through the real call: the planted delta that appends a keyframe
    (all three row sets, with the view), then an empty delta -- zero rows, so three offsets arrays of one entry each"""
    c = next(c for c in PLANTED if c["name"] == "append_keyframe")
    d = c["delta"]
    assert c["v"] is not None and d["view"] is not None and min(len(d[k]) for k in ("point_row", "kf_mp_row", "kf_link_row")) > 0
    g, v = cases.want(c)
    lm = rig.resident(c["g"], c["v"])
    lm.apply(d)
    la = lm.last_apply()
    assert la["path"] == 1 and la["bytes"] == delta_block_bytes(d)
    empty = cases.delta_between(cases.to_model(g, v), cases.to_model(g, v))
    assert len(empty["point_row"]) == len(empty["kf_mp_row"]) == len(empty["kf_link_row"]) == 0 and empty["view"] is not None
    lm.apply(empty)
    la = lm.last_apply()
    assert la["path"] == 1 and la["bytes"] == delta_block_bytes(empty) == 768   # (obs_off at 0, kf_mp_off at 256, kf_child_off at 512)
    check(lm, g, v, "empty delta")
    lm.close()


@pytest.mark.parametrize("seed,peek", [(SEQUENCE_SEEDS[0], True), (SEQUENCE_SEEDS[1], False), (SEQUENCE_SEEDS[2], False)])
def test_sequence_equals_a_fresh_upload(rig, seed, peek):
    """after every delta of a sequence the applied handle and a NEW handle set to the reference's graph give the same bytes through
    every consumer; with `peek` the snapshot is downloaded and compared after every delta, without it only at the end (the host copy
    stays stale across rebuilds).  Five deltas use both device blocks at least twice."""
    g, v, steps = sequence(seed)
    rng = np.random.default_rng(seed)
    lm = rig.resident(g, v)
    reallocated, culled = 0, 0
    assert len(steps) >= 4
    for i, (d, _, _) in enumerate(steps):
        g, v = ref.apply(g, v, d)
        lm.apply(d)
        la = lm.last_apply()
        assert la["path"] == 1, (seed, i)
        reallocated += la["reallocated"]
        if peek:
            check(lm, g, v, (seed, i))
        probe = probe_for(rng, g)
        fresh = rig.resident(g, v)
        want = rig.consumers(fresh, g, probe)
        same_bytes(rig.consumers(lm, g, probe), want, (seed, i))
        culled += int((want["culling/status"] == kcases.CULLED).sum())
        fresh.close()
    assert reallocated >= 1 and reallocated < len(steps)   # (the blocks grow with slack: not every delta allocates)
    assert culled > 0                                       # the culling calls did cull
    check(lm, g, v, (seed, "end"))
    lm.close()


@pytest.mark.parametrize("n_points,n_kfs", [(n, 5) for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TILE * TILE + 1)] +
                         [(50, n) for n in (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, TILE * TILE + 1)])
def test_scan_seams(rig, n_points, n_kfs):
    """a workgroup scans TILE rows: tables of 1, TILE - 1, TILE, TILE + 1, 2 TILE + 1 rows, and TILE * TILE + 1, where the pass over
    the workgroups' totals loops; the delta names rows on both sides of every seam.  Two deltas: both blocks."""
    rng = np.random.default_rng(1000 * n_points + n_kfs)
    m0 = cases.seam_model(n_points, n_kfs, rng)
    g, v = cases.to_arrays(m0)
    g = ref.stored(g)
    lm = rig.resident(g, v)
    lm.debug_apply_tile(TILE)
    for step in range(2):
        m1 = cases.seam_delta(m0, TILE, rng)
        d = cases.delta_between(m0, m1)
        rows, n = (d["point_row"], len(m0["pts"])) if n_kfs == 5 else (d["kf_link_row"], len(m0["kfs"]))
        for s in range(TILE, n, TILE):   # both sides of every seam are named (of a spread of them where there are 64)
            if n <= 4 * TILE:
                assert s - 1 in rows and s in rows
        assert 0 in rows and n - 1 in rows
        g, v = ref.apply(g, v, d)
        lm.apply(d)
        assert lm.last_apply()["path"] == 1
        check(lm, g, v, (n_points, n_kfs, step))
        m0 = m1
    lm.close()


def test_forced_host_path_and_the_upload_after_it(rig):
    g, v, steps = sequence(SEQUENCE_SEEDS[0])
    rng = np.random.default_rng(5)
    lm = rig.resident(g, v)
    lm.apply(steps[0][0])                     # the host copy is stale when the tap is called
    g, v = ref.apply(g, v, steps[0][0])
    assert lm.last_apply()["path"] == 1
    lm.apply_host(steps[1][0])
    g, v = ref.apply(g, v, steps[1][0])
    assert lm.last_apply()["path"] == 0
    probe = probe_for(rng, g)
    fresh = rig.resident(g, v)
    same_bytes(rig.consumers(lm, g, probe), rig.consumers(fresh, g, probe), "after the tap")   # (the consumers re-uploaded everything)
    fresh.close()
    check(lm, g, v, "after the tap")
    lm.apply(steps[2][0])                     # resident again: the device path
    g, v = ref.apply(g, v, steps[2][0])
    assert lm.last_apply()["path"] == 1
    check(lm, g, v, "device after host")
    lm.close()


def test_view_and_graph_set_behind_a_rebuild(rig):
    """aos2_local_map_set_culling_view checks against the host copy, which a rebuild leaves stale: it is downloaded first; and an
    aos2_local_map_set behind a rebuild replaces everything"""
    c = next(c for c in PLANTED if c["name"] == "append_keyframe")
    g, v = cases.want(c)
    lm = rig.resident(c["g"], None)
    lm.apply(dict(c["delta"], view=None))
    assert lm.last_apply()["path"] == 1 and lm.view() is None
    bad = dict(v, obs_idx=v["obs_idx"].copy())
    bad["obs_idx"][-1] = 6                        # the last entry observes the APPENDED keyframe of 6 features: only the new graph knows it
    with pytest.raises(rig.capi.AosError) as e:
        lm.set_culling_view(bad)
    assert e.value.code == rig.capi.AOS2_ERR_ARG and v["obs_idx"][-1] < 6 and g["obs_kf"][-1] == 6
    lm.set_culling_view(v)
    check(lm, g, v, "view behind a rebuild")
    rng = np.random.default_rng(23)
    probe = probe_for(rng, g)
    fresh = rig.resident(g, v)
    same_bytes(rig.consumers(lm, g, probe), rig.consumers(fresh, g, probe), "view behind a rebuild")
    lm.apply(cases.delta_between(cases.to_model(g, v), cases.to_model(g, v)))   # the empty delta, with the view: every array as it was
    assert lm.last_apply()["path"] == 1
    same_bytes(rig.consumers(lm, g, probe), rig.consumers(fresh, g, probe), "empty delta")
    fresh.close()
    lm.set(c["g"])                               # a whole new graph behind two rebuilds; the view is dropped
    check(lm, ref.stored(c["g"]), None, "set behind a rebuild")
    lm.close()


def test_ordering_of_enqueued_work(rig):
    """an update enqueued BEFORE aos2_local_map_apply and not waited for sees the old graph, one enqueued after it the new one"""
    g, v, steps = sequence(SEQUENCE_SEEDS[1])
    d = steps[0][0]
    g1, _ = ref.apply(g, v, d)
    rng = np.random.default_rng(9)
    n, mp = lcases.frames_arrays(lcases.random_frames(rng, g, 8, (40, 64, 130)), cap=130)
    local_cap, kf_cap = g1["n_points"], g1["n_keyframes"]
    lm = rig.resident(g, v)
    old, new = rig.resident(g, v), rig.resident(g1, None)
    want_old, want_new = old.update_host(n, mp, local_cap, kf_cap), new.update_host(n, mp, local_cap, kf_cap)
    assert want_old["local"].tobytes() != want_new["local"].tobytes()   # (the delta changes what the frames see)
    f = rig.batch(n, mp, n_points=g1["n_points"])
    before, after = rig.lists(len(n), local_cap, kf_cap), rig.lists(len(n), local_cap, kf_cap)
    rig.enqueue(lm, f, before, local_cap, kf_cap)
    lm.apply(d)                                    # at once: no wait on the batch's stream
    f.set_map_points(mp, f.table)
    rig.enqueue(lm, f, after, local_cap, kf_cap)
    f.wait()
    for got, want in ((rig.read(before), want_old), (rig.read(after), want_new)):
        for k in ("local", "n_local", "local_kfs", "n_local_kfs", "ref_kf"):
            assert np.array_equal(got[k], want[k].reshape(-1)), k
    f.close()
    for h in (lm, old, new):
        h.close()


def test_refused_delta_leaves_the_resident_graph(rig):
    capi = rig.capi
    g, v, steps = sequence(SEQUENCE_SEEDS[2])
    rng = np.random.default_rng(17)
    lm = rig.resident(g, v)
    lm.apply(steps[0][0])
    g, v = ref.apply(g, v, steps[0][0])
    probe = probe_for(rng, g)
    want = rig.consumers(lm, g, probe)
    bad = dict(steps[1][0])
    bad["obs_kf"] = bad["obs_kf"].copy()
    bad["obs_kf"][-1] = bad["n_keyframes"]            # a value outside the new count, at the end of the delta
    with pytest.raises(capi.AosError) as e:
        lm.apply(bad)
    assert e.value.code == capi.AOS2_ERR_ARG and lm.last_apply()["path"] == 1
    same_bytes(rig.consumers(lm, g, probe), want, "after the refusal")
    check(lm, g, v, "after the refusal")
    lm.apply(steps[1][0])                              # and the valid delta goes through
    g, v = ref.apply(g, v, steps[1][0])
    check(lm, g, v, "valid")
    lm.close()
