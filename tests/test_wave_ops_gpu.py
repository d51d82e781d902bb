"""csrc/wave_ops.h on its own (tap: aos2_debug_wave_ops_device): every wave / workgroup primitive against numpy, all
lanes, exact.  The integer results are integers; the f64 row sum is the same butterfly of two-operand additions in numpy
float64 (IEEE addition is commutative, so the bits agree); moves and readlanes are compared as bit patterns."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEAMS = (0, 15, 16, 31, 32, 47, 48, 63)   # row and half-wave seams: row_bcast:15 / :31, the readlanes of lanes 0 / 16 / 32 / 48
NTS = (128, 256)                          # the workgroup sizes the library instantiates block_excl_scan_i32 with
LANE = np.arange(64)
PERM = {"B1": LANE ^ 1, "4E": LANE ^ 2, "141": LANE ^ 7, "140": LANE ^ 15}   # quad swap, pair swap, half-row mirror, row mirror


def int_cases(nt, rng):
    """[cases][nt] int32, all >= 0: zero, one, a single non-zero at every seam of every wave, only the last thread, random < 2^20"""
    rows = [np.zeros(nt, np.int32), np.ones(nt, np.int32)]
    for w in range(nt // 64):
        for s in SEAMS:
            r = np.zeros(nt, np.int32)
            r[64 * w + s] = 7 + s
            rows.append(r)
    r = np.zeros(nt, np.int32)
    r[nt - 1] = 5
    rows.append(r)
    rows += [rng.integers(0, 1 << 20, nt).astype(np.int32) for _ in range(4)]
    return np.stack(rows)


def min_cases(nt, rng):
    """further cases for the unsigned min: all 0xFFFFFFFF, a duplicated minimum (in two rows, and twice in one row), keys above 2^31"""
    rows = [np.full(nt, 0xFFFFFFFF, np.uint32)]
    r = rng.integers(1000, 1 << 32, nt, dtype=np.uint64).astype(np.uint32)
    r[[3, 40]] = 17
    rows.append(r)
    r = rng.integers(1000, 1 << 32, nt, dtype=np.uint64).astype(np.uint32)
    r[[nt - 14, nt - 2]] = 5
    rows.append(r)
    return np.stack(rows)


def doubles(shape, rng):
    """mixed magnitude 1e-8 .. 1e8, both signs"""
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-8, 8, shape)


def waves(a):
    return a.reshape(a.shape[0], -1, 64)


def rows16(a):
    return a.reshape(a.shape[0], -1, 16)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def runs(pkg, gpu):
    """one launch per workgroup size; the inputs and what the device made of them, shared and left unchanged"""
    out = {}
    for nt in NTS:
        rng = np.random.default_rng(100 + nt)
        vi = int_cases(nt, rng)
        vu = min_cases(nt, rng)
        v = np.concatenate([vi, vu.view(np.int32)])
        d = doubles(v.shape, rng)
        d.view(np.uint64)[0, [0, 63]] = [0x8000000000000000, 0x7FF8DEADBEEF0001]   # readlane sources: -0.0, a NaN payload
        d.view(np.uint64)[1, [0, 63]] = [0xFFF0000000000001, 0x8000000000000000]   # a signalling NaN pattern, moved as bits
        out[nt] = dict(v=v, n_int=len(vi), d=d, got=pkg.capi.debug_wave_ops_device(v, d))
    return out


@pytest.mark.parametrize("nt", NTS)
def test_dpp_moves(runs, nt):
    r = runs[nt]
    v, d, got = waves(r["v"]), waves(r["d"]), r["got"]
    for name, perm in PERM.items():
        assert (waves(got["dpp_u32_" + name]) == v[..., perm]).all()
        assert (waves(got["dpp_i32_" + name]) == v[..., perm]).all()
        assert (bits(waves(got["dpp_f64_" + name])) == bits(d[..., perm])).all()


@pytest.mark.parametrize("nt", NTS)
def test_integer_sum_max_scan(runs, nt):
    r = runs[nt]
    n, got = r["n_int"], r["got"]
    v = r["v"][:n]
    assert (v >= 0).all()   # wave_max_i32's precondition
    want_row = np.broadcast_to(rows16(v).sum(-1, dtype=np.int32)[..., None], rows16(v).shape).reshape(v.shape)
    assert (got["row_sum"][:n] == want_row).all()
    for key, red in (("sum", np.sum), ("max", np.max)):
        want = np.broadcast_to(red(waves(v), axis=-1)[..., None], waves(v).shape).reshape(v.shape)
        assert (got[key][:n] == want).all(), key
    assert (waves(got["incl_scan"][:n]) == np.cumsum(waves(v), axis=-1, dtype=np.int32)).all()


@pytest.mark.parametrize("nt", NTS)
def test_unsigned_min(runs, nt):
    r = runs[nt]
    v, got = r["v"].view(np.uint32), r["got"]   # the integer cases and the min's own
    want_row = np.broadcast_to(rows16(v).min(-1)[..., None], rows16(v).shape).reshape(v.shape)
    want = np.broadcast_to(waves(v).min(-1)[..., None], waves(v).shape).reshape(v.shape)
    assert (got["row_min"] == want_row).all() and (got["min"] == want).all()
    assert (got["min"][r["n_int"]] == 0xFFFFFFFF).all() and got["min"][r["n_int"] + 1, 0] == 17


@pytest.mark.parametrize("nt", NTS)
def test_row_sum_f64_bits(runs, nt):
    r = runs[nt]
    x = waves(r["d"][2:]).copy()          # (the first two cases hold the NaNs of the readlane test)
    for perm in PERM.values():            # the order of wave_ops.h: 0xB1, 0x4E, 0x141, 0x140
        x = x + x[..., perm]
    assert (bits(waves(r["got"]["row_sum_f64"][2:])) == bits(x)).all()


@pytest.mark.parametrize("nt", NTS)
def test_readlane_f64_bits(runs, nt):
    r = runs[nt]
    d, got = waves(r["d"]), r["got"]
    for key, src in (("readlane_0", 0), ("readlane_63", 63)):
        want = np.broadcast_to(bits(d)[..., src:src + 1], d.shape)
        assert (bits(waves(got[key])) == want).all(), key
    assert bits(got["readlane_63"])[0, 0] == 0x7FF8DEADBEEF0001 and bits(got["readlane_0"])[0, 5] == 0x8000000000000000


@pytest.mark.parametrize("nt", NTS)
def test_block_excl_scan(runs, nt):
    r = runs[nt]
    n, got = r["n_int"], r["got"]
    v = r["v"][:n].astype(np.int64)
    incl = np.cumsum(v, axis=1)
    assert incl.max() < 2 ** 31
    assert (got["block_excl_scan"][:n] == incl - v).all()
    assert (got["block_total"][:n] == incl[:, -1:]).all()   # in every thread
    assert got["block_excl_scan"][2 + 8 * (nt // 64), nt - 1] == 0 and got["block_total"][2 + 8 * (nt // 64), 0] == 5   # only the last thread


@pytest.mark.parametrize("nt", NTS)
def test_block_sum(runs, nt):
    """block_sum_i32 twice in one kernel on the same LDS words: the tap returns sum(2 v) - sum(v), which is numpy's sum in
    every thread only if both calls are right -- the second one's stores wait behind the call's leading barrier for every
    wave's reads of the first"""
    r = runs[nt]
    n, got = r["n_int"], r["got"]
    want = np.sum(r["v"][:n], axis=1, dtype=np.int64)
    assert 2 * want.max() < 2 ** 31
    assert (got["block_sum"][:n] == want[:, None]).all()   # in every thread
    assert got["block_sum"][2 + 8 * (nt // 64), 0] == 5      # only the last thread
