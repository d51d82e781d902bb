"""row_sums_scatter_f64<K> of csrc/wave_ops.h on its own (tap: aos2_debug_row_sums_scatter_device): one wave, K values per lane,
every lane's slots back.  Expected: the tree of row_sum_f64 -- ((l0 + l1) + (l2 + l3)) + ((l4 + l5) + (l6 + l7)), the same for
lanes 8 .. 15, then the two halves -- in numpy float64, two-operand additions.  IEEE addition is commutative, so the bits agree
whichever lane of a pair adds: equality is bit for bit, for every value in the lane and slot the header's helper names, and every
slot of every lane is accounted for (the pairing restated here says which value it holds)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KS = (36, 42, 7)   # k_schur's PACK rows, workgroup_sum_k256 of k_schur / k_lin, an odd count (unpaired values at levels 0 and 3)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def inputs(K, rng):
    """[64][K]: exponents spread over 2^+-200, mixed signs, exact zeros of both signs, rows (of 16 lanes) of zeros"""
    v = rng.choice([-1.0, 1.0], (64, K)) * np.ldexp(rng.uniform(1.0, 2.0, (64, K)), rng.integers(-200, 201, (64, K)))
    z = rng.uniform(size=(64, K))
    v[z < 0.06] = 0.0
    v[(z >= 0.06) & (z < 0.12)] = -0.0
    v[16:32] = 0.0                   # a row of +0
    v[32:48, : K // 2] = -0.0        # half the values of a row: all -0 (the total is -0)
    v[48:64, 0] = np.ldexp(1.0, 200) * np.where(np.arange(16) % 2, -1.0, 1.0)   # total cancellation in the first level
    return v


def tree(v):
    """[4 rows][16 lanes][K] -> [4][K], the additions of row_sum_f64 as lane 0 of a row performs them"""
    a = v[:, 0::2] + v[:, 1::2]
    a = a[:, 0::2] + a[:, 1::2]
    a = a[:, 0::2] + a[:, 1::2]
    return a[:, 0] + a[:, 1]


def index_of(K, s, li):
    """the pairing restated: the value whose total sits in slot s of lane li of a row"""
    n = [K]
    for _ in range(3):
        n.append((n[-1] + 1) // 2)
    idx = s
    for level in (3, 2, 1, 0):
        idx = n[level] - 1 if n[level] % 2 and idx == n[level] // 2 else 2 * idx + ((li >> level) & 1)
    return idx


@pytest.fixture(scope="module")
def runs(pkg, gpu):
    out = {}
    for K in KS:
        v = inputs(K, np.random.default_rng(700 + K))
        got, owner = pkg.capi.debug_row_sums_scatter_device(v)
        out[K] = dict(v=v, got=got, owner=owner, want=tree(v.reshape(4, 16, K)))
    return out


@pytest.mark.parametrize("K", KS)
def test_every_total_in_the_lane_the_helper_names(runs, K):
    r = runs[K]
    got, owner, want = r["got"].reshape(4, 16, -1), r["owner"], r["want"]
    assert got.shape[2] == (K + 15) // 16
    assert ((owner[:, 0] >= 0) & (owner[:, 0] < 16) & (owner[:, 1] >= 0) & (owner[:, 1] < got.shape[2])).all()
    for i in range(K):
        li, s = owner[i]
        assert index_of(K, s, li) == i, (i, li, s)
        assert (bits(got[:, li, s]) == bits(want[:, i])).all(), f"value {i} in lane {li} slot {s}: {got[:, li, s]!r} != {want[:, i]!r}"


@pytest.mark.parametrize("K", KS)
def test_every_slot_of_every_lane(runs, K):
    """also the lanes that hold a second copy of a total (values unpaired at some level): the same bits"""
    r = runs[K]
    got, want = r["got"].reshape(4, 16, -1), r["want"]
    seen = set()
    for li in range(16):
        for s in range(got.shape[2]):
            i = index_of(K, s, li)
            assert 0 <= i < K
            seen.add(i)
            assert (bits(got[:, li, s]) == bits(want[:, i])).all(), f"lane {li} slot {s} (value {i})"
    assert seen == set(range(K))


def test_the_inputs_have_what_they_claim(runs):
    for K, r in runs.items():
        v = r["v"]
        e = np.frexp(v[v != 0])[1]
        assert e.min() < -150 and e.max() > 150 and (v > 0).any() and (v < 0).any()
        assert ((v == 0) & ~np.signbit(v)).any() and ((v == 0) & np.signbit(v)).any() and (v[16:32] == 0).all()
        assert (bits(r["want"][2, : K // 2]) == bits(-0.0)).all() and r["want"][3, 0] == 0.0
