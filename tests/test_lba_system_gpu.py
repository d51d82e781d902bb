"""The assembly of LocalBA's reduced camera system alone -- k_lin (init), k_lm_init and one k_schur, through the tap
aos2_debug_lba_assemble_device, which runs the host phase of aos2_lba_solve_batch and enqueues the shipped kernels through its helpers --
against tests/lba_system_ref.py: the g2o operation in long double from the estimates and masks the tap returns, with a scale M per
entry.  The condition on every quantity: omega = |q_dev - q_ref| / (2^-53 M_q) <= 4 x the worst omega of two float64 models of the
assembly (the textbook form, the factored record form) over the same family of inputs; the models run here on the very inputs
(tests/test_lba_system_cpu.py runs them without a device and holds them to omega <= 16).

Worst omega per quantity over all families, float64 models on the CPU (textbook / records) and the device:
    quantity   textbook  records   device (measured on the MI355X)
    Hll        0.54      0.55      0.42
    b_l        0.39      0.41      0.35
    Hpp        0.45      0.53      0.37
    b_p        0.24      0.23      0.24 / 0.24
    Hs diag    4.1       4.4       0.97
    Hs off     7.0       7.0       7.0
    bs         0.13      0.15      0.14
    lambda     0.33      0.33      0.33
    chi2       0.0055    0.0055    0.0045
(chi2 and bs are sums with heavy cancellation inside every term -- e = obs - proj -- whose M is far above their error.)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_system_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

MARGIN = 4.0
_taps = {}


@pytest.fixture(scope="module")
def ba(pkg, gpu):
    return pkg.LocalBA()


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def lam_of(case):
    """the lambda a case of the lambda family passes: the factor times lambda_init at the host's estimates (any value would do: the
    reference takes the value that was passed)"""
    if case["lam_factor"] is None:
        return 0.0
    k = ("lambda_init", id(case["win"]))
    if k not in _taps:
        _taps[k] = float(S.linearise(case["win"], S.host_estimates(case["win"]), np.float64)["lambda"][0])
    return _taps[k] * case["lam_factor"]


def tap(ba, cases, layout="slots", key=None):
    """one tap call for all cases (kept per family and layout: several tests look at the same launch)"""
    if key is not None and (key, layout) in _taps:
        return _taps[(key, layout)]
    lam = np.array([lam_of(c) for c in cases])
    got = ba.debug_assemble([c["win"] for c in cases], layout=layout, stage=cases[0]["stage"], lam=lam if (lam > 0).any() else None)
    for c, g, v in zip(cases, got, lam):
        g["lam_passed"] = v if v > 0 else None
    if key is not None:
        _taps[(key, layout)] = got
    return got


def estimates(g):
    return dict(pose=g["pose"], point=g["point"], e_level1=g["e_level1"], e_robust=g["e_robust"])


def structure(case, g):
    """what is checked exactly: the index maps, the sizes, Hs symmetric bit for bit, zero beyond n, the identity tail, empty blocks
    zero; lambda = 1e-5 max |diag| of the device's own first linearisation bit for bit (or the value passed)"""
    name = f"{case['family']}/{case['name']}"
    hp, hl = S.index_maps(case["win"])
    assert g["np"] == len(hp) and g["nl"] == len(hl) and (g["hpose"] == hp).all() and (g["hpoint"] == hl).all(), name
    n = 6 * g["np"]
    assert g["npad"] == (n + 15) // 16 * 16, name
    Hs = g["Hs"]
    assert Hs.shape == (g["npad"], g["npad"]) and bits(Hs) == bits(Hs.T), f"{name}: Hs is not symmetric bit for bit"
    assert bits(Hs[:n, n:] + 0.0) == bits(np.zeros((n, g["npad"] - n))), f"{name}: columns beyond n"
    assert bits(Hs[n:, :]) == bits(np.eye(g["npad"])[n:, :]), f"{name}: identity tail"
    kinds, counts, n_pack, _ = S.unit_kinds(g["blk_off"], g["np"])
    for (i1, i2), cnt in counts.items():
        if cnt == 0 and i1 != i2:
            blk = Hs[6 * i1:6 * i1 + 6, 6 * i2:6 * i2 + 6]
            assert bits(blk + 0.0) == bits(np.zeros((6, 6))), f"{name}: empty block ({i1}, {i2}) [{kinds[(i1, i2)]}] is not zero"
    if g["lam_passed"] is None:
        d = np.concatenate([np.abs(g["Hpp_init"][:, range(6), range(6)]).ravel(), np.abs(g["Hll"][:, range(3), range(3)]).ravel()])
        assert bits(g["lam"]) == bits(1e-5 * d.max()), f"{name}: lambda {g['lam']!r} is not 1e-5 max |diag| = {1e-5 * d.max()!r}"
    else:
        assert bits(g["lam"]) == bits(g["lam_passed"]), f"{name}: lambda override"
    return kinds, counts, n_pack


def measure(case, g):
    """-> (device omegas {quantity: (omega, where)}, worst omegas of the float64 models {quantity: omega}, reference)"""
    ref, worst, _ = S.evaluate(case, estimates(g), g["lam_passed"])
    n = 6 * g["np"]
    dev = dict(Hll=g["Hll"], b_l=g["b_l"].reshape(-1, 3), Hpp=g["Hpp_init"], b_p=g["b_init"].reshape(-1, 6), Hs=g["Hs"][:n, :n], bs=g["bs"],
               chi2=g["current_chi"])
    if g["lam_passed"] is None:
        dev["lambda"] = g["lam"]
    om = S.omegas(ref, dev)
    om["b_p (DIAG)"] = S.omegas(ref, dict(b_p=g["b_p"].reshape(-1, 6)))["b_p"]   # the second form: k_schur's own sum
    return om, worst, ref


def check_family(family, cases, results):
    """the condition of the module docstring on every case of a family, the structure checks, the printed worst omegas"""
    tol, seen, bad = {}, {}, []
    measured = []
    for c, g in zip(cases, results):
        kinds, counts, _ = structure(c, g)
        om, worst, _ = measure(c, g)
        measured.append((c, om, kinds, counts))
        for q, v in worst.items():
            tol[q] = max(tol.get(q, 0.0), v)
    tol["b_p (DIAG)"] = tol["b_p"]
    for c, om, kinds, counts in measured:
        for q, (v, where) in om.items():
            if v > seen.get(q, (-1.0,))[0]:
                seen[q] = (v, c["name"], where)
            if not v <= MARGIN * tol[q]:
                at = ""
                if q.startswith("Hs"):
                    i1, i2 = (where[0], where[0]) if q == "Hs_diag" else where[:2]
                    key = (min(i1, i2), max(i1, i2))
                    at = f" block ({i1}, {i2}) entry {where[-2:]}, {counts[key]} items, {kinds[key]} unit"
                bad.append(f"{q}: omega {v:.3g} > {MARGIN:g} x {tol[q]:.3g} in window {family}/{c['name']} at {where}{at}")
    for q in sorted(seen):
        print(f"worst omega {family:8s} {q:11s} device {seen[q][0]:9.3g} (window {seen[q][1]}, at {seen[q][2]})   models {tol[q]:9.3g}")
    assert not bad, "\n".join(bad)


def test_item_counts_of_an_off_diagonal_block(ba):
    """np = 2 (+ two fixed keyframes), the landmarks both free keyframes see: 0 (the empty block, whose zeros are written), 1, 15, 16, 17,
    32, 33, 255, 256 (16 PACK rows: a whole unit), 257 (the first BIG block), 600 (three strides of a BIG unit).  Which unit kind a
    block got is read from the unit list the host phase built -- the rule of build_schur_units is restated in lba_system_ref.unit_kinds --
    so that PACK, BIG and DIAG units all ran is asserted, not assumed."""
    cases = S.cases("counts")
    got = tap(ba, cases, key="counts")
    ran = set()
    for c, g, n_co in zip(cases, got, S.COUNTS):
        kinds, counts, n_pack = structure(c, g)
        assert counts[(0, 1)] == n_co and kinds[(0, 1)] == ("BIG" if n_co > 256 else "PACK"), (c["name"], counts, kinds)
        unit_kind = g["units"] >> 28
        assert (unit_kind == 0).sum() == 2 and sorted(g["units"][unit_kind == 0] & 0xfffffff) == [0, 1], c["name"]
        assert (unit_kind == 1).sum() == (1 if n_co > 256 else 0) and (unit_kind == 2).sum() == n_pack == (0 if n_co > 256 else 1), c["name"]
        if n_co > 256:
            assert (g["units"][unit_kind == 1] & 0xfffffff).tolist() == [1], c["name"]   # block rank of (0, 1)
        ran |= {("DIAG", "BIG", "PACK")[k] for k in unit_kind}
        assert g["phase"] == 0 and g["trials_first"] == 0, c["name"]
    assert ran == {"DIAG", "BIG", "PACK"}
    check_family("counts", cases, got)


def test_pack_rows_of_21_blocks(ba):
    """np = 7: the 21 off-diagonal blocks' item counts are chosen so that a block's rows would straddle a unit (the unit is padded), a 16-row
    block arrives at in_unit = 0 and at in_unit > 0, empty blocks sit first, in the middle and last, and the last unit is partial."""
    cases = S.cases("pack")
    got = tap(ba, cases, key="pack")
    kinds, counts, n_pack, trace = S.unit_kinds(got[0]["blk_off"], got[0]["np"])
    off = [counts[p] for p in S.pairs_upper(S.PACK_NP)]
    assert tuple(off) == S.PACK_COUNTS and all(kinds[p] == "PACK" for p in S.pairs_upper(S.PACK_NP))
    assert any(pad and rows < 16 for _, _, rows, at, pad in trace), "no block straddles a unit"
    assert any(rows == 16 and at == 0 for _, _, rows, at, pad in trace) and any(rows == 16 and at > 0 and pad for _, _, rows, at, pad in trace)
    assert off[0] == 0 and off[-1] == 0 and 0 in off[5:15]
    last = trace[-1]
    assert (0 if last[4] else last[3]) + last[2] < 16, "the last unit is full"
    assert ((got[0]["units"] >> 28) == 2).sum() == n_pack >= 4
    check_family("pack", cases, got)


def test_diagonal_units_of_1_to_1025_observations(ba):
    """free keyframes with 1, 255, 256, 257 and 1025 observations: one stride of a DIAG unit, its boundary, and five strides.  Both forms of
    Hpp / b_p meet the condition against the reference -- lin_poses_body's (read between k_lm_init and k_schur) and the one the DIAG
    units re-form from the records (b_p as stored, Hpp inside the diagonal blocks of Hs) -- and are not compared with each other."""
    cases = S.cases("diag")
    got = tap(ba, cases, key="diag")
    _, counts, _, _ = S.unit_kinds(got[0]["blk_off"], got[0]["np"])
    assert tuple(counts[(i, i)] for i in range(len(S.DIAG_OBS))) == S.DIAG_OBS
    check_family("diag", cases, got)


def test_sizes_and_padding(ba):
    """np in {1, 3, 8, 40, 41, 43}: npad 16, 32, 48, 240 (no tail), 256, 272 -- on both sides of the two reduced-system kernels' ranges --
    with the exact checks of `structure` on the padded matrix."""
    cases = S.cases("sizes")
    got = tap(ba, cases, key="sizes")
    assert [g["np"] for g in got] == list(S.SIZES) and [g["npad"] for g in got] == [16, 32, 48, 240, 256, 272]
    check_family("sizes", cases, got)


@pytest.mark.parametrize("layout", ["slots", "walk"])
def test_landmark_degree(ba, layout):
    """observations per landmark 1 (mono only), 2, 4, 5, 6, 7, 8, 9, 17 and all 40 keyframes -- both sides of kLmSlots = 8, kWalkChunkLin = 4
    and kWalkChunkE = 6 --, a landmark seen only by fixed keyframes and one seen by one free and several fixed; both landmark layouts."""
    cases = S.cases("degree")
    got = tap(ba, cases, layout=layout, key="degree")
    w = cases[0]["win"]
    free_deg = np.bincount(w["edge_point"][w["pose_fixed"][w["edge_pose"]] == 0], minlength=w["n_points"])
    all_deg = np.bincount(w["edge_point"], minlength=w["n_points"])
    assert set(S.DEGREES) <= set(free_deg.tolist())
    assert ((free_deg == 0) & (all_deg >= 2)).any() and ((free_deg == 1) & (all_deg >= 4)).any()
    lone = np.nonzero(all_deg == 1)[0]
    assert len(lone) and not w["edge_stereo"][np.isin(w["edge_point"], lone)].any()
    check_family("degree", cases, got)


def test_edge_kinds_and_huber_sides(ba):
    """mono only, stereo only and mixed windows; the Huber kernel is on and at least 20 % of the active edges lie on each side of delta for
    the reference; depths span 0.5 .. 50 and |t| reaches 10."""
    cases = S.cases("kinds")
    got = tap(ba, cases, key="kinds")
    for c, g in zip(cases, got):
        st = c["win"]["edge_stereo"]
        assert {"mono": not st.any(), "stereo": st.all(), "mixed": 0.2 < st.mean() < 0.8}[c["name"]]
        assert g["e_robust"].all() and not g["e_level1"].any()
        lin = S.linearise(c["win"], estimates(g))
        frac = lin["beyond"][lin["active"]].mean()
        assert 0.2 <= frac <= 0.8, (c["name"], frac)
        d = lin["depth"].astype(np.float64)
        assert 0.5 <= d.min() < 1.5 and 25 < d.max() <= 50, (c["name"], d.min(), d.max())
        assert 6 < np.abs(g["pose"][:, 4:]).max() <= 10.5
    check_family("kinds", cases, got)


def test_lambda_override(ba):
    """{1e-8, 1, 1e4} x lambda_init on the windows of the item-count and the landmark-degree tests: the value is copied into the state behind
    k_lm_init, k_schur reads it (bit for bit what was passed) and the system meets the condition at that lambda -- 1e-8: the landmark
    blocks of once-seen mono landmarks are inverted at the edge of singularity."""
    cases = S.cases("lambda")
    got = tap(ba, cases, key="lambda")
    assert len(cases) == 3 * (len(S.COUNTS) + 1) and all(g["lam_passed"] is not None for g in got)
    check_family("lambda", cases, got)


def test_second_optimisation_with_masked_edges(ba, oracle):
    """stage 1: the first optimisation as aos2_lba_solve_batch enqueues it, the outlier pass, the start of the second optimisation, one
    k_schur -- on windows with planted gross outliers (+-60 .. 200 px): every observation of landmark 0, every observation of the lightly
    observed free keyframe 5, 3 % of the rest.  The masked set is the planted set, no edge is robust any more, every step of the first
    optimisation was accepted; the emptied keyframe's diagonal block is exactly lambda I, its off-diagonal blocks and its bs are zero,
    the emptied landmark's Hll is zero (up to the sign of a zero: a sum of masked items is +-0); everything else meets the condition."""
    cases = S.cases("stage1")
    got = tap(ba, cases, key="stage1")
    for c, g in zip(cases, got):
        w = c["win"]
        assert g["phase"] == 2 and g["trials_first"] == g["iters_done_first"] == 5, (c["name"], g["phase"], g["trials_first"], g["iters_done_first"])
        assert not g["e_robust"].any() and np.nonzero(g["e_level1"])[0].tolist() == c["planted"].tolist(), c["name"]
        assert g["e_level1"][w["edge_point"] == 0].all() and g["e_level1"][w["edge_pose"] == 5].all()
        assert 0 < (g["e_level1"] == 1).sum() - (w["edge_point"] == 0).sum() - (w["edge_pose"] == 5).sum()   # masked edges elsewhere too
        i = g["hpose"].tolist().index(5)
        l = g["hpoint"].tolist().index(0)
        n = 6 * g["np"]
        row = g["Hs"][6 * i:6 * i + 6, :n].copy()
        assert bits(row[:, 6 * i:6 * i + 6] + 0.0) == bits(g["lam"] * np.eye(6)), f"{c['name']}: the emptied keyframe's diagonal block is not lambda I"
        row[:, 6 * i:6 * i + 6] = 0
        assert bits(row + 0.0) == bits(np.zeros((6, n))) and bits(g["bs"][6 * i:6 * i + 6] + 0.0) == bits(np.zeros(6)), c["name"]
        assert bits(g["Hll"][l] + 0.0) == bits(np.zeros((3, 3))) and bits(g["b_l"].reshape(-1, 3)[l] + 0.0) == bits(np.zeros(3)), c["name"]
    check_family("stage1", cases, got)


def test_same_bits_across_layouts_batches_and_handles(pkg, ba):
    """Hll, b_l, Hs, bs, Hpp and b_p are bit for bit the same between the slots and the walk layout, between a window alone and the same window
    shuffled into a batch of mixed sizes, and between two handles."""
    pick = {"counts": ("co17", "co257", "co600"), "sizes": ("np1", "np8", "np41"), "degree": ("degree",), "pack": ("pack",)}
    cases = [c for f, names in pick.items() for c in S.cases(f) if c["name"] in names]
    rng = np.random.default_rng(10)
    cases = [cases[i] for i in rng.permutation(len(cases))]
    keys = ("Hll", "b_l", "Hs", "bs", "Hpp_init", "b_init", "b_p", "lam", "current_chi")
    base = tap(ba, cases, "slots")
    other = pkg.LocalBA()
    runs = {"walk layout": tap(ba, cases, "walk"), "second handle": tap(other, cases, "slots"),
            "alone": [tap(ba, [c], "slots")[0] for c in cases], "alone, walk, second handle": [tap(other, [c], "walk")[0] for c in cases]}
    other.close()
    for what, res in runs.items():
        for c, a, b in zip(cases, base, res):
            for k in keys:
                assert bits(a[k]) == bits(b[k]), f"{what}: {k} of window {c['family']}/{c['name']} differs"
