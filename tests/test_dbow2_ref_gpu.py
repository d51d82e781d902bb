"""The HIP vocabulary path (csrc/vocabulary.hip: voc_descend_kernel, voc_assemble_kernel, both loaders, the binary writer,
score) against the reference's own DBoW2: the recorded fixtures tests/golden/dbow2_ref_*.npz always, and the live driver
oracle/_ref/dbow2_ref (a CPU process) on the full case list.  Cases, fixture layout and comparisons: tests/dbow2_cases.py.
Everything is bit for bit; nothing outside the repository tree is read."""
import numpy as np
import pytest

import dbow2_cases as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def impl(pkg, gpu):
    return D.Impl(pkg, False)


def _live_or_skip():
    if D.live_binary() is None:
        pytest.skip(D.SKIP_REASON)


def _check(impl, pkg, case, out, tmp_path):
    if case["binary"]:   # the file the reference loads is what our saveToBinaryFile writes for this tree
        voc, hdr = case["voc"], case["file"][16:24].view("<i4")
        V = pkg.Vocabulary()
        V.set_nodes(voc["k"], voc["L"], int(hdr[0]), int(hdr[1]), voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
        V.saveToBinaryFile(tmp_path / "ours.bin")
        D.same(np.frombuffer((tmp_path / "ours.bin").read_bytes(), np.uint8), case["file"], case["name"] + ": our writer's bytes")
    D.check_case(impl, case, out, tmp_path)


@pytest.mark.parametrize("fixture", D.FIXTURES)
def test_library_matches_recorded_reference(impl, pkg, tmp_path, fixture):
    for case, out in D.load_fixture(fixture):
        _check(impl, pkg, case, out, tmp_path)


@pytest.mark.parametrize("group", ["transform", "variants", "loader", "header", "score"])
def test_library_matches_live_reference(impl, pkg, tmp_path, group):
    _live_or_skip()
    cases = dict(transform=lambda: D.transform_cases(False), variants=lambda: D.variant_cases(False), loader=D.loader_cases,
                 header=D.header_cases, score=lambda: [D.score_case(False)])[group]()
    for case in cases:
        _check(impl, pkg, case, D.run_ref(case, tmp_path), tmp_path)


def _device_batch(pkg, case, out, frames, cap, levelsup, scoring=0, weighting=0):
    """transform_device on one batch whose frames are sets of `case` -> per frame the dict check_transform takes"""
    import torch
    dev = torch.device("cuda:0")
    voc = case["voc"]
    V = pkg.Vocabulary()
    V.set_nodes(voc["k"], voc["L"], scoring, weighting, voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
    B = len(frames)
    ns = np.array([len(case["sets"][s][0]) for s in frames], np.int32)
    assert ns.max() == cap and ns.min() == 0
    desc = np.full((B, cap, 32), 0xA5, np.uint8)     # rows past a frame's count hold junk, never read
    for b, s in enumerate(frames):
        desc[b, : ns[b]] = case["sets"][s][0]
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    d_desc, d_n = t(desc), t(ns)
    bw, bv, nb = z((B, cap), torch.int32), z((B, cap), torch.float64), z(B, torch.int32)
    fn, fo, fi, nf = z((B, cap), torch.int32), z((B, cap + 1), torch.int32), z((B, cap), torch.int32), z(B, torch.int32)
    wo, no = z((B, cap), torch.int32), z((B, cap), torch.int32)
    V.transform_device(B, d_desc.data_ptr(), d_n.data_ptr(), cap, levelsup, bw.data_ptr(), bv.data_ptr(), nb.data_ptr(),
                       fn.data_ptr(), fo.data_ptr(), fi.data_ptr(), nf.data_ptr(), wo.data_ptr(), no.data_ptr())
    torch.cuda.synchronize()
    h = lambda x: x.cpu().numpy()  # noqa: E731
    bw, bv, nb, fn, fo, fi, nf, wo, no = map(h, (bw, bv, nb, fn, fo, fi, nf, wo, no))
    res = []
    for b in range(B):
        kb, kf = int(nb[b]), int(nf[b])
        res.append(dict(bow_word=bw[b, :kb].view(np.uint32), bow_value=bv[b, :kb], fv_node=fn[b, :kf], fv_off=fo[b, : kf + 1],
                        fv_idx=fi[b, : fo[b, kf]], word_of=wo[b, : ns[b]].view(np.uint32), node_of=no[b, : ns[b]].view(np.uint32)))
    return res


def _device_case(tree, cap, scoring, weighting):
    """one batch: per-frame counts 0 ... cap across the workgroup, chunk and padding edges, one levelsup for all frames"""
    voc = D.make_tree(9, 10, 4, ragged=True) if tree == "ragged" else D.make_tree(1, 10, 3)
    counts = sorted({0, 1, 17, 255, 256, 257, 511, cap})
    sets = [(d, 2) for d, _ in D.descriptor_sets(voc, 90, counts=counts, n_all_lu=16)[: len(counts)]]
    rep = D.descriptor_sets(voc, 91, counts=(), n_all_lu=16)[-2]           # forty copies of one descriptor
    return D.make_case(f"device_{tree}_cap{cap}", voc, D.text_bytes(voc, scoring, weighting), 0, sets + [(rep[0], 2)])


# cap a power of two, and not; L1 / TF_IDF, and DOT_PRODUCT / TF, whose division by the frame's own BowVector size is
# the one value of the assembly that a neighbouring frame of the batch could leak into
@pytest.mark.parametrize("tree,cap,scoring,weighting", [("full", 512, 0, 0), ("ragged", 600, 5, 1)])
def test_transform_device_matches_live_reference(pkg, gpu, tmp_path, tree, cap, scoring, weighting):
    _live_or_skip()
    case = _device_case(tree, cap, scoring, weighting)
    out = D.run_ref(case, tmp_path)
    frames = list(range(len(case["sets"])))
    for b, got in enumerate(_device_batch(pkg, case, out, frames, cap, 2, scoring, weighting)):
        D.check_transform(got, out, frames[b], case["voc"]["L"], 2, case["name"])


def test_transform_device_matches_recorded_reference(pkg, gpu):
    """the recorded ragged tree: its sets with levelsup 2 as one batch (counts 0 ... 257 = cap, not a power of two)"""
    case, out = D.load_fixture("dbow2_ref_trees_a.npz")[0]
    frames = [s for s, (_, lu) in enumerate(case["sets"]) if lu == 2] + [0]
    assert len(frames) >= 3
    for b, got in enumerate(_device_batch(pkg, case, out, frames, 257, 2)):
        D.check_transform(got, out, frames[b], case["voc"]["L"], 2, case["name"])


def test_transform_device_variants_match_recorded_reference(pkg, gpu):
    """all 6 scorings x 4 weightings: the two recorded sets (120 and 17 features) as one batch plus an empty frame"""
    for case, out in D.load_fixture("dbow2_ref_variants.npz"):
        if not case["name"].startswith("h_"):
            continue
        empty = dict(case, sets=case["sets"] + [(np.zeros((0, 32), np.uint8), 2)])
        ref = dict(out)
        for key in ("bow_word", "fv_node", "fv_idx", "word_of", "node_of"):
            ref["s2." + key] = np.zeros(0, np.int32)
        ref.update({"s2.bow_value": np.zeros(0), "s2.weight_of": np.zeros(0), "s2.fv_off": np.zeros(1, np.int32)})
        sc, wt = int(out["scoring"][0]), int(out["weighting"][0])
        for b, got in enumerate(_device_batch(pkg, empty, ref, [0, 2, 1], 120, 2, sc, wt)):
            D.check_transform(got, ref, [0, 2, 1][b], case["voc"]["L"], 2, case["name"])
