"""aos2_kfdb_detect / aos2_kfdb_scores on the device against the Python restatement of src/KeyFrameDatabase.cc (tests/kfdb_ref.py),
byte for byte: the candidates in order, every integer, the float bits of best_acc_score and of the scored list, the sharing list.
The generator's seeds (tests/test_kfdb_cpu.py asserts what they contain) and the smallest shapes at which the kernels can go wrong:
queries of 1, 63, 64, 65 and 130 words (a lane round is 64 words), slot rows of 1 and 257 words, 0, 1, 63, 65 and 300 added slots
(a workgroup of the walk takes 8 slots, one of the rank 256), a slot whose only common word is the query's last."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def cases(oracle):
    return {seed: R.make_case(seed, oracle) for seed in SEEDS}


def fresh_db(pkg, n_words=R.N_WORDS):
    return pkg.KeyFrameDatabase(R.flat_vocabulary(pkg, n_words), device=0)


@pytest.mark.parametrize("seed", SEEDS)
def test_detect_and_scores_equal_the_restatement(pkg, gpu, cases, seed):
    """three detect calls around erase / re-add / drop + put (the third one reads the scores the first one left) and a scores call"""
    db = fresh_db(pkg)
    R.replay(cases[seed].ops, db, host=False)
    assert db.last_device_ms() > 0


@pytest.mark.parametrize("n_added", (0, 1, 63, 65, 300))
def test_kernel_shapes(pkg, gpu, oracle, n_added):
    S = R.make_shapes(7, oracle, n_added)
    db = fresh_db(pkg)
    R.replay(S.ops, db, host=False)
    queries, want = S.ops[-1][1], S.ops[-1][2]
    if n_added > 1:      # the slot that shares only the last word of the 130-word query is in its sharing list with one word
        i = list(want[4]["sharing_slot"]).index(1)
        assert want[4]["sharing_words"][i] == 1 and len(queries[4]["words"]) == 130
    if n_added:
        slots = list(range(n_added))
        for q in queries[:5]:
            assert R.same_scores(db.scores(q, slots), S.ref.scores(q, slots))


def test_eight_queries_in_one_call_equal_eight_calls(pkg, gpu, cases):
    """RELOC order included: the second call of the script holds the mixed queries, the third the RELOC queries that read what the
    first left; replayed with a call per query on one database and with a call per step on another"""
    one, many = [], []
    R.replay(cases[2].ops, fresh_db(pkg), host=False, collect=one)
    R.replay(cases[2].ops, fresh_db(pkg), host=False, single=True, collect=many)
    assert len(one) == 3 and len(one[1]) >= 8
    for a, b in zip(one, many):
        assert all(R.same(x, y) for x, y in zip(a, b))


def test_lists_are_optional(pkg, gpu, cases):
    """without the optional lists the counts and the candidates are the same, and RELOC queries still leave their scores"""
    full, bare = fresh_db(pkg), fresh_db(pkg)
    ops = cases[3].ops
    R.replay(ops, full, host=False)
    for op in ops:
        if op[0] == "detect":
            for g, w in zip(bare.detect(op[1], lists=()), op[2]):
                assert R.same(g, w, lists=("candidates",)) and "scored_slot" not in g
        elif op[0] == "put":
            bare.put(op[1], op[2])
        elif op[0] != "scores":
            getattr(bare, op[0])(*op[1:])


def test_results_before_and_after_an_arena_growth_are_equal(pkg, gpu, cases):
    S = cases[1]
    db = fresh_db(pkg)
    R.replay(S.ops, db, host=False)
    queries = S.ops[-1][1]
    before = db.detect(queries)
    cap = db.arena_capacity()
    rng = np.random.default_rng(5)
    while db.arena_capacity() == cap:
        for _ in range(100):
            db.put(*R.bow(rng, rng.choice(R.N_WORDS - R.RESERVED, 300, replace=False)))
        after = db.detect(queries)
        assert all(R.same(a, b) for a, b in zip(after, before))
    assert db.arena_capacity() >= 2 * cap and any(b["n_candidates"] >= 2 for b in before)
    assert all(R.same(a, b) for a, b in zip(db.detect(queries, host=True), before))


def test_rows_put_from_the_device_equal_rows_put_from_the_host(pkg, gpu):
    """BowVectors as aos2_vocabulary_transform_device wrote them, put straight from HBM, against the same rows put from host arrays:
    the same slots, the same answers; and a query by device arrays equals the query by host arrays"""
    import torch
    S = pkg.synth
    voc = S.synth_vocabulary(31, 10, 3)
    V = pkg.Vocabulary(device=0)
    V.set_nodes(voc["k"], voc["L"], 0, 0, voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
    rng = np.random.default_rng(31)
    B, cap = 12, 300
    ns = np.array([300, 257, 1, 64, 65, 0, 130, 200, 250, 299, 63, 180], np.int32)
    desc = np.zeros((B, cap, 32), np.uint8)
    for b in range(B):
        desc[b, : ns[b]] = S.vocab_descriptors(rng, voc, int(ns[b]))
    dev = torch.device("cuda:0")
    d_desc, d_n = torch.from_numpy(desc).to(dev), torch.from_numpy(ns).to(dev)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    bw, bv, nb = z((B, cap), torch.int32), z((B, cap), torch.float64), z(B, torch.int32)
    fn, fo, fi, nf = z((B, cap), torch.int32), z((B, cap + 1), torch.int32), z((B, cap), torch.int32), z(B, torch.int32)
    V.transform_device(B, d_desc.data_ptr(), d_n.data_ptr(), cap, 2, bw.data_ptr(), bv.data_ptr(), nb.data_ptr(), fn.data_ptr(),
                       fo.data_ptr(), fi.data_ptr(), nf.data_ptr())
    a, b = pkg.KeyFrameDatabase(V, device=0), pkg.KeyFrameDatabase(V, device=0)
    slots = a.put_device(V, B, bw.data_ptr(), bv.data_ptr(), nb.data_ptr(), cap)
    hw, hv, hn = bw.cpu().numpy().view(np.uint32), bv.cpu().numpy(), nb.cpu().numpy()
    assert list(slots) == [b.put(hw[i, : hn[i]], hv[i, : hn[i]]) for i in range(B)] and hn.max() > 64
    neigh = [[int(t) for t in rng.choice(B, 10, replace=False)] for _ in range(B)]
    for db in (a, b):
        db.set_neighbours(slots, neigh)
        for s in slots[:-2]:
            db.add(int(s))
    queries = [dict(mode=R.RELOC, slot=int(slots[-1])), dict(mode=R.LOOP, slot=int(slots[-2]), min_score=0.01, excluded=slots[:2])]
    on_device = [dict(q, slot=-1, d_words=bw[int(q["slot"])].data_ptr(), d_values=bv[int(q["slot"])].data_ptr(),
                      n_words=int(hn[int(q["slot"])])) for q in queries]
    got_a, got_b, got_d, got_h = a.detect(queries), b.detect(queries), a.detect(on_device), b.detect(on_device, host=True)
    assert got_a[0]["n_scored"] >= 1 and got_a[0]["n_candidates"] >= 1
    for other in (got_b, got_d, got_h):
        assert all(R.same(x, y) for x, y in zip(other, got_a))
    assert R.same_scores(a.scores(on_device[0], slots), b.scores(queries[0], slots, host=True))
