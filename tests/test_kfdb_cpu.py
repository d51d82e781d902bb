"""KeyFrameDatabase (src/KeyFrameDatabase.cc) without a GPU: the Python restatement the GPU tests compare against
(tests/kfdb_ref.py) checked against independent knowledge (numpy set intersections, a brute-force sort by the order key, the closed
form of the L1 score of normalised vectors, a plain loop for the scores), the conditions the shared generator has to meet, the
library's host tap (aos2_debug_kfdb_host: the routines of csrc/kfdb.h over a literal inverted file) against the restatement byte for
byte, the argument checks, and the host class's compile + link."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref as R  # noqa: E402

SEEDS = (1, 2, 3)
DBL_EPSILON = 2.220446049250313e-16
SENTINEL = 0x5A


@pytest.fixture(scope="module")
def cases(oracle):
    return {seed: R.make_case(seed, oracle) for seed in SEEDS}


def fresh_db(pkg, n_words=R.N_WORDS):
    return pkg.KeyFrameDatabase(R.flat_vocabulary(pkg, n_words))


def walk(ops):
    """the state a script is in at each detect step, from the steps alone: slot -> (words, values), slot -> add sequence"""
    rows, seq, counter = {}, {}, 0
    for op in ops:
        if op[0] == "put":
            rows[op[3]] = (op[1], op[2])
        elif op[0] == "add":
            seq[op[1]] = counter
            counter += 1
        elif op[0] in ("erase", "drop"):
            seq.pop(op[1], None)
            if op[0] == "drop":
                rows.pop(op[1])
        elif op[0] == "clear":
            seq.clear()
        elif op[0] in ("detect", "scores"):
            yield op, dict(rows), dict(seq)


# ---------------------------------------------------------------------------------------- the restatement against independent knowledge
def test_sharing_set_words_and_order(cases):
    """`words` = the size of the numpy set intersection; the sharing set = the added, non-excluded slots with a non-empty one; its
    order = a brute-force sort by (first common word, add sequence); the scored list = those above the cut, in the same order"""
    n = 0
    for S in cases.values():
        for op, rows, seq in walk(S.ops):
            if op[0] != "detect":
                continue
            for q, want in zip(op[1], op[2]):
                qw = rows[q["slot"]][0] if q.get("slot", -1) >= 0 else np.asarray(q["words"])
                excluded = set(int(s) for s in q.get("excluded", ())) if q["mode"] == R.LOOP else set()
                common = {s: np.intersect1d(qw, rows[s][0]) for s in seq if s not in excluded}
                keys = sorted((int(c[0]), seq[s], s) for s, c in common.items() if len(c))
                assert [k[2] for k in keys] == list(want["sharing_slot"])
                assert [len(common[k[2]]) for k in keys] == list(want["sharing_words"])
                mx = max([len(c) for c in common.values()], default=0)
                assert want["max_common_words"] == mx and want["min_common_words"] == int(np.float32(mx) * np.float32(0.8))
                assert [k[2] for k in keys if len(common[k[2]]) > want["min_common_words"]] == list(want["scored_slot"])
                n += 1
    assert n >= 60


def test_score_is_the_l1_closed_form(cases, oracle):
    """For L1-normalised vectors score(a, b) = 1 - 0.5 |a - b|_1 (the reference's own comment, ScoringObject.cpp:65-67); the oracle's
    double is within 4 DBL_EPSILON of that value formed in long double"""
    worst = 0.0
    for S in cases.values():
        rows = [k for k in S.ref.rows if k is not None]
        for a in rows[:12]:
            for b in rows:
                got = oracle.vocab_score_l1(dict(bow_word=a.words, bow_value=a.values), dict(bow_word=b.words, bow_value=b.values))
                u = np.union1d(a.words, b.words)
                va, vb = np.zeros(len(u), np.longdouble), np.zeros(len(u), np.longdouble)
                va[np.searchsorted(u, a.words)] = a.values
                vb[np.searchsorted(u, b.words)] = b.values
                want = np.longdouble(1) - np.longdouble(0.5) * np.abs(va - vb).sum()
                worst = max(worst, abs(float(np.longdouble(got) - want)) / DBL_EPSILON)
    print("worst |score - (1 - 0.5 |a - b|_1)| / DBL_EPSILON:", worst)
    assert worst <= 4


def test_scores_and_min_against_a_plain_loop(cases, oracle):
    n = 0
    for S in cases.values():
        for op, rows, _ in walk(S.ops):
            if op[0] != "scores":
                continue
            q, slots, (scores, mn) = op[1:]
            qw, qv = (q["words"], q["values"]) if q.get("slot", -1) < 0 else rows[q["slot"]]
            m = np.float32(1)
            for s, got in zip(slots, scores):
                sc = np.float32(oracle.vocab_score_l1(dict(bow_word=qw, bow_value=qv), dict(bow_word=rows[s][0], bow_value=rows[s][1])))
                assert sc.tobytes() == got.tobytes()
                m = min(m, sc)
            assert m == mn and mn < 1
            n += 1
    assert n == len(SEEDS)


# ---------------------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("seed", SEEDS)
def test_generator_conditions(cases, seed):
    """what a case has to contain, so that no comparison below is vacuous"""
    S = cases[seed]
    results = [w for op in S.ops if op[0] == "detect" for w in op[2]]
    queries = [q for op in S.ops if op[0] == "detect" for q in op[1]]
    n_two = sum(1 for w in results if w["n_candidates"] >= 2)
    ev, mc = S.ref.events, S.ref.max_common
    print("seed", seed, "queries", len(results), "with >= 2 candidates", n_two, dict(ev), "maxCommonWords", sorted(mc))
    assert 2 * n_two >= len(results)
    assert ev["dedupe"] >= 1 and ev["below_min_feeds_a_sum"] >= 1 and ev["score_equals_min"] >= 1 and ev["tie_at_max"] >= 1
    assert all(mc[n] >= 1 for n in (1, 4, 5, 6))
    assert ev["stale_read"] >= 1 and ev["initial_zero_read"] >= 1
    assert any(w["n_sharing"] == 0 and q["mode"] == R.RELOC for q, w in zip(queries, results))
    assert any(w["n_sharing"] == 0 and q["mode"] == R.LOOP and len(q["excluded"]) > 0 for q, w in zip(queries, results))
    assert sum(1 for op in S.ops if op[0] == "erase") >= 5 and any(op[0] == "drop" for op in S.ops)


# ---------------------------------------------------------------------------------------- the host tap against the restatement
@pytest.mark.parametrize("seed", SEEDS)
def test_host_tap_equals_the_restatement(pkg, cases, seed):
    """every detect and scores step of the script (three detect calls around erase / re-add / drop + put), byte for byte"""
    R.replay(cases[seed].ops, fresh_db(pkg), host=True)


@pytest.mark.parametrize("n_added", (0, 1, 63, 65, 300))
def test_host_tap_on_the_kernel_shapes(pkg, oracle, n_added):
    R.replay(R.make_shapes(7, oracle, n_added).ops, fresh_db(pkg), host=True)


def test_host_tap_one_call_equals_single_calls(pkg, cases):
    """the RELOC queries of one call take effect in index order: a call per query gives the same bytes"""
    R.replay(cases[1].ops, fresh_db(pkg), host=True, single=True)


def test_host_tap_across_an_arena_growth(pkg, cases, oracle):
    """the same queries before and after the arena has grown many times over give the same bytes"""
    S = cases[2]
    db = fresh_db(pkg)
    R.replay(S.ops, db, host=True)
    queries = [q for q in S.ops[-1][1]]
    before = db.detect(queries, host=True)
    rng = np.random.default_rng(5)
    for _ in range(400):
        db.put(*R.bow(rng, rng.choice(R.N_WORDS - R.RESERVED, 300, replace=False)))
    after = db.detect(queries, host=True)
    assert all(R.same(a, b) for a, b in zip(after, before))
    assert any(b["n_candidates"] >= 2 for b in before)


def test_clear_and_size(pkg, cases):
    S = cases[3]
    db = fresh_db(pkg)
    R.replay(S.ops, db, host=True)
    assert db.size() == S.ref.size() > 0
    db.clear()
    assert db.size() == 0
    (r,) = db.detect([S.ops[-1][1][0]], host=True)
    assert r["n_sharing"] == 0 and r["n_candidates"] == 0
    db.add(0)       # the slots stay put
    assert db.size() == 1


# ---------------------------------------------------------------------------------------- argument checks
def test_refusals_leave_the_results_untouched(pkg, cases):
    S = cases[1]
    db = fresh_db(pkg)
    R.replay(S.ops, db, host=True)
    good = dict(mode=R.RELOC, words=np.array([3, 9, 40], np.uint32), values=np.array([0.2, 0.3, 0.5]))
    bad = [dict(good, mode=2),                                                      # no such mode
           dict(good, words=np.array([3, 40, 9], np.uint32)),                       # words do not ascend
           dict(good, words=np.array([3, 9, R.N_WORDS], np.uint32)),                # a word the vocabulary does not have
           dict(mode=R.RELOC, slot=10 ** 6),                                        # a slot that is not put
           dict(good, n_words=-1),
           dict(good, mode=R.LOOP, excluded=np.zeros(1, np.int32), n_excluded=-1)]
    for q in bad:
        for host in (True, False):      # the checks run before a device is looked for
            with pytest.raises(pkg.AosError) as e:
                db.detect([good, q], host=host, sentinel=SENTINEL)
            assert e.value.code == pkg.capi.AOS2_ERR_ARG
            structs, arrays, before = db.last
            assert bytes(structs) == before
            assert all((a.view(np.uint8) == SENTINEL).all() for o in arrays for a in o.values())
    with pytest.raises(pkg.AosError) as e:
        db.detect([good], host=True, caps=dict(candidates=-1))
    assert e.value.code == pkg.capi.AOS2_ERR_ARG
    # a list that does not fit: AOS2_ERR_CAPACITY, and the count says what is needed
    q = S.ops[-1][1][0]
    db.detect([q], host=True)
    (want,) = db.detect([q], host=True)       # (a RELOC query leaves the scores it wrote: the second answer repeats)
    assert want["n_candidates"] >= 2
    with pytest.raises(pkg.AosError) as e:
        db.detect([q], host=True, caps=dict(candidates=1))
    assert e.value.code == pkg.capi.AOS2_ERR_CAPACITY
    assert db.last[0][0].n_candidates == want["n_candidates"] and db.last[1][0]["candidates"][0] == want["candidates"][0]


def test_life_cycle_refusals(pkg):
    E = pkg.capi.AOS2_ERR_ARG
    db = fresh_db(pkg)

    def refused(f, *a):
        with pytest.raises(pkg.AosError) as e:
            f(*a)
        assert e.value.code == E

    s = db.put([1, 5], [0.5, 0.5])
    assert s == 0 and db.put([], []) == 1
    refused(db.put, [5, 1], [0.5, 0.5])
    refused(db.put, [1, 1], [0.5, 0.5])
    refused(db.put, [R.N_WORDS], [1.0])
    db.add(s)
    refused(db.add, s)          # the reference would count the keyframe twice
    refused(db.add, 7)
    refused(db.erase, 7)
    refused(db.drop, -1)
    refused(db.set_neighbours, [7], [[-1] * 10])
    db.erase(s)
    db.erase(s)                 # erasing what is not added does nothing, as in the reference
    db.add(s)
    db.drop(s)
    assert db.size() == 0
    refused(db.add, s)
    assert db.put([2], [1.0]) == s      # the slot is handed out again
    refused(db.scores, dict(slot=5), [0])
    refused(db.scores, dict(slot=0), [5])
    sc, mn = db.scores(dict(slot=0), [], host=True)
    assert len(sc) == 0 and mn == 1
    assert db.detect([], host=True) == [] and db.detect([]) == []
    (r,) = db.detect([dict(mode=R.LOOP, slot=0, min_score=0.25)])      # an empty database needs no device
    assert r["n_sharing"] == 0 and r["best_acc_score"] == np.float32(0.25)


def test_other_scorings_are_refused(pkg):
    for scoring in (1, 2, 3, 4, 5):
        with pytest.raises(pkg.AosError) as e:
            pkg.KeyFrameDatabase(R.flat_vocabulary(pkg, 50, scoring=scoring))
        assert e.value.code == pkg.capi.AOS2_ERR_ARG


# ---------------------------------------------------------------------------------------- the host class
@pytest.mark.parametrize("flags", ([], ["-DAOS2_HOST_EXCEPTIONS"]))
def test_host_class_compiles_and_links(pkg, tmp_path, flags):
    libdir = os.path.dirname(pkg.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                          [os.path.join(ROOT, "tests", "cpp", "keyframe_database_test.cpp"), "-o", str(tmp_path / "kfdb_test"),
                           "-L" + libdir, "-laos2", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
