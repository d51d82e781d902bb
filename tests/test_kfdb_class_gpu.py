"""host/KeyFrameDatabase.h, the class at the reference's signatures, driven by tests/cpp/keyframe_database_test.cpp on the GPU over a
pointer graph built from the generator's places (tests/kfdb_ref.py): the KeyFrame* vectors DetectLoopCandidates and
DetectRelocalizationCandidates return and the members they leave in the keyframes (mnLoopQuery / mnLoopWords / mLoopScore,
mnRelocQuery / mnRelocWords / mRelocScore) against the restatement, around add, erase, re-add and clear."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bundle_io  # noqa: E402
import kfdb_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
ADD, ERASE, LOOP_Q, RELOC_Q, CLEAR = range(5)


def class_case(oracle, seed=4, places=3, per_cluster=4):
    """-> (the bundle's arrays, per query op: (op index, the query's mnId, mode, the restatement's answer))"""
    rng = np.random.default_rng(seed)
    ref = R.RefDB(R.N_WORDS, oracle)
    base = [rng.choice(R.N_WORDS - R.RESERVED, 60, replace=False) for _ in range(places)]
    cluster = {(p, c): [ref.put(*R.place_vector(rng, base[p])) for _ in range(per_cluster)] for p in range(places) for c in range(2)}
    x = cluster[0, 0][0]
    dup = ref.put(ref.rows[x].words.copy(), ref.rows[x].values.copy())      # the same vector as keyframe x
    cluster[0, 1].append(dup)
    in_db = [s for v in cluster.values() for s in v]
    current = [ref.put(*R.place_vector(rng, base[p], keep=0.95)) for p in range(places)]   # the loop queries' keyframes, never added
    K = len(ref.rows)
    neigh = np.full((K, 10), -1, np.int32)
    for (p, c), members in cluster.items():
        for s in members:
            mates = [t for t in members if t != s]
            rng.shuffle(mates)
            other = cluster[(p + 1) % places, int(rng.integers(2))]
            row = mates + [int(other[int(rng.integers(len(other)))])]
            neigh[s, : len(row)] = row
    ref.set_neighbours(range(K), neigh)
    connected = {k: [] for k in range(K)}
    for p, k in enumerate(current):      # one keyframe of each cluster, and a keyframe the database never saw
        connected[k] = [int(cluster[p, 0][1]), int(cluster[p, 1][2]), int(current[(p + 1) % places])]
    connected[current[0]] = [x, int(current[1])]      # the duplicate of x scores exactly minScore
    frames = [R.place_vector(rng, base[p], keep=0.85) for p in range(places)]
    frames.append((np.arange(R.N_WORDS - 9, R.N_WORDS, dtype=np.uint32), np.full(9, 1.0 / 9)))      # shares nothing

    ops, min_score, expected = [], [], []

    def do(op, arg):
        ops.append((op, arg))
        ms = 0.0
        if op == ADD:
            ref.add(arg)
        elif op == ERASE:
            ref.erase(arg)
        elif op == CLEAR:
            ref.clear()
        elif op == LOOP_Q:
            q = dict(mode=R.LOOP, slot=arg, excluded=connected[arg])
            ms = float(ref.scores(q, [s for s in connected[arg] if s in in_db])[1])   # src/LoopClosing.cc:126-140
            expected.append((len(ops) - 1, arg + 1, R.LOOP, ref.detect(dict(q, min_score=ms))))
        else:
            expected.append((len(ops) - 1, 1000 + len(ops) - 1, R.RELOC, ref.detect(dict(mode=R.RELOC, words=frames[arg][0], values=frames[arg][1]))))
        min_score.append(ms)

    order = list(in_db)
    rng.shuffle(order)
    for s in order:
        do(ADD, s)
    for f in range(places):
        do(RELOC_Q, f)
    gone = [int(s) for s in rng.choice([s for s in in_db if s not in (x, dup)], 3, replace=False)]
    for s in gone:
        do(ERASE, s)
    for s in gone[:2]:
        do(ADD, s)
    for k in current:
        do(LOOP_Q, k)
    for f in (2, 1, 0, 3):
        do(RELOC_Q, f)
    do(CLEAR, -1)
    do(RELOC_Q, 0)

    arrays = dict(n_words=np.array([R.N_WORDS], np.int32), neigh=neigh, ops=np.array(ops, np.int32), min_score=np.array(min_score, np.float32))
    for name, rows in (("kf", [(k.words, k.values) for k in ref.rows]), ("fr", frames)):
        arrays[name + "_off"] = np.cumsum([0] + [len(w) for w, _ in rows]).astype(np.int32)
        arrays[name + "_word"] = np.concatenate([w for w, _ in rows]).astype(np.int32)
        arrays[name + "_value"] = np.concatenate([v for _, v in rows]).astype(np.float64)
    arrays["conn_off"] = np.cumsum([0] + [len(connected[k]) for k in range(K)]).astype(np.int32)
    arrays["conn"] = np.array([s for k in range(K) for s in connected[k]], np.int32)
    return arrays, expected, ref.events


def test_keyframe_database_class_returns_what_the_restatement_returns(pkg, gpu, oracle, tmp_path):
    libdir = os.path.dirname(pkg.lib_path())
    exe = str(tmp_path / "keyframe_database_test")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-DAOS2_HOST_EXCEPTIONS",
                           os.path.join(ROOT, "tests", "cpp", "keyframe_database_test.cpp"), "-o", exe, "-L" + libdir, "-laos2", "-lpthread",
                           "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    arrays, expected, events = class_case(oracle)
    bundle_io.save(tmp_path / "in.bundle", arrays)
    subprocess.check_call([exe, str(tmp_path / "in.bundle"), str(tmp_path / "out.bundle")])
    out = bundle_io.load(tmp_path / "out.bundle")
    K = len(arrays["kf_off"]) - 1
    ints, floats = np.zeros((K, 4), np.int32), np.zeros((K, 2), np.float32)      # the members as the keyframes start
    summary = []
    for i, mn_id, mode, want in expected:
        q = "q%d_" % i
        assert list(out[q + "cand"]) == list(want["candidates"]), i
        got_i, got_f = out[q + "int"], out[q + "float"]
        c = 0 if mode == R.LOOP else 2          # the columns of the mode's query id and word count; the score's column is mode
        touched = np.zeros(K, bool)
        for s, words in zip(want["sharing_slot"], want["sharing_words"]):
            assert got_i[s, c] == mn_id and got_i[s, c + 1] == words, (i, s)
            touched[s] = True
        for s, score in zip(want["scored_slot"], want["scored_score"]):
            assert got_f[s, mode].tobytes() == np.float32(score).tobytes(), (i, s)
        scored = np.zeros(K, bool)
        scored[want["scored_slot"]] = True
        # everything else is as the call before left it
        assert (got_i[~touched] == ints[~touched]).all() and (got_i[:, 2 - c: 4 - c] == ints[:, 2 - c: 4 - c]).all(), i
        assert got_f[~scored].tobytes() == floats[~scored].tobytes() and got_f[:, 1 - mode].tobytes() == floats[:, 1 - mode].tobytes(), i
        ints, floats = got_i, got_f
        summary.append((mode, want["n_sharing"], want["n_scored"], want["n_candidates"]))
    print("(mode, sharing, scored, candidates) per query:", summary, dict(events))
    assert sum(1 for s in summary if s[3] >= 2) >= 6 and summary[-1][1] == 0 and any(s[1] == 0 for s in summary[:-1])
    assert events["stale_read"] >= 1 and events["score_equals_min"] >= 1 and events["dedupe"] >= 1
