"""The oracle's vocabulary path (oracle/dbow_oracle.c) against the reference's own DBoW2: the recorded fixtures
tests/golden/dbow2_ref_*.npz always, and the live driver oracle/_ref/dbow2_ref on the full case list where it is built.
Cases, fixture layout and comparisons: tests/dbow2_cases.py.  Everything is bit for bit."""
import numpy as np
import pytest

import dbow2_cases as D


@pytest.fixture(scope="module")
def impl(oracle):
    return D.Impl(oracle, True)


def _live_or_skip():
    if D.live_binary() is None:
        pytest.skip(D.SKIP_REASON)


@pytest.mark.parametrize("fixture", D.FIXTURES)
def test_oracle_matches_recorded_reference(impl, tmp_path, fixture):
    for case, out in D.load_fixture(fixture):
        D.check_case(impl, case, out, tmp_path)


@pytest.mark.parametrize("group", ["transform", "variants", "loader", "header", "score"])
def test_oracle_matches_live_reference(impl, tmp_path, group):
    _live_or_skip()
    cases = dict(transform=lambda: D.transform_cases(False), variants=lambda: D.variant_cases(False), loader=D.loader_cases,
                 header=D.header_cases, score=lambda: [D.score_case(False)])[group]()
    for case in cases:
        D.check_case(impl, case, D.run_ref(case, tmp_path), tmp_path)


@pytest.mark.parametrize("fixture", ["dbow2_ref_loader.npz", "dbow2_ref_trees_c.npz"])
def test_library_host_code_matches_recorded_reference(pkg, tmp_path, fixture):
    """The HIP library's loaders, writer, node table and score() are host code: checked here without a device."""
    for case, out in D.load_fixture(fixture):
        D.check_case(D.Impl(pkg, False), case, out, tmp_path, host_only=True)


def test_library_score_refuses_all_but_l1(pkg):
    """score() is implemented for L1_NORM, the ORB vocabulary's scoring; the other five are an error, never a number."""
    case, out = D.load_fixture("dbow2_ref_trees_c.npz")[1]
    voc, a = case["voc"], D.ref_bow(out, 0)
    for scoring in range(6):
        V = pkg.Vocabulary()
        V.set_nodes(voc["k"], voc["L"], scoring, 0, voc["parent"], voc["desc"], voc["weight"], voc["is_leaf"])
        if scoring == 0:
            D.same(np.float64(V.score(a, a)), out["score"][0], "L1 self score")
        else:
            with pytest.raises(pkg.AosError):
                V.score(a, a)


def test_fixtures_are_what_the_reference_produces_now(tmp_path):
    _live_or_skip()
    built = D.fixture_cases()
    for fixture in D.FIXTURES:
        recorded = D.load_fixture(fixture)
        assert [c["name"] for c, _ in recorded] == [c["name"] for c in built[fixture]]
        for (case, out), fresh in zip(recorded, built[fixture]):
            D.same(case["file"], fresh["file"], f"{fixture} {case['name']}: vocabulary file bytes")
            now = D.run_ref(case, tmp_path)
            assert sorted(now) == sorted(out), f"{fixture} {case['name']}: recorded arrays"
            for k in now:
                D.same(now[k], out[k], f"{fixture} {case['name']}: {k}")


def test_cases_cover_what_they_claim(tmp_path):
    """Preconditions of the cases, read off the recorded reference outputs: the score pairs are identical / overlapping /
    disjoint / empty, one set lands only on stopped words, one word is hit forty times, ragged trees leave nodes undefined."""
    by = {c["name"]: (c, o) for f in D.FIXTURES for c, o in D.load_fixture(f)}
    c, o = by["score_l1"]
    w = [set(o[f"s{s}.bow_word"].tolist()) for s in range(5)]
    assert w[0] & w[1] and w[0] != w[1] and w[2] and w[3] and not (w[2] & w[3]) and not w[4]
    assert len({len(d) for d, _ in c["sets"]}) == 5                      # distinct n
    sc = o["score"]
    assert abs(sc[0] - 1) < 1e-12 and 0 < sc[1] < 1 and sc[1] == sc[2] and sc[3] == 0 and sc[4] == 0 and sc[5] == 0
    c, o = by["ragged_k6_L3"]
    n_sets = len(c["sets"])
    assert len(o[f"s{n_sets - 1}.bow_word"]) == 0 and len(c["sets"][-1][0]) > 0          # only stopped words
    hit = np.bincount(o[f"s{n_sets - 2}.word_of"])
    assert hit.max() >= 40
    undefined = sum(int((o[f"s{s}.node_of"] == -1).sum()) for s in range(n_sets))
    assert undefined > 0                                                   # leaves above level L - levelsup exist
    # the phantom record after a final newline: what the pinned build does with the two values it reads unassigned
    for tag, parent in (("leaflast", 4), ("innerlast", 0)):
        plain, nl = by[tag + "_text"][1], by[tag + "_text_nl"][1]
        assert int(nl["n_nodes"][0]) == int(plain["n_nodes"][0]) + 1
        assert int(nl["size"][0]) == int(plain["size"][0]) + 1               # a word on both trees: our word count follows it
        assert int(nl["node_parent"][-1]) == parent                          # the previous record's pid
    z = by["innerlast_text_nl"][1]
    s = len(by["innerlast_text_nl"][0]["sets"]) - 1                            # zero descriptors: drawn at root level, stopped
    assert (z[f"s{s}.word_of"] == int(z["size"][0]) - 1).all() and (z[f"s{s}.weight_of"] == 0).all() and len(z[f"s{s}.bow_word"]) == 0
