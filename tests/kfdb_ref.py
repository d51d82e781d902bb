"""KeyFrameDatabase (src/KeyFrameDatabase.cc) restated literally in Python: a list of keyframes per word, the members of every
keyframe (mnLoopQuery, mnLoopWords, mLoopScore, mnRelocQuery, mnRelocWords, mRelocScore: never reset, as there), the statements of
DetectLoopCandidates (:76-197) and DetectRelocalizationCandidates (:199-309) in their order.  The score is the pinned
oracle.vocab_score_l1 (query first) cast to float32; every float32 sum is a numpy float32 sum in the reference's order.  What the
reference leaves open is fixed as DESIGN.md section 2 item 13 says: mRelocScore is 0.0f at put, and query ids do not repeat.

Keyframes are SLOTS, numbered as the library numbers them (the next index, or the last dropped one), so the results compare as they
are.  The module also holds the seeded generator of the tests: a script of put / add / erase / drop / neighbour / detect / scores
steps with the results the restatement gives, and the driver that replays a script on the library."""
from collections import Counter

import numpy as np

LOOP, RELOC = 0, 1
F32 = np.float32
LISTS = ("candidates", "scored_slot", "scored_words", "scored_score", "sharing_slot", "sharing_words")
SCALARS = ("n_candidates", "n_sharing", "max_common_words", "min_common_words", "n_scored", "n_matched")


class KF:
    def __init__(self, words, values):
        self.words, self.values = np.asarray(words, np.uint32), np.asarray(values, np.float64)
        self.neigh = []                 # GetBestCovisibilityKeyFrames(10), slots
        self.added = False
        self.loop_query = self.reloc_query = -1
        self.loop_words = self.reloc_words = 0
        self.loop_score = F32(0)
        self.reloc_score = F32(0)       # the convention; the reference leaves it uninitialised (src/KeyFrame.cc:35)
        self.reloc_written = False      # (bookkeeping of the tests' conditions only)


class RefDB:
    def __init__(self, n_words, oracle):
        self.oracle = oracle
        self.n_words = n_words
        self.inv = [[] for _ in range(n_words)]   # mvInvertedFile
        self.rows, self.free = [], []
        self.next_id = 0
        self.events = Counter()
        self.max_common = Counter()

    def score(self, qw, qv, k):
        return F32(self.oracle.vocab_score_l1(dict(bow_word=qw, bow_value=qv), dict(bow_word=k.words, bow_value=k.values)))

    # ---- the life cycle of a slot
    def put(self, words, values):
        k = KF(words, values)
        if self.free:
            s = self.free.pop()
            self.rows[s] = k
        else:
            s = len(self.rows)
            self.rows.append(k)
        return s

    def add(self, s):                    # :40-46
        k = self.rows[s]
        assert not k.added
        for w in k.words:
            self.inv[w].append(s)
        k.added = True

    def erase(self, s):                  # :48-67
        k = self.rows[s]
        if not k.added:
            return
        for w in k.words:
            self.inv[w].remove(s)
        k.added = False

    def drop(self, s):
        self.erase(s)
        self.rows[s] = None
        self.free.append(s)

    def clear(self):                     # :69-73
        self.inv = [[] for _ in range(self.n_words)]
        for k in self.rows:
            if k is not None:
                k.added = False

    def size(self):
        return sum(1 for k in self.rows if k is not None and k.added)

    def set_neighbours(self, slots, neigh):
        for s, row in zip(slots, neigh):
            self.rows[s].neigh = [int(x) for x in row]

    def _query_rows(self, q):
        if q.get("slot", -1) >= 0:
            k = self.rows[q["slot"]]
            return k.words, k.values
        return np.asarray(q["words"], np.uint32), np.asarray(q["values"], np.float64)

    def _neighbours(self, k):
        return [s for s in k.neigh if 0 <= s < len(self.rows) and self.rows[s] is not None]

    # ---- the two queries
    def detect(self, q):
        qw, qv = self._query_rows(q)
        qid = self.next_id
        self.next_id += 1
        out = dict(n_sharing=0, max_common_words=0, min_common_words=0, n_scored=0, n_matched=0, n_candidates=0,
                   candidates=[], scored_slot=[], scored_words=[], scored_score=[], sharing_slot=[], sharing_words=[])
        res = self._loop(q, qw, qv, qid, out) if q["mode"] == LOOP else self._reloc(qw, qv, qid, out)
        for k, dt in (("candidates", np.int32), ("scored_slot", np.int32), ("scored_words", np.int32), ("scored_score", F32),
                      ("sharing_slot", np.int32), ("sharing_words", np.int32)):
            res[k] = np.array(res[k], dt)
        res["n_candidates"] = len(res["candidates"])
        return res

    def _loop(self, q, qw, qv, qid, out):
        min_score = F32(q["min_score"])
        out["best_acc_score"] = min_score
        connected = set(int(s) for s in q.get("excluded", ()))       # spConnectedKeyFrames :78
        sharing = []
        for w in qw:                                                # :86-104
            for s in self.inv[w]:
                k = self.rows[s]
                if k.loop_query != qid:
                    k.loop_words = 0
                    if s not in connected:
                        k.loop_query = qid
                        sharing.append(s)
                k.loop_words += 1
        if not sharing:                                             # :107
            return out
        out["n_sharing"], out["sharing_slot"] = len(sharing), sharing
        out["sharing_words"] = [self.rows[s].loop_words for s in sharing]
        max_common = max(out["sharing_words"])                      # :113-118
        min_common = int(F32(max_common) * F32(0.8))                # :120
        out["max_common_words"], out["min_common_words"] = max_common, min_common
        self.max_common[max_common] += 1
        if out["sharing_words"].count(max_common) > 1:
            self.events["tie_at_max"] += 1
        match = []
        for s in sharing:                                           # :125-139
            k = self.rows[s]
            if k.loop_words > min_common:
                si = self.score(qw, qv, k)
                k.loop_score = si
                out["scored_slot"].append(s)
                out["scored_words"].append(k.loop_words)
                out["scored_score"].append(si)
                if si == min_score:
                    self.events["score_equals_min"] += 1
                if si >= min_score:
                    match.append((si, s))
        out["n_scored"], out["n_matched"] = len(out["scored_slot"]), len(match)
        if not match:                                               # :141
            return out
        acc_list, best_acc = [], min_score                          # :144-173
        for si, s in match:
            best_score, acc, best = si, si, s
            for s2 in self._neighbours(self.rows[s]):
                k2 = self.rows[s2]
                if k2.loop_query == qid and k2.loop_words > min_common:
                    if k2.loop_score < min_score:
                        self.events["below_min_feeds_a_sum"] += 1
                    acc = F32(acc + k2.loop_score)
                    if k2.loop_score > best_score:
                        best, best_score = s2, k2.loop_score
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_list, best_acc, out)

    def _reloc(self, qw, qv, qid, out):
        out["best_acc_score"] = F32(0)
        sharing = []
        for w in qw:                                                # :207-222
            for s in self.inv[w]:
                k = self.rows[s]
                if k.reloc_query != qid:
                    k.reloc_words = 0
                    k.reloc_query = qid
                    sharing.append(s)
                k.reloc_words += 1
        if not sharing:                                             # :224
            return out
        out["n_sharing"], out["sharing_slot"] = len(sharing), sharing
        out["sharing_words"] = [self.rows[s].reloc_words for s in sharing]
        max_common = max(out["sharing_words"])                      # :228-233
        min_common = int(F32(max_common) * F32(0.8))                # :235
        out["max_common_words"], out["min_common_words"] = max_common, min_common
        self.max_common[max_common] += 1
        if out["sharing_words"].count(max_common) > 1:
            self.events["tie_at_max"] += 1
        match = []
        for s in sharing:                                           # :242-253
            k = self.rows[s]
            if k.reloc_words > min_common:
                si = self.score(qw, qv, k)
                k.reloc_score, k.reloc_written = si, True
                out["scored_slot"].append(s)
                out["scored_words"].append(k.reloc_words)
                out["scored_score"].append(si)
                match.append((si, s))
        out["n_scored"], out["n_matched"] = len(out["scored_slot"]), len(match)
        if not match:                                               # :255
            return out
        acc_list, best_acc = [], F32(0)                             # :258-287
        for si, s in match:
            best_score, acc, best = si, si, s
            for s2 in self._neighbours(self.rows[s]):
                k2 = self.rows[s2]
                if k2.reloc_query != qid:
                    continue
                if k2.reloc_words <= min_common:
                    self.events["stale_read" if k2.reloc_written else "initial_zero_read"] += 1
                acc = F32(acc + k2.reloc_score)
                if k2.reloc_score > best_score:
                    best, best_score = s2, k2.reloc_score
            acc_list.append((acc, best))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_list, best_acc, out)

    def _retain(self, acc_list, best_acc, out):                     # :176-196 / :290-308
        out["best_acc_score"] = best_acc
        retain = F32(F32(0.75) * best_acc)
        already = set()
        for acc, best in acc_list:
            if acc > retain:
                if best not in already:
                    out["candidates"].append(best)
                    already.add(best)
                else:
                    self.events["dedupe"] += 1
        return out

    def scores(self, q, slots):                                     # src/LoopClosing.cc:126-140
        qw, qv = self._query_rows(q)
        min_score = F32(1)
        out = []
        for s in slots:
            sc = self.score(qw, qv, self.rows[s])
            out.append(sc)
            if sc < min_score:
                min_score = sc
        return np.array(out, F32), min_score


def same(got, want, lists=LISTS):
    """byte equality of one query's result: every integer, the float bits, every list in order"""
    for k in SCALARS:
        if int(got[k]) != int(want[k]):
            return False
    if F32(got["best_acc_score"]).tobytes() != F32(want["best_acc_score"]).tobytes():
        return False
    return all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() and np.asarray(got[k]).dtype == np.asarray(want[k]).dtype
               for k in lists if k in got)


def flat_vocabulary(pkg, n_words, scoring=0, device=0):
    """a vocabulary of n_words words right under the root (the database reads only its scoring type and its word count)"""
    V = pkg.Vocabulary(device=device)
    rng = np.random.default_rng(n_words)
    V.set_nodes(n_words, 1, scoring, 0, np.zeros(n_words, np.int32), rng.integers(0, 256, (n_words, 32), dtype=np.uint8),
                np.ones(n_words), np.ones(n_words, np.uint8))
    return V


# ---------------------------------------------------------------------------------------------------------- the generator
N_WORDS = 2000
RESERVED = 40          # the last word ids belong to no keyframe: a query made of them shares nothing


def bow(rng, words):
    """an ascending BowVector over `words` with L1-normalised values"""
    w = np.unique(np.asarray(words, np.uint32))
    v = rng.random(len(w)) + 0.05
    return w, v / v.sum()


def place_vector(rng, base, keep=0.9, extra=6):
    w = [x for x in base if rng.random() < keep] + list(rng.integers(0, N_WORDS - RESERVED, extra))
    return bow(rng, w)


class Script:
    """the steps of a case and what the restatement answers, formed while the steps are written"""

    def __init__(self, oracle, n_words=N_WORDS):
        self.ref = RefDB(n_words, oracle)
        self.n_words = n_words
        self.ops = []

    def put(self, w, v):
        s = self.ref.put(w, v)
        self.ops.append(("put", w, v, s))
        return s

    def step(self, name, *args):
        getattr(self.ref, name)(*args)
        self.ops.append((name,) + args)

    def detect(self, queries):
        want = [self.ref.detect(q) for q in queries]     # in index order: the RELOC queries take effect in it
        self.ops.append(("detect", queries, want))
        return want

    def scores(self, q, slots):
        want = self.ref.scores(q, slots)
        self.ops.append(("scores", q, list(slots), want))
        return want


def make_case(seed, oracle, places=4, per_cluster=5, base_words=60):
    """Places of two covisibility clusters each, whose keyframes share most words; a duplicate of one keyframe; neighbour rows inside
    a cluster plus one keyframe of another place; put / add (shuffled) / erase / re-add / drop + put; three detect calls (RELOC, a
    mix with the special queries, the first RELOC queries again) and a scores call."""
    rng = np.random.default_rng(seed)
    S = Script(oracle)
    base = [rng.choice(N_WORDS - RESERVED, base_words, replace=False) for _ in range(places)]
    cluster = {}           # (place, c) -> slots
    for p in range(places):
        for c in range(2):
            cluster[p, c] = [S.put(*place_vector(rng, base[p])) for _ in range(per_cluster)]
    all_kf = [s for v in cluster.values() for s in v]
    x = cluster[0, 0][0]
    dup = S.put(S.ref.rows[x].words.copy(), S.ref.rows[x].values.copy())      # the same vector as keyframe x
    cluster[0, 1].append(dup)
    all_kf.append(dup)

    def rows(slots):
        out = []
        for s in slots:
            (p, c), = [k for k, v in cluster.items() if s in v]
            mates = [t for t in cluster[p, c] if t != s]
            rng.shuffle(mates)
            other = cluster[(p + 1) % places, int(rng.integers(2))]
            row = mates[:8] + [int(other[int(rng.integers(len(other)))])]
            out.append(row + [-1] * (10 - len(row)))
        return out

    S.step("set_neighbours", all_kf, rows(all_kf))
    order = list(all_kf)
    rng.shuffle(order)
    for s in order:
        S.step("add", s)

    reloc = [dict(mode=RELOC, **dict(zip(("words", "values"), place_vector(rng, base[p], keep=0.85)))) for p in range(places)]
    S.detect(reloc)

    # erase five, add three of them again (they move to the end of every list), drop one and put another keyframe in its slot
    gone = [int(s) for s in rng.choice([s for s in all_kf if s not in (x, dup)], 5, replace=False)]
    for s in gone:
        S.step("erase", s)
    for s in gone[:3]:
        S.step("add", s)
    S.step("drop", gone[4])
    (pd, cd), = [k for k, v in cluster.items() if gone[4] in v]
    cluster[pd, cd].remove(gone[4])
    new = S.put(*place_vector(rng, base[pd]))
    assert new == gone[4]
    cluster[pd, cd].append(new)
    S.step("set_neighbours", [new], rows([new]))
    S.step("add", new)

    def loop_query(p, connected, **rows_or_slot):
        q = dict(mode=LOOP, excluded=np.array(connected, np.int32), **rows_or_slot)
        q["min_score"] = float(S.ref.scores(q, connected)[1]) if len(connected) else 0.0
        return q

    mixed = []
    for p in range(places):        # DetectLoop's query: connected = one keyframe of each cluster; minScore = their lowest score
        w, v = place_vector(rng, base[p], keep=0.95)
        connected = [int(cluster[p, c][1 + int(rng.integers(3))]) for c in range(2)]
        mixed.append(loop_query(p, connected, words=w, values=v))
    cur = S.put(*place_vector(rng, base[1], keep=0.95))      # a query by slot: the current keyframe, put and not added
    mixed.append(loop_query(1, [int(cluster[1, 0][0])], slot=cur))
    # connected = {x} alone, so minScore = score(query, x), and dup holds x's vector: si == minScore exactly
    w, v = place_vector(rng, base[0], keep=0.95)
    mixed.append(loop_query(0, [x], words=w, values=v))
    # x's own vector: x and dup both share every word, a tie at maxCommonWords
    mixed.append(dict(mode=RELOC, words=S.ref.rows[x].words.copy(), values=S.ref.rows[x].values.copy()))
    for n in (1, 4, 5, 6):         # maxCommonWords 1, 4, 5, 6: the truncation of maxCommonWords * 0.8f
        k = S.ref.rows[cluster[2, 0][0] if cluster[2, 0][0] != gone[3] else cluster[2, 0][1]]
        pick = np.sort(rng.choice(len(k.words), n, replace=False))
        mixed.append(dict(mode=RELOC, words=k.words[pick], values=np.full(n, 1.0 / n)))
    w = np.arange(N_WORDS - RESERVED, N_WORDS - RESERVED + 7, dtype=np.uint32)
    mixed.append(dict(mode=RELOC, words=w, values=np.full(7, 1.0 / 7)))          # shares nothing
    w, v = place_vector(rng, base[3])
    mixed.append(dict(mode=LOOP, words=w, values=v, min_score=0.01,
                      excluded=np.array([s for s in range(len(S.ref.rows))], np.int32)))   # everything excluded
    S.detect(mixed)
    S.scores(mixed[0], [int(s) for s in cluster[0, 0] + cluster[2, 1] + [cur]])
    S.detect(reloc[::-1] + reloc[:2])
    return S


def same_scores(got, want):
    return got[0].tobytes() == want[0].tobytes() and F32(got[1]).tobytes() == F32(want[1]).tobytes()


def replay(ops, db, host, single=False, collect=None):
    """the steps of a Script on a capi.KeyFrameDatabase (host: through the host taps); asserts every answer byte for byte.
    single: every query of a detect step in a call of its own."""
    for op in ops:
        name = op[0]
        if name == "put":
            assert db.put(op[1], op[2]) == op[3]
        elif name == "detect":
            queries, want = op[1], op[2]
            got = [db.detect([q], host=host)[0] for q in queries] if single else db.detect(queries, host=host)
            if collect is not None:
                collect.append(got)
            for i, (g, w) in enumerate(zip(got, want)):
                assert same(g, w), (i, {k: (g[k], w[k]) for k in g if np.asarray(g[k]).tobytes() != np.asarray(w[k]).tobytes()})
        elif name == "scores":
            assert same_scores(db.scores(op[1], op[2], host=host), op[3])
        else:
            getattr(db, name)(*op[1:])


QUERY_LENGTHS = (1, 63, 64, 65, 130)


def make_shapes(seed, oracle, n_added, pool=400):
    """The smallest shapes at which the kernels can go wrong: n_added slots over a pool of `pool` words (rows of 30..90 words, one of
    1 word and one of 257), queries of 1, 63, 64, 65 and 130 words in both modes (a lane round is 64 query words), and a slot whose
    only common word with the 130-word query is that query's last word.  Neighbour rows are random, so they cross every list."""
    rng = np.random.default_rng(seed)
    S = Script(oracle)
    queries = []
    for n in QUERY_LENGTHS:
        w, v = bow(rng, rng.choice(pool, n, replace=False))
        queries.append((w, v))
    last = int(queries[-1][0][-1])
    slots = []
    for i in range(n_added):
        if i == 1:
            w, v = bow(rng, [last] + list(rng.choice(np.arange(1000, 1900), 20, replace=False)))   # only the last word is common
        elif i == 2:
            w, v = bow(rng, [int(queries[1][0][5])])                                               # a row of 1 word
        elif i == 3:
            w, v = bow(rng, list(rng.choice(pool, 50, replace=False)) + list(rng.choice(np.arange(pool, 1000), 207, replace=False)))   # 257 words
        else:
            w, v = bow(rng, rng.choice(pool, int(rng.integers(30, 91)), replace=False))
        slots.append(S.put(w, v))
    if n_added:
        S.step("set_neighbours", slots, [[int(t) for t in rng.choice(slots, min(10, n_added), replace=False)] + [-1] * (10 - min(10, n_added))
                                          for _ in slots])
    for s in slots:
        S.step("add", s)
    batch = [dict(mode=RELOC, words=w, values=v) for w, v in queries]
    for w, v in queries:
        q = dict(mode=LOOP, words=w, values=v, excluded=np.array([int(t) for t in rng.choice(slots, min(3, n_added), replace=False)] if n_added
                                                                 else [], np.int32))
        q["min_score"] = float(S.ref.scores(q, list(q["excluded"]))[1]) if n_added else 0.3
        batch.append(q)
    S.detect(batch)
    return S
