"""KeyFrameDatabase (include/aos2.h: aos2_kfdb_*, aos2_debug_kfdb_host)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._abi import KFDB_MODES, _KfdbQuery, _KfdbResult
from ._build import _batch, _out
from ._core import _Handle, _check, _p


_KFDB_SCALARS = ("n_candidates", "n_sharing", "max_common_words", "min_common_words", "n_scored", "n_matched")
_KFDB_LISTS = (("candidates", "candidates", np.int32, "n_candidates"), ("scored_slot", "scored", np.int32, "n_scored"),
               ("scored_words", "scored", np.int32, "n_scored"), ("scored_score", "scored", np.float32, "n_scored"),
               ("sharing_slot", "sharing", np.int32, "n_sharing"), ("sharing_words", "sharing", np.int32, "n_sharing"))


class KeyFrameDatabase(_Handle):
    """KeyFrameDatabase (include/KeyFrameDatabase.h:42-70) over slots: the BowVectors resident on the device, the candidates of
    DetectLoopCandidates / DetectRelocalizationCandidates for a batch of queries in one call."""
    LOOP, RELOC = KFDB_MODES

    KIND = "kfdb"

    def __init__(self, voc, device=0):
        self._create(voc.h, device)

    def put(self, words, values):
        w, v = np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(values, np.float64)
        if len(w) != len(v):
            raise ValueError("words and values differ in length")
        s = C.c_int32(-1)
        _check(self.L.aos2_kfdb_put(self.h, _p(w), _p(v), len(w), C.byref(s)))
        return s.value

    def put_device(self, voc, batch, d_words, d_values, d_n_bow, cap):
        """rows as Vocabulary.transform_device wrote them (raw device pointers) -> the slots"""
        slots = np.full(max(batch, 1), -1, np.int32)
        V = C.c_void_p
        _check(self.L.aos2_kfdb_put_device(self.h, voc.h if voc is not None else None, batch, V(d_words), V(d_values), V(d_n_bow),
                                           cap, _p(slots)))
        return slots[:batch]

    def add(self, slot):
        _check(self.L.aos2_kfdb_add(self.h, slot))

    def erase(self, slot):
        _check(self.L.aos2_kfdb_erase(self.h, slot))

    def drop(self, slot):
        _check(self.L.aos2_kfdb_drop(self.h, slot))

    def clear(self):
        _check(self.L.aos2_kfdb_clear(self.h))

    def size(self):
        return self.L.aos2_kfdb_size(self.h)

    def arena_capacity(self):
        return int(self.L.aos2_kfdb_arena_capacity(self.h))

    def last_device_ms(self):
        return float(self.L.aos2_kfdb_last_device_ms(self.h))

    def set_neighbours(self, slots, neigh):
        s = np.ascontiguousarray(slots, np.int32)
        n = np.ascontiguousarray(neigh, np.int32).reshape(len(s), 10)
        _check(self.L.aos2_kfdb_set_neighbours(self.h, len(s), _p(s), _p(n)))

    @staticmethod
    def _query(Q, q, keep):
        """q: dict(mode, min_score, excluded) with slot=, or words= / values= (host), or d_words= / d_values= / n_words= (device)"""
        Q.mode, Q.min_score, Q.slot = int(q.get("mode", 0)), float(q.get("min_score", 0.0)), int(q.get("slot", -1))
        if "d_words" in q:
            Q.words, Q.values, Q.n_words, Q.on_device = q["d_words"], q["d_values"], int(q["n_words"]), 1
        elif "words" in q:
            w, v = np.ascontiguousarray(q["words"], np.uint32), np.ascontiguousarray(q["values"], np.float64)
            keep += [w, v]
            Q.words, Q.values, Q.n_words = w.ctypes.data, v.ctypes.data, int(q.get("n_words", len(w)))
        ex = q.get("excluded")
        if ex is not None:
            ex = np.ascontiguousarray(ex, np.int32)
            keep.append(ex)
            Q.excluded, Q.n_excluded = ex.ctypes.data, int(q.get("n_excluded", len(ex)))

    def detect_args(self, queries, lists=("scored", "sharing"), caps=None, sentinel=None):
        """the aos2_kfdb_query_t / aos2_kfdb_result_t arrays of a detect call -> (Q, R, what they point to, the result arrays per query).
        caps: dict(candidates=, scored=, sharing=), default the number of added slots; `sentinel` pre-fills structs and buffers."""
        nq = len(queries)
        Q, R, keep, outs = _batch(_KfdbQuery, _KfdbResult, nq)
        n_added = self.size()
        caps = dict(caps or {})
        if sentinel is not None:
            C.memset(R, sentinel, C.sizeof(R))
        for i, q in enumerate(queries):
            self._query(Q[i], q, keep)
            o = {}
            for name, group, dt, _ in _KFDB_LISTS:
                if group != "candidates" and group not in lists:
                    setattr(R[i], name, None)
                    continue
                cap = int(caps.get(group, n_added))
                o[name] = _out(max(cap, 1), dt, sentinel, bytewise=True)
                setattr(R[i], name, o[name].ctypes.data)
                setattr(R[i], "cap_" + group, cap)
            outs.append(o)
        return Q, R, keep, outs

    def detect(self, queries, host=False, lists=("scored", "sharing"), caps=None, sentinel=None):
        """aos2_kfdb_detect (host=True: aos2_debug_kfdb_host) -> one dict per query: the fields of aos2_kfdb_result_t, lists cut to
        their counts.  The result structs and buffers are kept in self.last (structs, arrays, the structs' bytes before the call) for a
        caller that expects a refusal."""
        nq = len(queries)
        Q, R, keep, outs = self.detect_args(queries, lists, caps, sentinel)
        self.last = (R, outs, bytes(R))
        _check((self.L.aos2_debug_kfdb_host if host else self.L.aos2_kfdb_detect)(self.h, Q, R, nq))
        res = []
        for i in range(nq):
            d = {k: int(getattr(R[i], k)) for k in _KFDB_SCALARS}
            d["best_acc_score"] = np.float32(R[i].best_acc_score)
            for name, group, dt, cnt in _KFDB_LISTS:
                if name in outs[i]:
                    d[name] = outs[i][name][: d[cnt]].copy()
            res.append(d)
        return res

    def scores(self, query, slots, host=False):
        """aos2_kfdb_scores (host=True: its host tap): the loop of LoopClosing::DetectLoop -> (float32 scores, their minimum from 1)"""
        Q, keep = _KfdbQuery(), []
        self._query(Q, query, keep)
        s = np.ascontiguousarray(slots, np.int32)
        out, mn = np.zeros(max(len(s), 1), np.float32), C.c_float(-1.0)
        f = self.L.aos2_debug_kfdb_scores_host if host else self.L.aos2_kfdb_scores
        _check(f(self.h, C.byref(Q), _p(s), len(s), _p(out), C.byref(mn)))
        return out[: len(s)], np.float32(mn.value)
