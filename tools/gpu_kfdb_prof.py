"""Stage driver: aos2_kfdb_detect calls on databases of 1 000 / 5 000 / 20 000 added keyframes of ~1000 words over 10^6 word ids --
places of 20 keyframes that share most of their words, neighbour rows inside a place -- for 1 and 64 RELOC queries and 1 LOOP query
with 30 excluded slots, returning the candidates (and, timed separately as with_lists_*, the scored and sharing lists too): 5 warm-up
calls, then the median of KFDB_REPS (30) calls, as wall time around the C call and as device time of its four kernels (HIP events of
the handle); one JSON line.  KFDB_HOST=1 also times the same calls through aos2_debug_kfdb_host,
this repository's own routine on one core, which walks an inverted file as the reference does (median of 5 calls).  KFDB_SIZES=1000,5000 picks the sizes.
Per kernel: rocprofv3 --kernel-trace --stats --output-format csv -- python tools/gpu_kfdb_prof.py (a run of its own)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g
pkg = g.load_package()
N_WORDS, PLACE, BASE, KEEP, EXTRA = 10 ** 6, 20, 1300, 0.7, 90


def vector(rng, base):
    w = np.unique(np.concatenate([base[rng.random(len(base)) < KEEP], rng.integers(0, N_WORDS, EXTRA)])).astype(np.uint32)
    v = rng.random(len(w)) + 0.05
    return w, v / v.sum()


def timed(db, queries, host, reps, lists=()):
    Q, R, keep, outs = db.detect_args(queries, lists=lists)
    f = db.L.aos2_kfdb_detect
    wall, dev = [], []
    for it in range(reps + 5):
        t0 = time.perf_counter()
        st = f(db.h, Q, R, len(queries))
        t1 = time.perf_counter()
        assert st == 0
        if it >= 5:
            wall.append((t1 - t0) * 1e3)
            dev.append(db.last_device_ms())
    out = dict(queries=len(queries), n_sharing=int(np.mean([R[i].n_sharing for i in range(len(queries))])),
               n_scored=int(np.mean([R[i].n_scored for i in range(len(queries))])),
               n_candidates=int(np.mean([R[i].n_candidates for i in range(len(queries))])),
               wall_ms_median=float(np.median(wall)), wall_ms_min=float(np.min(wall)), wall_ms_max=float(np.max(wall)))
    out.update(kernels_ms_median=float(np.median(dev)), kernels_ms_min=float(np.min(dev)))
    if not lists:      # the same call with the scored and the sharing list returned as well: what host/KeyFrameDatabase.h asks for
        both = timed(db, queries, False, reps, ("scored", "sharing"))
        out.update(with_lists_wall_ms_median=both["wall_ms_median"], with_lists_kernels_ms_median=both["kernels_ms_median"])
    if host:
        t = []
        for it in range(5):
            t0 = time.perf_counter()
            assert db.L.aos2_debug_kfdb_host(db.h, Q, R, len(queries)) == 0
            t.append((time.perf_counter() - t0) * 1e3)
        out["own_host_routine_one_core_ms_median"] = float(np.median(t))
    return out


def main():
    sizes = [int(s) for s in os.environ.get("KFDB_SIZES", "1000,5000,20000").split(",")]
    host, reps = bool(os.environ.get("KFDB_HOST")), int(os.environ.get("KFDB_REPS", "30"))
    V = pkg.Vocabulary(device=0)
    V.set_nodes(N_WORDS, 1, 0, 0, np.zeros(N_WORDS, np.int32), np.zeros((N_WORDS, 32), np.uint8), np.ones(N_WORDS), np.ones(N_WORDS, np.uint8))
    out = dict(words=N_WORDS, place=PLACE)
    for n in sizes:
        rng = np.random.default_rng(11)
        db = pkg.KeyFrameDatabase(V, device=0)
        bases, n_entries = [], 0
        for p in range(n // PLACE):
            bases.append(rng.choice(N_WORDS, BASE, replace=False))
            slots = []
            for _ in range(PLACE):
                w, v = vector(rng, bases[-1])
                n_entries += len(w)
                slots.append(db.put(w, v))
            db.set_neighbours(slots, [[t for t in slots if t != s][:10] for s in slots])
            for s in slots:
                db.add(s)
        places = rng.choice(len(bases), 64, replace=len(bases) < 64)
        reloc = [dict(mode=db.RELOC, **dict(zip(("words", "values"), vector(rng, bases[p])))) for p in places]
        first = int(places[0]) * PLACE
        loop = dict(reloc[0], mode=db.LOOP, excluded=np.arange(first, first + 30, dtype=np.int32) % n)
        loop["min_score"] = float(db.scores(loop, loop["excluded"])[1])
        r = dict(words_per_keyframe=n_entries // n)
        for name, queries in (("reloc_1", reloc[:1]), ("reloc_64", reloc), ("loop_1", [loop])):
            r[name] = timed(db, queries, host, reps)
        out["keyframes_%d" % n] = r
        db.close()
    print(json.dumps(out))


main()
