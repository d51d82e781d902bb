"""Hand-built windows for k_schur's fixed-order sums and its strided item loops (tests/test_lba_schur_runs_gpu.py,
tests/test_lba_schur_bits_gpu.py and the generator of tests/golden/lba_schur_bits.json): the shapes at which a row sum, a
workgroup sum, the next-item prefetch or the partition of the unit list can go wrong.

    off    np = 2, an off-diagonal block of 1, 15, 16, 17, 33 items (one lane, a row short of one lane, a full row, a row and a lane,
           three rows of one PACK unit); np = 2 is also the window whose PACK unit has one used row
    diag   DIAG units of 1, 255, 256, 257 observations and 513: three items in thread 0 -- the strided loop's first, middle and last
           iteration --, two in the others
    np1    one free keyframe: no PACK unit at all
    np7    21 off-diagonal blocks whose rows would straddle a unit (lba_system_ref.PACK_COUNTS: the padded-unit case)
    units  windows of 1, 2, 3, 4, 5 and 9 PACK units: a workgroup takes one unit per entry of the task list (R = 1), and these are
           1, R - 1, R, R + 1, 2 R + 1 units for R = 2 and for R = 4 as well
"""
import numpy as np

import lba_system_ref as S

OFF_COUNTS = (1, 15, 16, 17, 33)
DIAG_OBS = (1, 255, 256, 257, 513)
UNIT_COUNTS = (1, 2, 3, 4, 5, 9)
UNITS_NP = 5
_cache = {}


def sees_diag():
    s = []
    for i, n in enumerate(DIAG_OBS):
        s += [[i, len(DIAG_OBS) + l % 2] for l in range(n)]
    return s


def sees_units(n_units):
    """np = 5 (+ 2 fixed): the first n_units - 1 off-diagonal blocks in rank order hold 241 .. 256 items (16 rows: a PACK unit each), the
    other blocks are empty (one row each: together one more unit); n_units = 1: np = 2 and one block.  Every free keyframe also has six
    landmarks of its own."""
    n_free = 2 if n_units == 1 else UNITS_NP
    full = 1 if n_units == 1 else n_units - 1
    s = []
    for k, (i, j) in enumerate(S.pairs_upper(n_free)[:full]):
        s += [[i, j, n_free + l % 2] for l in range((241, 256, 250)[k % 3])]
    for i in range(n_free):
        s += [[i, n_free + l % 2] for l in range(6)]
    return n_free, s


def cases():
    """-> list of dicts like lba_system_ref.cases (family 'schur')"""
    if "all" in _cache:
        return _cache["all"]
    c = lambda name, win: dict(name=name, win=win, stage=0, lam_factor=None, planted=None, family="schur")
    out = [c("off%d" % n, S.make_window(1100 + n, 2, 2, S.sees_counts(n))) for n in OFF_COUNTS]
    out.append(c("diag", S.make_window(1201, len(DIAG_OBS), 2, sees_diag())))
    out.append(c("np1", S.make_window(1301, 1, 2, S.sees_size(1, np.random.default_rng(1)))))
    out.append(c("np7", S.make_window(1307, S.PACK_NP, 2, S.sees_pack())))
    for n in UNIT_COUNTS:
        n_free, s = sees_units(n)
        out.append(c("units%d" % n, S.make_window(1400 + n, n_free, 2, s)))
    _cache["all"] = out
    return out


BATCH = ("np7", "units5", "diag")   # the batch of three windows, run in two orders


def by_name(name):
    return next(c for c in cases() if c["name"] == name)


def digest_arrays(g):
    """what the golden digests cover: the reduced system k_schur writes -- Hs (padded), bs, and the pose part of b"""
    return dict(Hs=g["Hs"], bs=g["bs"], b_p=g["b_p"])
