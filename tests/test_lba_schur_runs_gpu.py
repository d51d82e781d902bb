"""k_schur on the windows of tests/lba_schur_cases.py (tap: aos2_debug_lba_assemble_device, stage 0): item counts on both sides of a
row of 16 lanes, DIAG units on both sides of one stride and with three items in a thread, windows without a PACK unit, with one
row, with padded units, and with 1 .. 9 PACK units.  Required: the omega condition of tests/test_lba_system_gpu.py against
tests/lba_system_ref.py (imported: the same reference, the same factor 4 over the float64 models), Hs symmetric bit for bit, and
the same bits for a window alone, in a batch of three in either order, among all windows, and on a second handle -- the task list
differs between these, so a sum that took a neighbour's row, or a unit that ran twice or not at all, shows."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_schur_cases as SC  # noqa: E402
import lba_system_ref as S  # noqa: E402
from test_lba_system_gpu import bits, check_family, structure  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("Hll", "b_l", "Hs", "bs", "Hpp_init", "b_init", "b_p", "lam", "current_chi")


def run(ba, cases):
    got = ba.debug_assemble([c["win"] for c in cases], layout="slots", stage=0)
    for g in got:
        g["lam_passed"] = None
    return got


@pytest.fixture(scope="module")
def ba(pkg, gpu):
    return pkg.LocalBA()


@pytest.fixture(scope="module")
def together(ba):
    """all windows in one call; shared and left unchanged"""
    return run(ba, SC.cases())


def test_the_windows_have_the_shapes_they_claim(together):
    for c, g in zip(SC.cases(), together):
        kinds, counts, n_pack, trace = S.unit_kinds(g["blk_off"], g["np"])
        unit_kind = g["units"] >> 28
        assert (unit_kind == 0).sum() == g["np"] and (unit_kind == 2).sum() == n_pack, c["name"]
        name = c["name"]
        if name.startswith("off"):
            assert counts[(0, 1)] == int(name[3:]) and kinds[(0, 1)] == "PACK" and n_pack == 1
        elif name == "diag":
            assert tuple(counts[(i, i)] for i in range(g["np"])) == SC.DIAG_OBS
        elif name == "np1":
            assert g["np"] == 1 and n_pack == 0 and len(g["units"]) == 1
        elif name == "np7":
            assert g["np"] == 7 and any(pad and rows < 16 for _, _, rows, at, pad in trace)
        else:
            assert n_pack == int(name[5:]) and (unit_kind == 1).sum() == 0, (name, n_pack)
    assert {int(c["name"][5:]) for c in SC.cases() if c["name"].startswith("units")} == set(SC.UNIT_COUNTS)


def test_omega_condition_and_symmetry(together):
    """`structure` (inside check_family) holds Hs symmetric bit for bit, the tail and the empty blocks exactly"""
    for c, g in zip(SC.cases(), together):
        structure(c, g)
    check_family("schur", SC.cases(), together)


def test_same_bits_alone_in_batches_and_on_a_second_handle(pkg, ba, together):
    cases = SC.cases()
    base = dict(zip((c["name"] for c in cases), together))
    three = [SC.by_name(n) for n in SC.BATCH]
    other = pkg.LocalBA()
    runs = [("alone", [[c] for c in cases], ba), ("batch of three", [three], ba), ("batch of three, other order", [[three[2], three[0], three[1]]], ba),
            ("second handle", [cases[::-1]], other), ("alone, second handle", [[c] for c in three], other)]
    try:
        for what, batches, handle in runs:
            for batch in batches:
                for c, g in zip(batch, run(handle, batch)):
                    for k in KEYS:
                        assert bits(base[c["name"]][k]) == bits(g[k]), f"{what}: {k} of window {c['name']} differs"
    finally:
        other.close()
