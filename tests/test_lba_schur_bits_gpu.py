"""The bits of the reduced system: SHA-256 digests of Hs, bs and the pose part of b of the windows of tests/lba_schur_cases.py, recorded
(tests/golden/make_lba_schur_bits.py) with the build before k_schur's row sums became a reduce-scatter.  The sums keep their operands
and their tree, so every later build reproduces them."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import lba_schur_cases as SC  # noqa: E402
from make_lba_schur_bits import digests  # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(HERE, "golden", "lba_schur_bits.json")) as f:
    GOLDEN = json.load(f)


def test_the_file_covers_every_window():
    assert sorted(GOLDEN) == sorted(c["name"] for c in SC.cases())
    assert all(sorted(v) == ["Hs", "b_p", "bs"] and all(len(h) == 64 for h in v.values()) for v in GOLDEN.values())


@pytest.fixture(scope="module")
def ba(pkg, gpu):
    return pkg.LocalBA()


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_digests(ba, name):
    got = digests(ba, SC.by_name(name))
    assert got == GOLDEN[name], f"the reduced system of window {name} changed its bits: {[k for k in got if got[k] != GOLDEN[name][k]]}"
