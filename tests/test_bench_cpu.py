"""bench.py's host side without a GPU: the --dump-outputs helpers and the options that need --full."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the module only: main() runs under __main__)


def test_dump_rows_are_a_fixed_sample():
    assert (bench.dump_rows(10) == np.arange(10)).all()
    r = bench.dump_rows(512)
    assert len(r) == bench.DUMP_ROWS and len(set(r.tolist())) == bench.DUMP_ROWS and (np.diff(r) > 0).all() and r.max() < 512
    assert (bench.dump_rows(512) == r).all()


def test_keypoint_table_and_masks(pkg):
    KP = pkg.capi.KP_DTYPE
    rec = np.zeros((2, 3), KP)
    rec["x"], rec["octave"], rec["class_id"] = 1.5, 7, -1
    raw = rec.view(np.float32).reshape(2, 3, 7)   # the device layout: 7 words per keypoint, octave / class_id as int32 bits
    t = bench.keypoint_table(raw, np.array([2, 0]), KP)
    assert t.dtype == np.float64 and t.shape == (2, 3, 7)
    assert (t[0, :2, 0] == 1.5).all() and (t[0, :2, 5] == 7).all() and (t[0, :2, 6] == -1).all()
    assert (t[0, 2] == 0).all() and (t[1] == 0).all()
    d = bench.per_keypoint(np.full((2, 3, 4), 9, np.uint8), np.array([1, 3]))
    assert (d[0, 0] == 9).all() and (d[0, 1:] == 0).all() and (d[1] == 9).all()


def test_dump_outputs_types_and_limit(tmp_path):
    bench.dump_outputs(str(tmp_path / "o"), {"a": np.arange(4, dtype=np.int32), "b": np.ones(3, np.uint8), "c": np.ones(2, np.float32),
                                              "d": [1.0, 2.0]})
    got = {k: np.load(tmp_path / "o" / (k + ".npy")) for k in "abcd"}
    assert got["a"].dtype == np.float64 and (got["a"] == np.arange(4)).all()
    assert got["b"].dtype == np.float32 and got["c"].dtype == np.float32 and got["d"].dtype == np.float64
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": np.zeros(bench.DUMP_LIMIT // 8 + 1)})
    assert not (tmp_path / "big").exists()


def test_verify_needs_full():
    """the oracle check of the last timed step is part of --full: asking for it in a plain run is an error, not a silent no-op"""
    r = subprocess.run([sys.executable, "bench.py", "--verify"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr
