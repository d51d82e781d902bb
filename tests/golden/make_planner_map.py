"""Writes planner_map_s.npz: the planner map the reference ships, narrowed to float32 the way camera(map_data, int) narrows map_data
(src/camera.cc:29-44).  The three text files are the ones include/OptimizationObj.h:15-17 names:
    python tests/golden/make_planner_map.py <reference checkout>/data
xyz [2681][3] = the first three columns of Corner_Map_S.txt, upper / lower [2681] = upper_bound.txt / lower_bound.txt.  The files
carry no ranges or ratios; the tests use max_range = FLT_MAX, min_range = 0, found_ratio = 1."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(data_dir):
    xyz = np.loadtxt(os.path.join(data_dir, "Corner_Map_S.txt"), dtype=np.float64)[:, :3]
    upper = np.loadtxt(os.path.join(data_dir, "upper_bound.txt"), dtype=np.float64)
    lower = np.loadtxt(os.path.join(data_dir, "lower_bound.txt"), dtype=np.float64)
    assert xyz.shape == (2681, 3) and upper.shape == lower.shape == (2681,)
    np.savez_compressed(os.path.join(HERE, "planner_map_s.npz"), xyz=xyz.astype(np.float32), upper=upper.astype(np.float32),
                        lower=lower.astype(np.float32))


if __name__ == "__main__":
    main(sys.argv[1])
