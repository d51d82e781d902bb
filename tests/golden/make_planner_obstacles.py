"""Writes planner_obstacles.npz: the obstacle file the reference ships, data/obs.txt (include/collisions.h:63), as doubles:
    python tests/golden/make_planner_obstacles.py <reference checkout>/data
xy [2800][2] = the columns x, y; r [2800] = the third column, 0.05 in every row.  The planner hands the rows to
collisionDetection(ppMatrix FloorMap) (src/collisions.cc:23-37), which never reads r: obs_r stays the class's 0.1
(include/collisions.h:61), and that is what the tests use."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main(data_dir):
    rows = np.loadtxt(os.path.join(data_dir, "obs.txt"), dtype=np.float64)
    assert rows.shape == (2800, 3) and (rows[:, 2] == 0.05).all()
    np.savez_compressed(os.path.join(HERE, "planner_obstacles.npz"), xy=np.ascontiguousarray(rows[:, :2]), r=np.ascontiguousarray(rows[:, 2]))


if __name__ == "__main__":
    main(sys.argv[1])
