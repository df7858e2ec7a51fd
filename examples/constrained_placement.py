"""Greedy sensor placement in a room where not every cell can hold a sensor and some sensors are
already installed.

A jittered grid stands for the room.  A slab of it is blocked (a wall, furniture: nothing can be
mounted there, but the field there still matters), and three probes are already in place.  The
script prints the k picks of the unconstrained placement and of the constrained one.

The blocked cells are NOT deleted from the covariance: they stay in the complement set of every
denominator, so the mutual information still counts the uncertainty there.

    python examples/constrained_placement.py [--grid 10 10 10] [--k 8]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from vgposp_amd.data_generation import grid_points, grid_spacing  # noqa: E402
from vgposp_amd.placement_algorithm2 import placement_from_points  # noqa: E402


def run(grid=(10, 10, 10), k=8):
    """-> (unconstrained picks, constrained picks, candidate mask, installed sensors)."""
    grid = tuple(int(g) for g in grid)
    X = grid_points(grid, jitter=0.05, seed=0)
    ls = 2.0 * grid_spacing(grid)
    ijk = np.stack(np.unravel_index(np.arange(len(X)), grid), axis=1)
    # a slab across the middle of the first axis, two cells thick, open on one side
    blocked = (np.abs(ijk[:, 0] - grid[0] // 2) <= 1) & (ijk[:, 1] < (2 * grid[1]) // 3)
    candidates = ~blocked
    installed = [int(np.ravel_multi_index(c, grid)) for c in
                 [(0, 0, 0), (grid[0] - 1, grid[1] - 1, grid[2] - 1), (0, grid[1] - 1, grid[2] // 2)]]
    free = placement_from_points(X, k, "eq", 1.0, ls)
    con = placement_from_points(X, k, "eq", 1.0, ls, candidates=candidates, placed=installed)
    return [int(a) for a in free], [int(a) for a in con], candidates, installed


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--grid", type=int, nargs=3, default=[10, 10, 10])
    ap.add_argument("--k", type=int, default=8, help="sensors to place")
    a = ap.parse_args()
    free, con, candidates, installed = run(a.grid, a.k)
    grid = tuple(a.grid)
    cell = lambda i: tuple(int(c) for c in np.unravel_index(i, grid))
    print(f"{int((~candidates).sum())} of {candidates.size} cells are blocked; installed sensors "
          f"at {[cell(i) for i in installed]}")
    print("unconstrained picks:", [cell(i) for i in free])
    print(f"  of which blocked: {sum(not candidates[i] for i in free)}")
    print("constrained picks:  ", [cell(i) for i in con])
    assert all(candidates[i] for i in con) and not set(con) & set(installed)


if __name__ == "__main__":
    main()
