"""CPU model of option "row_reach" = 2 (no GPU): which grid cells get cell rows under "row_reach" = 1 (populated 5^3 block and within a
metre of a query's initial position) and under 2 (of those: a query starts in the cell, or a target point lies within --near-m metres,
in cells P = max(1, ceil(near / cell)), Chebyshev; P >= 2 is the 5^3 block itself: the rows of 1),
and how many query positions on the straight line from the initial to the true pose fall into populated cells left without rows.
    python tests/row_reach_model.py [--scans 64] [--points 200000] [--h 64] [--w 1800] [--near-m 0.5]      (defaults: bench.py's configs[1] scene)
Cost = 1.2 per cell with rows (centre row) + 1.0 per such cell with a point in its 3^3 block (octant rows)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lis-slam_amd"))
from lisreg import synth  # noqa: E402


def box(a, r):
    """a dilated (bool: any; int: sum) over the (2 r + 1)^3 block, clipped at the grid"""
    for ax in range(3):
        p = np.pad(a, [(r, r) if d == ax else (0, 0) for d in range(3)])
        n = a.shape[ax]
        parts = [np.take(p, range(s, s + n), axis=ax) for s in range(2 * r + 1)]
        a = np.logical_or.reduce(parts) if a.dtype == bool else np.sum(parts, axis=0)
    return a


def cells(xyz, o, cell, dims):
    return tuple(np.clip(np.floor((xyz - o) / cell).astype(np.int64), 0, np.array(dims) - 1).T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=64); ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64); ap.add_argument("--w", type=int, default=1800); ap.add_argument("--near-m", type=float, default=0.5)
    a = ap.parse_args()
    targets = synth.make_submap(a.points)
    scans = [synth.make_scan(a.h, a.w, 1000 + i) for i in range(a.scans)]
    T0 = [synth.perturb_pose(s["T_true"], np.random.default_rng(1000 + i + 7919)).astype(np.float64) for i, s in enumerate(scans)]
    for kind, key in enumerate(("corner", "surf")):
        tgt = synth.pcl_xyz(targets[kind]).astype(np.float64)
        area = max(1.0, np.prod(np.ptp(tgt[:, :2], axis=0)))
        cell = min(0.5, max(0.25, 2.8 / np.sqrt(len(tgt) / area)))                       # make_grid; two cells of margin for the rows
        o = tgt.min(0) - 2 * cell
        dims = tuple((np.floor((tgt.max(0) + 2 * cell - o) / cell) + 1).astype(int))
        cnt = np.zeros(dims, np.int64); np.add.at(cnt, cells(tgt, o, cell, dims), 1)
        pop5, near = box(cnt, 2) > 0, box(cnt, max(1, int(np.ceil(a.near_m / cell - 1e-3)))) > 0
        pop3 = box(cnt, 1) > 0
        fr = (0.0, 0.25, 0.5, 0.75, 0.9, 1.0)
        visits = [np.zeros(dims, np.int64) for _ in fr]
        for s, t0 in zip(scans, T0):
            q = synth.pcl_xyz(s[key]).astype(np.float64)
            for v, f in zip(visits, fr):
                M = synth.pose_matrix(t0 + f * (s["T_true"] - t0))
                np.add.at(v, cells(q @ M[:3, :3].T + M[:3, 3], o, cell, dims), 1)
        qmark = visits[0] > 0
        reach = box(qmark, min(max(int(np.ceil(1.0 / cell - 1e-3)), 2), 16))
        old, new = pop5 & reach, pop5 & (qmark | (reach & near))
        cost = lambda m: 1.2 * m.sum() + 1.0 * (m & pop3).sum()
        ever = pop5 & np.logical_or.reduce([v > 0 for v in visits])
        print(f"{key} target ({len(tgt)} points, {cell:.3f} m cells): rows for {old.sum()} cells at row_reach 1, {new.sum()} at 2 "
              f"(cost {cost(new) / cost(old):.3f} of 1's); cells ever visited cost {cost(ever & old) / cost(old):.3f}")
        for v, f in zip(visits, fr):
            w = v * pop5                                                     # (a query in a cell with an empty 5^3 block needs no row)
            print(f"    path fraction {f:.2f}: query positions in populated cells with rows: {(w * old).sum() / w.sum():.5f} at 1, {(w * new).sum() / w.sum():.5f} at 2")


if __name__ == "__main__":
    main()
