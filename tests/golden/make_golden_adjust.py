"""Writes tests/golden/adjust/adjust_cloud.npz (a directory of its own: tests/test_golden.py takes every .npz directly under
tests/golden/ for a registration case): 500 seeded points with their times, intensities and rings, four motions (scan period, linear
velocity, angular velocity) and what tests/adjust_ref.py makes of them.

  python tests/golden/make_golden_adjust.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import adjust_ref as R  # noqa: E402


def main():
    out = R.golden_arrays()
    for k in R.GOLDEN_MOTIONS:
        seq = R.adjust_sequential(out["xyz"], out["time"], R.MOTIONS[k])["xyz"]
        assert np.array_equal(seq.view(np.uint32), out["out_" + k].view(np.uint32)), k
    path = os.path.join(HERE, "adjust", "adjust_cloud.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
