"""Writes tests/golden/ndt/ndt_cases.npz: what tests/ndt_ref.py (the definition of lisreg_ndt_*) makes of the seeded scenes of
tests/test_ndt.py — the valid voxels of the planted cloud and of the loop-verification scene (cell ids and counts of all, means and
inverse covariances of every eighth of the scene's), the 28 sums, their sums of magnitudes and pair counts of the one-evaluation cases,
and pose, iteration / evaluation counts, convergence flag and smallest decision margin of the four alignments.  The inputs come from
lisreg.synth with fixed seeds and are not stored.

  python tests/golden/make_golden_ndt.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lis-slam_amd"))

import ndt_ref as R  # noqa: E402


def main():
    g = R.golden_cases()
    for (seed, trans, rot, ls), c, p in zip(R.ALIGN_CASES, g["align_counts"], g["align_p"]):
        print(f"seed {seed} trans {trans} rot {rot} line_search {ls}: iters {c[0]}, evals {c[1]}, converged {c[2]}, "
              f"{1e3 * p[8]:.2f} mm / {1e3 * p[9]:.3f} mrad from the truth, smallest margin {p[7]:.2e}")
        assert p[7] > 1e-6, "a borderline decision: pick another seed"
    path = os.path.join(HERE, "ndt", "ndt_cases.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
