"""Writes tests/golden/vgicp/vgicp_cases.npz: what tests/vgicp_ref.py (the definition of lisreg_vgicp_*) makes of the seeded scenes of
tests/test_vgicp.py — the voxels of the loop-verification scene (cell ids and counts of all, means and covariances of every eighth, a
check sum of every eighth neighbour row), the 28 sums, their sums of magnitudes and pair counts of the one-linearisation cases, and
transform, iteration / evaluation / rejection counts, convergence flag and smallest margins of the four alignments.  The inputs come
from lisreg.synth with fixed seeds and are not stored.

  python tests/golden/make_golden_vgicp.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lis-slam_amd"))

import vgicp_ref as R  # noqa: E402


def main():
    g = R.golden_cases()
    for (seed, trans, rot, eps), c, f in zip(R.ALIGN_CASES, g["align_counts"], g["align_fig"]):
        print(f"seed {seed} trans {trans} rot {rot} eps {eps}: converged {c[0]}, iters {c[1]}, evals {c[2]}, rejected {c[3]}, pairs {c[4]}; "
              f"{1e3 * f[7]:.2f} mm / {1e3 * f[8]:.3f} mrad from the truth (guess {1e3 * f[9]:.0f} mm / {1e3 * f[10]:.1f} mrad); margins: "
              f"rho {f[2]:.2e}, convergence {f[3]:.2e}, voxel face {f[4]:.2e} m, neighbour gap target {f[5]:.2e} source {f[6]:.2e}")
        assert f[2] >= 1e-6 and f[3] >= 1e-6 and f[4] >= 1e-9 and f[5] >= 1e-6 and f[6] >= 1e-6, "a borderline decision: pick another seed"
    path = os.path.join(HERE, "vgicp", "vgicp_cases.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
