"""Writes tests/golden/fgicp/fgicp_cases.npz: what tests/fgicp_ref.py (the definition of lisreg_fgicp_*) makes of the seeded scenes of
tests/test_fgicp.py — every eighth correspondence row of the loop-verification scene at the guess, at the truth and 100 m away with the
searches' margins, the 28 sums, their sums of magnitudes and pair counts of the one-linearisation cases (the last two with the pairs of
the guess and the sums at the truth), and transform, iteration / evaluation / rejection / pair counts and smallest margins of the four
alignments.  The inputs come from lisreg.synth with fixed seeds and are not stored.

  python tests/golden/make_golden_fgicp.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lis-slam_amd"))

import fgicp_ref as R  # noqa: E402


def main():
    g = R.golden_cases()
    for (seed, trans, rot, eps), c, f in zip(R.ALIGN_CASES, g["align_counts"], g["align_fig"]):
        print(f"seed {seed} trans {trans} rot {rot} eps {eps}: converged {c[0]}, iters {c[1]}, evals {c[2]}, rejected {c[3]}, pairs {c[4]}; "
              f"{1e3 * f[6]:.2f} mm / {1e3 * f[7]:.3f} mrad from the truth (guess {1e3 * f[8]:.0f} mm / {1e3 * f[9]:.1f} mrad); margins: "
              f"rho {f[2]:.2e}, convergence {f[3]:.2e}, nearest / second gap {f[4]:.2e}, cut-off gap {f[5]:.2e}")
        assert c[0] == 1 and f[8] >= 10.0 * f[6], "not converged, or not ten times closer: pick another seed"
        assert f[2] >= 1e-6 and f[3] >= 1e-6 and f[4] >= 1e-9 and f[5] >= 1e-9, "a borderline decision: pick another seed"
    print("pairs of the one-linearisation cases:", g["lin_pairs"].tolist(), "search margins:", g["corr_gaps"].tolist())
    path = os.path.join(HERE, "fgicp", "fgicp_cases.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
