"""Writes tests/golden/gicp/gicp_cases.npz: what tests/gicp_ref.py (the definition of lisreg_gicp_*) makes of the seeded scenes of
tests/test_gicp.py — the 74 moments, their sums of magnitudes and the centre they are taken about at the guess, at the truth and 100 m
away; transform, counts and smallest margins of the five alignments; and the moment record, the outer iterate, the accepted state and
the counts of the inner minimisation of every outer iteration of every alignment (what tests/test_gicp_host.py feeds to
lisreg_gicp_inner).  The inputs come from lisreg.synth with fixed seeds and are not stored.

  python tests/golden/make_golden_gicp.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lis-slam_amd"))

import gicp_ref as R  # noqa: E402


def main():
    g = R.golden_cases()
    for (seed, trans, rot, eps), c, f in zip(R.ALIGN_CASES, g["align_counts"], g["align_fig"]):
        print(f"seed {seed} trans {trans} rot {rot} eps {eps}: converged {c[0]}, outer {c[1]}, inner {c[2]}, evals {c[3]}, rounds {c[4]}, "
              f"pairs {c[5]}, last inner exit {c[6]}; delta {f[1]:.3f}; {1e3 * f[7]:.2f} mm / {1e3 * f[8]:.3f} mrad from the truth (guess "
              f"{1e3 * f[9]:.0f} mm / {1e3 * f[10]:.1f} mrad); margins: convergence {f[2]:.2e}, nearest / second gap {f[3]:.2e}, cut-off gap "
              f"{f[4]:.2e}, smallest decision {f[5]:.2e}, f comparisons by {f[6]:.2e} eps |f|")
        assert c[0] == 1 and f[9] >= 10.0 * f[7], "not converged, or not ten times closer: pick another seed"
        assert f[2] >= 1e-6 and f[5] >= 1e-6 and f[3] >= 1e-9 and f[4] >= 1e-9, "a borderline decision: pick another seed"
    print("pairs of the moment cases:", g["mom_rec"][:, 73].tolist(), "; inner minimisations kept:", len(g["inner_rec"]))
    path = os.path.join(HERE, "gicp", "gicp_cases.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **g)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
