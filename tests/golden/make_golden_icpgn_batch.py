"""Records what lisreg_icp_gn_match returns for the inputs of tests/icpgn_batch_cases.py: the eight small sources under the two parameter
sets and the three large sources, 80 bytes each, into icpgn_batch/icpgn_parent_outputs.npz.

It was run on the MI355X on the commit BEFORE k_icpgn_assoc / k_icpgn_solve were split into the device functions the batch kernels
share; tests/test_icpgn_batch.py holds the single call to these bytes.  Run it again only to record a deliberate change of the single
call's arithmetic.

    python tests/golden/make_golden_icpgn_batch.py [out.npz]"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "lis-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import lisreg
    import icpgn_batch_cases as K
    if os.environ.get("LISREG_NN1_Q"):
        raise SystemExit("LISREG_NN1_Q is set: the lanes per query would not be the default ones")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "icpgn_batch", "icpgn_parent_outputs.npz")
    ctx = lisreg.Context(0)
    K.set_targets(ctx)
    small = K.small_single_all(ctx)
    K.set_targets(ctx, large=True)
    large = K.large_single_all(ctx)
    ctx.close()
    small = np.frombuffer(b"".join(b"".join(row) for row in small), np.uint8).reshape(len(K.PARAM_SETS), 8, 80)
    large = np.frombuffer(b"".join(large), np.uint8).reshape(3, 80)
    np.savez_compressed(out, small=small, large=large)
    for s, row in enumerate(small):
        for k, r in enumerate(row):
            v = r.view(np.float32); i = r.view(np.int32)
            print(f"set {s} item {k}: steps {i[16]} n_corr {i[17]} fitness {v[18]:.6g} t {v[3]:.5f} {v[7]:.5f} {v[11]:.5f}")
    for k, r in enumerate(large):
        v = r.view(np.float32); i = r.view(np.int32)
        print(f"large {k}: steps {i[16]} n_corr {i[17]} fitness {v[18]:.6g}")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
