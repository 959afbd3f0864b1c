"""Writes tests/golden/pretreat/pretreat_sweeps.npz (a directory of its own: tests/test_golden.py takes every .npz directly under
tests/golden/ for a registration case): three small seeded raw sweeps (one per beam table; NaN / inf / zero points injected, the
64-beam sweep with invalid first and last points) and what tests/pretreat_ref.py makes of them.

  python tests/golden/make_golden_pretreat.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pretreat_ref as R  # noqa: E402

CASES = (dict(n_scan=16, seed=101, order="time", span=1.97, n_az=200),
         dict(n_scan=32, seed=102, order="ring", span=2.04, n_az=120),
         dict(n_scan=64, seed=103, order="shuffled", span=2.0, n_az=80, bad_ends=True))


def main():
    out = {}
    for c in CASES:
        ns = c["n_scan"]
        raw = R.make_sweep(**c)
        assert len(raw) <= 8000
        res = R.pretreat_sequential(raw, ns)
        assert R.same(res, R.pretreat_vectorised(raw, ns)) is None
        out[f"raw{ns}"] = raw
        out[f"index{ns}"] = res["index"].astype(np.int32)
        out[f"ring{ns}"] = res["ring"]
        out[f"time{ns}"] = res["time"]
        out[f"header{ns}"] = np.array([res["start_ori"], res["end_ori"]], np.float32)
        out[f"half{ns}"] = np.array([res["half_index"]], np.int32)
    path = os.path.join(HERE, "pretreat", "pretreat_sweeps.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
