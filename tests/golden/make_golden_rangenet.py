"""Writes tests/golden/rangenet/rangenet_16x128.npz (a directory of its own: tests/test_golden.py takes every .npz directly under
tests/golden/ for a registration case): one small seeded 16-beam sweep with the deciding cases injected (duplicates, origin points,
near points, elevations outside the field of view, the yaw seam, non-finite points), projected at 16 x 128 with non-trivial means and
stds, and what tests/rangenet_ref.py makes of it: pixel indices, tensor, invalid mask, stand-in logits and the labels they give.

  python tests/golden/make_golden_rangenet.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pretreat_ref as PR  # noqa: E402
import rangenet_ref as R  # noqa: E402

FOV = (15.0, -15.0)
MEANS = (12.12, 10.88, 0.23, -1.04, 0.21)
STDS = (12.32, 11.47, 6.91, 0.86, 0.16)


def main():
    P = R.Params(16, 128, FOV[0], FOV[1], MEANS, STDS, 20)
    raw = R.inject(PR.make_sweep(301, 16, "shuffled", n_az=230), 301, P)
    assert len(raw) <= 4000
    res = R.project_literal(raw, P)
    assert R.same_projection(res, R.project_parallel(raw, P)) is None
    logits, _ = R.stand_in_logits(res["tensor"], P, 302)
    labels, image = R.label_parallel(res["pixel_index"], res["invalid_mask"], logits, P)
    assert np.array_equal(labels, R.label_literal(res["pixel_index"], res["invalid_mask"], logits, P)[0])
    path = os.path.join(HERE, "rangenet", "rangenet_16x128.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, raw=raw, fov=np.array(FOV, np.float64), means=np.array(MEANS, np.float32), stds=np.array(STDS, np.float32),
                        pixel_index=res["pixel_index"], tensor=res["tensor"], invalid_mask=res["invalid_mask"],
                        n_valid=np.array([res["n_valid"]], np.int32), logits=logits, labels=labels, label_image=image)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
