"""Writes tests/golden/rangenet/rangenet_knn_16x128.npz: the sweep, pixel indices and invalid mask of tests/golden/rangenet/
rangenet_16x128.npz (the same seeded 16-beam sweep with the deciding cases injected, projected at 16 x 128) and what
tests/rangenet_knn_ref.py makes of them and of THAT file's stand-in logits (160 KB that are not stored twice) with the default kNN
parameters (5, 5, 1.0, 1.0, no_vote_label 0): the range image and the cleaned-up labels, next to the plain labels and the label image
they start from.

  python tests/golden/make_golden_rangenet_knn.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import pretreat_ref as PR  # noqa: E402
import rangenet_knn_ref as KR  # noqa: E402
import rangenet_ref as R  # noqa: E402

FOV = (15.0, -15.0)
MEANS = (12.12, 10.88, 0.23, -1.04, 0.21)
STDS = (12.32, 11.47, 6.91, 0.86, 0.16)


def main():
    P = R.Params(16, 128, FOV[0], FOV[1], MEANS, STDS, 20)
    raw = R.inject(PR.make_sweep(301, 16, "shuffled", n_az=230), 301, P)
    assert len(raw) <= 4000
    res = R.project_literal(raw, P)
    logits, _ = R.stand_in_logits(res["tensor"], P, 302)
    labels, image = R.label_parallel(res["pixel_index"], res["invalid_mask"], logits, P)
    K = KR.Knn()
    knn_labels, image2, rimg = KR.knn_literal(raw, res["pixel_index"], res["invalid_mask"], logits, P, K)
    b, _, rimg_b = KR.knn_parallel(raw, res["pixel_index"], res["invalid_mask"], logits, P, K)
    assert np.array_equal(knn_labels, b) and np.array_equal(image, image2) and np.array_equal(rimg.view(np.uint32), rimg_b.view(np.uint32))
    path = os.path.join(HERE, "rangenet", "rangenet_knn_16x128.npz")
    sibling = np.load(os.path.join(HERE, "rangenet", "rangenet_16x128.npz"))
    assert np.array_equal(sibling["raw"].view(np.uint32), raw.view(np.uint32)) and np.array_equal(sibling["logits"].view(np.uint32), logits.view(np.uint32))
    np.savez_compressed(path, raw=raw, fov=np.array(FOV, np.float64), means=np.array(MEANS, np.float32), stds=np.array(STDS, np.float32),
                        pixel_index=res["pixel_index"], invalid_mask=res["invalid_mask"], labels=labels, label_image=image,
                        knn_params=np.array([K.knn, K.search, K.sigma, K.cutoff, K.no_vote_label], np.float64), range_image=rimg,
                        knn_labels=knn_labels)
    print(path, os.path.getsize(path), "bytes;", int((knn_labels != labels).sum()), "of", len(labels), "labels changed")


if __name__ == "__main__":
    main()
