"""Generator of globalmap/globalmap_small.npz: seeded class clouds of three small submaps, a list that names one of them twice, poses over the whole
angle range, and the global map tests/globalmap_ref.py makes of them (class masks 31 and 21).  Run from the repository root:
    python tests/golden/make_golden_globalmap.py
The file is reproducible: same seed, same bytes of every array."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import globalmap_ref as R  # noqa: E402

SEED = 20260117
COUNTS = {0: (0, 65, 257, 130, 1), 1: (63, 0, 300, 64, 40), 2: (256, 31, 0, 255, 0)}
IDS = (2, 0, 1, 0)


def make():
    rng = np.random.default_rng(SEED)
    store = R.make_store(rng, COUNTS)
    poses = R.agreed_poses(rng, len(IDS))
    out = dict(counts=np.array([COUNTS[m] for m in sorted(COUNTS)], np.int32), ids=np.array(IDS, np.int32), poses=poses,
               records=np.concatenate([store[m][k] for m in sorted(COUNTS) for k in range(5)]))
    for mask in (31, 21):
        cloud, off = R.global_map(store, IDS, poses, mask)
        out["cloud%d" % mask], out["off%d" % mask] = cloud, off
    return out


def store_of(g):
    """the {map id: five class arrays} store back out of the file's arrays"""
    store, o = {}, 0
    for m, cnt in enumerate(g["counts"]):
        store[m] = []
        for n in cnt:
            store[m].append(g["records"][o:o + int(n)])
            o += int(n)
    return store


if __name__ == "__main__":
    path = os.path.join(HERE, "globalmap", "globalmap_small.npz")
    np.savez_compressed(path, **make())
    print(path, os.path.getsize(path), "bytes")
