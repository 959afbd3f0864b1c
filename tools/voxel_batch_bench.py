"""The voxel grids of a sweep batch on one GPU: lisreg_voxel_downsample_batch against the two ways there were before it.  Prints one
JSON line.

Clouds: the corner and the surface cloud of --batch sweeps (synthetic_raw_drive, 64 x 1800 by default) as extract_features_batch_device
leaves them in device memory: 2 x batch clouds, leaves 0.2 (corner) / 0.4 (surface), LISREG_FMT_DEVICE_XYZI — currentCloudInit's
downSizeFilterCorner / downSizeFilterSurf.  After a warm-up, per repetition and alternating inside the same run (host clock, every
call ends in a synchronise):

  leg 1   voxel_downsample_batch_device: all clouds in one call;
  leg 2   the same clouds through voxel_downsample_multi_device in groups of 8 — the fastest way before the batch call;
  leg 3   the same clouds through single voxel_downsample_device calls;
  leg 4/5 a batch of ONE cloud (the first surface cloud) against its single call: the batch form is expected to gain nothing there.

The three legs' counts are compared once (the bytes are the tests' business).  Medians over --reps repetitions, per cloud; next to
every median stands its inter-quartile spread.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/voxel_batch_bench.py --reps 5`.

  python tools/voxel_batch_bench.py [--reps 20] [--batch 64] [--h 64] [--w 1800]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402

NAMES = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")


def quartiles(v):
    q = np.percentile(v, [25, 50, 75])
    return float(q[1]), float(q[2] - q[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--sweeps", type=int, default=4, help="different sweeps the batch cycles through")
    a = ap.parse_args()
    import lisreg
    from lisreg import replay
    clouds = [sw for sw, _ in replay.synthetic_raw_drive(a.sweeps, a.h, a.w)]
    S = a.batch
    D = lisreg.DeviceArray
    ctx = lisreg.Context(0)
    fp = lisreg.FeatureParams(a.h, a.w, 2, 0.0, 70.0, 1.0, 0.1)
    cap = a.h * a.w
    ns, ins = [], []
    for s in range(S):
        c = clouds[s % len(clouds)]
        rec = np.zeros((len(c), 4), np.float32)
        rec[:, 0], rec[:, 1], rec[:, 2] = c["x"], c["y"], c["z"]
        rec[:, 3] = c["ring"].astype(np.uint32).view(np.float32)
        ns.append(len(c)); ins.append(D(rec))
    f_outs = [{k: D(np.zeros((cap, 4), np.float32)) for k in NAMES} for _ in range(S)]
    counts = ctx.extract_features_batch_device([b.ptr for b in ins], ns, fp, [{k: v.ptr for k, v in o.items()} for o in f_outs], cap)
    for b in ins:
        b.free()
    in_ptrs = [f_outs[s][k].ptr for s in range(S) for k in ("corner", "surface")]
    n = [counts[s][k] for s in range(S) for k in ("corner", "surface")]
    leafs = [0.2, 0.4] * S
    K = 2 * S
    outs = [D(np.zeros((max(m, 1), 4), np.float32)) for m in n]
    out_ptrs = [o.ptr for o in outs]
    caps = [max(m, 1) for m in n]
    one = 1 if K > 1 else 0                                  # the first surface cloud

    def leg_batch():
        return ctx.voxel_downsample_batch_device(in_ptrs, n, leafs, out_ptrs, caps, intensity=True)[0]

    def leg_multi():
        got = []
        for g in range(0, K, 8):
            got += ctx.voxel_downsample_multi_device(in_ptrs[g:g + 8], n[g:g + 8], leafs[g:g + 8], out_ptrs[g:g + 8], caps[g:g + 8], intensity=True)
        return got

    def leg_single():
        return [ctx.voxel_downsample_device(in_ptrs[j], n[j], leafs[j], out_ptrs[j], caps[j], intensity=True)[1] if n[j] else 0 for j in range(K)]

    def leg_batch_one():
        return ctx.voxel_downsample_batch_device(in_ptrs[one:one + 1], n[one:one + 1], leafs[one:one + 1], out_ptrs[one:one + 1], caps[one:one + 1], intensity=True)[0]

    def leg_single_one():
        return [ctx.voxel_downsample_device(in_ptrs[one], n[one], leafs[one], out_ptrs[one], caps[one], intensity=True)[1]]

    legs = (leg_batch, leg_multi, leg_single, leg_batch_one, leg_single_one)
    times = [[] for _ in legs]
    n_out = None
    for r in range(a.warmup + a.reps):
        got = []
        for k, leg in enumerate(legs):
            t0 = time.perf_counter()
            got.append(leg())
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[k].append(1e3 * dt / (K if k < 3 else 1))
        assert got[0] == got[1] == got[2] and got[3] == got[4] == [got[0][one]], "the legs disagree on the voxel counts"
        n_out = got[0]
    ctx.close()
    (b, b_iqr), (m, m_iqr), (s, s_iqr), (b1, b1_iqr), (s1, s1_iqr) = [quartiles(t) for t in times]
    line = dict(workload="voxel_batch", shape=[a.h, a.w], batch_sweeps=S, clouds=K, reps=a.reps, points_in=int(sum(n)), voxels_out=int(sum(n_out)),
                corner_points_per_cloud=int(np.mean(n[0::2])), surface_points_per_cloud=int(np.mean(n[1::2])),
                batch_ms_per_cloud=round(b, 5), batch_spread_ms=round(b_iqr, 5),
                multi8_ms_per_cloud=round(m, 5), multi8_spread_ms=round(m_iqr, 5),
                single_ms_per_cloud=round(s, 5), single_spread_ms=round(s_iqr, 5),
                batch_ms_per_call=round(b * K, 4), multi8_ms_all_groups=round(m * K, 4), single_ms_all_calls=round(s * K, 4),
                batch_over_multi8=round(b / m, 4), batch_over_single=round(b / s, 4),
                faster_than_multi8_by_more_than_its_spread=bool(m - b > m_iqr),
                one_cloud_points=int(n[one]), one_cloud_batch_ms=round(b1, 5), one_cloud_batch_spread_ms=round(b1_iqr, 5),
                one_cloud_single_ms=round(s1, 5), one_cloud_single_spread_ms=round(s1_iqr, 5), one_cloud_batch_over_single=round(b1 / s1, 4),
                what="per cloud, medians over reps, host clock; *_spread_ms: inter-quartile range; batch: one lisreg_voxel_downsample_batch "
                     "call; multi8: lisreg_voxel_downsample_multi in groups of 8; single: one lisreg_voxel_downsample per cloud; one_cloud_*: "
                     "a batch of one cloud against its single call, per call")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
