"""Motion compensation of sweep batches on one GPU: the batched IMU de-skew (lisreg_extract_features_deskew_batch) and the
constant-velocity model (lisreg_adjust_cloud_batch), each against its single calls.  Prints one JSON line.

Sweeps: synthetic_raw_drive (64 x 1800 by default) as device records with their device times, --batch of them, each with its own IMU
table (500 Hz, 70 entries) and its own velocity.  After a warm-up, per repetition and alternating inside the same run (host clock,
every call ends in a synchronise):

  leg 1   extract_features_deskew_batch_device on the batch, against the same sweeps through single extract_features_device(..., deskew)
          calls — the only way to get these clouds without the batch call;
  leg 2   extract_features_batch_device on the same batch: the difference from leg 1 is the cost of the de-skew;
  leg 3   adjust_cloud_batch_device on the batch against single adjust_cloud_device calls, with the bytes moved per second (the kernel
          reads 20 B and writes 20 B per point).

Medians over --reps repetitions, per sweep; next to every ratio stands the inter-quartile spread of its reference leg (the single
calls).  Per-kernel times come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/motion_bench.py --reps 5`.

  python tools/motion_bench.py [--reps 20] [--batch 64] [--h 64] [--w 1800]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402

NAMES = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")


def imu_tables(seed, t0, n=70, rate=500.0):
    """integrated IMU rotation like imuDeskewInfo builds it: first entry zero, a smooth yaw-dominant motion"""
    rng = np.random.default_rng(seed)
    t = t0 - 0.01 + np.arange(n) / rate
    w = np.stack([0.05 * np.sin(6 * (t - t0)), 0.03 * np.cos(4 * (t - t0)), 0.6 + 0.2 * np.sin(3 * (t - t0))], 1) + rng.normal(0, 0.01, (n, 3))
    rot = np.zeros((n, 3))
    rot[1:] = np.cumsum(w[1:] * np.diff(t)[:, None], 0)
    return t, rot


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
    cap, pts_cap = a.h * a.w, max(len(c) for c in clouds)
    recs, ns, ins, times = [], [], [], []
    for s in range(S):
        c = clouds[s % len(clouds)]
        rec = np.zeros((len(c), 4), np.float32)
        rec[:, 0], rec[:, 1], rec[:, 2] = c["x"], c["y"], c["z"]
        rec[:, 3] = c["ring"].astype(np.uint32).view(np.float32)
        recs.append(rec); ns.append(len(c)); ins.append(D(rec)); times.append(D(np.ascontiguousarray(c["time"])))
    dks = []
    for s in range(S):
        t, rot = imu_tables(s, 100.0 + s)
        dks.append(lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0 + s, time_device_ptr=times[s].ptr))
    motions = [lisreg.make_motion((10.0 + 0.1 * s, -0.5, 0.1), (0.01, -0.02, 0.3 + 0.005 * s)) for s in range(S)]
    f_outs = [{k: D(np.zeros((cap, 4), np.float32)) for k in NAMES} for _ in range(S)]
    f_ptrs = [{k: v.ptr for k, v in o.items()} for o in f_outs]
    a_out = [D(np.zeros((pts_cap, 4), np.float32)) for _ in range(S)]
    a_time = [D(np.zeros(pts_cap, np.float32)) for _ in range(S)]
    in_ptrs, t_ptrs = [b.ptr for b in ins], [b.ptr for b in times]
    t_dsk_single, t_dsk_batch, t_plain_batch, t_adj_single, t_adj_batch = [], [], [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        for s in range(S):
            ctx.extract_features_device(in_ptrs[s], ns[s], fp, f_ptrs[s], cap, dks[s])
        t1 = time.perf_counter()
        ctx.extract_features_deskew_batch_device(in_ptrs, ns, fp, dks, f_ptrs, cap)
        t2 = time.perf_counter()
        ctx.extract_features_batch_device(in_ptrs, ns, fp, f_ptrs, cap)
        t3 = time.perf_counter()
        for s in range(S):
            ctx.adjust_cloud_device(in_ptrs[s], ns[s], t_ptrs[s], motions[s], a_out[s].ptr, a_time[s].ptr, pts_cap)
        t4 = time.perf_counter()
        ctx.adjust_cloud_batch_device(in_ptrs, ns, t_ptrs, motions, [b.ptr for b in a_out], [b.ptr for b in a_time], pts_cap)
        t5 = time.perf_counter()
        if r >= a.warmup:
            for lst, dt in ((t_dsk_single, t1 - t0), (t_dsk_batch, t2 - t1), (t_plain_batch, t3 - t2), (t_adj_single, t4 - t3), (t_adj_batch, t5 - t4)):
                lst.append(1e3 * dt / S)
    ctx.close()
    ds, ds_iqr = quartiles(t_dsk_single)
    db, db_iqr = quartiles(t_dsk_batch)
    pb, _ = quartiles(t_plain_batch)
    as_, as_iqr = quartiles(t_adj_single)
    ab, ab_iqr = quartiles(t_adj_batch)
    moved = 40.0 * (sum(ns) - S) / S                                          # bytes per sweep: 20 read + 20 written per output point
    line = dict(workload="motion", shape=[a.h, a.w], batch_sweeps=S, points_per_sweep=int(np.mean(ns)), reps=a.reps,
                deskew_single_ms_per_sweep=round(ds, 4), deskew_single_spread_ms=round(ds_iqr, 4),
                deskew_batch_ms_per_sweep=round(db, 4), deskew_batch_spread_ms=round(db_iqr, 4), deskew_batch_over_single=round(db / ds, 4),
                plain_batch_ms_per_sweep=round(pb, 4), deskew_cost_ms_per_sweep=round(db - pb, 4),
                adjust_single_ms_per_sweep=round(as_, 4), adjust_single_spread_ms=round(as_iqr, 4),
                adjust_batch_ms_per_sweep=round(ab, 4), adjust_batch_spread_ms=round(ab_iqr, 4), adjust_batch_over_single=round(ab / as_, 4),
                adjust_batch_gb_per_s=round(moved / (ab * 1e-3) / 1e9, 3), adjust_single_gb_per_s=round(moved / (as_ * 1e-3) / 1e9, 3),
                what="per sweep, medians; *_spread_ms: inter-quartile range; deskew_*: extract_features with the IMU de-skew, single calls "
                     "against one batch call; plain_batch: the same batch without de-skew; adjust_*: lisreg_adjust_cloud, single calls "
                     "against one batch call, 40 bytes moved per point")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
