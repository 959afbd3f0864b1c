"""Laser pretreatment (lisreg_pretreat) on one GPU against the host stand-in it replaces: prints one JSON line.

Sweeps: synthetic_raw_drive (64 x 1800 by default) with ring and time discarded, i.e. (n, 4) float32 records as KITTI stores them,
under the 64-beam table.  After a warm-up, per repetition and alternating in the same run (host clock, every call ends in a synchronise):

  parent path   replay.kitti_rings(raw) on the host + Context.upload_cloud of its PointXYZIRT structs — what DeviceOdomReplayer does per
                frame in front of the feature extraction;
  new path      Context.upload_cloud of the raw records as they are + Context.pretreat_device;
  batch         Context.pretreat_batch_device over --batch sweeps already in HBM, per sweep, next to pretreat_device alone (no upload) on
                the same sweeps.

Medians over --reps calls; `spread` is the parent path's own run-to-run spread (inter-quartile range of its calls).  Per-kernel times
come from a separate run under `rocprofv3 --kernel-trace --stats -- python tools/pretreat_bench.py --reps 50`.

  python tools/pretreat_bench.py [--reps 200] [--batch 64] [--h 64] [--w 1800]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--sweeps", type=int, default=4, help="different sweeps the calls cycle through")
    a = ap.parse_args()
    import lisreg
    from lisreg import replay
    raws = []
    for sw, _ in replay.synthetic_raw_drive(a.sweeps, a.h, a.w):
        raws.append(np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32))
    cap = max(len(r) for r in raws)
    ctx = lisreg.Context(0)
    P = lisreg.default_pretreat_params(64)
    z4, z1 = np.zeros((cap, 4), np.float32), np.zeros(cap, np.float32)
    d_in, d_out, d_time, d_old = lisreg.DeviceArray(z4), lisreg.DeviceArray(z4), lisreg.DeviceArray(z1), lisreg.DeviceArray(z4)
    t_old, t_new, kept = [], [], None
    for r in range(a.warmup + a.reps):
        raw = raws[r % len(raws)]
        t0 = time.perf_counter()
        pre = replay.kitti_rings(raw)
        ctx.upload_cloud(pre, d_old.ptr)
        t1 = time.perf_counter()
        ctx.upload_cloud(raw, d_in.ptr)
        res = ctx.pretreat_device(d_in.ptr, len(raw), P, d_out.ptr, d_time.ptr, cap)
        t2 = time.perf_counter()
        if r >= a.warmup:
            t_old.append(1e3 * (t1 - t0)); t_new.append(1e3 * (t2 - t1))
        kept = (len(pre), res["n"])
    # batch against single calls, device-resident inputs
    S = a.batch
    ins = [lisreg.DeviceArray(raws[s % len(raws)]) for s in range(S)]
    outs = [lisreg.DeviceArray(z4) for _ in range(S)]
    times = [lisreg.DeviceArray(z1) for _ in range(S)]
    ns = [len(raws[s % len(raws)]) for s in range(S)]
    t_single, t_batch = [], []
    reps_b = max(a.reps // 8, 5)
    for r in range(2 + reps_b):
        t0 = time.perf_counter()
        for s in range(S):
            ctx.pretreat_device(ins[s].ptr, ns[s], P, outs[s].ptr, times[s].ptr, cap)
        t1 = time.perf_counter()
        ctx.pretreat_batch_device([b.ptr for b in ins], ns, P, [b.ptr for b in outs], [b.ptr for b in times], cap)
        t2 = time.perf_counter()
        if r >= 2:
            t_single.append(1e3 * (t1 - t0) / S); t_batch.append(1e3 * (t2 - t1) / S)
    ctx.close()
    q = np.percentile(t_old, [25, 50, 75])
    line = dict(workload="pretreat", shape=[a.h, a.w], points=int(len(raws[0])), kept_host_stand_in=int(kept[0]), kept=int(kept[1]), reps=a.reps,
                parent_path_ms=round(float(q[1]), 4), parent_path_spread_ms=round(float(q[2] - q[0]), 4),
                new_path_ms=round(float(np.median(t_new)), 4), new_path_spread_ms=round(float(np.subtract(*np.percentile(t_new, [75, 25]))), 4),
                device_single_ms_per_sweep=round(float(np.median(t_single)), 4), batch_sweeps=S,
                device_batch_ms_per_sweep=round(float(np.median(t_batch)), 4),
                what="parent: replay.kitti_rings on the host + upload_cloud; new: upload_cloud of the raw records + pretreat_device; "
                     "device_*: inputs already in HBM, single calls against one batch call")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
