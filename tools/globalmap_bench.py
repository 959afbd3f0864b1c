"""The global map of the resident submaps (lisreg_submap_gather) on one GPU against the per-class calls it replaces: prints one JSON line.

Workload: --maps submaps (64) of about 60 k points each in the five classes (max_num_pts is 80 000), every submap under its own pose,
class mask 31 — publishGlobalMap after a loop closure has moved every pose.  After a warm-up, per repetition and alternating in the same
run (host clock, every timed stretch ends in a device synchronise):

  parent path   per submap and class: lisreg_localmap_get into a device buffer, then lisreg_transform_cloud (device records) into its place
                of the output — 2 x 5 x maps calls, each a host round trip;
  new path      one lisreg_submap_gather into the same device buffer.

Both outputs are compared bit for bit once before anything is timed.  `device_gather_event_ms` is the same call between two events on
the context's stream (table upload + kernel, without the host's launch and synchronise cost); GB/s figures count 32 B per point (one
16-byte load, one 16-byte store).  `big_*` repeats the list --big times in one call, so that the launch no longer dominates (the sources
then come out of the caches, the stores go to HBM).  Host destinations, fewer repetitions: the new call into a host array against
localmap_get to the host + the CPU oracle's transform_cloud per class.

Medians over --reps calls; `*_spread_ms` is the inter-quartile range of the same calls.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/globalmap_bench.py --reps 20`.

  python tools/globalmap_bench.py [--reps 50] [--maps 64] [--big 16]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<u4")])


def med_iqr(t):
    q = np.percentile(t, [25, 50, 75])
    return round(float(q[1]), 4), round(float(q[2] - q[0]), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--maps", type=int, default=64)
    ap.add_argument("--big", type=int, default=16, help="times the list is repeated in the large single call (0: skip)")
    a = ap.parse_args()
    import lisreg
    import oracle_ctypes as oc
    hip = lisreg.hip_runtime()
    L = lisreg.lib()
    rng = np.random.default_rng(64)
    ctx = lisreg.Context(0)
    prm = lisreg.localmap_default_params()
    share = np.array([0.05, 0.03, 0.50, 0.34, 0.08])                      # dynamic, pole, ground, building, outlier
    ids = np.arange(a.maps, dtype=np.int32)
    zero = np.zeros(6, np.float32)
    for m in ids:
        counts = (share * rng.integers(55000, 65000)).astype(int)
        cls = []
        for n in counts:
            rec = np.zeros((n, 4), np.float32)
            rec[:, :3] = rng.uniform(-60, 60, (n, 3)).astype(np.float32)
            rec.view(np.uint32)[:, 3] = rng.integers(0, 20, n, dtype=np.uint32)
            cls.append(lisreg.DeviceArray(rec))
        ctx.localmap_reset(int(m))
        ctx.submap_insert_device(int(m), [d.ptr for d in cls], [int(n) for n in counts], None, zero, prm)
        for d in cls:
            d.free()
    poses = np.concatenate([rng.uniform(-np.pi, np.pi, (a.maps, 3)), rng.uniform(-500, 500, (a.maps, 3))], 1).astype(np.float32)
    total, off = ctx.submap_gather_count(ids, 31)
    max_cls = int(np.diff(off).max())
    out_old = lisreg.DeviceArray(np.zeros((total, 4), np.float32))
    out_new = lisreg.DeviceArray(np.zeros((total, 4), np.float32))
    tmp = lisreg.DeviceArray(np.zeros((max_cls, 4), np.float32))
    n_c = C.c_int(0)

    def parent_device():
        for i, m in enumerate(ids):
            for k in range(5):
                n = int(off[5 * i + k + 1] - off[5 * i + k])
                if n == 0:
                    continue
                ctx._chk(L.lisreg_localmap_get(ctx._h, int(m), k, C.c_void_p(tmp.ptr), max_cls, C.byref(n_c)))
                ctx.transform_cloud_device(tmp.ptr, n, poses[i], out_old.ptr + 16 * int(off[5 * i + k]))
        hip.hipDeviceSynchronize()

    def new_device():
        ctx.submap_gather_device(ids, poses, out_new.ptr, total)
        hip.hipDeviceSynchronize()

    parent_device(); new_device()
    same = bool(np.array_equal(out_old.download(total).view(np.uint32), out_new.download(total).view(np.uint32)))
    if not same:
        raise SystemExit("the gather and the per-class path disagree")
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    assert hip.hipEventCreate(C.byref(ev0)) == 0 and hip.hipEventCreate(C.byref(ev1)) == 0
    stream = C.c_void_p(ctx.stream)
    ms = C.c_float(0)

    def evented(fn):
        hip.hipEventRecord(ev0, stream)
        fn()
        hip.hipEventRecord(ev1, stream)
        hip.hipEventSynchronize(ev1)
        hip.hipEventElapsedTime(C.byref(ms), ev0, ev1)
        return float(ms.value)

    t_old, t_new, t_ev = [], [], []
    for r in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        parent_device()
        t1 = time.perf_counter()
        new_device()
        t2 = time.perf_counter()
        e = evented(lambda: ctx.submap_gather_device(ids, poses, out_new.ptr, total))
        if r >= a.warmup:
            t_old.append(1e3 * (t1 - t0)); t_new.append(1e3 * (t2 - t1)); t_ev.append(e)
    line = dict(workload="globalmap", maps=int(a.maps), points=int(total), segments=int((np.diff(off) > 0).sum()), reps=a.reps, bit_equal=same)
    line["parent_device_ms"], line["parent_device_spread_ms"] = med_iqr(t_old)
    line["device_gather_ms"], line["device_gather_spread_ms"] = med_iqr(t_new)
    line["device_gather_event_ms"], line["device_gather_event_spread_ms"] = med_iqr(t_ev)
    line["device_gather_gbps"] = round(32e-6 * total / line["device_gather_ms"], 1)
    line["device_gather_event_gbps"] = round(32e-6 * total / line["device_gather_event_ms"], 1)
    line["speedup_device"] = round(line["parent_device_ms"] / line["device_gather_ms"], 1)

    if a.big > 0:
        big_ids, big_poses = np.tile(ids, a.big), np.tile(poses, (a.big, 1))
        big_total = total * a.big
        big = C.c_void_p()
        assert hip.hipMalloc(C.byref(big), C.c_size_t(16 * big_total)) == 0
        t_big = []
        for r in range(2 + max(a.reps // 4, 5)):
            e = evented(lambda: ctx.submap_gather_device(big_ids, big_poses, big.value, big_total))
            if r >= 2:
                t_big.append(e)
        hip.hipDeviceSynchronize()
        hip.hipFree(big)
        line["big_points"] = int(big_total)
        line["big_gather_event_ms"], line["big_gather_event_spread_ms"] = med_iqr(t_big)
        line["big_gather_event_gbps"] = round(32e-6 * big_total / line["big_gather_event_ms"], 1)

    # host destinations
    host_new = np.zeros((total, 4), np.float32)
    host_old = np.zeros((total, 4), np.float32)
    t_hold, t_hnew = [], []
    for r in range(1 + max(a.reps // 8, 3)):
        t0 = time.perf_counter()
        for i, m in enumerate(ids):
            for k in range(5):
                rec = ctx.localmap_get(int(m), k)
                if len(rec):
                    host_old[off[5 * i + k]:off[5 * i + k + 1]] = oc.transform_cloud(rec.view(RECORD).reshape(-1), poses[i]).view(np.float32).reshape(-1, 4)
        t1 = time.perf_counter()
        ctx.submap_gather_device(ids, poses, host_new.ctypes.data, total)
        t2 = time.perf_counter()
        if r >= 1:
            t_hold.append(1e3 * (t1 - t0)); t_hnew.append(1e3 * (t2 - t1))
    line["parent_host_ms"], line["parent_host_spread_ms"] = med_iqr(t_hold)
    line["host_gather_ms"], line["host_gather_spread_ms"] = med_iqr(t_hnew)
    line["host_gather_gbps_out"] = round(16e-6 * total / line["host_gather_ms"], 2)
    line["host_bit_equal"] = bool(np.array_equal(host_new.view(np.uint32), out_new.download(total).view(np.uint32)))
    line["what"] = ("parent_device: localmap_get to a device buffer + transform_cloud (device records) per class; device_gather: one "
                    "lisreg_submap_gather, host clock incl. synchronise; *_event: between two stream events; gbps at 32 B per point; "
                    "big: the list repeated in one call; parent_host: localmap_get to the host + the CPU oracle's transform_cloud; "
                    "host_gather: the new call into a pageable host array (gbps_out: 16 B per point over the link)")
    ctx.close()
    print(json.dumps(line))


if __name__ == "__main__":
    main()
