"""The class clouds of a key-frame batch on one GPU: lisreg_semantic_split_batch against single lisreg_semantic_split calls, and the
chain's tail, lisreg_concat_device_batch against single lisreg_concat_device calls.  Prints one JSON line.

Frames: --batch labelled frames of --h x --w device records (64 x 1800 by default), random coordinates, random labels 0 .. 19 in the
payload (what lisreg_rangenet_label*_batch writes), the default label map; five output buffers of n records per frame.  After a
warm-up, per repetition and alternating inside the same run (host clock; every leg ends synchronised):

  leg 1   semantic_split_batch_device: all frames in one call;
  leg 2   the same frames through single semantic_split_device calls (the single call is the only path there was before);
  leg 3/4 a batch of ONE frame against its single call;
  leg 5   concat_device_batch: per frame (dynamic, building, ground) end to end, all frames in one call;
  leg 6   the same through single concat_device calls, then one device synchronise (the single call does not wait).

The legs' counts are compared once (the bytes are the tests' business).  Medians over --reps repetitions, per frame; next to every
median stands its inter-quartile spread.  Per-pass kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/semantic_batch_bench.py --reps 5`.

  python tools/semantic_batch_bench.py [--reps 20] [--batch 64] [--h 64] [--w 1800]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402


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
    ap.add_argument("--frames", type=int, default=4, help="different frames the batch cycles through")
    a = ap.parse_args()
    import lisreg
    D = lisreg.DeviceArray
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    S, n = a.batch, a.h * a.w
    rng = np.random.default_rng(2026)
    hosts = []
    for _ in range(a.frames):
        rec = np.zeros((n, 4), np.uint32)
        rec[:, :3] = rng.uniform(-60, 60, (n, 3)).astype(np.float32).view(np.uint32)
        rec[:, 3] = rng.integers(0, 20, n)
        hosts.append(rec)
    ins = [D(hosts[s % a.frames]) for s in range(S)]
    outs = [[D(np.zeros((n, 4), np.float32)) for _ in range(5)] for _ in range(S)]
    cats = [D(np.zeros((n, 4), np.float32)) for _ in range(S)]
    in_ptrs, ns = [b.ptr for b in ins], [n] * S
    out_ptrs, caps = [[b.ptr for b in f] for f in outs], [[n] * 5 for _ in range(S)]
    counts0 = ctx.semantic_split_batch_device(in_ptrs, ns, out_ptrs, caps)[0]
    order = (0, 2, 1)                                        # dynamic + building + ground: currentCloudInit's surf source
    c_in = [[out_ptrs[s][k] for k in order] for s in range(S)]
    c_n = [[counts0[s][k] for k in order] for s in range(S)]
    c_out, c_cap = [b.ptr for b in cats], [n] * S

    def leg_batch():
        return ctx.semantic_split_batch_device(in_ptrs, ns, out_ptrs, caps)[0]

    def leg_single():
        return [ctx.semantic_split_device(in_ptrs[s], n, out_ptrs[s], n) for s in range(S)]

    def leg_batch_one():
        return ctx.semantic_split_batch_device(in_ptrs[:1], ns[:1], out_ptrs[:1], caps[:1])[0]

    def leg_single_one():
        return [ctx.semantic_split_device(in_ptrs[0], n, out_ptrs[0], n)]

    def leg_concat_batch():
        return ctx.concat_device_batch(c_in, c_n, c_out, c_cap)

    def leg_concat_single():
        got = [ctx.concat_device(c_in[s], c_n[s], c_out[s]) for s in range(S)]
        hip.hipDeviceSynchronize()
        return got

    legs = (leg_batch, leg_single, leg_batch_one, leg_single_one, leg_concat_batch, leg_concat_single)
    per = (S, S, 1, 1, S, S)
    times = [[] for _ in legs]
    for r in range(a.warmup + a.reps):
        got = []
        for k, leg in enumerate(legs):
            t0 = time.perf_counter()
            got.append(leg())
            dt = time.perf_counter() - t0
            if r >= a.warmup:
                times[k].append(1e3 * dt / per[k])
        assert got[0] == got[1] == counts0 and got[2] == got[3] == counts0[:1] and got[4] == got[5], "the legs disagree on the counts"
    ctx.close()
    (b, b_iqr), (s, s_iqr), (b1, b1_iqr), (s1, s1_iqr), (cb, cb_iqr), (cs, cs_iqr) = [quartiles(t) for t in times]
    line = dict(workload="semantic_batch", shape=[a.h, a.w], frames=S, reps=a.reps, points_in=S * n, tile=lisreg.SEMANTIC_BATCH_TILE,
                class_counts_frame0=counts0[0],
                batch_ms_per_frame=round(b, 5), batch_spread_ms=round(b_iqr, 5), single_ms_per_frame=round(s, 5), single_spread_ms=round(s_iqr, 5),
                batch_ms_per_call=round(b * S, 4), single_ms_all_calls=round(s * S, 4), batch_over_single=round(b / s, 4),
                faster_than_single_by_more_than_the_spread=bool(s - b > max(s_iqr, b_iqr)),
                one_frame_batch_ms=round(b1, 5), one_frame_batch_spread_ms=round(b1_iqr, 5), one_frame_single_ms=round(s1, 5),
                one_frame_single_spread_ms=round(s1_iqr, 5), one_frame_batch_over_single=round(b1 / s1, 4),
                concat_batch_ms_per_job=round(cb, 5), concat_batch_spread_ms=round(cb_iqr, 5), concat_single_ms_per_job=round(cs, 5),
                concat_single_spread_ms=round(cs_iqr, 5), concat_batch_over_single=round(cb / cs, 4), concat_records_per_job=int(np.mean([sum(x) for x in c_n])),
                what="per frame, medians over reps, host clock; *_spread_ms: inter-quartile range; batch: one lisreg_semantic_split_batch call; "
                     "single: one lisreg_semantic_split per frame; one_frame_*: a batch of one frame against its single call, per call; concat_*: "
                     "one lisreg_concat_device_batch call against one lisreg_concat_device per frame followed by one device synchronise")
    print(json.dumps(line))


if __name__ == "__main__":
    main()
