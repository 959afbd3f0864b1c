"""RangeNet++ projection and labelling (lisreg_rangenet_project / lisreg_rangenet_label) on one GPU against the host round trips they
remove: prints one JSON line and writes it to --out.

Sweeps: synthetic_raw_drive (64 x 1800 by default) as (n, 4) float32 records already in HBM, projected at --img-h x --img-w (64 x 2048)
with 20 classes.  After a warm-up, per repetition and alternating in the same run (host clock, every call ends in a synchronise):

  new path      Context.rangenet_project_device + Context.rangenet_label_device, device in, device out (the logits are a resident
                buffer: the network is not part of either path);
  transfers     the three copies any host implementation of the same two steps must make on this box, and nothing else: the sweep down
                (n x 16 B), the input tensor up (5 x H x W x 4 B), the logits down (n_classes x H x W x 4 B) — pinned hipMemcpy's;
  host stand-in the vectorised numpy restatement of the host work in between (labelled a stand-in: not the reference's loops, and not a
                pass criterion), a few repetitions only;
  batch         rangenet_project_batch_device / rangenet_label_batch_device over --batch sweeps, per sweep, next to single calls.

Medians and inter-quartile ranges over --reps calls.  Criterion (stated before the first run): the new path's median is below the
transfers' median by more than the larger of the two IQRs.  Per-kernel times come from a separate run under
`rocprofv3 --kernel-trace --stats -- python tools/rangenet_bench.py --reps 50 --no-host` (no counters in that run).

With --knn the run measures the kNN label clean-up instead (lisreg_rangenet_label_knn, default parameters unless --knn-params): per
repetition and alternating in the same run, Context.rangenet_label_device and Context.rangenet_label_knn_device on the same projected
sweep (host clock, every call ends in a synchronise), then the two batch calls over --batch sweeps per sweep; medians, IQRs and the
ratios kNN / plain.  No criterion: nobody has fixed a target for this step.

  python tools/rangenet_bench.py [--reps 200] [--batch 16] [--h 64] [--w 1800] [--img-h 64] [--img-w 2048] [--out profiles/rangenet_bench.json]
  python tools/rangenet_bench.py --knn [--knn-params 5,5,1.0,1.0] [--out profiles/rangenet_knn_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402


def med_iqr(v):
    q = np.percentile(v, [25, 50, 75])
    return round(float(q[1]), 4), round(float(q[2] - q[0]), 4)


def knn_bench(a):
    """--knn: lisreg_rangenet_label_knn next to lisreg_rangenet_label, single and batched"""
    import lisreg
    from lisreg import replay
    raws = []
    for sw, _ in replay.synthetic_raw_drive(a.sweeps, a.h, a.w):
        raws.append(np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32))
    cap = max(len(r) for r in raws)
    H, W, NC = a.img_h, a.img_w, a.classes
    hw = H * W
    ctx = lisreg.Context(0)
    P = lisreg.default_rangenet_params(H, W)
    P.n_classes = NC
    K = lisreg.default_rangenet_knn_params()
    knn, search, sigma, cutoff = a.knn_params.split(",")
    K.knn, K.search, K.sigma, K.cutoff = int(knn), int(search), float(sigma), float(cutoff)
    rng = np.random.default_rng(3)
    S = max(a.batch, len(raws))
    ins = [lisreg.DeviceArray(raws[s % len(raws)]) for s in range(S)]
    ns = [len(raws[s % len(raws)]) for s in range(S)]
    tensor = lisreg.DeviceArray(np.zeros((S, 5 * hw), np.float32))
    masks = [lisreg.DeviceArray(np.zeros(hw, np.uint8)) for _ in range(S)]
    pixs = [lisreg.DeviceArray(np.zeros(cap, np.int32)) for _ in range(S)]
    labs = [lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for _ in range(S)]
    labs_knn = [lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for _ in range(S)]
    # logits that look like a network's: smooth in the image (a class per patch of 16 x 64 pixels) plus noise, so neighbours often agree
    patch = rng.integers(0, NC, ((H + 15) // 16, (W + 63) // 64))
    base = np.kron(patch, np.ones((16, 64), np.int64))[:H, :W]
    logits_host = rng.normal(0, 1, (NC, H, W)).astype(np.float32)
    logits_host[base.ravel(), np.arange(hw) // W, np.arange(hw) % W] += 2.0
    d_logits = lisreg.DeviceArray(logits_host)
    lg_ptrs = [d_logits.ptr] * S
    n_valid = ctx.rangenet_project_batch_device([b.ptr for b in ins], ns, P, tensor.ptr, [m.ptr for m in masks], [p.ptr for p in pixs])
    t_plain, t_knn = [], []
    for r in range(a.warmup + a.reps):
        k = r % len(raws)
        t0 = time.perf_counter()
        ctx.rangenet_label_device(ins[k].ptr, ns[k], pixs[k].ptr, masks[k].ptr, d_logits.ptr, P, labs[k].ptr)
        t1 = time.perf_counter()
        ctx.rangenet_label_knn_device(ins[k].ptr, ns[k], pixs[k].ptr, masks[k].ptr, d_logits.ptr, P, K, labs_knn[k].ptr)
        t2 = time.perf_counter()
        if r >= a.warmup:
            t_plain.append(1e3 * (t1 - t0)); t_knn.append(1e3 * (t2 - t1))
    a0 = lisreg.device_to_host(labs[0].ptr, (cap, 4), np.float32)[: ns[0], 3].view(np.uint32)
    a1 = lisreg.device_to_host(labs_knn[0].ptr, (cap, 4), np.float32)[: ns[0], 3].view(np.uint32)
    t_bplain, t_bknn = [], []
    reps_b = max(a.reps // 8, 5)
    B = a.batch
    for r in range(2 + reps_b):
        t0 = time.perf_counter()
        ctx.rangenet_label_batch_device([b.ptr for b in ins[:B]], ns[:B], [p.ptr for p in pixs[:B]], [m.ptr for m in masks[:B]], lg_ptrs[:B], P,
                                        [o.ptr for o in labs[:B]])
        t1 = time.perf_counter()
        ctx.rangenet_label_knn_batch_device([b.ptr for b in ins[:B]], ns[:B], [p.ptr for p in pixs[:B]], [m.ptr for m in masks[:B]], lg_ptrs[:B], P, K,
                                            [o.ptr for o in labs_knn[:B]])
        t2 = time.perf_counter()
        if r >= 2:
            t_bplain.append(1e3 * (t1 - t0) / B); t_bknn.append(1e3 * (t2 - t1) / B)
    ctx.close()
    pm, pi = med_iqr(t_plain)
    km, ki = med_iqr(t_knn)
    bpm, bpi = med_iqr(t_bplain)
    bkm, bki = med_iqr(t_bknn)
    line = dict(workload="rangenet_knn", sweep_shape=[a.h, a.w], image=[H, W], n_classes=NC, points=int(ns[0]), valid_pixels=int(n_valid[0]),
                reps=a.reps, knn_params=[K.knn, K.search, K.sigma, K.cutoff, K.no_vote_label], labels_changed=int((a0 != a1).sum()),
                plain_label_ms=pm, plain_label_iqr_ms=pi, knn_label_ms=km, knn_label_iqr_ms=ki, knn_over_plain=round(km / pm, 3),
                batch_sweeps=B, batch_plain_label_ms_per_sweep=bpm, batch_plain_label_iqr_ms=bpi, batch_knn_label_ms_per_sweep=bkm,
                batch_knn_label_iqr_ms=bki, batch_knn_over_plain=round(bkm / bpm, 3),
                what="plain: rangenet_label_device (2 launches); knn: rangenet_label_knn_device (3 launches); alternating in one run, host clock "
                     "around calls that end in a synchronise, medians and inter-quartile ranges; batch: the two batch calls, per sweep")
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "rangenet_knn_bench.json")
    with open(out, "w") as f:
        f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--img-h", type=int, default=64)
    ap.add_argument("--img-w", type=int, default=2048)
    ap.add_argument("--classes", type=int, default=20)
    ap.add_argument("--sweeps", type=int, default=4, help="different sweeps the calls cycle through")
    ap.add_argument("--no-host", action="store_true", help="skip the numpy stand-in of the host path")
    ap.add_argument("--out", default="")
    ap.add_argument("--knn", action="store_true", help="measure lisreg_rangenet_label_knn next to lisreg_rangenet_label instead")
    ap.add_argument("--knn-params", default="5,5,1.0,1.0", help="knn,search,sigma,cutoff")
    a = ap.parse_args()
    if a.knn:
        return knn_bench(a)
    import lisreg
    from lisreg import replay
    raws = []
    for sw, _ in replay.synthetic_raw_drive(a.sweeps, a.h, a.w):
        raws.append(np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32))
    cap = max(len(r) for r in raws)
    H, W, NC = a.img_h, a.img_w, a.classes
    hw = H * W
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    P = lisreg.default_rangenet_params(H, W)
    P.n_classes = NC
    rng = np.random.default_rng(3)
    logits_host = rng.normal(0, 1, (NC, H, W)).astype(np.float32)
    d_in = [lisreg.DeviceArray(r) for r in raws]
    d_tensor, d_mask = lisreg.DeviceArray(np.zeros(5 * hw, np.float32)), lisreg.DeviceArray(np.zeros(hw, np.uint8))
    d_pix, d_lab = lisreg.DeviceArray(np.zeros(cap, np.int32)), lisreg.DeviceArray(np.zeros((cap, 4), np.float32))
    d_logits = lisreg.DeviceArray(logits_host)
    # pinned landing areas of the three transfers
    pin_cloud = lisreg.PinnedArray(np.zeros((cap, 4), np.float32))
    pin_tensor = lisreg.PinnedArray(np.zeros(5 * hw, np.float32))
    pin_logits = lisreg.PinnedArray(np.zeros(NC * hw, np.float32))

    def copy(dst, src, nbytes, kind):
        if hip.hipMemcpy(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), kind) != 0:
            raise RuntimeError("hipMemcpy failed")

    t_proj, t_label, t_new, t_xfer, n_valid = [], [], [], [], 0
    for r in range(a.warmup + a.reps):
        k = r % len(raws)
        n = len(raws[k])
        t0 = time.perf_counter()
        n_valid = ctx.rangenet_project_device(d_in[k].ptr, n, P, d_tensor.ptr, d_mask.ptr, d_pix.ptr)
        t1 = time.perf_counter()
        ctx.rangenet_label_device(d_in[k].ptr, n, d_pix.ptr, d_mask.ptr, d_logits.ptr, P, d_lab.ptr)
        t2 = time.perf_counter()
        copy(pin_cloud.ptr, d_in[k].ptr, n * 16, 2)                       # the sweep down
        copy(d_tensor.ptr, pin_tensor.ptr, 5 * hw * 4, 1)                 # the input tensor up
        copy(pin_logits.ptr, d_logits.ptr, NC * hw * 4, 2)                # the logits down
        hip.hipDeviceSynchronize()
        t3 = time.perf_counter()
        if r >= a.warmup:
            t_proj.append(1e3 * (t1 - t0)); t_label.append(1e3 * (t2 - t1)); t_new.append(1e3 * (t2 - t0)); t_xfer.append(1e3 * (t3 - t2))
    t_host = []
    if not a.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import rangenet_ref as R
        RP = R.Params(H, W, P.fov_up, P.fov_down, n_classes=NC)
        for r in range(3):
            t0 = time.perf_counter()
            res = R.project_parallel(raws[r % len(raws)], RP)
            R.label_parallel(res["pixel_index"], res["invalid_mask"], logits_host, RP)
            t_host.append(1e3 * (time.perf_counter() - t0))
    # batch against single calls
    S = a.batch
    ins = [d_in[s % len(raws)] for s in range(S)]
    ns = [len(raws[s % len(raws)]) for s in range(S)]
    b_tensor = lisreg.DeviceArray(np.zeros((S, 5 * hw), np.float32))
    b_logits = lisreg.DeviceArray(np.broadcast_to(logits_host.reshape(1, -1), (S, NC * hw)))
    masks = [lisreg.DeviceArray(np.zeros(hw, np.uint8)) for _ in range(S)]
    pixs = [lisreg.DeviceArray(np.zeros(cap, np.int32)) for _ in range(S)]
    labs = [lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for _ in range(S)]
    lg_ptrs = [b_logits.ptr + s * NC * hw * 4 for s in range(S)]
    t_single, t_bproj, t_blabel = [], [], []
    reps_b = max(a.reps // 8, 5)
    for r in range(2 + reps_b):
        t0 = time.perf_counter()
        for s in range(S):
            ctx.rangenet_project_device(ins[s].ptr, ns[s], P, b_tensor.ptr + s * 5 * hw * 4, masks[s].ptr, pixs[s].ptr)
            ctx.rangenet_label_device(ins[s].ptr, ns[s], pixs[s].ptr, masks[s].ptr, lg_ptrs[s], P, labs[s].ptr)
        t1 = time.perf_counter()
        ctx.rangenet_project_batch_device([b.ptr for b in ins], ns, P, b_tensor.ptr, [m.ptr for m in masks], [p.ptr for p in pixs])
        t2 = time.perf_counter()
        ctx.rangenet_label_batch_device([b.ptr for b in ins], ns, [p.ptr for p in pixs], [m.ptr for m in masks], lg_ptrs, P, [o.ptr for o in labs])
        t3 = time.perf_counter()
        if r >= 2:
            t_single.append(1e3 * (t1 - t0) / S); t_bproj.append(1e3 * (t2 - t1) / S); t_blabel.append(1e3 * (t3 - t2) / S)
    ctx.close()
    new_m, new_i = med_iqr(t_new)
    x_m, x_i = med_iqr(t_xfer)
    line = dict(workload="rangenet", sweep_shape=[a.h, a.w], image=[H, W], n_classes=NC, points=int(len(raws[0])), valid_pixels=int(n_valid), reps=a.reps,
                project_ms=med_iqr(t_proj)[0], project_iqr_ms=med_iqr(t_proj)[1], label_ms=med_iqr(t_label)[0], label_iqr_ms=med_iqr(t_label)[1],
                new_path_ms=new_m, new_path_iqr_ms=new_i, transfers_ms=x_m, transfers_iqr_ms=x_i,
                transfer_bytes=[int(len(raws[0])) * 16, 5 * hw * 4, NC * hw * 4],
                margin_ms=round(x_m - new_m, 4), criterion_met=bool(x_m - new_m > max(new_i, x_i)),
                host_stand_in_numpy_ms=round(float(np.median(t_host)), 2) if t_host else None, batch_sweeps=S,
                device_single_ms_per_sweep=med_iqr(t_single)[0], batch_project_ms_per_sweep=med_iqr(t_bproj)[0],
                batch_label_ms_per_sweep=med_iqr(t_blabel)[0],
                what="new: rangenet_project_device + rangenet_label_device, device-resident; transfers: pinned hipMemcpy of the sweep down, the "
                     "tensor up, the logits down; criterion: transfers - new > max(IQRs); host_stand_in: vectorised numpy, not a criterion")
    text = json.dumps(line)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
