"""NDT registration (lisreg_ndt_*) on one GPU in the loop-verification shape: prints one JSON line and writes it to --out.

Target: lisreg.synth.make_submap(--target-points, 200 000 by default), corner + surf clouds concatenated, resolution 1.0.  Source: the
corner + surf clouds of one --h x --w (64 x 1800) sweep, both as 16-byte records already in HBM; guess = the true pose moved by up to
0.3 m / 2 degrees.  Reported, medians and inter-quartile ranges over --reps calls after a warm-up:

  target build      Context.ndt_set_target (host clock; the call ends in a synchronise);
  one evaluation    Context.ndt_derivatives with and without the Hessian at the guess: HIP events on the context's stream around the
                    call (two launches, one 29-double read-back), and the host clock next to them;
  whole alignment   Context.ndt_align with the default parameters (host clock), with its iteration and evaluation counts;
  ICP, for scale    Context.icp_align_device with the loop-closure parameters on the same pair (host clock; its map index is built once,
                    outside the timed call, like the NDT target).

These are timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/ndt_bench.py [--reps 30] [--target-points 200000] [--h 64] [--w 1800] [--out profiles/ndt_bench.json]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lisreg
    from lisreg import synth
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)

    def records(*clouds):
        xyz = np.concatenate([synth.pcl_xyz(c) for c in clouds])
        rec = np.zeros((len(xyz), 4), np.float32)
        rec[:, :3] = xyz
        return rec
    tgt, src = records(tc, ts), records(sc["corner"], sc["surf"])
    guess = synth.pose_matrix(T0).astype(np.float32)
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    d_tgt, d_src, d_out = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src), lisreg.DeviceArray(np.zeros_like(src))
    P = lisreg.ndt_default_params()
    stream = C.c_void_p(ctx.stream)

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0

    def host_ms(fn, reps):
        out = []
        for _ in range(reps):
            sync()
            t = time.perf_counter()
            r = fn()
            sync()
            out.append(1e3 * (time.perf_counter() - t))
        return out, r
    ev = [C.c_void_p(), C.c_void_p()]
    for e in ev:
        assert hip.hipEventCreate(C.byref(e)) == 0

    def event_ms(fn, reps):
        out = []
        for _ in range(reps):
            sync()
            assert hip.hipEventRecord(ev[0], stream) == 0
            fn()
            assert hip.hipEventRecord(ev[1], stream) == 0
            assert hip.hipEventSynchronize(ev[1]) == 0
            ms = C.c_float()
            assert hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1]) == 0
            out.append(ms.value)
        return out
    build = lambda: ctx.ndt_set_target(0, (d_tgt.ptr, len(tgt)), P)
    info = build()                                                     # warm-up: every buffer is made
    t_build, info = host_ms(build, a.reps)
    G = guess.astype(np.float64)                                       # the guess in the library's chart (include/lisreg.h)
    p0 = np.array([G[0, 3], G[1, 3], G[2, 3], np.arctan2(-G[1, 2], G[2, 2]), np.arcsin(G[0, 2]), np.arctan2(-G[0, 1], G[0, 0])])
    evals = {}
    for hess in (True, False):
        call = lambda: ctx.ndt_derivatives(0, (d_src.ptr, len(src)), P, p0, hess)
        call()
        e_ms = event_ms(call, a.reps)
        h_ms, (_, pairs) = host_ms(call, a.reps)
        evals[hess] = (med_iqr(e_ms), med_iqr(h_ms), pairs)
    align = lambda: ctx.ndt_align(0, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    align()
    t_align, res = host_ms(align, a.reps)
    ctx.map_index_set_device(0, d_tgt.ptr, len(tgt))
    pi = lisreg.icp_default_params(0)
    icp = lambda: ctx.icp_align_device(0, d_src.ptr, len(src), pi, guess, out_ptr=d_out.ptr)
    icp()
    t_icp, ricp = host_ms(icp, a.reps)
    Tt = synth.pose_matrix(sc["T_true"])

    def off(T):
        return round(float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - Tt[:3, 3])), 4)
    line = dict(workload="ndt", target_points=len(tgt), source_points=len(src), sweep_shape=[a.h, a.w], resolution=P.resolution, reps=a.reps,
                dims=info["dims"], n_voxels=info["n_voxels"], n_valid=info["n_valid"],
                target_build_ms=med_iqr(t_build)[0], target_build_iqr_ms=med_iqr(t_build)[1],
                eval_hessian_event_ms=evals[True][0][0], eval_hessian_event_iqr_ms=evals[True][0][1], eval_hessian_host_ms=evals[True][1][0],
                eval_plain_event_ms=evals[False][0][0], eval_plain_event_iqr_ms=evals[False][0][1], eval_plain_host_ms=evals[False][1][0],
                pairs_per_eval=int(evals[True][2]),
                align_ms=med_iqr(t_align)[0], align_iqr_ms=med_iqr(t_align)[1], align_iters=res["iters"], align_evals=res["n_evals"],
                align_converged=bool(res["converged"]), align_end_from_truth_m=off(res["T"]),
                icp_align_ms=med_iqr(t_icp)[0], icp_align_iqr_ms=med_iqr(t_icp)[1], icp_iters=ricp["iters"], icp_end_from_truth_m=off(ricp["T"]),
                guess_from_truth_m=off(guess),
                what="timings only: host clock around calls that end in a synchronise, HIP events around one evaluation; no counters, nothing tuned")
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "ndt_bench.json")
    with open(out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
