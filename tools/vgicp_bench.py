"""VGICP registration (lisreg_vgicp_*) on one GPU in the loop-verification shape: prints one JSON line and writes it to --out.

Target: lisreg.synth.make_submap(--target-points, 200 000 by default), corner + surf clouds concatenated, resolution 1.0.  Source: the
corner + surf clouds of one --h x --w (64 x 1800) sweep, both as 16-byte records already in HBM; guess = the true pose moved by up to
0.3 m / 2 degrees.  Reported, medians and inter-quartile ranges over --reps calls after a warm-up:

  target build      Context.vgicp_set_target: host clock (the call ends in a synchronise), and the library's HIP-event intervals on the
                    context's stream (Context.set_profiling / timing) split into the distributions (search grid, k-nearest search,
                    covariances) and the voxels (voxel sort and statistics, with the wait for the voxel count between them);
  source            the distributions of the source, the same interval of a Context.vgicp_linearize call (every call with a source makes
                    its distributions anew);
  one linearisation the two launches of one evaluation with and without H, HIP events, from the same call; and the host clock of the call;
  whole alignment   Context.vgicp_align with the default parameters (host clock), with its iteration, evaluation and rejection counts and
                    the HIP-event sums of its distributions and of its linearisations;
  for scale         Context.ndt_align and Context.icp_align_device (loop-closure parameters) on the same pair (host clock; their targets
                    are built once, outside the timed calls, like the VGICP target).

These are timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/vgicp_bench.py [--reps 20] [--target-points 200000] [--h 64] [--w 1800] [--out profiles/vgicp_bench.json]"""
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--neighbors", type=int, choices=(1, 7, 27), default=1,
                    help="the voxel neighbourhood of the linearisations and alignments (DIRECT1 / 7 / 27, DESIGN.md section 7w)")
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
    P = lisreg.vgicp_default_params() if a.neighbors == 1 else lisreg.vgicp_default_params(neighbor_search=a.neighbors)
    stream = C.c_void_p(ctx.stream)

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0

    def timed(fn, reps):
        """host clock and the library's event intervals of every call"""
        host, ev = [], []
        for _ in range(reps):
            sync()
            t = time.perf_counter()
            r = fn()
            sync()
            host.append(1e3 * (time.perf_counter() - t))
            ev.append(ctx.timing())
        return host, ev, r
    build = lambda: ctx.vgicp_set_target(0, (d_tgt.ptr, len(tgt)), P)
    info = build()                                                     # warm-up: every buffer is made
    ctx.set_profiling(True)
    t_build, e_build, info = timed(build, a.reps)
    G = guess.astype(np.float64)
    lin = {}
    for hess in (True, False):
        call = lambda: ctx.vgicp_linearize(0, (d_src.ptr, len(src)), P, G, hess)
        call()
        h_ms, e_ms, (_, pairs) = timed(call, a.reps)
        lin[hess] = (med_iqr([e["assoc_ms"] for e in e_ms]), med_iqr(h_ms), med_iqr([e["index_ms"] for e in e_ms]), pairs)
    align = lambda: ctx.vgicp_align(0, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    align()
    t_align, e_align, res = timed(align, a.reps)
    ctx.set_profiling(False)
    Pn = lisreg.ndt_default_params()
    ctx.ndt_set_target(0, (d_tgt.ptr, len(tgt)), Pn)
    ndt = lambda: ctx.ndt_align(0, (d_src.ptr, len(src)), Pn, guess, out_ptr=d_out.ptr)
    ndt()
    t_ndt, _, rndt = timed(ndt, a.reps)
    ctx.map_index_set_device(0, d_tgt.ptr, len(tgt))
    pi = lisreg.icp_default_params(0)
    icp = lambda: ctx.icp_align_device(0, d_src.ptr, len(src), pi, guess, out_ptr=d_out.ptr)
    icp()
    t_icp, _, ricp = timed(icp, a.reps)
    Tt = synth.pose_matrix(sc["T_true"])

    def off(T):
        return round(float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - Tt[:3, 3])), 4)
    m = lambda key, evs: med_iqr([e[key] for e in evs])
    line = dict(workload="vgicp", target_points=len(tgt), source_points=len(src), sweep_shape=[a.h, a.w], resolution=P.resolution,
                k=P.k_correspondences, reps=a.reps, dims=info["dims"], n_voxels=info["n_voxels"],
                target_build_ms=med_iqr(t_build)[0], target_build_iqr_ms=med_iqr(t_build)[1],
                target_distributions_event_ms=m("index_ms", e_build)[0], target_distributions_event_iqr_ms=m("index_ms", e_build)[1],
                target_voxels_event_ms=m("solve_ms", e_build)[0], target_voxels_event_iqr_ms=m("solve_ms", e_build)[1],
                source_distributions_event_ms=lin[True][2][0], source_distributions_event_iqr_ms=lin[True][2][1],
                linearize_hessian_event_ms=lin[True][0][0], linearize_hessian_event_iqr_ms=lin[True][0][1], linearize_hessian_call_host_ms=lin[True][1][0],
                linearize_plain_event_ms=lin[False][0][0], linearize_plain_event_iqr_ms=lin[False][0][1], linearize_plain_call_host_ms=lin[False][1][0],
                pairs_per_eval=int(lin[True][3]),
                align_ms=med_iqr(t_align)[0], align_iqr_ms=med_iqr(t_align)[1], align_iters=res["iters"], align_evals=res["n_evals"],
                align_rejected=res["n_rejected"], align_converged=bool(res["converged"]), align_end_from_truth_m=off(res["T"]),
                align_distributions_event_ms=m("index_ms", e_align)[0], align_linearisations_event_ms=m("assoc_ms", e_align)[0],
                ndt_align_ms=med_iqr(t_ndt)[0], ndt_align_iqr_ms=med_iqr(t_ndt)[1], ndt_iters=rndt["iters"], ndt_evals=rndt["n_evals"],
                ndt_end_from_truth_m=off(rndt["T"]),
                icp_align_ms=med_iqr(t_icp)[0], icp_align_iqr_ms=med_iqr(t_icp)[1], icp_iters=ricp["iters"], icp_end_from_truth_m=off(ricp["T"]),
                guess_from_truth_m=off(guess),
                what="timings only: host clock around calls that end in a synchronise, the library's HIP-event intervals inside them; no counters, nothing tuned")
    if a.neighbors != 1:                                               # (the default's line is the one it always was)
        line["neighbors"] = a.neighbors
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "vgicp_bench.json")
    with open(out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
