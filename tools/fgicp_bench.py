"""FastGICP registration (lisreg_fgicp_*) on one GPU in the loop-verification shape: prints one JSON line and writes it to --out.

Two pairs.  "bench": target lisreg.synth.make_submap(--target-points, 200 000 by default), corner + surf clouds concatenated; source the
corner + surf clouds of one --h x --w (64 x 1800) sweep; guess = the true pose moved by up to 0.3 m / 2 degrees (the pair of
tools/vgicp_bench.py).  "scene": the pair of tests/test_fgicp.py (25 401 x 2 939 points).  All clouds are 16-byte records already in HBM.
Reported per pair, medians and inter-quartile ranges over --reps calls after a warm-up:

  target build      Context.fgicp_set_target: host clock (the call ends in a synchronise) and the library's HIP-event interval of the
                    distributions (search grid, k-nearest search, covariances; Context.set_profiling / timing);
  one search        the k_fgicp_pairs launch of a Context.fgicp_linearize call, HIP events ("solve" of lisreg_get_timing);
  one sum           the k_fgicp_sums + total launches of the same call with and without H, HIP events ("assoc");
  source            the distributions of the source, the same call's "index" interval (every call with a source makes them anew);
  whole alignment   Context.fgicp_align with the default parameters (host clock), its iteration, evaluation and rejection counts, the
                    number of search and sum launches and their HIP-event sums;
  for scale         Context.vgicp_align, Context.ndt_align and Context.icp_align_device (loop-closure parameters) on the same pair (host
                    clock; their targets are built once, outside the timed calls).

These are timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/fgicp_bench.py [--reps 20] [--target-points 200000] [--h 64] [--w 1800] [--out profiles/fgicp_bench.json]"""
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


def records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def measure(lisreg, ctx, hip, tgt, src, guess, T_true, reps):
    d_tgt, d_src, d_out = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src), lisreg.DeviceArray(np.zeros_like(src))
    P = lisreg.fgicp_default_params()
    stream = C.c_void_p(ctx.stream)

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0

    def timed(fn, n):
        """host clock and the library's event intervals of every call"""
        host, ev = [], []
        for _ in range(n):
            sync()
            t = time.perf_counter()
            r = fn()
            sync()
            host.append(1e3 * (time.perf_counter() - t))
            ev.append(ctx.timing())
        return host, ev, r
    m = lambda key, evs: med_iqr([e[key] for e in evs])
    build = lambda: ctx.fgicp_set_target(0, (d_tgt.ptr, len(tgt)), P)
    info = build()                                                     # warm-up: every buffer is made
    ctx.set_profiling(True)
    t_build, e_build, info = timed(build, reps)
    G = guess.astype(np.float64)
    lin = {}
    for hess in (True, False):
        call = lambda: ctx.fgicp_linearize(0, (d_src.ptr, len(src)), P, G, hess)
        call()
        h_ms, e_ms, (_, pairs) = timed(call, reps)
        lin[hess] = (m("assoc_ms", e_ms), m("solve_ms", e_ms), m("index_ms", e_ms), med_iqr(h_ms), pairs)
    align = lambda: ctx.fgicp_align(0, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    align()
    t_align, e_align, res = timed(align, reps)
    ctx.set_profiling(False)
    Pv = lisreg.vgicp_default_params()
    ctx.vgicp_set_target(0, (d_tgt.ptr, len(tgt)), Pv)
    vg = lambda: ctx.vgicp_align(0, (d_src.ptr, len(src)), Pv, guess, out_ptr=d_out.ptr)
    vg()
    t_vg, _, rvg = timed(vg, reps)
    Pn = lisreg.ndt_default_params()
    ctx.ndt_set_target(0, (d_tgt.ptr, len(tgt)), Pn)
    ndt = lambda: ctx.ndt_align(0, (d_src.ptr, len(src)), Pn, guess, out_ptr=d_out.ptr)
    ndt()
    t_ndt, _, rndt = timed(ndt, reps)
    ctx.map_index_set_device(0, d_tgt.ptr, len(tgt))
    pi = lisreg.icp_default_params(0)
    icp = lambda: ctx.icp_align_device(0, d_src.ptr, len(src), pi, guess, out_ptr=d_out.ptr)
    icp()
    t_icp, _, ricp = timed(icp, reps)

    def off(T):
        return round(float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - T_true[:3, 3])), 4)
    return dict(target_points=len(tgt), source_points=len(src), grid_dims=info["grid_dims"], target_finite_points=info["n_points"],
                target_build_ms=med_iqr(t_build)[0], target_build_iqr_ms=med_iqr(t_build)[1],
                target_distributions_event_ms=m("index_ms", e_build)[0], target_distributions_event_iqr_ms=m("index_ms", e_build)[1],
                source_distributions_event_ms=lin[True][2][0], source_distributions_event_iqr_ms=lin[True][2][1],
                search_event_ms=lin[True][1][0], search_event_iqr_ms=lin[True][1][1],
                sums_hessian_event_ms=lin[True][0][0], sums_hessian_event_iqr_ms=lin[True][0][1],
                sums_plain_event_ms=lin[False][0][0], sums_plain_event_iqr_ms=lin[False][0][1],
                linearize_call_host_ms=lin[True][3][0], pairs_per_search=int(lin[True][4]),
                align_ms=med_iqr(t_align)[0], align_iqr_ms=med_iqr(t_align)[1], align_iters=res["iters"], align_evals=res["n_evals"],
                align_rejected=res["n_rejected"], align_converged=bool(res["converged"]), align_pairs_last=res["n_pairs_last"],
                align_end_from_truth_m=off(res["T"]),
                align_distributions_event_ms=m("index_ms", e_align)[0],
                align_search_launches=int(e_align[-1]["solve_launches"]), align_searches_event_ms=m("solve_ms", e_align)[0],
                align_sum_launches=int(e_align[-1]["assoc_launches"]), align_sums_event_ms=m("assoc_ms", e_align)[0],
                vgicp_align_ms=med_iqr(t_vg)[0], vgicp_align_iqr_ms=med_iqr(t_vg)[1], vgicp_iters=rvg["iters"], vgicp_evals=rvg["n_evals"],
                vgicp_end_from_truth_m=off(rvg["T"]),
                ndt_align_ms=med_iqr(t_ndt)[0], ndt_align_iqr_ms=med_iqr(t_ndt)[1], ndt_iters=rndt["iters"], ndt_evals=rndt["n_evals"],
                ndt_end_from_truth_m=off(rndt["T"]),
                icp_align_ms=med_iqr(t_icp)[0], icp_align_iqr_ms=med_iqr(t_icp)[1], icp_iters=ricp["iters"], icp_end_from_truth_m=off(ricp["T"]),
                guess_from_truth_m=off(guess))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import lisreg
    from lisreg import synth
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    bench = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c) for c in (tc, ts)])),
                    records(np.concatenate([synth.pcl_xyz(c) for c in (sc["corner"], sc["surf"])])),
                    synth.pose_matrix(T0).astype(np.float32), synth.pose_matrix(sc["T_true"]), a.reps)
    # the pair of tests/test_fgicp.py (tests/vgicp_ref.py: scene())
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=1000, local_radius=12, trans=0.3, rot_deg=2.0, pose_xy=(32, 31))
    scene = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                    records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
                    synth.pose_matrix(c["T_init"]).astype(np.float32), synth.pose_matrix(c["T_true"].astype(np.float64)), a.reps)
    P = lisreg.fgicp_default_params()
    line = dict(workload="fgicp", sweep_shape=[a.h, a.w], max_correspondence_distance=P.max_correspondence_distance, k=P.k_correspondences,
                reps=a.reps, lane_order="input order of the source's finite points", bench=bench, scene=scene,
                what="timings only: host clock around calls that end in a synchronise, the library's HIP-event intervals inside them; no counters, nothing tuned")
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "fgicp_bench.json")
    with open(out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
