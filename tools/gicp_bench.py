"""PCL's GICP (lisreg_gicp_*) on one GPU in the loop-verification shape: prints one JSON line and writes it to --out.

Two pairs, those of tools/fgicp_bench.py.  "bench": target lisreg.synth.make_submap(--target-points, 200 000 by default), corner + surf
clouds concatenated; source the corner + surf clouds of one --h x --w (64 x 1800) sweep; guess = the true pose moved by up to 0.3 m /
2 degrees.  "scene": the pair of tests/test_gicp.py (25 401 x 2 939 points).  All clouds are 16-byte records already in HBM.  Reported
per pair, medians and inter-quartile ranges over --reps calls after a warm-up:

  whole alignment   Context.gicp_align with the default parameters (host clock; the call ends in a synchronise), its outer / inner
                    iteration, evaluation and round counts, the number of moment and total launches and their HIP-event sums
                    ("solve" = the search-and-moments launches, "assoc" = the fixed-order totals, "index" = the source's
                    distributions: Context.set_profiling / timing);
  one round         one Context.gicp_moments call at the guess: the same three intervals;
  host BFGS         the alignment replayed from Python with the two test hooks (gicp_moments for a round, lisreg.gicp_inner for the
                    inner minimisation — the library's own code): the host clock around every gicp_inner call, summed; the replay's
                    final state is checked against the alignment's;
  for scale         Context.fgicp_align with GICP's cut-off on the same slot (host clock).

And on the family's five scenes (the alignment cases of tests/vgicp_ref.py and tests/fgicp_ref.py: guesses 0.3 m / 2 degrees and 0.5 m /
3 degrees away — farther than tests/gicp_ref.py's own cases, see its comment): the pose error against the truth of GICP, FastGICP,
VGICP and NDT, each with its own defaults and the scene's transformation epsilon.

These are timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/gicp_bench.py [--reps 20] [--target-points 200000] [--h 64] [--w 1800] [--out profiles/gicp_bench.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402

# seed, trans, rot_deg, transformation_epsilon: the family's scenes
SCENES = ((1000, 0.3, 2.0, 1.0e-6), (1006, 0.3, 2.0, 1.0e-4), (1001, 0.5, 3.0, 5.0e-4), (1005, 0.5, 3.0, 5.0e-4), (1000, 0.3, 2.0, 0.01))


def med_iqr(v):
    q = np.percentile(v, [25, 50, 75])
    return round(float(q[1]), 4), round(float(q[2] - q[0]), 4)


def records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def pose_error(T, T_true):
    """(translation error in m, rotation error in rad)"""
    D = np.linalg.inv(np.asarray(T_true, np.float64)) @ np.asarray(T, np.float64)
    return float(np.linalg.norm(D[:3, 3])), float(np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0)))


def state_pose(x, G):
    """X(x) G, X = [Rz(yaw) Ry(pitch) Rx(roll) | t] — what the library forms"""
    cr, sr, cp, sp, cy, sy = np.cos(x[3]), np.sin(x[3]), np.cos(x[4]), np.sin(x[4]), np.cos(x[5]), np.sin(x[5])
    X = np.eye(4)
    X[:3, :3] = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                 [-sp, cp * sr, cp * cr]]
    X[:3, 3] = x[:3]
    return X @ G


def scene_clouds(synth, seed, trans, rot):
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=seed, local_radius=12, trans=trans, rot_deg=rot, pose_xy=(32, 31))
    return (records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
            records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
            synth.pose_matrix(c["T_init"]).astype(np.float32), synth.pose_matrix(c["T_true"].astype(np.float64)))


def measure(lisreg, ctx, hip, tgt, src, guess, T_true, reps):
    d_tgt, d_src, d_out = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src), lisreg.DeviceArray(np.zeros_like(src))
    P = lisreg.gicp_default_params()
    Pf = lisreg.fgicp_default_params(max_correspondence_distance=P.max_correspondence_distance)
    stream = C.c_void_p(ctx.stream)
    source = (d_src.ptr, len(src))

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
    info = ctx.fgicp_set_target(0, (d_tgt.ptr, len(tgt)), Pf)
    G = guess.astype(np.float64)
    ctx.set_profiling(True)
    one = lambda: ctx.gicp_moments(0, source, P, G)
    one()                                                              # warm-up: every buffer is made
    t_one, e_one, rec = timed(one, reps)
    align = lambda: ctx.gicp_align(0, source, P, guess, out_ptr=d_out.ptr)
    align()
    t_align, e_align, res = timed(align, reps)
    ctx.set_profiling(False)
    fg = lambda: ctx.fgicp_align(0, source, Pf, guess, out_ptr=d_out.ptr)
    fg()
    t_fg, _, rfg = timed(fg, reps)
    # the alignment replayed with the two hooks: the host clock around the inner minimisations alone
    bb = tgt[np.isfinite(tgt[:, :3]).all(1), :3].astype(np.float64)
    centre = (bb.min(0) + bb.max(0)) / 2.0
    host_ms = []
    for _ in range(max(3, reps // 4)):
        x, total, rounds = np.zeros(6), 0.0, 0
        while True:
            rec = ctx.gicp_moments(0, source, P, state_pose(x, G))
            rounds += 1
            if rec[73] < 4:
                break
            t = time.perf_counter()
            o = lisreg.gicp_inner(rec, centre, x, P)
            total += 1e3 * (time.perf_counter() - t)
            if rounds >= P.max_iters or rounds == res["iters"]:
                x = o["x"]
                break
            x = o["x"]
        host_ms.append(total)
    replay_dT = float(np.abs(state_pose(x, G) - res["T"]).max())
    rounds_ev = max(int(e_align[-1]["solve_launches"]), 1)
    et, er = pose_error(res["T"], T_true)
    etf, erf = pose_error(rfg["T"], T_true)
    et0, er0 = pose_error(G, T_true)
    return dict(target_points=len(tgt), source_points=len(src), grid_dims=info["grid_dims"], target_finite_points=info["n_points"],
                round_call_host_ms=med_iqr(t_one)[0], round_call_host_iqr_ms=med_iqr(t_one)[1],
                round_source_distributions_event_ms=m("index_ms", e_one)[0], round_moments_event_ms=m("solve_ms", e_one)[0],
                round_moments_event_iqr_ms=m("solve_ms", e_one)[1], round_total_event_ms=m("assoc_ms", e_one)[0],
                round_total_event_iqr_ms=m("assoc_ms", e_one)[1], pairs_at_the_guess=int(rec[73]) if rounds == 0 else int(res["n_pairs_last"]),
                align_ms=med_iqr(t_align)[0], align_iqr_ms=med_iqr(t_align)[1], align_converged=bool(res["converged"]),
                align_outer_iters=res["iters"], align_inner_iters=res["inner_iters"], align_evals=res["n_evals"], align_rounds=res["n_rounds"],
                align_inner_exit=res["inner_exit"], align_last_delta=round(res["last_delta"], 4), align_pairs_last=res["n_pairs_last"],
                align_moment_launches=int(e_align[-1]["solve_launches"]), align_total_launches=int(e_align[-1]["assoc_launches"]),
                align_source_distributions_event_ms=m("index_ms", e_align)[0], align_moments_event_ms=m("solve_ms", e_align)[0],
                align_totals_event_ms=m("assoc_ms", e_align)[0],
                align_ms_per_outer_iteration=round(med_iqr(t_align)[0] / max(res["iters"], 1), 4),
                moments_event_ms_per_round=round(m("solve_ms", e_align)[0] / rounds_ev, 4),
                total_event_ms_per_round=round(m("assoc_ms", e_align)[0] / rounds_ev, 4),
                host_bfgs_ms=med_iqr(host_ms)[0], host_bfgs_iqr_ms=med_iqr(host_ms)[1],
                host_bfgs_ms_per_outer_iteration=round(med_iqr(host_ms)[0] / max(res["iters"], 1), 4),
                host_bfgs_us_per_evaluation=round(1e3 * med_iqr(host_ms)[0] / max(res["n_evals"], 1), 3), replay_max_dT=replay_dT,
                align_end_from_truth_mm=round(1e3 * et, 3), align_end_from_truth_mrad=round(1e3 * er, 4),
                fgicp_align_ms=med_iqr(t_fg)[0], fgicp_align_iqr_ms=med_iqr(t_fg)[1], fgicp_iters=rfg["iters"], fgicp_evals=rfg["n_evals"],
                fgicp_end_from_truth_mm=round(1e3 * etf, 3), fgicp_end_from_truth_mrad=round(1e3 * erf, 4),
                guess_from_truth_mm=round(1e3 * et0, 3), guess_from_truth_mrad=round(1e3 * er0, 4))


def accuracy(lisreg, ctx, synth):
    """pose error against the truth of the four verifiers on the family's scenes, [mm, mrad, converged, outer iterations] each"""
    rows = []
    for seed, trans, rot, eps in SCENES:
        tgt, src, guess, T_true = scene_clouds(synth, seed, trans, rot)
        d_tgt, d_src = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src)
        target, source = (d_tgt.ptr, len(tgt)), (d_src.ptr, len(src))
        Pg, Pf = lisreg.gicp_default_params(transformation_epsilon=eps), lisreg.fgicp_default_params(transformation_epsilon=eps)
        Pv, Pn = lisreg.vgicp_default_params(transformation_epsilon=eps), lisreg.ndt_default_params(transformation_epsilon=eps)
        ctx.fgicp_set_target(1, target, Pf)
        ctx.vgicp_set_target(1, target, Pv)
        ctx.ndt_set_target(1, target, Pn)
        runs = dict(gicp=ctx.gicp_align(1, source, Pg, guess), fgicp=ctx.fgicp_align(1, source, Pf, guess),
                    vgicp=ctx.vgicp_align(1, source, Pv, guess), ndt=ctx.ndt_align(1, source, Pn, guess))
        row = dict(seed=seed, trans=trans, rot_deg=rot, transformation_epsilon=eps,
                   guess=[round(1e3 * v, 3) for v in pose_error(guess.astype(np.float64), T_true)])
        for name, r in runs.items():
            row[name] = [round(1e3 * v, 3) for v in pose_error(r["T"], T_true)] + [bool(r["converged"]), int(r["iters"])]
        rows.append(row)
    return rows


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
    scene = measure(lisreg, ctx, hip, *scene_clouds(synth, 1000, 0.3, 2.0), a.reps)
    P = lisreg.gicp_default_params()
    line = dict(workload="gicp", sweep_shape=[a.h, a.w], max_correspondence_distance=P.max_correspondence_distance, k=P.k_correspondences,
                transformation_epsilon=P.transformation_epsilon, max_iters=P.max_iters, max_inner_iters=P.max_inner_iters, reps=a.reps,
                bench=bench, scene=scene, accuracy_mm_mrad_converged_iters=accuracy(lisreg, ctx, synth),
                what="timings only: host clock around calls that end in a synchronise, the library's HIP-event intervals inside them; no counters, nothing tuned")
    text = json.dumps(line)
    print(text)
    out = a.out or os.path.join(ROOT, "profiles", "gicp_bench.json")
    with open(out, "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
