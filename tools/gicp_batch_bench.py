"""PCL's GICP verification of a candidate list (lisreg_gicp_align_batch) against the same candidates as a loop of
lisreg_gicp_align calls, in one session on one GPU: prints one JSON line, writes it to --out and a summary table to --md.

The two pairs of tools/gicp_bench.py: "bench" (a 200 000-point submap, the corner + surf clouds of a 64 x 1800 sweep) and "scene" (the
pair of tests/test_gicp.py, 25 401 x 2 939 points).  A candidate list of N: the pair's target resident in four FastGICP slots used in
turn, the pair's source, and N guesses spread a few cm / mrad around the pair's guess (seeded).  All clouds are 16-byte records already
in HBM.  Per pair and N, medians and inter-quartile ranges over --reps repetitions after a warm-up, the batch and the loop taking turns:

  batch     one Context.gicp_align_batch call with the fitness pass: host clock (the call ends in a synchronise); the same call without
            the fitness pass: host clock and the library's HIP-event intervals (Context.set_profiling / timing: "solve" = the moments
            launch of every round, "assoc" = its totals, "index" = the source's distributions), also divided by the rounds;
  host      what is left of the call without the fitness pass when its event intervals are taken off: the uploads, the launches, the
            copies, the synchronisations and the items' BFGS runs between a synchronisation and the next upload, per round; and, for
            scale, the inner minimisations of candidate 0 replayed through lisreg.gicp_inner (the library's own code), per outer
            iteration, times the evaluations the batch answered (one BFGS run each) divided by the rounds;
  loop      N Context.gicp_align calls over the same candidates: host clock around the loop, the same event intervals added up.  The
            loop computes no fitness score (a caller would add a lisreg_nearest call per candidate), so it is the cheaper job;
  check     the batch's results equal the loop's, bit for bit (asserted).

Timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/gicp_batch_bench.py [--candidates 1,4,16,64] [--reps 9] [--out profiles/gicp_batch_bench.json] [--md profiles/gicp_batch.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402

N_SLOTS = 4


def med_iqr(v):
    q = np.percentile(v, [25, 50, 75])
    return round(float(q[1]), 4), round(float(q[2] - q[0]), 4)


def records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def small_motion(rng):
    """a rigid motion of a few mrad and a few cm"""
    w, t = rng.uniform(-3e-3, 3e-3, 3), rng.uniform(-0.03, 0.03, 3)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    M = np.eye(4)
    M[:3, :3] = np.eye(3) + K + 0.5 * K @ K
    M[:3, 3] = t
    return M


def state_pose(x, G):
    """X(x) G, X = [Rz(yaw) Ry(pitch) Rx(roll) | t] — what the library forms"""
    cr, sr, cp, sp, cy, sy = np.cos(x[3]), np.sin(x[3]), np.cos(x[4]), np.sin(x[4]), np.cos(x[5]), np.sin(x[5])
    X = np.eye(4)
    X[:3, :3] = [[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr], [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                 [-sp, cp * sr, cp * cr]]
    X[:3, 3] = x[:3]
    return X @ G


def bfgs_replay_ms(lisreg, ctx, tgt, source, P, item, res):
    """the host clock around the lisreg.gicp_inner calls of one candidate's alignment, replayed with the two test hooks: (ms in all,
    outer iterations)"""
    bb = tgt[np.isfinite(tgt[:, :3]).all(1), :3].astype(np.float64)
    centre = (bb.min(0) + bb.max(0)) / 2.0
    G = item.guess.reshape(4, 4).astype(np.float64)
    x, total, iters = np.zeros(6), 0.0, 0
    while iters < res["iters"]:
        rec = ctx.gicp_moments(item.slot, source, P, state_pose(x, G))
        if rec[73] < 4:
            break
        t = time.perf_counter()
        x = lisreg.gicp_inner(rec, centre, x, P)["x"]
        total += 1e3 * (time.perf_counter() - t)
        iters += 1
    return total, iters


def measure(lisreg, ctx, hip, tgt, src, guess, candidates, reps):
    d_tgt, d_src = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src)
    P = lisreg.gicp_default_params()
    Pf = lisreg.fgicp_default_params(max_correspondence_distance=P.max_correspondence_distance)
    stream = C.c_void_p(ctx.stream)
    source = (d_src.ptr, len(src))

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0
    for s in range(N_SLOTS):
        ctx.fgicp_set_target(s, (d_tgt.ptr, len(tgt)), Pf)
    keys = ("assoc_ms", "assoc_launches", "solve_ms", "solve_launches", "index_ms")
    out = dict(target_points=len(tgt), source_points=len(src), by_candidates={})
    for n in candidates:
        rng = np.random.default_rng(4000 + n)
        items = [lisreg.GicpItem(0, k % N_SLOTS, (small_motion(rng) @ guess.astype(np.float64)).astype(np.float32)) for k in range(n)]

        def batch(want_fitness=True):
            return ctx.gicp_align_batch([source], items, P, want_fitness=want_fitness)

        def loop():
            tot = dict.fromkeys(keys, 0.0)
            res = []
            for it in items:
                res.append(ctx.gicp_align(it.slot, source, P, it.guess.reshape(4, 4)))
                t = ctx.timing()
                for k in keys:
                    tot[k] += t[k]
            return res, tot
        ctx.set_profiling(True)
        (res_b, fit, info), (res_l, _) = batch(), loop()                  # the warm-up, and the check
        batch(False)
        for a, b in zip(res_b, res_l):
            assert a["T"].tobytes() == b["T"].tobytes() and a["error"] == b["error"] and a["last_delta"] == b["last_delta"] and \
                all(a[k] == b[k] for k in ("converged", "iters", "inner_iters", "n_evals", "n_rounds", "inner_exit", "n_pairs_last")), \
                "the batch differs from the loop"
        t_b, t_nf, e_nf, t_l, e_l = [], [], [], [], []
        for _ in range(reps):                                             # the batch, the batch without the fitness pass and the loop take turns
            sync()
            t = time.perf_counter()
            batch()
            sync()
            t_b.append(1e3 * (time.perf_counter() - t))
            sync()
            t = time.perf_counter()
            batch(False)
            sync()
            t_nf.append(1e3 * (time.perf_counter() - t))
            e_nf.append(ctx.timing())
            sync()
            t = time.perf_counter()
            _, tot = loop()
            sync()
            t_l.append(1e3 * (time.perf_counter() - t))
            e_l.append(tot)
        ctx.set_profiling(False)
        replay_ms, replay_iters = bfgs_replay_ms(lisreg, ctx, tgt, source, P, items[0], res_b[0])
        m = lambda key, evs: med_iqr([e[key] for e in evs])[0]
        rounds = max(info["n_rounds"], 1)
        item_rounds = [r["n_rounds"] for r in res_b]
        outer = int(sum(r["iters"] for r in res_b))
        host_other = [t - e["assoc_ms"] - e["solve_ms"] - e["index_ms"] for t, e in zip(t_nf, e_nf)]
        bfgs_us = 1e3 * replay_ms / max(replay_iters, 1)
        out["by_candidates"][str(n)] = dict(
            candidates=n, converged=int(sum(bool(r["converged"]) for r in res_b)), item_rounds_total=int(sum(item_rounds)),
            item_rounds_min=int(min(item_rounds)), outer_iterations_total=outer,
            rounds=info["n_rounds"], best=info["best"], fitness_best=float(fit[info["best"]]) if info["best"] >= 0 else None,
            batch_ms=med_iqr(t_b)[0], batch_iqr_ms=med_iqr(t_b)[1], batch_without_fitness_ms=med_iqr(t_nf)[0],
            batch_without_fitness_iqr_ms=med_iqr(t_nf)[1],
            loop_ms=med_iqr(t_l)[0], loop_iqr_ms=med_iqr(t_l)[1], loop_over_batch=round(med_iqr(t_l)[0] / med_iqr(t_b)[0], 3),
            loop_over_batch_without_fitness=round(med_iqr(t_l)[0] / med_iqr(t_nf)[0], 3),
            batch_moments_event_ms=m("solve_ms", e_nf), batch_moment_launches=int(e_nf[-1]["solve_launches"]),
            batch_totals_event_ms=m("assoc_ms", e_nf), batch_total_launches=int(e_nf[-1]["assoc_launches"]),
            batch_distributions_event_ms=m("index_ms", e_nf),
            moments_event_ms_per_round=round(m("solve_ms", e_nf) / rounds, 4), totals_event_ms_per_round=round(m("assoc_ms", e_nf) / rounds, 4),
            host_ms_per_round=round(med_iqr(host_other)[0] / rounds, 4),
            bfgs_replay_us_per_outer_iteration=round(bfgs_us, 2), bfgs_estimate_ms_per_round=round(1e-3 * bfgs_us * outer / rounds, 4),
            loop_moments_event_ms=m("solve_ms", e_l), loop_moment_launches=int(e_l[-1]["solve_launches"]),
            loop_totals_event_ms=m("assoc_ms", e_l), loop_distributions_event_ms=m("index_ms", e_l),
            partial_records_mb=round(592.0 * n * ((len(src) + 63) // 64) / 2 ** 20, 3))
    return out


def table(line):
    rows = ["| pair | candidates | loop of single calls, ms | batch, ms (without fitness) | loop / batch (without fitness) | rounds | per round: moments / "
            "totals, ms (events) | per round: host, ms (BFGS estimate) | batch distributions, ms | loop: moments / totals / distributions, ms (events) |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for pair in ("scene", "bench"):
        for n, r in line[pair]["by_candidates"].items():
            rows.append(f"| {pair} ({line[pair]['target_points']} x {line[pair]['source_points']}) | {n} | {r['loop_ms']} (IQR {r['loop_iqr_ms']}) | "
                        f"{r['batch_ms']} (IQR {r['batch_iqr_ms']}; {r['batch_without_fitness_ms']}) | {r['loop_over_batch']} "
                        f"({r['loop_over_batch_without_fitness']}) | {r['rounds']} | {r['moments_event_ms_per_round']} / {r['totals_event_ms_per_round']} | "
                        f"{r['host_ms_per_round']} ({r['bfgs_estimate_ms_per_round']}) | {r['batch_distributions_event_ms']} | "
                        f"{r['loop_moments_event_ms']} / {r['loop_totals_event_ms']} / {r['loop_distributions_event_ms']} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    cand = [int(v) for v in a.candidates.split(",")]
    import lisreg
    from lisreg import synth
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=1000, local_radius=12, trans=0.3, rot_deg=2.0, pose_xy=(32, 31))
    scene = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                    records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
                    synth.pose_matrix(c["T_init"]).astype(np.float32), cand, a.reps)
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    bench = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(x) for x in (tc, ts)])),
                    records(np.concatenate([synth.pcl_xyz(x) for x in (sc["corner"], sc["surf"])])),
                    synth.pose_matrix(T0).astype(np.float32), cand, a.reps)
    line = dict(workload="gicp_batch", reps=a.reps, candidates=cand, slots=N_SLOTS, scene=scene, bench=bench,
                what="timings only: host clock around calls that end in a synchronise, the library's HIP-event intervals inside them; the loop of "
                     "single calls computes no fitness score; no counters, nothing tuned")
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "gicp_batch_bench.json"), "w") as f:
        f.write(text + "\n")
    with open(a.md or os.path.join(ROOT, "profiles", "gicp_batch.md"), "w") as f:
        f.write("# PCL's GICP verification of a candidate list: the batch against the loop of single calls\n\n"
                f"`python tools/gicp_batch_bench.py --candidates {a.candidates} --reps {a.reps}` on one MI355X, medians over {a.reps} repetitions in "
                "which the batch and the loop take turns (host clock around calls that end in a synchronise; the event columns are the library's "
                "HIP-event intervals of the call without the fitness pass, divided by its rounds).  The loop computes no fitness score, the batch "
                "does; its time without the fitness pass is in brackets.  \"host\" is what is left of that call per round when the event "
                "intervals are taken off: uploads, launches, copies, synchronisations and the items' BFGS runs; the BFGS estimate beside it is "
                "the inner minimisation of candidate 0 replayed through `lisreg_gicp_inner`, times the outer iterations of all items, per round — an upper bound, since every replayed call pays Python's foreign-function call as well. "
                "The results of the batch and of the loop are equal bit for bit (asserted by the tool).  Timings only: nothing was tuned to them.\n\n"
                + table(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
