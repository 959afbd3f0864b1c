"""NDT verification of a candidate list (lisreg_ndt_align_batch) against the same candidates as a loop of
lisreg_ndt_align calls, in one session on one GPU: prints one JSON line, writes it to --out and a summary table to --md.

Two pairs: "scene" (the pair of tests/test_ndt.py, 25 401 x 735 points) and "bench" (a 200 000-point submap, the corner + surf clouds of
a 64 x 1800 sweep, the pair of tools/vgicp_batch_bench.py).  A candidate list of N: the pair's target resident in four NDT slots used in
turn, the pair's source, and N guesses spread a few cm / mrad around the pair's guess (seeded).  All clouds are 16-byte records already
in HBM.  Per pair and N, medians and inter-quartile ranges over --reps alternating repetitions (batch, loop, batch, loop, ...) after a
warm-up:

  batch     one Context.ndt_align_batch call with the fitness pass, and one without it: host clock (the call ends in a synchronise) and
            the library's HIP-event intervals (Context.set_profiling / timing: the rounds' evaluation and total launches, the fitness
            search);
  loop      N Context.ndt_align calls over the same candidates: host clock around the loop.  The loop computes no fitness score (a
            caller would add a lisreg_nearest call per candidate), so it is the cheaper job;
  check     the batch's results equal the loop's, bit for bit (asserted).

Launch counts are read off the code, not measured: a single call makes two launches and one synchronisation per evaluation (the
evaluation, its total); a batch makes at most three launches, two small uploads and one synchronisation per round (the evaluations
with and without the Hessian, the totals), one count launch per staged source and two launches for the fitness pass.

Timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/ndt_batch_bench.py [--candidates 1,4,16] [--reps 9] [--out profiles/ndt_batch_bench.json] [--md profiles/ndt_batch_table.md]"""
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


def measure(lisreg, ctx, hip, tgt, src, guess, candidates, reps):
    d_tgt, d_src = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src)
    P = lisreg.ndt_default_params()
    stream = C.c_void_p(ctx.stream)
    source = (d_src.ptr, len(src))

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0
    t_set = []
    for k in range(N_SLOTS + 5):                                          # the targets; the last five calls are timed
        sync()
        t = time.perf_counter()
        ctx.ndt_set_target(k % N_SLOTS, (d_tgt.ptr, len(tgt)), P)
        t_set.append(1e3 * (time.perf_counter() - t))
    out = dict(target_points=len(tgt), source_points=len(src), set_target_ms=med_iqr(t_set[-5:])[0], set_target_iqr_ms=med_iqr(t_set[-5:])[1],
               by_candidates={})
    for n in candidates:
        rng = np.random.default_rng(4000 + n)
        items = [lisreg.NdtItem(0, k % N_SLOTS, (small_motion(rng) @ guess.astype(np.float64)).astype(np.float32)) for k in range(n)]

        def batch():
            return ctx.ndt_align_batch([source], items, P)

        def loop():
            return [ctx.ndt_align(it.slot, source, P, it.guess.reshape(4, 4)) for it in items]
        ctx.set_profiling(True)
        (res_b, fit, info), res_l = batch(), loop()                       # the warm-up, and the check
        for a, b in zip(res_b, res_l):
            assert a["p"].tobytes() == b["p"].tobytes() and a["T"].tobytes() == b["T"].tobytes() and a["score"] == b["score"] and \
                (a["converged"], a["iters"], a["n_evals"], a["n_pairs_last"]) == (b["converged"], b["iters"], b["n_evals"], b["n_pairs_last"]), \
                "the batch differs from the loop"
        t_b, e_b, t_l, t_nf = [], [], [], []
        for _ in range(reps):
            sync()
            t = time.perf_counter()
            batch()
            sync()
            t_b.append(1e3 * (time.perf_counter() - t))
            e_b.append(ctx.timing())
            sync()
            t = time.perf_counter()
            loop()
            sync()
            t_l.append(1e3 * (time.perf_counter() - t))
            sync()
            t = time.perf_counter()
            ctx.ndt_align_batch([source], items, P, want_fitness=False)     # the fitness pass alone: the batch without it
            sync()
            t_nf.append(1e3 * (time.perf_counter() - t))
        ctx.set_profiling(False)
        m = lambda key, evs: med_iqr([e[key] for e in evs])[0]
        evals = [r["n_evals"] for r in res_b]
        rounds = info["n_rounds"]
        out["by_candidates"][str(n)] = dict(
            candidates=n, converged=int(sum(bool(r["converged"]) for r in res_b)), evaluations_total=int(sum(evals)), evaluations_max=int(max(evals)),
            rounds=rounds, best=info["best"], fitness_best=float(fit[info["best"]]) if info["best"] >= 0 else None,
            batch_ms=med_iqr(t_b)[0], batch_iqr_ms=med_iqr(t_b)[1], batch_without_fitness_ms=med_iqr(t_nf)[0],
            loop_ms=med_iqr(t_l)[0], loop_iqr_ms=med_iqr(t_l)[1], loop_over_batch=round(med_iqr(t_l)[0] / med_iqr(t_b)[0], 3),
            batch_ms_per_round=round(med_iqr(t_nf)[0] / rounds, 4), loop_ms_per_evaluation=round(med_iqr(t_l)[0] / sum(evals), 4),
            batch_evaluations_event_ms=m("assoc_ms", e_b), batch_rounds_timed=int(e_b[-1]["assoc_launches"]),
            batch_fitness_event_ms=m("solve_ms", e_b),
            launches_loop_from_code=2 * int(sum(evals)), launches_batch_at_most_from_code=3 * rounds + 3,
            source_storage_mb=round(16.0 * len(src) / 2 ** 20, 2))
    return out


def table(line):
    rows = ["| pair | candidates | loop of single calls, ms | batch, ms (without fitness) | loop / batch | rounds | evaluations "
            "| launches, loop / batch (from the code) | loop ms per evaluation / batch ms per round | batch: evaluations / fitness search, ms (events) |",
            "|---|---|---|---|---|---|---|---|---|---|"]
    for pair in ("scene", "bench"):
        for n, r in line[pair]["by_candidates"].items():
            rows.append(f"| {pair} ({line[pair]['target_points']} x {line[pair]['source_points']}) | {n} | {r['loop_ms']} (IQR {r['loop_iqr_ms']}) | "
                        f"{r['batch_ms']} (IQR {r['batch_iqr_ms']}; {r['batch_without_fitness_ms']}) | {r['loop_over_batch']} | {r['rounds']} | "
                        f"{r['evaluations_total']} | {r['launches_loop_from_code']} / <= {r['launches_batch_at_most_from_code']} | "
                        f"{r['loop_ms_per_evaluation']} / {r['batch_ms_per_round']} | {r['batch_evaluations_event_ms']} / {r['batch_fitness_event_ms']} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="1,4,16")
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
    src = np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])
    scene = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                    records(np.ascontiguousarray(src[:: max(len(src) // 600, 1)])), synth.pose_matrix(c["T_init"]).astype(np.float32), cand, a.reps)
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    bench = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(x) for x in (tc, ts)])),
                    records(np.concatenate([synth.pcl_xyz(x) for x in (sc["corner"], sc["surf"])])),
                    synth.pose_matrix(T0).astype(np.float32), cand, a.reps)
    line = dict(workload="ndt_batch", reps=a.reps, candidates=cand, slots=N_SLOTS, scene=scene, bench=bench,
                what="timings only: host clock around calls that end in a synchronise, the library's HIP-event intervals inside the batch; "
                     "alternating repetitions; the loop of single calls computes no fitness score; launch counts read off the code; no counters, "
                     "nothing tuned")
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "ndt_batch_bench.json"), "w") as f:
        f.write(text + "\n")
    with open(a.md or os.path.join(ROOT, "profiles", "ndt_batch_table.md"), "w") as f:
        f.write("# NDT verification of a candidate list: the batch against the loop of single calls\n\n"
                f"`python tools/ndt_batch_bench.py --candidates {a.candidates} --reps {a.reps}` on one MI355X, medians over {a.reps} alternating "
                "repetitions (host clock around calls that end in a synchronise; the event columns are the library's HIP-event intervals added up "
                "over a call).  The loop computes no fitness score, the batch does; its time without the fitness pass is in brackets.  The results "
                "of the two are equal bit for bit (asserted by the tool).  Timings only: nothing was promised in advance or tuned to them.\n\n"
                + table(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
