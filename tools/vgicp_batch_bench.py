"""VGICP verification of a candidate list (lisreg_vgicp_align_batch) against the same candidates as a loop of
lisreg_vgicp_align calls, in one session on one GPU: prints one JSON line, writes it to --out and a summary table to --md.

The two pairs of tools/vgicp_bench.py: "bench" (a 200 000-point submap, the corner + surf clouds of a 64 x 1800 sweep) and "scene" (the
pair of tests/test_vgicp.py, 25 401 x 2 939 points).  A candidate list of N: the pair's target resident in four VGICP slots used in
turn, the pair's source, and N guesses spread a few cm / mrad around the pair's guess (seeded).  All clouds are 16-byte records already
in HBM.  Per pair and N, medians and inter-quartile ranges over --reps repetitions after a warm-up:

  batch     one Context.vgicp_align_batch call with the fitness pass, and one without it: host clock (the call ends in a synchronise)
            and the library's HIP-event intervals (Context.set_profiling / timing: the rounds' linearisation and total launches, the
            fitness search, the distributions);
  loop      N Context.vgicp_align calls over the same candidates: host clock around the loop, the same event intervals added up.  The
            loop computes no fitness score (a caller would add a lisreg_nearest call per candidate), so it is the cheaper job;
  check     the batch's results equal the loop's, bit for bit (asserted).

Timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/vgicp_batch_bench.py [--candidates 16,64] [--reps 20] [--out profiles/vgicp_batch_bench.json] [--md profiles/vgicp_batch.md]"""
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


def measure(lisreg, ctx, hip, tgt, src, guess, candidates, reps, neighbors=1):
    d_tgt, d_src = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src)
    P = lisreg.vgicp_default_params() if neighbors == 1 else lisreg.vgicp_default_params(neighbor_search=neighbors)
    stream = C.c_void_p(ctx.stream)
    source = (d_src.ptr, len(src))

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0
    for s in range(N_SLOTS):
        ctx.vgicp_set_target(s, (d_tgt.ptr, len(tgt)), P)
    keys = ("assoc_ms", "assoc_launches", "solve_ms", "solve_launches", "index_ms")
    out = dict(target_points=len(tgt), source_points=len(src), by_candidates={})
    for n in candidates:
        rng = np.random.default_rng(4000 + n)
        items = [lisreg.VgicpItem(0, k % N_SLOTS, (small_motion(rng) @ guess.astype(np.float64)).astype(np.float32)) for k in range(n)]

        def batch():
            return ctx.vgicp_align_batch([source], items, P)

        def loop():
            tot = dict.fromkeys(keys, 0.0)
            res = []
            for it in items:
                res.append(ctx.vgicp_align(it.slot, source, P, it.guess.reshape(4, 4)))
                t = ctx.timing()
                for k in keys:
                    tot[k] += t[k]
            return res, tot
        ctx.set_profiling(True)
        (res_b, fit, info), (res_l, _) = batch(), loop()                  # the warm-up, and the check
        for a, b in zip(res_b, res_l):
            assert a["T"].tobytes() == b["T"].tobytes() and a["error"] == b["error"] and a["lam"] == b["lam"] and \
                (a["converged"], a["iters"], a["n_evals"], a["n_rejected"], a["n_pairs_last"]) == \
                (b["converged"], b["iters"], b["n_evals"], b["n_rejected"], b["n_pairs_last"]), "the batch differs from the loop"
        t_b, e_b, t_l, e_l = [], [], [], []
        for _ in range(reps):
            sync()
            t = time.perf_counter()
            batch()
            sync()
            t_b.append(1e3 * (time.perf_counter() - t))
            e_b.append(ctx.timing())
            sync()
            t = time.perf_counter()
            _, tot = loop()
            sync()
            t_l.append(1e3 * (time.perf_counter() - t))
            e_l.append(tot)
        # the fitness pass alone: the batch without it
        t_nf = []
        for _ in range(reps):
            sync()
            t = time.perf_counter()
            ctx.vgicp_align_batch([source], items, P, want_fitness=False)
            sync()
            t_nf.append(1e3 * (time.perf_counter() - t))
        ctx.set_profiling(False)
        m = lambda key, evs: med_iqr([e[key] for e in evs])[0]
        evals = [r["n_evals"] for r in res_b]
        out["by_candidates"][str(n)] = dict(
            candidates=n, converged=int(sum(bool(r["converged"]) for r in res_b)), evaluations_total=int(sum(evals)), evaluations_max=int(max(evals)),
            rounds=info["n_rounds"], best=info["best"], fitness_best=float(fit[info["best"]]) if info["best"] >= 0 else None,
            batch_ms=med_iqr(t_b)[0], batch_iqr_ms=med_iqr(t_b)[1], batch_without_fitness_ms=med_iqr(t_nf)[0],
            loop_ms=med_iqr(t_l)[0], loop_iqr_ms=med_iqr(t_l)[1], loop_over_batch=round(med_iqr(t_l)[0] / med_iqr(t_b)[0], 3),
            batch_linearisations_event_ms=m("assoc_ms", e_b), batch_rounds_timed=int(e_b[-1]["assoc_launches"]),
            batch_fitness_event_ms=m("solve_ms", e_b), batch_fitness_launches=int(e_b[-1]["solve_launches"]),
            batch_distributions_event_ms=m("index_ms", e_b),
            loop_linearisations_event_ms=m("assoc_ms", e_l), loop_linearisation_launches=int(e_l[-1]["assoc_launches"]),
            loop_distributions_event_ms=m("index_ms", e_l),
            source_storage_mb=round(64.0 * len(src) / 2 ** 20, 2))
    return out


def table(line):
    rows = ["| pair | candidates | loop of single calls, ms | batch, ms (without fitness) | loop / batch | rounds "
            "| batch: linearisations / fitness search / distributions, ms (events) | loop: linearisations / distributions, ms (events) |",
            "|---|---|---|---|---|---|---|---|"]
    for pair in ("scene", "bench"):
        for n, r in line[pair]["by_candidates"].items():
            rows.append(f"| {pair} ({line[pair]['target_points']} x {line[pair]['source_points']}) | {n} | {r['loop_ms']} (IQR {r['loop_iqr_ms']}) | "
                        f"{r['batch_ms']} (IQR {r['batch_iqr_ms']}; {r['batch_without_fitness_ms']}) | {r['loop_over_batch']} | {r['rounds']} | "
                        f"{r['batch_linearisations_event_ms']} / {r['batch_fitness_event_ms']} / {r['batch_distributions_event_ms']} | "
                        f"{r['loop_linearisations_event_ms']} / {r['loop_distributions_event_ms']} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="16,64")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--neighbors", type=int, choices=(1, 7, 27), default=1,
                    help="the voxel neighbourhood of the batch and of the single calls (DIRECT1 / 7 / 27, DESIGN.md section 7w)")
    a = ap.parse_args()
    cand = [int(v) for v in a.candidates.split(",")]
    import lisreg
    from lisreg import synth
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=1000, local_radius=12, trans=0.3, rot_deg=2.0, pose_xy=(32, 31))
    scene = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                    records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
                    synth.pose_matrix(c["T_init"]).astype(np.float32), cand, a.reps, a.neighbors)
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    bench = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(x) for x in (tc, ts)])),
                    records(np.concatenate([synth.pcl_xyz(x) for x in (sc["corner"], sc["surf"])])),
                    synth.pose_matrix(T0).astype(np.float32), cand, a.reps, a.neighbors)
    line = dict(workload="vgicp_batch", reps=a.reps, candidates=cand, slots=N_SLOTS, scene=scene, bench=bench,
                what="timings only: host clock around calls that end in a synchronise, the library's HIP-event intervals inside them; the loop of "
                     "single calls computes no fitness score; no counters, nothing tuned")
    nb = "" if a.neighbors == 1 else f" --neighbors {a.neighbors}"          # (the default's output is the one it always was)
    if nb:
        line["neighbors"] = a.neighbors
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "vgicp_batch_bench.json"), "w") as f:
        f.write(text + "\n")
    with open(a.md or os.path.join(ROOT, "profiles", "vgicp_batch.md"), "w") as f:
        f.write("# VGICP verification of a candidate list: the batch against the loop of single calls\n\n"
                f"`python tools/vgicp_batch_bench.py --candidates {a.candidates} --reps {a.reps}{nb}` on one MI355X, medians over {a.reps} repetitions "
                "(host clock around calls that end in a synchronise; the event columns are the library's HIP-event intervals added up over a "
                "call).  The loop computes no fitness score, the batch does; its time without the fitness pass is in brackets.  The results of "
                "the two are equal bit for bit (asserted by the tool).  Timings only: nothing was promised in advance or tuned to them.\n\n"
                + table(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
