"""The FastGICP targets of a candidate list (lisreg_fgicp_set_target_batch) against the same targets set one by one with
lisreg_fgicp_set_target, in one session on one GPU: prints one JSON line, writes it to --out and a summary table to --md.

The two targets of tools/fgicp_bench.py: "bench" (a 200 000-point submap) and "scene" (the target of tests/test_fgicp.py, 25 401
points).  A candidate list of 16: 16 distinct clouds, each the pair's target under a rigid motion of a few cm / mrad (seeded), as 16-byte
records already in HBM.  Per target size, medians, inter-quartile ranges and the extremes over --reps repetitions after a warm-up, the
two ways taking turns (host clock around calls that end in a synchronise):

  targets       one batch call for the 16 targets against 16 single calls; a batch of one against one single call;
  end to end    the 16 targets and then lisreg_gicp_align_batch over 16 candidates (the pair's source against each target from a guess
                of its own), with the targets made either way;
  events        a separate pass with the library's HIP-event intervals (Context.set_profiling / timing: "index" = the compaction, the sort
                and the distributions of a call), added up over the single calls;
  check         every slot the batch sets equals the singly set one, bit for bit (asserted).

Timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/fgicp_target_batch_bench.py [--reps 21] [--out profiles/fgicp_target_batch.json] [--md profiles/fgicp_target_batch.md]"""
import argparse
import ctypes as C
import datetime
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402

N_TARGETS = 16


def stats(v):
    q = np.percentile(v, [25, 50, 75])
    return dict(median_ms=round(float(q[1]), 4), iqr_ms=round(float(q[2] - q[0]), 4), min_ms=round(float(min(v)), 4), max_ms=round(float(max(v)), 4))


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


def measure(lisreg, ctx, hip, tgt, src, guess, reps):
    rng = np.random.default_rng(5000 + len(tgt))
    motions = [np.eye(4)] + [small_motion(rng) for _ in range(N_TARGETS - 1)]
    clouds = [records((tgt[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)) for M in motions]
    devs = [lisreg.DeviceArray(c) for c in clouds]
    d_src = lisreg.DeviceArray(src)
    source = (d_src.ptr, len(src))
    P = lisreg.gicp_default_params()
    Pf = lisreg.fgicp_default_params(max_correspondence_distance=P.max_correspondence_distance)
    stream = C.c_void_p(ctx.stream)
    jobs_a = [(k, (devs[k].ptr, len(clouds[k]))) for k in range(N_TARGETS)]                    # the singles' slots
    jobs_b = [(N_TARGETS + k, (devs[k].ptr, len(clouds[k]))) for k in range(N_TARGETS)]        # the batch's
    guesses = [(small_motion(rng) @ motions[k] @ guess.astype(np.float64)).astype(np.float32) for k in range(N_TARGETS)]

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0

    def singles(jobs=jobs_a):
        for s, cloud in jobs:
            ctx.fgicp_set_target(s, cloud, Pf)

    def batch(jobs=jobs_b):
        res = ctx.fgicp_set_target_batch(jobs, Pf)
        assert all(r["status"] == 0 for r in res)

    def verify(first_slot):
        return ctx.gicp_align_batch([source], [lisreg.GicpItem(0, first_slot + k, guesses[k]) for k in range(N_TARGETS)], P)

    def clock(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return 1e3 * (time.perf_counter() - t), r
    # the warm-up, and the check
    singles(); batch(); singles(jobs_a[:1]); batch(jobs_b[:1])
    for k in range(N_TARGETS):
        a, b = ctx.fgicp_get_target(k), ctx.fgicp_get_target(N_TARGETS + k)
        assert all(np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes() for key in a), "a slot of the batch differs from the single call's"
    (ra, fa, ia), (rb, fb, ib) = verify(0), verify(N_TARGETS)
    assert fa.tobytes() == fb.tobytes() and ia == ib and all(x["T"].tobytes() == y["T"].tobytes() for x, y in zip(ra, rb))
    t = {k: [] for k in ("batch16", "single16", "batch1", "single1", "e2e_batch", "e2e_single", "verify")}
    for _ in range(reps):                                                                       # the ways take turns
        t["batch16"].append(clock(batch)[0])
        t["single16"].append(clock(singles)[0])
        t["batch1"].append(clock(lambda: batch(jobs_b[:1]))[0])
        t["single1"].append(clock(lambda: singles(jobs_a[:1]))[0])
        t["e2e_batch"].append(clock(lambda: (batch(), verify(N_TARGETS)))[0])
        t["e2e_single"].append(clock(lambda: (singles(), verify(0)))[0])
        t["verify"].append(clock(lambda: verify(0))[0])
    # the event intervals, in a pass of their own
    ctx.set_profiling(True)
    ev_b, ev_s = [], []
    for _ in range(5):
        batch()
        ev_b.append(ctx.timing()["index_ms"])
        tot = 0.0
        for s, cloud in jobs_a:
            ctx.fgicp_set_target(s, cloud, Pf)
            tot += ctx.timing()["index_ms"]
        ev_s.append(tot)
    ctx.set_profiling(False)
    out = dict(target_points=len(tgt), source_points=len(src), targets=N_TARGETS, converged=int(sum(bool(r["converged"]) for r in rb)),
               enqueues=ctx.fgicp_target_batch_counts()[0], synchronisations=ctx.fgicp_target_batch_counts()[1])
    for k, v in t.items():
        out[k] = stats(v)
    m = lambda k: out[k]["median_ms"]
    out["single16_over_batch16"] = round(m("single16") / m("batch16"), 3)
    out["single1_over_batch1"] = round(m("single1") / m("batch1"), 3)
    out["e2e_single_over_e2e_batch"] = round(m("e2e_single") / m("e2e_batch"), 3)
    out["batch16_index_event_ms"] = round(float(np.median(ev_b)), 4)
    out["single16_index_event_ms"] = round(float(np.median(ev_s)), 4)
    for d in devs + [d_src]:
        d.free()
    return out


def table(line):
    f = lambda s: f"{s['median_ms']} (IQR {s['iqr_ms']}, {s['min_ms']} .. {s['max_ms']})"
    rows = ["| target | 16 single calls, ms | one batch of 16, ms | singles / batch | one single call, ms | a batch of one, ms | single / batch of one | "
            "16 targets + gicp_align_batch(16): singles, ms | the same with the batch, ms | ratio | gicp_align_batch(16) alone, ms | "
            "\"index\" events: 16 singles / the batch, ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for pair in ("scene", "bench"):
        r = line[pair]
        rows.append(f"| {pair} ({r['target_points']} points) | {f(r['single16'])} | {f(r['batch16'])} | {r['single16_over_batch16']} | {f(r['single1'])} | "
                    f"{f(r['batch1'])} | {r['single1_over_batch1']} | {f(r['e2e_single'])} | {f(r['e2e_batch'])} | {r['e2e_single_over_e2e_batch']} | "
                    f"{f(r['verify'])} | {r['single16_index_event_ms']} / {r['batch16_index_event_ms']} |")
    return "\n".join(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 repetitions"
    import lisreg
    from lisreg import synth
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=1000, local_radius=12, trans=0.3, rot_deg=2.0, pose_xy=(32, 31))
    scene = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                    records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
                    synth.pose_matrix(c["T_init"]).astype(np.float32), a.reps)
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    bench = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(x) for x in (tc, ts)])),
                    records(np.concatenate([synth.pcl_xyz(x) for x in (sc["corner"], sc["surf"])])),
                    synth.pose_matrix(T0).astype(np.float32), a.reps)
    line = dict(workload="fgicp_target_batch", date=datetime.date.today().isoformat(), reps=a.reps, scene=scene, bench=bench,
                what="timings only, one session on one GPU: host clock around calls that end in a synchronise, the ways taking turns; medians, "
                     "inter-quartile ranges and extremes; no counters, nothing tuned")
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "fgicp_target_batch.json"), "w") as f:
        f.write(text + "\n")
    with open(a.md or os.path.join(ROOT, "profiles", "fgicp_target_batch.md"), "w") as f:
        f.write("# The FastGICP targets of a candidate list: one batch call against the single calls it replaces\n\n"
                f"`python tools/fgicp_target_batch_bench.py --reps {a.reps}` on one MI355X ({line['date']}, one session on one box): 16 distinct "
                "targets (the pair's target under 16 small rigid motions) as device records; host clock around calls that end in a synchronise, "
                f"medians over {a.reps} repetitions in which the ways take turns, with the inter-quartile range and the extremes in brackets.  "
                "The end-to-end columns set the 16 targets and then verify 16 candidates with `lisreg_gicp_align_batch` (the pair's source "
                "against each target from its own guess).  The event column is the library's \"index\" interval (compaction, sort, "
                "distributions) from a pass of its own, added up over the single calls.  Every slot of the batch equals the singly set one bit "
                f"for bit, and so do the verifications (asserted by the tool).  The batch call issued {bench['enqueues']} enqueues and "
                f"{bench['synchronisations']} synchronisations, whatever the number of targets.  Timings only: nothing was tuned to them.\n\n"
                + table(line) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
