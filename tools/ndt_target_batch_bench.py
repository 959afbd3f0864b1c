"""The NDT targets of a candidate list (lisreg_ndt_set_target_batch) against the same targets set one by one with
lisreg_ndt_set_target, in one session on one GPU: prints one JSON line, writes it to --out and a summary table to --md.

The two targets of tools/vgicp_target_batch_bench.py: "bench" (a 200 000-point submap) and "scene" (the target of tests/test_ndt.py,
25 401 points).  A candidate list of 16: 16 distinct clouds, each the pair's target under a rigid motion of a few cm / mrad (seeded), as
16-byte records already in HBM.  Per target size, medians, inter-quartile ranges and the extremes over --reps repetitions after a
warm-up, the two ways taking turns (host clock around calls that end in a synchronise):

  targets       one batch call for the 16 targets against 16 single calls; a batch of one against one single call;
  end to end    the 16 targets and then lisreg_ndt_align_batch over 16 candidates (the pair's source against each target from a guess
                of its own), with the targets made either way;
  events        a separate pass with the library's HIP-event intervals (Context.set_profiling / timing: "index" = the compaction and the
                search grids, "solve" = the voxel sort and the Gaussians), added up over the single calls;
  check         every slot the batch sets (lisreg_ndt_get_target with every voxel record, lisreg_ndt_get_voxels) and every result of the verification equal
                the singly set ones', byte for byte (asserted).

Each target size is measured by a child process of its own under its own `timeout`; the second starts only if the first ended well.
`--step trace --pair P` is the workload of a kernel trace: six batch calls of 16 (the first cold), nothing else;
`--trace-stats` adds that trace's kernel split to the report.
Timings only: no figure was promised in advance, no hardware counters are collected, and nothing was tuned to them.

  python tools/ndt_target_batch_bench.py [--reps 21] [--out profiles/ndt_target_batch.json] [--md profiles/ndt_target_batch.md]"""
import argparse
import ctypes as C
import datetime
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lis-slam_amd"))

import numpy as np  # noqa: E402

N_TARGETS = 16
TRACE_CALLS = 6                                    # batch calls of the trace step
STEP_TIMEOUT_S = {"scene": 240, "bench": 420}      # a child runs tens of seconds; the limit ends one that hangs


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


def same_bytes(a, b):
    return a.keys() == b.keys() and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def measure(lisreg, ctx, hip, tgt, src, guess, reps, trace_only=False):
    rng = np.random.default_rng(5000 + len(tgt))
    motions = [np.eye(4)] + [small_motion(rng) for _ in range(N_TARGETS - 1)]
    clouds = [records((tgt[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)) for M in motions]
    devs = [lisreg.DeviceArray(c) for c in clouds]
    d_src = lisreg.DeviceArray(src)
    source = (d_src.ptr, len(src))
    P = lisreg.ndt_default_params()
    stream = C.c_void_p(ctx.stream)
    jobs_a = [(k, (devs[k].ptr, len(clouds[k]))) for k in range(N_TARGETS)]                    # the singles' slots
    jobs_b = [(N_TARGETS + k, (devs[k].ptr, len(clouds[k]))) for k in range(N_TARGETS)]        # the batch's
    guesses = [(small_motion(rng) @ motions[k] @ guess.astype(np.float64)).astype(np.float32) for k in range(N_TARGETS)]

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0

    def singles(jobs=jobs_a):
        for s, cloud in jobs:
            ctx.ndt_set_target(s, cloud, P)

    def batch(jobs=jobs_b):
        res = ctx.ndt_set_target_batch(jobs, P)
        assert all(r["status"] == 0 for r in res)

    def verify(first_slot):
        return ctx.ndt_align_batch([source], [lisreg.NdtItem(0, first_slot + k, guesses[k]) for k in range(N_TARGETS)], P)

    def clock(fn):
        sync()
        t = time.perf_counter()
        r = fn()
        sync()
        return 1e3 * (time.perf_counter() - t), r
    if trace_only:
        for _ in range(TRACE_CALLS):
            batch()
        sync()
        return {}
    # the warm-up, and the check
    singles(); batch(); singles(jobs_a[:1]); batch(jobs_b[:1])
    for k in range(N_TARGETS):
        assert same_bytes(ctx.ndt_get_target(k), ctx.ndt_get_target(N_TARGETS + k)), "a slot of the batch differs from the single call's"
        assert same_bytes(ctx.ndt_get_voxels(k), ctx.ndt_get_voxels(N_TARGETS + k)), "the voxels of a slot of the batch differ from the single call's"
    (ra, fa, ia), (rb, fb, ib) = verify(0), verify(N_TARGETS)
    assert fa.tobytes() == fb.tobytes() and ia == ib and all(same_bytes(x, y) for x, y in zip(ra, rb)), "a verification over the batch's slots differs"
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
    ev = {k: [] for k in ("batch_index", "batch_solve", "single_index", "single_solve")}
    for _ in range(5):
        batch()
        tm = ctx.timing()
        ev["batch_index"].append(tm["index_ms"]); ev["batch_solve"].append(tm["solve_ms"])
        ti = ts = 0.0
        for s, cloud in jobs_a:
            ctx.ndt_set_target(s, cloud, P)
            tm = ctx.timing()
            ti += tm["index_ms"]; ts += tm["solve_ms"]
        ev["single_index"].append(ti); ev["single_solve"].append(ts)
    ctx.set_profiling(False)
    batch()
    info = ctx.ndt_get_target(N_TARGETS)
    out = dict(target_points=len(tgt), source_points=len(src), targets=N_TARGETS, voxels=int(info["n_voxels"]), valid_voxels=int(info["n_valid"]),
               converged=int(sum(bool(r["converged"]) for r in rb)),
               enqueues=ctx.ndt_target_batch_counts()[0], synchronisations=ctx.ndt_target_batch_counts()[1])
    for k, v in t.items():
        out[k] = stats(v)
    m = lambda k: out[k]["median_ms"]
    out["single16_over_batch16"] = round(m("single16") / m("batch16"), 3)
    out["single1_over_batch1"] = round(m("single1") / m("batch1"), 3)
    out["e2e_single_over_e2e_batch"] = round(m("e2e_single") / m("e2e_batch"), 3)
    for k, v in ev.items():
        out[k + "_event_ms"] = round(float(np.median(v)), 4)
    # the two bars of DESIGN.md §7v, with the session's margin (the sum of the two inter-quartile ranges)
    spread16 = out["batch16"]["iqr_ms"] + out["single16"]["iqr_ms"]
    spread1 = out["batch1"]["iqr_ms"] + out["single1"]["iqr_ms"]
    out["batch16_faster_by_more_than_the_margin"] = bool(m("single16") - m("batch16") > spread16)
    out["batch1_not_slower_by_more_than_the_margin"] = bool(m("batch1") - m("single1") <= spread1)
    for d in devs + [d_src]:
        d.free()
    return out


def pair_inputs(pair, a):
    from lisreg import synth
    if pair == "scene":
        c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=1000, local_radius=12, trans=0.3, rot_deg=2.0, pose_xy=(32, 31))
        return (records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
                synth.pose_matrix(c["T_init"]).astype(np.float32))
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    return (records(np.concatenate([synth.pcl_xyz(x) for x in (tc, ts)])),
            records(np.concatenate([synth.pcl_xyz(x) for x in (sc["corner"], sc["surf"])])), synth.pose_matrix(T0).astype(np.float32))


def child(a):
    import lisreg
    ctx = lisreg.Context(0)
    tgt, src, guess = pair_inputs(a.pair, a)
    out = measure(lisreg, ctx, lisreg.hip_runtime(), tgt, src, guess, a.reps, trace_only=a.step == "trace")
    ctx.close()
    if a.child_out:
        with open(a.child_out, "w") as f:
            json.dump(out, f)


def table(line):
    f = lambda s: f"{s['median_ms']} (IQR {s['iqr_ms']}, {s['min_ms']} .. {s['max_ms']})"
    rows = ["| target | 16 single calls, ms | one batch of 16, ms | singles / batch | one single call, ms | a batch of one, ms | single / batch of one | "
            "16 targets + ndt_align_batch(16): singles, ms | the same with the batch, ms | ratio | ndt_align_batch(16) alone, ms | "
            "\"index\" + \"solve\" events: 16 singles, ms | the batch, ms |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for pair in ("scene", "bench"):
        r = line[pair]
        rows.append(f"| {pair} ({r['target_points']} points, {r['voxels']} voxels, {r['valid_voxels']} valid) | {f(r['single16'])} | {f(r['batch16'])} | {r['single16_over_batch16']} | "
                    f"{f(r['single1'])} | {f(r['batch1'])} | {r['single1_over_batch1']} | {f(r['e2e_single'])} | {f(r['e2e_batch'])} | "
                    f"{r['e2e_single_over_e2e_batch']} | {f(r['verify'])} | {r['single_index_event_ms']} + {r['single_solve_event_ms']} | "
                    f"{r['batch_index_event_ms']} + {r['batch_solve_event_ms']} |")
    return "\n".join(rows)


def kernel_trace(path):
    """the kernels of a `rocprofv3 --kernel-trace --stats -- python tools/ndt_target_batch_bench.py --step trace --pair bench` run (its
    kernel_stats.csv): name, calls and total time, per batch call (the step makes TRACE_CALLS of them and nothing else)"""
    import csv
    import re
    rows = []
    for r in csv.DictReader(open(path)):
        name, calls, total = r["Name"], int(r["Calls"]), float(r["TotalDurationNs"])
        short = re.search(r"(k_\w+(?:<[^>]*>)?|__amd_\w+)", name)
        rows.append(dict(kernel=short.group(1) if short else name[:96], launches_per_call=round(calls / TRACE_CALLS, 2), us_per_call=round(total / TRACE_CALLS / 1e3, 1)))
    rows.sort(key=lambda r: -r["us_per_call"])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--md", default=None)
    ap.add_argument("--pair", choices=("scene", "bench"), default=None, help="measure this target size in this process (what the tool's children run)")
    ap.add_argument("--step", choices=("measure", "trace"), default="measure")
    ap.add_argument("--child-out", default=None)
    ap.add_argument("--trace-stats", default=None, help="kernel_stats.csv of a kernel trace of `--step trace --pair bench`: its split joins the report")
    a = ap.parse_args()
    assert a.reps >= 20, "medians of at least 20 repetitions"
    if a.pair:
        return child(a)
    line = dict(workload="ndt_target_batch", date=datetime.date.today().isoformat(), reps=a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        for pair in ("scene", "bench"):                            # every GPU step a process of its own under its own time limit
            path = os.path.join(tmp, pair + ".json")
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S[pair]), sys.executable, os.path.abspath(__file__), "--pair", pair, "--reps", str(a.reps),
                   "--target-points", str(a.target_points), "--h", str(a.h), "--w", str(a.w), "--seed", str(a.seed), "--child-out", path]
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit(f"ndt_target_batch_bench: the {pair} step ended with status {rc}; nothing more is started")
            line[pair] = json.load(open(path))
    line["what"] = ("timings only, one session on one GPU: host clock around calls that end in a synchronise, the ways taking turns; medians, "
                    "inter-quartile ranges and extremes; no counters, nothing tuned")
    scene, bench = line["scene"], line["bench"]
    if a.trace_stats:
        line["kernel_trace_bench"] = kernel_trace(a.trace_stats)
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "ndt_target_batch.json"), "w") as f:
        f.write(text + "\n")
    verdict = lambda r: (f"batch of 16 faster than 16 singles by more than the margin: {'yes' if r['batch16_faster_by_more_than_the_margin'] else 'NO'}; "
                         f"batch of one not slower than one single by more than the margin: {'yes' if r['batch1_not_slower_by_more_than_the_margin'] else 'NO'}")
    with open(a.md or os.path.join(ROOT, "profiles", "ndt_target_batch.md"), "w") as f:
        f.write("# The NDT targets of a candidate list: one batch call against the single calls it replaces\n\n"
                f"`python tools/ndt_target_batch_bench.py --reps {a.reps}` on one MI355X ({line['date']}, one session on one box): 16 distinct "
                "targets (the pair's target under 16 small rigid motions) as device records; host clock around calls that end in a synchronise, "
                f"medians over {a.reps} repetitions in which the ways take turns, with the inter-quartile range and the extremes in brackets.  "
                "The end-to-end columns set the 16 targets and then verify 16 candidates with `lisreg_ndt_align_batch` (the pair's source "
                "against each target from its own guess).  The event columns are the library's \"index\" (compaction, search grids) "
                "and \"solve\" (voxel sort and Gaussians) intervals from a pass of their own, added up over the single calls.  "
                "Every slot of the batch equals the singly set one byte for byte, and so do the verifications (asserted by the tool).  The batch "
                f"call issued {bench['enqueues']} enqueues and {bench['synchronisations']} synchronisations, whatever the number of targets.  "
                "The margin is the sum of the inter-quartile ranges of the two ways compared.  Timings only: nothing was tuned to them.\n\n"
                + table(line) + f"\n\nscene: {verdict(scene)}.\n\nbench: {verdict(bench)}.\n")
        if a.trace_stats:
            kt = line["kernel_trace_bench"]
            all_us = sum(r["us_per_call"] for r in kt)
            f.write("\n## Where the batch's time goes (bench, 16 targets)\n\nA kernel trace of `--step trace --pair bench` (a run of its own: "
                    f"{TRACE_CALLS} batch calls and nothing else, the first of them cold), per call; {round(all_us, 1)} us of kernels in all.\n\n"
                    "| kernel | launches per call | us per call | share |\n|---|---|---|---|\n"
                    + "\n".join(f"| `{r['kernel']}` | {r['launches_per_call']} | {r['us_per_call']} | {round(100 * r['us_per_call'] / all_us, 1)} % |" for r in kt) + "\n")


if __name__ == "__main__":
    main()
