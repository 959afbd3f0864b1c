"""OptimizedICPGN verification of a candidate list (lisreg_icp_gn_match_batch) against the same candidates as a loop of
lisreg_icp_gn_match calls, in one session on one GPU: prints one JSON line and writes it to --out.

The two pairs of tools/gicp_batch_bench.py: "scene" (25 401 x 2 939 points) and "bench" (a 200 000-point submap, the corner + surf
clouds of a 64 x 1800 sweep: 115 200 points).  A candidate list of N (16): the pair's target resident in four map-index slots used in
turn, the pair's source, and N poses spread a few cm / mrad around the pair's guess (seeded).  All clouds are 16-byte records already in
HBM.  The verifier's settings are the reference's `static OptimizedICPGN myICP(30, 10)`: 30 iterations, max_correspond_distance 10.
Per pair, medians and inter-quartile ranges over --reps repetitions after a warm-up, the batch and the loop taking turns:

  batch     one Context.icp_gn_match_batch call: host clock (the call ends in a synchronise);
  loop      N lisreg_icp_gn_match calls over the same candidates: host clock around the loop;
  check     the batch's results equal the loop's in all 80 bytes (asserted).

Timings only: no hardware counters are collected, and nothing was tuned to them.

  python tools/icpgn_batch_bench.py [--candidates 16] [--reps 9] [--out profiles/icpgn_batch_bench.json]"""
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
SLOT0 = 50
MAX_ITERATIONS, MAX_CORRESPOND_DISTANCE = 30, 10.0


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


def measure(lisreg, ctx, hip, tgt, src, guess, n, reps):
    d_tgt, d_src = lisreg.DeviceArray(tgt), lisreg.DeviceArray(src)
    stream = C.c_void_p(ctx.stream)
    source = (d_src.ptr, len(src))

    def sync():
        assert hip.hipStreamSynchronize(stream) == 0
    for s in range(N_SLOTS):
        ctx.map_index_set_device(SLOT0 + s, d_tgt.ptr, len(tgt))
    rng = np.random.default_rng(4000 + n)
    items = [lisreg.IcpGnItem(0, SLOT0 + k % N_SLOTS, (small_motion(rng) @ guess.astype(np.float64)).astype(np.float32)) for k in range(n)]
    L, h = ctx._L, ctx._h
    poses = [np.ascontiguousarray(it.predict_pose, np.float32).ravel() for it in items]
    fp = [p.ctypes.data_as(C.POINTER(C.c_float)) for p in poses]
    single = [lisreg.IcpGnResult() for _ in items]

    def batch():
        return ctx.icp_gn_match_batch([source], items, MAX_ITERATIONS, MAX_CORRESPOND_DISTANCE)

    def loop():
        for it, g, r in zip(items, fp, single):
            ctx._chk(L.lisreg_icp_gn_match(h, it.slot, C.c_void_p(d_src.ptr), len(src), 16, lisreg.FMT_DEVICE, MAX_ITERATIONS,
                                           MAX_CORRESPOND_DISTANCE, g, C.byref(r), None))
        return [bytes(r) for r in single]
    (res_b, info), res_l = batch(), loop()                      # the warm-up, and the check
    assert [r["bytes"] for r in res_b] == res_l, "the batch differs from the loop"
    t_b, t_l = [], []
    for _ in range(reps):                                       # the batch and the loop take turns
        sync()
        t = time.perf_counter()
        batch()
        sync()
        t_b.append(1e3 * (time.perf_counter() - t))
        sync()
        t = time.perf_counter()
        loop()
        sync()
        t_l.append(1e3 * (time.perf_counter() - t))
    out = dict(target_points=len(tgt), source_points=len(src), candidates=n, workgroups_per_single_launch=(len(src) * 4 + 255) // 256,
               steps_applied=[r["steps_applied"] for r in res_b], best=info["best"], fitness_best=float(res_b[info["best"]]["fitness"]),
               n_syncs=info["n_syncs"], batch_ms=med_iqr(t_b)[0], batch_iqr_ms=med_iqr(t_b)[1], loop_ms=med_iqr(t_l)[0],
               loop_iqr_ms=med_iqr(t_l)[1], loop_over_batch=round(med_iqr(t_l)[0] / med_iqr(t_b)[0], 3),
               device_mb=round((192 + 48) * n / 2 ** 20 + (176.0 * ((len(src) * 4 + 255) // 256) + 4.0 * len(src)) * n / 2 ** 20, 3))
    d_tgt.free(); d_src.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", type=int, default=16)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--target-points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--seed", type=int, default=1000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.reps >= 5, "medians of at least five runs"
    import lisreg
    from lisreg import synth
    ctx = lisreg.Context(0)
    hip = lisreg.hip_runtime()
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=1000, local_radius=12, trans=0.3, rot_deg=2.0, pose_xy=(32, 31))
    scene = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])),
                    records(np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])),
                    synth.pose_matrix(c["T_init"]).astype(np.float32), a.candidates, a.reps)
    tc, ts = synth.make_submap(a.target_points)
    sc = synth.make_scan(a.h, a.w, a.seed)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(a.seed + 7919), 0.3, 2.0)
    bench = measure(lisreg, ctx, hip, records(np.concatenate([synth.pcl_xyz(x) for x in (tc, ts)])),
                    records(np.concatenate([synth.pcl_xyz(x) for x in (sc["corner"], sc["surf"])])),
                    synth.pose_matrix(T0).astype(np.float32), a.candidates, a.reps)
    line = dict(workload="icpgn_batch", reps=a.reps, candidates=a.candidates, slots=N_SLOTS, max_iterations=MAX_ITERATIONS,
                max_correspond_distance=MAX_CORRESPOND_DISTANCE, scene=scene, bench=bench,
                what="timings only: host clock around calls that end in a synchronise; medians over the repetitions, the batch and the loop "
                     "taking turns; device-resident sources; no counters, nothing tuned")
    text = json.dumps(line)
    print(text)
    with open(a.out or os.path.join(ROOT, "profiles", "icpgn_batch_bench.json"), "w") as f:
        f.write(text + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
