"""FEPSC loop-closure candidate detection (lisreg_loopdet_detect) on one GPU: prints one JSON line.

Scene: the synth.py room (labels 9 / 13 / 18 reach the EPSC, SEPSC and projection counters).  The history of a database alternates
between two places A and B 30 m apart (stored with the gate switched off, so building it costs no candidates); a query key frame
at B after a frame at A then gates every A frame (query gate inflation 1e-4, so the B frames 30 m away never pass): G candidates, each a yaw search + 2-D ICP + the whole query frame (~1e5 semantic
points, synth-sized corner / surf) binned under its transform + the 20-shift score.

  python tools/loopdet_bench.py [--G 16 64 256] [--reps 5] [--cpu-G 16] [--kinds isc sc epsc sepsc fepsc ssc pose]

--kinds configures the database with those selectors (lisreg_loopdet_configure; default: unconfigured, i.e. FEPSC alone, and the
line is then the FEPSC bench line).  The CPU port always measures FEPSC alone.

device_ms: HIP events on the context's stream around one lisreg_loopdet_detect (upload, the six kernels, read-back and the final
synchronise); wall_ms: the call on the host clock.  cpu_port_ms: tests/loopdet_ref.py (numpy restatement + the oracle's ICP) on
one thread for the same query, kind "port"."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lis-slam_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def scans(h_big, w_big):
    from lisreg import synth
    A = np.array([0.0, 0.0, 0.3, -15.0, 0.0, synth.SENSOR_Z])
    B = np.array([0.0, 0.0, 0.3, 15.0, 0.0, synth.SENSOR_Z])
    out = {}
    for name, T, (h, w) in (("A", A, (16, 360)), ("B", B, (16, 360)), ("Q", B + [0, 0, 0.05, 0.4, 0.2, 0], (h_big, w_big))):
        s = synth.make_scan(h, w, seed=7 + len(out), labelled=True, T_true=T)
        out[name] = (s["corner"], s["surf"], synth.concat_clouds([s["corner"], s["surf"]]), synth.pose_matrix(T)[:3].astype(np.float32))
    return out


def build_history(ctx, db, sc, G, kinds=None):
    import lisreg
    off = lisreg.loopdet_default_params()
    off.inflation_covariance = -1.0                      # no gate while the history is stored
    ctx.loopdet_reset(db)
    if kinds is not None:
        ctx.loopdet_configure(kinds, db_id=db)
    frames = [sc["B"] if k % 2 == 0 else sc["A"] for k in range(2 * G)]       # ... B, A: the last stored frame is at A
    for i in range(0, len(frames), 64):
        ctx.loopdet_detect(frames[i:i + 64], db_id=db, params=off)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cpu-G", type=int, default=16)
    ap.add_argument("--h", type=int, default=64)
    ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--kinds", nargs="+", default=None, help="selectors to enable (isc sc epsc sepsc fepsc ssc pose, or all)")
    a = ap.parse_args()
    import torch
    import lisreg
    sc = scans(a.h, a.w)
    q = sc["Q"]
    kinds = None
    if a.kinds is not None:
        kinds = 127 if a.kinds == ["all"] else lisreg.loop_kinds(a.kinds)
    ctx = lisreg.Context(0)
    stream = torch.cuda.current_stream()
    ctx.set_stream(stream.cuda_stream)
    qp = lisreg.loopdet_default_params()
    qp.inflation_covariance = 1e-4                       # gates the A frames (0 m from the previous frame), never the B frames (30 m)
    rows = []
    for G in a.G:
        dev, wall = [], []
        for r in range(a.reps + 1):
            build_history(ctx, 0, sc, G, kinds)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record(stream)
            res = ctx.loopdet_detect([q], db_id=0, params=qp)[0]
            e1.record(stream)
            e1.synchronize()
            t1 = time.perf_counter()
            if r > 0:                                       # the first is warm-up (allocations, code loading)
                dev.append(e0.elapsed_time(e1)); wall.append(1e3 * (t1 - t0))
        assert res["n_candidates"] == G, res
        # batch: `batch` query frames in one call (each gates the A frames and, from the second on, the B frames before it)
        build_history(ctx, 0, sc, G, kinds)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ctx.loopdet_detect([q] * a.batch, db_id=0, params=qp)
        t1 = time.perf_counter()
        n_batch = sum(o["n_candidates"] for o in out)
        row = dict(G=G, device_ms_per_keyframe=round(float(np.median(dev)), 3), wall_ms_per_keyframe=round(float(np.median(wall)), 3),
                   candidates_per_s=round(G / (float(np.median(dev)) * 1e-3), 1), matched=res["matched_frame_id"], score=round(res["score"], 4),
                   batch_frames=a.batch, batch_candidates=n_batch, batch_ms=round(1e3 * (t1 - t0), 3),
                   batch_candidates_per_s=round(n_batch / (t1 - t0), 1))
        rows.append(row)
    cpu = None
    if a.cpu_G > 0:
        import oracle_ctypes as oc
        import loopdet_ref as R
        oc.build()
        E = R.EPSCGeneration(oc, params=(20.0, -1.0, 0.75))
        for k in range(2 * a.cpu_G):
            f = sc["B"] if k % 2 == 0 else sc["A"]
            E.loop_detection(*f)
        E.infl = 1e-4
        t0 = time.perf_counter()
        r = E.loop_detection(*q)
        t1 = time.perf_counter()
        assert len(r["candidates"]) == a.cpu_G
        cpu = dict(kind="port", G=a.cpu_G, ms_per_keyframe=round(1e3 * (t1 - t0), 1), threads=1,
                   what="tests/loopdet_ref.py: numpy restatement + oracle ICP")
    ctx.close()
    line = dict(workload="loopdet_fepsc", semantic_points=int(len(q[2])), corner_points=int(len(q[0])),
                surf_points=int(len(q[1])), rows=rows, cpu_baseline=cpu,
                stage_split="per kernel: rocprofv3 --kernel-trace --stats, profiles/loopdet_*")
    if kinds is not None:
        line["workload"] = "loopdet_kinds"
        line["kinds"] = [n for k, n in enumerate(lisreg.LOOP_KIND_NAMES) if (kinds >> k) & 1]
    print(json.dumps(line))


if __name__ == "__main__":
    main()
