"""Round 6: behaviour the round-5 review asked to pin."""
import ctypes as C
import time

import numpy as np
import pytest


def _pipeline_setup(n_extra_contexts, tile=8):
    """One context + `n_extra_contexts` other contexts that have each run a registration (their streams exist and are alive — the reference
    runs three node objects in one process, subMapOptmizationNode.cpp:5188-5195); a batch of pinned host clouds big enough for the
    feeder's thread pool (>= 262 144 points) whose upload and whose registration take about as long as each other."""
    import lisreg
    from lisreg import synth
    cases = [synth.make_case(h=64, w=900, m_points=40000, scan_seed=3600 + i) for i in range(6)]
    p = lisreg.default_params(1)
    p.fixed_iters = 10
    extra = []
    for k in range(n_extra_contexts):
        cx = lisreg.Context(0)
        cx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
        cx.align_batch([dict(src_corner=c["src_corner"], src_surf=c["src_surf"]) for c in cases[:2]],
                       np.stack([c["T_init"] for c in cases[:2]]).astype(np.float32), p)      # its compute, side and copy streams now exist
        extra.append(cx)
    # ... and a pool of idle streams like the one a PyTorch process holds (32 per priority, created together): they take references on the
    # process's hardware queues, so the streams created next share queues with each other rather than getting one each
    hip = lisreg.hip_runtime()
    pool = []
    for _ in range(32):
        sh = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(sh), C.c_uint(1)) == 0          # hipStreamNonBlocking
        pool.append(sh)
    ctx = lisreg.Context(0)
    ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
    n = len(cases) * tile
    keep, arr = [], (lisreg.Item * n)()
    pinned = {}
    for i in range(n):
        c = cases[i % len(cases)]
        for key in ("src_corner", "src_surf"):
            if (i % len(cases), key) not in pinned:
                pinned[(i % len(cases), key)] = lisreg.PinnedArray(np.ascontiguousarray(c[key]))
            t = pinned[(i % len(cases), key)]
            if key == "src_corner": arr[i].src_corner = C.c_void_p(t.ptr); arr[i].n_corner = len(c[key])
            else: arr[i].src_surf = C.c_void_p(t.ptr); arr[i].n_surf = len(c[key])
        arr[i].stride_bytes = c["src_surf"].dtype.itemsize; arr[i].fmt = lisreg.FMT_XYZI
    T0 = np.ascontiguousarray(np.stack([cases[i % len(cases)]["T_init"] for i in range(n)]).astype(np.float32))
    return lisreg, ctx, extra, list(pinned.values()), arr, n, T0, p, pool


@pytest.mark.gpu
def test_upload_hides_under_kernels_with_other_contexts_alive():
    """SURVEY section 8(d)'s metric includes the H2D of the sources: `lisreg_stage_host_items` for batch k + 1 has to run UNDERNEATH the
    kernels of batch k, whatever other contexts (streams) the process holds.  HIP maps streams onto a few hardware queues; rounds 3-5 put
    a device-side wait and the packing kernels on the copy stream, and with a few contexts alive those packets queued behind the running
    batch's kernels — the upload started when the batch ended (driver BENCH_r05: 12.8 k reg/s pipelined = the in-series rate, 21.8 k in
    round 4).  Round 6: the copy stream carries copies only.  Gate: with four extra contexts alive the pipelined
    stage -> fetch -> launch step takes at most 1.25 x max(stage alone, registration alone) (in series it is their sum)."""
    lisreg, ctx, extra, keep, arr, n, T0, p, pool = _pipeline_setup(4)
    L = ctx._L
    hip = lisreg.hip_runtime()
    fp = C.POINTER(C.c_float)
    staged = (lisreg.Item * n)()
    ctx._n_items = n

    def stage(): assert L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
    def launch():
        assert L.lisreg_batch_prepare(ctx._h, n, staged, C.byref(p), T0.ctypes.data_as(fp)) == 0
        assert L.lisreg_batch_run(ctx._h) == 0
    def fetch(): return ctx.batch_fetch()

    stage(); launch(); T_ref, st_ref = fetch()
    stage(); launch(); fetch()                                 # both staging buffers warm
    # stage alone / registration alone (sources already staged), medians
    ts, tr = [], []
    for _ in range(7):
        hip.hipDeviceSynchronize(); t0 = time.perf_counter(); stage(); hip.hipDeviceSynchronize(); ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); launch(); fetch(); tr.append(time.perf_counter() - t0)
    t_stage, t_run = sorted(ts)[len(ts) // 2], sorted(tr)[len(tr) // 2]
    steps, best = 12, 1e9
    for _ in range(4):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        stage(); launch()
        for _ in range(steps - 1):
            stage(); T, st = fetch(); launch()
        T, st = fetch()
        best = min(best, (time.perf_counter() - t0) / steps)
        assert np.array_equal(T, T_ref) and st == st_ref
    print(f"[overlap] {n} registrations, 4 other contexts alive: stage alone {1e3 * t_stage:.2f} ms, registration alone {1e3 * t_run:.2f} ms, "
          f"pipelined step {1e3 * best:.2f} ms (in series {1e3 * (t_stage + t_run):.2f}); chunks taken by the copy engine "
          f"{ctx.get_option('feeder_chunks_by_copy_engine')} of {ctx.get_option('feeder_chunks')}")
    ctx.close()
    for cx in extra: cx.close()
    for t in keep: t.free()
    for sh in pool: hip.hipStreamDestroy(sh)
    assert best <= 1.25 * max(t_stage, t_run) + 1.0e-4, (best, t_stage, t_run)


@pytest.mark.gpu
def test_row_reach_builds_fewer_rows_and_changes_nothing(gpu_ctx):
    """Option "row_reach" (round 6, default on): a run that rebuilds its targets builds cell rows only for the cells a query of the batch
    comes within two cells of under its initial pose (query marks made at the start of the run).  A query that reaches a cell without rows
    takes the cell walk, so poses and statistics are the bits of the unfiltered run; the table says -1 ("no row") for the cells left out,
    never -2 ("nothing within two cells"), and the cells that keep their rows keep the same octant masks."""
    import lisreg
    from lisreg import synth
    D = lisreg.DeviceArray
    tc, ts = synth.make_submap(60000)
    n = 8
    scans = [synth.make_scan(32, 900, 2000 + i) for i in range(n)]
    T0 = np.array([synth.perturb_pose(s["T_true"], np.random.default_rng(9000 + i)) for i, s in enumerate(scans)], np.float32)
    p = lisreg.default_params(1); p.fixed_iters = 8
    tcd, tsd = D(lisreg.pack_device_records(tc)), D(lisreg.pack_device_records(ts))
    recs = [(D(lisreg.pack_device_records(s["corner"])), D(lisreg.pack_device_records(s["surf"]))) for s in scans]
    items = [dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0]) for a, b in recs]
    out = {}
    try:
        gpu_ctx.set_option("search_mode", 5); gpu_ctx.set_option("rebuild_targets_each_run", 1); gpu_ctx.set_option("sort_sources", 0)
        for reach in (0, 1, 0):
            gpu_ctx.set_option("row_reach", reach)
            gpu_ctx.set_target_device(tcd.ptr, len(tc), tsd.ptr, len(ts))
            gpu_ctx.batch_prepare_device(items, T0, p)
            assert gpu_ctx.get_option("front_end") == 5
            gpu_ctx.batch_run()
            T, st = gpu_ctx.batch_fetch()
            gpu_ctx.batch_run()                                   # a second run re-makes the marks from clean words: the same again
            T2, st2 = gpu_ctx.batch_fetch()
            assert np.array_equal(T, T2) and st == st2
            assert gpu_ctx.get_option("row_reach_now") == reach
            tabs = [gpu_ctx.target_cell_rows(0, k) for k in (0, 1)]
            if reach in out:
                assert np.array_equal(out[reach][0], T) and out[reach][1] == st           # (switching back restores the full table)
                assert all(np.array_equal(a["table"], b["table"]) for a, b in zip(out[reach][2], tabs))
            out[reach] = (T, st, tabs)
    finally:
        gpu_ctx.set_option("search_mode", 4); gpu_ctx.set_option("rebuild_targets_each_run", 0); gpu_ctx.set_option("sort_sources", 2)
        gpu_ctx.set_option("row_reach", 1)
    (Ta, sa, ta), (Tb, sb, tb) = out[0], out[1]
    assert np.array_equal(Ta, Tb) and sa == sb
    for k in (0, 1):
        full, part = ta[k]["table"], tb[k]["table"]
        assert np.array_equal(full == -2, part == -2)                       # "nothing within two cells" is a fact about the target, not about the batch
        kept = part >= 0
        assert np.all(full[kept] >= 0) and np.array_equal(full[kept] & 255, part[kept] & 255)
        dropped = (full >= 0) & (part == -1)
        print(f"[row_reach] kind {k}: {ta[k]['n_rows']} rows -> {tb[k]['n_rows']}; cells with rows {int((full >= 0).sum())} -> {int(kept.sum())}")
        assert tb[k]["n_rows"] < ta[k]["n_rows"] and dropped.any()
