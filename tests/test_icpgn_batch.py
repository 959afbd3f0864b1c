"""lisreg_icp_gn_match_batch on the GPU: the candidate loop of detectLoopClosureForSubMapICP
(src/node/subMapOptmizationNode.cpp:2496-2621) over OptimizedICPGN (src/core/registration.cpp:19-115) as one call.

The contract is "batch equals single, in all 80 bytes of lisreg_icpgn_result": every comparison with lisreg_icp_gn_match below is of
bytes.  The single call itself is held to the bytes the commit before the batch returned (tests/golden/icpgn_batch/, recorded by
tests/golden/make_golden_icpgn_batch.py), since its kernels now share their arithmetic with the batch's.  Inputs: tests/icpgn_batch_cases.py;
the definition of the batch and of `best`: tests/icpgn_batch_ref.py; the CPU side: tests/test_icpgn_batch_host.py."""
import ctypes as C
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import icpgn_batch_cases as K
import icpgn_batch_ref as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "icpgn_batch", "icpgn_parent_outputs.npz")
f32 = np.float32


def _items(spec, poses):
    import lisreg
    return [lisreg.IcpGnItem(s, slot, None if p is None else poses[p]) for s, slot, p in spec]


def _bytes(results):
    return [r["bytes"] for r in results]


def _explain(got, want):
    """which items differ, and in which of the twenty 4-byte words"""
    out = []
    for k, (a, b) in enumerate(zip(got, want)):
        if a != b:
            wa, wb = np.frombuffer(a, np.uint32), np.frombuffer(b, np.uint32)
            out.append((k, np.nonzero(wa != wb)[0].tolist(), np.frombuffer(a, f32)[[3, 7, 11, 18]].tolist(), np.frombuffer(b, f32)[[3, 7, 11, 18]].tolist()))
    return out


@pytest.fixture(scope="module")
def small(gpu_ctx):
    """the two targets in their slots and the single calls of the batch of eight under both parameter sets, made once"""
    K.set_targets(gpu_ctx)
    tgt_a, tgt_b, sources, poses = K.small_scene()
    return SimpleNamespace(tgt={K.SLOT_A: tgt_a, K.SLOT_B: tgt_b}, sources=sources, poses=poses, spec=K.small_items(),
                           single=K.small_single_all(gpu_ctx))


@pytest.fixture(scope="module")
def large(gpu_ctx):
    assert not os.environ.get("LISREG_NN1_Q"), "LISREG_NN1_Q is set: every source would get the same lanes per query; unset it for this test"
    K.set_targets(gpu_ctx, large=True)
    return SimpleNamespace(sources=K.large_scene()[1], single=K.large_single_all(gpu_ctx))


def test_the_single_call_still_gives_the_parent_commits_bytes(small, large):
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024 and g["small"].shape == (2, 8, 80) and g["large"].shape == (3, 80)
    for s in range(2):
        got, want = small.single[s], [bytes(r) for r in g["small"][s]]
        assert got == want, (K.PARAM_SETS[s], _explain(got, want))
    got, want = large.single, [bytes(r) for r in g["large"]]
    assert got == want, _explain(got, want)


@pytest.mark.parametrize("pset", [0, 1])
def test_a_batch_of_eight_equals_the_single_calls_in_all_80_bytes(gpu_ctx, small, pset):
    import lisreg
    iters, max_d = K.PARAM_SETS[pset]
    res, info = gpu_ctx.icp_gn_match_batch(small.sources, _items(small.spec, small.poses), iters, max_d)
    assert all(len(b) == 80 for b in _bytes(res))
    assert _bytes(res) == small.single[pset], _explain(_bytes(res), small.single[pset])
    assert info["n_sources_staged"] == 8 and info["n_syncs"] == 1
    assert info["best"] == B.best_of([r["fitness"] for r in res])
    far = res[7]
    assert far["steps_applied"] == 0 and far["n_corr_last"] == 0 and far["fitness"] > 1e5        # 1 000 m away: no correspondence, no step
    assert res[0]["steps_applied"] == iters and res[1]["n_corr_last"] == 1
    # device records in give the same bytes as host structs in
    dev = [lisreg.DeviceArray(lisreg.pack_device_records(s)) for s in small.sources]
    try:
        res_d, info_d = gpu_ctx.icp_gn_match_batch([(d.ptr, len(s)) for d, s in zip(dev, small.sources)], _items(small.spec, small.poses), iters, max_d)
        assert _bytes(res_d) == small.single[pset], _explain(_bytes(res_d), small.single[pset])
        assert info_d == info
        # whatever else is in the batch: the items in another order, and a subset
        order = [5, 0, 7, 2, 6, 1]
        res_o, _ = gpu_ctx.icp_gn_match_batch(small.sources, _items([small.spec[k] for k in order], small.poses), iters, max_d)
        assert _bytes(res_o) == [small.single[pset][k] for k in order]
    finally:
        for d in dev:
            d.free()


def test_the_lane_classes_in_one_batch(gpu_ctx, large):
    """249 999, 250 000 and 500 000 points: the sizes at which the lanes per query of a single call change (icp_lanes); every item keeps
    its own, so the batch runs one correspondence launch per class present"""
    import lisreg
    iters, max_d = K.LARGE_PARAMS
    res, info = gpu_ctx.icp_gn_match_batch(large.sources, [lisreg.IcpGnItem(k, K.SLOT_L) for k in (2, 0, 1)], iters, max_d)
    want = [large.single[k] for k in (2, 0, 1)]
    assert _bytes(res) == want, _explain(_bytes(res), want)
    assert [r["steps_applied"] for r in res] == [iters] * 3 and info["n_sources_staged"] == 3


def test_edges_equal_the_single_call(gpu_ctx, small):
    import lisreg
    src, cut = small.sources[0], small.sources[5]
    bad = src.copy(); bad["x"][::7] = np.nan                     # pcl::isFinite filter
    P = small.poses
    its = [lisreg.IcpGnItem(0, K.SLOT_A, P[0]), lisreg.IcpGnItem(1, K.SLOT_B, None), lisreg.IcpGnItem(2, K.SLOT_B, P[1])]
    for iters, max_d in ((0, 4.0), (3, -1.0), (3, 4.0), (65, 4.0)):
        res, info = gpu_ctx.icp_gn_match_batch([src, cut, bad], its, iters, max_d)
        want = [K.single_bytes(gpu_ctx, K.SLOT_A, src, iters, max_d, P[0]), K.single_bytes(gpu_ctx, K.SLOT_B, cut, iters, max_d, None),
                K.single_bytes(gpu_ctx, K.SLOT_B, bad, iters, max_d, P[1])]
        assert _bytes(res) == want, ((iters, max_d), _explain(_bytes(res), want))
        if iters == 0 or max_d < 0:
            assert all(r["steps_applied"] == 0 and r["n_corr_last"] == 0 for r in res) and res[0]["T"].tobytes() == P[0].tobytes()
            assert res[0]["fitness"] > 0
        if max_d >= 0:
            assert info["n_syncs"] == iters // 64 + 1
        if iters == 65:
            assert info["n_syncs"] == 2                            # the bounding synchronisation after iteration 64, and the read-back
    assert 0 < res[2]["n_corr_last"] <= len(bad) - len(bad[::7])


def test_info_and_the_sources(gpu_ctx, small):
    import lisreg
    src = small.sources[0]
    its = [lisreg.IcpGnItem(1, K.SLOT_A if k % 2 else K.SLOT_B, small.poses[k % 3]) for k in range(16)]
    # one source under 16 items is staged once; the sources nobody names may be NULL with any n
    L = gpu_ctx._L
    ptrs = (C.c_void_p * 3)(None, src.ctypes.data, None)
    ns = (C.c_int * 3)(12345, len(src), -7)
    arr = (lisreg.IcpGnItemC * 16)()
    for k, it in enumerate(its):
        arr[k].source, arr[k].slot = it.source, it.slot
        arr[k].predict_pose = it.predict_pose.ctypes.data_as(C.POINTER(C.c_float))
    out = (lisreg.IcpGnResult * 16)()
    info = lisreg.IcpGnBatchInfo()
    rc = L.lisreg_icp_gn_match_batch(gpu_ctx._h, ptrs, ns, 3, src.dtype.itemsize, lisreg._fmt_of(src), arr, 16, 3, 25.0, out, C.byref(info))
    assert rc == 0, rc
    assert (info.n_sources_staged, info.n_syncs, info.reserved) == (1, 1, 0)
    for k in (0, 1, 2, 15):
        assert bytes(out[k]) == K.single_bytes(gpu_ctx, its[k].slot, src, 3, 25.0, its[k].predict_pose), k
    assert bytes(out[0]) == bytes(out[6]) and bytes(out[0]) != bytes(out[1])
    assert info.best == B.best_of([out[k].fitness for k in range(16)])
    # no items: LISREG_OK, best -1, nothing read
    info = lisreg.IcpGnBatchInfo(5, 5, 5, 5)
    assert L.lisreg_icp_gn_match_batch(gpu_ctx._h, None, None, 0, 0, 0, None, 0, 3, 25.0, None, C.byref(info)) == 0
    assert (info.best, info.n_sources_staged, info.n_syncs) == (-1, 0, 0)
    res, inf = gpu_ctx.icp_gn_match_batch([], [], 30, 10.0)
    assert res == [] and inf["best"] == -1
    assert L.lisreg_icp_gn_match_batch(gpu_ctx._h, None, None, 0, 0, 0, None, 0, 3, 25.0, None, None) == 0          # info may be NULL


def test_best_follows_the_ref(gpu_ctx, small):
    import lisreg
    spec = small.spec
    # a tie made by listing one item twice: the later copy wins, wherever the copies stand
    for order in ([3, 0, 3, 7], [5, 5, 0], [0, 3, 5, 7, 3, 5], [7, 0]):
        res, info = gpu_ctx.icp_gn_match_batch(small.sources, _items([spec[k] for k in order], small.poses), 3, 25.0)
        scores = [r["fitness"] for r in res]
        assert info["best"] == B.best_of(scores), (order, scores, info)
        assert info["best"] == max(k for k, s in enumerate(scores) if s == min(scores))
    res, info = gpu_ctx.icp_gn_match_batch(small.sources, _items([spec[3], spec[0], spec[3]], small.poses), 3, 25.0)
    assert res[0]["bytes"] == res[2]["bytes"] and info["best"] == 2


def test_against_the_cpu_restatement(oracle, gpu_ctx, small):
    """two items at the tolerances tests/test_icp.py::test_hip_icp_gn_matches_oracle holds the single call to"""
    from test_icp import _pose_diff
    spec = [(0, K.SLOT_A, small.poses[0]), (0, K.SLOT_B, None)]
    ref, best = B.match_batch(oracle, small.tgt, small.sources, spec, 12, 4.0)
    import lisreg
    res, info = gpu_ctx.icp_gn_match_batch(small.sources, [lisreg.IcpGnItem(*s) for s in spec], 12, 4.0)
    for rg, ro in zip(res, ref):
        assert rg["steps_applied"] == ro["steps_applied"] == 12
        dr, dt = _pose_diff(rg["T"], ro["T"])
        print(f"[icpgn_batch] against the restatement: {dr:.3e} rad, {dt:.3e} m, fitness {rg['fitness']:.6g} / {ro['fitness']:.6g}, "
              f"correspondences {rg['n_corr_last']} / {ro['n_corr_last']}")
        assert dr < 1e-3 and dt < 1e-3, (dr, dt)
        assert abs(rg["fitness"] - ro["fitness"]) <= 2e-3 * ro["fitness"]
        assert abs(rg["n_corr_last"] - ro["n_corr_last"]) <= max(3, ro["n_corr_last"] // 2000)
    assert info["best"] == best


def test_every_refusal_leaves_the_results_untouched(gpu_ctx, small):
    import lisreg
    L, h = gpu_ctx._L, gpu_ctx._h
    src, cut = small.sources[0], small.sources[3]
    stride, fmt = src.dtype.itemsize, lisreg.FMT_XYZIL
    pat = bytes([0xA5]) * (80 * 2)

    def call(ptrs, ns, n_sources, stride, fmt, items, n_items, iters, max_d=4.0, results=True, null=()):
        p = (C.c_void_p * max(len(ptrs), 1))(*ptrs)
        n = (C.c_int * max(len(ns), 1))(*ns)
        arr = (lisreg.IcpGnItemC * max(len(items), 1))()
        for k, (s, slot) in enumerate(items):
            arr[k].source, arr[k].slot = s, slot
        out = (lisreg.IcpGnResult * 2).from_buffer_copy(pat)
        info = lisreg.IcpGnBatchInfo(7, 7, 7, 7)
        rc = L.lisreg_icp_gn_match_batch(h, None if "sources" in null else p, None if "n" in null else n, n_sources, stride, fmt,
                                         None if "items" in null else arr, n_items, iters, max_d, out if results else None, C.byref(info))
        assert bytes(out) == pat and (info.best, info.n_syncs) == (7, 7), "a refused call wrote"
        return rc
    two = [src.ctypes.data, cut.ctypes.data]
    ns = [len(src), len(cut)]
    ok_items = [(0, K.SLOT_A), (1, K.SLOT_B)]
    E, NT = lisreg.ERR_ARG, lisreg.ERR_NO_TARGET
    assert call(two, ns, 2, stride, fmt, ok_items, 2, 3, null=("items",)) == E
    assert call(two, ns, 2, stride, fmt, ok_items, 2, 3, results=False) == E
    assert call(two, ns, 2, stride, fmt, ok_items, 2, 3, null=("sources",)) == E
    assert call(two, ns, 2, stride, fmt, ok_items, 2, 3, null=("n",)) == E
    assert call(two, ns, 2, stride, fmt, ok_items, -1, 3) == E
    assert call(two, ns, 2, stride, fmt, [(0, K.SLOT_A), (2, K.SLOT_B)], 2, 3) == E              # a source index out of range
    assert call(two, ns, 2, stride, fmt, [(-1, K.SLOT_A), (1, K.SLOT_B)], 2, 3) == E
    assert call(two, ns, 2, stride, fmt, [(0, K.SLOT_A), (1, 888)], 2, 3) == NT                   # a slot without a map index
    assert call(two, ns, 2, stride, fmt, [(0, -1), (1, K.SLOT_B)], 2, 3) == NT
    assert call(two, ns, 2, stride, fmt, ok_items, 2, 100001) == E
    # a named source the single call refuses: the (cloud, n, stride, fmt) contract of lisreg_icp_gn_match
    assert call([src.ctypes.data, None], ns, 2, stride, fmt, ok_items, 2, 3) == E                 # NULL cloud with n > 0
    assert call(two, [len(src), -1], 2, stride, fmt, ok_items, 2, 3) == E                         # n < 0
    assert call(two, ns, 2, 21, fmt, ok_items, 2, 3) == E                                         # stride below the label's offset
    assert call(two, ns, 2, 11, lisreg.FMT_XYZI, ok_items, 2, 3) == E
    for bad_fmt in (lisreg.FMT_DEVICE_XYZI, lisreg.FMT_XYZI_PACKED, 17, -1, 40):
        assert call(two, ns, 2, stride, bad_fmt, ok_items, 2, 3) == E, bad_fmt
    # ... while n = 0 is a source like any other (a fault in a source nobody names is not looked at: test_info_and_the_sources)
    res, info = gpu_ctx.icp_gn_match_batch([src, src[:0]], [lisreg.IcpGnItem(1, K.SLOT_A), lisreg.IcpGnItem(0, K.SLOT_A, small.poses[0])], 3, 4.0)
    assert res[0]["bytes"] == K.single_bytes(gpu_ctx, K.SLOT_A, src[:0], 3, 4.0, None) and res[0]["fitness"] == np.finfo(f32).max
    assert res[1]["bytes"] == K.single_bytes(gpu_ctx, K.SLOT_A, src, 3, 4.0, small.poses[0]) and info["best"] == 1
    # workgroups / partial rows / source points over all items that do not fit 32-bit counts: refused before anything is allocated or
    # read (the pointer is never followed: device format, 3 items of 2^30 points)
    big = 1 << 30
    p3 = (C.c_void_p * 1)(0x1000); n3 = (C.c_int * 1)(big)
    arr = (lisreg.IcpGnItemC * 3)()
    for k in range(3):
        arr[k].source, arr[k].slot = 0, K.SLOT_A
    out = (lisreg.IcpGnResult * 3).from_buffer_copy(bytes([0xA5]) * 240)
    assert L.lisreg_icp_gn_match_batch(h, p3, n3, 1, 16, lisreg.FMT_DEVICE, arr, 3, 3, 4.0, out, None) == E
    assert bytes(out) == bytes([0xA5]) * 240


def test_interleaved_with_the_other_users_of_the_icp_scratch(small):
    """icp_align_batch, icp_gn_match, the new batch, then the first two again on one context: every call returns the bytes it returns
    on a context that made no other call"""
    import lisreg
    from test_caller_stream import same
    srcs, P = small.sources, small.poses
    pg = lisreg.icp_default_params(0)
    icp_items = [(K.SLOT_A, srcs[0], P[0]), (K.SLOT_B, srcs[5], None), (K.SLOT_A, srcs[6], P[1])]
    gn_items = _items(small.spec, P)

    def fresh():
        c = lisreg.Context(0)
        K.set_targets(c)
        return c
    a, b, d = fresh(), fresh(), fresh()
    try:
        alone_icp = a.icp_align_batch(icp_items, pg)
        alone_gn = K.single_bytes(b, K.SLOT_B, srcs[0], 12, 4.0, P[2])
        alone_batch = _bytes(d.icp_gn_match_batch(srcs, gn_items, 12, 4.0)[0])
    finally:
        a.close(); b.close()
    try:
        c = d                                                     # (has made the batch call alone; now the sequence)
        seq = [c.icp_align_batch(icp_items, pg), K.single_bytes(c, K.SLOT_B, srcs[0], 12, 4.0, P[2]),
               _bytes(c.icp_gn_match_batch(srcs, gn_items, 12, 4.0)[0]), c.icp_align_batch(icp_items, pg),
               K.single_bytes(c, K.SLOT_B, srcs[0], 12, 4.0, P[2]), _bytes(c.icp_gn_match_batch(srcs, gn_items, 12, 4.0)[0])]
    finally:
        d.close()
    assert same(seq[0], alone_icp) and same(seq[3], alone_icp)
    assert seq[1] == alone_gn and seq[4] == alone_gn
    assert seq[2] == alone_batch == seq[5] == small.single[0]


def test_twenty_calls_do_not_change_free_device_memory(gpu_ctx, small):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        hip.hipDeviceSynchronize()
        f, t = C.c_size_t(0), C.c_size_t(0)
        assert hip.hipMemGetInfo(C.byref(f), C.byref(t)) == 0
        return f.value
    items = _items(small.spec, small.poses)
    gpu_ctx.icp_gn_match_batch(small.sources, items, 3, 25.0)
    before = free_bytes()
    for _ in range(20):
        res, _info = gpu_ctx.icp_gn_match_batch(small.sources, items, 3, 25.0)
    assert _bytes(res) == small.single[1]
    assert free_bytes() == before
    res, _info = gpu_ctx.icp_gn_match_batch(small.sources, items[2:5], 3, 25.0)      # a smaller batch fits into what is there
    assert _bytes(res) == small.single[1][2:5] and free_bytes() == before


def test_on_a_callers_busy_stream_the_source_arrives_late(small):
    """the late_case pattern of tests/test_caller_stream.py: the device source holds a decoy, the real records arrive on the caller's stream
    behind a stall; ordered on that stream the batch gives the idle-stream bytes"""
    import lisreg
    from stream_gate import Gate
    from test_caller_stream import late_case, moved
    gate = Gate()
    # The call is eight short launches and two small copies (0.27 ms on an idle GPU), and in the control run it shares the GPU with the
    # stall's 256 MiB copies, which slow it several times over: 3 x t_call (0.84 ms) was once shorter than the control call itself.  The
    # stall of this test is therefore at least 10 ms, an order of magnitude above the call under contention.
    rule = gate.stall_ms_for
    gate.stall_ms_for = lambda t_call_s: max(rule(t_call_s), 10.0)
    ctx = lisreg.Context(0)
    e = SimpleNamespace(gate=gate, ctx=ctx, S=gate.stream_create(), hip=gate.hip, lisreg=lisreg, D=lisreg.DeviceArray)
    try:
        K.set_targets(ctx)
        src = small.sources[0]
        rs = lisreg.pack_device_records(src)
        spec = [(0, K.SLOT_A, 0), (0, K.SLOT_B, None), (0, K.SLOT_A, 2)]
        items = _items(spec, small.poses)

        def make(dst):
            return (lambda: ctx.icp_gn_match_batch([(dst.ptr, len(rs))], items, 3, 25.0)), (lambda r: dict(res=_bytes(r[0]), info=r[1]))
        o, _ = late_case(e, "icp_gn_match_batch (device source)", rs, moved(rs, small=True), make)
        want = [K.single_bytes(ctx, slot, src, 3, 25.0, None if p is None else small.poses[p]) for _, slot, p in spec]
        assert o["res"] == want, _explain(o["res"], want)
    finally:
        ctx.set_stream(None)
        gate.hip.hipDeviceSynchronize()
        gate.stream_destroy(e.S)
        ctx.close()
        gate.close()


def test_the_smoke_program_runs_and_prints_its_ok_line():
    host = os.path.join(ROOT, "lis-slam_amd", "host")
    exe = os.path.join(host, "icpgn_batch_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", host, "icpgn_batch_smoke"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "icpgn_batch_smoke ok" in r.stdout and "same as alone: 0" not in r.stdout, r.stdout + r.stderr
