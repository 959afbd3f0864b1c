"""The library on a caller's BUSY stream (lisreg_set_stream): what bench.py, tools/loopdet_bench.py and INTEGRATION.md section 3c rely on.

Every other GPU test runs on the context's own stream, idle whenever a call starts; there a kernel or copy on a wrong stream (or on the
null stream, which orders nothing against hipStreamNonBlocking streams) and a staging buffer reused before its copy ran both pass.  Here
the caller's stream S is kept busy by tests/stream_gate.py (a bounded chain of device-to-device copies) and

 A. every device-resident entry point gets its input LATE: the input buffer holds a decoy, the real input arrives on S behind the stall.
    Ordered run (context on S): the outputs are, bit for bit, those of the same call on the idle own stream with the real input — and
    that idle result is held against the CPU reference the entry point's own test uses, where the suite has one in that form.  Control
    run (context on its own stream, producer on S — a caller's mistake): the outputs are the DECOY's; a control that returns the real
    result fails with "stall too short", so the harness is shown to detect misordering for this call on this machine.
 B. lisreg_concat_device, lisreg_submap_gather (device destination) and lisreg_batch_run return while an event behind the stall is
    still pending, and their output is consumed on S by a plain copy, with no host wait in between.  The forks of the library's side
    streams (interleaved halves, the strip build) get a late input of their own: a second-half item's source, the 2.1 M-point target.
 C. several calls are queued behind one stall (host staging reused while its copy has not run).
 D. a pending run meets a change of something the library owns (its copy of a host target, a submap store, the search counters).
 E. lisreg_set_stream itself.      F. torch on its own stream, no torch.cuda.synchronize() until the results are read."""
import ctypes as C
import os
import subprocess
import sys
import textwrap
from types import SimpleNamespace

import numpy as np
import pytest

import globalmap_ref as GR
import pretreat_ref as PR
import rangenet_ref as RR
from stream_gate import Gate, H2D, to_host

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEANS = (12.12, 10.88, 0.23, -1.04, 0.21)
STDS = (12.32, 11.47, 6.91, 0.86, 0.16)
NAMES = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
ZERO_POSE = np.zeros(6, np.float32)
f32 = np.float32


@pytest.fixture(scope="module")
def env():
    import lisreg
    gate = Gate()
    ctx = lisreg.Context(0)
    e = SimpleNamespace(gate=gate, ctx=ctx, S=gate.stream_create(), hip=gate.hip, lisreg=lisreg, D=lisreg.DeviceArray)
    yield e
    print("\n" + gate.report())
    ctx.set_stream(None)
    gate.hip.hipDeviceSynchronize()
    gate.stream_destroy(e.S)
    ctx.close()
    gate.close()


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def same(a, b):
    """equal word for word: arrays by their bytes (NaNs included), containers element by element"""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (a != a and b != b)
    return a == b


def moved(rec, small=False, roll_payload=False):
    """a different valid cloud of the same size: the (n, 4) records turned about z and shifted, the payload kept (or rolled)"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    a, t = (0.02, (0.12, -0.07, 0.03)) if small else (0.5, (1.5, -0.7, 0.05))
    c, s = f32(np.cos(a)), f32(np.sin(a))
    out = rec.copy()
    with np.errstate(invalid="ignore"):
        out[:, 0] = c * rec[:, 0] - s * rec[:, 1] + f32(t[0])
        out[:, 1] = s * rec[:, 0] + c * rec[:, 1] + f32(t[1])
        out[:, 2] = rec[:, 2] + f32(t[2])
    if roll_payload:
        out[:, 3] = np.roll(rec[:, 3], 7)
    return out


def records_pcl(rec, labelled=True):
    """(n, 4) records back as the PCL structs the CPU references take (payload = label)"""
    from lisreg import synth
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    return synth.to_pcl(rec[:, :3].copy(), (rec[:, 3].copy().view(np.uint32) & 0xffff).astype(np.uint16) if labelled else None)


def cat_pcl(a, b):
    o = np.zeros(len(a) + len(b), a.dtype)
    o[: len(a)], o[len(a):] = a, b
    return o


def settle(e):
    e.hip.hipDeviceSynchronize()


def fill(e, dst, src):
    """dst <- src (device arrays), complete on return"""
    settle(e)
    dst.copy_from_device(src.ptr, src.nbytes)
    settle(e)


def stall_for(e, fn):
    """t_call of fn on the idle stream (fn has run before: its allocations are made) -> the stall the header of stream_gate asks for"""
    settle(e)
    _, t = e.gate.wall(fn)
    settle(e)
    return e.gate.stall_ms_for(t)


def late_case(e, name, real, decoy, make_call):
    """Section A for one entry point.  make_call(dst) -> (run, fetch): run() makes the library calls that read the device array `dst`
    and returns what they return; fetch(ret) reads the outputs back (every stream is idle by then).  Returns the idle-stream outputs
    for the real and for the decoy input."""
    gate, ctx, S = e.gate, e.ctx, e.S
    real, decoy = np.ascontiguousarray(real), np.ascontiguousarray(decoy)
    assert real.shape == decoy.shape and real.dtype == decoy.dtype and real.tobytes() != decoy.tobytes()
    d_real, d_decoy, dst = e.D(real), e.D(decoy), e.D(decoy)
    run, fetch = make_call(dst)

    def idle(src):
        fill(e, dst, src)
        ret, t = gate.wall(run)
        gate.stream_sync(ctx.stream); settle(e)
        return fetch(ret), t
    assert ctx.stream != S
    out_decoy, _ = idle(d_decoy)                       # also the warm-up: every allocation of the call is made
    out_real, _ = idle(d_real)
    again, t_call = idle(d_real)
    assert same(out_real, again), (name, "the call is not repeatable on the idle stream")
    assert not same(out_real, out_decoy), (name, "real and decoy give the same outputs: the case shows nothing")
    ms = gate.stall_ms_for(t_call)
    # ordered: the context runs on the caller's stream.  The call has just run on the DECOY: whatever the library keeps between calls
    # (sorted sources, strip tables, result block) holds the decoy's values, so work that ran ahead of the late input shows
    idle(d_decoy)
    ctx.set_stream(S)
    try:
        assert ctx.stream == S
        gate.late_input(S, dst, d_real, d_decoy, ms)
        ret = run()
        gate.stream_sync(S)
    finally:
        ctx.set_stream(None)
    settle(e)
    got = fetch(ret)
    assert same(got, out_real), (name, "ordered run on the busy caller's stream differs from the idle-stream result",
                                 "it equals the DECOY's result" if same(got, out_decoy) else "it equals neither")
    # control: the producer is on S, the context on its own stream
    fill(e, dst, d_decoy)
    gate.late_input(S, dst, d_real, d_decoy, ms)
    ev = gate.mark(S)
    ret = run()
    gate.stream_sync(ctx.stream)
    pending = gate.event_pending(ev)
    gate.stream_sync(S); settle(e)
    gate.event_destroy(ev)
    got = fetch(ret)
    print(f"[caller_stream] {name}: t_call {1e3 * t_call:.3f} ms, stall {ms:.2f} ms, producer still pending after the control call: {pending}")
    assert pending, (name, "stall too short: the producer on the caller's stream had finished when the control call returned")
    assert not same(got, out_real), (name, "stall too short: the control run (context on its own stream) returned the real result", pending)
    assert same(got, out_decoy), (name, "control run returned neither the decoy's nor the real result", pending)
    for a in (d_real, d_decoy, dst):
        a.free()
    return out_real, out_decoy


def cparams(P):
    import lisreg
    p = lisreg.default_rangenet_params(P.img_h, P.img_w)
    p.fov_up, p.fov_down, p.n_classes = P.fov_up, P.fov_down, P.n_classes
    for k in range(5):
        p.means[k], p.stds[k] = float(P.means[k]), float(P.stds[k])
    return p


def sweep(seed):
    """a raw sweep of 16 rings x 450 columns: (n, 4) float32 x y z intensity, with the non-finite points make_sweep injects"""
    return PR.make_sweep(seed, 16, "time", n_az=450)


def labelled_cloud(seed, n=6000):
    """records of a labelled submap: a few thousand points, label in the payload"""
    import lisreg
    from lisreg import synth
    mc, ms = synth.make_submap(n, seed=seed, labelled=True)
    return lisreg.pack_device_records(cat_pcl(mc, ms))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- A: inputs produced late on the caller's stream ------------------------------------------------------------------------------
def a_pretreat(e, oracle):
    raw = sweep(11); n = len(raw)
    P = e.lisreg.default_pretreat_params(16)

    def make(dst):
        out, tm, it = e.D(np.zeros((n, 4), f32)), e.D(np.zeros(n, f32)), e.D(np.zeros(n, f32))

        def fetch(info):
            k = info["n"]
            return dict(info=info, rec=to_host(out.ptr, (n, 4))[:k], time=to_host(tm.ptr, (n,))[:k], inten=to_host(it.ptr, (n,))[:k])
        return (lambda: e.ctx.pretreat_device(dst.ptr, n, P, out.ptr, tm.ptr, n, it.ptr)), fetch
    o, _ = late_case(e, "pretreat_device", raw, moved(raw), make)
    r = PR.pretreat_vectorised(raw, 16, 0.0, 70.0)
    assert o["info"]["n"] == len(r["index"]) > 1000
    assert np.array_equal(bits(o["rec"][:, :3]), bits(r["xyzi"][:, :3])) and np.array_equal(bits(o["rec"][:, 3]), r["ring"].astype(np.uint32))
    assert np.array_equal(bits(o["inten"]), bits(r["xyzi"][:, 3])) and np.array_equal(bits(o["time"]), bits(r["time"]))
    assert bits(f32(o["info"]["start_ori"])) == bits(f32(r["start_ori"])) and bits(f32(o["info"]["end_ori"])) == bits(f32(r["end_ori"]))
    assert o["info"]["half_index"] == r["half_index"]


def _project_io(e, n, P):
    hw = P.img_h * P.img_w
    tensor, mask, pix = e.D(np.zeros(5 * hw, f32)), e.D(np.zeros(hw, np.uint8)), e.D(np.zeros(n, np.int32))

    def fetch(n_valid):
        return dict(n_valid=n_valid, tensor=to_host(tensor.ptr, (5, P.img_h, P.img_w)), invalid_mask=to_host(mask.ptr, (hw,), np.uint8),
                    pixel_index=to_host(pix.ptr, (n,), np.int32))
    return tensor, mask, pix, fetch


def _check_projection(o, ref):
    assert np.array_equal(o["pixel_index"], ref["pixel_index"]) and np.array_equal(o["invalid_mask"], ref["invalid_mask"])
    assert o["n_valid"] == ref["n_valid"] and np.array_equal(bits(o["tensor"]), bits(ref["tensor"]))


def a_rangenet_project(e, oracle):
    raw = sweep(12); n = len(raw)
    P = RR.Params(16, 128, 15.0, -15.0, MEANS, STDS, 20)

    def make(dst):
        tensor, mask, pix, fetch = _project_io(e, n, P)
        return (lambda: e.ctx.rangenet_project_device(dst.ptr, n, cparams(P), tensor.ptr, mask.ptr, pix.ptr)), fetch
    o, _ = late_case(e, "rangenet_project_device", raw, moved(raw), make)
    _check_projection(o, RR.project_parallel(raw, P))


def a_rangenet_label(e, oracle):
    """the logits arrive late: INTEGRATION.md section 3c"""
    raw = sweep(13); n = len(raw)
    P = RR.Params(16, 128, 15.0, -15.0, MEANS, STDS, 20)
    ref = RR.project_parallel(raw, P)
    din = e.D(raw)
    tensor, mask, pix, fetch_p = _project_io(e, n, P)
    _check_projection(fetch_p(e.ctx.rangenet_project_device(din.ptr, n, cparams(P), tensor.ptr, mask.ptr, pix.ptr)), ref)
    lg = [RR.stand_in_logits(ref["tensor"], P, seed)[0] for seed in (7001, 7002)]

    def make(dst):
        out, img = e.D(np.zeros((n, 4), f32)), e.D(np.zeros(P.img_h * P.img_w, np.uint8))
        return (lambda: e.ctx.rangenet_label_device(din.ptr, n, pix.ptr, mask.ptr, dst.ptr, cparams(P), out.ptr, img.ptr)), \
               (lambda _: dict(rec=to_host(out.ptr, (n, 4)), img=to_host(img.ptr, (P.img_h, P.img_w), np.uint8)))
    o, _ = late_case(e, "rangenet_label_device", lg[0], lg[1], make)
    want, want_img = RR.label_parallel(ref["pixel_index"], ref["invalid_mask"], lg[0], P)
    assert np.array_equal(bits(o["rec"][:, :3]), bits(raw[:, :3])) and np.array_equal(bits(o["rec"][:, 3]), want) and np.array_equal(o["img"], want_img)
    assert len(np.unique(want)) >= 3


def a_extract_features(e, oracle):
    """device records with a device time table (the de-skewed form)"""
    from lisreg import synth
    from test_features import _imu_tables
    c = synth.make_raw_scan(16, 450, 7301)
    rec = np.zeros((len(c), 4), f32)
    rec[:, 0], rec[:, 1], rec[:, 2] = c["x"], c["y"], c["z"]
    rec[:, 3] = c["ring"].astype(np.uint32).view(f32)
    n, cap = len(c), 16 * 450
    dt = e.D(np.ascontiguousarray(c["time"]))
    t, rot = _imu_tables(21)
    dk = e.lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0, time_device_ptr=dt.ptr)
    pg = e.lisreg.FeatureParams(16, 450, 1, 0.0, 70.0, 1.0, 0.1)

    def make(dst):
        outs = {k: e.D(np.zeros((cap, 4), f32)) for k in NAMES}
        return (lambda: e.ctx.extract_features_device(dst.ptr, n, pg, {k: v.ptr for k, v in outs.items()}, cap, dk)), \
               (lambda nd: dict(counts=nd, **{k: to_host(outs[k].ptr, (cap, 4))[: nd[k]] for k in NAMES}))
    o, _ = late_case(e, "extract_features_device", rec, moved(rec), make)
    ro = oracle.extract_features(c, oracle.FeatureParams(16, 450, 1, 0.0, 70.0, 1.0, 0.1))      # the selection does not depend on the de-skew
    host = e.ctx.extract_features(c, pg, e.lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0))
    for k in NAMES:
        assert o["counts"][k] == len(ro[k]) > 0, k
        assert np.array_equal(o[k][:, :3], synth.pcl_xyz(host[k])), k


def a_semantic_split(e, oracle):
    rec = labelled_cloud(31); n = len(rec)

    def make(dst):
        outs = [e.D(np.zeros((n, 4), f32)) for _ in range(5)]
        return (lambda: e.ctx.semantic_split_device(dst.ptr, n, [o.ptr for o in outs], n)), \
               (lambda cnt: dict(counts=cnt, clouds=[to_host(outs[k].ptr, (n, 4))[: cnt[k]] for k in range(5)]))
    o, _ = late_case(e, "semantic_split_device", rec, moved(rec, roll_payload=True), make)
    want = oracle.semantic_split(records_pcl(rec))
    assert o["counts"] == [len(w) for w in want] and sum(1 for k in o["counts"] if k > 0) >= 3
    for k in range(5):
        assert np.array_equal(bits(o["clouds"][k]), bits(e.lisreg.pack_device_records(want[k]))), k


def a_voxel(e, oracle):
    rec = labelled_cloud(32); n = len(rec)

    def make(dst):
        out = e.D(np.zeros((n, 4), f32))
        return (lambda: e.ctx.voxel_downsample_device(dst.ptr, n, 0.4, out.ptr, n)), (lambda r: dict(rc=r[0], n=r[1], rec=to_host(out.ptr, (n, 4))[: r[1]]))
    o, _ = late_case(e, "voxel_downsample_device", rec, moved(rec), make)
    _, do = oracle.voxel_grid(records_pcl(rec), 0.4)
    g = o["rec"]
    assert o["rc"] == 0 and 0 < o["n"] == len(do) < n
    assert np.array_equal(g[:, 0], do["x"]) and np.array_equal(g[:, 1], do["y"]) and np.array_equal(g[:, 2], do["z"])
    assert np.array_equal(bits(g[:, 3]) & 0xffff, do["label"].astype(np.uint32))


def a_voxel_multi(e, oracle):
    rec, other = labelled_cloud(33), labelled_cloud(34, 3001)
    n, m = len(rec), len(other)
    d_other = e.D(other)

    def make(dst):
        outs = [e.D(np.zeros((n, 4), f32)), e.D(np.zeros((m, 4), f32))]
        return (lambda: e.ctx.voxel_downsample_multi_device([dst.ptr, d_other.ptr], [n, m], [0.4, 0.2], [o.ptr for o in outs], [n, m])), \
               (lambda cnt: dict(counts=cnt, a=to_host(outs[0].ptr, (n, 4))[: cnt[0]], b=to_host(outs[1].ptr, (m, 4))[: cnt[1]]))
    o, od = late_case(e, "voxel_downsample_multi_device", rec, moved(rec), make)
    assert same(o["b"], od["b"])                                             # the cloud that was there all along
    for key, cloud, leaf in (("a", rec, 0.4), ("b", other, 0.2)):
        _, do = oracle.voxel_grid(records_pcl(cloud), leaf)
        g = o[key]
        assert len(g) == len(do) and np.array_equal(g[:, 0], do["x"]) and np.array_equal(g[:, 1], do["y"]) and np.array_equal(g[:, 2], do["z"])
        assert np.array_equal(bits(g[:, 3]) & 0xffff, do["label"].astype(np.uint32))


def a_transform(e, oracle):
    from lisreg import synth
    rec = labelled_cloud(35); n = len(rec)
    T = np.array([0.02, -0.01, -1.3, 12.0, -7.5, 0.25], f32)

    def make(dst):
        out = e.D(np.zeros((n, 4), f32))
        return (lambda: e.ctx.transform_cloud_device(dst.ptr, n, T, out.ptr)), (lambda _: dict(rec=to_host(out.ptr, (n, 4))))
    o, _ = late_case(e, "transform_cloud_device", rec, moved(rec), make)
    want = oracle.transform_cloud(records_pcl(rec), T)
    assert np.abs(o["rec"][:, :3] - synth.pcl_xyz(want)).max() <= 8e-6                           # FMA contraction only (tests/test_voxel.py)
    assert np.array_equal(bits(o["rec"][:, 3]), bits(rec[:, 3]))


def a_concat(e, oracle):
    parts = [labelled_cloud(36, 2001), labelled_cloud(37, 3003), labelled_cloud(38, 1000)]
    cnt = [len(p) for p in parts]
    d0, d2 = e.D(parts[0]), e.D(parts[2])

    def make(dst):
        out = e.D(np.zeros((sum(cnt), 4), f32))
        return (lambda: e.ctx.concat_device([d0.ptr, dst.ptr, d2.ptr], cnt, out.ptr)), (lambda tot: dict(tot=tot, rec=to_host(out.ptr, (sum(cnt), 4))))
    o, _ = late_case(e, "concat_device", parts[1], moved(parts[1]), make)
    assert o["tot"] == sum(cnt) and np.array_equal(bits(o["rec"]), bits(np.concatenate(parts)))


def a_bbx(e, oracle):
    rec = labelled_cloud(39); n = len(rec)
    box = np.array([-10.0, -12.0, -2.0, 15.0, 12.0, 10.0])

    def make(dst):
        out = e.D(np.zeros((n, 4), f32))
        return (lambda: e.ctx.bbx_filter_device(dst.ptr, n, box, False, out.ptr)), (lambda k: dict(n=k, rec=to_host(out.ptr, (n, 4))[:k]))
    o, _ = late_case(e, "bbx_filter_device", rec, moved(rec), make)
    want = oracle.bbx_filter(records_pcl(rec), box)
    assert 0 < o["n"] == len(want) < n and np.array_equal(bits(o["rec"]), bits(e.lisreg.pack_device_records(want)))


def _scene_records(e, seed):
    from test_mapfilter import _scene
    m, q = _scene(seed, n_map=4000)
    q = q[:3000].copy()
    return m, q, e.lisreg.pack_device_records(m), e.lisreg.pack_device_records(q)


def a_map_index_nearest(e, oracle):
    """the MAP arrives late: lisreg_map_index_set only references device records, its build reads them in stream order"""
    m, q, rm, rq = _scene_records(e, 41)
    dq = e.D(rq)

    def make(dst):
        idx, sqd = e.D(np.zeros(len(rq), np.int32)), e.D(np.zeros(len(rq), f32))

        def run():
            e.ctx.map_index_set_device(11, dst.ptr, len(rm))
            e.ctx.nearest_device(11, dq.ptr, len(rq), 1e18, idx.ptr, sqd.ptr)
        return run, (lambda _: dict(idx=to_host(idx.ptr, (len(rq),), np.int32), sqd=to_host(sqd.ptr, (len(rq),))))
    o, _ = late_case(e, "map_index_set_device + nearest_device", rm, moved(rm, small=True), make)
    o_idx, o_d2 = oracle.nearest(m, q)
    assert np.array_equal(o["sqd"], o_d2) and (o["idx"] == o_idx).mean() > 0.999                 # ties may differ (tests/test_mapfilter.py)


def a_dynamic_filter(e, oracle):
    m, q, rm, rq = _scene_records(e, 42)
    dm = e.D(rm)
    e.ctx.map_index_set_device(12, dm.ptr, len(rm))

    def make(dst):
        out = e.D(np.zeros_like(rq))
        return (lambda: e.ctx.dynamic_filter_device(12, dst.ptr, len(rq), 30.0, 0.3, 1.0, 0.05, out.ptr)), \
               (lambda k: dict(n=k, rec=to_host(out.ptr, rq.shape)[:k]))
    o, _ = late_case(e, "dynamic_filter_device", rq, moved(rq, small=True), make)
    want, _ = oracle.dynamic_filter(m, q, 30.0, 0.3, 1.0, 0.05)
    assert 0 < o["n"] == len(want) < len(rq) and np.array_equal(bits(o["rec"]), bits(e.lisreg.pack_device_records(want)))


def a_icp(e, oracle):
    from test_icp import _case, _check
    tgt, src, _ = _case(55, n_map=8000, hw=(16, 300))
    rs = e.lisreg.pack_device_records(src)
    e.ctx.map_index_set(13, tgt)
    pg = e.lisreg.icp_default_params(0)

    def make(dst):
        out = e.D(np.zeros_like(rs))
        return (lambda: e.ctx.icp_align_device(13, dst.ptr, len(rs), pg, out_ptr=out.ptr)), (lambda r: dict(res=r, aligned=to_host(out.ptr, rs.shape)))
    o, _ = late_case(e, "icp_align_device", rs, moved(rs, small=True), make)
    ro = oracle.icp_align(tgt, src, oracle.icp_default_params(0))
    _check(o["res"], ro)                                  # state, pose within 1e-3 m / 1e-3 rad, fitness, n_corr_last (tests/test_icp.py)
    assert o["res"]["iters"] == ro["iters"]


def _reg_case(seed=1000):
    from lisreg import synth
    return synth.make_case(h=16, w=300, m_points=8000, scan_seed=seed)


def a_set_target_align(e, oracle):
    """the TARGET's surface cloud arrives late: set_target on device records references them, its index build reads them in stream order"""
    from helpers import copy_params, pose_err
    case = _reg_case()
    pk = e.lisreg.pack_device_records
    tc, ts, sc, ss = (pk(case[k]) for k in ("tgt_corner", "tgt_surf", "src_corner", "src_surf"))
    dtc, dsc, dss = e.D(tc), e.D(sc), e.D(ss)
    p_o = oracle.default_params(1); p = copy_params(p_o, e.lisreg.Params)

    def make(dst):
        def run():
            e.ctx.set_target_device(dtc.ptr, len(tc), dst.ptr, len(ts))           # slot 0: the one lisreg_align registers against
            return e.ctx.align_device(dsc.ptr, len(sc), dss.ptr, len(ss), case["T_init"], p)
        return run, (lambda r: dict(T=r[0], stats=r[1]))
    o, _ = late_case(e, "set_target_device + align_device", ts, moved(ts, small=True), make)
    To, so, _ = oracle.align(case["tgt_corner"], case["tgt_surf"], case["src_corner"], case["src_surf"], case["T_init"], p_o)
    rot, tr = pose_err(o["T"], To)
    assert rot <= 1e-3 and tr <= 1e-3 and o["stats"]["status"] == 0 and o["stats"]["iters"] == so["iters"]
    assert o["stats"]["n_corr_last"] == so["n_corr_last"]


def _target_bits(ctx, slot):
    out = {}
    for kind in (0, 1):
        t = ctx.target_index(slot, kind)
        out[kind] = dict(n=t["n"], dims=(t["nx"], t["ny"], t["nz"]), sorted=t["sorted"], cell_start=t["cell_start"])
    return out


def a_keyframes(e, oracle):
    """no CPU reference in this form: compared with the same calls on the idle own stream.  Every run takes a ring of its own: resetting a
    ring that holds a frame frees the frame's buffer, and hipFree waits for the whole device — the control run's stall would be spent on
    the host before the first kernel of the call reads anything."""
    import itertools
    rings = itertools.count(40)
    case = _reg_case(1001)
    sc, ss = (e.lisreg.pack_device_records(case[k]) for k in ("src_corner", "src_surf"))
    dsc = e.D(sc)
    pose = np.array([0.01, -0.02, 0.3, 1.0, -0.5, 0.02], f32)

    def make(dst):
        def run():
            ring = next(rings)
            e.ctx.keyframes_reset(ring)
            a = e.ctx.keyframes_push_device(ring, dsc.ptr, len(sc), dst.ptr, len(ss), pose)
            return a, e.ctx.keyframes_target(ring, 0.2, 0.4, target_slot=5)
        return run, (lambda r: dict(info=r, target=_target_bits(e.ctx, 5)))
    o, _ = late_case(e, "keyframes_push_device + keyframes_target", ss, moved(ss), make)
    assert o["info"][1]["n_target_surf"] > 100 and o["info"][1]["n_target_corner"] > 0


def _classes(e, seed):
    """five class clouds in map order (dynamic, pole, ground, building, outlier) as device records"""
    parts = e.ctx.semantic_split(records_pcl(labelled_cloud(seed, 8000)))
    return [e.lisreg.pack_device_records(parts[k]) for k in (0, 3, 1, 2, 4)]


def a_localmap(e, oracle):
    """no CPU reference in this form: compared with the same calls on the idle own stream"""
    cls = _classes(e, 51)
    late = max(range(5), key=lambda k: len(cls[k]))
    dev = [e.D(c if len(c) else np.zeros((1, 4), f32)) for c in cls]
    lm = e.lisreg.localmap_default_params()
    pose = np.array([0, 0, 0.01, 0.2, -0.1, 0.0], f32)

    def make(dst):
        def run():
            e.ctx.localmap_reset(4)
            ptrs = [dst.ptr if k == late else dev[k].ptr for k in range(5)]
            a = e.ctx.localmap_insert_device(4, ptrs, [len(c) for c in cls], pose, lm)
            return a, e.ctx.localmap_extract(4, pose, lm, target_slot=6)
        return run, (lambda r: dict(info=r, corner=e.ctx.localmap_get(4, 5), surf=e.ctx.localmap_get(4, 6), target=_target_bits(e.ctx, 6)))
    o, _ = late_case(e, "localmap_insert_device + localmap_extract", cls[late], moved(cls[late], small=True), make)
    assert o["info"][1]["n_target_surf"] + o["info"][1]["n_target_corner"] > 500


def a_submap(e, oracle):
    cls = _classes(e, 52)
    late = max(range(5), key=lambda k: len(cls[k]))
    dev = [e.D(c if len(c) else np.zeros((1, 4), f32)) for c in cls]
    total = sum(len(c) for c in cls)
    prm = e.lisreg.localmap_default_params()
    poses = GR.agreed_poses(np.random.default_rng(5), 1)

    def make(dst):
        out = e.D(np.zeros((total, 4), f32))

        def run():
            e.ctx.localmap_reset(21)
            ptrs = [dst.ptr if k == late else dev[k].ptr for k in range(5)]
            a = e.ctx.submap_insert_device(21, ptrs, [len(c) for c in cls], None, ZERO_POSE, prm)
            n, off = e.ctx.submap_gather_device([21], poses, out.ptr, total)
            return a["n"], n, off
        return run, (lambda r: dict(counts=r[0], n=r[1], off=r[2], rec=to_host(out.ptr, (total, 4))[: r[1]]))
    o, _ = late_case(e, "submap_insert_device + submap_gather_device", cls[late], moved(cls[late]), make)
    want, off = GR.global_map({21: cls}, [21], poses, 31)
    assert o["n"] == total == len(want) and np.array_equal(o["off"], off) and GR.same_bits(o["rec"], want) is None


def _batch(e, n_items=4, seed0=2000, m_points=8000):
    """n_items registrations of 16 x 300 scans against one 8000-point submap: (cases, device records, items, T0)"""
    from lisreg import synth
    cases = [synth.make_case(h=16, w=300, m_points=m_points, scan_seed=seed0 + i) for i in range(n_items)]
    pk = e.lisreg.pack_device_records
    recs = [(e.D(pk(c["src_corner"])), e.D(pk(c["src_surf"]))) for c in cases]
    items = [dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0], target=0) for a, b in recs]
    return cases, recs, items, np.array([c["T_init"] for c in cases], f32)


def a_batch(e, oracle):
    from helpers import copy_params, pose_err
    cases, recs, items, T0 = _batch(e)
    e.ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"], slot=0)
    p_o = oracle.default_params(1); p = copy_params(p_o, e.lisreg.Params)
    surf2 = e.lisreg.pack_device_records(cases[2]["src_surf"])

    def make(dst):
        its = [dict(it) for it in items]
        its[2]["surf_ptr"] = dst.ptr

        def run():
            e.ctx.batch_prepare_device(its, T0, p)
            e.ctx.batch_run()
            return e.ctx.batch_fetch()
        return run, (lambda r: dict(T=r[0], stats=r[1]))
    o, od = late_case(e, "batch_prepare_device / batch_run / batch_fetch", surf2, moved(surf2, small=True), make)
    assert same(o["T"][[0, 1, 3]], od["T"][[0, 1, 3]])                         # the items whose inputs were there all along
    c = cases[2]
    To, so, _ = oracle.align(cases[0]["tgt_corner"], cases[0]["tgt_surf"], c["src_corner"], c["src_surf"], c["T_init"], p_o)
    rot, tr = pose_err(o["T"][2], To)
    assert rot <= 1e-3 and tr <= 1e-3 and o["stats"][2]["iters"] == so["iters"] and o["stats"][2]["n_corr_last"] == so["n_corr_last"]


A_CASES = dict(pretreat_device=a_pretreat, rangenet_project_device=a_rangenet_project, rangenet_label_device=a_rangenet_label,
               extract_features_device=a_extract_features, semantic_split_device=a_semantic_split, voxel_downsample_device=a_voxel,
               voxel_downsample_multi_device=a_voxel_multi, transform_cloud_device=a_transform, concat_device=a_concat,
               bbx_filter_device=a_bbx, map_index_set_device_nearest_device=a_map_index_nearest, dynamic_filter_device=a_dynamic_filter,
               icp_align_device=a_icp, set_target_device_align_device=a_set_target_align, keyframes_push_device_keyframes_target=a_keyframes,
               localmap_insert_device_localmap_extract=a_localmap, submap_insert_device_submap_gather_device=a_submap,
               batch_prepare_device_run_fetch=a_batch)


@pytest.mark.parametrize("entry", list(A_CASES))
def test_late_input_on_the_callers_stream(env, oracle, entry):
    try:
        A_CASES[entry](env, oracle)
    finally:
        env.ctx.set_stream(None)
        settle(env)


# ---- B: outputs consumed on the caller's stream; calls that must not wait -----------------------------------------------------------
def consume_on_stream(e, name, call, out_ptr_of, nbytes, poison=True):
    """call() once on the idle stream (reference bytes), then on S behind a stall: when it returns, an event recorded behind the stall
    is still pending; the output is copied to a snapshot ON S with no host wait in between.  Returns (idle bytes, snapshot bytes)."""
    gate, ctx, S = e.gate, e.ctx, e.S
    call(); gate.stream_sync(ctx.stream); settle(e)                          # warm-up
    ms = stall_for(e, call)
    gate.stream_sync(ctx.stream); settle(e)
    want = to_host(out_ptr_of(), (nbytes,), np.uint8)
    if poison:                                                               # (not the library's own result block)
        e.hip.hipMemset(C.c_void_p(out_ptr_of()), 0xA5, C.c_size_t(nbytes)); settle(e)
    snap = e.D(np.zeros(nbytes, np.uint8))
    ctx.set_stream(S)
    try:
        gate.stall(S, ms)
        ev = gate.mark(S)
        call()
        pending = gate.event_pending(ev)
        gate.copy_async(snap.ptr, out_ptr_of(), nbytes, S)
        gate.stream_sync(S)
        gate.event_destroy(ev)
    finally:
        ctx.set_stream(None)
    settle(e)
    print(f"[caller_stream] {name}: stall {ms:.2f} ms, pending when the call returned: {pending}")
    assert pending, (name, "the call waited for the GPU: the stall queued in front of it had finished when it returned")
    return want, to_host(snap.ptr, (nbytes,), np.uint8)


def test_concat_device_does_not_wait_and_feeds_the_stream(env):
    e = env
    parts = [labelled_cloud(61, 2001), labelled_cloud(62, 3003), labelled_cloud(63, 1000)]
    devs = [e.D(p) for p in parts]
    cnt = [len(p) for p in parts]
    out = e.D(np.zeros((sum(cnt), 4), f32))
    try:
        want, snap = consume_on_stream(e, "concat_device", lambda: e.ctx.concat_device([d.ptr for d in devs], cnt, out.ptr), lambda: out.ptr, out.nbytes)
    finally:
        e.ctx.set_stream(None)
    ref = np.concatenate(parts).view(np.uint8).ravel()
    assert np.array_equal(want, ref) and np.array_equal(snap, ref)


def _install_submaps(e, ids, seed):
    rng = np.random.default_rng(seed)
    store = GR.make_store(rng, {int(m): rng.integers(200, 1500, 5) for m in ids})
    prm = e.lisreg.localmap_default_params()
    for mid, cls in store.items():
        e.ctx.localmap_reset(mid)
        dev = [e.D(c) for c in cls]
        e.ctx.submap_insert_device(mid, [d.ptr for d in dev], [len(c) for c in cls], None, ZERO_POSE, prm)
        settle(e)
        for d in dev:
            d.free()
    return store


def test_submap_gather_device_does_not_wait_and_feeds_the_stream(env):
    e = env
    ids = [31, 32, 33]
    store = _install_submaps(e, ids, 71)
    poses = GR.agreed_poses(np.random.default_rng(72), len(ids))
    want_cloud, want_off = GR.global_map(store, ids, poses, 31)
    out = e.D(np.zeros((len(want_cloud), 4), f32))
    got = {}

    def call():
        got["n"], got["off"] = e.ctx.submap_gather_device(ids, poses, out.ptr, len(want_cloud))
    try:
        want, snap = consume_on_stream(e, "submap_gather_device", call, lambda: out.ptr, out.nbytes)
    finally:
        e.ctx.set_stream(None)
    assert got["n"] == len(want_cloud) and np.array_equal(got["off"], want_off)
    assert np.array_equal(want, snap) and GR.same_bits(snap.view(f32).reshape(-1, 4), want_cloud) is None


BATCH_RUN_WAYS = dict(plain={}, interleave_1=dict(interleave=1, interleave_min_blocks=2), interleave_2=dict(interleave=2, interleave_min_blocks=2),
                      rebuild_front_end_5=dict(rebuild_targets_each_run=1, search_mode=5))


@pytest.mark.parametrize("way", list(BATCH_RUN_WAYS))
def test_batch_run_does_not_synchronise_and_feeds_the_stream(env, way):
    """lisreg_batch_run behind a stall: it returns with the stall pending, the result block is copied on S, and block, snapshot and
    lisreg_batch_fetch agree with the same prepared batch run on the idle own stream — plain, with the batch split into interleaved halves
    (both forms: the halves fork from and join the context's stream) and with the targets rebuilt inside the run in front-end 5."""
    e = SimpleNamespace(**{**vars(env), "ctx": env.lisreg.Context(0)})        # a context of its own: its options end with it
    ctx = e.ctx
    cases, recs, items, T0 = _batch(e)
    p = e.lisreg.default_params(1); p.fixed_iters = 6
    try:
        for k, v in BATCH_RUN_WAYS[way].items():
            ctx.set_option(k, v)
        if way.startswith("interleave"):
            ctx.set_option("lanes_per_query", 1)       # (a small batch would take eight lanes per query: those are not interleaved)
        ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"], slot=0)
        ctx.batch_prepare_device(items, T0, p)
        ctx.batch_run(); T_idle, st_idle = ctx.batch_fetch()
        if "search_mode" in BATCH_RUN_WAYS[way]:
            assert ctx.front_end() == 5
        assert ctx.get_option("interleaved_now") == (1 if way.startswith("interleave") else 0), "the 4-item batch was not split"
        want, snap = consume_on_stream(e, f"batch_run ({way})", ctx.batch_run, lambda: ctx.result_device_ptr, 4 * 12 * len(items), poison=False)
        ctx.set_stream(e.S)
        T, st = ctx.batch_fetch()
    finally:
        ctx.set_stream(None)
        settle(e)
        ctx.close()
    assert np.array_equal(want, snap), way
    block = snap.view(f32).reshape(len(items), 12)
    assert np.array_equal(bits(block[:, :6]), bits(T)) and np.array_equal(bits(T), bits(T_idle)) and st == st_idle, way
    assert [int(v) for v in block[:, 6]] == [s["iters"] for s in st] == [6] * len(items)


def _big_target(seed, n=2_100_000):
    """2.1 M points: uniform over 80 m x 80 m x 3 m, one in thirty of them in one thin x-slab (strips beyond the LDS capacity of the
    small-strip variant: the big-strip variant, the one on the side stream, has work); the first two points pin the bounding box, so
    that two such clouds share one grid"""
    rng = np.random.default_rng(seed)
    big = np.zeros((n, 4), f32)
    big[:, :2] = rng.uniform(-40, 40, (n, 2)); big[:, 2] = rng.uniform(0, 3, n)
    k = n // 30
    big[2:2 + k, 0] = 3.0 + rng.uniform(0, 0.2, k); big[2:2 + k, 1] = rng.uniform(-30, 30, k)
    big[0, :3], big[1, :3] = (-40.0, -40.0, 0.0), (40.0, 40.0, 3.0)
    return big


def test_strip_build_side_stream_forks_from_the_busy_stream(env):
    """The strip form of the index build runs its big-strip variant on a side stream when the batch's targets make >= 512 chunks of 4096
    points: the build inside lisreg_batch_run ("rebuild_targets_each_run") of a 2.1 M-point target of device records.  The TARGET
    arrives late on S (another cloud in the same bounding box: the slot's grid stays as it was set), the run rebuilds the index from
    it, and the strip tables still hold the previous build of the decoy: a side stream forked ahead of the late copy, or not joined,
    leaves the decoy's records in the index.  Ordered run = the idle build of the real target, control run = the decoy's."""
    e = SimpleNamespace(**{**vars(env), "ctx": env.lisreg.Context(0)})        # a context of its own: its options end with it
    ctx = e.ctx
    real, decoy = _big_target(81), _big_target(82)
    case = _reg_case(1002)
    pk = e.lisreg.pack_device_records
    dtc, dsc, dss = e.D(pk(case["tgt_corner"])), e.D(pk(case["src_corner"])), e.D(pk(case["src_surf"]))
    items = [dict(corner_ptr=dsc.ptr, n_corner=dsc.shape[0], surf_ptr=dss.ptr, n_surf=dss.shape[0], target=7)]
    p = e.lisreg.default_params(1); p.fixed_iters = 1
    T0 = np.asarray(case["T_init"], f32)[None]

    def make(dst):
        ctx.set_target_device(dtc.ptr, dtc.shape[0], dst.ptr, len(real), slot=7)
        ctx.set_option("rebuild_targets_each_run", 1)
        ctx.batch_prepare_device(items, T0, p)
        assert ctx.get_option("index_build_now") == 1, "the batch did not choose the strip form"
        assert (len(real) + 4095) // 4096 >= 512

        def run():
            ctx.batch_run()
            return ctx.batch_fetch()
        return run, (lambda r: dict(T=r[0], index=_target_bits(ctx, 7)[1]))
    try:
        o, od = late_case(e, "batch_run rebuilding a 2.1 M-point target (strip build, side stream)", real, decoy, make)
    finally:
        ctx.set_stream(None)
        settle(e)
        ctx.close()
    assert o["index"]["n"] == len(real) and o["index"]["dims"] == od["index"]["dims"]
    order = o["index"]["sorted"][:, 3].copy().view(np.int32)                  # records by (cell, original index): a permutation of the real cloud
    assert np.array_equal(np.sort(order), np.arange(len(real))) and np.array_equal(o["index"]["sorted"][:, :3], real[order, :3])
    for a in (dtc, dsc, dss):
        a.free()


@pytest.mark.parametrize("interleave", [1, 2])
def test_interleaved_halves_fork_from_the_busy_stream(env, oracle, interleave):
    """"interleave" 1 / 2 with "interleave_min_blocks" = 2: a 4-item batch runs as two halves, the second on a side stream forked from
    the context's.  The surf source of an item of the SECOND half arrives late on S, and the batch has just run on the decoy: a side
    stream that forks ahead of the late copy, or is not joined before the results are read, gives the decoy's pose for that item."""
    from helpers import copy_params, pose_err
    e = SimpleNamespace(**{**vars(env), "ctx": env.lisreg.Context(0)})
    ctx = e.ctx
    cases, recs, items, T0 = _batch(e, seed0=2600)
    p_o = oracle.default_params(1); p_o.fixed_iters = 6
    p = copy_params(p_o, e.lisreg.Params)
    surf3 = e.lisreg.pack_device_records(cases[3]["src_surf"])

    def make(dst):
        its = [dict(it) for it in items]
        its[3]["surf_ptr"] = dst.ptr

        def run():
            ctx.batch_prepare_device(its, T0, p)
            ctx.batch_run()
            assert ctx.get_option("interleaved_now") == 1, "the 4-item batch was not split"
            return ctx.batch_fetch()
        return run, (lambda r: dict(T=r[0], stats=r[1]))
    try:
        ctx.set_option("lanes_per_query", 1)           # (a small batch would take eight lanes per query: those are not interleaved)
        ctx.set_option("interleave", interleave); ctx.set_option("interleave_min_blocks", 2)
        ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"], slot=0)
        o, od = late_case(e, f"batch_run, interleave {interleave}", surf3, moved(surf3, small=True), make)
    finally:
        ctx.set_stream(None)
        settle(e)
        ctx.close()
    assert same(o["T"][:3], od["T"][:3]) and not same(o["T"][3], od["T"][3])
    c = cases[3]
    To, so, _ = oracle.align(cases[0]["tgt_corner"], cases[0]["tgt_surf"], c["src_corner"], c["src_surf"], c["T_init"], p_o)
    rot, tr = pose_err(o["T"][3], To)
    assert rot <= 1e-3 and tr <= 1e-3 and o["stats"][3]["iters"] == so["iters"] == 6 and o["stats"][3]["n_corr_last"] == so["n_corr_last"]


# ---- C: several calls queued behind one stall ------------------------------------------------------------------------------------
def test_two_batches_behind_one_stall(env):
    """stall; prepare(A); run(A); snapshot A; prepare(B); run(B); fetch — different sources, initial poses and target slots: prepare(B)
    re-fills the host staging of the item tables and grids while A's copies of them have not run."""
    e = env
    ctx, gate, S = e.ctx, e.gate, e.S
    cases, recs, items, T0 = _batch(e, 8, seed0=2100)
    p = e.lisreg.default_params(1); p.fixed_iters = 5
    for slot, c in ((0, cases[0]), (1, cases[5])):
        ctx.set_target(c["tgt_corner"], c["tgt_surf"], slot=slot)
    A = ([dict(it, target=0) for it in items[:4]], T0[:4])
    B = ([dict(it, target=1) for it in items[4:][::-1]], T0[4:][::-1] + f32(0.01))
    snap = e.D(np.zeros((4, 12), f32))

    def both(stalled):
        if stalled:
            gate.stall(S, ms)
            ev = gate.mark(S)
        ctx.batch_prepare_device(*A, p); ctx.batch_run()
        gate.copy_async(snap.ptr, ctx.result_device_ptr, 4 * 48, ctx.stream)
        ctx.batch_prepare_device(*B, p); ctx.batch_run()
        pending = gate.event_pending(ev) if stalled else None
        TB = ctx.batch_fetch()
        if stalled:
            gate.event_destroy(ev)
        settle(e)
        return to_host(snap.ptr, (4, 12)), TB, pending
    try:
        both(False)                                                            # warm-up: no reallocation inside prepare afterwards
        snap_idle, TB_idle, _ = both(False)
        ms = stall_for(e, lambda: both(False))
        ctx.batch_prepare_device(*A, p); ctx.batch_run(); TA_alone = ctx.batch_fetch()
        ctx.set_stream(S)
        snap_busy, TB_busy, pending = both(True)
    finally:
        ctx.set_stream(None)
    assert np.array_equal(bits(snap_idle[:, :6]), bits(TA_alone[0]))
    print(f"[caller_stream] two batches: stall {ms:.2f} ms, still pending when run(B) returned: {pending} (prepare may wait for its staging)")
    assert np.array_equal(bits(snap_busy), bits(snap_idle)) and same(TB_busy, TB_idle)
    assert not np.array_equal(bits(snap_busy[:, :6]), bits(TB_busy[0]))


def test_two_gathers_behind_one_stall(env):
    e = env
    ctx, gate, S = e.ctx, e.gate, e.S
    store = _install_submaps(e, [41, 42, 43, 44], 91)
    lists = ([41, 43, 44], [44, 42])
    poses = [GR.agreed_poses(np.random.default_rng(92 + k), len(ids)) for k, ids in enumerate(lists)]
    wants = [GR.global_map(store, ids, ps, 31)[0] for ids, ps in zip(lists, poses)]
    outs = [e.D(np.zeros((len(w), 4), f32)) for w in wants]

    def both():
        for ids, ps, o, w in zip(lists, poses, outs, wants):
            assert ctx.submap_gather_device(ids, ps, o.ptr, len(w))[0] == len(w)
    try:
        both(); settle(e)
        ms = stall_for(e, both)
        for o in outs:
            e.hip.hipMemset(C.c_void_p(o.ptr), 0, C.c_size_t(o.nbytes))
        settle(e)
        ctx.set_stream(S)
        gate.stall(S, ms)
        ev = gate.mark(S)
        both()
        assert gate.event_pending(ev), "a gather into device memory waited for the GPU"
        gate.stream_sync(S)
        gate.event_destroy(ev)
    finally:
        ctx.set_stream(None)
    settle(e)
    for o, w in zip(outs, wants):
        assert GR.same_bits(to_host(o.ptr, (len(w), 4)), w) is None


def test_two_sweep_batches_behind_one_stall(env):
    """two lisreg_pretreat_batch calls and two lisreg_rangenet_project_batch calls with different sweep tables (pt_tab / rn_tab), the
    first of each queued behind a stall: every sweep equals the CPU restatement"""
    e = env
    ctx, gate, S = e.ctx, e.gate, e.S
    P = RR.Params(16, 128, 15.0, -15.0, MEANS, STDS, 20)
    hw = 16 * 128
    groups = [[sweep(101), sweep(102)], [sweep(103), sweep(104), sweep(105)]]
    cap = max(len(r) for g in groups for r in g)
    PP = e.lisreg.default_pretreat_params(16)
    dev = [[SimpleNamespace(raw=r, n=len(r), din=e.D(r), out=e.D(np.zeros((cap, 4), f32)), tm=e.D(np.zeros(cap, f32)), mask=e.D(np.zeros(hw, np.uint8)),
                            pix=e.D(np.zeros(cap, np.int32))) for r in g] for g in groups]
    tensors = [e.D(np.zeros(len(g) * 5 * hw, f32)) for g in groups]

    def all_calls(stalled):
        if stalled:
            gate.stall(S, ms)
        pre = [ctx.pretreat_batch_device([d.din.ptr for d in g], [d.n for d in g], PP, [d.out.ptr for d in g], [d.tm.ptr for d in g], cap) for g in dev]
        if stalled:
            gate.stall(S, ms)
        prj = [ctx.rangenet_project_batch_device([d.din.ptr for d in g], [d.n for d in g], cparams(P), t.ptr, [d.mask.ptr for d in g], [d.pix.ptr for d in g])
               for g, t in zip(dev, tensors)]
        return pre, prj
    try:
        all_calls(False)
        ms = stall_for(e, lambda: all_calls(False))
        ctx.set_stream(S)
        pre, prj = all_calls(True)
        gate.stream_sync(S)
    finally:
        ctx.set_stream(None)
    settle(e)
    for g, infos, nv, t in zip(dev, pre, prj, tensors):
        tens = to_host(t.ptr, (len(g), 5, 16, 128))
        for s, d in enumerate(g):
            r = PR.pretreat_vectorised(d.raw, 16, 0.0, 70.0)
            k = infos[s]["n"]
            assert k == len(r["index"]) and np.array_equal(bits(to_host(d.out.ptr, (cap, 4))[:k, :3]), bits(r["xyzi"][:, :3]))
            assert np.array_equal(bits(to_host(d.tm.ptr, (cap,))[:k]), bits(r["time"])) and infos[s]["half_index"] == r["half_index"]
            ref = RR.project_parallel(d.raw, P)
            _check_projection(dict(n_valid=nv[s], tensor=tens[s], invalid_mask=to_host(d.mask.ptr, (hw,), np.uint8),
                                   pixel_index=to_host(d.pix.ptr, (cap,), np.int32)[: d.n]), ref)


def test_staging_next_batch_while_the_run_is_stalled(env):
    """the header's loop stage(k+1); fetch(k); prepare(k+1); run(k+1) for three batches of pinned host clouds, run(0) held back by a stall:
    stage(1) fills the second feeder buffer while the first has not been read, every batch fetches its own unstalled result"""
    e = env
    ctx, gate, S, L = e.ctx, e.gate, e.S, e.ctx._L
    from lisreg import synth
    n = 4
    p = e.lisreg.default_params(1); p.fixed_iters = 4
    fp = C.POINTER(C.c_float)
    batches = []
    for b in range(3):
        cases = [synth.make_case(h=16, w=300, m_points=8000, scan_seed=2300 + 10 * b + i) for i in range(n)]
        pins = [(e.lisreg.PinnedArray(c["src_corner"]), e.lisreg.PinnedArray(c["src_surf"])) for c in cases]
        arr = (e.lisreg.Item * n)()
        for i, (c, (pc, ps)) in enumerate(zip(cases, pins)):
            arr[i].src_corner, arr[i].n_corner, arr[i].src_surf, arr[i].n_surf = C.c_void_p(pc.ptr), len(c["src_corner"]), C.c_void_p(ps.ptr), len(c["src_surf"])
            arr[i].stride_bytes, arr[i].fmt = c["src_corner"].dtype.itemsize, e.lisreg.FMT_XYZI
        batches.append(SimpleNamespace(cases=cases, pins=pins, arr=arr, staged=(e.lisreg.Item * n)(), T0=np.array([c["T_init"] for c in cases], f32)))
    ctx.set_target(batches[0].cases[0]["tgt_corner"], batches[0].cases[0]["tgt_surf"], slot=0)
    ctx._n_items = n

    def stage(b): assert L.lisreg_stage_host_items(ctx._h, n, b.arr, b.staged) == 0
    def launch(b):
        assert L.lisreg_batch_prepare(ctx._h, n, b.staged, C.byref(p), b.T0.ctypes.data_as(fp)) == 0
        assert L.lisreg_batch_run(ctx._h) == 0

    def loop(stalled):
        out = []
        stage(batches[0])
        if stalled:
            gate.stall(S, ms)
        launch(batches[0])
        for k in (1, 2):
            stage(batches[k]); out.append(ctx.batch_fetch()); launch(batches[k])
        out.append(ctx.batch_fetch())
        return out
    try:
        want = [ctx.align_batch([dict(src_corner=c["src_corner"], src_surf=c["src_surf"]) for c in b.cases], b.T0, p) for b in batches]
        loop(False)
        idle = loop(False)
        ms = stall_for(e, lambda: loop(False))
        ctx.set_stream(S)
        busy = loop(True)
    finally:
        ctx.set_stream(None)
    settle(e)
    for k in range(3):
        assert same(idle[k], want[k]) and same(busy[k], want[k]), k
    assert not same(want[0][0], want[1][0])
    for b in batches:
        for pc, ps in b.pins:
            pc.free(); ps.free()


_FEEDER_CASES = []


def _feeder_cases():
    from lisreg import synth
    if not _FEEDER_CASES:
        _FEEDER_CASES.extend(synth.make_case(h=64, w=900, m_points=40000, scan_seed=3500 + i) for i in range(6))
    return _FEEDER_CASES


@pytest.mark.parametrize("engine", [3, 0])
def test_threaded_staging_while_the_run_is_stalled(env, engine):
    """The same loop at the size where the feeder really runs (>= 262144 source points: packing threads; with "feeder_copy_engine" = 3
    also the pack stream and chunks the copy engine takes from the caller's pinned clouds), two batches alternating over both feeder
    buffers, run(0) held back by a stall.  The third stage meets the guards of buffer 0, and every fetch is the bits of
    lisreg_align_batch on the idle stream.  With the packing threads alone (0) stage(1) returns with the stall still pending: the upload
    goes underneath the queued run.  With chunks forced onto the copy engine (3) the call waits, by design, until the engine has read
    the caller's memory, and that event lies behind a packing kernel whose hardware queue may be the stalled stream's: results only."""
    e = SimpleNamespace(**{**vars(env), "ctx": env.lisreg.Context(0)})        # a context of its own: its options end with it
    ctx, gate, S, L = e.ctx, e.gate, e.S, e.ctx._L
    cases = _feeder_cases()
    n = len(cases)
    assert sum(len(c["src_corner"]) + len(c["src_surf"]) for c in cases) >= 262144
    p = e.lisreg.default_params(1); p.fixed_iters = 4
    fp = C.POINTER(C.c_float)
    pins = [(e.lisreg.PinnedArray(c["src_corner"]), e.lisreg.PinnedArray(c["src_surf"])) for c in cases]
    T0 = np.array([c["T_init"] for c in cases], f32)

    def batch(order):
        arr = (e.lisreg.Item * n)()
        for i, k in enumerate(order):
            c, (pc, ps) = cases[k], pins[k]
            arr[i].src_corner, arr[i].n_corner, arr[i].src_surf, arr[i].n_surf = C.c_void_p(pc.ptr), len(c["src_corner"]), C.c_void_p(ps.ptr), len(c["src_surf"])
            arr[i].stride_bytes, arr[i].fmt = c["src_corner"].dtype.itemsize, e.lisreg.FMT_XYZI
        return SimpleNamespace(arr=arr, staged=(e.lisreg.Item * n)(), T0=np.ascontiguousarray(T0[order]))
    fwd, rev = batch(list(range(n))), batch(list(range(n))[::-1])
    ctx._n_items = n
    taken = []

    def stage(b):
        assert L.lisreg_stage_host_items(ctx._h, n, b.arr, b.staged) == 0
        taken.append(ctx.get_option("feeder_chunks_by_copy_engine"))
    def launch(b):
        assert L.lisreg_batch_prepare(ctx._h, n, b.staged, C.byref(p), b.T0.ctypes.data_as(fp)) == 0
        assert L.lisreg_batch_run(ctx._h) == 0

    def loop(stalled):
        out, pending = [], None
        stage(fwd)
        if stalled:
            gate.stall(S, ms)
            ev = gate.mark(S)
        launch(fwd)
        stage(rev)
        if stalled:
            pending = gate.event_pending(ev)
            gate.event_destroy(ev)
        out.append(ctx.batch_fetch()); launch(rev)
        stage(fwd); out.append(ctx.batch_fetch()); launch(fwd)
        out.append(ctx.batch_fetch())
        return out, pending
    try:
        ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"], slot=0)
        T_ref, st_ref = ctx.align_batch([dict(src_corner=c["src_corner"], src_surf=c["src_surf"]) for c in cases], T0, p)
        ctx.set_option("feeder_copy_engine", engine)
        loop(False)
        idle, _ = loop(False)
        ms = stall_for(e, lambda: loop(False))
        ctx.set_stream(S)
        busy, pending = loop(True)
    finally:
        ctx.set_stream(None)
        settle(e)
        ctx.close()
    want = [(T_ref, st_ref), (T_ref[::-1], st_ref[::-1]), (T_ref, st_ref)]
    for k in range(3):
        assert same(idle[k], want[k]) and same(busy[k], want[k]), k
    print(f"[caller_stream] threaded staging, feeder_copy_engine {engine}: stall {ms:.2f} ms, pending after stage(1): {pending}, chunks by the copy engine {taken}")
    if engine == 3:
        assert min(taken) > 0, "the copy engine took no chunk"
    else:
        assert max(taken) == 0
        assert pending, "staging the next batch waited for the run queued in front of it"
    for pc, ps in pins:
        pc.free(); ps.free()


# ---- D: a pending run against something the library owns ----------------------------------------------------------------------------
@pytest.mark.parametrize("rebuild", [1, 0])
def test_set_target_from_host_clouds_behind_a_pending_run(env, rebuild):
    """stall; run(A) against slot 0 set from HOST clouds; set_target of slot 0 with other host clouds.  The device copy of a host target
    is the library's: the new one must not land before the pending run has read the old one (with "rebuild_targets_each_run" the run
    re-reads the raw records, without it the sorted index).  A's fetched result is A against the OLD target."""
    e = env
    ctx, gate, S = e.ctx, e.gate, e.S
    from lisreg import synth
    cases, recs, items, T0 = _batch(e, 4, seed0=2400)
    old = (cases[0]["tgt_corner"], cases[0]["tgt_surf"])
    new = synth.make_submap(8000, seed=977)
    p = e.lisreg.default_params(1); p.fixed_iters = 5
    before = ctx.get_option("rebuild_targets_each_run")
    try:
        ctx.set_option("rebuild_targets_each_run", rebuild)
        ctx.set_target(*new, slot=0); ctx.batch_prepare_device(items, T0, p); ctx.batch_run(); want_new = ctx.batch_fetch()
        ctx.set_target(*old, slot=0); ctx.batch_prepare_device(items, T0, p); ctx.batch_run(); want_old = ctx.batch_fetch()
        assert not same(want_old, want_new)
        ms = stall_for(e, lambda: (ctx.batch_run(), ctx.set_target(*old, slot=0)))
        ctx.batch_prepare_device(items, T0, p)
        snap = e.D(np.zeros((4, 12), f32))
        ctx.set_stream(S)
        gate.stall(S, ms)
        ev = gate.mark(S)
        ctx.batch_run()
        assert gate.event_pending(ev)
        gate.copy_async(snap.ptr, ctx.result_device_ptr, 4 * 48, S)
        ctx.set_target(*new, slot=0)                                         # may wait: that is fine
        gate.stream_sync(S)
        gate.event_destroy(ev)
        ctx.batch_prepare_device(items, T0, p); ctx.batch_run(); after = ctx.batch_fetch()
    finally:
        ctx.set_stream(None)
        ctx.set_option("rebuild_targets_each_run", before)
    settle(e)
    got = to_host(snap.ptr, (4, 12))
    assert not np.array_equal(bits(got[:, :6]), bits(want_new[0])), "the pending run registered against the NEW target"
    assert np.array_equal(bits(got[:, :6]), bits(want_old[0]))
    assert [int(v) for v in got[:, 10]] == [s["n_corr_last"] for s in want_old[1]]
    assert same(after, want_new)


def test_submap_insert_behind_a_pending_gather(env):
    """stall; gather of map m into device memory; then submap_insert into m: the gathered cloud is the old store"""
    e = env
    ctx, gate, S = e.ctx, e.gate, e.S
    store = _install_submaps(e, [51], 111)
    old = GR.global_map(store, [51], None, 31)[0]
    extra = GR.make_store(np.random.default_rng(112), {0: [300, 0, 700, 150, 20]})[0]
    out = e.D(np.zeros((len(old), 4), f32))
    prm = e.lisreg.localmap_default_params()
    rel = np.array([0.01, 0.0, 0.2, 3.0, -1.0, 0.1], f32)
    devs = [e.D(c if len(c) else np.zeros((1, 4), f32)) for c in extra]
    try:
        ctx.submap_gather_device([51], None, out.ptr, len(old)); settle(e)
        assert GR.same_bits(to_host(out.ptr, (len(old), 4)), old) is None
        ms = stall_for(e, lambda: ctx.submap_gather_device([51], None, out.ptr, len(old)))
        e.hip.hipMemset(C.c_void_p(out.ptr), 0, C.c_size_t(out.nbytes)); settle(e)
        ctx.set_stream(S)
        gate.stall(S, ms)
        ev = gate.mark(S)
        assert ctx.submap_gather_device([51], None, out.ptr, len(old))[0] == len(old)
        assert gate.event_pending(ev)
        info = ctx.submap_insert_device(51, [d.ptr for d in devs], [len(c) for c in extra], rel, ZERO_POSE, prm)
        gate.stream_sync(S)
        gate.event_destroy(ev)
    finally:
        ctx.set_stream(None)
    settle(e)
    assert sum(info["n"]) > len(old)                                         # the store did grow
    assert GR.same_bits(to_host(out.ptr, (len(old), 4)), old) is None


def test_count_searches_reset_behind_a_pending_counting_run(env):
    """set_option("count_searches", 1) zeroes the counters; with a counting run pending, the zeroing is ordered behind it: what is read
    after one more run is that run's counters alone, not a part of the pending run's on top"""
    e = SimpleNamespace(**{**vars(env), "ctx": env.lisreg.Context(0)})        # a context of its own: its options end with it
    ctx, gate, S = e.ctx, e.gate, e.S
    cases, recs, items, T0 = _batch(e, 4, seed0=2500)
    p = e.lisreg.default_params(1); p.fixed_iters = 5
    try:
        ctx.set_option("search_mode", 3); ctx.set_option("lanes_per_query", 1)   # the counters are the graph front-end's
        ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"], slot=0)
        ctx.set_option("count_searches", 1)
        ctx.batch_prepare_device(items, T0, p)
        ctx.batch_run(); ctx.batch_fetch()
        one = ctx.raw_counters()
        assert sum(one) > 0
        ms = stall_for(e, ctx.batch_run)
        ctx.batch_fetch()
        ctx.set_stream(S)
        gate.stall(S, ms)
        ev = gate.mark(S)
        ctx.batch_run()
        ctx.set_option("count_searches", 1)
        assert gate.event_pending(ev), "set_option waited for the GPU or the stall was spent"
        ctx.batch_run(); ctx.batch_fetch()
        gate.event_destroy(ev)
        got = ctx.raw_counters()
    finally:
        ctx.set_stream(None)
        settle(e)
        ctx.close()
    assert got == one


# ---- E: lisreg_set_stream itself ------------------------------------------------------------------------------------------------
def test_set_stream_reports_restores_and_drains(env):
    e = env
    ctx, gate = e.ctx, e.gate
    own = ctx.stream
    assert own != 0
    S1, S2 = gate.stream_create(), gate.stream_create()
    rec = labelled_cloud(121)
    n = len(rec)
    T = np.array([0.1, 0.0, 0.3, 1.0, 2.0, 3.0], f32)
    src, mid, out = e.D(rec), e.D(np.zeros_like(rec)), e.D(np.zeros_like(rec))
    try:
        ctx.transform_cloud_device(src.ptr, n, T, mid.ptr); ctx.concat_device([mid.ptr], [n], out.ptr)
        gate.stream_sync(own); settle(e)
        want = to_host(out.ptr, (n, 4))
        e.hip.hipMemset(C.c_void_p(mid.ptr), 0, C.c_size_t(mid.nbytes)); e.hip.hipMemset(C.c_void_p(out.ptr), 0, C.c_size_t(out.nbytes)); settle(e)
        ms = stall_for(e, lambda: ctx.concat_device([src.ptr], [n], mid.ptr))
        ctx.set_stream(S1)
        assert ctx.stream == S1
        gate.stall(S1, ms)
        ev = gate.mark(S1)
        ctx.concat_device([src.ptr], [n], mid.ptr)                            # returns without waiting: pending on S1
        assert gate.event_pending(ev)
        ctx.set_stream(S2)                                                    # the switch drains S1
        assert ctx.stream == S2 and not gate.event_pending(ev)
        ctx.transform_cloud_device(mid.ptr, n, T, mid.ptr)
        ctx.concat_device([mid.ptr], [n], out.ptr)
        gate.stream_sync(S2)
        gate.event_destroy(ev)
        ctx.set_stream(None)
        assert ctx.stream == own
        assert np.array_equal(bits(to_host(out.ptr, (n, 4))), bits(want))
        gate.stream_destroy(S1); gate.stream_destroy(S2)
        S1 = S2 = None
        ctx.transform_cloud_device(src.ptr, n, T, out.ptr)                    # the caller's streams are gone, the context works on
        gate.stream_sync(ctx.stream)
        assert np.array_equal(bits(to_host(out.ptr, (n, 4))), bits(want))
    finally:
        ctx.set_stream(None)
        for s in (S1, S2):
            if s:
                gate.stream_destroy(s)


# ---- F: torch on its own stream, no synchronisation until the results are read -------------------------------------------------------
TORCH_STREAM_CASE = """
import os, sys
sys.path.insert(0, os.path.join({root!r}, "lis-slam_amd")); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
if not torch.cuda.is_available():
    print("NO_TORCH_DEVICE"); sys.exit(0)
import lisreg
import pretreat_ref as PR
import rangenet_ref as R
H, W, C_ = 16, 128, 20
raw = PR.make_sweep(12, 16, "time", n_az=450)
P = R.Params(H, W, 15.0, -15.0, {means!r}, {stds!r}, C_)
cp = lisreg.default_rangenet_params(H, W)
cp.fov_up, cp.fov_down, cp.n_classes = P.fov_up, P.fov_down, C_
for k in range(5):
    cp.means[k], cp.stds[k] = float(P.means[k]), float(P.stds[k])
ctx = lisreg.Context(0)
dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(5)
conv = torch.nn.Conv2d(5, C_, 1, bias=True)
with torch.no_grad():
    conv.weight.copy_(torch.randn((C_, 5, 1, 1), generator=g)); conv.bias.copy_(0.5 * torch.randn((C_,), generator=g))
conv = conv.to(dev)
host = torch.from_numpy(raw).pin_memory()
cloud = torch.zeros((len(raw), 4), device=dev, dtype=torch.float32)           # the decoy: an empty sweep
tensor = torch.empty((5, H, W), device=dev, dtype=torch.float32)
mask = torch.empty((H * W,), device=dev, dtype=torch.uint8)
pix = torch.empty((len(raw),), device=dev, dtype=torch.int32)
out = torch.empty((len(raw), 4), device=dev, dtype=torch.float32)
img = torch.empty((H, W), device=dev, dtype=torch.uint8)
with torch.no_grad():
    conv(torch.zeros((1, 5, H, W), device=dev))                               # the convolution's one-time set-up, outside the stream case
torch.cuda.synchronize()
s = torch.cuda.Stream()
with torch.cuda.stream(s), torch.no_grad():
    ctx.set_stream(s.cuda_stream)
    torch.cuda._sleep(100_000_000)                                            # the stall: some tens of milliseconds
    cloud.copy_(host, non_blocking=True)
    n_valid = ctx.rangenet_project_device(cloud.data_ptr(), len(raw), cp, tensor.data_ptr(), mask.data_ptr(), pix.data_ptr())
    logits = conv(tensor[None])[0].contiguous()
    ctx.rangenet_label_device(cloud.data_ptr(), len(raw), pix.data_ptr(), mask.data_ptr(), logits.data_ptr(), cp, out.data_ptr(), img.data_ptr())
    got = [t.cpu().numpy() for t in (tensor, mask, pix, logits, out, img)]   # the first wait: the results are read
ctx.set_stream(None)
ref = R.project_parallel(raw, P)
assert n_valid == ref["n_valid"] > 500
assert np.array_equal(got[0].view(np.uint32), ref["tensor"].view(np.uint32))
assert np.array_equal(got[1], ref["invalid_mask"]) and np.array_equal(got[2], ref["pixel_index"])
want, want_img = R.label_parallel(ref["pixel_index"], ref["invalid_mask"], got[3], P)
assert np.array_equal(got[4][:, :3].view(np.uint32), raw[:, :3].view(np.uint32))
assert np.array_equal(got[4][:, 3].view(np.uint32), want) and np.array_equal(got[5], want_img)
assert len(np.unique(want)) >= 3
ctx.close()
print("CASE_DONE")
"""


def _have_torch():
    try:
        import importlib.util
        return importlib.util.find_spec("torch") is not None
    except Exception:
        return False


@pytest.mark.skipif(not _have_torch(), reason="torch not installed")
def test_torch_stream_without_synchronize():
    """INTEGRATION.md section 3c, the no-synchronise form: inside `with torch.cuda.stream(s)` the context is given s.cuda_stream; a
    sleep, the copy of the sweep into the input tensor, lisreg_rangenet_project, a fixed 1 x 1 convolution and lisreg_rangenet_label
    follow each other with no torch.cuda.synchronize(); labels and tensor equal the restatement on the logits that were produced.  A
    fresh interpreter with torch imported first (as in tests/test_rangenet.py)."""
    code = textwrap.dedent(TORCH_STREAM_CASE.format(root=ROOT, means=MEANS, stds=STDS))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "NO_TORCH_DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "CASE_DONE" in r.stdout and r.returncode == 0, f"exit status {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
