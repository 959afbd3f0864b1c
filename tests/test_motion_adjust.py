"""lisreg_adjust_cloud and lisreg_adjust_cloud_batch on the GPU against tests/adjust_ref.py (whose own CPU tests are in
tests/test_adjust_cloud.py): the library must equal the restatement bit for bit on host structs and on device records, under every
motion of the CPU list and at every size, in a batch, on the refusals, and handed over between the pretreatment and the feature
extraction.  Every comparison is exact: floats as uint32.  (The batch call on a caller's busy stream: tests/test_motion_stream.py.)"""
import ctypes as C

import numpy as np
import pytest

import adjust_ref as A

pytestmark = pytest.mark.gpu
NAMES = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
SENTINEL = -7.5
_cache = {}


def _structs(xyz, time, inten, ring):
    from lisreg import synth
    c = np.zeros(len(xyz), synth.XYZIRT_DTYPE)
    c["x"], c["y"], c["z"], c["intensity"], c["ring"], c["time"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], inten, ring, time
    return c


def _sweeps():
    """the clouds of the GPU tests as PointXYZIRT structs, made once: n = 0, 1, 2, 257, a full 16 x 450 sweep, one 64 x 1800 sweep"""
    if "sweeps" not in _cache:
        from lisreg import replay
        g = _structs(*A.make_points(A.GOLDEN_SEED, A.GOLDEN_N))
        full16 = next(iter(replay.synthetic_raw_drive(1, 16, 450)))[0]
        full64 = next(iter(replay.synthetic_raw_drive(1, 64, 1800)))[0]
        assert len(full16) > 5000 and len(full64) > 100000
        _cache["sweeps"] = dict(n0=g[:0], n1=g[:1], n2=g[:2], n257=g[:257], full16=full16, full64=full64)
    return _cache["sweeps"]


def _want(sweep_name, motion_name):
    """adjust_ref on a cloud of _sweeps(), computed once and shared"""
    key = (sweep_name, motion_name)
    if key not in _cache:
        _cache[key] = A.adjust_structs(_sweeps()[sweep_name], A.MOTIONS[motion_name])
    return _cache[key]


def _motion(name_or_tuple):
    import lisreg
    sp, v, w = A.MOTIONS[name_or_tuple] if isinstance(name_or_tuple, str) else name_or_tuple
    return lisreg.make_motion(v, w, sp)


def _records(c):
    rec = np.zeros((len(c), 4), np.float32)
    rec[:, 0], rec[:, 1], rec[:, 2] = c["x"], c["y"], c["z"]
    rec[:, 3] = c["ring"].astype(np.uint32).view(np.float32)
    return rec


class DeviceSweep:
    """a cloud's records and times in HBM, and sentinel-filled output buffers of `cap` points (+ 3 rows behind them)"""

    def __init__(self, c, cap=None):
        import lisreg
        self.n = len(c)
        self.cap = max(self.n - 1, 0) if cap is None else cap
        self.rows = self.cap + 3
        self.din = lisreg.DeviceArray(_records(c) if self.n else np.zeros((1, 4), np.float32))
        self.dtime = lisreg.DeviceArray(np.ascontiguousarray(c["time"]) if self.n else np.zeros(1, np.float32))
        self.out = lisreg.DeviceArray(np.full((self.rows, 4), SENTINEL, np.float32))
        self.otime = lisreg.DeviceArray(np.full(self.rows, SENTINEL, np.float32))

    def fetch(self):
        import lisreg
        return lisreg.device_to_host(self.out.ptr, (self.rows, 4), np.float32), lisreg.device_to_host(self.otime.ptr, (self.rows,), np.float32)


def _check_structs(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for f in ("x", "y", "z", "intensity", "time"):
        bad = np.flatnonzero(got[f].view(np.uint32) != want[f].view(np.uint32))
        assert len(bad) == 0, (what, f, len(bad), got[f][bad[:4]], want[f][bad[:4]])
    assert np.array_equal(got["ring"], want["ring"]), what


def _check_device(rec, tm, n_out, want, what):
    assert n_out == len(want), (what, n_out, len(want))
    for k, f in enumerate(("x", "y", "z")):
        bad = np.flatnonzero(rec[:n_out, k].view(np.uint32) != want[f].view(np.uint32))
        assert len(bad) == 0, (what, f, len(bad), rec[bad[:4], k], want[f][bad[:4]])
    assert np.array_equal(rec[:n_out, 3].view(np.uint32), want["ring"].astype(np.uint32)), what
    assert np.array_equal(tm[:n_out].view(np.uint32), want["time"].view(np.uint32)), what
    assert (rec[n_out:] == SENTINEL).all() and (tm[n_out:] == SENTINEL).all(), what           # nothing behind out->n


@pytest.mark.parametrize("motion", list(A.MOTIONS))
def test_hip_equals_restatement_on_host_structs_and_device_records(gpu_ctx, motion):
    M = _motion(motion)
    for name, c in _sweeps().items():
        want = _want(name, motion)
        assert len(want) == max(len(c) - 1, 0)
        guard = np.zeros(len(want) + 2, c.dtype)                                # host structs; a sentinel behind the output
        guard["x"] = SENTINEL
        ao = __import__("lisreg").AdjustOut()
        ao.cloud, ao.capacity = guard.ctypes.data_as(C.c_void_p), len(want)
        cc = np.ascontiguousarray(c)
        rc = gpu_ctx._L.lisreg_adjust_cloud(gpu_ctx._h, cc.ctypes.data_as(C.c_void_p) if len(cc) else None, len(cc), cc.dtype.itemsize, 3, None,
                                            C.byref(M), C.byref(ao))
        assert rc == 0 and ao.n == len(want), (name, rc, ao.n)
        _check_structs(guard[: ao.n], want, (motion, name, "host"))
        assert (guard["x"][ao.n:] == SENTINEL).all() and (guard["time"][ao.n:] == 0).all()
        _check_structs(gpu_ctx.adjust_cloud(c, M), want, (motion, name, "host wrapper"))
        d = DeviceSweep(c)
        n_out = gpu_ctx.adjust_cloud_device(d.din.ptr, d.n, d.dtime.ptr, M, d.out.ptr, d.otime.ptr, d.cap)
        _check_device(*d.fetch(), n_out, want, (motion, name, "device"))
    if motion == "drive":                                                      # the input really moves
        c, want = _sweeps()["full16"], _want("full16", motion)
        assert np.abs(want["x"] - c["x"][1:]).max() > 0.3


def _batch_sweeps():
    s = _sweeps()
    rng = np.random.default_rng(5)
    shuffled = s["full16"][rng.permutation(len(s["full16"]))]
    clouds = [s["n0"], s["n1"], s["n2"], s["n257"], s["full16"], s["full16"][::-1].copy(), shuffled, s["n257"][::2].copy()]
    motions = ["drive", "all_axes", "fast_yaw", "tiny_rate", "all_axes", "drive", "fast_yaw", "zero"]
    return clouds, motions


def test_hip_batch_equals_single_calls_and_repeats(gpu_ctx):
    """eight sweeps, each with its own motion: empty, one point, two points, 257 points, two full sweeps, a shuffled one, a zero-rate one"""
    clouds, motions = _batch_sweeps()
    Ms = [_motion(m) for m in motions]
    cap = max(len(c) for c in clouds)
    single = []
    for c, M, m in zip(clouds, Ms, motions):
        d = DeviceSweep(c, cap)
        n_out = gpu_ctx.adjust_cloud_device(d.din.ptr, d.n, d.dtime.ptr, M, d.out.ptr, d.otime.ptr, cap)
        single.append((n_out,) + d.fetch())
        _check_device(single[-1][1], single[-1][2], n_out, A.adjust_structs(c, A.MOTIONS[m]), ("single", m, len(c)))
    runs = []
    for rep in range(2):
        ds = [DeviceSweep(c, cap) for c in clouds]
        ns = gpu_ctx.adjust_cloud_batch_device([d.din.ptr for d in ds], [d.n for d in ds], [d.dtime.ptr for d in ds], Ms, [d.out.ptr for d in ds],
                                               [d.otime.ptr for d in ds], cap)
        runs.append([(n,) + d.fetch() for n, d in zip(ns, ds)])
    for s, (one, b0, b1) in enumerate(zip(single, runs[0], runs[1])):
        for other in (b0, b1):
            assert one[0] == other[0] == max(len(clouds[s]) - 1, 0), s
            assert one[1].tobytes() == other[1].tobytes() and one[2].tobytes() == other[2].tobytes(), s
    assert [r[0] for r in runs[0]][:4] == [0, 0, 1, 256]


def test_hip_refusals_leave_the_outputs_untouched(gpu_ctx):
    import lisreg
    ctx = gpu_ctx
    c = _sweeps()["n257"]
    M = _motion("drive")
    # capacity one too small: the count comes back, nothing is written
    d = DeviceSweep(c, cap=255)
    ao = lisreg.AdjustOut()
    ao.cloud, ao.capacity, ao.time_device = C.c_void_p(d.out.ptr), 255, C.c_void_p(d.otime.ptr)
    rc = ctx._L.lisreg_adjust_cloud(ctx._h, C.c_void_p(d.din.ptr), d.n, 16, lisreg.FMT_DEVICE, C.c_void_p(d.dtime.ptr), C.byref(M), C.byref(ao))
    assert rc == lisreg.ERR_ARG and ao.n == 256
    rec, tm = d.fetch()
    assert (rec == SENTINEL).all() and (tm == SENTINEL).all()
    host = np.zeros(255, c.dtype)
    host["x"] = SENTINEL
    with pytest.raises(lisreg.LisregError) as e:
        ctx.adjust_cloud(c, M, capacity=255)
    assert e.value.code == lisreg.ERR_ARG
    ao = lisreg.AdjustOut()
    ao.cloud, ao.capacity = host.ctypes.data_as(C.c_void_p), 255
    cc = np.ascontiguousarray(c)
    assert ctx._L.lisreg_adjust_cloud(ctx._h, cc.ctypes.data_as(C.c_void_p), len(cc), 32, lisreg.FMT_XYZIRT, None, C.byref(M), C.byref(ao)) == lisreg.ERR_ARG
    assert ao.n == 256 and (host["x"] == SENTINEL).all() and (host["ring"] == 0).all()
    ds = [DeviceSweep(c, cap=256), DeviceSweep(c, cap=255)]
    with pytest.raises(lisreg.LisregError) as e:
        ctx.adjust_cloud_batch_device([x.din.ptr for x in ds], [x.n for x in ds], [x.dtime.ptr for x in ds], [M, M], [x.out.ptr for x in ds],
                                      [x.otime.ptr for x in ds], [256, 255])
    assert e.value.code == lisreg.ERR_ARG
    for x in ds:
        rec, tm = x.fetch()
        assert (rec == SENTINEL).all() and (tm == SENTINEL).all()
    # overlapping in / out (the shift by one makes in-place a race)
    d = DeviceSweep(c)
    before = lisreg.device_to_host(d.din.ptr, (d.n, 4), np.float32)
    for out_ptr, time_ptr in ((d.din.ptr, d.otime.ptr), (d.din.ptr + 16 * (d.n - 1), d.otime.ptr), (d.out.ptr, d.dtime.ptr), (d.out.ptr, d.din.ptr + 64),
                              (d.dtime.ptr, d.otime.ptr)):
        with pytest.raises(lisreg.LisregError) as e:
            ctx.adjust_cloud_device(d.din.ptr, d.n, d.dtime.ptr, M, out_ptr, time_ptr, d.cap)
        assert e.value.code == lisreg.ERR_ARG
        with pytest.raises(lisreg.LisregError) as e:
            ctx.adjust_cloud_batch_device([d.din.ptr], [d.n], [d.dtime.ptr], [M], [out_ptr], [time_ptr], d.cap)
        assert e.value.code == lisreg.ERR_ARG
    assert lisreg.device_to_host(d.din.ptr, (d.n, 4), np.float32).tobytes() == before.tobytes()
    assert lisreg.device_to_host(d.dtime.ptr, (d.n,), np.float32).tobytes() == np.ascontiguousarray(c["time"]).tobytes()
    rec, tm = d.fetch()
    assert (rec == SENTINEL).all() and (tm == SENTINEL).all()
    inplace = c.copy()
    ao = lisreg.AdjustOut()
    ao.cloud, ao.capacity = inplace.ctypes.data_as(C.c_void_p), 256
    assert ctx._L.lisreg_adjust_cloud(ctx._h, inplace.ctypes.data_as(C.c_void_p), len(inplace), 32, lisreg.FMT_XYZIRT, None, C.byref(M), C.byref(ao)) == lisreg.ERR_ARG
    assert all(np.array_equal(inplace[f], c[f]) for f in c.dtype.names)
    # more than 256 sweeps
    two = DeviceSweep(_sweeps()["n2"])
    S = 257
    with pytest.raises(lisreg.LisregError) as e:
        ctx.adjust_cloud_batch_device([two.din.ptr] * S, [2] * S, [two.dtime.ptr] * S, [M] * S, [two.out.ptr + 16 * 0] * S, [two.otime.ptr] * S, 1)
    assert e.value.code == lisreg.ERR_ARG
    rec, tm = two.fetch()
    assert (rec == SENTINEL).all() and (tm == SENTINEL).all()
    # a format the call does not take, a missing time array
    with pytest.raises(lisreg.LisregError):
        ctx.adjust_cloud_device(d.din.ptr, d.n, 0, M, d.out.ptr, d.otime.ptr, d.cap)
    ao = lisreg.AdjustOut()
    ao.cloud, ao.capacity = host.ctypes.data_as(C.c_void_p), 255
    assert ctx._L.lisreg_adjust_cloud(ctx._h, cc.ctypes.data_as(C.c_void_p), 10, 32, lisreg.FMT_XYZI, None, C.byref(M), C.byref(ao)) == lisreg.ERR_ARG
    assert ctx._L.lisreg_adjust_cloud(ctx._h, cc.ctypes.data_as(C.c_void_p), 10, 24, lisreg.FMT_XYZIRT, None, C.byref(M), C.byref(ao)) == lisreg.ERR_ARG


def test_hand_over_pretreat_adjust_extract(oracle, gpu_ctx):
    """raw records -> pretreat_batch_device -> adjust_cloud_batch_device -> extract_features_batch_device: for every sweep the index lists
    of oracle.extract_features on adjust_ref(pretreat_ref(raw)) as host structs, and its coordinates to the bit"""
    import lisreg
    import pretreat_ref as R
    from lisreg import replay, synth
    ctx = gpu_ctx
    h, w, ns = 16, 450, 16
    raws = [np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32) for sw, _ in replay.synthetic_raw_drive(3, h, w)]
    raws.append(raws[1][::50].copy())                                         # a sparse sweep: too few points per ring for the stencil
    motions = ["drive", "all_axes", "zero", "fast_yaw"]
    S = len(raws)
    cap = max(len(r) for r in raws)
    P = lisreg.default_pretreat_params(ns)
    din = [lisreg.DeviceArray(r) for r in raws]
    rec = [lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for _ in raws]
    tim = [lisreg.DeviceArray(np.zeros(cap, np.float32)) for _ in raws]
    infos = ctx.pretreat_batch_device([d.ptr for d in din], [len(r) for r in raws], P, [d.ptr for d in rec], [d.ptr for d in tim], cap)
    adj = [lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for _ in raws]
    atim = [lisreg.DeviceArray(np.zeros(cap, np.float32)) for _ in raws]
    ns_adj = ctx.adjust_cloud_batch_device([d.ptr for d in rec], [i["n"] for i in infos], [d.ptr for d in tim], [_motion(m) for m in motions],
                                           [d.ptr for d in adj], [d.ptr for d in atim], cap)
    fp = lisreg.FeatureParams(h, w, 1, 0.0, 70.0, 1.0, 0.1)
    po = oracle.FeatureParams(h, w, 1, 0.0, 70.0, 1.0, 0.1)
    fcap = h * w
    outs = [{k: lisreg.DeviceArray(np.zeros((fcap, 4), np.float32)) for k in NAMES} for _ in raws]
    counts = ctx.extract_features_batch_device([d.ptr for d in adj], ns_adj, fp, [{k: v.ptr for k, v in o.items()} for o in outs], fcap)
    total = 0
    for s in range(S):
        host = A.adjust_structs(R.to_xyzirt(R.pretreat_vectorised(raws[s], ns), synth.XYZIRT_DTYPE), A.MOTIONS[motions[s]])
        assert ns_adj[s] == len(host) == infos[s]["n"] - 1 > 20
        ro = oracle.extract_features(host, po)
        want_rec = _records(host)
        for k in NAMES:
            assert counts[s][k] == len(ro[k]), (s, k, counts[s][k], len(ro[k]))
            got = lisreg.device_to_host(outs[s][k].ptr, (fcap, 4))[: counts[s][k]]
            assert got.tobytes() == want_rec[ro[k]].tobytes(), (s, k)
            total += counts[s][k]
        assert np.array_equal(lisreg.device_to_host(atim[s].ptr, (cap,), np.float32)[: ns_adj[s]].view(np.uint32), host["time"].view(np.uint32)), s
    assert total > 3000
