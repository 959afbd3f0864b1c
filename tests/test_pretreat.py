"""Laser pretreatment (lisreg_pretreat): ring and per-point time of a raw sweep.

The yardstick is tests/pretreat_ref.py, the numpy restatement of LaserPretreatment::Pretreatment: its literal sequential loop and the
parallel form the HIP kernels implement must agree bit for bit (CPU tests), and the library must equal it bit for bit on every input
format, on the edge cases, in a batch, handed over to the feature extraction and at the head of the odometry chain (GPU tests).  Every
comparison is exact: integers equal, floats bit-equal."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pretreat_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pretreat", "pretreat_sweeps.npz")
NAMES = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")


def small_cases():
    """(raw, n_scan, min_range, max_range) of >= 20 seeded sweeps: every table x every order x spans below / at / above 2 pi (az0 chosen
    so that both endOri adjustments are taken), less than half a turn, invalid first / last points, a near-range filter."""
    out = []
    seed = 0
    for ns in (16, 32, 64):
        for order in ("time", "ring", "shuffled"):
            for span, az0 in ((1.9, 0.95 * np.pi), (2.0, None), (2.1, -0.95 * np.pi)):
                seed += 1
                out.append((R.make_sweep(seed, ns, order, span, n_az=60, beams=min(ns, 32) if order != "time" else ns, az0=az0), ns, 0.0, 70.0))
    for ns in (16, 32, 64):
        seed += 1
        out.append((R.make_sweep(seed, ns, "time", half_turn=True, n_az=50), ns, 0.0, 70.0))
        seed += 1
        out.append((R.make_sweep(seed, ns, "ring", 2.02, n_az=50, bad_ends=True), ns, 3.0, 55.0))
    return out


def full_size_raw(h, w, frames=1):
    """synthetic_raw_drive with ring and time discarded: (n, 4) float32 x y z intensity"""
    from lisreg import replay
    return [np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32)
            for sw, _ in replay.synthetic_raw_drive(frames, h, w)]


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_sequential_form_equals_parallel_form():
    cases = small_cases()
    assert len(cases) >= 20
    branches, halves, kept_total = set(), [], 0
    window = {16: 0, 32: 0}
    nan_angle_points = 0
    for raw, ns, mn, mx in cases:
        a = R.pretreat_sequential(raw, ns, mn, mx)
        b = R.pretreat_vectorised(raw, ns, mn, mx)
        assert R.same(a, b) is None, (ns, R.same(a, b))
        assert len(a["index"]) > 0 and len(a["index"]) < len(raw)          # the tables and the filters drop points by design
        branches.add(a["end_branch"]); halves.append(a["half_index"]); kept_total += len(a["index"])
        ok = R._survivors(raw, mn, mx)
        angle = R._angle(raw)
        kept = np.zeros(len(raw), bool)
        kept[a["index"]] = True
        nan = ok & np.isnan(angle)
        nan_angle_points += int(nan.sum())
        assert not kept[nan].any()                                            # NaN angle: dropped explicitly
        if ns in window:                                                      # int(-0.75 .. -0.0) -> 0: ring 0, kept
            with np.errstate(invalid="ignore"):
                v = ((angle + np.float32(15)) / np.float32(2)).astype(np.float64) + 0.5 if ns == 16 else (angle.astype(np.float64) + 92.0 / 3.0) * 3.0 / 4.0
                w = ok & (v < 0) & (v > -1)
            window[ns] += int(w.sum())
            assert kept[w].all() and (a["ring"][np.searchsorted(a["index"], np.flatnonzero(w))] == 0).all()
    assert {1, 2} <= branches, branches                                       # endOri -= 2 pi and endOri += 2 pi both taken
    assert -1 in halves and any(h > 0 for h in halves)
    assert window[16] > 0 and window[32] > 0 and nan_angle_points > 0
    assert kept_total > 20000


def test_golden_sweeps_reproduce():
    g = np.load(GOLDEN)
    for ns in (16, 32, 64):
        raw = g[f"raw{ns}"]
        assert len(raw) <= 8000
        for form in (R.pretreat_sequential, R.pretreat_vectorised):
            r = form(raw, ns)
            assert np.array_equal(r["index"], g[f"index{ns}"]) and np.array_equal(r["ring"], g[f"ring{ns}"])
            assert np.array_equal(r["time"].view(np.uint32), g[f"time{ns}"].view(np.uint32))
            assert np.array_equal(np.array([r["start_ori"], r["end_ori"]], np.float32).view(np.uint32), g[f"header{ns}"].view(np.uint32))
            assert r["half_index"] == int(g[f"half{ns}"][0])
    raw = g["raw64"]                                                          # first and last points are invalid: the ends come from inside
    ok = R._survivors(raw, 0.0, 70.0)
    assert not ok[0] and not ok[1] and not ok[-1] and not ok[-2]


def _header_struct(name):
    """ctypes mirror of `typedef struct <name> { ... }` as include/lisreg.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "void*": C.c_void_p, "float*": C.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"(\w+\s*\*?)\s+(.*)", decl).groups()
        for n in names.split(","):
            fields.append((n.strip(), types[t.replace(" ", "")]))
    return type(name, (C.Structure,), {"_fields_": fields})


def test_abi_declares_pretreat_and_structs_match_header():
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for sym in ("lisreg_default_pretreat_params", "lisreg_pretreat", "lisreg_pretreat_batch"):
        assert re.search(r"^\s*int\s+%s\s*\(" % sym, hdr, re.M), sym
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym)
    assert re.search(r"#define\s+LISREG_FMT_XYZI_PACKED\s+5\b", hdr) and lisreg.FMT_XYZI_PACKED == 5
    for mine, name in ((lisreg.PretreatParams, "lisreg_pretreat_params"), (lisreg.PretreatOut, "lisreg_pretreat_out")):
        theirs = _header_struct(name)
        assert C.sizeof(mine) == C.sizeof(theirs), name
        assert [(n, getattr(mine, n).offset) for n, _ in mine._fields_] == [(n, getattr(theirs, n).offset) for n, _ in theirs._fields_], name
    assert C.sizeof(lisreg.PretreatParams) == 24 and C.sizeof(lisreg.PretreatOut) == 48
    p = lisreg.default_pretreat_params()
    assert (p.n_scan, p.min_range, p.max_range, p.scan_period) == (64, 0.0, 70.0, 0.1)
    assert lisreg.lib().lisreg_default_pretreat_params(None) == lisreg.ERR_ARG


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _params(ns, mn=0.0, mx=70.0):
    import lisreg
    p = lisreg.default_pretreat_params(ns)
    p.min_range, p.max_range = mn, mx
    return p


def _check_host(out, info, ref, what):
    assert info["n"] == len(out) == len(ref["index"]), (what, info["n"], len(ref["index"]))          # the kept COUNT, no share tolerated
    got = np.stack([out["x"], out["y"], out["z"], out["intensity"]], 1) if len(out) else np.zeros((0, 4), np.float32)
    assert np.array_equal(got.view(np.uint32), ref["xyzi"].view(np.uint32)), what
    assert np.array_equal(out["ring"], ref["ring"]), what
    bad = np.flatnonzero(out["time"].view(np.uint32) != ref["time"].view(np.uint32))
    assert len(bad) == 0, (what, len(bad), out["time"][bad[:5]], ref["time"][bad[:5]])
    _check_header(info, ref, what)


def _check_header(info, ref, what):
    assert np.float32(info["start_ori"]).view(np.uint32) == np.float32(ref["start_ori"]).view(np.uint32), (what, info, ref["start_ori"])
    assert np.float32(info["end_ori"]).view(np.uint32) == np.float32(ref["end_ori"]).view(np.uint32), (what, info, ref["end_ori"])
    assert info["half_index"] == ref["half_index"], (what, info, ref["half_index"])


class DeviceRun:
    """a raw sweep in HBM and the three output buffers of lisreg_pretreat"""

    def __init__(self, raw, cap=None, sentinel=None):
        import lisreg
        self.n = len(raw)
        self.cap = self.n if cap is None else cap
        rows = max(self.cap, 1)
        fill = 0.0 if sentinel is None else sentinel
        self.din = lisreg.DeviceArray(raw if self.n else np.zeros((1, 4), np.float32))
        self.out = lisreg.DeviceArray(np.full((rows, 4), fill, np.float32))
        self.time = lisreg.DeviceArray(np.full(rows, fill, np.float32))
        self.inten = lisreg.DeviceArray(np.full(rows, fill, np.float32))

    def fetch(self, n):
        import lisreg
        rows = max(self.cap, 1)
        rec = lisreg.device_to_host(self.out.ptr, (rows, 4), np.float32)[:n]
        return rec, lisreg.device_to_host(self.time.ptr, (rows,), np.float32)[:n], lisreg.device_to_host(self.inten.ptr, (rows,), np.float32)[:n]


def _check_device(rec, time, inten, info, ref, what):
    assert info["n"] == len(ref["index"]), (what, info["n"], len(ref["index"]))
    assert np.array_equal(rec[:, :3].view(np.uint32), ref["xyzi"][:, :3].view(np.uint32)), what
    assert np.array_equal(rec[:, 3].view(np.uint32), ref["ring"].astype(np.uint32)), what                # ring in the payload, upper bits zero
    assert np.array_equal(inten.view(np.uint32), ref["xyzi"][:, 3].view(np.uint32)), what
    bad = np.flatnonzero(time.view(np.uint32) != ref["time"].view(np.uint32))
    assert len(bad) == 0, (what, len(bad), time[bad[:5]], ref["time"][bad[:5]])
    _check_header(info, ref, what)


def _all_formats(ctx, raw, ns, mn, mx, what):
    from lisreg import synth
    ref = R.pretreat_vectorised(raw, ns, mn, mx)
    P = _params(ns, mn, mx)
    info = {}
    out = ctx.pretreat(raw, P, info=info)                                     # host, packed 16-byte records
    _check_host(out, info, ref, (what, "packed"))
    info = {}
    out = ctx.pretreat(synth.to_pcl(raw[:, :3], None, raw[:, 3]), P, info=info)    # host, PCL PointXYZI (intensity at byte 16)
    _check_host(out, info, ref, (what, "xyzi"))
    d = DeviceRun(raw)
    info = ctx.pretreat_device(d.din.ptr, d.n, P, d.out.ptr, d.time.ptr, d.cap, d.inten.ptr)
    _check_device(*d.fetch(info["n"]), info, ref, (what, "device"))
    return ref


@pytest.mark.gpu
def test_hip_equals_restatement_on_seeded_and_golden_sweeps(gpu_ctx):
    for k, (raw, ns, mn, mx) in enumerate(small_cases()):
        _all_formats(gpu_ctx, raw, ns, mn, mx, ("seeded", k, ns))
    g = np.load(GOLDEN)
    for ns in (16, 32, 64):
        ref = _all_formats(gpu_ctx, g[f"raw{ns}"], ns, 0.0, 70.0, ("golden", ns))
        assert np.array_equal(ref["index"], g[f"index{ns}"])


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,ns,kept,total", [(64, 1800, 64, 86303, 115146), (32, 900, 32, 28788, 28788), (16, 450, 16, 5398, 7198)])
def test_hip_equals_restatement_on_full_size_sweeps(gpu_ctx, h, w, ns, kept, total):
    raws = full_size_raw(h, w, 2)
    ref = _all_formats(gpu_ctx, raws[0], ns, 0.0, 70.0, ("full", h, w, 0))
    assert (len(ref["index"]), len(raws[0])) == (kept, total)                  # what the restatement alone keeps of the first sweep
    _all_formats(gpu_ctx, raws[1], ns, 0.0, 70.0, ("full", h, w, 1))


@pytest.mark.gpu
def test_hip_edge_cases(gpu_ctx):
    import lisreg
    ctx = gpu_ctx
    raw = R.make_sweep(900, 64, "time", n_az=40)
    ref = R.pretreat_vectorised(raw, 64)
    P = _params(64)
    # n = 0
    info = {}
    assert len(ctx.pretreat(np.zeros((0, 4), np.float32), P, info=info)) == 0
    assert (info["n"], info["half_index"], float(info["start_ori"]), float(info["end_ori"])) == (0, -1, 0.0, 0.0)
    d = DeviceRun(np.zeros((0, 4), np.float32), cap=4)
    assert ctx.pretreat_device(d.din.ptr, 0, P, d.out.ptr, d.time.ptr, 4)["n"] == 0
    # everything out of range
    far = raw.copy()
    far[:, :3] *= 100.0
    info = {}
    assert len(ctx.pretreat(far, P, info=info)) == 0 and info["half_index"] == -1 and info["n"] == 0
    _check_header(info, R.pretreat_vectorised(far, 64), "far")
    d = DeviceRun(far)
    info = ctx.pretreat_device(d.din.ptr, d.n, P, d.out.ptr, d.time.ptr, d.cap)
    assert (info["n"], info["half_index"]) == (0, -1)
    # capacity one short: LISREG_ERR_ARG, the count comes back, the output is untouched
    n_keep = len(ref["index"])
    d = DeviceRun(raw, cap=n_keep - 1, sentinel=-7.5)
    with pytest.raises(lisreg.LisregError) as e:
        ctx.pretreat_device(d.din.ptr, d.n, P, d.out.ptr, d.time.ptr, d.cap, d.inten.ptr)
    assert e.value.code == lisreg.ERR_ARG
    rec, tm, it = d.fetch(d.cap)
    assert (rec == -7.5).all() and (tm == -7.5).all() and (it == -7.5).all()
    from lisreg import synth
    host = np.zeros(n_keep - 1, synth.XYZIRT_DTYPE)
    host["x"] = -7.5
    po = lisreg.PretreatOut()
    po.cloud, po.capacity = host.ctypes.data_as(C.c_void_p), n_keep - 1
    rc = lisreg.lib().lisreg_pretreat(ctx._h, raw.ctypes.data_as(C.c_void_p), len(raw), 16, lisreg.FMT_XYZI_PACKED, C.byref(P), C.byref(po))
    assert rc == lisreg.ERR_ARG and po.n == n_keep and (host["x"] == -7.5).all() and (host["ring"] == 0).all()
    d = DeviceRun(raw, cap=n_keep)                                            # exactly enough
    info = ctx.pretreat_device(d.din.ptr, d.n, P, d.out.ptr, d.time.ptr, d.cap, d.inten.ptr)
    _check_device(*d.fetch(info["n"]), info, ref, "exact capacity")
    # n_scan = 48, negative n
    for bad in (48, 0, 128):
        with pytest.raises(lisreg.LisregError) as e:
            ctx.pretreat(raw, _params(bad))
        assert e.value.code == lisreg.ERR_ARG
    po = lisreg.PretreatOut()
    po.cloud, po.capacity = host.ctypes.data_as(C.c_void_p), len(host)
    assert lisreg.lib().lisreg_pretreat(ctx._h, raw.ctypes.data_as(C.c_void_p), -1, 16, lisreg.FMT_XYZI_PACKED, C.byref(P), C.byref(po)) == lisreg.ERR_ARG
    # output aliasing the input
    d = DeviceRun(raw, sentinel=-7.5)
    for out_ptr, time_ptr in ((d.din.ptr, d.time.ptr), (d.din.ptr + 16 * (d.n - 1), d.time.ptr), (d.out.ptr, d.din.ptr + 64)):
        with pytest.raises(lisreg.LisregError) as e:
            ctx.pretreat_device(d.din.ptr, d.n, P, out_ptr, time_ptr, d.cap)
        assert e.value.code == lisreg.ERR_ARG
    assert np.array_equal(lisreg.device_to_host(d.din.ptr, raw.shape, np.float32).view(np.uint32), raw.view(np.uint32))
    assert (d.fetch(d.cap)[0] == -7.5).all()
    # 128 x 2048: 2.6e5 points
    big = full_size_raw(128, 2048)[0]
    assert len(big) > 250000
    _all_formats(ctx, big, 64, 0.0, 70.0, "128x2048")


@pytest.mark.gpu
def test_hip_batch_equals_single_calls_and_repeats(gpu_ctx):
    import lisreg
    ctx = gpu_ctx
    g = np.load(GOLDEN)
    for ns in (16, 64):
        raws = [g[f"raw{ns}"], np.zeros((0, 4), np.float32), R.make_sweep(40 + ns, ns, "ring", n_az=33), full_size_raw(16, 450)[0],
                R.make_sweep(41 + ns, ns, "time", half_turn=True, n_az=20), g[f"raw{ns}"][:257], g[f"raw{ns}"][:256]]
        P = _params(ns)
        cap = max(len(r) for r in raws)
        single = []
        for r in raws:
            d = DeviceRun(r, cap=cap)
            info = ctx.pretreat_device(d.din.ptr, d.n, P, d.out.ptr, d.time.ptr, cap, d.inten.ptr)
            single.append((info,) + d.fetch(info["n"]))
            _check_device(*d.fetch(info["n"]), info, R.pretreat_vectorised(r, ns), ("single", ns, len(r)))
        runs = []
        for rep in range(2):
            ds = [DeviceRun(r, cap=cap, sentinel=float(rep + 1)) for r in raws]
            infos = ctx.pretreat_batch_device([d.din.ptr for d in ds], [d.n for d in ds], P, [d.out.ptr for d in ds], [d.time.ptr for d in ds], cap,
                                              [d.inten.ptr for d in ds])
            runs.append([(info,) + d.fetch(info["n"]) for info, d in zip(infos, ds)])
        for s, (one, b0, b1) in enumerate(zip(single, runs[0], runs[1])):
            for other in (b0, b1):
                assert one[0]["n"] == other[0]["n"] and one[0]["half_index"] == other[0]["half_index"], (ns, s)
                for key in ("start_ori", "end_ori"):
                    assert np.float32(one[0][key]).view(np.uint32) == np.float32(other[0][key]).view(np.uint32), (ns, s, key)
                for a, b in zip(one[1:], other[1:]):
                    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (ns, s)
        assert runs[0][1][0]["n"] == 0 and runs[0][1][0]["half_index"] == -1                      # the empty sweep
    # a batch whose one sweep does not fit: LISREG_ERR_ARG
    ds = [DeviceRun(g["raw64"], cap=len(g["index64"])), DeviceRun(g["raw64"], cap=len(g["index64"]))]
    with pytest.raises(lisreg.LisregError) as e:
        ctx.pretreat_batch_device([d.din.ptr for d in ds], [d.n for d in ds], _params(64), [d.out.ptr for d in ds], [d.time.ptr for d in ds], len(g["index64"]) - 1)
    assert e.value.code == lisreg.ERR_ARG


def _imu_tables(seed, t0=100.0, n=70, rate=500.0):
    """integrated IMU rotation like imuDeskewInfo builds it: first entry zero, 500 Hz, a smooth yaw-dominant motion
    (the construction of tests/test_features.py::test_hip_deskew_matches_oracle)"""
    rng = np.random.default_rng(seed)
    t = t0 - 0.01 + np.arange(n) / rate
    w = np.stack([0.05 * np.sin(6 * (t - t0)), 0.03 * np.cos(4 * (t - t0)), 0.6 + 0.2 * np.sin(3 * (t - t0))], 1) + rng.normal(0, 0.01, (n, 3))
    rot = np.zeros((n, 3))
    rot[1:] = np.cumsum(w[1:] * np.diff(t)[:, None], 0)
    return t, rot


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,ns,rate", [(64, 1800, 64, 2), (16, 450, 16, 1)])
def test_hand_over_to_feature_extraction_with_deskew(gpu_ctx, h, w, ns, rate):
    """(restatement -> PointXYZIRT host structs -> extract_features with a de-skew) and (raw device records -> pretreat_device ->
    extract_features_device with time_device) give the same five clouds."""
    import lisreg
    from lisreg import synth
    ctx = gpu_ctx
    raw = full_size_raw(h, w)[0]
    ref = R.pretreat_vectorised(raw, ns)
    host = R.to_xyzirt(ref, synth.XYZIRT_DTYPE)
    fp = lisreg.FeatureParams(h, w, rate, 0.0, 70.0, 1.0, 0.1)
    t, rot = _imu_tables(31 + ns)
    want = ctx.extract_features(host, fp, lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0))
    plain = ctx.extract_features(host, fp)
    assert len(want["deskewed"]) > 1000 and len(want["corner"]) > 0 and len(want["surface"]) > 0
    assert np.abs(synth.pcl_xyz(want["deskewed"]) - synth.pcl_xyz(plain["deskewed"])).max() > 0.05          # the table is not trivial
    d = DeviceRun(raw)
    info = ctx.pretreat_device(d.din.ptr, d.n, _params(ns), d.out.ptr, d.time.ptr, d.cap)
    assert info["n"] == len(host)
    cap = h * w
    outs = {k: lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for k in NAMES}
    dk = lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0, time_device_ptr=d.time.ptr)
    nd = ctx.extract_features_device(d.out.ptr, info["n"], fp, {k: v.ptr for k, v in outs.items()}, cap, dk)
    for k in NAMES:
        assert nd[k] == len(want[k]), k
        got = lisreg.device_to_host(outs[k].ptr, (cap, 4), np.float32)[: nd[k]]
        assert np.array_equal(got[:, :3].view(np.uint32), synth.pcl_xyz(want[k]).astype(np.float32).view(np.uint32)), k
        assert np.array_equal(got[:, 3].view(np.uint32), want[k]["ring"].astype(np.uint32)), k


@pytest.mark.gpu
def test_raw_input_chain_equals_chain_fed_with_the_restatement(gpu_ctx):
    """RawOdomReplayer (raw records -> lisreg_pretreat in HBM) against DeviceOdomReplayer fed with the restatement's PointXYZIRT structs:
    same pose bits, key-frame decisions and counts on every frame; every frame after the first registers on both."""
    from lisreg import replay, synth
    raws = full_size_raw(64, 1800, 6)
    recs = []
    for make, feed in ((lambda: replay.RawOdomReplayer(gpu_ctx), lambda raw: raw),
                       (lambda: replay.DeviceOdomReplayer(gpu_ctx), lambda raw: R.to_xyzirt(R.pretreat_vectorised(raw, 64), synth.XYZIRT_DTYPE))):
        r = make()
        recs.append([r.step(feed(raw)) for raw in raws])
    for a, b in zip(*recs):
        assert np.array_equal(np.asarray(a["T"], np.float32).view(np.uint32), np.asarray(b["T"], np.float32).view(np.uint32)), (a["frame"], a["T"], b["T"])
        assert (a["keyframe"], a["key_id"], a["n_corner"], a["n_surf"]) == (b["keyframe"], b["key_id"], b["n_corner"], b["n_surf"]), a["frame"]
        if a["frame"] > 0:
            assert a["stats"]["status"] == 0 and b["stats"]["status"] == 0, (a["frame"], a["stats"], b["stats"])
            assert a["stats"]["iters"] == b["stats"]["iters"] and (a["n_src_corner"], a["n_src_surf"]) == (b["n_src_corner"], b["n_src_surf"])
