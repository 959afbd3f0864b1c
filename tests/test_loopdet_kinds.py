"""The other six loopDetection selectors (ISC, SC, EPSC, SEPSC, SSC, Pose; src/core/epscGeneration.cpp:403-476, 564-589, 611-992): the
restatement's quirks on hand-built clouds (CPU), the exported C ABI (CPU), and the device path against the restatement (GPU)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import loopdet_ref as R
import loopdet_kinds_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pcl(xyz, label=None, intensity=None):
    from lisreg import synth
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return synth.to_pcl(xyz, None if label is None else np.asarray(label, np.uint16).reshape(-1),
                        None if intensity is None else np.asarray(intensity, np.float32).reshape(-1))


def empty():
    return pcl(np.zeros((0, 3)), [])


def polar(r, a, z=0.0):
    t = a - math.pi
    return [r * math.cos(t), r * math.sin(t), z]


CELL = (int(7.0 / R.RING_STEP), int(1.0 / R.SECTOR_STEP))       # the cell of polar(10.0, 1.0)


def z_of(v):
    """a z whose SC value (int)(100 * (z + 5) / 8) is v."""
    z = np.float32(v * 8.0 / 100.0 - 5.0 + math.copysign(0.01, v))      # truncation is toward zero
    assert K.sc_values([z])[0] == v
    return float(z)


# ---- CPU: the restatement's quirks ---------------------------------------------------------------------------------------------

def test_sc_signed_char_wrap_depends_on_order():
    a, b = polar(10.0, 1.0, z_of(200)), polar(10.0, 1.0, z_of(50))
    assert K.sc(pcl([a, b], [9, 9]))[CELL] == 50           # 200 stores -56, then 50 > -56
    assert K.sc(pcl([b, a], [9, 9]))[CELL] == 200          # 50, then 200 > 50 stores byte 200
    assert K.sc(pcl([b], [9]))[CELL] == 50


def test_sc_values_below_minus_128_never_update():
    a, low, mid = (polar(10.0, 1.0, z_of(v)) for v in (200, -130, -50))
    assert K.sc(pcl([a, low], [9, 9]))[CELL] == 200        # -130 < -56 but never stored
    assert K.sc(pcl([a, mid], [9, 9]))[CELL] == 256 - 50   # -50 > -56 is
    assert K.sc(pcl([low], [9]))[CELL] == 0
    # NaN z: INT_MIN, a no-op; z = 1e30: out of range, INT_MIN too (not a saturated 2^31 - 1)
    assert list(K.sc_values(np.array([np.nan, 1e30, -1e30], np.float32))) == [K.INT_MIN] * 3
    assert K.sc(pcl([polar(10.0, 1.0, 1e30)], [9]))[CELL] == 0


def test_isc_reset_then_max():
    p = polar(10.0, 1.0)
    assert K.isc(pcl([p, p], [9, 9], [1.2, 0.5]))[CELL] == 127       # 306 stores 50, then 127 > 50
    assert K.isc(pcl([p, p], [9, 9], [0.5, 1.2]))[CELL] == 50        # 127, then 306 > 127 stores 306 & 255
    assert K.isc(pcl([p, p], [9, 9], [0.5, -3.0]))[CELL] == 127      # negative: never
    assert K.isc(pcl([p], [9], [np.nan]))[CELL] == 0


def test_index_ordered_fold_equals_the_sequential_loop():
    rng = np.random.default_rng(5)
    for signed, lo, hi in ((True, -300, 400), (False, -100, 700)):
        cells = rng.integers(-1, 6, 4000)
        vals = rng.integers(lo, hi, 4000)
        vals[rng.random(4000) < 0.02] = K.INT_MIN
        assert np.array_equal(K.fold_indexed(cells, vals, signed), K.fold_sequential(cells, vals, signed)), signed


def test_ssc_priority_ties_and_labels_past_order_vec():
    p = polar(10.0, 1.0)
    assert K.ssc(pcl([p, p], [17, 9]))[CELL] == 9          # order 10 beats 9
    assert K.ssc(pcl([p, p, p], [19, 13, 15]))[CELL] == 19
    assert K.ssc(pcl([p, p], [9, 9]))[CELL] == 9           # a tie keeps the first point: the same label
    assert K.ssc(pcl([p], [25]))[CELL] == 0                # >= 20: order 0 (the deviation), skipped
    assert K.ssc(pcl([p, p], [25, 13]))[CELL] == 13
    assert K.ssc(pcl([p], [8]))[CELL] == 0                 # order 0
    rng = np.random.default_rng(1)
    r = rng.uniform(0, 70, 3000); t = rng.uniform(-math.pi, math.pi, 3000)
    cl = pcl(np.stack([r * np.cos(t), r * np.sin(t), np.zeros(3000)], 1), rng.integers(0, 30, 3000))
    assert np.array_equal(K.ssc(cl), K.ssc_sequential(cl))


def test_label_sim_nan_is_never_selected():
    z = np.zeros((20, 80), np.uint8)
    s = K.label_sim(z, z)
    assert math.isnan(s) and not (s > K.LABEL_THRESHOLD)
    a = z.copy(); a[0, 0] = 9; a[0, 1] = 13
    b = z.copy(); b[0, 0] = 9
    assert K.label_sim(a, b) == 0.5


def _fake_icp(T):
    def g(hist_proj, cur_proj, yaw_diff, oracle):
        return dict(shift=0, angle=np.float32(0), T=T.copy(), state=0, iters=0, n_corr=0)
    return g


def _room(seed=3):
    rng = np.random.default_rng(seed)
    n = 3000
    r = rng.uniform(4, 50, n); t = rng.uniform(-math.pi, math.pi, n)
    xyz = np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-3, 9, n)], 1)
    sem = pcl(xyz, rng.integers(9, 20, n), rng.uniform(0, 1.3, n))
    return pcl(xyz[:500]), pcl(xyz[500:]), sem


def test_push_order_duplicates_and_epsc_unwrapped_yaw(monkeypatch):
    """frames at x = 0, 21, 0 with the same clouds and an identity ICP: frame 2 gates frame 1 and every kind matches it, so the
    matched list holds history id 1 seven times in push order; EPSC's rotation is the unwrapped yaw difference (0.2 - 0.5)."""
    from lisreg import synth
    monkeypatch.setattr(R, "global_icp", _fake_icp(np.eye(4, dtype=np.float32)))
    E = K.EPSCGenerationKinds(None, K.ALL)
    cl = _room()
    out = [E.loop_detection(*cl, synth.pose_matrix([0, 0, yaw, x, 0, 0])[:3].astype(np.float32))
           for x, yaw in ((0.0, 0.0), (21.0, 0.5), (0.0, 0.2))]
    assert [m[0] for m in out[2]["matches"]] == [K.ISC, K.SC, K.EPSC, K.SEPSC, K.FEPSC, K.SSC, K.POSE]
    assert all(m[1] == 1 for m in out[2]["matches"])
    kinds = {m[0]: m for m in out[2]["matches"]}
    yaw_diff = float(np.float32(np.float32(0.2) - np.float32(0.5)))
    assert yaw_diff < 0
    c = out[2]["candidates"][0]
    assert c["shift"][K.EPSC] == 0 and c["score"][K.EPSC] == 1.0
    assert np.array_equal(kinds[K.EPSC][2], K.planar(np.eye(4, dtype=np.float32), yaw_diff))
    # an ICP rotation of 0.1: ISC / SC / SEPSC refine the ICP's angle, EPSC the unwrapped yaw difference, FEPSC keeps the ICP's
    T = R.rot_z(np.float32(0.1))
    monkeypatch.setattr(R, "global_icp", _fake_icp(T))
    E = K.EPSCGenerationKinds(None, K.ALL)
    out = [E.loop_detection(*cl, synth.pose_matrix([0, 0, yaw, x, 0, 0])[:3].astype(np.float32))
           for x, yaw in ((0.0, 0.0), (21.0, 0.5), (0.0, 0.2))]
    c = out[2]["candidates"][0]
    icp = float(R.atan2f(T[1, 0], T[0, 0]))
    assert c["angle"][K.EPSC] == yaw_diff + c["shift"][K.EPSC] * R.SECTOR_STEP
    for k in (K.ISC, K.SC, K.SEPSC):
        assert c["angle"][k] == icp + c["shift"][k] * R.SECTOR_STEP
    assert c["angle"][K.FEPSC] == icp
    assert np.array_equal(kinds[K.FEPSC][2], np.eye(4, dtype=np.float32))
    assert kinds[K.SSC][3] == 1.0 and kinds[K.POSE][3] == 0.0
    # FEPSC alone is the restatement of loopdet_ref
    E1, E2 = K.EPSCGenerationKinds(None), R.EPSCGeneration(None)
    for x, yaw in ((0.0, 0.0), (21.0, 0.5), (0.0, 0.2)):
        odom = synth.pose_matrix([0, 0, yaw, x, 0, 0])[:3].astype(np.float32)
        a, b = E1.loop_detection(*cl, odom), E2.loop_detection(*cl, odom)
        assert [(m[1], m[3]) for m in a["matches"]] == ([(b["matched_frame_id"], b["score"])] if b["matched_frame_id"] >= 0 else [])


def test_library_exports_kind_symbols():
    import lisreg
    L = C.CDLL(lisreg.LIB_PATH)
    for s in ("lisreg_loopdet_configure", "lisreg_loopdet_matches", "lisreg_loopdet_candidate_scores", "lisreg_loopdet_get_descriptor",
              "lisreg_loop_descriptor_kind"):
        assert hasattr(L, s), s
    assert C.sizeof(lisreg.LoopdetMatch) == 80 and C.sizeof(lisreg.LoopdetKindScores) == 88
    assert (lisreg.LOOP_ISC, lisreg.LOOP_FEPSC, lisreg.LOOP_POSE) == (1, 16, 64)
    assert lisreg.loop_kinds(["isc", "POSE"]) == 65


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _keep_off_edges(cloud, M, margin=1e-4):
    if len(cloud) == 0:
        return cloud
    x, y, _ = R._moved(cloud, M)
    a = math.pi + np.arctan2(y.astype(np.float64), x.astype(np.float64))
    f = a / R.SECTOR_STEP
    keep = np.abs(f - np.round(f)) > margin
    return cloud[keep]


def _frame_clouds(seed, n_sem=6000):
    """the test_loopdet clouds, with intensities up to 1.3 (ISC wraps), some NaN / negative ones, and points up to 9 m high (SC wraps)."""
    from lisreg import synth
    rng = np.random.default_rng(seed)
    s = synth.make_scan(16, 360, seed=seed, labelled=True)
    n = n_sem
    r = np.concatenate([rng.uniform(0, 70, n - 8), [3.0, 60.0, 3.0, 60.0, 0.0, 2.99, 59.99, 1e-3]])
    t = rng.uniform(-math.pi, math.pi, n)
    xyz = np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-13, 9, n)], 1)
    lab = rng.integers(0, 60, n)
    inten = rng.uniform(-0.1, 1.3, n)
    inten[rng.random(n) < 0.01] = np.nan
    sem = synth.concat_clouds([synth.to_pcl(xyz.astype(np.float32), lab.astype(np.uint16), inten.astype(np.float32)), s["corner"], s["surf"]])
    return s["corner"], s["surf"], sem


MATRICES = [None,
            np.array([[0.8, -0.6, 0, 1.5], [0.6, 0.8, 0, -2.25], [0, 0, 1, 0.1], [0, 0, 0, 1]], np.float32),
            np.array([[math.cos(2.9), -math.sin(2.9), 0.01, -4.0], [math.sin(2.9), math.cos(2.9), 0, 3.0], [0, 0.02, 1, 0.7],
                      [0, 0, 0, 1]], np.float32)]


@pytest.mark.gpu
def test_kind_descriptors_exact(gpu_ctx):
    import lisreg
    for seed in (1, 2):
        corner, surf, sem = _frame_clouds(seed)
        for M in MATRICES:
            c, s, m = (_keep_off_edges(x, M) for x in (corner, surf, sem))
            ref = K.all_descriptors(c, s, m, M)
            assert ref[K.SC].max() > 127 and ref[K.ISC].any() and ref[K.SSC].any()
            devs = [lisreg.DeviceArray(lisreg.pack_device_records(x)) if len(x) else None for x in (c, s, m)]
            dev_clouds = [(d.ptr, len(x)) if d is not None else (0, 0) for d, x in zip(devs, (c, s, m))]
            for k in range(6):
                got = gpu_ctx.loop_descriptor_kind(1 << k, c, s, m, M)
                assert np.array_equal(got, ref[k]), (seed, K.NAMES[k], np.count_nonzero(got != ref[k]))
                if k != K.ISC:
                    assert np.array_equal(gpu_ctx.loop_descriptor_kind(1 << k, *dev_clouds, M), ref[k]), (seed, K.NAMES[k])
    for k in range(6):
        assert not gpu_ctx.loop_descriptor_kind(1 << k, empty(), empty(), empty()).any()


def _drive():
    """make_loop_drive(24, 3, w=361) with seeded intensities (up to 1.3) and 5 % of the semantic points raised above 5.24 m."""
    from lisreg import synth
    frames = synth.make_loop_drive(24, 3, h=16, w=361)
    for j, f in enumerate(frames):
        rng = np.random.default_rng(100 + j)
        sem = f["semantic"].copy()
        sem["intensity"] = rng.uniform(0.0, 1.3, len(sem)).astype(np.float32)
        tall = rng.random(len(sem)) < 0.05
        sem["z"][tall] = rng.uniform(5.3, 9.0, int(tall.sum())).astype(np.float32)
        f["semantic"] = sem
    return frames


def _close(a, b, tol):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol


@pytest.mark.gpu
def test_end_to_end_all_kinds_against_restatement(gpu_ctx, oracle):
    frames = _drive()
    label_thr = 0.5                          # this drive's SSC scores are ~0.4 - 0.65: below the default 0.79 nothing would be selected
    E = K.EPSCGenerationKinds(oracle, K.ALL, label_threshold=label_thr)
    ref = [E.loop_detection(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    gpu_ctx.loopdet_reset(5)
    gpu_ctx.loopdet_configure(K.ALL, db_id=5, label_threshold=label_thr)
    got = gpu_ctx.loopdet_detect([(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames], db_id=5)
    n_cand, n_match = 0, np.zeros(7, int)
    for k, (r, g) in enumerate(zip(ref, got)):
        cs = gpu_ctx.loopdet_candidate_scores(k, db_id=5)
        assert [c["history_id"] for c in cs] == [c["history_id"] for c in r["candidates"]], k
        n_cand += len(cs)
        for c, rc in zip(cs, r["candidates"]):
            for kk in range(6):
                assert _close(c["score"][kk], rc["score"][kk], 5e-3), (k, K.NAMES[kk], c["score"][kk], rc["score"][kk])
            assert c["score"][K.POSE] == rc["pos_distance"]
        ms = gpu_ctx.loopdet_matches(k, db_id=5)
        kinds = [m["kind"].bit_length() - 1 for m in ms]
        assert kinds == sorted(kinds) and len(set(kinds)) == len(kinds), k          # push order, one entry per kind
        byk = {m["kind"].bit_length() - 1: m for m in ms}
        rk = {m[0]: m for m in r["matches"]}
        for kk in range(7):
            if kk == K.POSE:
                ok = True
            else:
                thr = label_thr if kk == K.SSC else 0.75
                sc = sorted((c["score"][kk] for c in r["candidates"] if not math.isnan(c["score"][kk])), reverse=True)
                ok = (len(sc) < 2 or sc[0] - sc[1] > 1e-2) and (not sc or abs(sc[0] - thr) > 5e-3)
            if ok:
                assert (kk in byk) == (kk in rk), (k, K.NAMES[kk])
                if kk in byk:
                    assert byk[kk]["history_id"] == rk[kk][1], (k, K.NAMES[kk])
            if kk in byk and kk in rk and byk[kk]["history_id"] == rk[kk][1]:
                assert np.abs(byk[kk]["transform"] - rk[kk][2]).max() <= 1e-3, (k, K.NAMES[kk], byk[kk]["transform"], rk[kk][2])
                n_match[kk] += 1
        # the FEPSC result of lisreg_loopdet_detect is the FEPSC entry of the list
        fe = byk.get(K.FEPSC)
        assert g["matched_frame_id"] == (fe["history_id"] if fe else -1)
        if fe:
            assert np.array_equal(g["matched_transform"], fe["transform"]) and g["score"] == fe["score"]
        f = frames[k]
        for kk in range(6):
            stored = gpu_ctx.loopdet_get_descriptor(k, 1 << kk, db_id=5)
            assert np.array_equal(stored, gpu_ctx.loop_descriptor_kind(1 << kk, f["corner"], f["surf"], f["semantic"])), (k, kk)
            assert np.count_nonzero(stored != E.db[kk][k]) <= 16, (k, K.NAMES[kk])
    assert n_cand >= 40
    assert all(n_match >= 10), n_match


@pytest.mark.gpu
def test_batch_equals_sequential_all_kinds(gpu_ctx):
    frames = _drive()[:60]
    items = [(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    for db in (6, 7):
        gpu_ctx.loopdet_reset(db)
        gpu_ctx.loopdet_configure(K.ALL, db_id=db)
    batch = gpu_ctx.loopdet_detect(items, db_id=6)
    mb = [gpu_ctx.loopdet_matches(k, db_id=6) for k in range(len(items))]
    sb = [gpu_ctx.loopdet_candidate_scores(k, db_id=6) for k in range(len(items))]
    assert sum(len(m) for m in mb) > 0
    for k, it in enumerate(items):
        one = gpu_ctx.loopdet_detect([it], db_id=7)[0]
        assert one["matched_frame_id"] == batch[k]["matched_frame_id"] and one["score"] == batch[k]["score"], k
        m1 = gpu_ctx.loopdet_matches(0, db_id=7)
        assert len(m1) == len(mb[k]), k
        for a, b in zip(m1, mb[k]):
            assert a["kind"] == b["kind"] and a["history_id"] == b["history_id"] and np.array_equal(a["transform"], b["transform"])
            assert a["score"] == b["score"], k
        s1 = gpu_ctx.loopdet_candidate_scores(0, db_id=7)
        for a, b in zip(s1, sb[k]):
            assert a["history_id"] == b["history_id"] and np.array_equal(a["shift"], b["shift"])
            assert np.array_equal(a["score"], b["score"], equal_nan=True), k


@pytest.mark.gpu
def test_fepsc_configured_equals_unconfigured(gpu_ctx):
    import lisreg
    frames = _drive()[:50]
    items = [(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    gpu_ctx.loopdet_reset(8)
    gpu_ctx.loopdet_reset(9)
    gpu_ctx.loopdet_configure(lisreg.LOOP_FEPSC, db_id=9)
    a, b = gpu_ctx.loopdet_detect(items, db_id=8), gpu_ctx.loopdet_detect(items, db_id=9)
    assert sum(r["matched_frame_id"] >= 0 for r in a) > 0
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["matched_frame_id"] == y["matched_frame_id"] and x["score"] == y["score"], k
        assert np.array_equal(x["matched_transform"], y["matched_transform"])
        for p, q in zip(gpu_ctx.loopdet_candidates(k, db_id=8), gpu_ctx.loopdet_candidates(k, db_id=9)):
            assert p["score"] == q["score"] and p["score_shift"] == q["score_shift"] and np.array_equal(p["transform"], q["transform"])
        m = gpu_ctx.loopdet_matches(k, db_id=8)
        assert len(m) == (x["matched_frame_id"] >= 0) and (not m or m[0]["kind"] == lisreg.LOOP_FEPSC)
    assert np.array_equal(gpu_ctx.loopdet_get(3, db_id=8)[0], gpu_ctx.loopdet_get_descriptor(3, "fepsc", db_id=9))


@pytest.mark.gpu
def test_kind_argument_errors(gpu_ctx):
    import lisreg
    L, h = gpu_ctx._L, gpu_ctx._h
    f = _drive()[0]
    gpu_ctx.loopdet_reset(10)
    for bad in (0, 128, 255):
        assert L.lisreg_loopdet_configure(h, 10, bad, 0.79) == lisreg.ERR_ARG
    assert L.lisreg_loopdet_configure(h, -1, 1, 0.79) == lisreg.ERR_ARG
    gpu_ctx.loopdet_configure(["isc", "sc"], db_id=10)
    gpu_ctx.loopdet_detect([(f["corner"], f["surf"], f["semantic"], f["odom"])], db_id=10)
    assert L.lisreg_loopdet_configure(h, 10, lisreg.LOOP_FEPSC, 0.79) == lisreg.ERR_ARG      # not empty
    out = np.zeros(1600, np.uint8)
    u8 = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.lisreg_loopdet_get_descriptor(h, 10, 0, lisreg.LOOP_SSC, u8) == lisreg.ERR_ARG    # not enabled
    assert L.lisreg_loopdet_get_descriptor(h, 10, 0, lisreg.LOOP_POSE, u8) == lisreg.ERR_ARG
    assert L.lisreg_loopdet_get_descriptor(h, 10, 1, lisreg.LOOP_SC, u8) == lisreg.ERR_ARG     # no frame 1
    assert L.lisreg_loopdet_get(h, 10, 0, u8, None) == lisreg.ERR_ARG                           # FEPSC not enabled
    assert L.lisreg_loopdet_get_descriptor(h, 10, 0, lisreg.LOOP_SC, u8) == lisreg.OK
    # ISC reads host intensities: device records are refused, by detect and by the descriptor call
    dev = [lisreg.DeviceArray(lisreg.pack_device_records(x)) for x in (f["corner"], f["surf"], f["semantic"])]
    fr = (lisreg.LoopdetFrame * 1)()
    fr[0].corner, fr[0].n_corner = dev[0].ptr, len(f["corner"])
    fr[0].surf, fr[0].n_surf = dev[1].ptr, len(f["surf"])
    fr[0].semantic, fr[0].n_semantic = dev[2].ptr, len(f["semantic"])
    res = (lisreg.LoopdetResult * 1)()
    assert L.lisreg_loopdet_detect(h, 10, fr, 1, 16, lisreg.FMT_DEVICE, None, res) == lisreg.ERR_ARG
    assert "intensity" in lisreg.lib().lisreg_last_error(h).decode()
    assert L.lisreg_loop_descriptor_kind(h, lisreg.LOOP_ISC, dev[0].ptr, len(f["corner"]), dev[1].ptr, len(f["surf"]), dev[2].ptr,
                                         len(f["semantic"]), 16, lisreg.FMT_DEVICE, None, u8) == lisreg.ERR_ARG
    assert L.lisreg_loop_descriptor_kind(h, 3, None, 0, None, 0, None, 0, 32, lisreg.FMT_XYZIL, None, u8) == lisreg.ERR_ARG
    # reset keeps the configuration: SC stays enabled, FEPSC stays off
    gpu_ctx.loopdet_reset(10)
    gpu_ctx.loopdet_detect([(f["corner"], f["surf"], f["semantic"], f["odom"])], db_id=10)
    assert L.lisreg_loopdet_get_descriptor(h, 10, 0, lisreg.LOOP_SC, u8) == lisreg.OK
    assert L.lisreg_loopdet_get(h, 10, 0, u8, None) == lisreg.ERR_ARG


@pytest.mark.gpu
def test_host_mirror_epsc_generation_kinds():
    exe = os.path.join(ROOT, "lis-slam_amd", "host", "host_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lis-slam_amd", "host")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "EPSCGeneration kinds ok" in out.stdout, out.stdout
