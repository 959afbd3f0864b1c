"""FEPSC loop-closure candidate detection (EPSCGeneration::loopDetection, src/core/epscGeneration.cpp:663-992): the numpy restatement's
quirks on hand-built clouds (CPU), the exported C ABI (CPU), and the device path against the restatement (GPU)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import loopdet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pcl(xyz, label=None):
    from lisreg import synth
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    return synth.to_pcl(xyz, None if label is None else np.asarray(label, np.uint16).reshape(-1))


def empty():
    return pcl(np.zeros((0, 3)))


def polar(r, a, z=0.0):
    """point at distance r whose M_PI + atan2 angle is a (so sector = floor(a / step))."""
    t = a - math.pi
    return [r * math.cos(t), r * math.sin(t), z]


# ---- CPU: the restatement's quirks ---------------------------------------------------------------------------------------------

def test_uchar_counter_wraps():
    # 300 surf points in one cell: psc = 300 mod 256 = 44, esc = 0 -> 100 * 44 / 1 = 4400 mod 256 = 48
    surf = pcl([polar(10.0, 1.0)] * 300)
    f, e, s = R.descriptors(empty(), surf, pcl(np.zeros((0, 3)), []))
    cell = (int((10.0 - 3.0) / R.RING_STEP), int(1.0 / R.SECTOR_STEP))
    assert e[cell] == (100 * 44) % 256
    assert e.sum() == e[cell]


def test_ratio_wraps_mod_256():
    # psc = 3, esc = 0: 300 -> 44; psc = 3, esc = 1: 150
    surf = pcl([polar(10.0, 1.0)] * 3)
    f, e, _ = R.descriptors(empty(), surf, pcl(np.zeros((0, 3)), []))
    cell = (int(7.0 / R.RING_STEP), int(1.0 / R.SECTOR_STEP))
    assert e[cell] == 44
    f, e, _ = R.descriptors(pcl([polar(10.0, 1.0)]), surf, pcl(np.zeros((0, 3)), []))
    assert e[cell] == 150


def test_fepsc_double_truncation():
    # sepsc = 44 (3 points of label 9), epsc = 44: 44 * 0.4 + 44 * 0.6 = 44.00000000000001 -> 44; sepsc 100, epsc 0 -> 40
    p = polar(10.0, 1.0)
    cell = (int(7.0 / R.RING_STEP), int(1.0 / R.SECTOR_STEP))
    f, e, s = R.descriptors(empty(), pcl([p] * 3), pcl([p] * 3, [9] * 3))
    assert (e[cell], s[cell], f[cell]) == (44, 44, int(44 * 0.4 + 44 * 0.6))
    f, e, s = R.descriptors(empty(), empty(), pcl([p], [13]))
    assert (s[cell], f[cell]) == (100, 40)
    # 0.4 * 1 + 0.6 * 0... truncation of a value just under an integer: sepsc 5, epsc 2 -> 2 + 1.2 = 3.2 -> 3
    assert int(np.uint8(np.float64(5) * 0.4 + np.float64(2) * 0.6)) == 3


def test_labels_of_sepsc_and_no_aliasing():
    p = polar(10.0, 1.0)
    cell = (int(7.0 / R.RING_STEP), int(1.0 / R.SECTOR_STEP))
    # 16 / 18 / 19 -> esc; 9, 10, 11, 13, 14 -> psc; 41 (= 9 + 32) maps to 0, not to 40
    _, _, s = R.descriptors(empty(), empty(), pcl([p] * 3, [9, 41, 50]))
    assert s[cell] == 100
    _, _, s = R.descriptors(empty(), empty(), pcl([p] * 2, [13, 18]))
    assert s[cell] == 50


def test_project_last_writer_and_label_filter():
    a = 10.0 * float(R.STEP360) + 0.005
    pts = [polar(5.0, a), polar(6.0, a), polar(7.0, a), polar(8.0, a), polar(0.001, a)]
    pr = R.project(pcl(pts, [13, 18, 9, 17, 13]))
    s = int(np.floor(np.float32(a) / R.STEP360))
    assert pr[s, 0] == 2 and pr[s, 3] == 18                      # labels 9 and 17 skipped; the < 1e-2 m point skipped
    assert np.isclose(pr[s, 1], np.float32(pts[1][0])) and np.isclose(pr[s, 2], np.float32(pts[1][1]))
    assert pr[:, 0].sum() == 2


def test_yaw_search_fallback_and_modulo_wrap():
    zero = np.zeros((360, 4), np.float32)
    # all-zero counts: every shift costs 0 < 100000, the first one (tmp_id - 30) wins
    shift, ang = R.yaw_search(zero, zero, np.float32(0.5))
    assert shift == int(np.floor(np.float32(0.5) / R.STEP360)) - 30
    # counts large enough that no shift beats 100000: the angle is the wrapped yaw times the step
    big = zero.copy(); big[:, 0] = 1000.0
    shift, ang = R.yaw_search(big, zero, np.float32(-0.1))
    a, _ = R.wrap_yaw(np.float32(-0.1))
    assert shift == R.NO_SHIFT and ang == np.float32(a * R.STEP360)
    # a slightly negative yaw: tmp_id ~ 354, shifts reach 383 and read columns wrapped modulo 360
    h = zero.copy(); c = zero.copy()
    h[5, 0] = 7.0; c[(5 + 357) % 360, 0] = 7.0
    a, tmp = R.wrap_yaw(np.float32(-0.05))
    assert tmp > 331
    shift, _ = R.yaw_search(h, c, np.float32(-0.05))
    assert shift % 360 == 357


def test_gate_uses_previous_key_frame_and_strict_thresholds():
    E = R.EPSCGeneration(None)
    # frames at x = 0, 21, 0 (travel 0, 21, 42).  The distance is taken to the PREVIOUS key frame: frame 1 gates frame 0 (its own
    # predecessor, 0 m away, though frame 1 itself is 21 m from it); frame 2 gates frame 1, not frame 0 where it actually is
    assert E.gate(np.float32(0), np.float32(0)) == []
    E.pos.append((0.0, 0.0))
    assert E.gate(np.float32(21), np.float32(0)) == [0]
    E.pos.append((21.0, 0.0))
    assert E.gate(np.float32(0), np.float32(0)) == [1]
    # strictness: a travel of exactly 20 is not enough
    E2 = R.EPSCGeneration(None)
    E2.travel, E2.pos = [0.0], [(0.0, 0.0)]
    assert E2.gate(np.float32(20), np.float32(0)) == []


def test_score_first_wins_ties():
    d = np.zeros((20, 80), np.uint8)
    d[3, 10] = 200
    e = np.zeros((20, 80), np.uint8)
    e[3, 12] = 200
    score, shift = R.distance(d, e)
    assert shift == 2 and score == 1.0
    # two equal candidates: the strict `score > best` keeps the earlier one (selection in EPSCGeneration.loop_detection)
    best, best_id = 0.0, -1
    for i, s in enumerate([0.8, 0.8, 0.7]):
        if s > 0.75 and s > best:
            best, best_id = s, i
    assert best_id == 0


def test_restatement_finds_the_revisit(oracle):
    from lisreg import synth
    frames = synth.make_loop_drive(24, 2)
    E = R.EPSCGeneration(oracle)
    out = [E.loop_detection(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    assert all(o["matched_frame_id"] == -1 and not o["candidates"] for o in out[:24])      # first lap: nothing to close
    hits = [o for o in out[24:] if o["matched_frame_id"] >= 0]
    assert len(hits) >= 16
    for o in hits:
        assert abs(o["matched_frame_id"] - (o["current_frame_id"] - 24)) <= 1


def test_library_exports_loopdet_symbols():
    import lisreg
    L = C.CDLL(lisreg.LIB_PATH)
    for s in ("lisreg_loopdet_default_params", "lisreg_loopdet_reset", "lisreg_loopdet_detect", "lisreg_loopdet_candidates",
              "lisreg_loopdet_get", "lisreg_loop_descriptor"):
        assert hasattr(L, s), s
    p = lisreg.loopdet_default_params()
    assert (p.skip_neighbour_distance, p.inflation_covariance, p.distance_threshold) == (20.0, 0.01, 0.75)
    assert C.sizeof(lisreg.LoopdetFrame) == 96 and C.sizeof(lisreg.LoopdetResult) == 88 and C.sizeof(lisreg.LoopdetCandidate) == 104


# ---- GPU ----------------------------------------------------------------------------------------------------------------------

def _keep_off_edges(cloud, M, margin=1e-4):
    """drop points within margin sector widths of a sector edge (80 and 360 sectors) under M: atan2 ulps must not decide a bin."""
    if len(cloud) == 0:
        return cloud
    x, y, _ = R._moved(cloud, M)
    a = math.pi + np.arctan2(y.astype(np.float64), x.astype(np.float64))
    keep = np.ones(len(cloud), bool)
    for step in (R.SECTOR_STEP, 2 * math.pi / 360):
        f = a / step
        keep &= np.abs(f - np.round(f)) > margin
    return cloud[keep]


def _frame_clouds(seed, n_sem=6000):
    from lisreg import synth
    rng = np.random.default_rng(seed)
    s = synth.make_scan(16, 360, seed=seed, labelled=True)
    n = n_sem
    r = np.concatenate([rng.uniform(0, 70, n - 8), [3.0, 60.0, 3.0, 60.0, 0.0, 2.99, 59.99, 1e-3]])
    t = rng.uniform(-math.pi, math.pi, n)
    xyz = np.stack([r * np.cos(t), r * np.sin(t), rng.uniform(-2, 5, n)], 1)
    lab = rng.integers(0, 60, n)                 # labels >= 20 included
    sem = synth.concat_clouds([synth.to_pcl(xyz.astype(np.float32), lab.astype(np.uint16)), s["corner"], s["surf"]])
    return s["corner"], s["surf"], sem


MATRICES = [None,
            np.eye(4, dtype=np.float32),
            np.array([[0.8, -0.6, 0, 1.5], [0.6, 0.8, 0, -2.25], [0, 0, 1, 0.1], [0, 0, 0, 1]], np.float32),
            np.array([[math.cos(2.9), -math.sin(2.9), 0.01, -4.0], [math.sin(2.9), math.cos(2.9), 0, 3.0], [0, 0.02, 1, 0],
                      [0, 0, 0, 1]], np.float32)]


@pytest.mark.gpu
def test_descriptors_exact(gpu_ctx):
    import lisreg
    for seed in (1, 2):
        corner, surf, sem = _frame_clouds(seed)
        for M in MATRICES:
            c, s, m = (_keep_off_edges(x, M) for x in (corner, surf, sem))
            fe, ep, se = R.descriptors(c, s, m, M)
            pr = R.project(m, M)
            out = gpu_ctx.loop_descriptor(c, s, m, M)
            assert np.array_equal(out["epsc"], ep) and np.array_equal(out["sepsc"], se) and np.array_equal(out["fepsc"], fe), (seed, M)
            assert np.array_equal(out["projection"], pr), (seed, M)
            # the same through device records
            devs = [lisreg.DeviceArray(lisreg.pack_device_records(x)) if len(x) else None for x in (c, s, m)]
            out_d = gpu_ctx.loop_descriptor(*[(d.ptr, len(x)) if d is not None else (0, 0) for d, x in zip(devs, (c, s, m))], M)
            for k in ("fepsc", "epsc", "sepsc", "projection"):
                assert np.array_equal(out_d[k], out[k]), k
    out = gpu_ctx.loop_descriptor(empty(), empty(), pcl(np.zeros((0, 3)), []))
    assert not out["fepsc"].any() and not out["projection"].any()


def _drive():
    from lisreg import synth
    return synth.make_loop_drive(24, 3, h=16, w=361)          # 361 columns: azimuths off the 4.5 / 1 degree sector edges


@pytest.mark.gpu
def test_end_to_end_against_restatement(gpu_ctx, oracle):
    frames = _drive()
    E = R.EPSCGeneration(oracle)
    ref = [E.loop_detection(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    gpu_ctx.loopdet_reset(0)
    got = gpu_ctx.loopdet_detect([(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames], db_id=0)
    n_cand = 0
    for k, (r, g) in enumerate(zip(ref, got)):
        assert g["current_frame_id"] == r["current_frame_id"] == k
        cands = gpu_ctx.loopdet_candidates(k, db_id=0)
        assert [c["history_id"] for c in cands] == [c["history_id"] for c in r["candidates"]], k
        assert g["n_candidates"] == len(cands)
        n_cand += len(cands)
        for c, rc in zip(cands, r["candidates"]):
            # the yaw search and ICP are held exact where both 1 x 360 projections are (a point within atan2 ulps of a 1-degree edge
            # can move one count, and a near-tie of the count search then picks a neighbouring shift): test_icp_2d_exact
            same_proj = all(np.array_equal(gpu_ctx.loopdet_get(j, db_id=0)[1], E.proj[j]) for j in (k, c["history_id"]))
            if same_proj:
                assert c["yaw_shift"] == rc["shift"] and c["yaw_angle"] == rc["angle"], k
                assert c["icp_state"] == rc["state"] and c["icp_iters"] == rc["iters"] and c["icp_n_corr"] == rc["n_corr"], k
                assert np.abs(c["transform"] - rc["T"]).max() <= 1e-3, (k, c["transform"], rc["T"])
            assert abs(c["score"] - rc["score"]) <= 5e-3, (k, c["score"], rc["score"])
        scores = sorted((c["score"] for c in r["candidates"]), reverse=True)
        decisive = len(scores) < 2 or scores[0] - scores[1] > 1e-2
        if decisive and (not scores or abs(scores[0] - 0.75) > 5e-3):
            assert g["matched_frame_id"] == r["matched_frame_id"], k
        if r["matched_frame_id"] < 0 and not r["candidates"]:
            assert g["matched_frame_id"] == -1
        if g["matched_frame_id"] >= 0 and g["matched_frame_id"] == r["matched_frame_id"]:
            assert np.abs(g["matched_transform"] - r["matched_transform"]).max() <= 1e-3
        d, pr = gpu_ctx.loopdet_get(k, db_id=0)
        f = frames[k]
        assert np.array_equal(d, gpu_ctx.loop_descriptor(f["corner"], f["surf"], f["semantic"])["fepsc"])   # stored: untransformed clouds
        assert np.count_nonzero(d != E.fepsc[k]) <= 16, k             # cells decided by a point within atan2 ulps of a sector edge
    assert n_cand >= 40
    assert sum(g["matched_frame_id"] >= 0 for g in got) >= 30


@pytest.mark.gpu
def test_icp_2d_exact(gpu_ctx, oracle):
    """frames at X, Y (21 m away), X: frame 2 gates frame 1 (the gate measures from the previous key frame); with every point off the
    1-degree edges the projections are exact, so the yaw shift is exact and trans * trans1 is within 1e-3 of the oracle ICP's."""
    from lisreg import synth
    for seed, yaw1, yaw2 in ((3, 0.2, 0.5), (4, 0.1, -0.05), (5, 1.0, -2.5), (6, 0.0, 0.0)):
        clouds = []
        for j, (x, yaw) in enumerate(((0.0, 0.0), (21.0, yaw1), (0.0, yaw2))):
            c, s_, m = _frame_clouds(seed * 10 + j, n_sem=3000)
            clouds.append([_keep_off_edges(v, None, 1e-3) for v in (c, s_, m)] + [synth.pose_matrix([0, 0, yaw, x, 0, 0])[:3].astype(np.float32)])
        E = R.EPSCGeneration(oracle)
        ref = [E.loop_detection(*f) for f in clouds]
        gpu_ctx.loopdet_reset(4)
        got = gpu_ctx.loopdet_detect([tuple(f) for f in clouds], db_id=4)
        assert [len(r["candidates"]) for r in ref] == [g["n_candidates"] for g in got] == [0, 1, 1]
        for k in (1, 2):
            (c,), rc = gpu_ctx.loopdet_candidates(k, db_id=4), ref[k]["candidates"][0]
            assert np.array_equal(gpu_ctx.loopdet_get(k, db_id=4)[1], E.proj[k])
            assert c["history_id"] == rc["history_id"] and c["yaw_shift"] == rc["shift"] and c["yaw_angle"] == rc["angle"], (seed, k)
            assert c["icp_state"] == rc["state"] and c["icp_iters"] == rc["iters"] and c["icp_n_corr"] == rc["n_corr"], (seed, k)
            assert np.abs(c["transform"] - rc["T"]).max() <= 1e-3, (seed, k, c["transform"], rc["T"])
            assert abs(c["score"] - rc["score"]) <= 5e-3


@pytest.mark.gpu
def test_batch_equals_sequential(gpu_ctx):
    frames = _drive()[:60]
    items = [(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    gpu_ctx.loopdet_reset(1)
    batch = gpu_ctx.loopdet_detect(items, db_id=1)
    cb = [gpu_ctx.loopdet_candidates(k, db_id=1) for k in range(len(items))]
    gpu_ctx.loopdet_reset(2)
    for k, it in enumerate(items):
        one = gpu_ctx.loopdet_detect([it], db_id=2)[0]
        assert one["current_frame_id"] == batch[k]["current_frame_id"]
        assert one["matched_frame_id"] == batch[k]["matched_frame_id"] and one["score"] == batch[k]["score"], k
        assert np.array_equal(one["matched_transform"], batch[k]["matched_transform"]), k
        c1 = gpu_ctx.loopdet_candidates(0, db_id=2)
        assert len(c1) == len(cb[k])
        for a, b in zip(c1, cb[k]):
            assert a["history_id"] == b["history_id"] and a["score"] == b["score"] and np.array_equal(a["transform"], b["transform"])
    # reset starts over: the same frames give the same answers again
    gpu_ctx.loopdet_reset(1)
    again = gpu_ctx.loopdet_detect(items[:30], db_id=1)
    for a, b in zip(again, batch[:30]):
        assert a["matched_frame_id"] == b["matched_frame_id"] and a["score"] == b["score"]


@pytest.mark.gpu
def test_argument_errors(gpu_ctx):
    import lisreg
    L, h = gpu_ctx._L, gpu_ctx._h
    fr = (lisreg.LoopdetFrame * 1)()
    res = (lisreg.LoopdetResult * 1)()
    assert L.lisreg_loopdet_reset(h, -1) == lisreg.ERR_ARG
    assert L.lisreg_loopdet_reset(h, lisreg.LOOPDET_MAX_DB) == lisreg.ERR_ARG
    assert L.lisreg_loopdet_detect(h, 99, fr, 1, 32, lisreg.FMT_XYZIL, None, res) == lisreg.ERR_ARG
    fr[0].n_corner = 5                                     # NULL cloud with n > 0
    assert L.lisreg_loopdet_detect(h, 0, fr, 1, 32, lisreg.FMT_XYZIL, None, res) == lisreg.ERR_ARG
    gpu_ctx.loopdet_reset(3)
    d = np.zeros(1600, np.uint8)
    assert L.lisreg_loopdet_get(h, 3, 0, d.ctypes.data_as(C.POINTER(C.c_uint8)), None) == lisreg.ERR_ARG
    n = C.c_int(0)
    assert L.lisreg_loopdet_candidates(h, 3, 0, None, 0, C.byref(n)) == lisreg.ERR_ARG
    assert L.lisreg_loop_descriptor(h, None, 3, None, 0, None, 0, 32, lisreg.FMT_XYZIL, None, None, None, None, None) == lisreg.ERR_ARG


@pytest.mark.gpu
def test_host_mirror_epsc_generation():
    exe = os.path.join(ROOT, "lis-slam_amd", "host", "host_smoke")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "lis-slam_amd", "host")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "EPSCGeneration ok" in out.stdout, out.stdout
