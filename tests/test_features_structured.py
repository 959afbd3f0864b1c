"""Feature extraction on structured sweeps (tests/feature_sweeps.py): ranges on a 1/64 m lattice, so that curvatures tie exactly by
the thousand; dropped column runs of 8 .. 40 columns, so that suppression runs are cut and the `columnDiff < 10` / `> 10` tests take
both sides; rings of 0 .. 18 points; sectors that reach the 20-corner cap; full rings of 4096 columns; range limits hit exactly; and the
IMU de-skew at and beyond the ends of its table.

CPU: the C oracle, the Python mirror and the census agree on such sweeps, and the census shows that every event class really occurs.
GPU: liblisreg against the oracle — the same points in the same order, all fields — through the single call, device records and the
batch; de-skewed coordinates bit for bit."""
import numpy as np
import pytest

import feature_sweeps as fs
from test_features import NAMES, _pd, _records, same_points

DEFAULTS = (0.0, 70.0, 1.0, 0.1)            # min_range, max_range, edge_threshold, surf_threshold

# three 16 x 450 sweeps that meet every floor of the census on their own: short and empty rings, two cap rings, a dense ring
SMALL = [
    dict(h=16, w=450, seed=1, ring_points={0: 18, 5: 1, 6: 0, 7: 0, 11: 5, 15: 13}, cap_rings=(3, 9), ring_kinds={2: "flat", 13: "full"}),
    dict(h=16, w=450, seed=2, ring_points={0: 0, 4: 12, 8: 17, 12: 11, 14: 5, 15: 18}, cap_rings=(2, 13), ring_kinds={1: "flat", 6: "full", 10: "zigzag"}),
    dict(h=16, w=450, seed=3, ring_points={0: 5, 1: 0, 2: 0, 7: 18, 15: 1}, cap_rings=(5, 10), ring_kinds={4: "saw6", 12: "flat"},
         shuffle=True, dup_fraction=0.05, bad_ring_points=20),
]
_cache = {}


def sweep(**kw):
    """a structured sweep, built once per session and handed out read-only"""
    key = repr(sorted(kw.items()))
    if key not in _cache:
        c = fs.structured_sweep(**kw)
        c.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def fparams(mod, h, w, rate=1, rest=DEFAULTS):
    return mod.FeatureParams(h, w, rate, *rest)


def report(tag, cs):
    print(f"census {tag}: {fs.counts_line(cs)}")


def assert_gpu_equals_oracle(oracle, gpu_ctx, c, h, w, rate=1, rest=DEFAULTS):
    import lisreg
    ro = oracle.extract_features(c, fparams(oracle, h, w, rate, rest))
    rg = gpu_ctx.extract_features(c, fparams(lisreg, h, w, rate, rest))
    for k in NAMES:
        assert len(rg[k]) == len(ro[k]), (k, len(rg[k]), len(ro[k]))
        assert same_points(rg[k], c[ro[k]]), k
    return ro, rg


# ---------------------------------------------------------------------------------------------------------------- CPU
@pytest.mark.parametrize("case", range(len(SMALL)))
def test_oracle_mirror_and_census_agree_on_structured_sweeps(oracle, case):
    import lisreg_numpy as ln
    kw = SMALL[case]
    c = sweep(**kw)
    p = fparams(oracle, kw["h"], kw["w"])
    a = oracle.extract_features(c, p)
    b = ln.extract_features(c["x"], c["y"], c["z"], c["ring"], _pd(p))
    cs = fs.census(c, p)
    report(f"small[{case}]", cs)
    for k in NAMES:
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], cs["lists"][k]), k
    assert not fs.floors_missed(cs), fs.floors_missed(cs)
    assert cs["sectors_over_10_surface"] >= 1
    assert int(np.sum(cs["pos_curv"] == 0)) >= 500                              # flat arcs: curvatures exactly zero


def test_generator_ranges_are_exact_and_columns_centred():
    """every range on the lattice bit for bit; limit points exactly on / one ulp outside; columns from the reference's formula"""
    c = sweep(h=8, w=240, seed=5, limits=(13.0, 40.0), n_limit_points=6, bad_ring_points=10)
    r = np.sqrt(c["x"] * c["x"] + c["y"] * c["y"] + c["z"] * c["z"])
    on = r * np.float32(64) == np.round(r * np.float32(64))
    off = np.sort(np.unique(r[~on]))
    assert np.array_equal(off, np.sort([np.nextafter(np.float32(13), np.float32(0)), np.nextafter(np.float32(40), np.float32(np.inf))]))
    assert np.sum(r == np.float32(13)) >= 6 and np.sum(r == np.float32(40)) >= 6
    ha = np.degrees(np.arctan2(c["x"].astype(np.float64), c["y"].astype(np.float64)))
    t = (ha - 90.0) / (360.0 / 240)
    assert np.abs(t - np.round(t)).max() < 1e-3                                 # column centres: far from a rounding boundary
    assert fs.structured_sweep.last_nudges <= 200


def test_census_counts_on_hand_built_rings():
    """the census on inputs small enough to count by hand"""
    # one flat ring of 60 points, columns 0 .. 59, but 10 columns dropped between positions 29 and 30 (column difference 11)
    col = np.concatenate([np.arange(30), np.arange(40, 70)])
    x, y, z, _ = fs.exact_points(col, np.full(60, 12.0), np.full(60, 20.0, np.float32), 240)
    c = np.zeros(60, fs.XYZIRT); c["x"], c["y"], c["z"] = x, y, z
    cs = fs.census(c, dict(n_scan=1, horizon_scan=240, downsample_rate=1, min_range=0.0, max_range=70.0, edge_threshold=1.0, surf_threshold=0.1))
    assert cs["n_extracted"] == 60 and cs["largest_sector"] == 9 and cs["rings_start_after_end"] == 0
    # sp = 4, 12, 20, 29, 37, 45 and ep = 11, 19, 28, 36, 44, 53: the sorted ranges [sp, ep) hold 7, 7, 8, 7, 7, 8 equal curvatures
    assert cs["surf_ties"] == 6 + 6 + 7 + 6 + 6 + 7 and cs["edge_ties"] == 0
    assert cs["pairs_col10"] == 0 and cs["occl_rejected_by_column"] == 0
    assert cs["cut_fwd"] >= 1 and cs["cut_bwd"] >= 1                            # all-zero curvatures: picks 6 apart from sp, some next to the gap
    # the same with 9 dropped columns: difference exactly 10, nothing cut; and a 0.5 m step across it, rejected by the column test alone
    col = np.concatenate([np.arange(30), np.arange(39, 69)])
    tgt = np.concatenate([np.full(30, 20.0), np.full(30, 20.5)]).astype(np.float32)
    x, y, z, _ = fs.exact_points(col, np.full(60, 12.0), tgt, 240)
    c["x"], c["y"], c["z"] = x, y, z
    cs = fs.census(c, dict(n_scan=1, horizon_scan=240, downsample_rate=1, min_range=0.0, max_range=70.0, edge_threshold=1.0, surf_threshold=0.1))
    assert cs["pairs_col10"] == 1 and cs["cut_fwd"] == 0 and cs["cut_bwd"] == 0
    assert cs["occl_rejected_by_column"] == 1 and cs["occl_near_first"] == 0 and cs["occl_near_second"] == 0


# ---------------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(SMALL)))
def test_hip_structured_small_sweeps(oracle, gpu_ctx, case):
    """16 x 450 with every event class of the census at or above its floor (ties, cut runs, pairs exactly 10 apart, occlusion marks and
    column-only rejections, the 21st corner candidate, skipped sectors, short rings)"""
    kw = SMALL[case]
    c = sweep(**kw)
    cs = fs.census(c, fparams(oracle, kw["h"], kw["w"]))
    report(f"small[{case}]", cs)
    assert not fs.floors_missed(cs), fs.floors_missed(cs)
    assert_gpu_equals_oracle(oracle, gpu_ctx, c, kw["h"], kw["w"])


@pytest.mark.gpu
def test_hip_structured_64x1800_rate2(oracle, gpu_ctx):
    kw = dict(h=64, w=1800, seed=11, ring_points={0: 13, 8: 0, 10: 0, 20: 18, 40: 5, 62: 11}, cap_rings=(4, 30), ring_kinds={16: "full", 50: "saw6"})
    c = sweep(**kw)
    cs = fs.census(c, fparams(oracle, 64, 1800, 2))
    report("64x1800 rate 2", cs)
    assert cs["edge_ties"] >= 20 and cs["surf_ties"] >= 200 and cs["cut_fwd"] >= 5 and cs["cut_bwd"] >= 5 and cs["sectors_reaching_21"] >= 2
    assert_gpu_equals_oracle(oracle, gpu_ctx, c, 64, 1800, 2)


@pytest.mark.gpu
def test_hip_structured_32x1024_shuffled_duplicates(oracle, gpu_ctx):
    kw = dict(h=32, w=1024, seed=12, ring_points={0: 17, 9: 0, 31: 12}, cap_rings=(5, 20), ring_kinds={7: "full"}, shuffle=True,
              dup_fraction=0.08, bad_ring_points=50)
    c = sweep(**kw)
    cs = fs.census(c, fparams(oracle, 32, 1024))
    report("32x1024 shuffled", cs)
    assert cs["n_extracted"] < len(c) - 50                                      # duplicates lost their pixel
    assert cs["edge_ties"] >= 20 and cs["surf_ties"] >= 200 and cs["cut_fwd"] >= 5 and cs["cut_bwd"] >= 5
    assert_gpu_equals_oracle(oracle, gpu_ctx, c, 32, 1024)


@pytest.mark.gpu
def test_hip_structured_2x4096_full_rings(oracle, gpu_ctx):
    """both rings hold all 4096 columns: sectors of 681 points (three passes of the rank sort), the LDS window at its limit"""
    c = sweep(h=2, w=4096, seed=13, ring_kinds={0: "full", 1: "full"})
    cs = fs.census(c, fparams(oracle, 2, 4096))
    report("2x4096", cs)
    assert cs["n_extracted"] == 2 * 4096 and cs["largest_sector"] >= 673
    assert cs["edge_ties"] >= 20 and cs["surf_ties"] >= 200
    assert_gpu_equals_oracle(oracle, gpu_ctx, c, 2, 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("edge_thr,surf_thr", [(-1.0, 0.1), (1e30, 1e30)])
def test_hip_structured_8x240_threshold_extremes(oracle, gpu_ctx, edge_thr, surf_thr):
    """every point edge-eligible (a curvature is never below zero) / none edge-eligible and all surface-eligible"""
    c = sweep(h=8, w=240, seed=14, ring_points={3: 13}, drops=(9, 10, 11))
    rest = (0.0, 70.0, edge_thr, surf_thr)
    cs = fs.census(c, fparams(oracle, 8, 240, 1, rest))
    report(f"8x240 edge_threshold {edge_thr}", cs)
    ro, _ = assert_gpu_equals_oracle(oracle, gpu_ctx, c, 8, 240, 1, rest)
    if edge_thr < 0:
        assert cs["edge_ties"] >= 200 and len(ro["corner"]) >= 100
    else:
        assert len(ro["corner"]) == 0 and len(ro["surface_sharp"]) > 0 and cs["surf_ties"] >= 200


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 5, 11, 12, 13, 17, 18])
def test_hip_short_and_empty_rings_among_normal_ones(oracle, gpu_ctx, k):
    """a ring of k points as the first, a middle and the last ring, and two consecutive empty rings, among normal rings"""
    c = sweep(h=16, w=450, seed=20 + k, ring_points={0: k, 7: k, 15: k, 3: 0, 4: 0})
    cs = fs.census(c, fparams(oracle, 16, 450))
    report(f"short rings k={k}", cs)
    assert cs["rings_start_after_end"] == (5 if k < 10 else 2)
    if k == 18:
        assert cs["sectors_skipped_in_live_rings"] >= 3 * 4                     # 4 of the 6 sectors of an 18-point ring have sp >= ep
    ro, _ = assert_gpu_equals_oracle(oracle, gpu_ctx, c, 16, 450)
    assert np.sum(c["ring"][ro["deskewed"]] == 15) == k and np.sum(c["ring"][ro["deskewed"]] == 4) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kinds", [("flat", "saw"), ("flat", "flat", "saw", "zigzag", "pattern")])
def test_hip_column_gaps_of_9_10_11(oracle, gpu_ctx, kinds):
    """runs of 9, 10 and 11 dropped columns (column differences 10, 11, 12) inside and at the edge of flat arcs and saw-teeth; the census
    must show a pick within 5 positions of every such gap, a peak next to some and a flat arc next to others"""
    c = sweep(h=16, w=450, seed=31, drops=(9, 10, 11, 9, 10, 11, 10), steps=False, segment_kinds=kinds)
    cs = fs.census(c, fparams(oracle, 16, 450))
    report(f"gaps {kinds}", cs)
    gaps = fs.gap_pick_distances(cs)
    curv = cs["pos_curv"]
    for cd in (10, 11, 12):
        mine = [(i, d) for i, c_, d in gaps if c_ == cd]
        assert len(mine) >= 8, (cd, len(mine))
        assert max(d for _, d in mine) <= 5, (cd, mine)
        assert any(curv[max(i - 2, 0):i + 4].max() > 1.0 for i, _ in mine), cd       # next to a high-curvature peak
        assert any(curv[max(i - 2, 0):i + 4].max() == 0.0 for i, _ in mine), cd      # inside a flat arc
    assert cs["cut_fwd"] >= 5 and cs["cut_bwd"] >= 5 and cs["pairs_col10"] >= 3
    assert_gpu_equals_oracle(oracle, gpu_ctx, c, 16, 450)


def _positions_of(cloud, got, cs):
    """extracted positions of the points of an output cloud (found by their coordinates and ring)"""
    where = {(float(p["x"]), float(p["y"]), float(p["z"]), int(p["ring"])): i for i, p in enumerate(cloud)}
    pos_of_src = {int(s): k for k, s in enumerate(cs["pos_src"])}
    return np.array([pos_of_src[where[(float(p["x"]), float(p["y"]), float(p["z"]), int(p["ring"]))]] for p in got], np.int64)


@pytest.mark.gpu
def test_hip_corner_and_surface_caps(oracle, gpu_ctx):
    """sectors with >= 25 corner candidates that do not suppress one another — peaks 6 apart, peaks 6 and 7 apart, and candidates
    separated by gaps of 11 columns: exactly 20 corners, of them 4 sharp; a flat ring with 28 surface picks per sector: exactly 10 sharp"""
    c = sweep(h=4, w=1024, seed=41, ring_kinds={0: "saw6", 2: "saw67", 3: "flat"}, cap_rings=(1,))
    cs = fs.census(c, fparams(oracle, 4, 1024))
    report("caps", cs)
    _, rg = assert_gpu_equals_oracle(oracle, gpu_ctx, c, 4, 1024)
    pos = {k: _positions_of(c, rg[k], cs) for k in ("corner", "corner_sharp", "surface_sharp")}
    inside = lambda k, s: int(np.sum((pos[k] >= s["sp"]) & (pos[k] <= s["ep"])))
    capped = [s for s in cs["sectors"] if s["reached_21"]]
    assert {s["ring"] for s in capped} == {0, 1, 2} and len(capped) == 6 + 1 + 6
    for s in capped:
        assert s["edge_candidates"] >= 25, s
        assert inside("corner", s) == 20 and inside("corner_sharp", s) == 4, s
    flat = [s for s in cs["sectors"] if s["ring"] == 3]
    assert len(flat) == 6
    for s in flat:
        assert s["surface_picks"] > 10 and inside("surface_sharp", s) == 10, s


@pytest.mark.gpu
def test_hip_range_limits_and_rings_off_the_lattice(oracle, gpu_ctx):
    """points at min_range and max_range are kept (`<` / `>`), one ulp outside they are dropped; rings >= n_scan and rings off the
    downsample_rate lattice are dropped"""
    lo, hi = np.float32(18.0), np.float32(28.0)
    c = sweep(h=16, w=450, seed=51, limits=(18.0, 28.0), n_limit_points=40, bad_ring_points=60)
    rest = (18.0, 28.0, 1.0, 0.1)
    for rate in (1, 2):
        cs = fs.census(c, fparams(oracle, 16, 450, rate, rest))
        report(f"range limits rate {rate}", cs)
        _, rg = assert_gpu_equals_oracle(oracle, gpu_ctx, c, 16, 450, rate, rest)
        d = rg["deskewed"]
        r_in = np.sqrt(c["x"] * c["x"] + c["y"] * c["y"] + c["z"] * c["z"])
        r_out = np.sqrt(d["x"] * d["x"] + d["y"] * d["y"] + d["z"] * d["z"])
        live = (c["ring"] < 16) & (c["ring"] % rate == 0)
        assert np.sum(r_in[live] == np.nextafter(lo, np.float32(0))) >= 10 and np.sum(r_in[live] == np.nextafter(hi, np.float32(np.inf))) >= 10
        assert np.sum(r_in[live] < lo) > 100 and np.sum(r_in[live] > hi) > 100
        for v in (lo, hi):
            assert np.sum(r_out == v) == np.sum(r_in[live] == v) >= 10          # every point exactly on a limit is kept
        assert r_out.min() == lo and r_out.max() == hi                         # nothing outside, not even by one ulp
        assert d["ring"].max() < 16 and np.all(d["ring"] % rate == 0)


@pytest.mark.gpu
def test_hip_structured_device_records_and_batch(oracle, gpu_ctx):
    """the same sweeps as device records through the single call and stacked in one batch: sweeps whose first and last rings are full
    right up to the boundary, an all-empty sweep between two structured ones, short first and last rings"""
    import lisreg
    h, w = 16, 450
    dense = [sweep(h=h, w=w, seed=60 + k, ring_kinds={0: "full", h - 1: "full"}, cap_rings=(6,)) for k in range(2)]
    zig = sweep(h=h, w=w, seed=63, ring_kinds={0: "zigzag", h - 1: "saw6"})
    sweeps = [dense[0], dense[1], sweep(**SMALL[0]), dense[0][:0], sweep(**SMALL[1]), zig, sweep(**SMALL[2]), dense[1]]
    for c in (dense[0], dense[1], zig):                                        # dense up to the boundary: both end rings hold every column
        assert np.sum(c["ring"] == 0) == w and np.sum(c["ring"] == h - 1) == w
    pg, po = fparams(lisreg, h, w), fparams(oracle, h, w)
    recs = [_records(c) for c in sweeps]
    dins = [lisreg.DeviceArray(r) if len(r) else None for r in recs]
    cap = h * w
    outs = [{k: lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for k in NAMES} for _ in sweeps]
    counts = gpu_ctx.extract_features_batch_device([d.ptr if d else 0 for d in dins], [len(r) for r in recs], pg,
                                                   [{k: v.ptr for k, v in o.items()} for o in outs], cap)
    one = {k: lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for k in NAMES}
    for s, c in enumerate(sweeps):
        ro = oracle.extract_features(c, po)
        single = gpu_ctx.extract_features_device(dins[s].ptr if dins[s] else 0, len(c), pg, {k: v.ptr for k, v in one.items()}, cap)
        for k in NAMES:
            assert counts[s][k] == single[k] == len(ro[k]), (s, k, counts[s][k], single[k], len(ro[k]))
            want = recs[s][ro[k]].tobytes()
            assert lisreg.device_to_host(one[k].ptr, (cap, 4))[: single[k]].tobytes() == want, (s, k, "single")
            assert lisreg.device_to_host(outs[s][k].ptr, (cap, 4))[: counts[s][k]].tobytes() == want, (s, k, "batch")
    assert all(v == 0 for v in counts[3].values()) and counts[2]["corner"] > 0


# ---- IMU de-skew at the ends of the table --------------------------------------------------------------------------------
T_SCAN = 100.0
STAMPS = T_SCAN + np.arange(4, 21) / 256.0          # 17 IMU stamps, 100.015625 .. 100.078125: exact in double, and float32-exact offsets


def _imu_rot(n):
    k = np.arange(n, dtype=np.float64)
    rot = np.stack([0.004 * np.sin(0.7 * k), 0.003 * (1 - np.cos(0.5 * k)), 0.012 * k + 0.002 * np.sin(0.9 * k)], 1)
    rot[0] = 0
    return rot


def _edge_times(n, first_kind):
    """point times on multiples of 1/1024 s in [0, 102/1024]: 0 .. 15 lie before the first stamp (16/1024), 81 .. 102 after the last
    (80/1024), every multiple of 4 from 16 to 80 exactly on a stamp.  The first input point gets a time of the wanted kind."""
    m = (np.arange(n) * 7) % 103
    m[0] = {"before": 3, "after": 97, "on_stamp": 44, "on_first_stamp": 16, "on_last_stamp": 80}[first_kind]
    t = (m / 1024.0).astype(np.float32)
    assert np.array_equal(t.astype(np.float64) * 1024, m)                      # float32-exact, so time_scan_cur + (double)time is exact
    return t, m


@pytest.mark.gpu
@pytest.mark.parametrize("first_kind", ["before", "after", "on_stamp", "on_first_stamp", "on_last_stamp", "one_entry"])
def test_hip_deskew_table_edges(oracle, gpu_ctx, first_kind):
    """findRotation's other branches: a point time before the first IMU stamp (front == 0), after the last, exactly on a stamp; the
    first pixel-owning point (it sets transStartInverse) at each of them; and a table of one entry"""
    import lisreg
    from lisreg import synth
    c = sweep(**SMALL[0]).copy()
    t, m = _edge_times(len(c), "on_stamp" if first_kind == "one_entry" else first_kind)
    c["time"] = t
    stamps = STAMPS[:1] if first_kind == "one_entry" else STAMPS
    rot = _imu_rot(len(STAMPS))[5:6] if first_kind == "one_entry" else _imu_rot(len(STAMPS))
    po, pg = fparams(oracle, 16, 450), fparams(lisreg, 16, 450)
    dko = oracle.make_deskew(stamps, rot[:, 0], rot[:, 1], rot[:, 2], T_SCAN)
    dkg = lisreg.make_deskew(stamps, rot[:, 0], rot[:, 1], rot[:, 2], T_SCAN)
    assert dkg.imu_pointer_cur == len(stamps) - 1
    ro = oracle.extract_features(c, po)
    assert ro["deskewed"].min() == 0                                           # the first input point owns its pixel
    pt = T_SCAN + c["time"][ro["deskewed"]].astype(np.float64)
    if first_kind != "one_entry":                                              # every branch is taken by pixel-owning points
        assert np.sum(pt < STAMPS[0]) > 100 and np.sum(pt > STAMPS[-1]) > 100 and np.sum(np.isin(pt, STAMPS)) > 100
        assert np.sum(pt == STAMPS[0]) > 5 and np.sum(pt == STAMPS[-1]) > 5
        assert np.sum((pt > STAMPS[0]) & (pt < STAMPS[-1]) & ~np.isin(pt, STAMPS)) > 100
    rg = gpu_ctx.extract_features(c, pg, dkg)
    xyz_all = {int(i): v for i, v in zip(ro["deskewed"], oracle.deskew_points(c, dko, ro["deskewed"]))}
    for k in NAMES:
        assert len(rg[k]) == len(ro[k]), k
        want = np.stack([xyz_all[int(i)] for i in ro[k]]) if len(ro[k]) else np.zeros((0, 3), np.float32)
        assert np.array_equal(synth.pcl_xyz(rg[k]), want), k                    # coordinates bit for bit
        for f in ("intensity", "ring", "time"):                                 # everything else is the raw point's
            assert np.array_equal(rg[k][f], c[ro[k]][f]), (k, f)
    moved = np.abs(synth.pcl_xyz(rg["deskewed"]) - synth.pcl_xyz(c[ro["deskewed"]])).max()
    assert (moved < 1e-4) if first_kind == "one_entry" else (moved > 0.5)       # one entry: every point gets the start's rotation
    # device records, the times in a device array of their own
    rec = _records(c)
    din, dt = lisreg.DeviceArray(rec), lisreg.DeviceArray(np.ascontiguousarray(c["time"]))
    cap = 16 * 450
    outs = {k: lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for k in NAMES}
    dkd = lisreg.make_deskew(stamps, rot[:, 0], rot[:, 1], rot[:, 2], T_SCAN, time_device_ptr=dt.ptr)
    nd = gpu_ctx.extract_features_device(din.ptr, len(c), pg, {k: v.ptr for k, v in outs.items()}, cap, dkd)
    for k in NAMES:
        assert nd[k] == len(rg[k]), k
        got = lisreg.device_to_host(outs[k].ptr, (cap, 4), np.float32)[: nd[k]]
        assert np.array_equal(got[:, :3], synth.pcl_xyz(rg[k])), k
