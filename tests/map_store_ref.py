"""Planted sequences for the device-resident map stores (lisreg_localmap_*, lisreg_submap_*, lisreg_keyframes_*) and their census.

A case is a short list of operations over small clouds whose coordinates are multiples of 1/64 m, under poses whose translations
are exact, so that "this point lies ON the threshold" is a property of the input.  Expected values come from the restatement
(oracle/replay_oracle.py: LocalMapOracle, SubMapOracle, extract_submap_cloud, submap_crop_boxes) with the case's parameters passed
through; the ring's restatement (ring_push / ring_target) lives here.  Every planted point carries its own label (the 16-bit payload
of a device record travels through transform, filter, crop and a one-point voxel unchanged), which is how the census finds it again.

run_localmap / run_submaps / run_ring execute a case on the restatement and return one expected state per operation;
census_* assert FROM THOSE STATES ALONE that the branch the case exists for was reached.  The GPU tests compare the device with
the same states, so a case that stops reaching its branch fails on the CPU instead of passing empty on the GPU."""
from __future__ import annotations

import functools

import numpy as np

FLT_MAX = 3.4028234663852886e38
Q = 1.0 / 64
LEAF_TOO_SMALL = 3

# poses are (roll, pitch, yaw, x, y, z); the angles are dyadic too, the translations exact
LEVEL_A = (0.0, 0.0, 0.0, 1.0, -2.0, 0.5)
LEVEL_B = (0.0, 0.0, 0.0, -2.0, 3.0, 0.25)
LEVEL_C = (0.0, 0.0, 0.0, 0.5, 0.5, -0.25)
TILTED = (0.03125, -0.046875, 0.40625, 3.0, -1.5, 0.25)          # all three angles non-zero
TILTED_2 = (-0.0625, 0.03125, -0.28125, -1.0, 2.5, 0.5)

DEFAULTS = dict(max_num_pts=80000, on=1, r=30.0, tmin=0.3, tmax=3.0, near=0.03, leaf=(0.1, 0.05, 0.4, 0.2, 0.6),
                crop_box=(-70.0, -70.0, -10.0, 70.0, 70.0, 20.0), pad=2.0)


def params(**over):
    p = dict(DEFAULTS)
    p.update(over)
    return p


def device_params(prm):
    import lisreg
    P = lisreg.localmap_default_params()
    P.max_num_pts, P.dynamic_removal_on, P.dynamic_removal_center_radius = prm["max_num_pts"], prm["on"], prm["r"]
    P.dynamic_dist_thre_min, P.dynamic_dist_thre_max, P.near_dist_thre = prm["tmin"], prm["tmax"], prm["near"]
    for k in range(5):
        P.leaf[k] = prm["leaf"][k]
    for k in range(6):
        P.crop_box[k] = prm["crop_box"][k]
    P.crop_pad = prm["pad"]
    return P


def insert_kw(prm):
    return dict(max_num_pts=prm["max_num_pts"], dynamic_removal_on=bool(prm["on"]), center_radius=prm["r"], thre_min=prm["tmin"],
                thre_max=prm["tmax"], near_thre=prm["near"])


def extract_kw(prm):
    return dict(leaf=prm["leaf"], crop_box=prm["crop_box"], pad=prm["pad"])


# ---- clouds ---------------------------------------------------------------------------------------------------------------
def mk(xyz, tag):
    """PointXYZIL structs at multiples of 1/64 m; tag = the label, one value or one per point."""
    from lisreg import synth
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    assert np.array_equal(xyz * 64, np.round(xyz * 64)), "coordinates must be multiples of 1/64 m"
    return synth.to_pcl(xyz.astype(np.float32), np.broadcast_to(np.asarray(tag, np.uint16), (len(xyz),)))


def empty():
    return mk(np.zeros((0, 3)), 0)


def seen_from(xyz_map, pose):
    """Sensor-frame coordinates of map-frame points.  Level pose: exact.  Otherwise rounded to 1/64 m — the transformed point then
    lies within 1/64 m * sqrt(3) / 2 of where it was meant, which such cases allow for."""
    from lisreg import synth
    xyz_map = np.asarray(xyz_map, np.float64).reshape(-1, 3)
    if pose[0] == 0 and pose[1] == 0 and pose[2] == 0:
        return xyz_map - np.asarray(pose[3:6], np.float64)
    M = np.linalg.inv(synth.pose_matrix(np.asarray(pose, np.float64)))
    return np.round((xyz_map @ M[:3, :3].T + M[:3, 3]) * 64) / 64


def tags(cloud):
    return set(int(v) for v in cloud["label"])


def lattice(n, seed, pitch=0.125, z=0.0):
    """n points of a square lattice of the given pitch around the origin, each moved by a seeded multiple of 1/64 m (|.| <= 2/64)."""
    side = int(np.ceil(np.sqrt(n)))
    i = np.arange(n)
    rng = np.random.default_rng(seed)
    xyz = np.stack([(i % side - side // 2) * pitch, (i // side - side // 2) * pitch, np.full(n, z)], 1)
    return xyz + rng.integers(-2, 3, (n, 3)) * Q


# ---- the planted frames of the local-map cases ----------------------------------------------------------------------------
# map-frame anchors: the map's dynamic points.  8 m apart, so a point planted within 3 m of one has that one as its nearest
GRID = [(0, 0), (8, 0), (-8, 0), (0, 8), (0, -8), (8, 8), (-8, -8), (8, -8), (-8, 8)]
ANCHORS = np.array([(x, y, 0.0) for x, y in GRID] + [(5.125, 12.0, 0.0), (12.0, 5.25, 0.0), (-4.0, 4.0, 0.0)])
R = 13.0                                                    # (5, 12, 0) lies exactly on x^2 + y^2 == R^2


def _filler(extra_ground=0):
    pole = [(-15.0, 15.0, 0.25 * k) for k in range(20)]
    ground = [(float(i), float(j), -1.5) for i in range(-5, 5) for j in range(-5, 5)]
    ground += [(50.0 + k, 0.0, -1.5) for k in range(extra_ground)]
    building = [(20.0, float(j), float(k)) for j in range(-8, 9) for k in range(4)]
    outlier = [(30.0 + k, 30.0, 1.0) for k in range(7)]
    return pole, ground, building, outlier


def frame(pose, dynamic=(), pole=(), ground=(), building=(), outlier=(), dyn_tags=None, tag0=0):
    """The five class clouds (dynamic, pole, ground, building, outlier) of a frame whose points are given in the MAP frame."""
    out = []
    for k, pts in enumerate((dynamic, pole, ground, building, outlier)):
        pts = np.asarray(pts, np.float64).reshape(-1, 3)
        t = dyn_tags if (k == 0 and dyn_tags is not None) else tag0 + 10 * (k + 1)
        out.append(mk(seen_from(pts, pose), t) if len(pts) else empty())
    return out


def first_frame(extra_ground=0):
    """200 + extra_ground points in the four classes a local map keeps, 7 outliers it does not."""
    pole, ground, building, outlier = _filler(extra_ground)
    return frame(LEVEL_A, ANCHORS, pole, ground, building, outlier, dyn_tags=100 + np.arange(len(ANCHORS)))


# the second frame's dynamic points, by distance to their anchor (along z, so x^2 + y^2 is the anchor's)
PLANT_D = [0.125, 0.25, 0.375, 0.5, 1.0, 2.0, 2.0 + Q, 2.5]          # near = 0.25, min = 0.5, max = 2.0
PLANT_TAG = dict(below_near=200, on_near=201, near_to_min=202, on_min=203, band=204, on_max=205, above_max=206, far=207,
                 on_circle=208, outside_circle=209, below_near_2=210, far_2=211)
PLANT_DROP = {200, 201, 203, 204, 205, 208, 210}
PLANT_KEEP = {202, 206, 207, 209, 211}


def planted_frame(pose=LEVEL_B):
    pts = [ANCHORS[i] + (0, 0, d) for i, d in enumerate(PLANT_D)]
    pts += [(5.0, 12.0, 0.0), (12.0, 5.125, 0.0), ANCHORS[8] + (0, 0, 0.125), ANCHORS[11] + (0, 0, 3.0)]
    return frame(pose, pts, ground=[(30.0, -30.0, -1.5), (31.0, -30.0, -1.5), (32.0, -30.0, -1.5)], dyn_tags=200 + np.arange(12))


THRESH = params(max_num_pts=1003, r=R, tmin=0.5, tmax=2.0, near=0.25, leaf=(0.5, 0.125, 0.5, 0.25, 1.0),
                crop_box=(-24.0, -16.0, -4.0, 40.0, 28.0, 8.0), pad=1.0)


def case_at_threshold():
    """feature_point_num == max_num_pts / 5 (1003 / 5 = 200 in integers, 200.6 otherwise): the filter must NOT run."""
    return dict(name="at_threshold", prm=THRESH, ops=[("insert", first_frame(0), LEVEL_A), ("insert", planted_frame(), LEVEL_B)])


def case_above_threshold():
    """feature_point_num one above max_num_pts / 5: the filter runs, on every threshold's both sides; then a dynamic cloud of 10
    (unfiltered) and one of 11 that is removed completely; extract under a tilted pose, extract again, insert, extract without a slot."""
    band = lambda dz, idx: [ANCHORS[i] + (0, 0, dz) for i in idx]
    ops = [("insert", first_frame(1), LEVEL_A),
           ("insert", planted_frame(), LEVEL_B),
           ("insert", frame(TILTED, band(1.0, range(9)) + [ANCHORS[11] + (0, 0, 1.0)], dyn_tags=300 + np.arange(10)), TILTED),
           ("insert", frame(LEVEL_C, band(-1.0, range(9)) + [ANCHORS[11] + (0, 0, -1.0), ANCHORS[0] + (0, 0, -1.25)],
                            pole=[(-15.0, 15.0, 6.0), (-15.0, 15.0, 6.5)],
                            ground=[(2.5, 2.5, -1.5), (2.5 + Q, 2.5, -1.5), (2.5, 2.5 + Q, -1.5), (2.5 + Q, 2.5 + Q, -1.5)],     # one voxel
                            dyn_tags=400 + np.arange(11)), LEVEL_C),
           ("extract", TILTED, 0),
           ("extract", TILTED, 0),
           ("insert", frame(LEVEL_B, band(-1.0, range(6)) + band(-3.0, range(6)), building=[(20.0, 0.5, 0.5)], dyn_tags=500 + np.arange(12)), LEVEL_B),
           ("extract", LEVEL_C, -1)]
    return dict(name="above_threshold", prm=THRESH, ops=ops)


# the band cases: one pair of frames under four parameter sets
BAND_D = [1.0 + Q, 1.0625, 1.09375, 1.109375, 1.125, 0.5, 1.0, 0.125, 0.25, 3.0, 0.375, 2.0]      # (anchors 9 and 10 lie outside the circle)
BAND = dict(widen=params(max_num_pts=103, r=R, tmin=1.0, tmax=1.0, near=0.25),
            off=params(max_num_pts=103, on=0, r=R, tmin=1.0, tmax=1.0, near=0.25),
            fltmax=params(max_num_pts=103, r=R, tmin=FLT_MAX, tmax=FLT_MAX, near=0.25),
            radius_fltmax=params(max_num_pts=103, r=FLT_MAX, tmin=0.5, tmax=2.0, near=0.0))


def case_band(kind):
    """widen: min = max = 1 -> the band reaches (float)(1 + 0.1); points at 1 + 1/64 .. 1.09375 fall to the widening alone.
    off: dynamic_removal_on = 0 above the threshold.  fltmax / radius_fltmax: thresholds of FLT_MAX (their squares are +inf)."""
    f1 = frame(LEVEL_A, ANCHORS, ground=[(float(i), -3.0, -1.5) for i in range(10)], dyn_tags=100 + np.arange(12))
    f2 = frame(LEVEL_B, [ANCHORS[i] + (0, 0, d) for i, d in enumerate(BAND_D)], dyn_tags=600 + np.arange(12))
    return dict(name="band_" + kind, prm=BAND[kind], ops=[("insert", f1, LEVEL_A), ("insert", f2, LEVEL_B), ("extract", LEVEL_A, 0)])


def case_empty_dynamic():
    """The map's dynamic class is empty when the filter condition holds: no filter (the restatement's reading is the rule)."""
    f1 = frame(LEVEL_A, ground=[(float(i), float(j), -1.5) for i in range(6) for j in range(5)])
    f2 = frame(LEVEL_B, ANCHORS, dyn_tags=100 + np.arange(12))
    f3 = frame(LEVEL_C, [ANCHORS[i] + (0, 0, d) for i, d in enumerate(PLANT_D)] + [ANCHORS[k] + (0, 0, -1.0) for k in (8, 9, 10, 11)],
               dyn_tags=200 + np.arange(12))
    return dict(name="empty_dynamic", prm=params(max_num_pts=103, r=R, tmin=0.5, tmax=2.0, near=0.25),
                ops=[("insert", f1, LEVEL_A), ("insert", f2, LEVEL_B), ("insert", f3, LEVEL_C), ("extract", LEVEL_A, 0)])


FAR = (1408.0, 1408.0, 128.0)             # 28161 x 28161 x 2561 voxels of 0.05 m: more than INT_MAX
POLE_TRIO = [(0.0, 0.0, 0.0), (Q, 0.0, 0.0), (0.0, Q, 0.0)]         # one voxel of 0.05 m, had the grid run


def case_leaf_too_small():
    """Pole points 2 000 m apart at the default 0.05 m: PCL refuses the grid and hands the class through; its neighbours are gridded."""
    f = frame(LEVEL_A, dynamic=[(4.0, 4.0, 0.0), (4.0 + Q, 4.0, 0.0), (6.0, 6.0, 0.0)], pole=POLE_TRIO + [FAR],
              ground=[(2.5, 2.5, -1.5), (2.5 + Q, 2.5, -1.5), (5.0, 5.0, -1.5)], building=[(9.0, 0.0, 1.0), (9.0, Q, 1.0), (9.0, 3.0, 1.0)],
              dyn_tags=100 + np.arange(3))
    f[1]["label"] = 700 + np.arange(4)
    return dict(name="leaf_too_small", prm=params(), ops=[("insert", f, LEVEL_A), ("extract", LEVEL_B, 0), ("extract", LEVEL_B, 0)])


PAD0_GROUND = dict(x_min=(-4.0, 0.0, 0.0), on_crop_face=(9.0, 0.5, 0.0), inside_crop_face=(9.0 - Q, 1.0, 0.25),
                   outside_crop_face=(9.0 + Q, -1.0, 0.25), far_outside=(12.0, 0.0, 0.5), y_max=(0.0, 3.0, 0.0), y_min=(0.0, -3.0, 0.0),
                   z_max=(0.0, 0.0, 1.0), z_min=(0.0, 0.0, -1.0), interior_1=(1.0, 1.0, 0.5), interior_2=(2.0, -1.0, -0.5))
PAD0_DROP = ("x_min", "on_crop_face", "outside_crop_face", "far_outside", "y_max", "y_min", "z_max", "z_min")
PAD0_KEEP = ("inside_crop_face", "interior_1", "interior_2")
PAD0_POSE = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def case_pad_zero():
    """crop_pad = 0: the intersection box's faces are the map's own extremes (and, in +x, the crop box's face at 8 + 1 = 9 m);
    bbx_filter is strictly inside, so the points ON the faces go."""
    f = frame(LEVEL_A, dynamic=[(1.0, -1.0, 0.25)], pole=[(2.0, 2.0, 0.25)], ground=list(PAD0_GROUND.values()), dyn_tags=np.array([100]))
    f[2]["label"] = 800 + np.arange(len(PAD0_GROUND))
    prm = params(crop_box=(-8.0, -64.0, -64.0, 8.0, 64.0, 64.0), pad=0.0)
    return dict(name="pad_zero", prm=prm, ops=[("insert", f, LEVEL_A), ("extract", PAD0_POSE, 0)])


def case_after_reset():
    return dict(name="after_reset", prm=params(), ops=[("extract", TILTED, 0), ("insert", first_frame(0), LEVEL_A), ("reset",), ("extract", LEVEL_A, -1)])


def localmap_cases():
    return [case_at_threshold(), case_above_threshold()] + [case_band(k) for k in BAND] + \
           [case_empty_dynamic(), case_leaf_too_small(), case_pad_zero(), case_after_reset()]


# ---- running a case on the restatement ------------------------------------------------------------------------------------
def _copy(cls):
    """The class clouds as they stand (the restatement replaces a class's array on every change and never writes into one)."""
    return list(cls)


def run_localmap(case, submap=False):
    """One expected state per operation.  insert: n, fpn, bound, cls, and for the census fpn_before, dyn_before, moved_dyn (the frame's
    dynamic cloud in the map frame, before any filter).  extract: corner / surf target, crop, cls, and grid_rc / grid_n per class."""
    import oracle_ctypes as oc
    import replay_oracle as ro
    from lisreg import synth
    prm = case["prm"]
    lm = ro.LocalMapOracle(synth.PCL_DTYPE)
    states = []
    for op in case["ops"]:
        if op[0] == "reset":
            lm = ro.LocalMapOracle(synth.PCL_DTYPE)
            states.append(dict(kind="reset"))
        elif op[0] == "insert":
            _, clouds, pose = op
            st = dict(kind="insert", fpn_before=lm.feature_point_num, dyn_before=lm.cls[0], frame=clouds,
                      moved_dyn=oc.transform_cloud(clouds[0], pose, fmt=1) if len(clouds[0]) else clouds[0])
            lm.insert(clouds, np.asarray(pose, np.float32), **insert_kw(prm))
            st.update(n=[len(c) for c in lm.cls], fpn=lm.feature_point_num, bound=lm.bound.copy(), cls=_copy(lm.cls))
            states.append(st)
        else:
            _, pose, slot = op
            grid = [oc.voxel_grid(c, float(np.float32(prm["leaf"][k])), fmt=1) if len(c) else (0, c) for k, c in enumerate(lm.cls)]
            st = dict(kind="extract", slot=slot, n_before=[len(c) for c in lm.cls], cls_before=_copy(lm.cls),
                      grid_rc=[g[0] for g in grid], grid_n=[len(g[1]) for g in grid], gridded=[g[1] for g in grid])
            tc, ts, isect = lm.extract(np.asarray(pose, np.float32), **extract_kw(prm))
            st.update(tc=tc, ts=ts, crop=isect, n=[len(c) for c in lm.cls], fpn=lm.feature_point_num, bound=lm.bound.copy(), cls=_copy(lm.cls))
            states.append(st)
    return states


def would_drop(st, prm, widened=True):
    """The tags of the frame's dynamic points that map_scan_feature_pts_distance_removal drops, from the restatement's own filter run
    on the state's inputs (widened = the band as the reference widens it; False = the parameters as given)."""
    import oracle_ctypes as oc
    f = np.float32
    tmax = f(prm["tmax"])
    if widened:
        tmax = max(tmax, f(np.float64(f(prm["tmin"])) + 0.1))
    if len(st["moved_dyn"]) <= 10 or len(st["dyn_before"]) == 0:
        # (what the filter WOULD do to a larger cloud against this map: pad the frame with copies of its last point)
        if len(st["dyn_before"]) == 0 or len(st["moved_dyn"]) == 0:
            return set()
        import replay_oracle as ro
        pad = ro.cat([st["moved_dyn"]] + [st["moved_dyn"][-1:]] * 11)
        kept, _ = oc.dynamic_filter(st["dyn_before"], pad, prm["r"], float(f(prm["tmin"])), float(tmax), float(f(prm["near"])))
        return tags(st["moved_dyn"]) - tags(kept)
    kept, _ = oc.dynamic_filter(st["dyn_before"], st["moved_dyn"], prm["r"], float(f(prm["tmin"])), float(tmax), float(f(prm["near"])))
    return tags(st["moved_dyn"]) - tags(kept)


def appended_dyn(st):
    """Tags of the frame's dynamic points that reached the map in this insert."""
    return tags(st["cls"][0][len(st["dyn_before"]):])


# ---- census: local map -----------------------------------------------------------------------------------------------------
def census_localmap(case, states):
    """Asserts that the case's input still reaches the branch it exists for.  Returns the names of the branches proven."""
    name, prm = case["name"], case["prm"]
    thr = prm["max_num_pts"] // 5
    proven = []
    if name == "at_threshold":
        a, b = states
        assert prm["max_num_pts"] % 5 != 0 and thr != round(prm["max_num_pts"] / 5), "the integer division must matter"
        assert b["fpn_before"] == a["fpn"] == thr
        assert a["n"][4] == 0 and len(a["frame"][4]) > 0, "a local map does not take the outlier class"
        assert would_drop(b, prm) == PLANT_DROP, "the planted points must be ones a running filter drops"
        assert appended_dyn(b) == PLANT_DROP | PLANT_KEEP, "the filter ran at feature_point_num == max_num_pts / 5"
        proven += ["filter_not_run_at_threshold", "outlier_not_appended"]
    elif name == "above_threshold":
        a, b, c10, d11, e1, e2, ins, e3 = states
        assert b["fpn_before"] == thr + 1 and len(b["moved_dyn"]) > 10
        got = appended_dyn(b)
        assert got == PLANT_KEEP and tags(b["moved_dyn"]) - got == PLANT_DROP
        T = PLANT_TAG                                            # one dropped and one kept on each side of every threshold
        for dropped, kept in ((T["below_near"], T["near_to_min"]), (T["on_near"], T["near_to_min"]), (T["on_min"], T["near_to_min"]),
                              (T["band"], T["above_max"]), (T["on_max"], T["above_max"]), (T["on_circle"], T["outside_circle"])):
            assert dropped not in got and kept in got
        proven += ["filter_ran_one_above_threshold", "near", "min", "max", "centre_radius"]
        # the cloud of 10: every point would have been dropped, none was
        assert len(c10["moved_dyn"]) == 10 and c10["fpn_before"] > thr and len(c10["dyn_before"]) > 0
        assert would_drop(c10, prm) == tags(c10["moved_dyn"]) == appended_dyn(c10)
        proven.append("dynamic_cloud_of_10_unfiltered")
        # the cloud of 11: removed completely
        assert len(d11["moved_dyn"]) == 11 and d11["fpn_before"] > thr
        assert d11["n"][0] == len(d11["dyn_before"]) and would_drop(d11, prm) == tags(d11["moved_dyn"])
        proven.append("dynamic_cloud_of_11_removed_completely")
        # extract under the tilted pose: the in-place grids merged something, the crop dropped and kept something; a second one in a row
        assert e1["grid_n"][2] < e1["n_before"][2] and e1["grid_n"][0] < e1["n_before"][0]
        assert 0 < sum(e1["n"]) < sum(e1["grid_n"])
        assert e2["n_before"] == e1["n"] and e2["slot"] == e1["slot"] == 0
        assert len(e1["tc"]) > 0 and min(e1["n"][0], e1["n"][2], e1["n"][3]) > 0, "the surf target needs all three of its classes"
        proven += ["extract_tilted", "extract_twice"]
        assert ins["fpn_before"] > thr and 0 < len(appended_dyn(ins)) < len(ins["moved_dyn"]), "insert after two extracts: filter against the gridded class"
        assert e3["slot"] == -1 and sum(e3["n"]) > 0
        proven += ["insert_after_extract", "extract_without_slot"]
    elif name.startswith("band_"):
        a, b, e = states
        kind = name[5:]
        assert b["fpn_before"] > thr and len(b["moved_dyn"]) > 10 and len(b["dyn_before"]) > 0
        got, all_ = appended_dyn(b), tags(b["moved_dyn"])
        if kind == "widen":
            only_widened = would_drop(b, prm) - would_drop(b, prm, widened=False)
            assert {600, 601, 602} <= only_widened, "points between max and (float)(min + 0.1) fall to the widening alone"
            assert not (only_widened & got) and {603, 604} <= got, "just above the widened band: kept"
            assert all_ - got == would_drop(b, prm)
            proven.append("band_widened")
        elif kind == "off":
            assert would_drop(b, prm) and got == all_
            proven.append("dynamic_removal_off_above_threshold")
        elif kind == "fltmax":
            assert all_ - got == {607, 608} == would_drop(b, prm), "min = max = FLT_MAX: only points within `near` go (on it included)"
            proven.append("thresholds_flt_max")
        else:
            assert all_ - got == would_drop(b, prm) and 0 < len(got) < len(all_)
            proven.append("radius_flt_max")
        assert e["n"][0] > 0
    elif name == "empty_dynamic":
        a, b, c, e = states
        assert b["fpn_before"] > thr and len(b["dyn_before"]) == 0 and len(b["moved_dyn"]) > 10
        assert appended_dyn(b) == tags(b["moved_dyn"])
        assert 0 < len(appended_dyn(c)) < len(c["moved_dyn"]), "the next frame is filtered against what was kept"
        proven.append("empty_dynamic_class_no_filter")
    elif name == "leaf_too_small":
        a, e1, e2 = states
        assert e1["grid_rc"] == [0, LEAF_TOO_SMALL, 0, 0, 0] and e1["grid_n"][1] == e1["n_before"][1] == 4
        for k in (0, 2, 3):
            assert e1["grid_n"][k] < e1["n_before"][k], "the neighbour classes are gridded normally"
        assert tags(e1["tc"]) == {700, 701, 702} and len(e1["tc"]) == 3, "the corner target holds the ungridded poles that survive the crop"
        assert e2["grid_rc"][1] == 0 and len(e2["tc"]) == 1, "cropped to the trio, the class is gridded by the second extract"
        proven += ["leaf_too_small_in_localmap_extract", "extract_twice"]
    elif name == "pad_zero":
        a, e = states
        names = list(PAD0_GROUND)
        left = tags(e["cls"][2])
        assert np.array_equal(e["crop"], [-4.0, -3.0, -1.0, 9.0, 3.0, 1.0]), e["crop"]
        assert e["grid_n"][2] == len(names), "every planted point is alone in its voxel"
        for k in PAD0_DROP:
            assert 800 + names.index(k) not in left, k
        for k in PAD0_KEEP:
            assert 800 + names.index(k) in left, k
        proven.append("crop_pad_zero_faces")
    elif name == "after_reset":
        e0, a, r, e1 = states
        for e in (e0, e1):
            assert e["n_before"] == [0] * 5 and sum(e["n"]) == 0 and len(e["tc"]) == len(e["ts"]) == 0
        assert e0["slot"] == 0 and e1["slot"] == -1
        proven.append("extract_after_reset")
    else:
        raise AssertionError("no census for " + name)
    return proven


# ---- submaps ---------------------------------------------------------------------------------------------------------------
SUB = params(max_num_pts=103, r=R, tmin=0.5, tmax=2.0, near=0.25)


def _sub_first(small=False):
    """fisrt_submap: the clouds as they are (their own frame is the submap's)."""
    if small:
        return [mk(ANCHORS[:6], 100 + np.arange(6)), mk([(-15.0, 15.0, 0.25 * k) for k in range(3)], 20),
                mk([(float(i), -3.0, -1.5) for i in range(4)], 30), mk([(20.0, 0.0, 1.0)], 40), mk([(30.0, 30.0, 1.0)], 50)]
    return [mk(ANCHORS, 100 + np.arange(12)), mk([(-15.0, 15.0, 0.25 * k) for k in range(6)] + [(-15.0 + Q, 15.0, 0.0), (-10.0, 10.0, 0.5), (-10.0 + Q, 10.0, 0.5)], 20),
            mk([(float(i), -3.0, -1.5) for i in range(10)] + [(Q, -3.0, -1.5)], 30), mk([(20.0, float(j), 1.0) for j in range(6)], 40),
            mk([(30.0 + k, 30.0, 1.0) for k in range(5)], 50)]


def case_submap_main():
    """Two submaps.  A: first key frame, a filtered insert, a tilted insert of 10 dynamic points (unfiltered).  B: a first key frame at
    the threshold exactly, so its second insert is unfiltered, then a filtered one.  All five classes, the outlier class among them.
    Extracts with pad, corner_leaf, surf_leaf other than 10 / 0.2 / 0.5, with and without a target slot."""
    pl = planted_frame(LEVEL_B)
    pl[4] = mk(seen_from([(31.0, 31.0, 1.5), (32.0, 31.0, 1.5), (33.0, 31.0, 1.5)], LEVEL_B), 51)
    ten = frame(TILTED, [ANCHORS[i] + (0, 0, 1.0) for i in range(9)] + [ANCHORS[11] + (0, 0, 1.0)], outlier=[(28.0, 28.0, 0.5)],
                dyn_tags=300 + np.arange(10))
    b_first = _sub_first(small=True)                                   # 6 + 3 + 4 + 1 + 1 = 15
    b_first[2] = mk([(float(i), -3.0, -1.5) for i in range(9)], 30)    # ... = 20 = 103 / 5
    pl_b = planted_frame(LEVEL_C)
    pl_b2 = frame(LEVEL_B, [ANCHORS[i] + (0, 0, -d) for i, d in enumerate(PLANT_D[:6])] + [ANCHORS[i] + (0, 0, -1.0) for i in range(6, 12)],
                  pole=[(-14.0, 14.0, 0.5), (-14.0 + Q, 14.0, 0.5)], building=[(20.0, 2.0, 2.0)], outlier=[(29.0, 29.0, 0.5)], dyn_tags=500 + np.arange(12))
    ops = [("sinsert", "A", _sub_first(), None, TILTED),
           ("sinsert", "A", pl, LEVEL_B, TILTED),
           ("sinsert", "A", ten, TILTED, TILTED),
           ("sinsert", "B", b_first, None, TILTED_2),
           ("sinsert", "B", pl_b, LEVEL_C, TILTED_2),
           ("sinsert", "B", pl_b2, LEVEL_B, TILTED_2),
           ("sextract", "A", "B", TILTED, TILTED_2, 3.0, 0.125, 0.25, 0),
           ("sextract", "B", "A", LEVEL_C, TILTED, 0.5, 0.25, 1.0, -1),
           ("srefuse", "A", "A"), ("srefuse", "A", "never"), ("srefuse", "never", "B")]
    return dict(name="submap_main", prm=SUB, ops=ops)


def case_submap_empty_source():
    """The current submap's poles lie outside the pair's intersection box: its corner source comes out empty (nk == 0 skips the grid),
    its surf source does not."""
    c = [mk([(2.0, 2.0, 0.0)], 100), mk([(1.0, 1.0, 0.5), (9.0, 9.0, 0.5)], 20), mk([(float(i), float(i), -1.5) for i in range(11)], 30),
         mk([(5.0, 0.0, 1.0)], 40), empty()]
    d = [mk([(3.0, 3.0, 0.0)], 100), mk([(55.0, 5.0, 0.5), (58.0, 5.0, 0.5)], 20),
         mk([(float(i), float(i) + 0.5, -1.5) for i in range(11)] + [(60.0, 5.0, -1.5), (4.0, 4.5 + Q, -1.5)], 30), mk([(6.0, 0.0, 1.0)], 40), empty()]
    ops = [("sinsert", "C", c, None, LEVEL_A), ("sinsert", "D", d, None, LEVEL_C),
           ("sextract", "C", "D", LEVEL_A, LEVEL_C, 1.0, 0.2, 0.5, 0)]
    return dict(name="submap_empty_source", prm=SUB, ops=ops)


def case_submap_leaf_too_small():
    """Both submaps reach 2 000 m, so the intersection box does; the current one's corner source is refused by the 0.05 m grid and
    handed through, its surf source is gridded."""
    e = [mk([(2.0, 2.0, 0.0)], 100), mk([(1.0, 1.0, 0.5)], 20), mk([(0.0, 0.0, -1.5), FAR], 30), empty(), empty()]
    f = [mk([(3.0, 3.0, 0.0), (3.0 + Q, 3.0, 0.0)], 100), mk(POLE_TRIO + [(1400.0, 1400.0, 120.0)], 700 + np.arange(4)),
         mk([(1.0, 1.0, -1.5), (1.0 + Q, 1.0, -1.5), (4.0, 4.0, -1.5)], 30), mk([(6.0, 0.0, 1.0)], 40), mk([(7.0, 7.0, 1.0)], 50)]
    ops = [("sinsert", "E", e, None, LEVEL_A), ("sinsert", "F", f, None, LEVEL_A),
           ("sextract", "E", "F", LEVEL_A, LEVEL_B, 16.0, 0.05, 0.5, 0)]
    return dict(name="submap_leaf_too_small", prm=SUB, ops=ops)


def submap_cases():
    return [case_submap_main(), case_submap_empty_source(), case_submap_leaf_too_small()]


def run_submaps(case):
    import oracle_ctypes as oc
    import replay_oracle as ro
    from lisreg import synth
    prm = case["prm"]
    maps, states = {}, []
    for op in case["ops"]:
        if op[0] == "sinsert":
            _, key, clouds, rel, sub_pose = op
            so = maps.setdefault(key, ro.SubMapOracle(synth.PCL_DTYPE))
            st = dict(kind="sinsert", key=key, fpn_before=so.feature_point_num, dyn_before=so.cls[0], frame=clouds, first=rel is None,
                      n_before=[len(c) for c in so.cls],
                      moved_dyn=clouds[0] if rel is None or not len(clouds[0]) else oc.transform_cloud(clouds[0], rel, fmt=1))
            so.insert(clouds, None if rel is None else np.asarray(rel, np.float32), **insert_kw(prm))
            st.update(n=[len(c) for c in so.cls], fpn=so.feature_point_num, local_bound=so.bound.copy(),
                      bound=so.global_bound(np.asarray(sub_pose, np.float32)), cls=_copy(so.cls))
            states.append(st)
        elif op[0] == "sextract":
            _, pk, ck, pp, cp, pad, cl, sl, slot = op
            pre, cur = maps[pk], maps[ck]
            pp32, cp32 = np.asarray(pp, np.float32), np.asarray(cp, np.float32)
            tc, ts, sc, ss, isect, isect_local = ro.extract_submap_cloud(pre, cur, pp32, cp32, pad, cl, sl)
            # for the census: the sources as cropped, before their grids, and what the grids answered
            crop_c = oc.bbx_filter(cur.cls[1], isect_local) if len(cur.cls[1]) else cur.cls[1]
            surf = ro.cat([cur.cls[0], cur.cls[2], cur.cls[3]])
            crop_s = oc.bbx_filter(surf, isect_local) if len(surf) else surf
            rc_c = oc.voxel_grid(crop_c, float(np.float32(cl)), fmt=1)[0] if len(crop_c) else None
            rc_s = oc.voxel_grid(crop_s, float(np.float32(sl)), fmt=1)[0] if len(crop_s) else None
            states.append(dict(kind="sextract", pre=pk, cur=ck, slot=slot, tc=tc, ts=ts, sc=sc, ss=ss, isect=isect, isect_local=isect_local,
                               n_src_before=(len(cur.cls[1]), len(surf)), n_cropped=(len(crop_c), len(crop_s)), grid_rc=(rc_c, rc_s),
                               n_tgt_before=(len(pre.cls[1]), len(pre.cls[2]) + len(pre.cls[3]) + len(pre.cls[0])),
                               boxes_in=(pre.bound.copy(), pp32, cur.bound.copy(), cp32, pad)))
        else:
            states.append(dict(kind="srefuse", pre=op[1], cur=op[2]))
    return states


def census_submaps(case, states):
    name, prm = case["name"], case["prm"]
    thr = prm["max_num_pts"] // 5
    proven = []
    if name == "submap_main":
        a1, a2, a3, b1, b2, b3, x1, x2 = states[:8]
        assert a1["first"] and a1["n"] == [len(c) for c in a1["frame"]] and a1["n"][4] > 0
        assert a2["fpn_before"] > thr and appended_dyn(a2) == PLANT_KEEP and tags(a2["moved_dyn"]) - appended_dyn(a2) == PLANT_DROP
        assert a2["n"][4] > a1["n"][4] and a3["n"][4] > a2["n"][4], "only submaps append the outlier class"
        assert len(a3["moved_dyn"]) == 10 and would_drop(a3, prm) == tags(a3["moved_dyn"]) == appended_dyn(a3)
        proven += ["first_key_frame_then_filtered_insert", "outlier_class_appended", "dynamic_cloud_of_10_unfiltered"]
        assert b1["first"] and b1["fpn"] == thr == b2["fpn_before"]
        assert would_drop(b2, prm) and appended_dyn(b2) == tags(b2["moved_dyn"]), "at the threshold: unfiltered"
        assert b3["fpn_before"] > thr and 0 < len(appended_dyn(b3)) < len(b3["moved_dyn"])
        proven += ["unfiltered_insert_at_threshold", "filtered_insert"]
        assert not np.array_equal(a3["bound"], a3["local_bound"])
        for x in (x1, x2):
            for before, after in zip(x["n_tgt_before"] + x["n_cropped"], (len(x["tc"]), len(x["ts"]), len(x["sc"]), len(x["ss"]))):
                assert 0 < after < before, "each of the four clouds must lose points to its crop or its grid, and keep some"
            assert x["grid_rc"] == (0, 0)
        assert x1["slot"] == 0 and x2["slot"] == -1
        assert all(s["kind"] == "srefuse" for s in states[8:]) and len(states) == 11
        proven += ["submap_extract_non_default", "submap_extract_without_slot", "refusals"]
    elif name == "submap_empty_source":
        c, d, x = states
        assert x["n_src_before"][0] > 0 and x["n_cropped"][0] == 0 and len(x["sc"]) == 0 and x["grid_rc"][0] is None
        assert 0 < len(x["ss"]) < x["n_cropped"][1] < x["n_src_before"][1] and len(x["ts"]) > 0
        proven.append("source_emptied_by_the_crop")
    elif name == "submap_leaf_too_small":
        e, f, x = states
        assert x["grid_rc"] == (LEAF_TOO_SMALL, 0) and len(x["sc"]) == x["n_cropped"][0] == 4 and tags(x["sc"]) == {700, 701, 702, 703}
        assert 0 < len(x["ss"]) < x["n_cropped"][1], "the other source is gridded normally"
        proven.append("leaf_too_small_in_submap_extract")
    else:
        raise AssertionError("no census for " + name)
    return proven


def crop_box_inputs():
    """(pre local bound, pre pose, cur local bound, cur pose, pad) of every submap extract of the cases."""
    out = []
    for case in submap_cases():
        out += [s["boxes_in"] for s in run_submaps(case) if s["kind"] == "sextract"]
    return out


# ---- the key-frame ring -----------------------------------------------------------------------------------------------------
def ring_push(oc, kc, ks, corner, surf, T, max_keep):
    """saveKeyFrames (odomEstimationNode.cpp:421-468): both clouds transformPointCloud'ed into the map frame and appended; the oldest
    frames beyond max_keep leave.  Returns the new (corner frames, surf frames)."""
    kc = kc + [oc.transform_cloud(corner, T) if len(corner) else corner]
    ks = ks + [oc.transform_cloud(surf, T) if len(surf) else surf]
    return kc[-max_keep:], ks[-max_keep:]


def ring_target(oc, kc, ks, corner_leaf, surf_leaf):
    """laserCloudInfoHandler (:185-207): the kept frames NEWEST FIRST, then the two voxel grids (a refused grid hands its input through).
    Returns (corner target, surf target, (corner status, surf status))."""
    import replay_oracle as ro
    rc_c, want_c = oc.voxel_grid(ro.cat(kc[::-1]), corner_leaf)
    rc_s, want_s = oc.voxel_grid(ro.cat(ks[::-1]), surf_leaf)
    return want_c, want_s, (rc_c, rc_s)


def _kf(seed, n_c, n_s, far_corner=False):
    c = lattice(n_c, seed, pitch=0.125, z=1.0) if n_c else np.zeros((0, 3))
    s = lattice(n_s, seed + 50, pitch=0.25, z=-1.5) if n_s else np.zeros((0, 3))
    if far_corner:
        c = np.concatenate([c, [FAR]])
    return mk(c, 0), mk(s, 0)


def ring_cases():
    P = [LEVEL_A, TILTED, LEVEL_B, TILTED_2, LEVEL_C]
    push = lambda i, nc, ns, keep, far=False: ("push",) + _kf(10 + i, nc, ns, far) + (P[i % 5], keep)
    return [
        dict(name="max_keep_1", ops=[push(0, 60, 150, 1), ("target", 0.25, 0.5, 0), push(1, 70, 140, 1), ("target", 0.25, 0.5, 0)]),
        dict(name="shrink", ops=[push(i, 40 + i, 90 + i, 5) for i in range(5)] + [("target", 0.25, 0.5, 0), push(5, 33, 77, 2), ("target", 0.25, 0.5, 0)]),
        dict(name="kinds", ops=[push(0, 0, 120, 3), ("target", 0.25, 0.5, 0), push(1, 50, 0, 3), ("target", 0.25, 0.5, 0),
                                push(2, 45, 0, 3), ("target", 0.25, 0.5, 0), push(3, 44, 0, 2), ("target", 0.25, 0.5, 0),
                                push(4, 0, 0, 1), ("target", 0.25, 0.5, 0)]),
        dict(name="leaf_too_small", ops=[push(0, 40, 100, 3, True), ("target", 0.25, 0.5, 0), push(1, 30, 0, 1, True), ("target", 0.25, 0.5, 0)]),
        # the shortcut: one condition changed at a time; "hand" = lisreg_set_target_slot on that slot by the caller in between
        dict(name="shortcut", ops=[push(0, 60, 150, 3), push(1, 55, 145, 3), ("target", 0.25, 0.5, 0), ("target", 0.25, 0.5, 0),
                                   ("hand", 0), ("target", 0.25, 0.5, 0),
                                   ("target", 0.5, 0.5, 0), ("target", 0.5, 1.0, 0), ("target", 0.5, 1.0, 1), ("target", 0.5, 1.0, 1),
                                   ("target", 0.5, 1.0, -1), ("hand", 1), ("target", 0.5, 1.0, -1), ("target", 0.5, 1.0, 1),
                                   push(2, 50, 140, 3), ("target", 0.5, 1.0, 1)]),
    ]


def run_ring(case):
    import oracle_ctypes as oc
    kc, ks, states = [], [], []
    for op in case["ops"]:
        if op[0] == "push":
            _, corner, surf, T, keep = op
            before = len(kc)
            kc, ks = ring_push(oc, kc, ks, corner, surf, np.asarray(T, np.float32), keep)
            states.append(dict(kind="push", n_keyframes=len(kc), dropped=before + 1 - len(kc)))
        elif op[0] == "target":
            _, cl, sl, slot = op
            want_c, want_s, rc = ring_target(oc, kc, ks, cl, sl)
            states.append(dict(kind="target", slot=slot, leaf=(cl, sl), tc=want_c, ts=want_s, rc=rc, n_keyframes=len(kc),
                               n_cat=(sum(len(c) for c in kc), sum(len(s) for s in ks))))
        else:
            states.append(dict(kind="hand", slot=op[1]))
    return states


def census_ring(case, states):
    name = case["name"]
    tg = [s for s in states if s["kind"] == "target"]
    pu = [s for s in states if s["kind"] == "push"]
    if name == "max_keep_1":
        assert [p["n_keyframes"] for p in pu] == [1, 1] and pu[1]["dropped"] == 1
        assert not np.array_equal(tg[0]["tc"]["x"][:5], tg[1]["tc"]["x"][:5])
        return ["max_keep_1"]
    if name == "shrink":
        assert pu[4]["n_keyframes"] == 5 and pu[5]["dropped"] == 4 and pu[5]["n_keyframes"] == 2, "several frames leave in one push"
        assert 0 < tg[1]["n_cat"][0] < tg[0]["n_cat"][0]
        return ["push_drops_several"]
    if name == "kinds":
        assert [t["n_cat"][0] > 0 for t in tg] == [False, True, True, True, False]
        assert [t["n_cat"][1] > 0 for t in tg] == [True, True, True, False, False]
        assert tg[3]["n_keyframes"] == 2 and tg[4]["n_keyframes"] == 1, "a ring of corner-only frames; a ring whose one frame is empty"
        return ["frame_without_corners", "frame_without_surfs", "single_kind_ring", "empty_ring_target"]
    if name == "leaf_too_small":
        assert tg[0]["rc"] == (LEAF_TOO_SMALL, 0) and len(tg[0]["tc"]) == tg[0]["n_cat"][0] and 0 < len(tg[0]["ts"]) < tg[0]["n_cat"][1]
        assert tg[1]["rc"][0] == LEAF_TOO_SMALL and tg[1]["n_cat"] == (31, 0) and len(tg[1]["tc"]) == 31
        return ["leaf_too_small_joint_grids", "leaf_too_small_single_grid"]
    if name == "shortcut":
        events, last, pushed, hands = [], None, False, set()
        for s in states:
            if s["kind"] == "push":
                pushed = True
            elif s["kind"] == "hand":
                hands.add(s["slot"])
            else:
                if last is not None:
                    ev = [w for w, a, b in (("corner_leaf", s["leaf"][0], last["leaf"][0]), ("surf_leaf", s["leaf"][1], last["leaf"][1]),
                                            ("slot", s["slot"], last["slot"])) if a != b]
                    ev += ["push"] if pushed else []
                    ev += ["hand"] if s["slot"] == last["slot"] and s["slot"] in hands else []
                    events.append(ev)
                last, pushed, hands = s, False, set()
        # exactly one condition changes between two calls, or none
        assert events == [[], ["hand"], ["corner_leaf"], ["surf_leaf"], ["slot"], [], ["slot"], [], ["slot"], ["push"]], events
        assert len(tg[2]["tc"]) > len(tg[3]["tc"]) and len(tg[3]["ts"]) > len(tg[4]["ts"]), "each leaf change must change its target"
        return ["shortcut_conditions"]
    raise AssertionError("no census for " + name)


# ---- growth -----------------------------------------------------------------------------------------------------------------
# grow_keep asks for max(1.5 * bytes, min(2 * cap, ..), 16 MB) = 16 MB for a class cloud's first allocation, and DevBuf::ensure
# (lisreg_ctx.hpp) adds a quarter and 256 bytes of head-room to whatever it is asked for: 20 MB + 256 bytes = 1 310 736 records of 16 bytes
FIRST_ALLOCATION_RECORDS = ((16 << 20) + (16 << 20) // 4 + 256) // 16
GROW_N = 400000
GROW_POSES = (LEVEL_A, TILTED, LEVEL_B, TILTED_2)


def big_cloud(seed, tag):
    return mk(lattice(GROW_N, seed), tag)


@functools.lru_cache(maxsize=None)
def growth_localmap_case():
    """The ground class takes 400 000 points four times (level, tilted, level, tilted): an insert asks for n + 1 records, so the first
    three fit the first allocation and the fourth moves the buffer with 1 200 000 records kept; then the in-place grid and crop over the
    grown buffer, and one more insert."""
    small = lambda pose, t: frame(pose, ANCHORS[:11] + (0, 0, 0.125 * t), pole=[(-15.0, 15.0, 0.25 * k + t) for k in range(4)],
                                  building=[(20.0, float(j), float(t)) for j in range(5)], dyn_tags=100 * (t + 1) + np.arange(11))
    ops = []
    for t, pose in enumerate(GROW_POSES):
        f = small(pose, t)
        f[2] = big_cloud(t, 30 + t)
        ops.append(("insert", f, pose))
    f = small(LEVEL_C, 4)
    f[2] = big_cloud(4, 34)
    ops += [("extract", TILTED_2, 0), ("insert", f, LEVEL_C)]
    return dict(name="growth_localmap", prm=params(), ops=ops)


@functools.lru_cache(maxsize=None)
def growth_submap_case():
    """All five classes of a submap take 400 000 points four times (first key frame, tilted, level, tilted); the filter is on and keeps
    everything (near = 0, min = max = FLT_MAX), so the dynamic class grows through the filtered path's append.  Then an extract with the
    grown submap as the target, and one more (small) insert."""
    prm = params(r=8.0, near=0.0, tmin=FLT_MAX, tmax=FLT_MAX)
    ops = []
    for t, rel in enumerate((None,) + GROW_POSES[1:]):
        ops.append(("sinsert", "G", [big_cloud(10 * t + k, 10 * k + t) for k in range(5)], rel, TILTED_2))
    small = [mk(ANCHORS, 100 + np.arange(12)), mk([(-15.0, 15.0, 0.5)], 20), mk([(float(i), 1.0, -1.5) for i in range(8)], 30),
             mk([(20.0, 0.0, 1.0)], 40), mk([(25.0, 25.0, 1.0)], 50)]
    ops += [("sinsert", "H", small, None, LEVEL_A), ("sextract", "G", "H", TILTED_2, LEVEL_A, 10.0, 0.2, 0.5, 0),
            ("sinsert", "G", [mk(lattice(200, 40 + k), 10 * k + 4) for k in range(5)], LEVEL_C, TILTED_2)]
    return dict(name="growth_submap", prm=prm, ops=ops)


def census_growth(states, classes, inserts="insert"):
    ins = [s for s in states if s["kind"] == inserts and max(s["n"]) > GROW_N // 2]
    for k in classes:
        assert ins[0]["n"][k] < ins[1]["n"][k] < ins[2]["n"][k] <= FIRST_ALLOCATION_RECORDS - 1 < ins[3]["n"][k], \
            "the fourth insert, and no earlier one, must pass the first allocation with contents to keep"
    return ["grow_keep_with_contents"]
