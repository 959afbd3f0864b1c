"""The exact searches and the grid kernels on map-frame clouds kilometres from the origin (tests/far_frame.py).

Every kernel here that promises an exact answer sorts points into cells laid out from a float32 origin, and the float32 searches prove
exactness with an absolute slack of one millimetre that has to absorb roundings at ulp(|coordinate|) — 0.49 mm in [4096, 8192) m.
The rest of the suite never leaves the first hundred metres.  This file moves the planted clouds of the other tests into three frames
— `origin` (the control: a failure there indicts the helper), `km` = (1000, -2000, 30) and `edge` = (8000, -8000, -200), just inside the
documented range |coordinate| < 8192 m — and checks only outputs that have an EXACT definition at any offset: indices, survivor lists,
cell ids and counts, bit patterns against the CPU restatement of the same arithmetic.  Poses of the production arithmetic far out are
not judged here (tests/test_fit_device.py covers the residual models out to 1 km).

CPU (-m "not gpu"): every planted event is proven to occur in every frame — the planted properties of tests/nn1_ref.py on the moved
clouds, the face plants' census, the dynamic filter's radius gate, the boxes whose faces pass through points, the five-nearest
reference's own near-ties.  GPU: the library against those definitions."""
import numpy as np
import pytest

import far_frame as F
import nn1_ref as R
from test_nn1_forms import FORMS, _bits, _pcl, _same_found, _same_grid, _seed_choices, check_planted

f32 = np.float32
FRAMES = F.FRAME_NAMES
SLOT = 91
HUGE_RADIUS = 1.0e6                       # center_radius^2 = 1e12 is a float32 like any other: the distance predicate decides
DYN = dict(dmin=0.3, dmax=1.0, near=0.05)


# ================================================================ the helper itself
def test_shift_is_the_float32_sum_for_every_kind_of_cloud():
    from lisreg import synth
    xyz = R.case("lattice")["map"]
    for frame in FRAMES:
        o = F.offset(frame)
        got = F.shift(xyz, frame)
        assert got.dtype == f32 and np.array_equal(got, (xyz + o).astype(f32))
        assert np.array_equal(got.astype(np.float64), xyz.astype(np.float64) + o.astype(np.float64))      # the 1/8 m lattice moves EXACTLY
        c = synth.to_pcl(xyz, np.arange(len(xyz)) % 7, np.arange(len(xyz), dtype=f32))
        s = F.shift(c, frame)
        assert s.dtype == c.dtype and np.array_equal(synth.pcl_xyz(s), got)
        assert np.array_equal(s["label"], c["label"]) and np.array_equal(s["intensity"], c["intensity"])
        rec = np.concatenate([xyz, np.arange(len(xyz), dtype=f32)[:, None]], 1)
        assert np.array_equal(F.shift(rec, frame)[:, :3], got) and np.array_equal(F.shift(rec, frame)[:, 3], rec[:, 3])
        assert F.in_range(got, s)
    assert np.array_equal(F.shift(xyz, "origin"), xyz)
    assert not F.in_range(np.array([[8192.0, 0, 0]], f32)) and F.in_range(np.array([[np.nan, 8191.9, 0]], f32))
    assert np.spacing(f32(8191.0)) == f32(2.0 ** -11) and np.spacing(f32(8192.0)) == f32(2.0 ** -10)


# ================================================================ k = 1 search
def _face_case(base, frame):
    if (base, frame) not in _FACE:
        fp = F.face_plants(R.case("scene")["map"], frame) if base == "scene" else F.face_plants(F.dense_patch(), frame, site=7.5)
        fp["brute"] = F.check_face_plants(fp)
        _FACE[(base, frame)] = fp
    return _FACE[(base, frame)]


_FACE = {}
FACE_BASES = ("scene", "dense")           # cell edge 0.5 m (faces exact at any offset) / 0.48 m (faces round at ulp(|coordinate|))


def _assert_case_in_range(name, c):
    """Every map and every query lies inside the documented range — except the queries that `edges` plants 30 and 500 m OUTSIDE the
    grid, which at 8 km reach 8545 m.  They stay in on purpose: for a query outside the grid the walk's box is clamped to the grid,
    so every face it recomputes is the grid's own, inside the range; of the query itself only qx - rad is rounded, half a float step
    of 0.98 mm there against a radius that carries the millimetre."""
    assert F.in_range(c["map"])
    if name == "edges":
        out = c["groups"]["outside"]
        inside = np.setdiff1d(np.arange(len(c["queries"])), out)
        assert F.in_range(c["queries"][inside]) and np.nanmax(np.abs(c["queries"][out])) < 2 * F.COORD_LIMIT
    else:
        assert F.in_range(c["queries"])


@pytest.mark.parametrize("name", R.CASE_NAMES)
@pytest.mark.parametrize("frame", FRAMES)
def test_planted_properties_hold_in_every_frame(frame, name):
    check_planted(name, frame)
    c = R.case(name, frame)
    _assert_case_in_range(name, c)
    if name == "edges":                   # rebuilt from the moved map's geometry
        g = R.grid_geometry(c["map"])
        assert np.array_equal(c["queries"][c["groups"]["origin"][0]], g["o"])


@pytest.mark.parametrize("base", FACE_BASES)
@pytest.mark.parametrize("frame", FRAMES)
def test_face_plants_census(frame, base):
    fp = _face_case(base, frame)
    assert (fp["geom"]["cell"] == f32(0.5)) == (base == "scene")
    idx, d2 = fp["brute"]
    found = {cap: R.apply_cap(idx, d2, cap)[0] >= 0 for cap in R.CAPS}      # the first pass, doubled passes and the capped runs all occur
    assert found[1e18].all() and found[3.0].sum() > 200 and 0 < found[0.5].sum() < len(idx) and not found[0.0].any()
    assert (d2 < 0.25).sum() > 40 and ((d2 > 0.25) & (d2 < 1.0)).sum() > 20 and (d2 > 4.0).sum() > 10


@pytest.mark.parametrize("base", FACE_BASES)
@pytest.mark.parametrize("frame", FRAMES)
def test_faces_and_cell_assignment_agree_far_out(frame, base):
    """What the searches' millimetre has to cover on these grids (far_frame.face_overhang): around the origin the cell assignment
    rounds v - o coarser than the points are spaced, and floats of column i lie microns below the face the walk recomputes — far
    under the millimetre; in the far frames points and faces share one float lattice and not one float lies on the wrong side."""
    n, worst = F.face_overhang(_face_case(base, frame)["geom"])
    assert n > 100
    if frame == "origin":
        assert 0.0 < worst < 2.0e-5, worst
    else:
        assert worst == 0.0, worst


def _check_every_form(gpu_ctx, monkeypatch, m, q, idx, d2, what):
    """every form of lisreg_test_nn1, then the production launcher lisreg_nearest at LISREG_NN1_Q = 1, 4, 8, at every cap"""
    gpu_ctx.map_index_set(SLOT, _pcl(m))
    _same_grid(gpu_ctx, m, SLOT)
    for form in FORMS:
        for cap in R.CAPS:
            got = gpu_ctx.test_nn1(SLOT, q, cap, form)
            _same_found(got, R.apply_cap(idx, d2, cap), (what, form, cap))
            miss = got[0] < 0
            assert np.all(_bits(got[1])[miss] == _bits(R.not_found_d2(cap))), (what, form, cap)
    qc = _pcl(q)
    for lanes in ("1", "4", "8"):
        monkeypatch.setenv("LISREG_NN1_Q", lanes)
        for cap in R.CAPS:
            got = gpu_ctx.nearest(SLOT, qc, cap)
            _same_found(got, R.apply_cap(idx, d2, cap), (what, "lisreg_nearest", lanes, cap))
            miss = got[0] < 0
            assert np.all(_bits(got[1])[miss] == _bits(R.not_found_d2(cap))), (what, "lisreg_nearest", lanes, cap)
    monkeypatch.delenv("LISREG_NN1_Q")


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.CASE_NAMES)
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_every_form_matches_the_definition_in_every_frame(gpu_ctx, monkeypatch, frame, name):
    check_planted(name, frame)
    c = R.case(name, frame)
    _assert_case_in_range(name, c)
    idx, d2, _, _ = R.brute(name, frame)
    _check_every_form(gpu_ctx, monkeypatch, c["map"], c["queries"], idx, d2, (frame, name))


@pytest.mark.gpu
@pytest.mark.parametrize("base", FACE_BASES)
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_every_form_finds_the_winner_across_the_face(gpu_ctx, monkeypatch, frame, base):
    fp = _face_case(base, frame)
    idx, d2 = fp["brute"]
    _check_every_form(gpu_ctx, monkeypatch, fp["map"], fp["queries"], idx, d2, (frame, base, "face plants"))
    # seeded with the decoy, as the ICP kernels seed with last iteration's neighbour: the bound is the decoy's distance before the
    # first column is looked at, so the winner's column passes the column test by four float steps of z, whichever column comes first
    for form in FORMS:
        for cap in (1e18, 3.0):
            got = gpu_ctx.test_nn1(SLOT, fp["queries"], cap, form, fp["decoy"])
            _same_found(got, R.apply_cap(idx, d2, cap), (frame, base, "seeded with the decoy", form, cap))


@pytest.mark.gpu
@pytest.mark.parametrize("form", (0, 4))
@pytest.mark.parametrize("name", ("lattice", "scene"))
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_the_seed_never_changes_the_result_in_any_frame(gpu_ctx, frame, name, form):
    check_planted(name, frame)
    c = R.case(name, frame)
    idx, d2, cnt, last = R.brute(name, frame)
    gpu_ctx.map_index_set(SLOT, _pcl(c["map"]))
    seeds = _seed_choices(name, frame)
    for cap in (1e18, 0.5):
        want = R.apply_cap(idx, d2, cap)
        plain = gpu_ctx.test_nn1(SLOT, c["queries"], cap, form)
        _same_found(plain, want, (frame, name, form, cap, "no seeds"))
        for kind, s in seeds.items():
            got = gpu_ctx.test_nn1(SLOT, c["queries"], cap, form, s)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(_bits(got[1]), _bits(plain[1])), (frame, name, form, cap, kind)


# ================================================================ dynamic filter
def _dynamic_cases(frame):
    """[(map, queries, center_radius, dmin, dmax, near, keep)]: the moved scene and threshold clouds, at the reference's radius and at a
    huge one.  The reference compares center_radius with x^2 + y^2 of the MAP-FRAME point, so far out the gate keeps everything."""
    out = []
    T = R.THRESHOLDS
    for name, radius, dmin, dmax, near in (("scene", 30.0, DYN["dmin"], DYN["dmax"], DYN["near"]),
                                           ("thresholds", T["center_radius"], T["dmin"], T["dmax"], T["near"])):
        c = R.case(name, frame)
        for r in (radius, HUGE_RADIUS):
            assert F.in_range(c["map"], c["queries"])
            keep = R.dynamic_keep(c["map"], c["queries"], r, dmin, dmax, near)
            out.append((name, c["map"], c["queries"], r, dmin, dmax, near, keep))
    return out


@pytest.mark.parametrize("frame", FRAMES)
def test_dynamic_filter_census(frame):
    for name, m, q, r, dmin, dmax, near, keep in _dynamic_cases(frame):
        assert F.in_range(m, q) and len(q) > 10
        if r == HUGE_RADIUS:
            assert 0 < keep.sum() < len(q), (frame, name)                  # the distance predicate decides
        elif frame == "origin":
            assert 0 < keep.sum() < len(q), (frame, name)
        else:
            assert keep.all(), (frame, name)                               # every point lies outside the radius about the ORIGIN


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_dynamic_filter_in_every_frame(gpu_ctx, frame):
    for name, m, q, r, dmin, dmax, near, keep in _dynamic_cases(frame):
        gpu_ctx.map_index_set(SLOT, _pcl(m))
        qc = _pcl(q, intensity=np.arange(len(q), dtype=f32))
        got, applied = gpu_ctx.dynamic_filter(SLOT, qc, r, dmin, dmax, near)
        want = qc[keep]
        assert applied and len(got) == len(want), (frame, name, r, len(got), len(want))
        assert all(np.array_equal(got[f], want[f]) for f in want.dtype.names), (frame, name, r)


# ================================================================ box crop and bounds
def _box_case(frame):
    """the moved scene scan and a box every face of which passes through a point of it (the comparison is strict: those six stay out)"""
    q = R.case("scene", frame)["queries"]
    assert F.in_range(q)
    cloud = _pcl(q, intensity=np.arange(len(q), dtype=f32))
    order = [np.argsort(q[:, d]) for d in range(3)]
    n = len(q)
    lo_i = [order[d][n // 4] for d in range(3)]; hi_i = [order[d][3 * n // 4] for d in range(3)]
    box = np.array([float(q[lo_i[d], d]) for d in range(3)] + [float(q[hi_i[d], d]) for d in range(3)])
    return cloud, q, box, lo_i + hi_i


@pytest.mark.parametrize("frame", FRAMES)
def test_box_census(oracle, frame):
    cloud, q, box, on_face = _box_case(frame)
    x = q.astype(np.float64)
    inside = np.all((x > box[:3]) & (x < box[3:]), axis=1)
    assert 0 < inside.sum() < len(q) and not inside[on_face].any()
    loose = np.all((x >= box[:3]) & (x <= box[3:]), axis=1)
    assert loose.sum() > inside.sum()                                       # points ON a face: `>=` would keep them
    assert np.array_equal(oracle.bbx_filter(cloud, box)["intensity"], np.flatnonzero(inside).astype(f32))
    assert np.array_equal(oracle.bbx_filter(cloud, box, True)["intensity"], np.flatnonzero(~inside).astype(f32))
    assert np.array_equal(oracle.cloud_bounds(cloud), np.concatenate([x.min(0), x.max(0)]))


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_bbx_and_bounds_in_every_frame(oracle, gpu_ctx, frame):
    cloud, q, box, _ = _box_case(frame)
    for delete in (False, True):
        got, want = gpu_ctx.bbx_filter(cloud, box, delete), oracle.bbx_filter(cloud, box, delete)
        assert len(got) == len(want) and all(np.array_equal(got[f], want[f]) for f in want.dtype.names), (frame, delete)
    assert np.array_equal(gpu_ctx.cloud_bounds(cloud), oracle.cloud_bounds(cloud))


# ================================================================ voxel grids and transformPointCloud
LEAVES = (0.05, 0.2, 0.4, 0.6)


def _voxel_clouds(frame):
    """20 000 random labelled points in a 40 x 40 x 6 m box, and the crowded-voxel cloud of test_voxel.py, moved into the frame"""
    from lisreg import synth
    from test_voxel import crowded_cloud
    if frame not in _VOX:
        rng = np.random.default_rng(2020)
        xyz = (rng.uniform(-1.0, 1.0, (20000, 3)) * np.array([20.0, 20.0, 3.0])).astype(f32)
        rand = synth.to_pcl(xyz, rng.integers(0, 20, len(xyz)).astype(np.uint16), rng.uniform(0, 255, len(xyz)).astype(f32))
        crowd, pops = crowded_cloud(31)
        _VOX[frame] = (F.shift(rand, frame), F.shift(crowd, frame), pops)
        assert F.in_range(*_VOX[frame][:2])
    return _VOX[frame]


_VOX = {}
FAR_POSE = np.array([0.02, -0.01, -1.3, 12.0, -7.5, 0.25], f32)           # test_voxel.py's pose; the frame's offset goes on top


@pytest.mark.parametrize("frame", FRAMES)
def test_voxel_census(oracle, frame):
    """the case to catch: at 0.05 m and 8 km floorf(x * inv_leaf) is about 160 000 and min_b is negative on one axis; the crowded
    voxels keep their populations (the 0.5 m lattice moves exactly, the points stay inside their cells)"""
    from lisreg import synth
    rand, crowd, pops = _voxel_clouds(frame)
    assert F.in_range(rand, crowd)
    xyz = synth.pcl_xyz(rand)
    ijk = np.floor(xyz * (f32(1) / f32(0.05)))
    if frame == "edge":
        assert ijk[:, 0].max() > 159000 and ijk[:, 1].min() < -159000 and ijk[:, 2].min() < 0
    for leaf in LEAVES:
        rc, ds = oracle.voxel_grid(rand, leaf)
        assert rc == 0 and 0 < len(ds) < len(rand), (leaf, rc, len(ds))
    rc, ds = oracle.voxel_grid(crowd, 0.5)
    assert rc == 0 and len(ds) == len(pops)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_voxel_grids_in_every_frame(oracle, gpu_ctx, frame):
    import lisreg
    rand, crowd, pops = _voxel_clouds(frame)
    jobs = [(rand, leaf) for leaf in LEAVES] + [(crowd, 0.5)]
    wants = []
    for cloud, leaf in jobs:
        rc_o, want = oracle.voxel_grid(cloud, leaf)
        rc_g, got = gpu_ctx.voxel_downsample(cloud, leaf)
        assert rc_g == rc_o == 0 and len(got) == len(want), (frame, leaf, len(got), len(want))
        for f in ("x", "y", "z", "intensity", "label"):
            assert np.array_equal(got[f], want[f]), (frame, leaf, f)
        wants.append(want)
    # the same five grids through ONE sort and one centroid launch (lisreg_voxel_downsample_multi), device records in and out
    recs = [lisreg.pack_device_records(c) for c, _ in jobs]
    ins = [lisreg.DeviceArray(r) for r in recs]
    outs = [lisreg.DeviceArray(np.zeros_like(r)) for r in recs]
    counts = gpu_ctx.voxel_downsample_multi_device([b.ptr for b in ins], [len(r) for r in recs], [leaf for _, leaf in jobs],
                                                   [o.ptr for o in outs], [len(r) for r in recs])
    assert counts == [len(w) for w in wants], (frame, counts)
    for o, w, cnt, (_, leaf) in zip(outs, wants, counts, jobs):
        got = o.download(cnt)
        assert np.array_equal(got[:, 0], w["x"]) and np.array_equal(got[:, 1], w["y"]) and np.array_equal(got[:, 2], w["z"]), (frame, leaf)
        assert np.array_equal(got[:, 3].copy().view(np.uint32) & 0xffff, w["label"].astype(np.uint32)), (frame, leaf)
    for b in ins + outs:
        b.free()


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_transform_cloud_to_a_far_pose(oracle, gpu_ctx, frame):
    """sensor-frame cloud -> map frame under a key-frame pose with the frame's translation: bit for bit (every product and sum of
    transformPointCloud is rounded on its own on both sides)"""
    from lisreg import synth
    rand = _voxel_clouds("origin")[0]
    T = F.shift_pose(FAR_POSE, frame)
    want, got = oracle.transform_cloud(rand, T), gpu_ctx.transform_cloud(rand, T)
    assert F.in_range(want)
    for f in ("x", "y", "z", "intensity", "label"):
        assert np.array_equal(got[f], want[f]), (frame, f)
    if frame != "origin":
        assert np.abs(synth.pcl_xyz(want)).max() > 1000.0


# ================================================================ the sliding local map
def _drive():
    """four 16 x 450 labelled sweeps (under 30 000 points in all) and their key-frame poses"""
    from lisreg import replay
    if not _DRIVE:
        frames, truth = zip(*replay.synthetic_drive(4, h=16, w=450))
        assert sum(len(c) for c in frames) <= 30000
        _DRIVE.append((frames, truth))
    return _DRIVE[0]


_DRIVE = []


LOCALMAP_SETTINGS = dict(reference_radius=30.0, huge_radius=HUGE_RADIUS)
LOCALMAP_MAX_PTS = 30000                  # the dynamic removal starts once feature_point_num > max_num_pts / 5 = 6000: at the second frame


def _localmap_run(oracle, frame, radius, gpu_ctx=None):
    """the body of test_replay.test_localmap_composite_equals_oracle_bitwise with the key-frame poses and the current pose moved into
    the frame; with a context, every state of the device-resident map is compared with the host restatement.  Returns whether the
    map-based dynamic removal dropped a point."""
    import lisreg
    import replay_oracle as ro
    frames, truth = _drive()
    lm, removed_any = None, False
    if gpu_ctx is not None:
        P = lisreg.localmap_default_params()
        P.max_num_pts, P.dynamic_removal_center_radius = LOCALMAP_MAX_PTS, radius
        gpu_ctx.localmap_reset(4)
    for k, (cloud, T) in enumerate(zip(frames, truth)):
        T = F.shift_pose(T, frame)
        parts = oracle.semantic_split(cloud)
        full = dict(dynamic=parts[0], ground=parts[1], building=parts[2], pole=parts[3], outlier=parts[4])
        clouds = [full[c] for c in ro.CLASSES]
        if lm is None:
            lm = ro.LocalMapOracle(cloud.dtype)
        if k > 0:
            tc, ts, isect = lm.extract(T)
            assert len(tc) > 0 and len(ts) > 0
            if gpu_ctx is not None:
                info = gpu_ctx.localmap_extract(4, T, P, target_slot=0)
                assert np.array_equal(info["crop"], isect), (frame, k)
                assert info["n_target_corner"] == len(tc) and info["n_target_surf"] == len(ts), (frame, k)
                assert np.array_equal(gpu_ctx.localmap_get(4, 5), lisreg.pack_device_records(tc)), (frame, k)
                assert np.array_equal(gpu_ctx.localmap_get(4, 6), lisreg.pack_device_records(ts)), (frame, k)
        n_dyn_before = len(lm.cls[0])
        lm.insert(clouds, T, max_num_pts=LOCALMAP_MAX_PTS, center_radius=radius)
        removed_any |= len(lm.cls[0]) - n_dyn_before < len(full["dynamic"])
        assert F.in_range(*[c for c in lm.cls if len(c)])
        if gpu_ctx is not None:
            info = gpu_ctx.localmap_insert(4, clouds, T, P)
            assert info["n"] == [len(c) for c in lm.cls] and info["feature_point_num"] == lm.feature_point_num, (frame, k)
            assert np.array_equal(info["bound"], lm.bound), (frame, k)
            for c in range(5):
                assert np.array_equal(gpu_ctx.localmap_get(4, c), lisreg.pack_device_records(lm.cls[c])), (frame, k, c)
    if gpu_ctx is not None:
        gpu_ctx.localmap_reset(4)
    return removed_any


@pytest.mark.parametrize("frame", FRAMES)
def test_localmap_census(oracle, frame):
    """the drive exercises the map-based dynamic removal: at the reference's radius only around the origin (the radius is compared with
    x^2 + y^2 of the map-frame point, so far out everything is kept), at a huge radius in every frame"""
    assert _localmap_run(oracle, frame, LOCALMAP_SETTINGS["reference_radius"]) == (frame == "origin")
    assert _localmap_run(oracle, frame, LOCALMAP_SETTINGS["huge_radius"])


@pytest.mark.gpu
@pytest.mark.parametrize("setting", LOCALMAP_SETTINGS)
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_localmap_in_every_frame(oracle, gpu_ctx, frame, setting):
    """class clouds, bound, crop box and both targets equal the host restatement bit for bit, dynamic removal included"""
    _localmap_run(oracle, frame, LOCALMAP_SETTINGS[setting], gpu_ctx)


# ================================================================ the 5-NN front-ends at a far pose
def _knn_case(frame):
    """synth.make_case(16 x 450 vs 20 000) with the target moved into the frame, the source rotated by T_init's rotation ON THE HOST and
    handed in with a pose of zero angles and translation float32(t_init + offset): the device's query is float32(src + t), to the bit.
    Reference: float32 brute force of those queries against the moved target (six nearest, for the gap behind the fifth)."""
    import lisreg
    from lisreg import synth
    if frame not in _KNN:
        case = synth.make_case(h=16, w=450, m_points=20000, scan_seed=4321)
        T = F.translation_pose(case["T_init"][3:6], frame)
        out = dict(T=T, tau=float(lisreg.default_params(1).knn_sq_thresh))
        for kind in ("corner", "surf"):
            out["tgt_" + kind] = F.shift(case["tgt_" + kind], frame)
            out["src_" + kind] = F.rotate_on_host(case["src_" + kind], case["T_init"])
            q = (synth.pcl_xyz(out["src_" + kind]) + T[3:6]).astype(f32)
            out["q_" + kind] = q
            out["ref_" + kind] = F.knn5_brute(synth.pcl_xyz(out["tgt_" + kind]), q)
            assert F.in_range(out["tgt_" + kind], q)
        _KNN[frame] = out
    return _KNN[frame]


_KNN = {}
KNN_RUNS = (("walk1", 1, 1), ("walk8", 1, 8), ("graph", 3, 1), ("cells", 5, 1))


def _loose(c):
    """bool [n] over corner then surf queries: the reference's own 5th and 6th squared distances, or the 5th and tau, lie within 1e-6
    relative (FMA contraction inside the device's squared distance may swap such a pair: tests/test_neighbors.py's term); and how many
    queries hold an exact tie among their six"""
    loose, ties = [], 0
    for kind in ("corner", "surf"):
        _, d2 = c["ref_" + kind]
        d = d2.astype(np.float64)
        loose.append((np.abs(d[:, 5] - d[:, 4]) <= 1e-6 * d[:, 5]) | (np.abs(d[:, 4] - c["tau"]) <= 1e-6 * c["tau"]))
        ties += int((d2[:, 1:] == d2[:, :-1]).any(1).sum())
    return np.concatenate(loose), ties


def test_pose_of_zero_angles_is_exactly_the_identity():
    import lisreg
    for frame in FRAMES:
        T = F.translation_pose([0.3, -0.2, 0.05], frame)
        M = lisreg.pose_to_matrix(T)
        assert M.dtype == f32 and np.array_equal(M[:3, :3], np.eye(3, dtype=f32)) and np.array_equal(M[:3, 3], T[3:6])


KNN_CENSUS = dict(origin=0, km=1, edge=0)


@pytest.mark.parametrize("frame", FRAMES)
def test_knn_reference_census(frame):
    """the reference alone: 7 200 queries, most of them with five neighbours inside tau, 0 / 1 / 0 rounding-level queries in the three
    frames and no exact ties"""
    c = _knn_case(frame)
    assert F.in_range(c["tgt_corner"], c["tgt_surf"], c["q_corner"], c["q_surf"])
    loose, ties = _loose(c)
    found = np.concatenate([c["ref_" + k][1][:, 4] < c["tau"] for k in ("corner", "surf")])
    assert len(loose) == 7200 and 0.5 * len(found) < found.sum() < len(found)
    assert int(loose.sum()) == KNN_CENSUS[frame] and ties == 0, (frame, int(loose.sum()), ties)
    # the queries are the float32 sum, nothing else: one rounding of src + t
    from lisreg import synth
    for kind in ("corner", "surf"):
        exact = synth.pcl_xyz(c["src_" + kind]).astype(np.float64) + c["T"][3:6].astype(np.float64)
        assert np.array_equal(c["q_" + kind], exact.astype(f32))


def _dump(c, mode, lanes, canonical=0):
    import lisreg
    ctx = lisreg.Context(0)
    ctx.set_option("search_mode", mode); ctx.set_option("lanes_per_query", lanes); ctx.set_option("dump_neighbors", 1)
    ctx.set_option("canonical_ties", canonical)
    ctx.set_target(c["tgt_corner"], c["tgt_surf"])
    p = lisreg.default_params(1); p.fixed_iters = 1
    _, st, _ = ctx.align(c["src_corner"], c["src_surf"], c["T"], p)
    assert st["iters"] == 1 and ctx.front_end() == mode
    # "lanes_per_query" other than 1 means auto: the eight-lane walk has to be what the batch plan really took for this run
    assert ctx.get_option("lanes_per_query") == (8 if (mode == 1 and lanes != 1) else 1), (mode, lanes)
    ids = ctx.neighbors(len(c["src_corner"]) + len(c["src_surf"]))[:5].copy()
    ctx.close()
    return ids


@pytest.mark.gpu
@pytest.mark.parametrize("run", KNN_RUNS, ids=[r[0] for r in KNN_RUNS])
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_five_nearest_at_a_far_pose(frame, run):
    """the set of five and the found flag equal the float32 brute force's, except at the reference's own rounding-level queries"""
    c = _knn_case(frame)
    loose, _ = _loose(c)
    ids = _dump(c, run[1], run[2])
    nc = len(c["src_corner"])
    ref_idx = np.concatenate([c["ref_corner"][0][:, :5], c["ref_surf"][0][:, :5]])
    ref_found = np.concatenate([c["ref_corner"][1][:, 4] < c["tau"], c["ref_surf"][1][:, 4] < c["tau"]])
    got_found = ids[4] >= 0
    bad_found = np.flatnonzero(got_found != ref_found)
    both = ref_found & got_found
    bad_set = np.flatnonzero(both & (np.sort(ids.T, 1) != np.sort(ref_idx, 1)).any(1))
    bad = np.union1d(bad_found, bad_set)
    print(f"[far 5-NN] {frame} {run[0]}: found flags differ for {len(bad_found)}, sets for {len(bad_set)} of {len(loose)} queries; "
          f"{int(loose.sum())} rounding-level in the reference")
    strict = bad[~loose[bad]]
    assert strict.size == 0, (frame, run[0], strict[:8], ids[:, strict[:4]].T, ref_idx[strict[:4]], nc)
    assert len(bad) <= max(2, 1e-3 * len(loose))
    assert both.sum() > 0.5 * len(loose)


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_front_ends_agree_index_for_index_at_a_far_pose(frame):
    """canonical_ties = 1: the walk with one and with eight lanes per query, the graph scan and the cell rows return the same five in
    the same order (the auto choice, search_mode 4, resolves to the eight-lane walk at this size: it would be the second run again)"""
    c = _knn_case(frame)
    dumps = {name: _dump(c, mode, lanes, canonical=1) for name, mode, lanes in KNN_RUNS}
    first = dumps["walk1"]
    found = first[4] >= 0
    assert found.sum() > 0.5 * found.size
    for name, ids in dumps.items():
        assert np.array_equal(ids[4] >= 0, found), (frame, name)
        bad = np.flatnonzero((ids[:, found] != first[:, found]).any(0))
        assert bad.size == 0, (frame, name, bad[:8])


# ================================================================ the exact build against the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("mode", (1, 5))
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_exact_build_equals_oracle_in_every_frame(oracle, frame, mode):
    """the small case with its rotation left in the pose, exact_arithmetic = 1, three fixed iterations: accept flags, correspondence
    counts and iteration counts equal the oracle's (test_exact.check_exact), poses equal to the bit"""
    import lisreg
    from lisreg import synth
    from test_exact import check_exact
    case = dict(synth.make_case(h=16, w=450, m_points=20000, scan_seed=4321))
    case["tgt_corner"], case["tgt_surf"] = F.shift(case["tgt_corner"], frame), F.shift(case["tgt_surf"], frame)
    case["T_init"] = F.shift_pose(case["T_init"], frame)
    assert F.in_range(case["tgt_corner"], case["tgt_surf"])
    p_o = oracle.default_params(1)
    p_o.fixed_iters = 3
    worst, n = check_exact(oracle, lisreg, case, p_o, None, opts=(("search_mode", mode),))
    assert n > 0 and worst == 0.0, (frame, mode, worst, n)


# ================================================================ the fp64 verifiers
VSLOT = 17
K = 20


def _verifier_world(frame):
    """the planted clouds of vgicp_ref / ndt_ref / test_fgicp and a 5 000-point cut of their scene (the points nearest the target's
    centre, so that the density is the scene's), moved into the frame, with the restatement of each made once"""
    import fgicp_ref as FR
    import ndt_ref as NR
    import vgicp_ref as VR
    from test_fgicp import _planted
    if frame not in _VER:
        tgt, src, guess, T_true = VR.scene()
        c = tgt.astype(np.float64).mean(0)
        cut = np.ascontiguousarray(tgt[np.sort(np.argsort(((tgt[:, :2] - c[:2]) ** 2).sum(1))[:5000])])
        guess = np.array(guess, np.float64)
        near = np.abs((src.astype(np.float64) @ guess[:3, :3].T + guess[:3, 3])[:, :2] - c[:2]).max(1) < 12.0
        W = dict(cut=F.shift(cut, frame), src=np.ascontiguousarray(src[near][:1500]))
        W["guess"] = guess.copy(); W["guess"][:3, 3] += F.offset(frame).astype(np.float64)
        pv, groups = VR.planted_cloud()
        W["v_planted"], W["v_groups"] = F.shift(pv, frame), groups
        W["n_planted"] = F.shift(NR.planted_cloud(), frame)
        ft, fq, rows, fgroups, n0 = _planted()
        W["f_tgt"], W["f_q"], W["f_rows"], W["f_groups"], W["f_n0"] = F.shift(ft, frame), F.shift(fq, frame), rows, fgroups, n0
        prm = VR.params()
        W["D_cut"] = VR.distributions(W["cut"], prm)
        W["D_planted"] = VR.distributions(W["v_planted"], prm)
        W["VT_cut"] = VR.build_target(W["cut"], prm, W["D_cut"])
        W["VT_planted"] = VR.build_target(W["v_planted"], prm, W["D_planted"])
        W["NT_cut"] = NR.build_target(W["cut"], NR.params())
        W["NT_planted"] = NR.build_target(W["n_planted"], NR.params())
        W["FT_cut"] = FR.build_target(W["cut"], FR.params(), W["D_cut"])
        W["FT_planted"] = FR.build_target(W["f_tgt"], FR.params())
        W["FS"] = FR.prepare_source(W["src"], FR.params())
        assert F.in_range(W["cut"], W["v_planted"], W["n_planted"], W["f_tgt"], W["f_q"], FR.transform_points(W["guess"], W["FS"]["x"]))
        _VER[frame] = W
    return _VER[frame]


_VER = {}


@pytest.mark.parametrize("frame", FRAMES)
def test_verifier_census(frame):
    """the restatements alone: nearly every row of the moved clouds stands above the gap bars the existing tests use, the planted
    voxel populations survive the move, the cut has pairs at the moved guess and both lane and wavefront voxels"""
    import fgicp_ref as FR
    W = _verifier_world(frame)
    assert F.in_range(W["cut"], W["v_planted"], W["n_planted"], W["f_tgt"]) and len(W["cut"]) == 5000
    D = W["D_cut"]
    assert (D["gap"] >= 1e-6).sum() >= len(W["cut"]) - 5 and (D["eig_gap"] >= 1e-3).sum() >= len(W["cut"]) - 5
    assert {6, 9, 12, 24, 25, 40, 70, 3000} == set(W["NT_planted"]["counts"].tolist())
    assert {True, False} == set((W["VT_cut"]["counts"] > 48).tolist())
    pairs = FR.find_pairs(W["FT_cut"], W["FS"], W["guess"], FR.params())
    sure = (pairs["row_nn"] >= 1e-9) & (pairs["row_cut"] >= 1e-9)
    assert (pairs["idx"] >= 0).sum() > 0.5 * len(W["src"]) and sure.sum() >= len(W["src"]) - 2
    fin = W["D_planted"]["nbr"][:, 0] >= 0
    assert set(np.flatnonzero(~fin)) == set(W["v_groups"]["nan"])


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_vgicp_covariances_in_every_frame(gpu_ctx, frame):
    """neighbour lists equal wherever the restatement's k-th and (k + 1)-th distances stand apart; covariances at test_vgicp.py's bar"""
    import vgicp_ref as VR
    W = _verifier_world(frame)
    for what, xyz, D in (("cut", W["cut"], W["D_cut"]), ("planted", W["v_planted"], W["D_planted"])):
        cov, nbr = gpu_ctx.vgicp_covariances(_pcl(xyz), K)
        fin = D["nbr"][:, 0] >= 0
        assert np.isnan(cov[~fin]).all() and (nbr[~fin] == -1).all(), (frame, what)
        sure = fin & (D["gap"] >= 1e-6)
        assert np.array_equal(nbr[sure], D["nbr"][sure]), (frame, what, np.flatnonzero((nbr != D["nbr"]).any(1) & sure)[:8])
        defined = fin & (D["eig_gap"] >= 1e-3)
        err = np.abs(cov[defined] - VR.cov6(D["C"][defined])).max()
        print(f"[far vgicp] {frame} {what}: {int(sure.sum())} of {len(xyz)} rows above the gap bar, worst cov6 error {err:.3e}")
        assert err <= 1e-9, (frame, what, err)
    g = W["v_groups"]
    want = np.sort(g["identical"])[:K]                                     # the tie rule survives the move: identical points stay identical
    assert all(np.array_equal(nbr[i], want) for i in g["identical"])


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_fgicp_correspondences_in_every_frame(gpu_ctx, frame):
    """pair indices equal: the planted target under the identity (x' exact: every row, ties and face pairs included) and the scene cut
    at the moved guess (every row above the gap bars of test_fgicp.py)"""
    import fgicp_ref as FR
    import lisreg
    W = _verifier_world(frame)
    rows, g, n0 = W["f_rows"], W["f_groups"], W["f_n0"]
    eye = np.eye(4)
    for kind in (0, 1):
        P = lisreg.fgicp_default_params(kind)
        gpu_ctx.fgicp_set_target(VSLOT, _pcl(W["f_tgt"]), P)
        idx, sq = gpu_ctx.fgicp_correspondences(VSLOT, _pcl(W["f_q"]), P, eye)
        w_idx, w_sq, _, _ = FR.search(W["FT_planted"], W["f_q"].astype(np.float64), P.max_correspondence_distance)
        assert np.array_equal(idx, w_idx), (frame, kind, np.flatnonzero(idx != w_idx)[:8])
        assert np.array_equal(np.isnan(sq), np.isnan(w_sq)) and np.array_equal(sq[idx >= 0], w_sq[idx >= 0]), (frame, kind)
        assert not np.isin(idx, g["nan"]).any() and (idx[rows["nan"]] == -1).all(), (frame, kind)
        assert idx[rows["identical"]][0] == g["identical"].min() and sq[rows["identical"]][0] == 0.0, (frame, kind)
        assert idx[rows["mid_a"]][0] == n0 and idx[rows["mid_b"]][0] == n0 + 2 and sq[rows["mid_a"]][0] == 1.0, (frame, kind)
        if kind == 0:                                                      # (the integer offsets move the 5 m cut exactly)
            assert idx[rows["cut_on"]][0] == -1 and idx[rows["cut_on_inside"]][0] == -1, frame
            assert (idx[rows["face_near"]] >= 0).all() and (idx[rows["face_far"]] == -1).all() and idx[rows["corner_far"]][0] == -1, frame
        else:
            assert (idx[~np.isnan(W["f_q"]).any(1)] >= 0).all() and sq[rows["cut_on"]][0] == 25.0, frame
    P = lisreg.fgicp_default_params()
    gpu_ctx.fgicp_set_target(VSLOT, _pcl(W["cut"]), P)
    idx, sq = gpu_ctx.fgicp_correspondences(VSLOT, _pcl(W["src"]), P, W["guess"])
    want = FR.find_pairs(W["FT_cut"], W["FS"], W["guess"], FR.params())
    sure = (want["row_nn"] >= 1e-9) & (want["row_cut"] >= 1e-9)
    assert np.array_equal(idx[sure], want["idx"][sure]), (frame, np.flatnonzero((idx != want["idx"]) & sure)[:8])
    # The squared distances of equal pairs.  test_fgicp.py's bar of 1e-12 relative is one for coordinates of tens of metres; here x' =
    # ((R0 a0 + R1 a1) + R2 a2) + t is formed in double at |t| = 8 km on both sides, in an order the device may contract: each side is
    # within (5 max|a| + max|x'|) u of the exact x' per axis (u = 2^-53: three products, three sums), so the two differ by delta =
    # 2 (5 max|a| + max|x'|) u, the squared distances by 2 sqrt(3) d delta + 3 delta^2, plus 4 u d^2 for each side's own three
    # squares and two sums.
    both = (want["idx"] >= 0) & (idx == want["idx"])
    u = 2.0 ** -53
    xt = FR.transform_points(W["guess"], W["FS"]["x"])
    delta = 2.0 * (5.0 * np.abs(W["FS"]["x"]).max() + np.abs(xt).max()) * u
    d = np.sqrt(want["sq"][both])
    bar = 2.0 * np.sqrt(3.0) * d * delta + 3.0 * delta * delta + 8.0 * u * want["sq"][both]
    err = np.abs(sq[both] - want["sq"][both])
    rel = float(np.max(err / want["sq"][both]))
    print(f"[far fgicp] {frame}: {int(both.sum())} pairs of {len(idx)}, worst squared-distance error {rel:.3e} relative, "
          f"{float(np.max(err / bar)):.3f} of the rounding bar")
    assert both.sum() > 0.5 * len(idx) and np.all(err <= bar), (frame, rel, float(np.max(err / bar)))


@pytest.mark.gpu
@pytest.mark.parametrize("frame", FRAMES)
def test_hip_voxel_tables_in_every_frame(gpu_ctx, frame):
    """lisreg_ndt_get_voxels and lisreg_vgicp_get_voxels: cell ids and counts equal, means within 1e-12 of max|coordinate|, matrices
    within 1e-9 (test_ndt._check_voxels and test_vgicp's bars, unchanged: both sides centre on the double mean)"""
    import lisreg
    import vgicp_ref as VR
    from test_ndt import _check_voxels
    W = _verifier_world(frame)
    for what, xyz, T in (("cut", W["cut"], W["NT_cut"]), ("planted", W["n_planted"], W["NT_planted"])):
        info = gpu_ctx.ndt_set_target(VSLOT, _pcl(xyz), lisreg.ndt_default_params())
        assert info["dims"] == [int(v) for v in T["dims"]] and info["n_voxels"] == T["n_voxels"] and info["n_valid"] == len(T["cell_ids"])
        _check_voxels(gpu_ctx.ndt_get_voxels(VSLOT), T, xyz, f"{frame}, {what}")
    for what, xyz, T in (("cut", W["cut"], W["VT_cut"]), ("planted", W["v_planted"], W["VT_planted"])):
        info = gpu_ctx.vgicp_set_target(VSLOT + 1, _pcl(xyz), lisreg.vgicp_default_params())
        assert info == dict(dims=[int(v) for v in T["dims"]], n_voxels=len(T["cell_ids"]), n_points=T["n_points"]), (frame, what)
        V = gpu_ctx.vgicp_get_voxels(VSLOT + 1)
        assert np.array_equal(V["cell_ids"], T["cell_ids"]) and np.array_equal(V["counts"], T["counts"]), (frame, what)
        e_mean = np.abs(V["means"] - T["means"]).max() / np.nanmax(np.abs(xyz))
        # the mean covariance of a voxel is compared where every point in it has a defined normal
        low = np.flatnonzero(~(T["dist"]["eig_gap"] >= 1e-3) & (T["dist"]["nbr"][:, 0] >= 0))
        cells, _, _ = VR.NR.voxel_cells(xyz, 1.0)
        clean = ~np.isin(T["cell_ids"], cells[low])
        e_cov = np.abs(V["cov6"][clean] - VR.cov6(T["covs"])[clean]).max()
        print(f"[far vgicp] {frame} {what}: {len(T['cell_ids'])} voxels, mean error / max|coordinate| {e_mean:.3e}, cov6 error {e_cov:.3e}")
        assert clean.sum() > 100 and e_mean <= 1e-12 and e_cov <= 1e-9, (frame, what, e_mean, e_cov)
