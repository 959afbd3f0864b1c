"""lisreg_ndt_set_target_batch (lis-slam_amd/csrc/lisreg_ndt_target_batch.hip): the NDT targets of a candidate list in
one call, against single lisreg_ndt_set_target calls on a fresh context.

Equality is byte for byte: everything lisreg_ndt_get_target reads back (info, the voxel grid, the search grid's geometry and the bounding
box, the points by cell, the cells' starts, the dense table, and the cell id, the flag and the ten doubles of EVERY voxel record, valid
or not), the valid voxels of lisreg_ndt_get_voxels, the returned info and what lisreg_ndt_derivatives returns on the slot, with and
without the Hessian, for a 48-point source at a small offset.  Where the test says so the voxels are also held to the definition
(tests/ndt_ref.build_target) at the bars tests/test_ndt.py holds the single call to: the valid set and the counts equal, means within
1e-12 of the largest coordinate, C^-1 within 1e-9 of max|C^-1| per voxel."""
import ctypes as C

import numpy as np
import pytest

import ndt_ref as R

pytestmark = pytest.mark.gpu
TILE = 256                     # records per workgroup of the batch's per-record kernels (kFtTile, kBlockQ)
NO_TARGET = "no NDT target in this slot (lisreg_ndt_set_target)"
NAN = np.nan


def _rec(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def _cloud(n, seed, shift=(0, 0, 0), extent=(4, 4, 4), holes=()):
    """n random points of a box of `extent` at `shift`; holes: positions made NaN records, of the three kinds in turn (as
    tests/test_vgicp_target_batch.py makes them)"""
    xyz = (np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)) * np.array(extent) + np.array(shift)).astype(np.float32)
    for h, kind in zip(holes, range(len(holes))):
        # (the second kind has a finite coordinate outside the box: the bounding box takes every coordinate on its own, as cloud_bbox does)
        xyz[h] = [(NAN, NAN, NAN), (NAN, -7.0, 1.0), (1.0, 1.0, NAN)][kind % 3]
    return xyz


class Fresh:
    """a context of its own with the clouds on its device"""

    def __init__(self):
        import lisreg
        self.lisreg = lisreg
        self.ctx = lisreg.Context(0)
        self.P = lisreg.ndt_default_params()
        self.keep = []

    def dev(self, xyz):
        d = self.lisreg.DeviceArray(_rec(xyz))
        self.keep.append(d)
        return (d.ptr, len(xyz))

    def close(self):
        self.ctx.close()
        for d in self.keep:
            d.free()


@pytest.fixture
def pair():
    a, b = Fresh(), Fresh()
    yield a, b
    a.close()
    b.close()


def _source_for(xyz):
    fin = xyz[~np.isnan(xyz).any(1)]
    return (fin[:48] + np.float32(0.03)).astype(np.float32)


def snapshot(f, slot, xyz=None, P=None):
    """every byte of the slot a later call can observe"""
    g = f.ctx.ndt_get_target(slot)
    v = f.ctx.ndt_get_voxels(slot)
    out = {k: np.asarray(x) for k, x in g.items()}
    out.update(v_cell_ids=v["cell_ids"], v_counts=v["counts"], v_means=v["means"], v_icov6=v["icov6"])
    assert len(v["cell_ids"]) == g["n_valid"] == int(g["record_flags"].sum()) == int((g["table"] >= 0).sum())
    assert int((g["records"][:, 9] > 0).sum()) == g["n_voxels"] and g["n_voxels"] <= g["n_records"] <= g["n_voxels"] + 1
    if xyz is not None:
        src = f.dev(_source_for(xyz))
        p = np.array([0.01, -0.02, 0.015, 0.002, -0.001, 0.003])
        for hess in (True, False):
            out[f"der{int(hess)}"], pairs = f.ctx.ndt_derivatives(slot, src, P or f.P, p, with_hessian=hess)
            out[f"pairs{int(hess)}"] = np.int64(pairs)
    return out


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    return True


def single_then_batch(pair, clouds, slots=None, order=None, P=None):
    """clouds set one by one on pair[0], in one batch call on pair[1] (jobs in `order`); returns (singles, batch) snapshots by job"""
    a, b = pair
    P = P or a.P
    slots = slots or list(range(3, 3 + len(clouds)))
    singles = []
    for xyz, s in zip(clouds, slots):
        info = a.ctx.ndt_set_target(s, a.dev(xyz), P)
        singles.append((info, snapshot(a, s, xyz, P)))
    order = list(range(len(clouds))) if order is None else order
    devs = [b.dev(xyz) for xyz in clouds]
    res = b.ctx.ndt_set_target_batch([(slots[i], devs[i]) for i in order], P)
    batch = [None] * len(clouds)
    for pos, i in enumerate(order):
        assert res[pos]["status"] == 0, (i, b.ctx.last_error())
        batch[i] = (res[pos], snapshot(b, slots[i], clouds[i], P))
    for i, ((si, ss), (bi, bs)) in enumerate(zip(singles, batch)):
        assert {k: bi[k] for k in ("dims", "n_voxels", "n_valid")} == si, i            # the returned info
        assert same(ss, bs), i
    return singles, batch


def check_definition(xyz, snap, prm, what):
    """the slot's valid voxels against tests/ndt_ref.build_target, at the bars of tests/test_ndt.py (_check_voxels)"""
    T = R.build_target(xyz, prm)
    assert list(snap["dims"]) == [int(v) for v in T["dims"]] and list(snap["min_b"]) == [int(v) for v in T["min_b"]]
    assert snap["n_voxels"] == T["n_voxels"] and snap["n_valid"] == len(T["cell_ids"])
    assert np.array_equal(snap["v_cell_ids"], T["cell_ids"]), (what, "valid set")
    assert np.array_equal(snap["v_counts"], T["counts"]), (what, "counts")
    if len(T["cell_ids"]):
        e_mean = np.max(np.abs(snap["v_means"] - T["means"])) / np.nanmax(np.abs(xyz))
        ic = R.icov6(T["icov"])
        e_ic = np.max(np.max(np.abs(snap["v_icov6"] - ic), 1) / np.max(np.abs(ic), 1))
        print(f"[ndt_target_batch] {what}: {len(T['cell_ids'])} valid voxels, mean error / max|coordinate| {e_mean:.3e}, "
              f"C^-1 error / max|C^-1| {e_ic:.3e}")
        assert e_mean <= 1e-12, (what, e_mean)
        assert e_ic <= 1e-9, (what, e_ic)
    # the dense table names every valid voxel's record at its cell and nothing else
    tab, rc, rf = snap["table"], snap["record_cells"], snap["record_flags"]
    assert np.all(np.diff(rc) > 0)
    assert np.array_equal(tab[rc[rf == 1]], np.flatnonzero(rf == 1)) and (tab >= 0).sum() == (rf == 1).sum()


# ---- tile and block boundaries ---------------------------------------------------------------------------------------------------------
def boundary_clouds():
    clouds = []
    for n in (255, 256, 257, 511, 513, 1500):
        holes = ()
        if n == 1500:
            holes = (0, n - 1, TILE - 1, TILE, 5 * TILE)           # the first, the last, a tile's last and first record
        elif n in (257, 513):
            holes = (10, TILE - 1, TILE)
        elif n == 511:
            holes = (TILE, 510, 0)
        clouds.append(_cloud(n, 100 + n, holes=holes))
    return clouds


def test_tile_boundaries_equal_single_calls_and_the_definition(pair):
    clouds = boundary_clouds()
    singles, batch = single_then_batch(pair, clouds, slots=[40, 7, 65535, 0, 300, 12], order=[4, 3, 5, 2, 1, 0])
    assert [b[1]["n_points"] for b in batch] == [255, 256, 254, 508, 510, 1495]
    prm = R.params()
    for xyz, (_, snap) in zip(clouds, batch):
        check_definition(xyz, snap, prm, f"{len(xyz)} records")


# ---- the lane / wavefront threshold ------------------------------------------------------------------------------------------------------
def planted(counts, seed, shift=(0, 0, 0), corner_nans=0):
    """clusters of the given sizes inside distinct unit cells (every second cell along x, the first one the box's minimum-corner cell),
    away from the cell faces, plus corner_nans NaN records, in shuffled order"""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(0.2, 0.8, (c, 3)) + np.array([2 * i, 0, 0]) + np.array(shift) for i, c in enumerate(counts)]
    parts.append(np.full((corner_nans, 3), NAN))
    xyz = np.concatenate(parts).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]


def test_the_48_49_threshold_counts_nan_records(pair):
    sizes = [10, 48, 49, 64, 65, 130]
    clouds = [planted(sizes, 7, (10, 20, 0), corner_nans=38),      # the corner voxel's run: 48 records, the lane path
              planted(sizes, 7, (10, 20, 0), corner_nans=39),      # 49 records: the wavefront path
              planted([60, 3, 200, 48, 49], 8, (-30, 5, 2))]
    singles, batch = single_then_batch(pair, clouds)
    for i in (0, 1):
        snap = batch[i][1]
        assert list(snap["records"][:, 9].astype(int)) == sizes and list(snap["record_cells"][:1]) == [0]
        assert snap["n_records"] == 6 and snap["n_voxels"] == 6 and snap["n_valid"] == 6
        check_definition(clouds[i], snap, R.params(), f"threshold cloud {i}")
    # the corner voxel's ten finite points are the same in both clouds; which path summed them may show in the last bits only
    r0, r1 = batch[0][1]["records"][0], batch[1][1]["records"][0]
    assert np.abs(r0[:3] - r1[:3]).max() <= 1e-12 * 21 and r0[9] == r1[9] == 10
    # and with the targets the other way round: another first voxel for each
    single_then_batch(pair, clouds[::-1], slots=[11, 12, 13])


# ---- the NaN-only corner voxel -------------------------------------------------------------------------------------------------------------
def test_the_nan_only_corner_voxel_has_a_record_and_shifts_the_numbering(pair):
    rng = np.random.default_rng(3)
    body = rng.uniform(1.2, 4.8, (400, 3))
    # the per-axis minima come from three different points: the minimum corner's cell holds no finite point
    ext = np.array([[0.1, 2.5, 2.5], [2.5, 0.1, 2.5], [2.5, 2.5, 0.1]])
    fin = np.concatenate([body, ext]).astype(np.float32)
    with_nan = np.concatenate([fin, np.array([[NAN, NAN, NAN], [NAN, 2.0, 2.0], [3.0, NAN, 1.0], [2.0, 2.0, NAN]], np.float32)])
    with_nan = with_nan[rng.permutation(len(with_nan))]
    singles, batch = single_then_batch(pair, [with_nan, fin])
    s_nan, s_fin = batch[0][1], batch[1][1]
    assert s_nan["record_cells"][0] == 0 and s_nan["records"][0, 9] == 0 and s_nan["record_flags"][0] == 0      # a record with count 0
    assert s_fin["record_cells"][0] != 0
    assert s_nan["n_records"] == s_fin["n_records"] + 1 and s_nan["n_voxels"] == s_fin["n_voxels"]
    assert s_nan["table"][0] == -1
    # the same voxels, every number one higher
    assert np.array_equal(s_nan["record_cells"][1:], s_fin["record_cells"])
    both = s_fin["table"] >= 0
    assert np.array_equal(s_nan["table"][both], s_fin["table"][both] + 1) and np.array_equal(s_nan["table"] >= 0, both)
    check_definition(with_nan, s_nan, R.params(), "NaN-only corner voxel")
    check_definition(fin, s_fin, R.params(), "the same without NaN records")


# ---- validity edges ------------------------------------------------------------------------------------------------------------------------
def validity_cloud():
    rng = np.random.default_rng(5)

    def cell(i, pts):
        return np.asarray(pts, np.float64) + np.array([2 * i, 0, 0])
    parts = [cell(0, rng.uniform(0.2, 0.8, (5, 3))), cell(1, rng.uniform(0.2, 0.8, (6, 3))), cell(2, rng.uniform(0.2, 0.8, (7, 3))),
             cell(3, rng.uniform(0.2, 0.8, (1, 3))), cell(4, [[0.3, 0.5, 0.5], [0.7, 0.5, 0.5]]),
             cell(5, np.full((6, 3), 0.5)),                                                        # coincident
             cell(6, np.c_[np.linspace(0.2, 0.8, 7), np.full(7, 0.5), np.full(7, 0.25)]),          # collinear (along an axis: exact zeros)
             cell(7, np.c_[rng.uniform(0.2, 0.8, (8, 2)), np.full(8, 0.5)]),                       # coplanar
             cell(8, rng.uniform(0.2, 0.8, (20, 3)))]
    xyz = np.concatenate(parts).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]


@pytest.mark.parametrize("min_pts", [6, 1])
def test_validity_edges(pair, min_pts):
    a, _ = pair
    P = a.lisreg.ndt_default_params(min_points_per_voxel=min_pts)
    xyz = validity_cloud()
    singles, batch = single_then_batch(pair, [xyz, _cloud(300, 71)], P=P)
    snap = batch[0][1]
    counts = snap["records"][:, 9].astype(int).tolist()
    assert counts == [5, 6, 7, 1, 2, 6, 7, 8, 20] and snap["n_voxels"] == 9
    flags = snap["record_flags"].tolist()
    if min_pts == 6:
        assert flags == [0, 1, 1, 0, 0, 0, 1, 1, 1]
    else:
        assert flags == [1, 1, 1, 0, 1, 0, 1, 1, 1]                                   # one point: n >= 2 fails; coincident: no variance
    # the voxels of distinct points against the definition (the two-point voxel is a collinear one; the definition needs no n >= 2 rule
    # of its own when it is asked for two points at least)
    check_definition(xyz, snap, R.params(min_points_per_voxel=max(min_pts, 2)), f"validity edges, min_points_per_voxel {min_pts}")


# ---- failures ------------------------------------------------------------------------------------------------------------------------------
def failing_clouds():
    inf = _cloud(300, 12)
    inf[150, 1] = np.inf
    nan_only = np.full((30, 3), NAN, np.float32)
    box_only = np.array([[1.0, 2.0, NAN], [NAN, 3.0, 4.0], [2.0, NAN, 5.0], [1.5, 2.5, NAN]], np.float32)   # a finite box, no finite record
    huge = _cloud(21, 16)
    huge[0], huge[1] = (0, 0, 0), (500, 500, 500)                                      # 501^3 voxels at resolution 1: more than 2^26
    five = _cloud(5, 17, extent=(0.5, 0.5, 0.5))                                        # no voxel of six points
    return dict(inf=inf, nan_only=nan_only, box_only=box_only, huge=huge, five=five)


def test_failures_stay_with_their_target(pair):
    a, b = pair
    bad = failing_clouds()
    kinds = list(bad)
    clouds = [_cloud(500, 10)] + [bad[k] for k in kinds] + [_cloud(257, 13, holes=(256,)), _cloud(64, 14, extent=(1, 1, 1))]
    slots = list(range(3, 3 + len(clouds)))
    bad_at = list(range(1, 1 + len(kinds)))
    good_at = [0, len(clouds) - 2, len(clouds) - 1]
    # every slot of a job that will fail holds a valid target before
    for i in bad_at:
        b.ctx.ndt_set_target(slots[i], b.dev(_cloud(100, 15, extent=(1, 1, 1))), b.P)
        assert b.ctx.ndt_get_target(slots[i])["n_points"] == 100
    res = b.ctx.ndt_set_target_batch([(s, b.dev(x)) for s, x in zip(slots, clouds)], b.P)
    E = b.lisreg.ERR_ARG
    assert [r["status"] for r in res] == [0] + [E] * len(kinds) + [0, 0]
    assert b.ctx.last_error() == "ndt_set_target_batch: job 1: ndt_set_target: the cloud has infinite coordinates"
    texts = {}
    src = _source_for(clouds[0])
    for i, kind in zip(bad_at, kinds):
        with pytest.raises(a.lisreg.LisregError) as single:
            a.ctx.ndt_set_target(slots[i], a.dev(clouds[i]), a.P)
        texts[kind] = str(single.value)
        for f in (a, b):
            with pytest.raises(f.lisreg.LisregError) as e:
                f.ctx.ndt_align(slots[i], f.dev(src), f.P)
            assert NO_TARGET in str(e.value) and "ndt_align" in str(e.value)
            with pytest.raises(f.lisreg.LisregError):
                f.ctx.ndt_get_target(slots[i])
    assert "infinite coordinates" in texts["inf"] and "no finite point" in texts["nan_only"]
    assert "fewer finite points than k_correspondences" in texts["box_only"]
    assert "more than 2^26 cells (the cell table is dense" in texts["huge"] and "no valid voxel (min_points_per_voxel" in texts["five"]
    # the last kind is known only at the end: info is filled as the single call fills it before refusing
    info = a.lisreg.NdtInfo()
    d = a.dev(bad["five"])
    assert a.lisreg.lib().lisreg_ndt_set_target(a.ctx._h, 90, C.c_void_p(d[0]), d[1], 16, a.lisreg.FMT_DEVICE, C.byref(a.P), C.byref(info)) == E
    five = res[bad_at[kinds.index("five")]]
    assert (five["dims"], five["n_voxels"], five["n_valid"]) == (list(info.dims), info.n_voxels, 0) and info.n_valid == 0 and info.n_voxels >= 1
    for i in good_at:
        a.ctx.ndt_set_target(slots[i], a.dev(clouds[i]), a.P)
        assert same(snapshot(a, slots[i], clouds[i]), snapshot(b, slots[i], clouds[i])), i
    # every kind alone among good targets: the first failure named is the first failed JOB, with the single call's text behind the job
    for kind in kinds:
        word = texts[kind]
        tail = word[word.index("ndt_set_target: "):]
        res = b.ctx.ndt_set_target_batch([(20, b.dev(clouds[0])), (21, b.dev(bad[kind])), (22, b.dev(bad["nan_only"]))], b.P)
        assert [r["status"] for r in res] == [0, E, E], kind
        assert b.ctx.last_error() == "ndt_set_target_batch: job 1: " + tail, kind
        assert same(snapshot(b, 20, clouds[0]), snapshot(a, slots[0], clouds[0])), kind


# ---- whole-call refusals -------------------------------------------------------------------------------------------------------------------
def test_whole_call_refusals_touch_nothing(pair):
    a, _ = pair
    L, lisreg = a.lisreg.lib(), a.lisreg
    held = _cloud(300, 21)
    a.ctx.ndt_set_target(3, a.dev(held), a.P)
    want = snapshot(a, 3, held)
    good = a.dev(_cloud(200, 22, extent=(2, 2, 2)))

    def call(jobs, n=None, params=a.P, null_jobs=False):
        arr = (lisreg.NdtTargetJob * max(len(jobs), 1))()
        for k, (slot, (ptr, cnt)) in enumerate(jobs):
            arr[k].slot, arr[k].cloud, arr[k].n = slot, ptr, cnt
            arr[k].status, arr[k].info.n_valid, arr[k].info.dims[0], arr[k].info.n_voxels = 77, 123, 45, 9
        rc = L.lisreg_ndt_set_target_batch(a.ctx._h, len(jobs) if n is None else n, None if null_jobs else arr,
                                           C.byref(params) if params is not None else None)
        for k in range(len(jobs)):
            assert (arr[k].status, arr[k].info.n_valid, arr[k].info.dims[0], arr[k].info.n_voxels) == (77, 123, 45, 9), "a refused call wrote a job field"
        return rc

    ok = (3, good)
    big = lisreg.NDT_TARGET_BATCH_MAX_POINTS // 2 + 1
    cases = {
        "null jobs": dict(jobs=[ok], null_jobs=True),
        "null params": dict(jobs=[ok], params=None),
        "resolution 0": dict(jobs=[ok], params=lisreg.ndt_default_params(resolution=0.0)),
        "outlier_ratio 1": dict(jobs=[ok], params=lisreg.ndt_default_params(outlier_ratio=1.0)),
        "negative min_covar_eigvalue_mult": dict(jobs=[ok], params=lisreg.ndt_default_params(min_covar_eigvalue_mult=-1.0)),
        "slot -1": dict(jobs=[ok, (-1, good)]),
        "slot 65536": dict(jobs=[ok, (65536, good)]),
        "slot twice": dict(jobs=[ok, (9, good), (3, good)]),
        "n 0": dict(jobs=[ok, (4, (good[0], 0))]),
        "n negative": dict(jobs=[ok, (4, (good[0], -5))]),
        "null cloud": dict(jobs=[ok, (4, (None, 50))]),
        "negative n_targets": dict(jobs=[ok], n=-1),
        "too many targets": dict(jobs=[(s, good) for s in range(lisreg.NDT_TARGET_BATCH_MAX + 1)]),
        "too many points": dict(jobs=[(3, (good[0], big)), (4, (good[0], big))]),
    }
    bare = {k: v for k, v in want.items() if not k.startswith(("der", "pairs"))}
    for name, kw in cases.items():
        assert a.ctx.ndt_set_target_batch([(8, good)], a.P)[0]["status"] == 0 and a.ctx.ndt_target_batch_counts()[1] == 2
        assert call(**kw) == lisreg.ERR_ARG, name
        assert "ndt_set_target_batch" in a.ctx.last_error(), name
        assert same(snapshot(a, 3), bare), name
        assert a.ctx.ndt_target_batch_counts() == (0, 0), name                         # nothing enqueued, nothing waited for
    assert same(snapshot(a, 3, held), want)
    with pytest.raises(lisreg.LisregError):
        a.ctx.ndt_get_target(4)                                                        # no refused call made a slot
    assert lisreg.NDT_TARGET_BATCH_MAX == 1024 and lisreg.NDT_TARGET_BATCH_MAX_POINTS == 1 << 27
    assert call([], n=0) == lisreg.OK and call([], n=0, null_jobs=True) == lisreg.OK
    assert a.ctx.ndt_target_batch_counts() == (0, 0)
    assert same(snapshot(a, 3, held), want)
    # the read-back hook's own refusals
    info = lisreg.NdtInfo()
    buf = (C.c_int * 4)()
    N = None
    assert L.lisreg_ndt_get_target(a.ctx._h, 3, C.byref(info), N, N, N, N, N, N, N, N, buf, N, N, N, N, 0, 4, 0, 0) == lisreg.ERR_ARG
    assert info.n_valid == want["n_valid"] and "capacity_cells" in a.ctx.last_error()
    assert L.lisreg_ndt_get_target(a.ctx._h, 3, N, N, N, N, N, N, N, N, N, N, buf, N, N, N, 0, 0, 1, 0) == lisreg.ERR_ARG
    assert "capacity_table" in a.ctx.last_error()
    assert L.lisreg_ndt_get_target(a.ctx._h, 3, N, N, N, N, N, N, N, N, N, N, N, N, buf, N, 0, 0, 0, 1) == lisreg.ERR_ARG
    assert "capacity_records" in a.ctx.last_error()
    assert L.lisreg_ndt_get_target(a.ctx._h, 3, N, N, N, N, N, N, N, N, N, N, N, N, N, N, -1, 0, 0, 0) == lisreg.ERR_ARG


# ---- reuse ---------------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_one_and_slots_that_held_other_targets(pair):
    a, b = pair
    mid = _cloud(1000, 31, holes=(5,))
    a.ctx.ndt_set_target(3, a.dev(mid), a.P)
    want = snapshot(a, 3, mid)
    big = [_cloud(5000, 32, extent=(20, 20, 3)), _cloud(4000, 35, extent=(9, 9, 9), holes=(1, 2, 3))]
    b.ctx.ndt_set_target_batch([(3, b.dev(big[0])), (4, b.dev(big[1]))], b.P)          # bigger targets in the slots first
    res = b.ctx.ndt_set_target_batch([(3, b.dev(mid))], b.P)                            # a batch of one
    assert res[0]["status"] == 0 and same(snapshot(b, 3, mid), want)
    res = b.ctx.ndt_set_target_batch([(4, b.dev(mid)), (3, b.dev(mid))], b.P)           # the batch called again: the same bytes
    assert [r["status"] for r in res] == [0, 0] and same(snapshot(b, 4, mid), want) and same(snapshot(b, 3, mid), want)
    # and a single call over a slot a batch set
    small = _cloud(64, 34, extent=(1, 1, 1))
    b.ctx.ndt_set_target(4, b.dev(small), b.P)
    a.ctx.ndt_set_target(4, a.dev(small), a.P)
    assert same(snapshot(b, 4, small), snapshot(a, 4, small))
    assert b.ctx.ndt_set_target_batch([], b.P) == [] and b.ctx.ndt_target_batch_counts() == (0, 0)
    assert same(snapshot(b, 3, mid), want)


# ---- counts --------------------------------------------------------------------------------------------------------------------------------
def test_launches_and_synchronisations_do_not_depend_on_the_number_of_targets(pair):
    _, b = pair
    counts = []
    for n in (1, 17):
        jobs = [(3 + i, b.dev(_cloud(300 + 17 * i, 50 + i))) for i in range(n)]
        res = b.ctx.ndt_set_target_batch(jobs, b.P)
        assert all(r["status"] == 0 for r in res)
        counts.append(b.ctx.ndt_target_batch_counts())
    print(f"[ndt_target_batch] (enqueues, synchronisations) for 1 and for 17 targets: {counts}")
    assert counts[0] == counts[1] and counts[0][1] == 2 and 0 < counts[0][0] <= 24
    # a refused call enqueues nothing and waits for nothing
    with pytest.raises(b.lisreg.LisregError):
        b.ctx.ndt_set_target_batch([(3, jobs[0][1]), (3, jobs[1][1])], b.P)
    assert b.ctx.ndt_target_batch_counts() == (0, 0)


# ---- consumers -----------------------------------------------------------------------------------------------------------------------------
def test_four_slots_verify_like_singly_set_slots(pair):
    a, b = pair
    rng = np.random.default_rng(9)
    # four targets of about 3 000 points (a floor, two walls, a crowded voxel), the third one far from the origin
    slots = [20, 21, 22, 23]
    targets, srcs, guesses = [], [], []
    for k in range(4):
        n = 3000 + 100 * k
        floor = np.c_[rng.uniform(0, 12, (n // 2, 2)), rng.normal(0, 0.02, n // 2)]
        wall = np.c_[rng.uniform(0, 12, n // 4), rng.normal(0, 0.02, n // 4), rng.uniform(0, 3, n // 4)]
        wall2 = np.c_[rng.normal(0, 0.02, n // 4), rng.uniform(0, 12, n // 4), rng.uniform(0, 3, n // 4)]
        blob = rng.uniform(0.1, 0.9, (100, 3)) + np.array([5.0, 5.0, 1.0])                # one voxel of a hundred points
        x = np.concatenate([floor, wall, wall2, blob])
        x[rng.integers(0, len(x), 7)] = NAN
        if k == 2:
            x = x + np.array([8000.0, -8000.0, 100.0])                                  # the far frame
        targets.append(x.astype(np.float32))
        fin = targets[-1][~np.isnan(targets[-1]).any(1)]
        srcs.append((fin[rng.choice(len(fin), 300, replace=False)].astype(np.float64) + np.array([0.05, -0.04, 0.02])).astype(np.float32))
        g = np.eye(4, dtype=np.float32)
        g[:3, 3] = rng.uniform(-0.03, 0.03, 3)
        guesses.append(g)
    for s, x in zip(slots, targets):
        a.ctx.ndt_set_target(s, a.dev(x), a.P)
    res = b.ctx.ndt_set_target_batch([(s, b.dev(x)) for s, x in zip(slots, targets)], b.P)
    assert all(r["status"] == 0 for r in res)
    for s, x in zip(slots, targets):
        assert same(snapshot(a, s, x), snapshot(b, s, x)), s
    assert {True, False} == set((b.ctx.ndt_get_target(20)["records"][:, 9] > 48).tolist())     # the lane and the wavefront form
    assert b.ctx.ndt_get_target(22)["geom"][5] >= 7999.0
    check_definition(targets[2], snapshot(b, 22), R.params(), "far frame")
    out = []
    for f in (a, b):
        one = [f.ctx.ndt_align(s, f.dev(src), f.P, g) for s, src, g in zip(slots, srcs, guesses)]
        many = f.ctx.ndt_align_batch([f.dev(src) for src in srcs], [f.lisreg.NdtItem(k, s, g) for k, (s, g) in enumerate(zip(slots, guesses))], f.P)
        out.append((one, many))
    (one0, (r0, f0, i0)), (one1, (r1, f1, i1)) = out
    assert f0.tobytes() == f1.tobytes() and i0 == i1 and i1["best"] >= 0
    for x, y in list(zip(r0, r1)) + list(zip(one0, one1)):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    assert any(r["converged"] for r in r1) and all(r["n_pairs_last"] > 0 for r in r1)


# ---- memory --------------------------------------------------------------------------------------------------------------------------------
def test_twenty_batches_do_not_grow_device_memory(pair):
    _, b = pair
    hip = b.lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    clouds = boundary_clouds()
    jobs = [(3 + i, b.dev(x)) for i, x in enumerate(clouds)]
    b.ctx.ndt_set_target_batch(jobs, b.P)                                               # every buffer of the call is made
    first = [snapshot(b, s) for s, _ in jobs]
    before = free_bytes()
    for _ in range(20):
        res = b.ctx.ndt_set_target_batch(jobs, b.P)
    assert free_bytes() == before and all(r["status"] == 0 for r in res)
    assert all(same(snapshot(b, s), f) for (s, _), f in zip(jobs, first))


# ---- a caller's busy stream ------------------------------------------------------------------------------------------------------------------
import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


def test_batch_on_a_callers_busy_stream(env):
    """the clouds arrive late on the caller's stream, as in tests/test_caller_stream.py: the slots equal those set on the idle stream,
    and a context left on its own stream reads the decoy"""
    e = env
    P = e.lisreg.ndt_default_params()
    parts = [_cloud(3000, 61, extent=(10, 10, 2)), _cloud(700, 62, shift=(50, 0, 0), holes=(3, 256)), _cloud(1300, 63, extent=(3, 8, 3))]
    rs = np.concatenate([_rec(p) for p in parts])
    offs = np.r_[0, np.cumsum([len(p) for p in parts])]
    slots = [40, 41, 42]

    def make(dst):
        def run():
            return e.ctx.ndt_set_target_batch([(s, (dst.ptr + 16 * int(offs[i]), len(parts[i]))) for i, s in enumerate(slots)], P)

        def fetch(res):
            out = {}
            for s, r in zip(slots, res):
                assert r["status"] == 0
                g = e.ctx.ndt_get_target(s)
                out.update({f"{s}_{k}": np.asarray(x) for k, x in g.items()})
            return out
        return run, fetch
    TCS.late_case(e, "ndt_set_target_batch (device records)", rs, TCS.moved(rs), make)
