"""lisreg_vgicp_set_target_batch (lis-slam_amd/csrc/lisreg_vgicp_target_batch.hip): the VGICP targets of a candidate list
in one call, against single lisreg_vgicp_set_target calls on a fresh context.

Equality is byte for byte: everything lisreg_vgicp_get_target reads back (info, the voxel grid, the search grid's geometry and the
bounding box, the points by cell, the cells' starts, the dense table), the voxel records of lisreg_vgicp_get_voxels, the returned info
and what lisreg_vgicp_linearize returns on the slot, with and without the Hessian, for a 48-point source.  The voxels are also held to
the definition (tests/vgicp_ref.build_target) at the bars tests/test_vgicp.py holds the single call to: cell ids and counts equal, means
within 1e-12 of the largest coordinate, the mean covariance within 1e-9 absolute for every voxel all of whose points lie above the
restatement's gap bars (neighbour gap >= 1e-6, eigenvalue gap >= 1e-3)."""
import ctypes as C

import numpy as np
import pytest

import vgicp_ref as R

pytestmark = pytest.mark.gpu
K = 20
TILE = 256                     # points per workgroup of the batch's per-point kernels (kFtTile)
NO_TARGET = "no VGICP target in this slot (lisreg_vgicp_set_target)"
TARGET_KEYS = ("dims", "n_voxels", "n_points", "min_b", "resolution", "geom", "grid_dims", "sorted", "cell_start", "table",
               "v_cell_ids", "v_counts", "v_means", "v_cov6")


def _rec(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def _cloud(n, seed, shift=(0, 0, 0), extent=(4, 4, 4), holes=()):
    """n random points of a box of `extent` at `shift`; holes: positions made NaN points"""
    xyz = (np.random.default_rng(seed).uniform(0.0, 1.0, (n, 3)) * np.array(extent) + np.array(shift)).astype(np.float32)
    for h, kind in zip(holes, range(len(holes))):
        # (the second kind has a finite coordinate outside the box: the bounding box takes every coordinate on its own, as cloud_bbox does)
        xyz[h] = [(np.nan, np.nan, np.nan), (np.nan, -7.0, 1.0), (1.0, 1.0, np.nan)][kind % 3]
    return xyz


class Fresh:
    """a context of its own with the clouds on its device"""

    def __init__(self):
        import lisreg
        self.lisreg = lisreg
        self.ctx = lisreg.Context(0)
        self.P = lisreg.vgicp_default_params()
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
    g = f.ctx.vgicp_get_target(slot)
    v = f.ctx.vgicp_get_voxels(slot)
    out = {k: np.asarray(g[k]) for k in TARGET_KEYS if k in g}
    out.update(v_cell_ids=v["cell_ids"], v_counts=v["counts"], v_means=v["means"], v_cov6=v["cov6"])
    assert len(v["cell_ids"]) == g["n_voxels"]
    if xyz is not None:
        src = f.dev(_source_for(xyz))
        for hess in (True, False):
            lin, pairs = f.ctx.vgicp_linearize(slot, src, P or f.P, np.eye(4), with_hessian=hess)
            out[f"lin{int(hess)}"] = np.asarray(lin)
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
        info = a.ctx.vgicp_set_target(s, a.dev(xyz), P)
        singles.append((info, snapshot(a, s, xyz, P)))
    order = list(range(len(clouds))) if order is None else order
    devs = [b.dev(xyz) for xyz in clouds]
    res = b.ctx.vgicp_set_target_batch([(slots[i], devs[i]) for i in order], P)
    batch = [None] * len(clouds)
    for pos, i in enumerate(order):
        assert res[pos]["status"] == 0, (i, b.ctx.last_error())
        batch[i] = (res[pos], snapshot(b, slots[i], clouds[i], P))
    for i, ((si, ss), (bi, bs)) in enumerate(zip(singles, batch)):
        assert {k: bi[k] for k in ("dims", "n_voxels", "n_points")} == si, i          # the returned info
        assert same(ss, bs), i
    return singles, batch


def block_boundary_clouds():
    sizes = (20, 21, 63, 64, 65, 127, 129, 2939)
    clouds = []
    for n in sizes:
        holes = ()
        if n == 2939:
            holes = (0, n - 1, TILE - 1, TILE, 5 * TILE)          # the first, the last, both sides of a tile boundary
        elif n in (65, 129):
            holes = (10, 63, 64)
        clouds.append(_cloud(n, 100 + n, holes=holes))
    return clouds


def check_definition(xyz, snap, prm):
    """the slot's voxels against tests/vgicp_ref.build_target, at the bars of tests/test_vgicp.py"""
    T = R.build_target(xyz, prm)
    D = T["dist"]
    m = T["n_points"]
    assert snap["n_points"] == m and list(snap["dims"]) == [int(v) for v in T["dims"]] and list(snap["min_b"]) == [int(v) for v in T["min_b"]]
    assert np.array_equal(snap["v_cell_ids"], T["cell_ids"]) and np.array_equal(snap["v_counts"], T["counts"])
    assert np.abs(snap["v_means"] - T["means"]).max() <= 1e-12 * np.nanmax(np.abs(xyz))
    fin = ~np.isnan(xyz).any(1)
    sure = fin & (D["gap"] >= 1e-6) & (D["eig_gap"] >= 1e-3)
    assert sure.sum() >= 0.99 * m - 2                              # only points under the gap bars are left out
    cells, _, _ = R.NR.voxel_cells(xyz, prm["resolution"])
    clean = ~np.isin(T["cell_ids"], cells[fin & ~sure])
    err = np.abs(snap["v_cov6"][clean] - R.cov6(T["covs"])[clean]).max() if clean.any() else 0.0
    print(f"[vgicp_target_batch] {len(xyz)} points, {m} finite, {sure.sum()} above the gap bars, {clean.sum()} of {len(clean)} voxels "
          f"compared: worst cov6 error {err:.3e}")
    assert err <= 1e-9
    # the dense table names every voxel at its cell and nothing else
    tab = snap["table"]
    assert (tab >= 0).sum() == len(T["cell_ids"]) and np.array_equal(tab[T["cell_ids"]], np.arange(len(T["cell_ids"])))


# ---- block and tile boundaries ---------------------------------------------------------------------------------------------------------
def test_block_boundaries_equal_single_calls_and_the_definition(pair):
    clouds = block_boundary_clouds()
    singles, batch = single_then_batch(pair, clouds)
    assert [s[0]["n_points"] for s in singles] == [20, 21, 63, 64, 62, 127, 126, 2934]
    prm = R.params()
    for xyz, (_, snap) in zip(clouds, batch):
        check_definition(xyz, snap, prm)


# ---- the lane / wavefront threshold ----------------------------------------------------------------------------------------------------
def planted(counts, seed, shift):
    """clusters of the given sizes inside distinct unit cells (every second cell along x), away from the cell faces, in shuffled order"""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(0.2, 0.8, (c, 3)) + np.array([2 * i, 0, 0]) + np.array(shift) for i, c in enumerate(counts)]
    xyz = np.concatenate(parts).astype(np.float32)
    return xyz[rng.permutation(len(xyz))]


def test_the_lane_and_wavefront_threshold(pair):
    sizes = [1, 47, 48, 49, 64, 65, 128, 129]
    other = [60, 3, 200, 48, 49]
    clouds = [planted(sizes, 7, (10, 20, 0)), planted(other, 8, (-30, 5, 2))]
    singles, batch = single_then_batch(pair, clouds)
    assert list(batch[0][1]["v_counts"]) == sizes and list(batch[1][1]["v_counts"]) == other
    assert batch[0][0]["n_voxels"] == 8 and batch[1][0]["n_voxels"] == 5
    # and with the targets the other way round: another first voxel for each
    single_then_batch(pair, clouds[::-1], slots=[11, 12])


# ---- voxel geometry --------------------------------------------------------------------------------------------------------------------
def geometry_clouds():
    rng = np.random.default_rng(40)
    lattice = np.concatenate([rng.integers(-3, 4, (300, 3)).astype(np.float32), _cloud(200, 41, shift=(-3, -3, -3), extent=(6, 6, 6))])
    return [_cloud(800, 42, shift=(-50, -60, -9), extent=(6, 5, 3)),                    # wholly at negative coordinates
            lattice.astype(np.float32),                                                 # points exactly on multiples of the resolution
            _cloud(30, 43, shift=(5.1, 5.1, 5.1), extent=(0.8, 0.8, 0.8)),              # a single voxel
            _cloud(400, 44, extent=(4, 4, 4)),                                          # very different extents in one batch
            _cloud(3000, 45, shift=(100, -40, 0), extent=(60, 60, 5), holes=(17, 300))]


@pytest.mark.parametrize("resolution", [1.0, 0.5, 2.0])
def test_voxel_grids_of_one_batch_do_not_mix(pair, resolution):
    a, _ = pair
    P = a.lisreg.vgicp_default_params(resolution=resolution)
    clouds = geometry_clouds()
    singles, batch = single_then_batch(pair, clouds, P=P)
    assert all(snap["resolution"] == resolution for _, snap in batch)
    assert all((snap["min_b"] < 0).all() for snap in (batch[0][1],))
    if resolution == 1.0:
        assert batch[2][0]["n_voxels"] == 1 and list(batch[2][1]["dims"]) == [1, 1, 1]
    assert len({tuple(b[1]["dims"]) for b in batch}) >= 4
    prm = R.params(resolution=resolution)
    for i in (0, 3):
        check_definition(clouds[i], batch[i][1], prm)


# ---- position independence ---------------------------------------------------------------------------------------------------------------
def test_slots_do_not_depend_on_the_position_in_the_batch(pair):
    clouds = geometry_clouds()
    single_then_batch(pair, clouds, slots=[40, 7, 65535, 0, 300], order=[4, 3, 2, 1, 0])


# ---- failures ------------------------------------------------------------------------------------------------------------------------------
def test_failures_stay_with_their_target(pair):
    a, b = pair
    few = _cloud(40, 11)
    few[19:] = np.nan                                                                  # 19 finite points
    inf = _cloud(300, 12)
    inf[150, 1] = np.inf
    nan_only = np.full((30, 3), np.nan, np.float32)
    huge = _cloud(21, 16)
    huge[0], huge[1] = (0, 0, 0), (500, 500, 500)                                      # 501^3 voxels at resolution 1: more than 2^26
    clouds = [_cloud(500, 10), few, inf, nan_only, huge, _cloud(257, 13, holes=(256,)), _cloud(64, 14)]
    slots = [3, 4, 5, 6, 7, 8, 9]
    bad = (1, 2, 3, 4)
    # slots 4 and 7 hold valid targets before the failed jobs
    for s in (4, 7):
        b.ctx.vgicp_set_target(s, b.dev(_cloud(100, 15)), b.P)
        assert b.ctx.vgicp_get_target(s)["n_points"] == 100
    res = b.ctx.vgicp_set_target_batch([(s, b.dev(x)) for s, x in zip(slots, clouds)], b.P)
    E = b.lisreg.ERR_ARG
    assert [r["status"] for r in res] == [0, E, E, E, E, 0, 0]
    assert b.ctx.last_error() == "vgicp_set_target_batch: job 1: vgicp_set_target: the cloud has fewer finite points than k_correspondences"
    texts = {}
    for i in bad:
        with pytest.raises(a.lisreg.LisregError) as single:
            a.ctx.vgicp_set_target(slots[i], a.dev(clouds[i]), a.P)
        texts[i] = str(single.value)
        src = _source_for(clouds[0])
        for f in (a, b):
            with pytest.raises(f.lisreg.LisregError) as e:
                f.ctx.vgicp_align(slots[i], f.dev(src), f.P)
            assert NO_TARGET in str(e.value) and "vgicp_align" in str(e.value)
            with pytest.raises(f.lisreg.LisregError):
                f.ctx.vgicp_get_target(slots[i])
    assert "fewer finite points than k_correspondences" in texts[1] and "infinite coordinates" in texts[2]
    assert "fewer finite points than k_correspondences" in texts[3] and "more than 2^26 cells (the voxel table is dense" in texts[4]
    for i in (0, 5, 6):
        a.ctx.vgicp_set_target(slots[i], a.dev(clouds[i]), a.P)
        assert same(snapshot(a, slots[i], clouds[i]), snapshot(b, slots[i], clouds[i])), i
    # the first failure named is the first failed JOB, with the single call's text behind the job
    for first, word in ((inf, texts[2]), (huge, texts[4])):
        res = b.ctx.vgicp_set_target_batch([(20, b.dev(first)), (21, b.dev(few))], b.P)
        assert [r["status"] for r in res] == [E] * 2
        tail = word[word.index("vgicp_set_target: "):]
        assert b.ctx.last_error() == "vgicp_set_target_batch: job 0: " + tail


# ---- whole-call refusals -------------------------------------------------------------------------------------------------------------------
def test_whole_call_refusals_touch_nothing(pair):
    a, _ = pair
    L, lisreg = a.lisreg.lib(), a.lisreg
    held = _cloud(300, 21)
    a.ctx.vgicp_set_target(3, a.dev(held), a.P)
    want = snapshot(a, 3, held)
    good = a.dev(_cloud(200, 22))

    def call(jobs, n=None, params=a.P, null_jobs=False):
        arr = (lisreg.VgicpTargetJob * max(len(jobs), 1))()
        for k, (slot, (ptr, cnt)) in enumerate(jobs):
            arr[k].slot, arr[k].cloud, arr[k].n = slot, ptr, cnt
            arr[k].status, arr[k].info.n_points, arr[k].info.dims[0], arr[k].info.n_voxels = 77, 123, 45, 9
        rc = L.lisreg_vgicp_set_target_batch(a.ctx._h, len(jobs) if n is None else n, None if null_jobs else arr,
                                             C.byref(params) if params is not None else None)
        for k in range(len(jobs)):
            assert (arr[k].status, arr[k].info.n_points, arr[k].info.dims[0], arr[k].info.n_voxels) == (77, 123, 45, 9), "a refused call wrote a job field"
        return rc

    ok = (3, good)
    big = lisreg.VGICP_TARGET_BATCH_MAX_POINTS // 2 + 1
    cases = {
        "null jobs": dict(jobs=[ok], null_jobs=True),
        "null params": dict(jobs=[ok], params=None),
        "k outside 4 .. 32": dict(jobs=[ok], params=lisreg.vgicp_default_params(k_correspondences=33)),
        "resolution 0": dict(jobs=[ok], params=lisreg.vgicp_default_params(resolution=0.0)),
        "plane_epsilon 0": dict(jobs=[ok], params=lisreg.vgicp_default_params(plane_epsilon=0.0)),
        "slot -1": dict(jobs=[ok, (-1, good)]),
        "slot 65536": dict(jobs=[ok, (65536, good)]),
        "slot twice": dict(jobs=[ok, (9, good), (3, good)]),
        "n 0": dict(jobs=[ok, (4, (good[0], 0))]),
        "n negative": dict(jobs=[ok, (4, (good[0], -5))]),
        "null cloud": dict(jobs=[ok, (4, (None, 50))]),
        "negative n_targets": dict(jobs=[ok], n=-1),
        "too many targets": dict(jobs=[(s, good) for s in range(lisreg.VGICP_TARGET_BATCH_MAX + 1)]),
        "too many points": dict(jobs=[(3, (good[0], big)), (4, (good[0], big))]),
    }
    bare = {k: v for k, v in want.items() if not k.startswith(("lin", "pairs"))}
    for name, kw in cases.items():
        assert call(**kw) == lisreg.ERR_ARG, name
        assert "vgicp_set_target_batch" in a.ctx.last_error(), name
        assert same(snapshot(a, 3), bare), name
    assert same(snapshot(a, 3, held), want)
    with pytest.raises(lisreg.LisregError):
        a.ctx.vgicp_get_target(4)                                                      # no refused call made a slot
    assert lisreg.VGICP_TARGET_BATCH_MAX == 1024 and lisreg.VGICP_TARGET_BATCH_MAX_POINTS == 1 << 27
    assert call([], n=0) == lisreg.OK and call([], n=0, null_jobs=True) == lisreg.OK
    assert same(snapshot(a, 3, held), want)
    # the read-back hook's own refusals
    info = lisreg.VgicpInfo()
    buf = (C.c_int * 4)()
    assert L.lisreg_vgicp_get_target(a.ctx._h, 3, C.byref(info), None, None, None, None, None, None, buf, None, 0, 4, 0) == lisreg.ERR_ARG
    assert info.n_points == 300 and "capacity_cells" in a.ctx.last_error()
    assert L.lisreg_vgicp_get_target(a.ctx._h, 3, None, None, None, None, None, None, None, None, buf, 0, 0, 1) == lisreg.ERR_ARG
    assert "capacity_table" in a.ctx.last_error()
    assert L.lisreg_vgicp_get_target(a.ctx._h, 3, None, None, None, None, None, None, None, None, None, -1, 0, 0) == lisreg.ERR_ARG


# ---- a batch of one ------------------------------------------------------------------------------------------------------------------------
def test_a_batch_of_one_and_slots_that_held_other_targets(pair):
    a, b = pair
    mid = _cloud(1000, 31, holes=(5,))
    a.ctx.vgicp_set_target(3, a.dev(mid), a.P)
    want = snapshot(a, 3, mid)
    b.ctx.vgicp_set_target(3, b.dev(_cloud(5000, 32, extent=(20, 20, 3))), b.P)        # a larger target in the slot
    b.ctx.vgicp_set_target_batch([(4, b.dev(_cloud(30, 33)))], b.P)                     # a smaller one, set by a batch
    res = b.ctx.vgicp_set_target_batch([(3, b.dev(mid))], b.P)
    assert res[0]["status"] == 0 and same(snapshot(b, 3, mid), want)
    res = b.ctx.vgicp_set_target_batch([(4, b.dev(mid))], b.P)
    assert res[0]["status"] == 0 and same(snapshot(b, 4, mid), want)
    # and a single call over a slot a batch set
    small = _cloud(64, 34)
    b.ctx.vgicp_set_target(4, b.dev(small), b.P)
    a.ctx.vgicp_set_target(4, a.dev(small), a.P)
    assert same(snapshot(b, 4, small), snapshot(a, 4, small))


# ---- the scene -----------------------------------------------------------------------------------------------------------------------------
def test_the_scene_in_four_slots_verifies_like_singly_set_slots(pair):
    a, b = pair
    tgt, src, guess, _ = R.scene()
    tgt = np.asarray(tgt, np.float32)
    assert (~np.isnan(tgt).any(1)).sum() == 25401
    slots = [20, 21, 22, 23]
    rng = np.random.default_rng(7)
    moved, guesses = [], []
    for _ in slots:
        M = R.se3_exp(np.r_[rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.1, 0.1, 3)])
        moved.append(R.transform_points(M, tgt.astype(np.float64)).astype(np.float32))
        g = np.array(guess, np.float32)
        g[:3, 3] += rng.uniform(-0.05, 0.05, 3).astype(np.float32)
        guesses.append(g)
    for s, x in zip(slots, moved):
        a.ctx.vgicp_set_target(s, a.dev(x), a.P)
    res = b.ctx.vgicp_set_target_batch([(s, b.dev(x)) for s, x in zip(slots, moved)], b.P)
    assert all(r["status"] == 0 and r["n_points"] == 25401 for r in res)
    assert {True, False} == set((b.ctx.vgicp_get_voxels(20)["counts"] > 48).tolist())   # the lane and the wavefront form
    for s in slots:
        assert same(snapshot(a, s), snapshot(b, s)), s
    out = []
    for f in (a, b):
        out.append(f.ctx.vgicp_align_batch([f.dev(src)], [f.lisreg.VgicpItem(0, s, g) for s, g in zip(slots, guesses)], f.P))
    (r0, f0, i0), (r1, f1, i1) = out
    assert f0.tobytes() == f1.tobytes() and i0 == i1
    for x, y in zip(r0, r1):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    assert any(r["converged"] for r in r1)


# ---- memory --------------------------------------------------------------------------------------------------------------------------------
def test_twenty_batches_do_not_grow_device_memory(pair):
    _, b = pair
    hip = b.lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    clouds = geometry_clouds()
    jobs = [(3 + i, b.dev(x)) for i, x in enumerate(clouds)]
    b.ctx.vgicp_set_target_batch(jobs, b.P)                                             # every buffer of the call is made
    first = [snapshot(b, s) for s, _ in jobs]
    before = free_bytes()
    for _ in range(20):
        res = b.ctx.vgicp_set_target_batch(jobs, b.P)
    assert free_bytes() == before and all(r["status"] == 0 for r in res)
    assert all(same(snapshot(b, s), f) for (s, _), f in zip(jobs, first))


# ---- counts --------------------------------------------------------------------------------------------------------------------------------
def test_launches_and_synchronisations_do_not_depend_on_the_number_of_targets(pair):
    _, b = pair
    counts = []
    for n in (2, 16):
        jobs = [(3 + i, b.dev(_cloud(300 + 17 * i, 50 + i))) for i in range(n)]
        res = b.ctx.vgicp_set_target_batch(jobs, b.P)
        assert all(r["status"] == 0 for r in res)
        counts.append(b.ctx.vgicp_target_batch_counts())
    print(f"[vgicp_target_batch] (enqueues, synchronisations) for 2 and for 16 targets: {counts}")
    assert counts[0] == counts[1] and counts[0][1] <= 3 and counts[0][0] <= 24


# ---- a caller's busy stream ------------------------------------------------------------------------------------------------------------------
import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


def test_batch_on_a_callers_busy_stream(env):
    """the clouds arrive late on the caller's stream, as in tests/test_caller_stream.py: the slots equal those set on the idle stream,
    and a context left on its own stream reads the decoy"""
    e = env
    P = e.lisreg.vgicp_default_params()
    parts = [_cloud(3000, 61, extent=(10, 10, 2)), _cloud(700, 62, shift=(50, 0, 0), holes=(3, 256)), _cloud(1300, 63, extent=(3, 8, 3))]
    rs = np.concatenate([_rec(p) for p in parts])
    offs = np.r_[0, np.cumsum([len(p) for p in parts])]
    slots = [40, 41, 42]

    def make(dst):
        def run():
            return e.ctx.vgicp_set_target_batch([(s, (dst.ptr + 16 * int(offs[i]), len(parts[i]))) for i, s in enumerate(slots)], P)

        def fetch(res):
            out = {}
            for s, r in zip(slots, res):
                assert r["status"] == 0
                g = e.ctx.vgicp_get_target(s)
                v = e.ctx.vgicp_get_voxels(s)
                out.update({f"{s}_{k}": np.asarray(x) for k, x in g.items()})
                out.update({f"{s}_v_{k}": np.asarray(x) for k, x in v.items()})
            return out
        return run, fetch
    TCS.late_case(e, "vgicp_set_target_batch (device records)", rs, TCS.moved(rs), make)
