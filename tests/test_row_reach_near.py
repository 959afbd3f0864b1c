"""Option "row_reach" = 2 (the default): of the cells within a metre of a query's initial position ("row_reach" = 1), a run that rebuilds
its targets builds cell rows only for those a query starts in or that have a target point in their 3 x 3 x 3 block (grids with cells of
0.5 m and more; smaller cells keep the rows of 1).  A query in a populated cell left without rows walks: results never change.

The switch is a third value of "row_reach" (tests/test_option_state.py pins the list of option names): 0 all rows, 1 the rows of round 6,
2 the narrower set."""
import functools

import numpy as np
import pytest

OPTS = (("search_mode", 5), ("rebuild_targets_each_run", 1), ("sort_sources", 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# scenes (made once, shared, never written to)

@functools.lru_cache(maxsize=None)
def _room(m_points=60000, n=8, iters=8, off=0.0):
    """the batch of test_round6_edges.test_row_reach_builds_fewer_rows_and_changes_nothing: a 60 k-point submap, 8 scans of 32 x 900"""
    from lisreg import synth
    tc, ts = synth.make_submap(m_points)
    scans = [synth.make_scan(32, 900, 2000 + i) for i in range(n)]
    T0 = np.array([synth.perturb_pose(s["T_true"], np.random.default_rng(9000 + i)) for i, s in enumerate(scans)], np.float32)
    T0[:, 3] += off; T0[:, 4] -= off
    for a in (tc, ts, T0): a.setflags(write=False)
    return tc, ts, [(s["corner"], s["surf"]) for s in scans], T0, iters


@functools.lru_cache(maxsize=None)
def _slab(tall):
    """A floor with two walls and three poles, seen from its own frame by two sources that are samples of it.
    tall = False: 17.3 x 23.2 m, walls of 6 m — nx and ny are no multiples of the classification's 4 x 8 tile, and the walls stand ON the
    grid's edge tiles.  tall = True: 30 x 30 m with walls and poles of 70 m — 145 cells in z: the tile does not fit the LDS and the
    per-cell classification runs.  Point counts keep both grids at 0.5 m cells (footprint density under 31 per square metre)."""
    from lisreg import synth
    rng = np.random.default_rng(5 + tall)
    ex, ey, ez = (30.0, 30.0, 70.0) if tall else (17.3, 23.2, 6.0)
    nf, nw = (9000, 8500) if tall else (5000, 2500)
    floor = np.stack([rng.uniform(0, ex, nf), rng.uniform(0, ey, nf), np.zeros(nf)], 1)
    wall_x = np.stack([np.zeros(nw), rng.uniform(0, ey, nw), rng.uniform(0, ez, nw)], 1)
    wall_y = np.stack([rng.uniform(0, ex, nw), np.full(nw, ey), rng.uniform(0, ez, nw)], 1)
    surf = np.concatenate([floor, wall_x, wall_y]) + rng.normal(0, 0.02, (nf + 2 * nw, 3))
    feet = np.array([[0.3 * ex, 0.4 * ey], [0.7 * ex, 0.2 * ey], [0.5 * ex, 0.8 * ey]])
    k = rng.integers(0, 3, 900)
    corner = np.concatenate([feet[k], rng.uniform(0, ez, (900, 1))], 1) + rng.normal(0, 0.02, (900, 3))
    centre = np.array([0.5 * ex, 0.5 * ey, 1.5])
    scans, T0 = [], []
    for i in range(2):
        T_true = np.array([0, 0, 0, *centre], np.float64)
        sc = corner[rng.random(len(corner)) < 0.5] - centre + rng.normal(0, 0.02, (1, 3))
        ss = surf[rng.random(len(surf)) < 0.4] - centre
        scans.append((synth.to_pcl(sc.astype(np.float32)), synth.to_pcl((ss + rng.normal(0, 0.02, ss.shape)).astype(np.float32))))
        T0.append(synth.perturb_pose(T_true, np.random.default_rng(70 + i)))
    T0 = np.array(T0, np.float32); T0.setflags(write=False)
    return synth.to_pcl(corner.astype(np.float32)), synth.to_pcl(surf.astype(np.float32)), scans, T0, 8


# ---------------------------------------------------------------------------------------------------------------------------------
# the predicate on the host

def _box(a, r):
    """a over the (2 r + 1)^3 block around every cell, clipped at the grid (bool: any, int: sum)"""
    for ax in range(3):
        p = np.pad(a, [(r, r) if d == ax else (0, 0) for d in range(3)])
        parts = [np.take(p, range(s, s + a.shape[ax]), axis=ax) for s in range(2 * r + 1)]
        a = np.logical_or.reduce(parts) if a.dtype == bool else np.sum(parts, axis=0)
    return a


def _marks(sources, mats, origin, cell, dims, band=1e-4):
    """(certain, possible) query marks: k_query_marks' expression in float32 — cell = clamp(floor((M q - origin) * (1 / cell))) —;
    a query within `band` cells of a cell boundary on some axis marks nothing in `certain` and all cells it may fall into in `possible`"""
    f = np.float32
    o, inv, hi = origin.astype(f), f(1) / f(cell), np.array(dims) - 1
    lo_m, hi_m = np.zeros(dims, bool), np.zeros(dims, bool)
    for q, M in zip(sources, mats):
        q, M = q.astype(f), M.astype(f)
        w = np.stack([M[r, 0] * q[:, 0] + M[r, 1] * q[:, 1] + M[r, 2] * q[:, 2] + M[r, 3] for r in range(3)], 1)
        u = (w - o) * inv
        edge = (np.abs(u - np.round(u)) < band).any(1)
        lo_m[tuple(np.clip(np.floor(u[~edge]).astype(np.int64), 0, hi).T)] = True
        for s in range(8):
            d = np.array([(s >> b & 1) * 2 - 1 for b in range(3)]) * 1.01 * band
            hi_m[tuple(np.clip(np.floor(u[edge].astype(np.float64) + d).astype(np.int64), 0, hi).T)] = True
    return lo_m, lo_m | hi_m


def _near_cells(cell):
    return max(1, int(np.ceil(0.5 / cell - 1e-3)))


def _predicate(mode, marks, cnt, cell):
    """cells that get rows under "row_reach" = mode, for (certain, possible) marks: (must, may)"""
    pop5 = _box(cnt, 2) > 0
    if mode == 0:
        return pop5, pop5
    D = min(max(int(np.ceil(1.0 / cell - 1e-3)), 2), 16)
    P = _near_cells(cell)
    assert P <= 2
    out = []
    for m in marks:
        reach = _box(m, D)
        out.append(pop5 & reach if (mode == 1 or P >= 2) else pop5 & (m | (reach & (_box(cnt, 1) > 0))))
    return tuple(out)


def _host_grid(cloud):
    """make_grid's geometry for a cell-row target (two cells of margin), restated: (origin, cell, dims, points per cell)"""
    from lisreg import synth
    f = np.float32
    xyz = synth.pcl_xyz(cloud)
    lo, hi = xyz.min(0), xyz.max(0)
    area = max(1.0, float(hi[0] - lo[0]) * float(hi[1] - lo[1]))
    cell = f(min(0.5, max(0.25, 2.8 / np.sqrt(len(xyz) / area))))
    o, top = lo - f(2) * cell, hi + f(2) * cell
    dims = tuple(int(np.floor((top[d] - o[d]) / cell)) + 1 for d in range(3))
    cnt = np.zeros(dims, np.int64)
    np.add.at(cnt, tuple(np.clip(np.floor((xyz - o) / cell).astype(np.int64), 0, np.array(dims) - 1).T), 1)
    return o, float(cell), dims, cnt


def test_rounding_exemption_of_the_chosen_scene_is_under_one_per_cent():
    """The GPU test below leaves out the cells whose membership turns on queries within 1e-4 cells of a cell boundary; on the room scene
    that must be under 1 % of the marked cells (CPU: the grid geometry restated from make_grid, poses through synth.pose_matrix)."""
    from lisreg import synth
    tc, ts, scans, T0, _ = _room()
    mats = [synth.pose_matrix(T)[:3] for T in T0]
    for k, cloud in enumerate((tc, ts)):
        o, cell, dims, cnt = _host_grid(cloud)
        assert cell == 0.5
        marks = _marks([synth.pcl_xyz(s[k]) for s in scans], mats, o, cell, dims)
        for mode in (1, 2):
            must, may = _predicate(mode, marks, cnt, cell)
            assert not (must & ~may).any()
            print(f"[row_reach {mode}] kind {k}: {int(marks[1].sum())} marked cells, {int(may.sum())} cells with rows, {int((may & ~must).sum())} turn on a rounding")
            assert (may & ~must).sum() * 100 < marks[1].sum()
        assert _predicate(2, marks, cnt, cell)[1].sum() < _predicate(1, marks, cnt, cell)[1].sum()


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU

class _Dev:
    """a scene on the device + a private context"""

    def __init__(self, scene):
        import lisreg
        D = lisreg.DeviceArray
        self.tc, self.ts, self.scans, self.T0, iters = scene
        self.p = lisreg.default_params(1); self.p.fixed_iters = iters
        self.tcd, self.tsd = D(lisreg.pack_device_records(self.tc)), D(lisreg.pack_device_records(self.ts))
        self.recs = [(D(lisreg.pack_device_records(a)), D(lisreg.pack_device_records(b))) for a, b in self.scans]
        self.items = [dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0]) for a, b in self.recs]
        self.n_elems = sum(a.shape[0] + b.shape[0] for a, b in self.recs)
        self.c = lisreg.Context(0)
        for k, v in OPTS:
            self.c.set_option(k, v)

    def run(self, mode, twice=True):
        """set "row_reach", prepare, run (twice: the second run of the prepared batch must equal the first) -> (T, stats, tables)"""
        c = self.c
        c.set_option("row_reach", mode)
        c.set_target_device(self.tcd.ptr, len(self.tc), self.tsd.ptr, len(self.ts))
        c.batch_prepare_device(self.items, self.T0, self.p)
        assert c.get_option("front_end") == 5
        c.batch_run()
        T, st = c.batch_fetch()
        if twice:
            c.batch_run()
            T2, st2 = c.batch_fetch()
            assert np.array_equal(T, T2) and st == st2
        assert c.get_option("row_reach_now") == (1 if mode else 0) and c.get_option("row_reach") == mode
        return T, st, [c.target_cell_rows(0, k) for k in (0, 1)]

    def close(self):
        self.c.close()


def _relations(full, off, on, strictly=(0, 1)):
    """tables of "row_reach" 0 / 1 / 2: -2 is the same set, kept cells keep their masks, every dropped cell is -1, 2's cells are 1's"""
    for k in (0, 1):
        a, b, z = full[k]["table"], off[k]["table"], on[k]["table"]
        assert np.array_equal(a == -2, b == -2) and np.array_equal(a == -2, z == -2)
        for t in (b, z):
            kept = t >= 0
            assert np.all(a[kept] >= 0) and np.array_equal(a[kept] & 255, t[kept] & 255)
            assert np.all(t[(a >= 0) & ~kept] == -1)
        assert np.all(b[z >= 0] >= 0)
        print(f"[row_reach] kind {k}: rows {full[k]['n_rows']} (0) -> {off[k]['n_rows']} (1) -> {on[k]['n_rows']} (2)")
        assert on[k]["n_rows"] <= off[k]["n_rows"] < full[k]["n_rows"]
        if k in strictly:
            assert on[k]["n_rows"] < off[k]["n_rows"]


@pytest.mark.gpu
def test_switch_off_on_off_changes_rows_only():
    """1 / 2 / 1 (and 0): poses and stats equal to the bit, two runs of one prepared batch equal, 1's table restored by switching back;
    with 2 the same -2 set, the same masks on the kept cells, -1 on every dropped one, strictly fewer rows for both kinds."""
    d = _Dev(_room())
    try:
        full = d.run(0)
        off = d.run(1)
        on = d.run(2)
        miss = d.c.get_option("row_reach_misses")
        off2 = d.run(1)
    finally:
        d.close()
    for r in (off, on, off2):
        assert np.array_equal(r[0], full[0]) and r[1] == full[1]
    assert all(np.array_equal(a["table"], b["table"]) and a["n_rows"] == b["n_rows"] for a, b in zip(off[2], off2[2]))
    _relations(full[2], off[2], on[2])
    print(f"[row_reach 2] {miss} query-iterations of {d.n_elems * d.p.fixed_iters} found their cell without rows")
    assert miss * 1000 <= d.n_elems * d.p.fixed_iters             # (under the watchdog's bar: the rows stay narrowed)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_rows_are_the_predicate(mode):
    """The cells with rows, from target_cell_rows, against the predicate recomputed with numpy from the sources, the initial poses and
    the grid's geometry: every cell with rows satisfies it and every cell with a populated 5 x 5 x 5 block that satisfies it has rows —
    but for cells whose membership turns on a query within 1e-4 cells of a cell boundary (at most 1 % of the marked cells).
    mode 1: populated and reached (round 6's rows); mode 2: populated and (marked or (reached and near))."""
    import lisreg
    from lisreg import synth
    d = _Dev(_room())
    try:
        _, _, tabs = d.run(mode, twice=False)
        idx = [d.c.target_index(0, k) for k in (0, 1)]
    finally:
        d.close()
    mats = [np.asarray(lisreg.pose_to_matrix(T), np.float32).reshape(3, 4) for T in d.T0]
    for k in (0, 1):
        g = idx[k]
        dims = (g["nx"], g["ny"], g["nz"])
        assert g["cell"] == 0.5
        cnt = np.diff(g["cell_start"]).astype(np.int64).reshape(dims)
        marks = _marks([synth.pcl_xyz(s[k]) for s in d.scans], mats, g["origin"], g["cell"], dims)
        must, may = _predicate(mode, marks, cnt, g["cell"])
        table = tabs[k]["table"].reshape(dims)
        rows = table >= 0
        assert np.array_equal(table == -2, _box(cnt, 2) == 0)
        print(f"[row_reach {mode}] kind {k}: {int(rows.sum())} cells with rows; predicate {int(must.sum())} certain, {int((may & ~must).sum())} on a rounding; "
              f"{int(marks[1].sum())} marked cells")
        assert (may & ~must).sum() * 100 < marks[1].sum()
        assert not (rows & ~may).any(), np.argwhere(rows & ~may)[:5]
        assert not (must & ~rows).any(), np.argwhere(must & ~rows)[:5]


@pytest.mark.gpu
def test_quarter_metre_cells_keep_their_rows():
    """A 900 k-point submap of the same extent: make_grid gives its surf target 0.25 m cells, where half a metre is two cells — the
    5 x 5 x 5 count itself: tables of 1 and 2 are identical.  (Its 45 k-point corner target keeps 0.5 m cells and is narrowed.)"""
    d = _Dev(_room(m_points=900000, n=4, iters=4))
    try:
        full = d.run(0, twice=False)
        off = d.run(1, twice=False)
        on = d.run(2, twice=False)
        cells = [d.c.target_index(0, k)["cell"] for k in (0, 1)]
    finally:
        d.close()
    assert cells == [0.5, 0.25]
    for r in (off, on):
        assert np.array_equal(r[0], full[0]) and r[1] == full[1]
    assert np.array_equal(off[2][1]["table"], on[2][1]["table"]) and off[2][1]["n_rows"] == on[2][1]["n_rows"]
    _relations(full[2], off[2], on[2], strictly=(0,))


@pytest.mark.gpu
@pytest.mark.parametrize("tall", [False, True])
def test_edge_tiles_and_the_per_cell_classification(tall):
    """The same relations on a grid whose walls stand on its edge tiles (39 x 51 and 19 x 33 columns: no multiples of the 4 x 8 tile), and on a
    target 145 cells tall, which the per-cell classification handles (its tile would not fit the LDS)."""
    d = _Dev(_slab(tall))
    try:
        full = d.run(0)
        off = d.run(1)
        on = d.run(2)
        idx = [d.c.target_index(0, k) for k in (0, 1)]
    finally:
        d.close()
    for g in idx:
        assert g["cell"] == 0.5, g["cell"]
        assert (g["nz"] >= 128) == tall, g["nz"]
        if not tall:
            assert g["nx"] % 4 != 0 and g["ny"] % 8 != 0, (g["nx"], g["ny"])
    for r in (off, on):
        assert np.array_equal(r[0], full[0]) and r[1] == full[1]
    _relations(full[2], off[2], on[2])


@pytest.mark.gpu
def test_watchdog_guards_the_narrower_rows():
    """Initial poses 1.7 m off (test_option_state.test_row_reach_walk_and_back_off): the queries leave the cells with rows and walk —
    the poses of "row_reach" = 0 —, the fetch counts more than one query-iteration in a thousand, and the next run builds all rows."""
    scene = _room(iters=12, off=1.2)
    ref = _Dev(scene)
    try:
        want = ref.run(0, twice=False)
    finally:
        ref.close()
    d = _Dev(scene)
    try:
        c = d.c
        c.set_option("row_reach", 2)
        c.set_target_device(d.tcd.ptr, len(d.tc), d.tsd.ptr, len(d.ts))
        c.batch_prepare_device(d.items, d.T0, d.p)
        c.batch_run()
        first = c.batch_fetch()
        assert c.get_option("row_reach_now") == 1
        miss = c.get_option("row_reach_misses")
        print(f"[row_reach 2] initial poses 1.7 m off: {miss} query-iterations of {d.n_elems * d.p.fixed_iters} found their cell without rows")
        assert miss * 1000 > d.n_elems * d.p.fixed_iters
        c.batch_run()
        again = c.batch_fetch()
        assert c.get_option("row_reach_now") == 0
        tabs = [c.target_cell_rows(0, k) for k in (0, 1)]
    finally:
        d.close()
    for r in (first, again):
        assert np.array_equal(r[0], want[0]) and r[1] == want[1]
    assert all(np.array_equal(a["table"], b["table"]) for a, b in zip(tabs, want[2]))
