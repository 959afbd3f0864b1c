"""The target search index (uniform grid, records ordered by (cell, original index), cell_start) in both device build forms —
the bucket sort (one global atomic per point) and the slab form (x-slab partition + one workgroup per slab in LDS) — against a
numpy restatement of the ordering, bit for bit.  Covers many targets per launch sequence (own-target batches, BASELINE configs[3]),
empty and tiny targets, a cloud that lives in ONE x-slab (the slab too big for LDS: global slot tables), and clouds with points
outside the grid's clamped range.  This replaces the two pcl::KdTreeFLANN::setInputCloud calls per registration
(/root/reference/src/node/odomEstimationNode.cpp:602-603)."""
import numpy as np
import pytest


def _expected(idx, cloud_xyz):
    """numpy restatement: cell of every point (float32 arithmetic as on the device), stable order by cell then index."""
    o, inv = idx["origin"], np.float32(1.0) / np.float32(idx["cell"])
    dims = (idx["nx"], idx["ny"], idx["nz"])
    c = []
    for a in range(3):
        v = np.floor((cloud_xyz[:, a].astype(np.float32) - o[a]) * inv).astype(np.int64)
        c.append(np.clip(v, 0, dims[a] - 1))
    cell = (c[0] * dims[1] + c[1]) * dims[2] + c[2]
    order = np.lexsort((np.arange(len(cell)), cell))
    cs = np.zeros(idx["n_cells"] + 1, np.int64)
    np.add.at(cs, cell + 1, 1)
    return order, np.cumsum(cs)


def _check(ctx, slot, kind, cloud):
    import lisreg
    idx = ctx.target_index(slot, kind)
    xyz = lisreg.synth.pcl_xyz(cloud)
    assert idx["n"] == len(cloud)
    if len(cloud) == 0:
        return
    order, cs = _expected(idx, xyz)
    assert np.array_equal(idx["cell_start"], cs), "cell_start"
    assert np.array_equal(idx["sorted"][:, 3].view(np.int32), order.astype(np.int32)), "record order (cell, original index)"
    assert np.array_equal(idx["sorted"][:, :3], xyz[order].astype(np.float32))


def _clouds(seed):
    from lisreg import synth
    rng = np.random.default_rng(seed)
    tc, ts = synth.make_submap(30000 + 1000 * seed, 300 + seed)
    wall = np.zeros((40000, 3), np.float32)                     # one x-slab, 40 k points: beyond the LDS capacity of a slab
    wall[:, 0] = 3.0 + rng.uniform(0, 0.2, len(wall)); wall[:, 1] = rng.uniform(-30, 30, len(wall)); wall[:, 2] = rng.uniform(-1, 6, len(wall))
    thick = np.concatenate([rng.uniform(-40, 40, (20000, 3)).astype(np.float32) * np.array([1, 1, 0.1], np.float32), wall[:25000]])
    return tc, ts, synth.to_pcl(wall, np.zeros(len(wall), np.uint16)), synth.to_pcl(thick, np.zeros(len(thick), np.uint16))


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1])
def test_batched_index_build_is_exactly_cell_then_index_order(gpu_ctx, form):
    import lisreg
    from lisreg import synth
    tc, ts, wall, thick = _clouds(1)
    tc2, ts2, _, _ = _clouds(2)
    empty = synth.to_pcl(np.zeros((0, 3), np.float32), np.zeros(0, np.uint16))
    tiny = synth.to_pcl(np.array([[0, 0, 0], [0.1, 0, 0], [5, 5, 1], [5, 5.01, 1], [-3, 2, 0]], np.float32), np.zeros(5, np.uint16))
    targets = [(tc, ts), (tc2, wall), (tiny, thick), (empty, ts2)]
    for s, (a, b) in enumerate(targets):
        gpu_ctx.set_target(a, b, slot=s)
    sc = synth.make_scan(16, 300, 77)
    items = [dict(src_corner=sc["corner"], src_surf=sc["surf"], target=s) for s in range(len(targets))]
    p = lisreg.default_params(1); p.fixed_iters = 2
    gpu_ctx.set_option("index_build", form); gpu_ctx.set_option("rebuild_targets_each_run", 1)
    try:
        gpu_ctx.align_batch(items, np.tile(sc["T_true"].astype(np.float32), (len(targets), 1)), p)
        assert gpu_ctx.get_option("index_build_now") == form
        for s, (a, b) in enumerate(targets):
            _check(gpu_ctx, s, 0, a)
            _check(gpu_ctx, s, 1, b)
    finally:
        gpu_ctx.set_option("index_build", 2); gpu_ctx.set_option("rebuild_targets_each_run", 0)


@pytest.mark.gpu
def test_single_target_build_matches_too(gpu_ctx):
    tc, ts, wall, thick = _clouds(3)
    gpu_ctx.set_target(tc, thick, slot=0)
    _check(gpu_ctx, 0, 0, tc)
    _check(gpu_ctx, 0, 1, thick)


@pytest.mark.gpu
def test_wide_sparse_map_still_takes_the_strip_form(gpu_ctx):
    """A 700 m x 700 m map: its grid has far more (ix, iy-run) strips than the partition histogram holds at the default strip
    length, so the strips are made longer; still the strip form, still exact."""
    import lisreg
    from lisreg import synth
    rng = np.random.default_rng(5)
    xyz = np.concatenate([rng.uniform(-350, 350, (120000, 2)), rng.uniform(-2, 8, (120000, 1))], 1).astype(np.float32)
    big = synth.to_pcl(xyz, np.zeros(len(xyz), np.uint16))
    tc, ts, _, _ = _clouds(4)
    gpu_ctx.set_target(tc, big, slot=0)
    sc = synth.make_scan(16, 300, 78)
    p = lisreg.default_params(1); p.fixed_iters = 1
    gpu_ctx.set_option("index_build", 1); gpu_ctx.set_option("rebuild_targets_each_run", 1)
    try:
        gpu_ctx.align_batch([dict(src_corner=sc["corner"], src_surf=sc["surf"], target=0)], sc["T_true"].astype(np.float32)[None], p)
        assert gpu_ctx.get_option("index_build_now") == 1
        idx = gpu_ctx.target_index(0, 1)
        assert idx["nx"] * idx["ny"] > 8192 * 16                  # the default 2048-cell strips would not have fitted
        _check(gpu_ctx, 0, 1, big)
        _check(gpu_ctx, 0, 0, tc)
    finally:
        gpu_ctx.set_option("index_build", 2); gpu_ctx.set_option("rebuild_targets_each_run", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("m_points,kind", [(60000, 1), (8000, 1), (60000, 0)])
def test_graph_rows_cover_their_radius(gpu_ctx, m_points, kind):
    """The k-NN graph behind search front-end 3 (lisreg_get_target_graph): for every row, (1) the entries are other points, each once,
    in ascending distance from the row's point (to 2^-16 relative), (2) the coordinates stored in the row are the listed points' own, bit for bit (the
    scan never gathers them), (3) EVERY target point closer than rho is listed — the guarantee the 5-NN certificate rests on —
    checked against a float64 kd-tree, (4) padded entries carry the point's own coordinates and id -1."""
    from lisreg import synth
    from row_checks import check_graph_rows
    tc, ts = synth.make_submap(m_points, 77)
    gpu_ctx.set_target(tc, ts)
    check_graph_rows(gpu_ctx, 0, kind, sample=4000)


@pytest.mark.gpu
@pytest.mark.parametrize("m_points,kind", [(60000, 1), (8000, 1), (60000, 0), (400000, 1)])
def test_cell_rows_cover_their_radius(gpu_ctx, m_points, kind):
    """The cell rows behind search front-end 5 (lisreg_get_target_cell_rows).  Table: -2 only where no target point lies in the 5 x 5 x 5 cell
    block, every other cell has a centre row and one row per octant of its mask, rows laid end to end.  For every row, about its centre
    (cell centre, or octant centre = cell corner + 0.25 / 0.75 of the edge): (1) the entries are target points, each once, ascending in
    distance to 2^-16 relative (the build sorts quantised keys), (2) the stored coordinates are the listed points' own, bit for bit,
    (3) EVERY target point closer than rho is listed — the guarantee the certificate rests on — against a float64 kd-tree, (4) padded
    entries carry the centre's coordinates and id -1, (5) an octant with a target point inside its box has a row."""
    from lisreg import synth
    from row_checks import check_cell_rows
    tc, ts = synth.make_submap(m_points, 78)
    gpu_ctx.set_target(tc, ts)
    check_cell_rows(gpu_ctx, 0, kind, sample=4000)


PLANTED = ("lattice", "shell", "clusters", "grown")


def _set_planted(gpu_ctx, name):
    import knn5_ref as R
    from lisreg import synth
    c = R.case(name)
    gpu_ctx.set_target(synth.to_pcl(R.to_f32(c["tgt"][0])), synth.to_pcl(R.to_f32(c["tgt"][1])))
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", PLANTED)
def test_graph_rows_cover_their_radius_on_planted_clouds(gpu_ctx, name, kind):
    """The same checks on the lattice clouds of tests/knn5_ref.py — whole rows of candidates at ONE distance, where the key quantisation
    of the row sort meets rho — on EVERY row, the rho guarantee by brute force in integers (tests/row_checks.py).  `shell`: the row of a
    point with more than k equidistant neighbours has rho no larger than their distance."""
    from row_checks import check_graph_rows
    _set_planted(gpu_ctx, name)
    crowded = check_graph_rows(gpu_ctx, 0, kind, exact=True, shell=name == "shell")
    assert name != "shell" or kind == 0 or crowded >= 1          # (surf: the centre point of the 72-shell; corner shells are halves)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("name", PLANTED)
def test_cell_rows_cover_their_radius_on_planted_clouds(gpu_ctx, name, kind):
    """The cell rows of the planted clouds, every row; the grid is the one knn5_ref.grid_geometry restates (two-cell margin, grown cell).
    `shell`: a row about a cell or octant centre with 72 points at one distance has rho no larger than that distance."""
    import knn5_ref as R
    from row_checks import check_cell_rows
    c = _set_planted(gpu_ctx, name)
    crowded = check_cell_rows(gpu_ctx, 0, kind, exact=True, shell=name == "shell")
    idx, want = gpu_ctx.target_index(0, kind), R.grid_geometry(R.to_f32(c["tgt"][kind]))
    assert (idx["nx"], idx["ny"], idx["nz"]) == want["dims"] and np.float32(idx["cell"]) == want["cell"], (idx["cell"], want)
    assert np.array_equal(idx["origin"].astype(np.float32), want["o"])
    assert name != "shell" or kind == 0 or crowded >= 2          # (surf: the cell-centre row and the octant-centre row of the 72-shells)
