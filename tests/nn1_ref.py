"""The exact k = 1 search of csrc/lisreg_nn1.hip, DEFINED in plain numpy, and the planted clouds its tests share.

`nearest` is brute force over all pairs in the arithmetic the kernels use (float32, FLANN's L2_Simple order, no contraction):
the winner is the lexicographic minimum of (d2, original index), found iff d2 <= max_dist * max_dist.  `dynamic_keep` is the
predicate of SubMapManager::map_scan_feature_pts_distance_removal (subMap.h:1076-1087) on top of it.  `grid_geometry` restates
make_grid (csrc/lisreg_api_ctx.hip), so that a test can say on the CPU which path of the walk its inputs take.

Every `*_case()` returns dict(map=float32[n, 3], queries=float32[k, 3], groups=name -> indices it planted); `case(name)` makes each
once per process and `brute(name)` its reference, so the CPU and the GPU tests read one definition.  `case(name, frame)` is the same case
moved into one of the map frames of tests/far_frame.py (None: as planted, around the origin): the float32 sum of every coordinate and
the frame's offset IS the moved cloud; a case that is built from the grid's geometry is rebuilt from the moved map's geometry."""
import numpy as np

f32 = np.float32
FLT_MAX = 3.4028234663852886e38
K_NN1_CAP = 8                      # kNn1Cap of lisreg_nn1.hip: the LDS run list of the flattened walk
CAPS = (1e18, 3.0, 0.5, 0.0)


# ---------------------------------------------------------------- the definition
def _brute_chunk(m, c, ties):
    """one block of queries against the whole map: (idx, d2, count, last) as brute_force returns them"""
    n = len(m)
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = c[:, 0:1] - m[None, :, 0]; d2 *= d2                       # ex * ex
        t = c[:, 1:2] - m[None, :, 1]; t *= t; d2 += t                 # + ey * ey
        t = c[:, 2:3] - m[None, :, 2]; t *= t; d2 += t                 # (...) + ez * ez: float32 throughout, numpy never contracts
    assert d2.dtype == f32
    np.copyto(d2, f32(np.inf), where=np.isnan(d2))                     # a NaN distance (NaN map point, NaN query) never wins
    first = d2.argmin(1)                                               # the FIRST index that attains the minimum
    dmin = d2[np.arange(len(c)), first]
    any_ = np.isfinite(dmin)
    idx = np.where(any_, first, -1).astype(np.int32)
    dmin = np.where(any_, dmin, f32(np.inf)).astype(f32)
    if not ties:
        return idx, dmin, None, None
    eq = (d2 == dmin[:, None]) & any_[:, None]
    last = np.where(any_, n - 1 - eq[:, ::-1].argmax(1), -1).astype(np.int32)
    return idx, dmin, eq.sum(1).astype(np.int32), last


def brute_force(map_xyz, query_xyz, ties=True, pair_budget=1_000_000):
    """(idx int32 [k], d2 float32 [k], count int32 [k], last int32 [k]) of the unbounded search: idx = the LOWEST original index that
    attains the minimum squared distance (-1: no map point with a non-NaN distance), d2 that minimum (+inf with idx -1), count = how
    many map points attain it, last = the HIGHEST index that does (both None with ties=False, which spares two passes).
    All pairs, in blocks of `pair_budget` pairs so that 30 000 x 150 000 stay small in memory; the blocks are independent and go to a
    few threads (numpy releases the interpreter lock inside its loops)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    m = np.ascontiguousarray(map_xyz, f32).reshape(-1, 3)
    q = np.ascontiguousarray(query_xyz, f32).reshape(-1, 3)
    k, n = len(q), len(m)
    idx = np.full(k, -1, np.int32); last = np.full(k, -1, np.int32)
    d2o = np.full(k, np.inf, f32); cnt = np.zeros(k, np.int32)
    if n == 0 or k == 0:
        return (idx, d2o, cnt, last) if ties else (idx, d2o, None, None)
    step = max(1, pair_budget // n)
    starts = list(range(0, k, step))
    workers = max(1, min(8, len(starts), (os.cpu_count() or 1)))
    with ThreadPoolExecutor(workers) as pool:
        for s, r in zip(starts, pool.map(lambda s: _brute_chunk(m, q[s:s + step], ties), starts)):
            idx[s:s + step], d2o[s:s + step] = r[0], r[1]
            if ties:
                cnt[s:s + step], last[s:s + step] = r[2], r[3]
    return (idx, d2o, cnt, last) if ties else (idx, d2o, None, None)


def cap2_of(max_dist):
    """the squared cap as lisreg_nearest forms it: max_dist clipped to 1.8e19, the product in float32"""
    md = f32(min(float(max_dist), 1.8e19))
    return f32(md * md)


def apply_cap(idx, d2, max_dist):
    """(idx, d2) of the search bounded by max_dist from the unbounded one: the winner is the same point, found iff d2 <= cap2"""
    found = (idx >= 0) & (d2 <= cap2_of(max_dist))
    return np.where(found, idx, -1).astype(np.int32), d2.copy()


def nearest(map_xyz, query_xyz, max_dist=1e18):
    """(idx int32, d2 float32): idx = -1 where nothing lies within max_dist (d2 is then of no meaning)"""
    idx, d2, _, _ = brute_force(map_xyz, query_xyz, ties=False)
    return apply_cap(idx, d2, max_dist)


def not_found_d2(max_dist):
    """what lisreg_nearest documents for sqd_out where idx_out is -1: the first float above the squared cap"""
    return np.nextafter(cap2_of(max_dist), f32(np.inf))


def dynamic_keep(map_xyz, q_xyz, center_radius, dmin, dmax, near):
    """bool [k]: the points map_scan_feature_pts_distance_removal keeps (subMap.h:1076-1087), unbounded search; every square is a
    float32 product (+inf for FLT_MAX).  An empty map keeps everything."""
    q = np.ascontiguousarray(q_xyz, f32).reshape(-1, 3)
    if len(np.asarray(map_xyz).reshape(-1, 3)) == 0:
        return np.ones(len(q), bool)
    _, d2, _, _ = brute_force(map_xyz, q, ties=False)
    with np.errstate(over="ignore"):
        cr2, near2 = f32(center_radius) * f32(center_radius), f32(near) * f32(near)
        dmin2, dmax2 = f32(dmin) * f32(dmin), f32(dmax) * f32(dmax)
        r2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
    return (r2 > cr2) | ((d2 > near2) & (d2 < dmin2)) | (d2 > dmax2)


# ---------------------------------------------------------------- make_grid, restated
def grid_geometry(map_xyz):
    """dict(o=float32[3], cell, inv_cell (float32), dims=(nx, ny, nz)) of the map index make_grid lays out for this cloud: cell edge
    0.25 .. 0.5 m from the footprint density, origin at the bounding box's minimum (NaN coordinates ignored one by one), the edge grown
    by 1.26 while the grid would have more than 2^24 cells."""
    m = np.ascontiguousarray(map_xyz, f32).reshape(-1, 3)
    n = len(m)
    lo, hi = np.nanmin(m, 0).astype(f32), np.nanmax(m, 0).astype(f32)
    area = max(1.0, float(f32(hi[0] - lo[0])) * float(f32(hi[1] - lo[1])))
    cell = f32(min(0.5, max(0.25, 2.8 / np.sqrt(n / area))))
    while True:
        dims = [int(np.floor(float(f32(f32(hi[d] - lo[d]) / cell))) + 1) for d in range(3)]
        if dims[0] * dims[1] * dims[2] <= (1 << 24):
            break
        cell = f32(cell * f32(1.26))
    return dict(o=lo, cell=cell, inv_cell=f32(f32(1.0) / cell), dims=tuple(dims))


def cell_coords(xyz, geom, clamp=True):
    """int [k, 3]: floor((v - origin) * inv_cell) in float32, as the build (clamped into the grid) and the walk (not clamped) form it;
    a NaN coordinate gives 0"""
    v = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        c = np.floor((v - geom["o"][None, :]) * geom["inv_cell"])
    c = np.where(np.isnan(c), 0, np.clip(c, -2.0e9, 2.0e9)).astype(np.int64)
    if clamp:
        c = np.minimum(np.maximum(c, 0), np.array(geom["dims"], np.int64)[None, :] - 1)
    return c


def cell_counts(map_xyz, geom):
    """points per occupied cell (the runs of one cell the walks step through)"""
    c = cell_coords(map_xyz, geom)
    nx, ny, nz = geom["dims"]
    return np.unique((c[:, 0] * ny + c[:, 1]) * nz + c[:, 2], return_counts=True)[1]


def columns_in_last_pass(map_xyz, geom, q, d2):
    """A LOWER bound on the non-empty (x, y) columns the flattened walk lists in its last pass for query q whose nearest point lies at
    squared distance d2: the columns strictly closer (in x, y) than sqrt(d2) with a point in the z cells of [qz - sqrt(d2), qz + sqrt(d2)].
    The last pass's own box and bound are no smaller than these (its radius carries 1e-4 relative and 1 mm of slack, and the best
    distance it prunes with never drops below d2)."""
    m = np.ascontiguousarray(map_xyz, f32).reshape(-1, 3)
    nx, ny, nz = geom["dims"]
    occ = np.zeros((nx, ny, nz), bool)
    c = cell_coords(m[~np.isnan(m).any(1)], geom)
    occ[c[:, 0], c[:, 1], c[:, 2]] = True
    r = float(np.sqrt(float(d2)))
    q = np.asarray(q, np.float64)
    lo = cell_coords((q - r).astype(f32), geom)[0]; hi = cell_coords((q + r).astype(f32), geom)[0]
    cell, o = float(geom["cell"]), geom["o"].astype(np.float64)
    ix = np.arange(lo[0], hi[0] + 1); iy = np.arange(lo[1], hi[1] + 1)
    xl, yl = o[0] + ix * cell, o[1] + iy * cell
    dx = np.maximum(np.maximum(xl - q[0], q[0] - (xl + cell)), 0.0)
    dy = np.maximum(np.maximum(yl - q[1], q[1] - (yl + cell)), 0.0)
    near = (dx[:, None] ** 2 + dy[None, :] ** 2) < float(d2) * (1.0 - 1e-6)
    filled = occ[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1].any(2)
    return int((near & filled).sum())


# ---------------------------------------------------------------- planted clouds and query sets
def _xyz_of(cloud):
    return np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(f32)


def scene_case(seed=21, n_map=20000, n_query=4096):
    """A synthetic submap and a scan of the same scene jittered by 0.35 m in x, y (2 % of it lifted 5 .. 40 m above everything), as
    tests/test_mapfilter.py's scenes; the last 16 queries are map points themselves (d2 = 0)."""
    from lisreg import synth
    mc, ms = synth.make_submap(n_map, seed=seed)
    m = np.concatenate([_xyz_of(mc), _xyz_of(ms)])
    sc = synth.make_scan(32, 900, seed + 1)
    q = np.concatenate([_xyz_of(sc["corner"]), _xyz_of(sc["surf"])])
    M = synth.pose_matrix(sc["T_true"])
    w = q.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    rng = np.random.default_rng(seed)
    w[:, :2] += rng.normal(0, 0.35, (len(w), 2))
    far = rng.random(len(w)) < 0.02
    w[far, 2] += rng.uniform(5, 40, int(far.sum()))
    pick = rng.permutation(len(w))[: n_query - 16]
    on = rng.permutation(len(m))[:16]
    queries = np.concatenate([w[pick].astype(f32), m[on]])
    return dict(map=m, queries=queries, groups=dict(far=np.flatnonzero(far[pick]), on_map=np.arange(n_query - 16, n_query)))


def lattice_case(twice=False):
    """The permuted 0.25 m lattice of test_icp's tie test (13 x 13 x 5 points; with `twice` every point is listed a second time, in
    reverse order) plus one outlier 20 m above it, and queries whose nearest neighbour is an exact tie between different points: the cell
    centres (eight points), the face centres of the x-y faces (four) and the midpoints of the x edges (two).  Every coordinate and
    every squared distance is a dyadic number float32 holds exactly."""
    g = np.arange(-6, 7, dtype=f32) * f32(0.25)
    X, Y, Z = np.meshgrid(g, g, g[:5], indexing="ij")
    lat = np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(f32)
    rng = np.random.default_rng(5)
    lat = lat[rng.permutation(len(lat))]
    pts = np.concatenate([lat, lat[::-1]]) if twice else lat
    m = np.concatenate([pts, np.array([[0.25, 0.25, 20.0]], f32)])      # (straight above: the footprint, and so the cell edge, stay the tie test's)
    inner = lat[np.all(lat[:, :2] < 1.4, axis=1)]
    centres = inner[inner[:, 2] < -0.6] + f32(0.125)
    faces = inner + np.array([0.125, 0.125, 0.0], f32)
    edges = lat[lat[:, 0] < 1.4] + np.array([0.125, 0.0, 0.0], f32)
    queries = np.concatenate([centres, faces, edges]).astype(f32)
    queries = queries[rng.permutation(len(queries))]
    mult = 2 if twice else 1
    return dict(map=m, queries=queries, groups=dict(far=np.array([len(m) - 1]), tie_sizes=(8 * mult, 4 * mult, 2 * mult)))


def duplicates_case():
    """Clusters of m identical points for every m in 1 .. 9 (six of each), the clusters at least 1.5 m apart in x, y so that each is a
    run of its own, original indices scattered, one outlier 20 m off; queries at every cluster itself (d2 = 0) and 0.1 m beside it.
    The nearest point of every query is an m-way tie: the cluster's lowest index wins."""
    rng = np.random.default_rng(909)
    sizes = np.repeat(np.arange(1, 10), 6)
    rng.shuffle(sizes)
    gx, gy = np.meshgrid(np.arange(8), np.arange(7), indexing="ij")
    centre = np.stack([gx.ravel()[: len(sizes)] * 1.5, gy.ravel()[: len(sizes)] * 1.5, rng.uniform(0.0, 3.0, len(sizes))], 1)
    centre[:, :2] += rng.uniform(0.0, 0.4, (len(sizes), 2))
    centre = centre.astype(f32)
    owner = np.repeat(np.arange(len(sizes)), sizes)
    pts = np.concatenate([centre[owner], np.array([[31.0, 4.0, 1.0]], f32)])
    owner = np.concatenate([owner, [-1]])
    perm = rng.permutation(len(pts))
    pts, owner = pts[perm], owner[perm]
    members = [np.flatnonzero(owner == c) for c in range(len(sizes))]
    queries = np.concatenate([centre, centre + np.array([0.1, 0.0, 0.0], f32)]).astype(f32)
    return dict(map=pts, queries=queries,
                groups=dict(members=members, sizes=sizes, far=np.flatnonzero(owner == -1), cluster_of_query=np.tile(np.arange(len(sizes)), 2)))


def _around(m, rng, k=96, spread=2.0):
    """queries: map points themselves, points beside them, and a few far off"""
    m = m[~np.isnan(m).any(1)]
    a = m[rng.integers(0, len(m), k // 3)]
    b = m[rng.integers(0, len(m), k // 3)] + rng.normal(0, spread, (k // 3, 3))
    c = m[rng.integers(0, len(m), k - 2 * (k // 3))] + rng.normal(0, 15 * spread, (k - 2 * (k // 3), 3))
    return np.concatenate([a, b, c]).astype(f32)


def degenerate_case(kind):
    """grids with an extent of one cell: 'one' point, 'ident25' identical points (1 x 1 x 1), a 'plane' z = const (nz = 1), a 'line'
    along x (ny = nz = 1), and 'corners': eight clusters at the corners of a 200 x 200 x 250 m box, whose grid at 0.5 m would have
    8e7 cells — make_grid has to grow the cell to stay under 2^24."""
    rng = np.random.default_rng(77)
    if kind == "one":
        m = np.array([[1.5, -2.25, 0.75]], f32)
    elif kind == "ident25":
        m = np.repeat(np.array([[3.5, 9.5, 0.75]], f32), 25, 0)
    elif kind == "plane":
        m = np.c_[rng.uniform(-5, 5, (400, 2)), np.full(400, 1.5)].astype(f32)
    elif kind == "line":
        m = np.c_[rng.uniform(0, 20, 200), np.full(200, 2.0), np.full(200, 1.0)].astype(f32)
    elif kind == "corners":
        cs = np.array([[x, y, z] for x in (0.0, 200.0) for y in (0.0, 200.0) for z in (0.0, 250.0)])
        m = (np.repeat(cs, 20, 0) + rng.uniform(-0.5, 0.5, (160, 3)) * 0.5).astype(f32)
        m = m[rng.permutation(len(m))]
    else:
        raise KeyError(kind)
    q = _around(m, rng)
    if kind == "corners":
        q = np.concatenate([q, np.array([[100.0, 100.0, 125.0], [100.0, 0.0, 0.0], [-40.0, 230.0, 260.0]], f32)])
    return dict(map=m, queries=q, groups={})


def nan_map_case():
    """2 000 random points in a 10 m box with three planted NaN points — NaN x, NaN z, all NaN — each next to a query that would
    otherwise take it (its finite coordinates are the query's)"""
    rng = np.random.default_rng(404)
    m = rng.uniform(0.0, 10.0, (2000, 3)).astype(f32)
    spots = np.array([[2.0, 3.0, 1.0], [7.5, 1.25, 4.0], [5.0, 5.0, 9.5]], f32)
    planted = np.array([17, 801, 1999])
    m[planted] = spots
    m[17, 0] = np.nan; m[801, 2] = np.nan; m[1999] = np.nan
    q = np.concatenate([spots, spots + f32(0.01), _around(m, rng, 61)]).astype(f32)
    return dict(map=m, queries=q, groups=dict(nan=planted, beside=np.arange(6)))


def edges_case(frame=None):
    """On the scene map: queries 1, 30 and 500 m outside the grid on each of its six sides and past a corner, a query exactly on a
    cell face and one on the grid's origin, and NaN queries (NaN x, NaN z, all NaN).  In a frame: the same, from the moved map's grid."""
    m = case("scene", frame)["map"]
    geom = grid_geometry(m)
    lo = geom["o"].astype(np.float64)
    hi = lo + np.array(geom["dims"]) * float(geom["cell"])            # the grid's far faces (up to a cell past the cloud)
    mid = (lo + hi) / 2
    qs = []
    for off in (1.0, 30.0, 500.0):
        for d in range(3):
            a, b = mid.copy(), mid.copy()
            a[d], b[d] = lo[d] - off, hi[d] + off
            qs += [a, b]
        qs.append(hi + off)
    n_out = len(qs)
    o, cell = geom["o"], geom["cell"]
    face = np.array([o[0] + f32(3) * cell, o[1] + f32(2) * cell, o[2] + cell], f32)
    qs += [face.astype(np.float64), o.astype(np.float64)]
    nan = np.nan
    qs += [np.array([nan, mid[1], mid[2]]), np.array([mid[0], mid[1], nan]), np.array([nan, nan, nan])]
    q = np.array(qs).astype(f32)
    return dict(map=m, queries=q, groups=dict(outside=np.arange(n_out), face=np.array([n_out]), origin=np.array([n_out + 1]),
                                              nan=np.arange(n_out + 2, n_out + 5)))


def count_case(k, frame=None):
    """the first k scene queries (k = 1, 63, 64, 65, 257: the last wavefront and workgroup are partial for every lane count)"""
    s = case("scene", frame)
    return dict(map=s["map"], queries=s["queries"][:k], groups={})


def threshold_case():
    """The dynamic filter at its thresholds near = 0.25, dmin = 0.5, dmax = 1.0 m, center_radius = 40 m: isolated map points (8 m and
    more apart, dyadic coordinates) and, for each of three of them, each axis and each threshold, the query at exactly that offset along
    the axis and the floats just below and just above it; a query with x^2 + y^2 == center_radius^2 exactly (24, 32) whose nearest point is
    0.75 m away — dropped if it goes through the search as the strict > says, kept if it did not; its neighbour one float outside the
    radius; a query 5 m from every map point; and a pad of 12 points outside the radius, kept whatever the thresholds.
    Returns map, queries, and groups: exact[name] / below / above -> query indices, on_radius, off_radius, lonely, pad."""
    m = np.array([[0, 0, 0], [16, 0, 0], [0, 24, 0.5], [-32, 8, 1], [8, -32, 0], [24, 32, 0.75], [-16, -16, 2], [32, -8, 0]], f32)
    qs, tag = [], []
    for pi in (0, 1, 3):
        for axis in range(3):
            for name, off in (("near", 0.25), ("dmin", 0.5), ("dmax", 1.0)):
                base = m[pi].copy()
                base[axis] = f32(base[axis] + f32(off))
                for var, to in (("below", -np.inf), ("exact", None), ("above", np.inf)):
                    p = base.copy()
                    if to is not None:
                        p[axis] = np.nextafter(p[axis], f32(to))
                    qs.append(p); tag.append((var, name))
    n_cases = len(qs)
    qs += [np.array([24, 32, 0], f32), np.array([24, np.nextafter(f32(32), f32(np.inf)), 0], f32), np.array([8, 8, 5], f32)]
    pad = [np.array([100 + 3 * i, -7, 1], f32) for i in range(12)]
    q = np.array(qs + pad, f32)
    groups = dict(on_radius=np.array([n_cases]), off_radius=np.array([n_cases + 1]), lonely=np.array([n_cases + 2]),
                  pad=np.arange(n_cases + 3, len(q)), cases=np.arange(n_cases))
    for var in ("below", "exact", "above"):
        groups[var] = {name: np.array([i for i, t in enumerate(tag) if t == (var, name)]) for name in ("near", "dmin", "dmax")}
    return dict(map=m, queries=q, groups=groups)


THRESHOLDS = dict(center_radius=40.0, near=0.25, dmin=0.5, dmax=1.0)

_MAKERS = dict(scene=scene_case, lattice=lattice_case, lattice2=lambda: lattice_case(True), duplicates=duplicates_case,
               one=lambda: degenerate_case("one"), ident25=lambda: degenerate_case("ident25"), plane=lambda: degenerate_case("plane"),
               line=lambda: degenerate_case("line"), corners=lambda: degenerate_case("corners"), nan_map=nan_map_case, edges=edges_case,
               count1=lambda f=None: count_case(1, f), count63=lambda f=None: count_case(63, f), count64=lambda f=None: count_case(64, f),
               count65=lambda f=None: count_case(65, f), count257=lambda f=None: count_case(257, f), thresholds=threshold_case)
_FROM_GEOMETRY = ("edges", "count1", "count63", "count64", "count65", "count257")     # makers that take the frame themselves
CASE_NAMES = tuple(k for k in _MAKERS if k != "thresholds")
_CASES, _BRUTE = {}, {}


def case(name, frame=None):
    """the named case as planted (frame None) or moved into a frame of far_frame.FRAMES"""
    key = (name, frame)
    if key not in _CASES:
        if frame is None:
            _CASES[key] = _MAKERS[name]()
        elif name in _FROM_GEOMETRY:
            _CASES[key] = _MAKERS[name](frame)
        else:
            from far_frame import offset, shift
            c = case(name)
            m, q = c["map"], c["queries"]
            if name == "corners":                 # 200 m wide: hung on the INNER side of a positive offset, so that it stays within range
                back = np.where(offset(frame) > 0, f32(-200.0), f32(0.0)).astype(f32)
                m, q = m + back, q + back
            _CASES[key] = dict(map=shift(m, frame), queries=shift(q, frame), groups=c["groups"])
    return _CASES[key]


def brute(name, frame=None):
    """brute_force of a named case (in a frame: of the moved clouds), computed once and never written to"""
    key = (name, frame)
    if key not in _BRUTE:
        c = case(name, frame)
        if name.startswith("count"):
            k = len(c["queries"])
            _BRUTE[key] = tuple(a[:k] for a in brute("scene", frame))
        else:
            _BRUTE[key] = brute_force(c["map"], c["queries"])
        for a in _BRUTE[key]:
            a.setflags(write=False)
    return _BRUTE[key]
