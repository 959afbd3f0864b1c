"""The exact five-nearest search behind k_assoc_walk (csrc/lisreg_assoc.hip), DEFINED in integer arithmetic, and the planted clouds
its tests share (tests/test_knn5_forms.py, the structure checks of tests/test_index_build.py).

Every target point and every query lies on the dyadic lattice: integer multiples of 1/64 m.  Under a pose of zero angles the device's
q = src + t is exact, and so are dx, dx^2 and the three-term sum of every pair closer than 64 m (each below 2^24 in units of 2^-12
m^2), in any order, contracted or not; larger distances round monotonically and never compete for a place inside tau <= 2.  The
reference is therefore integer arithmetic: d2 = dx^2 + dy^2 + dz^2 in int64, in units of 2^-12 m^2 (tau = 1 is 4096), ranked by
(d2, original index) — what nearestKSearch(5) + the `sqDist[4] < tau` test return with equal distances resolved by index.  Nothing
about the device's arithmetic enters.

`case(name)` -> dict(tgt=(corner, surf) int64 [n, 3] lattice coordinates in their ORIGINAL order (a fixed random permutation: index
is unrelated to position), queries int64 [k, 3] — fed as corner AND as surf sources, each searched in its own target —, t int64 [3]
a lattice translation for the translated legs, groups name -> query indices, taus).  `brute5(name, tau)` -> per kind the reference of
every query, made once per process and never written to.  `grid_geometry` restates make_grid (csrc/lisreg_api_ctx.hip) with the two-cell
margin the cell rows add, so that planted properties that depend on cells can be asserted on the CPU."""
import numpy as np

f32 = np.float32
UNIT = 64                          # lattice steps per metre
INF = np.int64(1) << 62            # d2 of a place that no target point fills
ROW_MARGIN = 2                     # kCrowGridMargin: cells the grid of a target with cell rows reaches past the cloud
GRAPH_K = 64                       # kGraphK: entries of a graph row / cell row
KINDS = ("corner", "surf")


def to_f32(i):
    """lattice coordinates -> float32 metres, exactly"""
    a = np.asarray(i, np.int64).reshape(-1, 3)
    out = (a.astype(np.float64) / UNIT).astype(f32)
    assert np.array_equal(out.astype(np.float64) * UNIT, a.astype(np.float64))
    return out


def tau_units(tau):
    t = float(tau) * UNIT * UNIT
    assert t == int(t)
    return int(t)


# ---------------------------------------------------------------- the definition
def brute5_cloud(tgt, q, tau):
    """dict(idx int32 [k, 5] the five smallest (d2, original index) (-1 where the target has fewer points), d2 int64 [k, 5] (INF there),
    found bool [k] = d2[4] < tau * 4096 (strict), ties5 int [k] = how many target points lie at exactly the fifth distance (0: no fifth),
    n_in int [k] = how many of the five lie inside tau: idx[i, :n_in[i]] is the ascending list of a query with fewer than five)"""
    tgt = np.asarray(tgt, np.int64).reshape(-1, 3); q = np.asarray(q, np.int64).reshape(-1, 3)
    n, k, tu = len(tgt), len(q), tau_units(tau)
    idx = np.full((k, 5), -1, np.int32); d2 = np.full((k, 5), INF, np.int64); ties = np.zeros(k, np.int64)
    if n:
        step = max(1, 2_000_000 // n)
        ar = np.arange(n, dtype=np.int64)
        for s in range(0, k, step):
            c = q[s:s + step]
            D = ((c[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
            key = D * n + ar[None, :]                                  # (d2, index) as one integer: d2 < 2^40, n < 2^15
            m = min(5, n)
            part = np.sort(np.partition(key, m - 1, axis=1)[:, :m], axis=1) if n > m else np.sort(key, axis=1)
            idx[s:s + step, :m] = (part % n).astype(np.int32)
            d2[s:s + step, :m] = part // n
            if n >= 5:
                ties[s:s + step] = (D == d2[s:s + step, 4:5]).sum(1)
    n_in = (d2 < tu).sum(1)
    return dict(idx=idx, d2=d2, found=d2[:, 4] < tu, ties5=ties, n_in=n_in, n=n, tau=float(tau))


def expected_dump(ref):
    """int32 [5, k]: what the neighbour dump holds under canonical ties — the five in (d2, index) order where found; else the points
    inside tau in that order, then -1; nothing at all for a target of fewer than five points (the kernel leaves before it searches)"""
    out = np.where(np.arange(5)[None, :] < ref["n_in"][:, None], ref["idx"], -1).astype(np.int32)
    if ref["n"] < 5:
        out[:] = -1
    return np.ascontiguousarray(out.T)


# ---------------------------------------------------------------- make_grid, restated
def grid_geometry(xyz, margin=ROW_MARGIN):
    """dict(o float32 [3], cell, inv_cell float32, dims) of the grid make_grid lays out for float32 cloud xyz: the cell edge is
    min(0.5, max(0.25, 2.8 / sqrt(n / max(1, xy-area)))) from the cloud's own bounding box, the grid reaches `margin` cells past that box on every
    side, and the edge grows by 1.26 (the margin with it) while the grid would have more than 2^24 cells."""
    m = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    n = len(m)
    if n == 0:
        return dict(o=np.zeros(3, f32), cell=f32(0.5), inv_cell=f32(2.0), dims=(0, 0, 0))
    lo0, hi0 = m.min(0), m.max(0)
    area = max(1.0, float(f32(hi0[0] - lo0[0])) * float(f32(hi0[1] - lo0[1])))
    cell = f32(min(0.5, max(0.25, 2.8 / np.sqrt(n / area))))
    while True:
        lo = (lo0 - f32(margin) * cell).astype(f32); hi = (hi0 + f32(margin) * cell).astype(f32)
        dims = [int(np.floor(float(f32(f32(hi[d] - lo[d]) / cell))) + 1) for d in range(3)]
        if dims[0] * dims[1] * dims[2] <= (1 << 24):
            break
        cell = f32(cell * f32(1.26))
    return dict(o=lo, cell=cell, inv_cell=f32(f32(1.0) / cell), dims=tuple(dims))


def cell_coords(xyz, geom, clamp=True):
    """int64 [k, 3]: floor((v - origin) * inv_cell) in float32, clamped into the grid as the build and the row look-up do"""
    v = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    c = np.floor((v - geom["o"][None, :]) * geom["inv_cell"]).astype(np.int64)
    if clamp:
        c = np.minimum(np.maximum(c, 0), np.array(geom["dims"], np.int64)[None, :] - 1)
    return c


def cells_with_rows(xyz, geom):
    """bool [nx, ny, nz]: a target point lies in the 5 x 5 x 5 block of the cell (every other cell is -2 in the row table)"""
    from scipy.ndimage import maximum_filter
    occ = np.zeros(geom["dims"], np.uint8)
    c = cell_coords(xyz, geom)
    occ[c[:, 0], c[:, 1], c[:, 2]] = 1
    return maximum_filter(occ, size=5, mode="constant", cval=0).astype(bool)


def in_minus2_cell(tgt, q, geom=None):
    """bool [k]: the query lies INSIDE the grid, in a cell without rows (where the kernel may skip the search: lisreg_assoc.hip, `v == -2`)"""
    x = to_f32(tgt)
    geom = geom or grid_geometry(x)
    near = cells_with_rows(x, geom)
    raw = cell_coords(to_f32(q), geom, clamp=False)
    inside = ((raw >= 0) & (raw < np.array(geom["dims"])[None, :])).all(1)
    c = cell_coords(to_f32(q), geom)
    return inside & ~near[c[:, 0], c[:, 1], c[:, 2]]


def minus2_shortcut_applies(geom, tau):
    """the kernel's own condition for trusting a -2 cell: tau <= (2 cell - 2 kEps)^2 in float32"""
    e = f32(f32(2.0) * geom["cell"] - f32(2.0) * f32(1e-3))
    return bool(f32(tau) <= f32(e * e))


# ---------------------------------------------------------------- planted clouds and query sets
def _signed_perms(a, b, c):
    from itertools import permutations, product
    out = set()
    for p in permutations((a, b, c)):
        for s in product((1, -1), repeat=3):
            out.add(tuple(int(v * w) for v, w in zip(p, s)))
    return np.array(sorted(out), np.int64)


SHELL48 = _signed_perms(1, 3, 4)                                        # norm^2 26 in units of 1/64 m
SHELL24 = _signed_perms(0, 1, 5)
SHELL72 = np.concatenate([SHELL48, SHELL24])
SHELL64 = np.concatenate([SHELL48, SHELL24[:16]])


def _finish(corner, surf, queries, groups, seed, t=(96, -160, 32), taus=(1.0,)):
    rng = np.random.default_rng(seed)
    corner = np.asarray(corner, np.int64).reshape(-1, 3); surf = np.asarray(surf, np.int64).reshape(-1, 3)
    corner = corner[rng.permutation(len(corner))]; surf = surf[rng.permutation(len(surf))]
    q = np.asarray(queries, np.int64).reshape(-1, 3)
    assert len(corner) <= 20000 and len(surf) <= 20000 and len(q) <= 4096
    groups = {k: np.asarray(v, np.int64) for k, v in groups.items()}
    return dict(tgt=(corner, surf), queries=q, t=np.array(t, np.int64), groups=groups, taus=tuple(taus))


def _grid3(nx, ny, nz, pitch):
    X, Y, Z = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), Z.ravel()], 1).astype(np.int64) * pitch


def lattice_case():
    """surf: a cubic lattice of pitch 1/8 m, 17 x 17 x 9 points (650 points per m^2 of footprint: 0.25 m cells, whose faces are lattice
    planes); corner: its five lowest layers.  Queries on lattice points (a six-way tie behind the point itself), on face centres
    (4 + 8), edge centres (2 + 8) and body centres (8) — every one ties inside its five AND at the fifth / sixth place —, among them
    grid-cell corners, faces and octant faces; `above`: 63/64 m above the top layer (five inside tau in surf, none in corner);
    `random`: 300 lattice positions in and around the block."""
    surf = _grid3(17, 17, 9, 8)
    corner = surf[surf[:, 2] <= 32]
    base = _grid3(5, 5, 3, 8) + np.array([48, 48, 16])
    offs = dict(on=(0, 0, 0), face_xy=(4, 4, 0), face_xz=(4, 0, 4), face_yz=(0, 4, 4), edge_x=(4, 0, 0), edge_y=(0, 4, 0),
                edge_z=(0, 0, 4), body=(4, 4, 4))
    qs, groups, at = [], {}, 0
    for name, o in offs.items():
        qs.append(base + np.array(o)); groups[name] = np.arange(at, at + len(base)); at += len(base)
    above = np.array([[64, 64, 127], [60, 68, 127], [8, 8, 127], [64, 64, 128], [61, 64, 126]])
    qs.append(above); groups["above"] = np.arange(at, at + len(above)); at += len(above)
    rng = np.random.default_rng(11)
    rnd = np.stack([rng.integers(-100, 230, 300), rng.integers(-100, 230, 300), rng.integers(-100, 170, 300)], 1)
    qs.append(rnd); groups["random"] = np.arange(at, at + 300)
    groups["planted"] = np.arange(0, len(offs) * len(base))
    return _finish(corner, surf, np.concatenate(qs), groups, 101)


def _half_holes(T):
    """in-plane lattice offsets (pitch 32) to REMOVE around a hole centre so that exactly the four axis neighbours stay closer than T"""
    i = np.arange(-3, 4) * 32
    X, Y = np.meshgrid(i, i, indexing="ij")
    p = np.stack([X.ravel(), Y.ravel()], 1)
    r2 = (p ** 2).sum(1)
    return p[(r2 < T) & (r2 != 1024)]


def half_case():
    """surf: the planar lattice of pitch 0.5 m (41 x 41 points at z = 0: 0.5 m cells, every point on a cell corner) with two kinds of
    holes; corner: every second point of it.  4096 = 64^2 and 8192 = 2 * 64^2 are sums of three squares in ONE way each — (64, 0, 0),
    (64, 64, 0) — so a fifth distance of exactly tau needs the fifth point a metre along an axis (a metre along two): around a hole
    centre everything closer than that is removed except the four axis neighbours, and the query AT the centre has four points inside
    tau and a four-way tie at exactly tau: not found.  `at_tau_1` / `at_tau_2`: those queries, for tau = 1 / 2; `beside_*`: one lattice step
    off (the fifth distance drops below tau: found).  `below_tau_1` / `below_tau_2`: queries over the intact lattice whose fifth d2 is
    4094 / 8190 — the largest values below tau that any lattice pair can have (4095 and 8191 are not sums of three squares): found."""
    full = _grid3(41, 41, 1, 32)
    centres1 = np.array([[8, 8], [8, 20], [8, 32]]) * 32
    centres2 = np.array([[24, 8], [24, 20], [24, 32]]) * 32
    gone = set()
    for cs, T in ((centres1, 4096), (centres2, 8192)):
        for c in cs:
            for o in _half_holes(T):
                gone.add((int(c[0] + o[0]), int(c[1] + o[1])))
    keep = np.array([(int(p[0]), int(p[1])) not in gone for p in full])
    surf = full[keep]
    ij = surf[:, :2] // 32
    corner = surf[(ij.sum(1) % 2) == 0]
    z0 = np.zeros((3, 1), np.int64)
    qs = [np.c_[centres1, z0], np.c_[centres2, z0], np.c_[centres1 + [1, 0], z0], np.c_[centres2 + [1, 1], z0]]
    names = ["at_tau_1", "at_tau_2", "beside_1", "beside_2"]
    spots = np.array([[15, 15], [16, 28], [33, 17], [34, 30]]) * 32
    b1 = [(7, 6, 51), (11, 10, 47), (14, 1, 53), (15, 5, 50)]
    b2 = [(7, 3, 82)]
    for name, offs in (("below_tau_1", b1), ("below_tau_2", b2)):
        q = [np.array([s[0] + sx * a, s[1] + sy * b, sz * h]) for s in spots for (a, b, h) in offs for sx, sy, sz in ((1, 1, 1), (-1, 1, -1), (1, -1, 1))]
        qs.append(np.array(q)); names.append(name)
    groups, at = {}, 0
    for name, q in zip(names, qs):
        groups[name] = np.arange(at, at + len(q)); at += len(q)
    return _finish(corner, surf, np.concatenate(qs), groups, 102, taus=(1.0, 2.0))


SHELL_BOX = np.array([512, 512, 128])


def shell_centres():
    """name -> (centre, offsets): 72 points around a cell centre, an octant centre and a target point, 48 and 64 around cell centres.
    The grid (0.5 m cells, origin 1 m below the box's corner at 0) has cell i at [-64 + 32 i, -32 + 32 i) in lattice steps."""
    cc = lambda i, j, k: np.array([-64 + 32 * i + 16, -64 + 32 * j + 16, -64 + 32 * k + 16])
    return dict(cell72=(cc(5, 5, 3), SHELL72), octant72=(cc(12, 5, 3) - 8, SHELL72), point72=(np.array([109, 333, 50]), SHELL72),
                cell48=(cc(12, 12, 3), SHELL48), cell64=(cc(8, 8, 3), SHELL64))


def shell_case():
    """surf: shells of 72, 48 and 64 points at ONE distance (sqrt(26) / 64 m) from a cell centre, an octant centre and a target point,
    metres apart, and the eight corners of an 8 x 8 x 2 m box that fix the grid; corner: every second point of each shell.  A row built
    about such a centre cannot hold all its equals.  Queries at each centre and a few lattice steps from it."""
    steps = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 0], [1, 1, 1], [2, 0, 1], [3, 3, 3], [5, 0, 0], [1, 3, 4], [8, 8, 8], [16, 16, 16], [0, 0, 16]])
    box = np.array([[x, y, z] for x in (0, 512) for y in (0, 512) for z in (0, 128)])
    surf, corner, qs, groups, at = [box], [box], [], {}, 0
    for name, (c, offs) in shell_centres().items():
        pts = c + offs
        if name == "point72":
            pts = np.concatenate([c[None, :], pts])
        surf.append(pts); corner.append(pts[::2])
        qs.append(c + steps); groups[name] = np.arange(at, at + len(steps)); at += len(steps)
    groups["centres"] = np.arange(0, at, len(steps))
    return _finish(np.concatenate(corner), np.concatenate(surf), np.concatenate(qs), groups, 103)


CLUSTER_SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 16, 33, 64, 65, 100, 200)


def clusters_case():
    """surf: exact duplicates in groups of 1 .. 200 on a 0.375 m raster (they see each other), and three groups of exactly 4 and three
    of exactly 5 standing 3 m from everything: on them, 4 is not found and 5 is found at d2 = 0.  corner: the same with one member of
    every group taken away (the 5s become 4s).  The groups of 65, 100 and 200 put more than 64 points into one octant.  Queries on
    every group, one step beside it, between groups, and `empty`: in cells that have no target point within two cells."""
    pos = [np.array([40 + 24 * (k % 4), 40 + 24 * (k // 4), 20 + 3 * k]) for k in range(len(CLUSTER_SIZES))]
    iso = [np.array([400 + 192 * k, 40 + 192 * r, 37]) for r in (0, 1) for k in range(3)]         # row 0: fours, row 1: fives
    iso_sizes = [4, 4, 4, 5, 5, 5]
    surf, corner = [], []
    for p, s in zip(pos + iso, list(CLUSTER_SIZES) + iso_sizes):
        surf.append(np.repeat(p[None, :], s, 0)); corner.append(np.repeat(p[None, :], s - 1, 0))
    on = np.array(pos + iso)
    qs = [on, on + [1, 0, 0], on + [0, 3, -2], np.array(pos) + [12, 0, 0], np.array(iso) + [64, 0, 0], np.array(iso) + [63, 0, 0]]
    names = ["on", "beside", "beside2", "between", "iso_at_tau", "iso_below_tau"]
    empty = np.array([[496, 136, 37], [700, 130, 40], [250, 200, 30], [600, 140, 30]])
    qs.append(empty); names.append("empty")
    groups, at = {}, 0
    for name, q in zip(names, qs):
        groups[name] = np.arange(at, at + len(q)); at += len(q)
    n_pos = len(pos)
    groups["iso4"] = groups["on"][n_pos:n_pos + 3]; groups["iso5"] = groups["on"][n_pos + 3:]
    return _finish(np.concatenate(corner), np.concatenate(surf), np.concatenate(qs), groups, 104)


FEW_POINTS = np.array([[0, 0, 0], [8, 0, 0], [0, 8, 0], [0, 0, 8], [8, 8, 8]])
FEW_SIZES = dict(few05=(0, 5), few14=(1, 4), few45=(4, 5), few51=(5, 1))


def few_case(name):
    """targets of 0, 1, 4 and 5 points, corner and surf of different sizes in the same run (the first points of one set of five within
    0.2 m); queries on them, beside them, and exactly 1 m and 63/64 m from the first along x"""
    nc, ns = FEW_SIZES[name]
    q = np.concatenate([FEW_POINTS, FEW_POINTS + [1, -1, 2], np.array([[-64, 0, 0], [-63, 0, 0], [4, 4, 4], [300, 0, 0], [-56, 0, 0]])])
    return _finish(FEW_POINTS[:nc], FEW_POINTS[:ns], q, dict(all=np.arange(len(q))), 105)


def _around(pts, rng, k=90, near=20, far=300):
    a = pts[rng.integers(0, len(pts), k // 3)]
    b = pts[rng.integers(0, len(pts), k // 3)] + rng.integers(-near, near + 1, (k // 3, 3))
    c = pts[rng.integers(0, len(pts), k // 3)] + rng.integers(-far, far + 1, (k // 3, 3))
    return np.concatenate([a, b, c]), dict(on=np.arange(0, k // 3), near=np.arange(k // 3, 2 * (k // 3)), far=np.arange(2 * (k // 3), 3 * (k // 3)))


def degenerate_case(kind):
    """grids with an extent of one cell before the margin: `one_cell` (40 points inside 0.3 m: dims (1, 1, 1)), `plane` (z constant:
    nz = 1), `line` (y and z constant: ny = nz = 1); corner is the first half of surf"""
    rng = np.random.default_rng(dict(one_cell=31, plane=32, line=33)[kind])
    if kind == "one_cell":
        surf = rng.integers(0, 20, (40, 3))
    elif kind == "plane":
        surf = np.c_[rng.integers(0, 640, (400, 2)), np.full(400, 96)]
    else:
        surf = np.c_[rng.integers(0, 1280, 200), np.full(200, 128), np.full(200, 64)]
    q, groups = _around(surf, rng)
    return _finish(surf[: len(surf) // 2], surf, q, groups, 106)


def outside_case():
    """surf: 1 500 lattice points in an 8 x 8 x 2 m box with its corners planted (0.5 m cells: the grid's outer faces are lattice
    planes, at -1 m and 9.5 / 3.5 m) and five duplicates ON the box's x = 0 face with nothing else within 1.5 m; corner: the first third.
    Queries 1, 30 and 500 m outside the grid on every side and past a corner; in the two-cell margin; exactly on the outer faces and
    on the grid's corners; exactly 1 m (`at_tau`: on the outer face, the five at d2 == tau) and 1 m - 1/64 (`below_tau`) from the
    boundary point."""
    rng = np.random.default_rng(41)
    pts = np.stack([rng.integers(0, 513, 1500), rng.integers(0, 513, 1500), rng.integers(0, 129, 1500)], 1)
    b = np.array([0, 256, 64])
    pts = pts[((pts - b) ** 2).sum(1) > 96 * 96]
    box = np.array([[x, y, z] for x in (0, 512) for y in (0, 512) for z in (0, 128)])
    surf = np.concatenate([pts, box, np.repeat(b[None, :], 5, 0)])
    corner = np.concatenate([pts[: len(pts) // 3], box])
    lo = np.array([-64, -64, -64]); hi = np.array([608, 608, 224])       # the outer faces of the surf grid (asserted by check_planted)
    mid = (lo + hi) // 2
    far = []
    for off in (64, 30 * 64, 500 * 64):
        for d in range(3):
            a, c = mid.copy(), mid.copy()
            a[d], c[d] = lo[d] - off, hi[d] + off
            far += [a, c]
        far.append(hi + off)
    far = np.array(far)
    margin = np.stack([rng.integers(-64, 0, 40), rng.integers(-64, 577, 40), rng.integers(-64, 193, 40)], 1)
    margin[20:, 0] = rng.integers(513, 577, 20)
    faces = np.array([[lo[0], 100, 40], [hi[0], 100, 40], [100, lo[1], 40], [100, hi[1], 40], [100, 100, lo[2]], [100, 100, hi[2]],
                      lo, hi, [lo[0], hi[1], lo[2]], [0, 0, 0], [512, 512, 128]])
    at_tau = np.array([b - [64, 0, 0]]); below = np.array([b - [63, 0, 0], b - [62, 11, 2]])
    qs, groups, at = [], {}, 0
    for name, q in (("far", far), ("margin", margin), ("faces", faces), ("at_tau", at_tau), ("below_tau", below)):
        qs.append(q); groups[name] = np.arange(at, at + len(q)); at += len(q)
    return _finish(corner, surf, np.concatenate(qs), groups, 107)


def grown_case():
    """eight clusters of 20 points at the corners of a 200 x 200 x 250 m box: at 0.5 m the grid would have 8e7 cells, make_grid grows
    the edge to about 1.0002 m — cell faces are no longer lattice planes, and a cell without rows may skip the search (`empty`).
    Queries on the clusters, beside them, a few metres off, in the empty middle and outside."""
    rng = np.random.default_rng(51)
    cs = np.array([[x, y, z] for x in (0, 12800) for y in (0, 12800) for z in (0, 16000)])
    surf = np.repeat(cs, 20, 0) + rng.integers(-16, 17, (160, 3))
    surf = np.concatenate([surf, cs])                                    # (the corners themselves: the box is exact)
    surf = np.clip(surf, 0, [12800, 12800, 16000])
    corner = surf[::2]
    q, groups = _around(surf, rng, k=120, near=40, far=260)
    empty = np.array([[6400, 6400, 8000], [300, 300, 300], [12500, 12600, 15700], [0, 6400, 0], [200, 0, 0], [12800 - 193, 12800, 16000]])
    out = np.array([[-100, -100, -100], [13000, 13000, 16300], [-20000, 0, 0]])
    groups["empty"] = np.arange(len(q), len(q) + len(empty)); groups["out"] = np.arange(len(q) + len(empty), len(q) + len(empty) + len(out))
    return _finish(corner, surf, np.concatenate([q, empty, out]), groups, 108)


def scene_case():
    """a 12 x 12 m window of synth.make_submap(400 000) at the room's +x wall, snapped to 1/64 m (about 80 surf points per m^2 of
    footprint: a cell edge strictly between 0.25 and 0.5 m), and the points of a synth.make_scan taken inside it, moved to the world by
    the scan's own pose on the host and snapped: ties arise on their own, as they would in a quantised map"""
    from lisreg import synth
    tc, ts = synth.make_submap(400000, seed=61)
    win_lo, win_hi = np.array([28.5, -6.0]), np.array([40.5, 6.0])

    def cut(cloud):
        x = synth.pcl_xyz(cloud).astype(np.float64)
        x = x[((x[:, :2] >= win_lo) & (x[:, :2] <= win_hi)).all(1)]
        return np.round(x * UNIT).astype(np.int64)
    corner, surf = cut(tc), cut(ts)
    sc = synth.make_scan(32, 900, 62, T_true=np.array([0.0, 0.0, 0.3, 34.0, 0.5, 1.7]))
    M = synth.pose_matrix(sc["T_true"])
    w = np.concatenate([synth.pcl_xyz(sc["corner"]), synth.pcl_xyz(sc["surf"])]).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    w = w[((w[:, :2] >= win_lo - 1.0) & (w[:, :2] <= win_hi + 1.0)).all(1)]
    rng = np.random.default_rng(63)
    w[:, :2] += rng.normal(0, 0.2, (len(w), 2))
    q = np.round(w * UNIT).astype(np.int64)[:3000]
    return _finish(corner, surf, q, dict(all=np.arange(len(q))), 109)


_MAKERS = dict(lattice=lattice_case, half=half_case, shell=shell_case, clusters=clusters_case,
               few05=lambda: few_case("few05"), few14=lambda: few_case("few14"), few45=lambda: few_case("few45"), few51=lambda: few_case("few51"),
               one_cell=lambda: degenerate_case("one_cell"), plane=lambda: degenerate_case("plane"), line=lambda: degenerate_case("line"),
               outside=outside_case, grown=grown_case, scene=scene_case)
CASE_NAMES = tuple(_MAKERS)
_CASES, _BRUTE = {}, {}


def case(name):
    if name not in _CASES:
        c = _MAKERS[name]()
        for a in (*c["tgt"], c["queries"], c["t"], *c["groups"].values()):
            a.setflags(write=False)
        _CASES[name] = c
    return _CASES[name]


def runs():
    """every (case, tau) the tests go through"""
    return [(n, tau) for n in CASE_NAMES for tau in case(n)["taus"]]


def brute5(name, tau=1.0):
    """(corner reference, surf reference) of brute5_cloud for the named case at tau, computed once and never written to"""
    key = (name, float(tau))
    if key not in _BRUTE:
        c = case(name)
        out = tuple(brute5_cloud(t, c["queries"], tau) for t in c["tgt"])
        for r in out:
            for a in r.values():
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
        _BRUTE[key] = out
    return _BRUTE[key]
