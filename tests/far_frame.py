"""Map frames kilometres from the origin, for the kernels whose answer has an exact definition at any offset.

Every grid the library builds is laid out from a float32 origin, and the float32 searches prove exactness with an absolute slack of one
millimetre that has to absorb roundings at ulp(|coordinate|): 2^-11 m = 0.49 mm in [4096, 8192) m.  The frames below are applied as
float32 offsets to clouds that were planted around the origin; the rounded sum IS the input of every test, on the CPU and on the GPU.
`edge` keeps every coordinate of a <= 90 m scene under 8192 m, the documented range (include/lisreg.h); mixed signs, because
floorf of negative arguments is the other classic failure.  The 1/64 m lattices of the planted clouds move exactly (2^-6 >> 2^-11), so
planted exact ties stay exact ties.

`face_plants` builds the adversarial k = 1 cases of a frame: a query whose nearest point (the winner) sits on the near face of ANOTHER
(x, y) column of the grid, to the float, with a decoy in the query's own column that is farther by less than the search's millimetre."""
import numpy as np

f32 = np.float32
FRAMES = dict(origin=(0.0, 0.0, 0.0), km=(1000.0, -2000.0, 30.0), edge=(8000.0, -8000.0, -200.0))
FRAME_NAMES = tuple(FRAMES)
COORD_LIMIT = 8192.0              # |coordinate| below this: the supported range of the float32 searches


def offset(frame):
    return np.array(FRAMES[frame], f32)


def shift(cloud, frame):
    """the cloud moved into the frame: float32(coordinate + offset).  xyz arrays [n, 3] (or [n, >= 3]: further columns, e.g. a device
    record's payload, are kept), and structured clouds with x, y, z fields (PCL structs, records): every other field is kept."""
    o = offset(frame)
    a = np.asarray(cloud)
    if a.dtype.names:
        out = a.copy()
        for k, f in enumerate(("x", "y", "z")):
            out[f] = (a[f].astype(f32) + o[k]).astype(f32)
        return out
    out = np.array(a, f32, copy=True)
    out[..., :3] = out[..., :3] + o
    assert out.dtype == f32
    return out


def in_range(*clouds):
    """every finite coordinate of these xyz arrays / clouds lies inside the supported range"""
    for c in clouds:
        a = np.asarray(c)
        xyz = np.stack([a["x"], a["y"], a["z"]], 1) if a.dtype.names else a.reshape(-1, a.shape[-1])[:, :3]
        if xyz.size and not np.nanmax(np.abs(np.where(np.isfinite(xyz), xyz, 0.0))) < COORD_LIMIT:
            return False
    return True


def shift_pose(T, frame):
    """pose [roll, pitch, yaw, x, y, z] with the frame's offset added to the translation in float32 (a key frame's pose in the map)"""
    T = np.array(T, f32, copy=True)
    T[3:6] = T[3:6] + offset(frame)
    return T


def translation_pose(t_init, frame):
    """The pure-translation pose of the 5-NN tests: zero angles, translation float32(t_init + offset).  With zero angles the pose matrix
    is exactly the identity, so M[0]*x + M[1]*y + M[2]*z + M[3] is ONE rounding of x + tx whether or not the compiler contracts it:
    the query the device searches at is float32(src + t), known to the bit."""
    T = np.zeros(6, f32)
    T[3:6] = np.asarray(t_init, f32)[-3:] + offset(frame)
    return T


def rotate_on_host(cloud, T):
    """the cloud under the ROTATION of pose T (float64 on the host, rounded once): what is handed in with translation_pose"""
    from lisreg import synth
    R = synth.pose_matrix(np.asarray(T, np.float64))[:3, :3]
    out = cloud.copy()
    w = synth.pcl_xyz(cloud).astype(np.float64) @ R.T
    out["x"], out["y"], out["z"] = w[:, 0].astype(f32), w[:, 1].astype(f32), w[:, 2].astype(f32)
    return out


# ---------------------------------------------------------------- the five nearest, float32 brute force
def knn5_brute(tgt_xyz, q_xyz, block=512):
    """(idx int32 [n, 6], d2 float32 [n, 6]): the six nearest target points of every query by float32 squared distance in
    flann::L2_Simple order ((ex*ex + ey*ey) + ez*ez, no contraction), ties by the lower index.  All pairs, in blocks."""
    m = np.ascontiguousarray(tgt_xyz, f32)
    q = np.ascontiguousarray(q_xyz, f32)
    k = min(6, len(m))
    idx = np.zeros((len(q), k), np.int32); d2o = np.zeros((len(q), k), f32)
    for s in range(0, len(q), block):
        c = q[s:s + block]
        d2 = c[:, 0:1] - m[None, :, 0]; d2 *= d2
        t = c[:, 1:2] - m[None, :, 1]; t *= t; d2 += t
        t = c[:, 2:3] - m[None, :, 2]; t *= t; d2 += t
        assert d2.dtype == f32
        part = np.argpartition(d2, k - 1, axis=1)[:, :k] if len(m) > k else np.tile(np.arange(len(m)), (len(c), 1))
        # (a tie between the k-th and the next candidate is cut arbitrarily; the census of the tests counts exact ties among the k)
        pd = np.take_along_axis(d2, part, 1)
        order = np.lexsort((part, pd), axis=1)[:, :k]
        idx[s:s + block] = np.take_along_axis(part, order, 1)
        d2o[s:s + block] = np.take_along_axis(pd, order, 1)
    return idx, d2o


# ---------------------------------------------------------------- face plants
N_D = 19                          # distances per (axis, side, t): 2 * 2 * 3 * 19 = 228 cases per frame
SITE = 9.0                        # spacing of the sites: another case's points stay farther from a query than its own 3 m


def face_plants(map_xyz, frame, site=SITE):
    """Adversarial k = 1 cases on the grid of a map in a frame.  `map_xyz` is the map as planted (around the origin); the result's map
    is that map moved into the frame PLUS the planted points, hung on a lattice of sites above it (and one roof point that fixes the
    bounding box), so the grid's origin, cell edge and footprint are the moved map's.

    For every axis (x, y), side and t = 0, 1, 2: the winner is the t-th float, counted from two floats on the query's side of the face
    F = o + i * cell (in float32, product and sum rounded one by one; see below), that the build's arithmetic assigns to the column across the face from the
    query — seen from below the first floats of the upper column, seen from above the last floats of the lower one, which may include
    F itself or end a few floats short of it (v - o is rounded before the floor) — and the query lies D away straight across that face, in the middle of its cell on the other axis.  The decoy is the query's own column's point, D + four float steps of z above or below the query.

    dict(map, queries, winner, decoy (indices into map), D, geom, n_base)"""
    import nn1_ref as R
    base = shift(map_xyz, frame)
    finite = base[~np.isnan(base).any(1)]
    lo, hi = finite.min(0).astype(np.float64), finite.max(0).astype(np.float64)
    combos = [(axis, side, t) for axis in (0, 1) for side in (+1, -1) for t in (0, 1, 2)]
    n_cases = len(combos) * N_D
    per = [max(1, int((hi[d] - lo[d] - 2 * site) // site) + 1) for d in (0, 1)]
    layers = -(-n_cases // (per[0] * per[1]))
    z0 = hi[2] + site
    roof = np.array([[lo[0], lo[1], z0 + layers * site]])
    sites = np.array([[lo[0] + site + ix * site, lo[1] + site + iy * site, z0 + iz * site]
                      for iz in range(layers) for ix in range(per[0]) for iy in range(per[1])])[:n_cases]
    # the geometry depends on the planted points only through their NUMBER and the roof: fix it with stand-ins at the sites
    standin = np.concatenate([base, np.repeat(sites, 2, 0).astype(f32), roof.astype(f32)])
    geom = R.grid_geometry(standin)
    o, cell = geom["o"], geom["cell"]
    Ds = np.geomspace(0.1, 3.0, N_D)
    planted, queries, Dout = [], [], []
    for k, site in enumerate(sites):
        axis, side, t = combos[k % len(combos)]
        D = float(Ds[k // len(combos)])
        other = 1 - axis
        i = int(np.floor((site[axis] - float(o[axis])) / float(cell)))
        # g.ox + (float)ix * g.cell with BOTH roundings.  The device may contract it into one fused multiply-add, so on a grid whose
        # cell edge is no dyadic number its face can lie one float from this one.  Nothing rests on the difference: the winner is chosen
        # by the build's cell assignment below, and the census only asks that it lie within two floats of this face
        face = f32(o[axis] + f32(f32(i) * cell))
        if face == 0:                                                    # (the floats next to zero are denormals: take the next face)
            i += 1
            face = f32(o[axis] + f32(f32(i) * cell))
        # the first floats that the build's own arithmetic (cell_coords) puts in the column ACROSS the face from the query: the rounded
        # face and floor((v - o) * inv_cell) need not agree on which float is the first of column i
        step, across, v = (f32(np.inf) if side > 0 else f32(-np.inf)), [], np.nextafter(face, f32(-np.inf) if side > 0 else f32(np.inf))
        v = np.nextafter(v, -step)                                       # start two floats on the query's side of F
        while len(across) < 3:
            c = int(np.floor(f32(f32(v - o[axis]) * geom["inv_cell"])))
            if (c == i if side > 0 else c == i - 1):
                across.append(v)                                         # nearest to the query first
            v = np.nextafter(v, step)
        close = [v for v in across if abs(float(v) - float(face)) <= 2.0 * float(np.spacing(np.abs(face)))] or across[:1]
        w_ax = close[min(t, len(close) - 1)]
        j = int(np.floor((site[other] - float(o[other])) / float(cell)))
        mid = f32(float(o[other]) + (j + 0.5) * float(cell))
        w = np.zeros(3, f32); w[axis] = w_ax; w[other] = mid; w[2] = f32(site[2])
        q = w.copy(); q[axis] = f32(float(w_ax) - side * D)               # from below (side +1): the query is under the face
        d_real = abs(float(q[axis]) - float(w_ax))
        # the decoy: straight above or below the query, farther than the winner by four float steps of z (finer than those of x, y in
        # the far frames) — a column test that over-estimates the winner's column by more than that loses the winner to it
        gap = 4.0 * float(np.spacing(f32(abs(float(q[2])) + d_real)))
        dec = q.copy(); dec[2] = f32(float(q[2]) + (1 if k % 2 else -1) * (d_real + gap))
        planted += [w, dec]; queries.append(q); Dout.append(d_real)
    m = np.concatenate([base, np.array(planted, f32), roof.astype(f32)])
    n_base = len(base)
    winner = n_base + 2 * np.arange(n_cases)
    return dict(map=m, queries=np.array(queries, f32), winner=winner.astype(np.int32), decoy=(winner + 1).astype(np.int32),
                D=np.array(Dout), geom=geom, n_base=n_base, combos=[combos[k % len(combos)] for k in range(n_cases)])


def dense_patch(n=30000, side=30.0, seed=808):
    """a map dense enough for a cell edge inside (0.25, 0.5) m — no dyadic number, so the faces o + i * cell round — uniform in a
    side x side x 3 m slab"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, (n, 3)) * np.array([side, side, 3.0]) - np.array([side / 2, side / 2, 0.0])).astype(f32)


def check_face_plants(fp):
    """the census of face_plants, from nn1_ref alone: the geometry is the final map's; winner and query lie in different columns, the
    winner within two ulp of the face between them; brute force answers the winner, and without the winner the decoy, whose float32
    d2 exceeds the winner's by less than D^2 - (D - 1 mm)^2 — so a search that skipped the winner's column answers the decoy."""
    import nn1_ref as R
    m, q, geom = fp["map"], fp["queries"], fp["geom"]
    got = R.grid_geometry(m)
    assert np.array_equal(got["o"], geom["o"]) and got["cell"] == geom["cell"] and got["dims"] == geom["dims"], (got, geom)
    assert len(q) >= 200 and in_range(m, q)
    assert fp["D"].min() < 0.11 and fp["D"].max() > 2.9 and (fp["D"] < 0.5).sum() > 40 and (fp["D"] > 0.5).sum() > 40
    cq, cw, cd = R.cell_coords(q, geom, clamp=False), R.cell_coords(m[fp["winner"]], geom, clamp=False), R.cell_coords(m[fp["decoy"]], geom, clamp=False)
    dims = np.array(geom["dims"])
    assert np.all((cq >= 0) & (cq < dims)) and np.all((cw >= 0) & (cw < dims)) and np.all((cd >= 0) & (cd < dims))
    assert np.all((cq[:, :2] != cw[:, :2]).sum(1) == 1)                   # another column, across ONE face
    assert np.array_equal(cq[:, :2], cd[:, :2])                           # the decoy shares the query's column
    o, cell = geom["o"], geom["cell"]
    for k, (axis, side, t) in enumerate(fp["combos"]):
        w = m[fp["winner"][k]]
        i = cw[k, axis] if side > 0 else cw[k, axis] + 1                  # the face towards the query
        face = f32(o[axis] + f32(f32(i) * cell))
        # within 2 ulp of the face, or the very first float of its column (near the origin v - o, which the build rounds before its
        # floor, is coarser than the floats of v: the first float across can lie farther than two of them)
        towards = np.nextafter(w[axis], f32(-np.inf) if side > 0 else f32(np.inf))
        first = int(np.floor(f32(f32(towards - o[axis]) * geom["inv_cell"]))) != cw[k, axis]
        assert abs(float(w[axis]) - float(face)) <= 2.0 * float(np.spacing(np.abs(face))) or first, (k, axis, side, t, w[axis], face)
        assert (cq[k, axis] < cw[k, axis]) == (side > 0)
    idx, d2, cnt, _ = R.brute_force(m, q)
    assert np.array_equal(idx, fp["winner"]) and np.all(cnt == 1)
    without = m.copy(); without[fp["winner"]] = np.nan
    idx2, d22, _, _ = R.brute_force(without, q, ties=False)
    assert np.array_equal(idx2, fp["decoy"])
    D = np.sqrt(d2.astype(np.float64))
    assert np.all(d22 > d2) and np.all(d22.astype(np.float64) - d2.astype(np.float64) < D * D - (D - 1e-3) ** 2)
    return idx, d2


def face_overhang(geom):
    """How far the build's cell assignment and the walk's recomputed faces disagree on this grid, over every inner x and y face:
    (n_faces, overhang in metres) — the largest distance by which a float that floor((v - o) * inv_cell) puts into column i lies BELOW
    the lower face o + i * cell the walk forms for that column, or one of column i - 1 lies ABOVE its upper face (o + (i - 1) * cell) +
    cell; 0 where no float does.  Both forms of the face are taken: product and sum rounded one by one, and fused into one rounding
    (float64 holds the product of two float32 exactly).  This is what the searches' millimetre has to cover."""
    o, cell, inv = geom["o"], geom["cell"], geom["inv_cell"]
    worst, n = 0.0, 0
    for axis in (0, 1):
        i = np.arange(1, geom["dims"][axis], dtype=np.int64)
        n += len(i)
        lowers = [(o[axis] + (i.astype(f32) * cell).astype(f32)).astype(f32),
                  (np.float64(o[axis]) + i.astype(np.float64) * np.float64(cell)).astype(f32)]
        prevs = [(o[axis] + ((i - 1).astype(f32) * cell).astype(f32)).astype(f32),
                 (np.float64(o[axis]) + (i - 1).astype(np.float64) * np.float64(cell)).astype(f32)]
        for xl, xp in zip(lowers, prevs):
            up = (xp + cell).astype(f32)
            v = xl.copy()
            for _ in range(8):
                v = np.nextafter(v, f32(-np.inf))
            for _ in range(17):                                           # the floats F - 8 .. F + 8
                col = np.floor(((v - o[axis]).astype(f32) * inv).astype(f32)).astype(np.int64)
                below = (col == i) & (v < xl)
                above = (col == i - 1) & (v > up)
                if below.any():
                    worst = max(worst, float((xl.astype(np.float64) - v)[below].max()))
                if above.any():
                    worst = max(worst, float((v.astype(np.float64) - up)[above].max()))
                v = np.nextafter(v, f32(np.inf))
    return n, worst
