"""The structure checks of the k-NN graph rows (search front-end 3) and the cell rows (front-end 5) of a target that is already set
in a context, as functions: tests/test_index_build.py runs them on random submaps (a sample of rows, the rho guarantee against a float64
k-d tree) and on the planted lattice clouds of tests/knn5_ref.py (every row, the rho guarantee by brute force in integers).

exact=True: the target's points, and with them the centres of the rows where the grid's cells are dyadic, are multiples of 1/128 m; all
squared distances are then integers in units of 2^-14 m^2, and "EVERY target point closer than rho is listed" is checked as it is
stated, with no shrink of rho.  Where a centre is no such multiple (a grown cell edge: knn5_ref's `grown`) the distance from it is
formed in float64 from the float32 centre, and rho^2 is shrunk by 2^-20: the device forms that distance in float32 (three products, two
sums: under 2^-22 relative) and cuts its rows by that value."""
import numpy as np

SUB = 128                                    # lattice steps per metre that hold points (1/64 m) and dyadic row centres alike


def _listed_mask(ids, count, n):
    """bool [rows, n]: point j is listed in row r"""
    out = np.zeros((len(ids), n), bool)
    k = ids.shape[1]
    r = np.repeat(np.arange(len(ids)), k)[(np.arange(k)[None, :] < count[:, None]).ravel()]
    out[r, ids[np.arange(k)[None, :] < count[:, None]]] = True
    return out


def _brute_rho(centres32, pts32, ids, count, rho2, k, shell=False):
    """(3) for EVERY row by brute force; shell: a row whose centre has more than k equidistant points has rho no larger than that
    distance.  Returns the number of such rows."""
    P = np.round(pts32.astype(np.float64) * SUB)
    assert np.array_equal(P / SUB, pts32.astype(np.float64))
    Cq = np.round(centres32.astype(np.float64) * SUB)
    lattice = (Cq / SUB == centres32.astype(np.float64)).all(1)
    n, crowded = len(pts32), 0
    step = max(1, 4_000_000 // max(n, 1))
    for s in range(0, len(centres32), step):
        e = slice(s, s + step)
        Di = ((Cq[e, None, :] - P[None, :, :]) ** 2).sum(-1)                      # integers below 2^53: exact in float64
        Df = ((centres32[e, None, :].astype(np.float64) - pts32[None, :, :].astype(np.float64)) ** 2).sum(-1)
        r2 = rho2[e].astype(np.float64)
        closer = np.where(lattice[e, None], Di < r2[:, None] * (SUB * SUB), Df < r2[:, None] * (1.0 - 2.0 ** -20))
        have = _listed_mask(ids[e], count[e], n)
        missing = closer & ~have
        assert not missing.any(), ("closer than rho but not listed", s + np.argwhere(missing)[:4].T[0], np.argwhere(missing)[:4].T[1])
        assert (have.sum(1) == count[e]).all()                                     # each once
        if shell:
            for r in np.flatnonzero(lattice[e]):
                vals, cnt = np.unique(Di[r], return_counts=True)
                for v in vals[cnt > k]:
                    crowded += 1
                    assert r2[r] * (SUB * SUB) <= v, (s + r, r2[r], v / (SUB * SUB))
    return crowded


def check_graph_rows(ctx, slot, kind, sample=4000, exact=False, shell=False):
    """The k-NN graph behind search front-end 3 (lisreg_get_target_graph): for every row, (1) the entries are other points, each once,
    in ascending distance from the row's point (to 2^-16 relative), (2) the coordinates stored in the row are the listed points' own, bit for bit (the
    scan never gathers them), (3) EVERY target point closer than rho is listed — the guarantee the 5-NN certificate rests on —
    checked against a float64 kd-tree on `sample` rows, or (exact) by brute force in integers on every row, (4) padded entries carry the
    point's own coordinates and id -1."""
    from scipy.spatial import cKDTree
    idx = ctx.target_index(slot, kind); g = ctx.target_graph(slot, kind)
    n, k = idx["n"], g["k"]
    pts32 = idx["sorted"][:, :3]; pts = pts32.astype(np.float64)
    assert g["ids"].shape == (n, k) and (g["count"] >= 0).all() and (g["count"] <= k).all()
    col = np.arange(k)[None, :]
    listed = col < g["count"][:, None]
    assert ((g["ids"] >= 0) == listed).all()                                   # a prefix of real entries, then padding
    own = np.broadcast_to(pts32[:, None, :], g["xyz"].shape)
    assert np.array_equal(g["xyz"][~listed], own[~listed])                     # (4)
    safe = np.where(listed, g["ids"], 0)
    assert np.array_equal(g["xyz"][listed], pts32[safe][listed])               # (2)
    assert (g["ids"][listed] != np.broadcast_to(np.arange(n)[:, None], (n, k))[listed]).all()
    d = np.linalg.norm(g["xyz"].astype(np.float64) - pts[:, None, :], axis=2)
    dd = np.where(listed, d, np.inf)
    # (1) ascending up to the key quantisation: since round 5 the graph's rows go through the 32-bit-key sort of the cell rows (the squared
    # distance's float bits with the low 7 bits replaced by the lane), exact to 2^-16 relative — inside the scan's millimetre of slack
    # (as a product, not a ratio: exact duplicates of the row's point stand at distance 0 one after the other)
    assert (dd[:, 1:][listed[:, 1:]] >= dd[:, :-1][listed[:, 1:]] * (1 - 2.0 ** -15)).all()
    # (a listed entry is inside rho up to the key quantisation: keys are compared with their low 7 mantissa bits cleared)
    assert (dd[listed] <= np.sqrt(g["rho2"].astype(np.float64))[:, None].repeat(k, 1)[listed] * (1 + 2.0 ** -15)).all()
    if exact:
        # (the row's own point is not listed: it is taken out of "closer than rho" by listing it for the comparison)
        own_listed = np.concatenate([np.where(listed, g["ids"], -1), np.arange(n)[:, None]], 1)
        order = np.argsort(own_listed < 0, axis=1, kind="stable")                  # real entries first
        packed = np.take_along_axis(own_listed, order, 1)
        return _brute_rho(pts32, pts32, packed, g["count"] + 1, g["rho2"], k, shell)
    tree = cKDTree(pts)
    rng = np.random.default_rng(1)
    for s in rng.choice(n, min(n, sample), replace=False):
        rho = float(np.sqrt(g["rho2"][s]))
        want = set(tree.query_ball_point(pts[s], rho * (1 - 1e-5))) - {int(s)}
        have = set(g["ids"][s][:g["count"][s]].tolist())
        assert len(have) == g["count"][s]                                      # each once
        assert want <= have, (s, rho, sorted(want - have)[:4])                 # (3)
    return 0


def check_cell_rows(ctx, slot, kind, sample=4000, exact=False, shell=False):
    """The cell rows behind search front-end 5 (lisreg_get_target_cell_rows).  Table: -2 only where no target point lies in the 5 x 5 x 5 cell
    block, every other cell has a centre row and one row per octant of its mask, rows laid end to end.  For every row, about its centre
    (cell centre, or octant centre = cell corner + 0.25 / 0.75 of the edge): (1) the entries are target points, each once, ascending in
    distance to 2^-16 relative (the build sorts quantised keys), (2) the stored coordinates are the listed points' own, bit for bit,
    (3) EVERY target point closer than rho is listed — the guarantee the certificate rests on — against a float64 kd-tree on `sample`
    rows, or (exact) by brute force in integers on every row, (4) padded entries carry the centre's coordinates and id -1, (5) an octant with
    a target point inside its box has a row."""
    from scipy.spatial import cKDTree
    g = ctx.target_cell_rows(slot, kind); idx = ctx.target_index(slot, kind)      # (building the rows gives the grid its two-cell margin)
    n, k, R = idx["n"], g["k"], g["n_rows"]
    nx, ny, nz, cell, org = idx["nx"], idx["ny"], idx["nz"], np.float32(idx["cell"]), idx["origin"].astype(np.float32)
    pts32 = idx["sorted"][:, :3]; pts = pts32.astype(np.float64)
    tab = g["table"]
    assert tab.shape == (nx * ny * nz,) and ((tab >= 0) | (tab == -2)).all()      # (-1 only when the buffers are too small: not here)
    # occupancy -> which cells may be -2
    cs = idx["cell_start"]; occ = (np.diff(cs) > 0).reshape(nx, ny, nz)
    from scipy.ndimage import maximum_filter
    near = maximum_filter(occ.astype(np.uint8), size=5, mode="constant", cval=0).astype(bool).reshape(-1)
    assert np.array_equal(tab >= 0, near)
    have = np.flatnonzero(tab >= 0)
    base = tab[have] >> 8; mask = tab[have] & 255
    cnt = 1 + np.array([bin(int(m)).count("1") for m in mask])
    order = np.argsort(base)
    assert base[order][0] == 0 and np.array_equal(base[order][1:], np.cumsum(cnt[order])[:-1]) and base[order][-1] + cnt[order][-1] == R
    # (5): cells that hold a point have the octant that point is in
    pc = np.floor((pts32 - org) / cell).astype(np.int64)
    pc = np.minimum(np.maximum(pc, 0), np.array([nx - 1, ny - 1, nz - 1]))
    frac = (pts32 - org) / cell - pc
    inner = ((frac > 0.01) & (frac < 0.49)) | ((frac > 0.51) & (frac < 0.99))   # clear of the octant faces (float rounding)
    ok = inner.all(1)
    octv = (frac[:, 0] >= 0.5).astype(int) + 2 * (frac[:, 1] >= 0.5) + 4 * (frac[:, 2] >= 0.5)
    cid = (pc[:, 0] * ny + pc[:, 1]) * nz + pc[:, 2]
    assert ((tab[cid[ok]] >> octv[ok]) & 1).all()
    # rows -> centres
    centre = np.zeros((R, 3), np.float32)
    for c_, b_, m_ in zip(have, base, mask):
        iz = c_ % nz; iy = (c_ // nz) % ny; ix = c_ // (nz * ny)
        h = np.array([ix, iy, iz], np.float32)
        centre[b_] = (org.astype(np.float64) + (h.astype(np.float64) + 0.5) * np.float64(cell)).astype(np.float32)
        slot_ = 1
        for o in range(8):
            if (m_ >> o) & 1:
                f = np.array([0.75 if o & 1 else 0.25, 0.75 if o & 2 else 0.25, 0.75 if o & 4 else 0.25], np.float32)
                centre[b_ + slot_] = (org.astype(np.float64) + (h.astype(np.float64) + f.astype(np.float64)) * np.float64(cell)).astype(np.float32)
                slot_ += 1
    col = np.arange(k)[None, :]
    listed = col < g["count"][:, None]
    assert (g["count"] >= 0).all() and (g["count"] <= k).all() and ((g["ids"] >= 0) == listed).all()
    # (4) (the device forms a centre with one fused multiply-add; float64 here, rounded once: the same value up to double rounding)
    assert np.abs(g["xyz"][~listed] - np.broadcast_to(centre[:, None, :], g["xyz"].shape)[~listed]).max(initial=0) <= 4e-6
    safe = np.where(listed, g["ids"], 0)
    assert np.array_equal(g["xyz"][listed], pts32[safe][listed])               # (2)
    d = np.linalg.norm(g["xyz"].astype(np.float64) - centre.astype(np.float64)[:, None, :], axis=2)
    dd = np.where(listed, d, np.inf)
    assert (dd[:, 1:][listed[:, 1:]] >= dd[:, :-1][listed[:, 1:]] * (1 - 2.0 ** -15)).all()      # (1) ascending up to the key quantisation
    if exact:
        return _brute_rho(centre, pts32, g["ids"], g["count"], g["rho2"], k, shell)
    tree = cKDTree(pts)
    rng = np.random.default_rng(2)
    for r in rng.choice(R, min(R, sample), replace=False):
        rho = float(np.sqrt(g["rho2"][r]))
        want = set(tree.query_ball_point(centre[r].astype(np.float64), rho * (1 - 1e-5)))
        got = g["ids"][r][:g["count"][r]].tolist()
        assert len(set(got)) == len(got)                                       # each once
        assert want <= set(got), (r, rho, sorted(want - set(got))[:4])         # (3)
    return 0
