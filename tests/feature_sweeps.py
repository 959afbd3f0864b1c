"""Structured LiDAR sweeps for the feature-extraction tests, and a census of the events they are built to produce.

`structured_sweep` builds a PointXYZIRT sweep whose float32 ranges sit EXACTLY on a 1/64 m lattice, the way a real sensor reports
them: flat arcs, ramps, small periodic patterns, steps around the 0.3 m occlusion bound, saw-teeth and zig-zags whose peaks share one
curvature, dropped column runs, short and empty rings.  Every point sits on the azimuth of its column's centre (the column formula of
laserProcessing.cpp:489-494 inverted) and its z is nudged ulp by ulp until sqrtf(x*x + y*y + z*z) equals the target bit for bit; the
ring comes from the record's ring field, so z is free.

`census` restates projection, smoothness, occlusion marks and the greedy selection (laserProcessing.cpp:467-713) with numpy float32 and
left-to-right sums, and COUNTS what happens on the way: curvature ties, suppression runs cut at column gaps, occlusion marks and
rejections, sectors that hit the 20-corner cap, skipped sectors, short rings.  It calls neither the oracle nor the library; the tests use
it to prove that an input really contains the events a test is there for.  numpy only."""
import numpy as np

LATTICE = 64                      # ranges are multiples of 1/64 m
f32 = np.float32

XYZIRT = np.dtype({"names": ["x", "y", "z", "intensity", "ring", "time"], "formats": ["<f4", "<f4", "<f4", "<f4", "<u2", "<f4"],
                   "offsets": [0, 4, 8, 16, 20, 24], "itemsize": 32})


# ------------------------------------------------------------------------------------------------------------ generator
def column_azimuth_deg(col, w):
    """horizonAngle (degrees) of the centre of column `col`: the inverse of
        columnIdn = -round((horizonAngle - 90.0) / ang_res_x) + Horizon_SCAN / 2;  if (columnIdn >= Horizon_SCAN) columnIdn -= Horizon_SCAN
    (laserProcessing.cpp:493-495) on the range of atan2, (-180, 180]."""
    res = float(f32(360.0 / float(f32(w))))
    ha = 90.0 + (w // 2 - np.asarray(col, np.float64)) * res
    return np.where(ha > 180.0, ha - 360.0, ha)


def _range32(x, y, z):
    return np.sqrt(x * x + y * y + z * z)           # float32 arrays: every product and sum rounds to float32, left to right


def exact_points(col, ring_el_deg, target, w):
    """x, y, z (float32) on the azimuth of column `col`, elevation about ring_el_deg, with float32 range == target bit for bit.
    The float32 range is a monotone staircase in z that visits every float (z * z is finer than the sum's ulp), so stepping z one ulp
    towards the target always arrives.  Returns x, y, z and the largest number of single-ulp nudges any point needed."""
    target = np.asarray(target, f32)
    az = np.radians(column_azimuth_deg(col, w))
    el = np.radians(np.asarray(ring_el_deg, np.float64))
    r = target.astype(np.float64)
    x = (r * np.cos(el) * np.sin(az)).astype(f32)   # horizonAngle = atan2(x, y)
    y = (r * np.cos(el) * np.cos(az)).astype(f32)
    z = (r * np.sin(el)).astype(f32)
    for _ in range(3):                              # Newton in double: d range / d z = z / range
        err = r - _range32(x, y, z).astype(np.float64)
        z = (z.astype(np.float64) + err * r / z.astype(np.float64)).astype(f32)
    nudges = 0
    for nudges in range(401):
        got = _range32(x, y, z)
        lo, hi = got < target, got > target
        if not (lo.any() or hi.any()):
            break
        z[lo] = np.nextafter(z[lo], f32(np.inf))    # z > 0: larger z, larger range
        z[hi] = np.nextafter(z[hi], f32(0))
    assert np.array_equal(_range32(x, y, z), target), "a range did not come out exact"
    return x, y, z, nudges


class _Ring:
    """a ring in EXTRACTION space: q[e] = range of the e-th kept point in lattice units, gap[e] = columns dropped just before it"""

    def __init__(self):
        self.q, self.gap, self.pending = [], [], 0

    def emit(self, vals):
        for v in vals:
            self.q.append(int(v)); self.gap.append(self.pending); self.pending = 0

    def columns_used(self):
        return len(self.q) + sum(self.gap) + self.pending


_PATTERNS = ([0, 1], [0, 1, 0, -1], [0, 2, 1], [0, 0, 3], [0, 1, 2, 1])
_STEPS = (18, 19, 20, 24, 40, 64)                   # 19/64 = 0.297 m and 20/64 = 0.3125 m straddle the 0.3 m occlusion bound


def _segment(rng, level, kind):
    """values of one segment starting from `level` (lattice units) and the level it ends on"""
    if kind == "flat":
        return [level] * int(rng.integers(8, 41)), level
    if kind == "ramp":
        s, n = int(rng.choice([-2, -1, 1, 2])), int(rng.integers(8, 31))
        return [level + s * k for k in range(n)], level + s * (n - 1)
    if kind == "pattern":
        pat, amp, n = _PATTERNS[int(rng.integers(len(_PATTERNS)))], int(rng.integers(1, 3)), int(rng.integers(12, 37))
        return [level + amp * pat[k % len(pat)] for k in range(n)], level
    if kind == "saw":                                # peaks of one height every `period` points: equal curvatures (10 a)^2 at period 6
        period = int(rng.choice([4, 5, 6, 6, 6, 7]))
        a = 8 if level < 900 else int(rng.choice([8, 12, 16]))      # a < 0.02 range (parallel-beam test) and a < 0.3 m (occlusion test)
        n = period * int(rng.integers(3, 9)) + 6
        return [level + (a if k % period == 5 else 0) for k in range(n)], level
    if kind == "zigzag":                             # +-6 units: every interior point has |diffRange| = 72/64, curvature 1.265625
        n = int(rng.integers(8, 21))
        return [level + (6 if k % 2 else -6) for k in range(n)], level
    raise ValueError(kind)


def _generic_ring(rng, w, drops, kinds=("flat", "flat", "ramp", "pattern", "pattern", "saw", "saw", "zigzag"), steps=True):
    """random segments until the ring's w columns are used; each run of `drops` (dropped columns) lands inside or at the edge of a segment,
    half of them together with a range step above 0.3 m (an occlusion candidate that only the column test rejects)"""
    R = _Ring()
    level = int(rng.integers(12 * LATTICE, 36 * LATTICE))
    drops = list(drops)
    R.pending = int(rng.integers(0, 4)) if drops else 0
    every = max(2, 14 // max(len(drops), 1))
    k = 0
    while R.columns_used() < w:
        kind = kinds[int(rng.integers(len(kinds)))]
        vals, level_next = _segment(rng, level, kind)
        k += 1
        if drops and k % every == 0:
            run = drops.pop(0)
            cut = int(rng.integers(0, len(vals) + 1)) if rng.random() < 0.6 else int(rng.choice([0, len(vals)]))
            jump = int(rng.choice([-1, 1])) * int(rng.choice([20, 24, 40])) if rng.random() < 0.5 else 0
            R.emit(vals[:cut]); R.pending += run
            R.emit([v + jump for v in vals[cut:]]); level_next += jump
        else:
            R.emit(vals)
        level = level_next
        if steps and rng.random() < 0.5:
            level += int(rng.choice([-1, 1])) * int(rng.choice(_STEPS))
        if level < 12 * LATTICE or level > 48 * LATTICE:
            level = int(rng.integers(16 * LATTICE, 32 * LATTICE))
    return R


def _uniform_ring(w, kind, level=20 * LATTICE):
    """a whole ring of one texture, every column populated"""
    e = np.arange(w)
    if kind == "flat":
        q = np.full(w, level)
    elif kind == "saw6":                             # a peak every 6th point: picks 6 apart do not suppress one another
        q = level + np.where(e % 6 == 3, 16, 0)
    elif kind == "saw67":                            # peaks alternately 6 and 7 apart
        q = level + np.where(np.isin(e % 13, (3, 9)), 16, 0)
    elif kind == "zigzag":
        q = level + np.where(e % 2 == 1, 6, -6)
    else:
        raise ValueError(kind)
    R = _Ring(); R.emit(q.tolist())
    return R


def cap_sector_length(w):
    """points per sector of a cap ring: 24 where the image has room for no more (424 of 450 columns), else 30"""
    return 24 if w < 520 else 30


def _cap_ring(rng, w):
    """6 L + 10 points, so six sectors of L points: sector 2 = ring positions 4 + 2 L .. 3 + 3 L.  Its points (and two beyond each end)
    are each separated from their neighbours by 10 dropped columns (column difference 11 > 10: no suppression across) and lie in a
    zig-zag whose points all share one curvature above the edge threshold: L tied corner candidates that do not suppress one another,
    so the sector reaches a 21st.  The rest of the ring is flat."""
    L = cap_sector_length(w)
    n, first, last = 6 * L + 10, 4 + 2 * L, 3 + 3 * L
    assert w >= n + 10 * (L + 3), "too few columns for a cap ring"
    level = int(rng.integers(14 * LATTICE, 30 * LATTICE))
    R = _Ring()
    for e in range(n):
        if first - 1 <= e <= last + 2:
            R.pending = 10
        R.emit([level + ((6 if e % 2 else -6) if first - 8 <= e <= last + 8 else 0)])
    return R


def _short_ring(rng, w, k):
    R = _Ring()
    level = int(rng.integers(12 * LATTICE, 36 * LATTICE))
    R.pending = int(rng.integers(0, max(w - k, 1)))
    R.emit([level + int(rng.integers(-2, 3)) for _ in range(k)])
    return R


DEFAULT_DROPS = (9, 10, 11, 40, 8, 10, 12)


def structured_sweep(h, w, seed, *, drops=DEFAULT_DROPS, ring_points=None, cap_rings=(), ring_kinds=None, dup_fraction=0.0,
                     shuffle=False, bad_ring_points=0, limits=None, n_limit_points=0, steps=True, segment_kinds=None):
    """A PointXYZIRT sweep of h rings x w columns with exact lattice ranges (see the module docstring).

    drops           lengths of the dropped column runs laid into every generic ring (rotated from ring to ring); () for none
    ring_points     {ring: k}: that ring holds exactly k points (0 = an empty ring)
    cap_rings       rings built by _cap_ring: one sector with 24 tied, mutually unsuppressed corner candidates
    ring_kinds      {ring: "full" | "flat" | "saw6" | "saw67" | "zigzag"}: "full" = generic segments, every column populated; the others are
                    one texture over the whole ring
    dup_fraction    share of extra points that compete for an occupied pixel (same column and ring, range a few lattice steps off)
    shuffle         permute the input order (the first point in input order wins a pixel)
    bad_ring_points points with ring >= h (projection drops them)
    limits, n_limit_points   (lo, hi) and a count: per count four points are moved to ranges lo, hi (kept by `<` / `>`) and one ulp
                    outside each (dropped)
    steps           range steps between the segments of a generic ring
    segment_kinds   the textures a generic ring draws its segments from (default: all of flat, ramp, pattern, saw, zigzag)"""
    rng = np.random.default_rng(seed)
    ring_points, ring_kinds = dict(ring_points or {}), dict(ring_kinds or {})
    cols, rings, targets = [], [], []
    gk = dict(steps=steps) if segment_kinds is None else dict(steps=steps, kinds=tuple(segment_kinds))
    for ring in range(h):
        if ring in ring_points:
            R = _short_ring(rng, w, ring_points[ring])
        elif ring in cap_rings:
            R = _cap_ring(rng, w)
        elif ring_kinds.get(ring, "generic") == "full":
            R = _generic_ring(rng, w, (), **gk)
        elif ring in ring_kinds:
            R = _uniform_ring(w, ring_kinds[ring], level=int(rng.integers(16 * LATTICE, 30 * LATTICE)))
        else:
            d = list(drops)
            R = _generic_ring(rng, w, d[ring % len(d):] + d[:ring % len(d)] if d else (), **gk)
        col = np.arange(len(R.q)) + np.cumsum(np.asarray(R.gap, np.int64))
        keep = col < w
        cols.append(col[keep]); rings.append(np.full(int(keep.sum()), ring)); targets.append(np.asarray(R.q, np.int64)[keep])
    col, ring, q = np.concatenate(cols), np.concatenate(rings), np.concatenate(targets)
    target = (q.astype(np.float64) / LATTICE).astype(f32)
    assert np.array_equal(target.astype(np.float64) * LATTICE, q)                      # the lattice is float32-exact
    if limits is not None and n_limit_points:
        lo, hi = f32(limits[0]), f32(limits[1])
        vals = [lo, hi, np.nextafter(lo, f32(0)), np.nextafter(hi, f32(np.inf))]
        where = rng.choice(len(target), 4 * n_limit_points, replace=False)
        target[where] = np.tile(np.array(vals, f32), n_limit_points)
    n_dup = int(dup_fraction * len(col))
    if n_dup:                                                                           # later in input order unless shuffled
        pick = rng.integers(0, len(col), n_dup)
        col, ring = np.concatenate([col, col[pick]]), np.concatenate([ring, ring[pick]])
        off = rng.integers(1, 4, n_dup) * rng.choice([-1, 1], n_dup)
        target = np.concatenate([target, (target[pick].astype(np.float64) + off / LATTICE).astype(f32)])
    if bad_ring_points:
        col = np.concatenate([col, rng.integers(0, w, bad_ring_points)])
        bad = h + rng.integers(0, 4, bad_ring_points); bad[::3] = 65535
        ring = np.concatenate([ring, bad])
        target = np.concatenate([target, (rng.integers(12 * LATTICE, 30 * LATTICE, bad_ring_points) / LATTICE).astype(f32)])
    el = 8.0 + 16.0 * (np.minimum(ring, h) / max(h, 1))                                 # 8 .. 24 degrees: z keeps its leverage on the range
    x, y, z, nudges = exact_points(col, el, target, w)
    if shuffle:
        perm = rng.permutation(len(x))
        x, y, z, ring = x[perm], y[perm], z[perm], ring[perm]
    out = np.zeros(len(x), XYZIRT)
    out["x"], out["y"], out["z"], out["ring"] = x, y, z, ring.astype(np.uint16)
    out["intensity"] = rng.uniform(0, 255, len(x)).astype(f32)
    out["time"] = np.linspace(0, 0.1, len(x), dtype=f32)
    structured_sweep.last_nudges = nudges
    return out


# --------------------------------------------------------------------------------------------------------------- census
def _cdiv(a, b):
    """C integer division: truncates toward zero"""
    return abs(a) // b if a >= 0 else -(abs(a) // b)


def params_dict(p):
    """a FeatureParams structure (the oracle's or the library's) or a dict -> dict"""
    if isinstance(p, dict):
        return dict(p)
    return {f: getattr(p, f) for f, _ in p._fields_}


def census(cloud, params):
    """Restates laserProcessing.cpp:467-713 on `cloud` and counts the events on the way.  Where the reference has no defined
    behaviour this follows the project's definitions: per-frame arrays start at zero, the +-5 neighbour accesses stop at the cloud's
    ends, equal curvatures sort by index.  Returns a dict of counts (see the keys below), the five index lists under "lists", and per
    position arrays under "pos_*" for tests that look at single gaps or sectors."""
    p = params_dict(params)
    H, W, rate = p["n_scan"], p["horizon_scan"], p["downsample_rate"]
    edge_thr, surf_thr = f32(p["edge_threshold"]), f32(p["surf_threshold"])
    x, y, z = (np.asarray(cloud[k], f32) for k in "xyz")
    rng_ = _range32(x, y, z)                                                            # :483, pointDistance
    ring = np.asarray(cloud["ring"]).astype(np.int64)
    ok = ~((rng_ < f32(p["min_range"])) | (rng_ > f32(p["max_range"]))) & (ring < H) & (ring % rate == 0)
    at = np.arctan2(x.astype(np.float64), y.astype(np.float64)).astype(f32)             # float atan2 = the correctly rounded value
    ha = ((at * f32(180)).astype(np.float64) / np.pi).astype(f32)                       # :491
    v = (ha.astype(np.float64) - 90.0) / float(f32(360.0 / float(f32(W))))
    rnd = np.sign(v) * np.floor(np.abs(v) + 0.5)                                        # C round(): halves away from zero
    col = (-rnd + W // 2).astype(np.int64)
    col = np.where(col >= W, col - W, col)
    ok &= (col >= 0) & (col < W)
    idx = np.nonzero(ok)[0]
    pix, first = np.unique(ring[idx] * W + col[idx], return_index=True)                 # :499 the first point in input order owns the pixel
    src = idx[first]                                                                    # row-major pixel order = cloudExtraction's
    n = len(src)
    ccol = (pix % W).astype(np.int64)
    pr = np.concatenate([rng_[src], np.zeros(16, f32)]).astype(f32)
    r_begin = np.searchsorted(pix, np.arange(H + 1) * W)                                # extracted range of every ring
    # calculateSmoothness :544-563
    curv = np.zeros(n + 16, f32)
    if n > 10:
        s = pr[0:n - 10] + pr[1:n - 9]
        s = s + pr[2:n - 8]; s = s + pr[3:n - 7]; s = s + pr[4:n - 6]
        s = s - pr[5:n - 5] * f32(10)
        s = s + pr[6:n - 4]; s = s + pr[7:n - 3]; s = s + pr[8:n - 2]; s = s + pr[9:n - 1]; s = s + pr[10:n]
        curv[5:n - 5] = s * s
    # markOccludedPoints :568-605
    picked = np.zeros(n + 16, np.int64)
    out = dict(n_extracted=n, occl_near_first=0, occl_near_second=0, parallel_marks=0, occl_rejected_by_column=0, pairs_col10=0)
    same_ring = np.zeros(max(n - 1, 0), bool)
    for r in range(H):
        same_ring[r_begin[r]:max(r_begin[r + 1] - 1, r_begin[r])] = True
    if n > 1:
        out["pairs_col10"] = int(np.sum((np.abs(np.diff(ccol)) == 10) & same_ring))     # inside a ring; the tests compare any neighbours
    if n > 11:
        i = np.arange(5, n - 6)
        d1, d2 = pr[i], pr[i + 1]
        cd = np.abs(ccol[i + 1] - ccol[i])
        a = (d1 - d2).astype(np.float64) > 0.3
        b = ~a & ((d2 - d1).astype(np.float64) > 0.3)
        near = cd < 10
        for l in range(-5, 1):
            picked[i[a & near] + l] = 1
        for l in range(1, 7):
            picked[i[b & near] + l] = 1
        diff1, diff2 = np.abs(pr[i - 1] - pr[i]), np.abs(pr[i + 1] - pr[i])
        par = (diff1.astype(np.float64) > 0.02 * pr[i].astype(np.float64)) & (diff2.astype(np.float64) > 0.02 * pr[i].astype(np.float64))
        picked[i[par]] = 1
        out.update(occl_near_first=int(np.sum(a & near)), occl_near_second=int(np.sum(b & near)), parallel_marks=int(par.sum()),
                   occl_rejected_by_column=int(np.sum((a | b) & ~near)))
    # extractFeatures :610-713
    picked = picked.tolist(); ccl = ccol.tolist(); cv = curv.tolist()
    label = [0] * (n + 16)
    cuts = dict(fwd=0, bwd=0)
    pick_pos = []

    def suppress(ind):
        for l in range(1, 6):
            if ind + l >= n or ind + l - 1 < 0:
                break
            if abs(ccl[ind + l] - ccl[ind + l - 1]) > 10:
                cuts["fwd"] += 1
                break
            picked[ind + l] = 1
        for l in range(-1, -6, -1):
            if ind + l < 0 or ind + l + 1 >= n:
                break
            if abs(ccl[ind + l] - ccl[ind + l + 1]) > 10:
                cuts["bwd"] += 1
                break
            picked[ind + l] = 1

    corner, surface, csharp, ssharp = [], [], [], []
    sectors = []                                                                       # one record per live sector
    edge_ties = surf_ties = skipped_in_live = short_rings = 0
    largest_sector = 0
    for r in range(H):
        start, end = int(r_begin[r]) - 1 + 5, int(r_begin[r + 1]) - 1 - 5
        if start > end:
            short_rings += 1
        live = skipped = 0
        for j in range(6):
            sp = _cdiv(start * (6 - j) + end * j, 6)
            ep = _cdiv(start * (5 - j) + end * (j + 1), 6) - 1
            if sp >= ep:
                skipped += 1
                continue
            live += 1
            largest_sector = max(largest_sector, ep - sp + 1)
            cs = curv[sp:ep]
            order = (np.lexsort((np.arange(sp, ep), cs)) + sp).tolist() + [ep]          # [sp, ep) by (curvature, index); ep stays put
            e_sel, s_sel = cs[cs > edge_thr], cs[cs < surf_thr]                          # ties: members of a group of equals beyond its first
            te, ts = len(e_sel) - len(np.unique(e_sel)), len(s_sel) - len(np.unique(s_sel))
            edge_ties += te; surf_ties += ts
            cand = int(sum(1 for k in range(sp, ep + 1) if picked[k] == 0 and f32(cv[k]) > edge_thr))
            rec = dict(ring=r, sector=j, sp=sp, ep=ep, edge_ties=te, surf_ties=ts, edge_candidates=cand, corners=0, corner_sharp=0, surface_picks=0, surface_sharp=0, reached_21=False)
            cnt = 0
            for k in range(ep, sp - 1, -1):
                ind = order[k - sp]
                if picked[ind] == 0 and f32(cv[ind]) > edge_thr:
                    cnt += 1
                    if cnt <= 20:
                        label[ind] = 1; corner.append(ind); rec["corners"] += 1
                        if cnt <= 4:
                            csharp.append(ind); rec["corner_sharp"] += 1
                    else:
                        rec["reached_21"] = True
                        break
                    picked[ind] = 1; pick_pos.append(ind); suppress(ind)
            cnt = 0
            for k in range(sp, ep + 1):
                ind = order[k - sp]
                if picked[ind] == 0 and f32(cv[ind]) < surf_thr:
                    cnt += 1; label[ind] = -1; picked[ind] = 1
                    rec["surface_picks"] += 1
                    if cnt <= 10:
                        ssharp.append(ind); rec["surface_sharp"] += 1
                    pick_pos.append(ind); suppress(ind)
            for k in range(sp, ep + 1):
                if label[k] <= 0:
                    surface.append(k)
            sectors.append(rec)
        if live:
            skipped_in_live += skipped
    to_src = lambda l: src[np.asarray(l, np.int64)].astype(np.int32) if len(l) else np.zeros(0, np.int32)
    out.update(edge_ties=edge_ties, surf_ties=surf_ties, cut_fwd=cuts["fwd"], cut_bwd=cuts["bwd"],
               sectors_reaching_21=sum(s["reached_21"] for s in sectors), sectors_over_10_surface=sum(s["surface_picks"] > 10 for s in sectors),
               max_edge_ties_in_sector=max([s["edge_ties"] for s in sectors] or [0]), max_surf_ties_in_sector=max([s["surf_ties"] for s in sectors] or [0]),
               sectors_skipped_in_live_rings=skipped_in_live, rings_start_after_end=short_rings, largest_sector=largest_sector,
               sectors=sectors, pos_col=ccol, pos_src=src.astype(np.int32), pos_curv=curv[:n], pick_pos=np.asarray(sorted(pick_pos), np.int64),
               ring_begin=r_begin,
               lists=dict(deskewed=src.astype(np.int32), corner=to_src(corner), surface=to_src(surface), corner_sharp=to_src(csharp),
                          surface_sharp=to_src(ssharp)))
    return out


FLOORS = dict(edge_ties=20, surf_ties=200, cut_fwd=5, cut_bwd=5, pairs_col10=3, occl_near_first=5, occl_near_second=5,
              occl_rejected_by_column=3, sectors_reaching_21=2, sectors_skipped_in_live_rings=3, rings_start_after_end=2)


def floors_missed(cs, floors=FLOORS):
    """the event classes of a census that stay under their floor: {name: (count, floor)}"""
    return {k: (cs[k], v) for k, v in floors.items() if cs[k] < v}


def counts_line(cs):
    """the census's scalar counts, for a test's printed record"""
    return ", ".join(f"{k}={v}" for k, v in cs.items() if isinstance(v, (int, np.integer)) and not isinstance(v, bool))


def gap_pick_distances(cs, min_cols=10, max_cols=12):
    """for every neighbour pair inside a ring whose columns differ by min_cols .. max_cols: (position of the pair's first point, column
    difference, distance in positions from the gap to the nearest pick on either side)"""
    col, picks, rb = cs["pos_col"], cs["pick_pos"], cs["ring_begin"]
    res = []
    for r in range(len(rb) - 1):
        for i in range(int(rb[r]), int(rb[r + 1]) - 1):
            cd = abs(int(col[i + 1]) - int(col[i]))
            if min_cols <= cd <= max_cols:
                d = int(min(np.min(np.abs(picks - i)), np.min(np.abs(picks - (i + 1))))) if len(picks) else 10 ** 9
                res.append((i, cd, d))
    return res
