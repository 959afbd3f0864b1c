"""The definition behind tests/test_normal_rows.py: the normal-equation partial rows of `row_and_reduce` (csrc/lisreg_assoc.hip) in
float64, the planted batch they are checked on, and the float64 residual models that say which planted query is accepted.  No GPU.

A partial row is 28 numbers per workgroup of <= 256 queries: with row = [arz, arx, ary, cz, cx, cy] and b = -coeff.intensity of
LMOptimization (odomEstimationNode.cpp:862-915) for every ACCEPTED query, entries 0-20 are the upper triangle of sum row^T row
(row-major), 21-26 sum row * b, 27 the number of accepted queries.  rows_from_coefficients() forms the 28 terms of every query from
the float32 pose, the float32 untransformed source point and float32 coefficients, in float64, from the reference's formulas as they
are written there — sines and cosines of the float32 angles taken in float64, no pose-only factors pulled out (`K[]` of
write_pose_cache is the device's business) — and block_sums() adds them per block descriptor with math.fsum.  The coefficients and
the accept flags are INPUTS: the GPU test hands in the kernel's own (lisreg_get_partial_rows), so that the comparison holds no
threshold straddler and no conditioning of a fit, only the roundings of the stage under test.

The error budget, counted from the code.  u = 2^-24 is the bound of one float32 rounding relative to the rounded value; every count is
relative to the MAGNITUDE sum of the quantity — the same formula with every factor's absolute value and every difference made a sum,
which is what rows_from_coefficients returns as the second array — so that cancellation inside arx / ary / arz cannot break it.

  sinf / cosf (write_pose_cache, lisreg_solve.hip)       2 ulp each (the bar tests/test_solve_step.py holds the pose cache to), and an
                                                         ulp is at most 2 u of the value:                              4 u per factor
  a pose-only factor K[i]: at most three such factors, two products                     3 * 4 + 2                 = 14 u
      K[9], K[10], K[12], K[13], K[15], K[18] are differences of two such products: one more rounding              = 15 u
  jacobian_row: K[i] * p (1), the sum of three such products (2), times the coefficient (1), the sum of the three
      groups (2)  (contraction to fused multiply-adds only removes roundings)              15 + 1 + 2 + 1 + 2          = 21 u
      row[3..5] and b are the coefficients themselves: exact
  the term row[r] * row[c]: both factors' errors and the product's rounding                21 + 21 + 1                 = 43 u
  the halving butterfly: six float32 additions on the way from 64 lanes to one (a value meets one addition per level; levels
      permlane32, permlane16, row mirror, half-row mirror, quad [3,2,1,0], quad [1,0,3,2])                            +  6 u
  the fp64 part (conversion exact, three additions of the four wave sums at 2^-53 each) and every second-order term of the
      above ((1 + u)^49 - 1 - 49 u < 2e-4 u)                                                                          +  1 u
                                                                                                          C_ROUND   = 50

so |device - fsum| <= C_ROUND * 2^-24 * A per entry, A the block's sum of the terms' magnitudes.  Entry 27 is a sum of exact ones in
float32 (<= 64 per wavefront) and fp64: no budget, it is compared exactly.  C_ROUND is derived, not tuned on any device output.

The planted batch (planted_batch): every accepted query has its own five-point target patch on a 3 m lattice, so that its five
neighbours are unambiguous at knn_sq_thresh = 1; rejected queries are of four planted kinds (KINDS_REJECTED); which query of a segment is
accepted is decided by its POSITION in the segment (PATTERNS), i.e. by the lane and wavefront it lands on in the 256-query workgroups.
models() restates the two residual models in float64 and reports every decision with its margin; check_margins() asserts the margins
with no query exempt.  census() is the mutation census: what a subtly wrong reduction would do to the rows, against the budget."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
U = 2.0 ** -24
C_ROUND = 50
N_ACC = 28
# value index k of the 28 terms -> (r, c) of the upper triangle, row-major (the kernel's R[] / C[])
TRI_R = (0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4, 4, 5)
TRI_C = (0, 1, 2, 3, 4, 5, 1, 2, 3, 4, 5, 2, 3, 4, 5, 3, 4, 5, 4, 5, 5)
TAU = 1.0                           # knn_sq_thresh
LINE_RATIO, PLANE_TOL, ACCEPT_S = 3.0, 0.2, 0.1       # lisreg_default_params


# ---------------------------------------------------------------- the rows
def _lm_row(trig, p, c, sub, neg):
    """arx, ary, arz of odomEstimationNode.cpp:898-907, literally.  sub(a, b) = a - b and neg(a) = -a give the values; with the
    absolute values of every input, sub = a + b and neg = a they give the magnitude sums."""
    srx, crx, sry, cry, srz, crz = trig
    px, py, pz = p
    cx, cy, cz = c
    arx = (sub(crx * sry * srz * px + crx * crz * sry * py, srx * sry * pz) * cx
           + sub(sub(neg(srx * srz * px), crz * srx * py), crx * pz) * cy
           + sub(crx * cry * srz * px + crx * cry * crz * py, cry * srx * pz) * cz)
    ary = ((sub(cry * srx * srz, crz * sry) * px + (sry * srz + cry * crz * srx) * py + crx * cry * pz) * cx
           + sub(sub(neg(cry * crz), srx * sry * srz) * px + sub(cry * srz, crz * srx * sry) * py, crx * sry * pz) * cz)
    arz = ((sub(crz * srx * sry, cry * srz) * px + sub(neg(cry * crz), srx * sry * srz) * py) * cx
           + sub(crx * crz * px, crx * srz * py) * cy
           + ((sry * srz + cry * crz * srx) * px + sub(crz * sry, cry * srx * srz) * py) * cz)
    return arx, ary, arz


def rows_from_coefficients(T, src_xyz, cf, ok):
    """T: the float32 pose [roll, pitch, yaw, x, y, z]; src_xyz[n, 3]: the UNtransformed float32 source points; cf[n, 4]: float32
    coefficients (coeff.x, y, z, intensity); ok[n]: accept flags.  Returns (terms[n, 28], magnitudes[n, 28]) in float64; the rows of
    queries that are not accepted are zero."""
    T = np.asarray(T, f32).astype(f64)
    src = np.asarray(src_xyz, f32).astype(f64).reshape(-1, 3)
    cf = np.asarray(cf, f32).astype(f64).reshape(-1, 4)
    ok = np.asarray(ok).astype(bool).reshape(-1)
    cf = np.where(ok[:, None], cf, 0.0)                       # (a rejected plane's coefficients are NaN on the device)
    # :862-867 — srx = sin(T[1]) ..., in float64 on the float32 angles
    trig = (math.sin(T[1]), math.cos(T[1]), math.sin(T[2]), math.cos(T[2]), math.sin(T[0]), math.cos(T[0]))
    # :889-896 — lidar -> camera
    p = (src[:, 1], src[:, 2], src[:, 0])
    c = (cf[:, 1], cf[:, 2], cf[:, 0])
    arx, ary, arz = _lm_row(trig, p, c, lambda a, b: a - b, lambda a: -a)
    mrx, mry, mrz = _lm_row(tuple(abs(t) for t in trig), tuple(np.abs(x) for x in p), tuple(np.abs(x) for x in c),
                            lambda a, b: a + b, lambda a: a)
    row = np.stack([arz, arx, ary, c[2], c[0], c[1]], 1)      # :909-914
    mag = np.stack([mrz, mrx, mry, np.abs(c[2]), np.abs(c[0]), np.abs(c[1])], 1)
    b = -cf[:, 3]                                             # :915
    n = len(src)
    terms, mags = np.zeros((n, N_ACC)), np.zeros((n, N_ACC))
    for k in range(21):
        terms[:, k] = row[:, TRI_R[k]] * row[:, TRI_C[k]]
        mags[:, k] = mag[:, TRI_R[k]] * mag[:, TRI_C[k]]
    for k in range(6):
        terms[:, 21 + k] = row[:, k] * b
        mags[:, 21 + k] = mag[:, k] * np.abs(b)
    terms[:, 27] = 1.0
    mags[:, 27] = 1.0
    terms[~ok] = 0.0
    mags[~ok] = 0.0
    return terms, mags


def fsum_rows(a):
    """math.fsum down the columns of a[n, 28]"""
    a = np.asarray(a, f64).reshape(-1, N_ACC)
    return np.array([math.fsum(a[:, k]) for k in range(N_ACC)], f64)


def block_sums(blocks, terms, mags):
    """blocks[n_blocks, 4] = (item, kind, first batch position, count); terms / mags[n_elems, 28] in batch-position order.  Returns
    (sums[n_blocks, 28], A[n_blocks, 28]): the exactly rounded sums of every block's terms and of their magnitudes."""
    blocks = np.asarray(blocks).reshape(-1, 4)
    S, A = np.zeros((len(blocks), N_ACC)), np.zeros((len(blocks), N_ACC))
    for i, (_, _, first, count) in enumerate(blocks):
        S[i] = fsum_rows(terms[first:first + count])
        A[i] = fsum_rows(mags[first:first + count])
    return S, A


def budget(A):
    """the bound on |device - fsum| per entry (module docstring); entry 27, the count, has none"""
    out = C_ROUND * U * np.asarray(A, f64)
    out[..., 27] = 0.0
    return out


def terms_of_batch(batch, coef, coef_ok):
    """rows_from_coefficients for every segment of a batch, in batch-position order"""
    terms, mags = np.zeros((batch["n_elems"], N_ACC)), np.zeros((batch["n_elems"], N_ACC))
    for sg in batch["segments"]:
        a, b = sg["base"], sg["base"] + sg["n"]
        terms[a:b], mags[a:b] = rows_from_coefficients(batch["items"][sg["item"]]["T"], sg["src"][:, :3], coef[a:b], coef_ok[a:b])
    return terms, mags


def plan_blocks(batch):
    """plan_item_tables (csrc/lisreg_batch_plan.hpp) restated: 256-query workgroups per segment, corner then surf of every item"""
    out = []
    for sg in batch["segments"]:
        for s in range(0, sg["n"], 256):
            out.append((sg["item"], sg["kind"], sg["base"] + s, min(256, sg["n"] - s)))
    return np.array(out, np.int32).reshape(-1, 4)


# ---------------------------------------------------------------- the float64 residual models
def pose_matrix(T):
    """trans2Affine3f (common.cpp:54-57) of the float32 pose, in float64: Rz(yaw) Ry(pitch) Rx(roll), then the translation"""
    T = np.asarray(T, f32).astype(f64)
    A, B, C, D, E, F = math.cos(T[2]), math.sin(T[2]), math.cos(T[1]), math.sin(T[1]), math.cos(T[0]), math.sin(T[0])
    M = np.eye(4)
    M[:3, :3] = [[A * C, A * D * F - B * E, B * F + A * D * E], [B * C, A * E + B * D * F, B * D * E - A * F], [-D, C * F, C * E]]
    M[:3, 3] = T[3:6]
    return M


def to_map(T, src_xyz):
    M = pose_matrix(T)
    return np.asarray(src_xyz, f32).astype(f64) @ M[:3, :3].T + M[:3, 3]


def knn5(tgt, q):
    """the five nearest target points of every query, float64 on the float32 coordinates: (idx[n, 5] (-1 where the target is short),
    d2[n, 5] (inf there))"""
    tgt = np.asarray(tgt, f32).astype(f64).reshape(-1, 3)
    n = len(q)
    idx, d2 = np.full((n, 5), -1, np.int64), np.full((n, 5), np.inf)
    if len(tgt) and n:
        D = ((q[:, None, :] - tgt[None, :, :]) ** 2).sum(-1)
        k = min(5, len(tgt))
        o = np.argsort(D, axis=1, kind="stable")[:, :k]
        idx[:, :k] = o
        d2[:, :k] = np.take_along_axis(D, o, 1)
    return idx, d2


def surf_model(nb, q, w=1.0):
    """surfOptimization's body (odomEstimationNode.cpp:776-821) in float64 for one query: nb[5, 3], q[3] (transformed).  Returns
    dict(normal, pd, res (max |n.p + pd| of the five), pd2, s, cf[4], plane_ok, ok)."""
    x = np.linalg.lstsq(nb, -np.ones(5), rcond=None)[0]
    ps = np.linalg.norm(x)
    n, pd = x / ps, 1.0 / ps
    res = np.abs(nb @ n + pd).max()
    pd2 = n @ q + pd
    s = 1.0 - 0.9 * abs(pd2) / math.sqrt(np.linalg.norm(q))
    plane_ok = bool(res <= PLANE_TOL)
    return dict(normal=n, pd=pd, res=res, dist=pd2, s=s, cf=w * s * np.append(n, pd2), model_ok=plane_ok, ok=plane_ok and s > ACCEPT_S)


def corner_model(nb, q, w=1.0):
    """cornerOptimization's body (:658-742) in float64: the line through the centroid along the top eigenvector of the covariance,
    lambda0 > 3 lambda1, the point-to-line distance and its gradient."""
    c = nb.mean(0)
    a = nb - c
    lam, vec = np.linalg.eigh(a.T @ a / 5.0)
    l0, l1, v = lam[2], lam[1], vec[:, 2]
    p1, p2 = c + 0.1 * v, c - 0.1 * v
    x0, y0, z0 = q
    (x1, y1, z1), (x2, y2, z2) = p1, p2
    m11 = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)
    m22 = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)
    m33 = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)
    a012 = math.sqrt(m11 * m11 + m22 * m22 + m33 * m33)
    l12 = math.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2 + (z1 - z2) ** 2)
    la = ((y1 - y2) * m11 + (z1 - z2) * m22) / a012 / l12
    lb = -((x1 - x2) * m11 - (z1 - z2) * m33) / a012 / l12
    lc = -((x1 - x2) * m22 + (y1 - y2) * m33) / a012 / l12
    ld2 = a012 / l12
    s = 1.0 - 0.9 * abs(ld2)
    line_ok = bool(l0 > LINE_RATIO * l1)
    return dict(normal=np.array([la, lb, lc]), l0=l0, l1=l1, direction=v, dist=ld2, s=s, cf=w * s * np.array([la, lb, lc, ld2]),
                model_ok=line_ok, ok=line_ok and s > ACCEPT_S)


def label_weights(payload_bits, label_score):
    """label_weight (lisreg_assoc.hip): w = float32(2.0 - LabelSorce[label]) for labels below 32, else 2.0; the label is the low 16 bits"""
    lab = np.asarray(payload_bits, np.uint32) & np.uint32(0xffff)
    wtab = (2.0 - np.asarray(label_score, f32).astype(f64)).astype(f32)
    return np.where(lab < 32, wtab[np.minimum(lab, 31)], f32(2.0)).astype(f64)


def models(batch, label_score=None):
    """Every query of the batch through the float64 models on the float32 inputs.  Per segment a dict of arrays over its queries:
    d5 (squared distance of the fifth neighbour), found, idx[n, 5], ok, cf[n, 4] as float32 (zero where no model was evaluated), s, res /
    l0 / l1 (NaN where not applicable), dist, normal."""
    out = []
    for sg in batch["segments"]:
        it = batch["items"][sg["item"]]
        tgt = it["tgt"][sg["kind"]]
        n = sg["n"]
        q = to_map(it["T"], sg["src"][:, :3])
        idx, d2 = knn5(tgt, q)
        found = d2[:, 4] < TAU
        w = np.ones(n) if label_score is None else label_weights(sg["src"][:, 3].copy().view(np.uint32), label_score)
        r = dict(d5=d2[:, 4], found=found, idx=idx, ok=np.zeros(n, bool), cf=np.zeros((n, 4), f32), s=np.full(n, np.nan), res=np.full(n, np.nan),
                 l0=np.full(n, np.nan), l1=np.full(n, np.nan), dist=np.full(n, np.nan), normal=np.full((n, 3), np.nan), w=w, q=q)
        t64 = np.asarray(tgt, f32).astype(f64).reshape(-1, 3)
        for i in np.flatnonzero(found):
            m = (corner_model if sg["kind"] == 0 else surf_model)(t64[idx[i]], q[i], w[i])
            r["ok"][i], r["cf"][i], r["s"][i], r["dist"][i], r["normal"][i] = m["ok"], m["cf"].astype(f32), m["s"], m["dist"], m["normal"]
            if sg["kind"] == 0:
                r["l0"][i], r["l1"][i] = m["l0"], m["l1"]
            else:
                r["res"][i] = m["res"]
        out.append(r)
    return out


def flat(batch, per_segment, key):
    return np.concatenate([r[key] for r in per_segment]) if per_segment else np.zeros(0)


def check_margins(batch, mods):
    """every planted decision keeps its margin in the float64 models, no query exempt, and comes out as planted"""
    for sg, r in zip(batch["segments"], mods):
        what = (sg["item"], sg["kind"])
        assert np.all((r["d5"] <= 0.5) | (r["d5"] >= 2.0)), (what, "fifth neighbour", r["d5"][(r["d5"] > 0.5) & (r["d5"] < 2.0)])
        f = r["found"]
        if sg["kind"] == 1:
            assert np.all((r["res"][f] <= PLANE_TOL / 2) | (r["res"][f] >= PLANE_TOL * 2)), (what, "plane tolerance", r["res"][f])
        else:
            assert np.all((r["l0"][f] >= 2 * LINE_RATIO * r["l1"][f]) | (r["l0"][f] <= LINE_RATIO / 2 * r["l1"][f])), (what, "eigenvalue ratio")
        assert np.all(np.abs(r["s"][f] - ACCEPT_S) >= 0.05), (what, "accept_s", r["s"][f])
        kinds = sg["planted"]
        assert np.array_equal(r["ok"], kinds == "accept"), (what, "accepted set", np.flatnonzero(r["ok"] != (kinds == "accept")))
        assert not f[np.isin(kinds, ("nofound", "four"))].any() and f[np.isin(kinds, ("rough", "far"))].all(), (what, "found")
        if sg["kind"] == 1:
            assert np.all(r["res"][kinds == "rough"] >= 2 * PLANE_TOL) and np.all(r["res"][kinds == "far"] <= PLANE_TOL / 2), what
            assert np.all(r["s"][kinds == "far"] <= ACCEPT_S - 0.05) and np.all(r["s"][kinds == "rough"] >= ACCEPT_S + 0.05), what
        else:
            assert np.all(r["l0"][kinds == "rough"] <= LINE_RATIO / 2 * r["l1"][kinds == "rough"]), what


# ---------------------------------------------------------------- the planted batch
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
KINDS_REJECTED = ("nofound", "four", "rough", "far")     # no point within 1 m / a four-point patch / a rough plane or a fat line / s < accept_s


def pattern_mask(name, n):
    """which positions of an n-query segment are accepted.  Position p sits on lane p % 64 of wavefront (p % 256) // 64 of the
    segment's workgroup p // 256 (k_rows_reduce: tid = p - bd.start, workgroups start at multiples of 256)."""
    pos = np.arange(n)
    lane, wave = pos % 64, pos // 64
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "lane0":
        return lane == 0
    if name == "lane63":
        return lane == 63
    if name == "lanes31_32":
        return (lane == 31) | (lane == 32)
    if name == "lanes15_16":
        return (lane == 15) | (lane == 16)
    if name == "one_per_wave":                               # another lane in every wavefront, inside a short last one too
        wave_len = np.minimum(64, n - wave * 64)
        return lane == (7 * wave + 3) % wave_len
    if name == "last_of_tail":
        return pos == n - 1
    if name == "alternating":
        return pos % 2 == 0
    raise KeyError(name)


PATTERNS = ("all", "none", "lane0", "lane63", "lanes31_32", "lanes15_16", "one_per_wave", "last_of_tail", "alternating")

# name, pose [roll, pitch, yaw, x, y, z], (corner size, pattern), (surf size, pattern), flags
ITEMS = (
    dict(name="quiet_a", T=(0.31, -0.47, 0.93, 1.0, -0.5, 0.25), corner=(1, "all"), surf=(63, "lane0"), where="quiet"),
    dict(name="loud", T=(-0.83, 0.29, -1.13, 3.0, -2.0, 1.5), corner=(65, "all"), surf=(257, "all"), where="loud"),
    dict(name="quiet_b", T=(-0.22, 0.64, -0.38, -0.75, 0.5, 1.0), corner=(64, "lane63"), surf=(64, "lanes31_32"), where="quiet"),
    dict(name="alternating", T=(1.17, -0.21, 0.55, -4.0, 2.5, -1.0), corner=(63, "alternating"), surf=(255, "alternating"), where="mid"),
    dict(name="tails", T=(-0.36, -1.05, 0.27, 2.0, 5.0, -3.0), corner=(255, "last_of_tail"), surf=(513, "one_per_wave"), where="mid"),
    dict(name="level", T=(0.0, 0.0, 0.0, 1.5, -2.5, 0.75), corner=(256, "lanes31_32"), surf=(256, "lanes15_16"), where="mid", far=True),
    dict(name="no_corner", T=(0.58, 0.77, -0.71, -2.0, -3.5, 2.0), corner=(0, "none"), surf=(65, "lane63"), where="mid"),
    dict(name="four_point_surf_target", T=(-1.09, 0.33, 1.19, 3.5, 1.0, -2.0), corner=(257, "one_per_wave"), surf=(1, "none"), where="mid",
         short_surf=True),
    dict(name="wide", T=(0.24, -0.62, -0.97, -1.5, 4.0, 2.5), corner=(513, "lanes15_16"), surf=(1, "all"), where="mid", far=True),
    dict(name="none", T=(0.71, 1.12, 0.43, 2.5, -1.5, -4.0), corner=(63, "none"), surf=(64, "none"), where="mid"),
)

# labels 0-19 (config/label.yaml), 20-31 (read as score 0), >= 32, each under high payload bits of its own
LABELS = tuple(range(20)) + (20, 25, 31, 32, 40, 1000, 65535)


def _unit(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def _frame(n):
    u = np.cross(n, [1.0, 0.0, 0.0] if abs(n[0]) < 0.9 else [0.0, 1.0, 0.0])
    u /= np.linalg.norm(u)
    return u, np.cross(n, u)


_FLAT5 = np.array([[0.25, 0.0], [-0.2, 0.15], [-0.1, -0.25], [0.15, 0.2], [0.0, -0.05]])


def _plane_patch(rng, centre, normal, scale=1.0, noise=0.01):
    u, v = _frame(normal)
    a = rng.uniform(0, 2 * np.pi)
    R = np.array([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]])
    uv = _FLAT5 @ R.T * rng.uniform(0.7, 1.0) * scale
    return centre + np.outer(uv[:, 0], u) + np.outer(uv[:, 1], v) + np.outer(rng.uniform(-noise, noise, 5), normal)


def _item_geometry(rng, spec, n_nodes):
    """lattice nodes (3 m apart) and cell centres in the SOURCE frame.  Quiet items: the eight nodes (+-1.5)^3, every coordinate below
    2 m; the loud item: nodes from 54 m up; the others: a lattice laid so that the pre-image of the map's origin is a cell centre
    (every node is then 2.6 m from the map origin: the robust weight of surf_eval, which divides by the square root of the range,
    stays well defined, and the origin cell is free for the patch of the `far` kind)."""
    M = pose_matrix(np.array(spec["T"], f32))
    if spec["where"] == "quiet":
        g, base = 2, np.full(3, -1.5)
    else:
        g = 2
        while g ** 3 < n_nodes:
            g += 1
        g += 1
        s_star = -M[:3, :3].T @ M[:3, 3]
        base = np.array([54.0, 51.0, 57.0]) if spec["where"] == "loud" else s_star + 1.5 - 3.0 * (g // 2)
    ijk = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), -1).reshape(-1, 3)
    nodes = base + 3.0 * ijk
    cells = base + 1.5 + 3.0 * ijk[(ijk < g - 1).all(1)]
    if spec["where"] == "mid":
        s_star = -M[:3, :3].T @ M[:3, 3]
        cells = cells[np.linalg.norm(cells - s_star, axis=1) > 1.0]
    return M, nodes[rng.permutation(len(nodes))], cells


def _segment(rng, spec, kind, M, nodes, cells, payload_at):
    """the target cloud (map frame, float32) and the source records (float32 [n, 4]) of one (item, kind), with the planted kind of every query"""
    size, pattern = spec["corner" if kind == 0 else "surf"]
    accept = pattern_mask(pattern, size)
    if kind == 1 and spec.get("short_surf"):
        accept[:] = False
    Rm, t = M[:3, :3], M[:3, 3]
    fwd = lambda p: p @ Rm.T + t
    back = lambda p: (p - t) @ Rm
    tgt, src, planted = [], np.zeros((size, 3)), np.empty(size, object)
    node = iter(nodes)
    short = kind == 1 and spec.get("short_surf")
    # the two shared patches of the rejected kinds: four points; a rough plane / a fat line
    four_c = next(node)
    tgt.append(four_c + rng.uniform(-0.2, 0.2, (4, 3)))
    rough_c = None
    if not short:
        rough_c = next(node)
        Q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
        shape = (np.array([[0, 0, 0.62], [0, 0, -0.62], [0.62, 0, 0], [-0.62, 0, 0], [0, 0.62, 0]]) if kind == 1 else
                 np.array([[0.3, 0.25, 0], [-0.3, 0.25, 0], [0.3, -0.25, 0], [-0.3, -0.25, 0], [0.02, 0.01, 0]]))
        tgt.append(rough_c + shape @ Q.T)
    far = kind == 1 and spec.get("far")
    n0 = _unit(rng)
    if far:                                                  # in the MAP frame: a small plane patch 0.55 m from the map's origin
        tgt.append(back(_plane_patch(rng, 0.55 * n0, n0, scale=0.45, noise=0.0)))
    kinds = ["nofound", "four"] + ([] if short else ["rough"]) + (["far"] if far else [])
    if short:
        kinds = ["four"]
    turn = 0
    for i in range(size):
        if accept[i]:
            c = next(node)
            d = _unit(rng)
            if kind == 1:
                while abs((Rm @ d) @ fwd(c)) < 0.5:          # the plane keeps half a metre from the map's origin ([p] n = -1 has a solution)
                    d = _unit(rng)
                tgt.append(_plane_patch(rng, c, d))
                u, v = _frame(d)
                src[i] = c + rng.choice([-1, 1]) * rng.uniform(0.05, 0.25) * d + rng.uniform(-0.1, 0.1) * u + rng.uniform(-0.1, 0.1) * v
            else:
                tgt.append(c + np.outer(np.array([-0.3, -0.15, 0.0, 0.15, 0.3]) * rng.uniform(0.7, 1.0), d) + rng.uniform(-0.005, 0.005, (5, 3)))
                u, v = _frame(d)
                a = rng.uniform(0, 2 * np.pi)
                src[i] = c + rng.uniform(0.05, 0.3) * (np.cos(a) * u + np.sin(a) * v) + rng.uniform(-0.1, 0.1) * d
            planted[i] = "accept"
            continue
        k = kinds[turn % len(kinds)]
        turn += 1
        planted[i] = k
        if k == "nofound":
            src[i] = cells[rng.integers(len(cells))] + rng.uniform(-0.3, 0.3, 3)
        elif k == "four":
            src[i] = four_c + rng.uniform(-0.2, 0.2, 3)
        elif k == "rough":
            src[i] = rough_c + rng.uniform(-0.04, 0.04, 3)
        else:
            u, v = _frame(n0)
            qm = rng.choice([-1, 1]) * rng.uniform(0.02, 0.05) * n0 + rng.uniform(-0.06, 0.06) * u + rng.uniform(-0.06, 0.06) * v
            src[i] = back(qm)
    tgt = fwd(np.concatenate(tgt))
    tgt = tgt[rng.permutation(len(tgt))].astype(f32)
    rec = np.zeros((size, 4), f32)
    rec[:, :3] = src.astype(f32)
    bits = np.array([payload_at(i) for i in range(size)], np.uint32)
    rec[:, 3] = bits.view(f32)
    return tgt, rec, planted.astype(str), accept


_BATCHES = {}


def planted_batch(seed=0):
    """dict(items=[dict(name, T float32[6], tgt=(corner, surf) float32[n, 3], src=(corner, surf) float32[n, 4], spec)],
    segments=[dict(item, kind, base, n, src, planted, accept, pattern)] in batch order (every item's corner, then its surf),
    n_elems).  Cached: the same arrays serve every test and nobody writes to them."""
    if seed in _BATCHES:
        return _BATCHES[seed]
    rng = np.random.default_rng(1000 + seed)
    items, segments, base = [], [], 0
    counter = [0]

    def payload_at(_):
        k = counter[0]
        counter[0] += 1
        hi = 1 + (k * 2654435761 >> 7) % 0x7f00               # high payload bits, never an all-ones exponent
        return (hi << 16) | LABELS[k % len(LABELS)]
    for i, spec in enumerate(ITEMS):
        n_acc = [int(pattern_mask(spec[k][1], spec[k][0]).sum()) for k in ("corner", "surf")]
        M, nodes, cells = _item_geometry(rng, spec, max(n_acc) + 2)
        tg, sr = [], []
        for kind in (0, 1):
            tgt, rec, planted, accept = _segment(rng, spec, kind, M, nodes, cells, payload_at)
            tg.append(tgt)
            sr.append(rec)
            segments.append(dict(item=i, kind=kind, base=base, n=len(rec), src=rec, planted=planted, accept=accept,
                                 pattern=spec["corner" if kind == 0 else "surf"][1]))
            base += len(rec)
        items.append(dict(name=spec["name"], T=np.array(spec["T"], f32), tgt=tuple(tg), src=tuple(sr), spec=spec))
    b = dict(items=items, segments=segments, n_elems=base)
    for sg in segments:
        sg["src"].setflags(write=False)
        sg["planted"].setflags(write=False)
    _BATCHES[seed] = b
    return b


# ---------------------------------------------------------------- the mutation census
def census(batch, mods, factor=100.0):
    """For every block with an accepted row: each mutation of the module docstring's kind must move at least one of entries 0-26 of a
    block's reference row by more than factor x that entry's budget (the count, entry 27, is left out of the census: it is compared
    exactly, and a census it could satisfy alone would say nothing about the other 27).  Returns the smallest ratio
    (moved / budget, maximum over the entries) per mutation kind; raises AssertionError naming the first survivor."""
    ok = flat(batch, mods, "ok")
    cf = np.concatenate([r["cf"] for r in mods])
    found = flat(batch, mods, "found")
    blocks = plan_blocks(batch)
    terms, mags = terms_of_batch(batch, cf, ok)
    would, _ = terms_of_batch(batch, cf, found)              # the would-be rows of rejected queries whose model was evaluated
    S, A = block_sums(blocks, terms, mags)
    worst = dict(remove=np.inf, add=np.inf, move=np.inf, swap=np.inf)

    def ratio(delta, a_ref):
        """max over entries 0-26 of |delta| / budget (budget 0 with a non-zero move counts as infinite)"""
        bud = (C_ROUND * U * a_ref)[:27]
        d = np.abs(delta[:27])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(d > 0, d / bud, 0.0)
        return float(np.max(r))

    def seen(kind, r, what):
        assert r > factor, (kind, what, r)
        worst[kind] = min(worst[kind], r)
    for bi, (item, kind, first, count) in enumerate(blocks):
        sl = slice(first, first + count)
        acc = np.flatnonzero(ok[sl]) + first
        # (the budget a faulty device row is held to is the REFERENCE's: the GPU test makes A from the accept flags, not from the rows)
        for q in acc:                                                                   # one accepted row lost
            seen("remove", ratio(terms[q], A[bi]), (bi, int(q)))
        for q in np.flatnonzero(found[sl] & ~ok[sl]) + first:                           # one rejected query's row added
            if np.any(cf[q] != 0):
                seen("add", ratio(would[q], A[bi]), (bi, int(q)))
        for nb_ in (bi - 1, bi + 1):                                                    # one row moved into the adjacent block: both blocks are off
            if 0 <= nb_ < len(blocks):
                for q in acc:
                    seen("move", min(ratio(terms[q], A[nb_]), ratio(terms[q], A[bi])), (bi, nb_, int(q)))
        if len(acc):
            for k in range(12):                                                         # value index k swapped with k + 16
                mut, mut_a = S[bi].copy(), A[bi].copy()
                mut[[k, k + 16]] = mut[[k + 16, k]]
                mut_a[[k, k + 16]] = mut_a[[k + 16, k]]
                seen("swap", ratio(mut - S[bi], A[bi]), (bi, k))
    return worst
