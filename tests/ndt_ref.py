"""The definition of lisreg_ndt_* : Normal Distributions Transform registration, restated in numpy float64.

The reference selects pcl::NormalDistributionsTransform with epsilon 0.01, step size 0.1, resolution 1.0 and 35 iterations
(src/core/registration.cpp:147-155, subMapOptmizationNode.cpp:2756-2760).  Neither PCL nor its source is available to this
project, so this file restates the method from Magnusson 2009 (eq. 6.8-6.21, algorithm 2) and More & Thuente 1994 the way PCL's
class is remembered to drive them.  Where PCL versions differ or memory of PCL is unsure, this file picks ONE reading and says
so; what is written here is the definition the GPU code is tested against — it is not "PCL's".

Readings picked (each one a possible departure from the PCL a user has installed):
  * the source points are transformed in DOUBLE from their float coordinates (PCL transforms the cloud in float): the
    definition then does not depend on whether a compiler contracts a*b+c;
  * the voxel covariance is  sum d d^T / (n - 1)  around the double mean, two passes (PCL's single-pass form is believed to
    differ by a factor of the order (n - 1) / n);
  * p = (tx, ty, tz, a, b, c) with x' = Rx(a) Ry(b) Rz(c) x + t; the angles of a guess matrix are a = atan2(-R12, R22),
    b = asin(R02), c = atan2(-R01, R00) — Eigen's [0, pi] range convention of eulerAngles is not reproduced (the OUTPUT is the
    transform, which does not depend on the chart);
  * the point Jacobian / Hessian (eq. 6.19 / 6.21) are the first and second derivatives of Rx Ry Rz x, written as products of the
    elementary matrices and their derivatives; PCL's small-angle shortcut (|angle| < 10e-5 => cos = 1, sin = 0) applies to the
    DERIVATIVES only, x' itself uses the true sine and cosine;
  * line_search = 1: More-Thuente with the interval starting NOT converged; some PCL releases are remembered to initialise that
    flag so that the loop never runs — that behaviour is line_search = 0 (one evaluation at clamp(|delta|, step_min, step_max));
  * the step is accepted under the STRONG Wolfe conditions as published (psi <= 0 and |phi'| <= nu |phi'(0)|); PCL is remembered
    to test phi' <= nu |phi'(0)| on one side only;
  * the next trial is selected from the interval BEFORE the current trial updates it, as in the published algorithm (MINPACK's
    dcstep); selected after the update, the trial would coincide with an end point after every U2 / U3 update;
  * degenerate trials: when the (clamped) trial coincides with the end point a_l — or with a_u where case 4 interpolates from
    a_u — the interpolation would divide by zero: the search ENDS and that trial is the step.  A cubic whose discriminant is
    negative has no minimiser and is not a candidate; if a selection yields no finite value the search ends the same way.  No NaN
    can reach p;
  * a source point meets every valid voxel whose mean lies within `resolution` of x' (squared distance <= resolution^2).  The
    loop form searches all voxels, the vector form the 27 cells around the cell of x' (floor(x' / resolution) in double): a mean
    lies in its own cell up to float rounding of the cell index, so the two can differ only for a pair within rounding of the
    radius;
  * NaN target points belong to no voxel; the bounding box that places the grid takes each coordinate's finite minimum / maximum;
  * H^+ drops singular values <= 6 eps sigma_max.
"""
import numpy as np

DEFAULTS = dict(resolution=1.0, step_size=0.1, transformation_epsilon=0.01, outlier_ratio=0.55,
                min_covar_eigvalue_mult=0.01, max_iters=35, min_points_per_voxel=6, line_search=1)
MU, NU, MAX_TRIALS = 1.0e-4, 0.9, 10
TRI = [(i, j) for i in range(6) for j in range(i, 6)]          # the 21 upper-triangle entries of the Hessian, row-major


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def gauss_constants(outlier_ratio, resolution):
    c1 = 10.0 * (1.0 - outlier_ratio)
    c2 = outlier_ratio / resolution ** 3
    d3 = -np.log(c2)
    d1 = -np.log(c1 + c2) - d3
    d2 = -2.0 * np.log((-np.log(c1 * np.exp(-0.5) + c2) - d3) / d1)
    return d1, d2


# ---- target voxels -----------------------------------------------------------------------------------------------------------
def voxel_cells(xyz32, resolution):
    """cell id of every point (-1: a NaN point), grid dims, min_b — pcl::VoxelGrid's float arithmetic (k_voxel_keys)."""
    xyz32 = np.ascontiguousarray(xyz32, np.float32)
    inv = np.float32(1.0) / np.float32(resolution)
    with np.errstate(invalid="ignore"):
        lo, hi = np.nanmin(xyz32, 0), np.nanmax(xyz32, 0)
        min_b = np.floor(lo * inv).astype(np.int64)
        max_b = np.floor(hi * inv).astype(np.int64)
        dims = max_b - min_b + 1
        ok = ~np.isnan(xyz32).any(1)
        ijk = np.zeros(xyz32.shape, np.int64)
        ijk[ok] = (np.floor(xyz32[ok] * inv) - min_b.astype(np.float32)).astype(np.int64)
    cell = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]
    cell[~ok] = -1
    return cell, dims, min_b


def voxel_stats_one(pts64, min_pts, mult):
    """(mean, inverse covariance) of one voxel's points, or None if the voxel is not valid."""
    n = len(pts64)
    if n < min_pts:
        return None
    mean = pts64.sum(0) / n
    d = pts64 - mean
    cov = (d.T @ d) / (n - 1)
    lam, V = np.linalg.eigh(cov)                         # ascending
    if lam[0] < 0 or lam[1] < 0 or lam[2] <= 0:
        return None
    floor_ = mult * lam[2]
    lam = np.array([max(lam[0], floor_), max(lam[1], floor_), lam[2]])
    with np.errstate(all="ignore"):
        try:
            icov = np.linalg.inv((V * lam) @ V.T)
        except np.linalg.LinAlgError:
            return None
    if not np.isfinite(icov).all():
        return None
    return mean, 0.5 * (icov + icov.T)


def build_target(xyz32, prm):
    xyz32 = np.ascontiguousarray(xyz32, np.float32)
    cell, dims, min_b = voxel_cells(xyz32, prm["resolution"])
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    first = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    last = np.r_[first[1:], len(sc)]
    ids, counts, means, icovs = [], [], [], []
    n_voxels = 0
    for a, b in zip(first, last):
        if sc[a] < 0:
            continue
        n_voxels += 1
        r = voxel_stats_one(xyz32[order[a:b]].astype(np.float64), prm["min_points_per_voxel"], prm["min_covar_eigvalue_mult"])
        if r is None:
            continue
        ids.append(sc[a]); counts.append(b - a); means.append(r[0]); icovs.append(r[1])
    return dict(resolution=float(prm["resolution"]), dims=dims, min_b=min_b, n_voxels=n_voxels,
                cell_ids=np.array(ids, np.int64), counts=np.array(counts, np.int64),
                means=np.array(means, np.float64).reshape(-1, 3), icov=np.array(icovs, np.float64).reshape(-1, 3, 3))


def icov6(icov):
    """upper triangle (xx, xy, xz, yy, yz, zz) of [m, 3, 3]"""
    return np.stack([icov[:, 0, 0], icov[:, 0, 1], icov[:, 0, 2], icov[:, 1, 1], icov[:, 1, 2], icov[:, 2, 2]], 1)


# ---- pose ----------------------------------------------------------------------------------------------------------------------
def _cs(angle, shortcut):
    if shortcut and abs(angle) < 10e-5:
        return 1.0, 0.0
    return np.cos(angle), np.sin(angle)


def _elem(axis, c, s):
    """the elementary rotation about `axis` and its first and second derivative by the angle"""
    if axis == 0:
        return (np.array([[1, 0, 0], [0, c, -s], [0, s, c]], float), np.array([[0, 0, 0], [0, -s, -c], [0, c, -s]], float),
                np.array([[0, 0, 0], [0, -c, s], [0, -s, -c]], float))
    if axis == 1:
        return (np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], float), np.array([[-s, 0, c], [0, 0, 0], [-c, 0, -s]], float),
                np.array([[-c, 0, -s], [0, 0, 0], [s, 0, -c]], float))
    return (np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], float), np.array([[-s, -c, 0], [c, -s, 0], [0, 0, 0]], float),
            np.array([[-c, s, 0], [-s, -c, 0], [0, 0, 0]], float))


def pose_matrices(p):
    """R (true trigonometry), dR [3] and ddR [6: aa, ab, ac, bb, bc, cc] (small-angle shortcut), products formed left to right."""
    X, _, _ = _elem(0, *_cs(p[3], False)); Y, _, _ = _elem(1, *_cs(p[4], False)); Z, _, _ = _elem(2, *_cs(p[5], False))
    R = (X @ Y) @ Z
    X, X1, X2 = _elem(0, *_cs(p[3], True)); Y, Y1, Y2 = _elem(1, *_cs(p[4], True)); Z, Z1, Z2 = _elem(2, *_cs(p[5], True))
    dR = np.stack([(X1 @ Y) @ Z, (X @ Y1) @ Z, (X @ Y) @ Z1])
    ddR = np.stack([(X2 @ Y) @ Z, (X1 @ Y1) @ Z, (X1 @ Y) @ Z1, (X @ Y2) @ Z, (X @ Y1) @ Z1, (X @ Y) @ Z2])
    return R, dR, ddR


ANG_PAIR = {(0, 0): 0, (0, 1): 1, (0, 2): 2, (1, 1): 3, (1, 2): 4, (2, 2): 5}


def p_from_matrix(M):
    M = np.asarray(M, np.float64).reshape(4, 4)
    R = M[:3, :3]
    return np.array([M[0, 3], M[1, 3], M[2, 3], np.arctan2(-R[1, 2], R[2, 2]), np.arcsin(min(1.0, max(-1.0, R[0, 2]))),
                     np.arctan2(-R[0, 1], R[0, 0])])


def matrix_from_p(p):
    M = np.eye(4)
    M[:3, :3] = pose_matrices(p)[0]
    M[:3, 3] = p[:3]
    return M


def transform_points(p, src32):
    R = pose_matrices(p)[0]
    x = np.asarray(src32, np.float32).astype(np.float64)
    return ((R[:, 0] * x[:, 0:1] + R[:, 1] * x[:, 1:2]) + R[:, 2] * x[:, 2:3]) + np.asarray(p[:3], np.float64)


# ---- one evaluation ------------------------------------------------------------------------------------------------------------
def _empty_eval():
    return dict(out=np.zeros(28), abs=np.zeros(28), n_pairs=0)


def evaluate_loops(tgt, src32, p, prm, with_hessian=True):
    """score, gradient [6], Hessian upper triangle [21] as out[28]; abs[28] = sum of |term| per output; n_pairs."""
    d1, d2 = gauss_constants(prm["outlier_ratio"], prm["resolution"])
    r2 = prm["resolution"] ** 2
    R, dR, ddR = pose_matrices(p)
    ev = _empty_eval()
    for x32 in np.asarray(src32, np.float32).reshape(-1, 3):
        x = x32.astype(np.float64)
        if np.isnan(x).any():
            continue
        xt = ((R[:, 0] * x[0] + R[:, 1] * x[1]) + R[:, 2] * x[2]) + p[:3]
        J = [np.array([1.0, 0, 0]), np.array([0, 1.0, 0]), np.array([0, 0, 1.0])] + [dR[k] @ x for k in range(3)]
        Hv = [ddR[k] @ x for k in range(6)]
        for v in range(len(tgt["means"])):
            q = xt - tgt["means"][v]
            if not (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] <= r2):
                continue
            C = tgt["icov"][v]
            cq = C @ q
            e = np.exp(-d2 * (q @ cq) / 2.0)
            ev["n_pairs"] += 1
            ev["out"][0] += -d1 * e
            ev["abs"][0] += abs(d1 * e)
            w = d2 * e
            if w > 1 or w < 0 or np.isnan(w):
                continue
            w *= d1
            cJ = [cq @ J[i] for i in range(6)]
            for i in range(6):
                ev["out"][1 + i] += w * cJ[i]
                ev["abs"][1 + i] += abs(w * cJ[i])
            if with_hessian:
                for k, (i, j) in enumerate(TRI):
                    t = -d2 * cJ[i] * cJ[j] + J[j] @ (C @ J[i])
                    if i >= 3:
                        t += cq @ Hv[ANG_PAIR[(i - 3, j - 3)]]
                    ev["out"][7 + k] += w * t
                    ev["abs"][7 + k] += abs(w * t)
    return ev


def _cell_table(tgt):
    if "_table" not in tgt:
        tab = np.full(int(np.prod(tgt["dims"])), -1, np.int64)
        tab[tgt["cell_ids"]] = np.arange(len(tgt["cell_ids"]))
        tgt["_table"] = tab
    return tgt["_table"]


def find_pairs(tgt, xt, r):
    """(point index, voxel index) of every pair within r, through the 27 cells around the cell of each x'"""
    dims, tab = tgt["dims"], _cell_table(tgt)
    ok = ~np.isnan(xt).any(1)
    ijk = np.zeros(xt.shape, np.int64)
    big = np.clip(np.floor(xt[ok] * (1.0 / r)), -2.0e9, 2.0e9)
    ijk[ok] = big.astype(np.int64) - tgt["min_b"]
    pi, vi = [], []
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                c = ijk + np.array([dx, dy, dz])
                inb = ok & (c >= 0).all(1) & (c < dims).all(1)
                idx = np.flatnonzero(inb)
                v = tab[c[idx, 0] + c[idx, 1] * dims[0] + c[idx, 2] * dims[0] * dims[1]]
                keep = v >= 0
                idx, v = idx[keep], v[keep]
                q = xt[idx] - tgt["means"][v]
                near = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2] <= r * r
                pi.append(idx[near]); vi.append(v[near])
    return np.concatenate(pi), np.concatenate(vi)


def evaluate(tgt, src32, p, prm, with_hessian=True, pairs=None):
    """the vector form of evaluate_loops.  pairs: a fixed (point index, voxel index) set instead of the radius search at p — the score
    as a smooth function of p, for the tests that difference it"""
    d1, d2 = gauss_constants(prm["outlier_ratio"], prm["resolution"])
    p = np.asarray(p, np.float64)
    R, dR, ddR = pose_matrices(p)
    x = np.asarray(src32, np.float32).reshape(-1, 3).astype(np.float64)
    xt = transform_points(p, src32)
    ev = _empty_eval()
    if len(tgt["means"]) == 0 or len(x) == 0:
        return ev
    pi, vi = find_pairs(tgt, xt, prm["resolution"]) if pairs is None else pairs
    ev["n_pairs"] = len(pi)
    if len(pi) == 0:
        return ev
    q = xt[pi] - tgt["means"][vi]
    C = tgt["icov"][vi]
    cq = np.einsum("nij,nj->ni", C, q)
    e = np.exp(-d2 * np.einsum("ni,ni->n", q, cq) / 2.0)
    ev["out"][0] = np.sum(-d1 * e); ev["abs"][0] = np.sum(np.abs(d1 * e))
    w = d2 * e
    use = ~((w > 1) | (w < 0) | np.isnan(w))
    w = np.where(use, w * d1, 0.0)
    J = np.zeros((len(pi), 6, 3))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, 3:] = np.einsum("kij,nj->nki", dR, x[pi])
    cJ = np.einsum("ni,nki->nk", cq, J)
    ev["out"][1:7] = np.sum(w[:, None] * cJ, 0); ev["abs"][1:7] = np.sum(np.abs(w[:, None] * cJ), 0)
    if with_hessian:
        Hv = np.einsum("kij,nj->nki", ddR, x[pi])
        CJ = np.einsum("nij,nkj->nki", C, J)
        JCJ = np.einsum("nji,nki->njk", J, CJ)                 # [n, j, i] = J_j . C J_i
        for k, (i, j) in enumerate(TRI):
            t = -d2 * cJ[:, i] * cJ[:, j] + JCJ[:, j, i]
            if i >= 3:
                t = t + np.einsum("ni,ni->n", cq, Hv[:, ANG_PAIR[(i - 3, j - 3)]])
            ev["out"][7 + k] = np.sum(w * t); ev["abs"][7 + k] = np.sum(np.abs(w * t))
    return ev


def unpack(out):
    g = np.array(out[1:7])
    H = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRI):
        H[i, j] = H[j, i] = out[7 + k]
    return out[0], g, H


# ---- decisions: every comparison a run's path depends on goes through here -------------------------------------------------------
class Decisions:
    """records the smallest margin |a - b| / scale by which a comparison of a run was decided (min_margin) and the branches taken"""

    def __init__(self):
        self.min_margin = np.inf
        self.where = None
        self.log = []

    def _note(self, a, b, scale, tag):
        m = abs(a - b) / scale if scale > 0 else np.inf
        if m < self.min_margin:
            self.min_margin, self.where = m, tag

    def gt(self, a, b, scale, tag): self._note(a, b, scale, tag); return a > b
    def lt(self, a, b, scale, tag): self._note(a, b, scale, tag); return a < b
    def ge(self, a, b, scale, tag): self._note(a, b, scale, tag); return a >= b
    def le(self, a, b, scale, tag): self._note(a, b, scale, tag); return a <= b


# ---- More-Thuente ----------------------------------------------------------------------------------------------------------------
def _cubic(a_e, f_e, g_e, a_t, f_t, g_t):
    """minimiser of the cubic through (a_e, f_e, g_e), (a_t, f_t, g_t) (Sun & Yuan 2006, eq. 2.4.52 / 2.4.56), or None"""
    z = 3.0 * (f_t - f_e) / (a_t - a_e) - g_t - g_e
    disc = z * z - g_t * g_e
    if not disc >= 0:
        return None
    w = np.sqrt(disc)
    den = g_t - g_e + 2.0 * w
    if den == 0:
        return None
    a_c = a_e + (a_t - a_e) * (w - g_e - z) / den
    return a_c if np.isfinite(a_c) else None


def trial_value(I, a_t, f_t, g_t, D, sf, sg):
    """next trial from the interval I = [a_l, f_l, g_l, a_u, f_u, g_u] and the current trial; None: no finite value (the search ends)."""
    a_l, f_l, g_l, a_u, f_u, g_u = I
    sa = abs(a_t - a_l)
    if D.gt(f_t, f_l, sf, "case1"):
        D.log.append("case1")
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t))
        if a_c is None:
            return a_q if np.isfinite(a_q) else None
        if not np.isfinite(a_q):
            return a_c
        if D.lt(abs(a_c - a_l), abs(a_q - a_l), sa, "case1 pick"):
            return a_c
        return 0.5 * (a_q + a_c)
    if D.lt(g_t * g_l, 0.0, sg * abs(g_l), "case2"):
        D.log.append("case2")
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l
        if a_c is None:
            return a_s if np.isfinite(a_s) else None
        if D.ge(abs(a_c - a_t), abs(a_s - a_t), sa, "case2 pick"):
            return a_c
        return a_s
    if D.le(abs(g_t), abs(g_l), sg, "case3"):
        D.log.append("case3")
        a_c = _cubic(a_l, f_l, g_l, a_t, f_t, g_t)
        a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l if g_l != g_t else np.inf
        guard = a_t + 0.66 * (a_u - a_t)
        if a_c is not None and np.isfinite(a_s):
            nxt = a_c if D.lt(abs(a_c - a_t), abs(a_s - a_t), sa, "case3 pick") else a_s
        elif a_c is not None:
            nxt = a_c
        elif np.isfinite(a_s):
            nxt = a_s
        else:
            return guard
        return min(guard, nxt) if a_t > a_l else max(guard, nxt)
    D.log.append("case4")
    if a_t == a_u:
        return None
    return _cubic(a_u, f_u, g_u, a_t, f_t, g_t)


def update_interval(I, a_t, f_t, g_t, D, sf, sg):
    """the three updates; True: the interval has converged (g_t == 0)"""
    if D.gt(f_t, I[0 + 1], sf, "U1"):
        D.log.append("U1")
        I[3:6] = [a_t, f_t, g_t]
        return False
    s = g_t * (I[0] - a_t)
    D._note(g_t, 0.0, sg, "U2/U3")
    if s > 0:
        D.log.append("U2")
        I[0:3] = [a_t, f_t, g_t]
        return False
    if s < 0:
        D.log.append("U3")
        I[3:6] = I[0:3]
        I[0:3] = [a_t, f_t, g_t]
        return False
    return True


def line_search_mt(fun, phi_0, d_phi_0, step_init, step_max, step_min, D=None, sf=None, sg=None, max_trials=MAX_TRIALS):
    """fun(a) -> (phi(a), phi'(a)); d_phi_0 < 0.  Returns (a_t, trials made inside the loop).  sf / sg: the scales the decisions on
    function values / derivatives are measured against (default: |phi_0|, |d_phi_0|)."""
    D = D or Decisions()
    sf = abs(phi_0) if sf is None else sf
    sg = abs(d_phi_0) if sg is None else sg
    I = [0.0, 0.0, d_phi_0 - MU * d_phi_0, 0.0, 0.0, d_phi_0 - MU * d_phi_0]      # psi form: psi(0) = 0, psi'(0) = (1 - mu) phi'(0)

    def clamp(a):
        if D.gt(a, step_max, step_max, "clamp max"):
            a = step_max
        if D.lt(a, step_min, step_max, "clamp min"):
            a = step_min
        return a

    a_t = clamp(step_init)
    phi_t, d_phi_t = fun(a_t)
    psi_t, d_psi_t = phi_t - phi_0 - MU * d_phi_0 * a_t, d_phi_t - MU * d_phi_0
    open_interval, converged, trials = True, False, 0
    while not converged and trials < max_trials and not (D.le(psi_t, 0.0, sf, "wolfe 1") and D.le(abs(d_phi_t), NU * abs(d_phi_0), sg, "wolfe 2")):
        if open_interval and D.le(psi_t, 0.0, sf, "phase f") and D.ge(d_psi_t, 0.0, sg, "phase g"):
            open_interval = False
            I[1] += phi_0 - MU * d_phi_0 * I[0]; I[2] += MU * d_phi_0
            I[4] += phi_0 - MU * d_phi_0 * I[3]; I[5] += MU * d_phi_0
        f_t, g_t = (psi_t, d_psi_t) if open_interval else (phi_t, d_phi_t)
        if a_t == I[0]:
            D.log.append("degenerate")
            break
        a_next = trial_value(I, a_t, f_t, g_t, D, sf, sg)
        if a_next is None or not np.isfinite(a_next):
            D.log.append("no trial")
            break
        converged = update_interval(I, a_t, f_t, g_t, D, sf, sg)
        a_t = clamp(a_next)
        phi_t, d_phi_t = fun(a_t)
        psi_t, d_psi_t = phi_t - phi_0 - MU * d_phi_0 * a_t, d_phi_t - MU * d_phi_0
        trials += 1
    return a_t, trials


# ---- the loop --------------------------------------------------------------------------------------------------------------------
def solve_step(H, g):
    """delta = H^+ (-g) through the SVD; singular values <= 6 eps sigma_max are dropped"""
    if not np.isfinite(H).all():
        return np.full(6, np.nan)
    U, s, Vt = np.linalg.svd(H)
    keep = s > 6 * np.finfo(float).eps * (s[0] if len(s) else 0.0)
    y = (U.T @ (-g))
    y = np.where(keep, y / np.where(keep, s, 1.0), 0.0)
    return Vt.T @ y


def align(tgt, src32, prm, guess=None, D=None, history=None):
    """the whole registration; returns dict(p, T (float32 4x4), converged, iters, n_evals, n_pairs_last, score, trans_probability)"""
    D = D or Decisions()
    src32 = np.ascontiguousarray(np.asarray(src32, np.float32).reshape(-1, 3))
    p = p_from_matrix(np.eye(4) if guess is None else np.asarray(guess, np.float32).reshape(4, 4))
    eps = prm["transformation_epsilon"]
    state = dict(ev=evaluate(tgt, src32, p, prm, True), n_evals=1)
    iters, converged = 0, False
    while not converged:
        score, g, H = unpack(state["ev"]["out"])
        if history is not None:
            history.append((p.copy(), score))
        delta = solve_step(H, g)
        nrm = float(np.sqrt(np.sum(delta * delta)))
        if nrm == 0 or np.isnan(nrm):
            converged = not np.isnan(nrm)
            break
        delta = delta / nrm
        phi_0, d_phi_0 = -score, -float(g @ delta)
        absg = state["ev"]["abs"][1:7]
        a_t = 0.0
        if d_phi_0 != 0:
            if D.gt(d_phi_0, 0.0, float(absg @ np.abs(delta)), "reverse"):
                d_phi_0, delta = -d_phi_0, -delta
            sf, sg = abs(phi_0), float(absg @ np.abs(delta))
            base = p.copy()

            def fun(a, hess=False):
                state["ev"] = evaluate(tgt, src32, base + a * delta, prm, hess)
                state["n_evals"] += 1
                out = state["ev"]["out"]
                return -out[0], -float(out[1:7] @ delta)

            if prm["line_search"]:
                first = [True]

                def fun_mt(a):
                    h = first[0]; first[0] = False
                    return fun(a, h)                    # the first trial carries the Hessian; those inside the loop do not
                a_t, trials = line_search_mt(fun_mt, phi_0, d_phi_0, nrm, prm["step_size"], eps / 2, D, sf, sg)
                if trials:
                    fun(a_t, True)                      # one Hessian pass at the accepted step
            else:
                a_t = min(max(nrm, eps / 2), prm["step_size"])
                fun(a_t, True)
            p = base + a_t * delta
        if iters > prm["max_iters"] or (iters and D.lt(abs(a_t), eps, eps, "epsilon")):
            converged = True
        iters += 1
    score = state["ev"]["out"][0]
    return dict(p=p, T=matrix_from_p(p).astype(np.float32), converged=int(converged), iters=iters, n_evals=state["n_evals"],
                n_pairs_last=int(state["ev"]["n_pairs"]), score=float(score), trans_probability=float(score) / max(len(src32), 1),
                min_margin=D.min_margin, margin_where=D.where)


def smallest_margin(tgt, src32, prm, guess=None):
    """the smallest relative margin by which any line-search or convergence comparison of the run was decided"""
    D = Decisions()
    align(tgt, src32, prm, guess, D)
    return D.min_margin, D.where


def pose_error(T, T_true):
    """(translation distance, rotation angle) between two 4x4 transforms"""
    T, T_true = np.asarray(T, np.float64).reshape(4, 4), np.asarray(T_true, np.float64).reshape(4, 4)
    dR = T[:3, :3].T @ T_true[:3, :3]
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.arccos(min(1.0, max(-1.0, (np.trace(dR) - 1) / 2))))


# ---- the scenes of the tests -----------------------------------------------------------------------------------------------------
def scene(scan_seed=1000, trans=0.3, rot_deg=2.0):
    """(target xyz float32, source xyz float32, guess 4x4 float32, T_true 4x4 float64) of the loop-verification test scene"""
    from lisreg import synth
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=scan_seed, local_radius=12, trans=trans, rot_deg=rot_deg, pose_xy=(32, 31))
    tgt = np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])
    src = np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])
    src = np.ascontiguousarray(src[:: max(len(src) // 600, 1)])
    return tgt, src, synth.pose_matrix(c["T_init"]).astype(np.float32), synth.pose_matrix(c["T_true"].astype(np.float64))


def planted_cloud():
    """voxels of exactly 5 and 6 points, a coplanar and a collinear voxel, six identical points, NaN points, one crowded voxel"""
    rng = np.random.default_rng(77)

    def box(cx, cy, cz, n, scale=(0.8, 0.8, 0.8)):
        return np.array([cx, cy, cz]) + 0.1 + rng.uniform(0, 1, (n, 3)) * np.array(scale)
    parts = [box(0, 0, 0, 5), box(2, 0, 0, 6), box(4, 0, 0, 40),
             box(0, 2, 0, 12, (0.8, 0.8, 0.0)),                  # coplanar: z constant, one eigenvalue raised
             box(2, 2, 0, 9, (0.8, 0.0, 0.0)),                   # collinear: two eigenvalues raised
             np.repeat(np.array([[4.5, 2.5, 0.5]]), 6, 0),       # six identical points: rejected
             box(0, 0, 2, 3000), box(2, 2, 2, 25), box(3, 2, 2, 24), box(4, 2, 2, 70),
             np.full((3, 3), np.nan), np.array([[np.nan, 0.5, 0.5], [0.5, 0.5, np.nan]])]
    xyz = np.concatenate(parts).astype(np.float32)
    return np.ascontiguousarray(xyz[rng.permutation(len(xyz))])


# ---- the expected outputs kept in tests/golden/ndt (tests/golden/make_golden_ndt.py writes them, tests/test_ndt.py reads them) ------
DERIV_SIZES = (1, 63, 64, 65, 257, 0)              # source sizes of the one-evaluation cases; 0: the whole source
ALIGN_CASES = ((1000, 0.3, 2.0, 1), (1000, 0.3, 2.0, 0), (1001, 0.5, 3.0, 1), (1005, 0.5, 3.0, 1))     # scan seed, trans, rot_deg, line_search


def deriv_poses(guess, T_true):
    """the guess, the true pose, a pose whose three angles take the small-angle shortcut, a pose 100 m away (no pairs)"""
    pt = p_from_matrix(T_true)
    return np.stack([p_from_matrix(guess), pt, np.r_[pt[:3], 5e-5, -3e-5, 8e-5], pt + np.array([100.0, 0, 0, 0, 0, 0])])


def golden_cases():
    out = {}
    prm = params()
    planted = build_target(planted_cloud(), prm)
    tgt, src, guess, T_true = scene()
    T = build_target(tgt, prm)
    for name, t in (("planted", planted), ("scene", T)):
        sub = slice(None) if name == "planted" else slice(None, None, 8)          # the scene's statistics: every eighth voxel
        out[name + "_dims"] = np.r_[t["dims"], t["n_voxels"]].astype(np.int64)
        out[name + "_cell_ids"], out[name + "_counts"] = t["cell_ids"].astype(np.int32), t["counts"].astype(np.int32)
        out[name + "_means"], out[name + "_icov6"] = t["means"][sub], icov6(t["icov"])[sub]
    poses = deriv_poses(guess, T_true)
    out["deriv_p"] = poses
    sums, absum, pairs = [], [], []
    for p in poses:
        for n in DERIV_SIZES:
            for hess in (1, 0):
                ev = evaluate(T, src[: n or len(src)], p, prm, bool(hess))
                sums.append(ev["out"]); absum.append(ev["abs"]); pairs.append(ev["n_pairs"])
    out["deriv_out"], out["deriv_abs"], out["deriv_pairs"] = np.array(sums), np.array(absum), np.array(pairs, np.int64)
    rows, ps, absg = [], [], []
    for seed, trans, rot, ls in ALIGN_CASES:
        tg, sr, gs, tt = scene(seed, trans, rot)
        Tk = T if seed == 1000 else build_target(tg, prm)
        r = align(Tk, sr, params(line_search=ls), gs)
        et, er = pose_error(r["T"], tt)
        rows.append([r["iters"], r["n_evals"], r["converged"], r["n_pairs_last"], len(sr), len(Tk["means"])])
        ps.append(np.r_[r["p"], r["score"], r["min_margin"], et, er])
        absg.append(evaluate(Tk, sr, r["p"], params(line_search=ls), False)["abs"][1:7])
    out["align_counts"], out["align_p"], out["align_absg"] = np.array(rows, np.int64), np.array(ps), np.array(absg)
    return out
