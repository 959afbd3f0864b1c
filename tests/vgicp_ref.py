"""The definition of lisreg_vgicp_* : voxelised GICP registration (Koide et al. 2021), restated in numpy float64.

The reference's loop-closure step names select_registration_method("FAST_VGICP") as its authors' latest choice of verifier
(src/node/subMapOptmizationNode.cpp:2771) and src/core/registration.cpp:156-187 shows why it stayed a comment: the fast_gicp family
would not link.  fast_gicp's source is not available to this project, so this file restates FastVGICP + LsqRegistration from the paper
and from memory.  What is written here is the definition the GPU code is tested against — it is not "fast_gicp's".

Readings picked (each one a possible departure from the fast_gicp a user has installed):
  * distributions: the k nearest points of a point within its own cloud, itself included, by the squared distance
    ((dx dx + dy dy) + dz dz) in double from the float coordinates, ties by the lower index (fast_gicp asks a kd-tree, whose tie order
    is unspecified); covariance sum d d^T / k around the double mean, two passes (fast_gicp's single pass over homogeneous 4-vectors
    is believed to divide by k as well);
  * regularisation PLANE: eigenvalues (1, 1, plane_epsilon), C_i = I - (1 - plane_epsilon) n n^T with n the eigenvector of the smallest
    eigenvalue — written through the normal, so the result does not depend on the eigenvectors chosen inside the plane (fast_gicp
    multiplies U diag V^T of an SVD);
  * NaN points are no points: never a neighbour, no distribution, in no voxel, in no pair (fast_gicp expects clean clouds);
  * voxels: coordinate floor(x * (1 / resolution)) per axis — in float for the target's own points, against the grid placed at the
    floor of the finite bounding box (the voxel keys the library's voxel filter and NDT use); in double for a transformed source point.
    Both equal floor(x / resolution) at resolution 1.0, the reference's setting;
  * voxel statistics ADDITIVE: N points, mean of the points, mean of the points' C_i;
  * neighbourhood DIRECT1: the voxel containing x' only;  weight sqrt(N) on the pair's squared Mahalanobis distance
    (fast_gicp is remembered to weight the voxel's residual by sqrt(N); whether it squares that weight is not known here);
  * the source points are transformed in DOUBLE from their float coordinates;
  * M = (C_voxel + R C_a R^T)^-1 of the full 3 x 3 (fast_gicp works on 4 x 4 with a 1 planted at [3, 3]: the same numbers);
  * left perturbation T <- exp(delta) T, delta = (omega, v), residual mu - x', J = [skew(x') | -I], H = sum w J^T M J, b = sum w J^T M d;
  * Levenberg-Marquardt (LsqRegistration::step_lm as remembered): lambda starts at lm_init_lambda_factor max|diag H| of the FIRST
    linearisation and is carried across outer iterations; per outer iteration nu = 2 and at most lm_max_iterations trials of
    (H + lambda I) delta = -b; rho = (e - e') / (delta . (lambda delta - b)); NOT (rho >= 0) is a rejection (so a NaN rho rejects):
    converged delta -> the alignment stops as converged, else lambda <- nu lambda, nu <- 2 nu; rho >= 0 accepts, lambda <- lambda
    max(1/3, 1 - (2 rho - 1)^3), converged iff delta is;
  * a trial loop that runs out of trials ENDS the alignment, not converged (fast_gicp is remembered to return false from step_lm and
    to leave its loop); so does a (H + lambda I) that is not positive definite or not finite — no NaN can reach T;
  * "delta converged": max|exp(delta).R - I| / rotation_epsilon < 1 and max|exp(delta).t| / transformation_epsilon < 1, entry-wise;
  * a source without a pair at the guess: converged = 0, iters = 0, the guess (fast_gicp would solve a zero system).
"""
import numpy as np

import ndt_ref as NR

DEFAULTS = dict(resolution=1.0, transformation_epsilon=0.01, rotation_epsilon=2.0e-3, lm_init_lambda_factor=1.0e-9,
                plane_epsilon=1.0e-3, k_correspondences=20, max_iters=50, lm_max_iterations=10)
TRI = [(i, j) for i in range(6) for j in range(i, 6)]
pose_error = NR.pose_error


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


# ---- 1. distributions ----------------------------------------------------------------------------------------------------------
def sqdist(a64, b64):
    """((dx dx + dy dy) + dz dz), broadcasting over the leading axes"""
    d = a64 - b64
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def knn_loops(xyz32, k):
    """(neighbours [n, k] ascending by (distance, index), -1 rows for NaN points; gap [n] = relative gap between the k-th and the
    (k + 1)-th squared distance, inf when there is no (k + 1)-th point)"""
    x = np.asarray(xyz32, np.float32).astype(np.float64)
    ok = np.flatnonzero(~np.isnan(x).any(1))
    nbr = np.full((len(x), k), -1, np.int64)
    gap = np.full(len(x), np.inf)
    for i in ok:
        cand = sorted((float(sqdist(x[i], x[j])), int(j)) for j in ok)
        nbr[i] = [j for _, j in cand[:k]]
        if len(cand) > k:
            gap[i] = (cand[k][0] - cand[k - 1][0]) / cand[k][0] if cand[k][0] > 0 else 0.0
    return nbr, gap


def _knn_rows(x, rows, cand, k):
    """the k best of `cand` (ascending global indices) for every row: (neighbours, k-th distance, (k + 1)-th distance or inf)"""
    d = sqdist(x[rows][:, None, :], x[cand][None, :, :])
    kk = min(k, len(cand) - 1)
    part = np.partition(d, (k - 1, kk), axis=1)
    dk = part[:, k - 1]
    dk1 = part[:, k] if len(cand) > k else np.full(len(rows), np.inf)
    r, c = np.nonzero(d <= dk[:, None])                      # >= k per row; more only where distances tie with the k-th
    o = np.lexsort((c, d[r, c], r))                          # by row, then distance, then index (cand ascends)
    r, c = r[o], c[o]
    first = np.searchsorted(r, np.arange(len(rows)))
    take = first[:, None] + np.arange(k)[None, :]
    return cand[c[take]], dk, dk1


def knn(xyz32, k, tile=4.0, chunk=256):
    """the vector form of knn_loops.  Candidates come from the 3 x 3 block of xy tiles around a point's tile; a row whose k-th (and
    (k + 1)-th, for the gap) distance does not stay inside the block's inner margin is done again against all points."""
    x = np.asarray(xyz32, np.float32).astype(np.float64)
    n = len(x)
    ok = np.flatnonzero(~np.isnan(x).any(1))
    nbr = np.full((n, k), -1, np.int64)
    gap = np.full(n, np.inf)
    if len(ok) < k:
        raise ValueError("fewer finite points than k")
    txy = np.floor(x[ok, :2] / tile).astype(np.int64)
    txy -= txy.min(0)
    w = int(txy[:, 1].max()) + 3
    key = (txy[:, 0] + 1) * w + (txy[:, 1] + 1)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    again = []
    for t in np.unique(skey):
        rows = ok[order[np.searchsorted(skey, t):np.searchsorted(skey, t, "right")]]
        ks = np.array([t + dx * w + dy for dx in (-1, 0, 1) for dy in (-1, 0, 1)])
        cand = np.sort(np.concatenate([ok[order[np.searchsorted(skey, q):np.searchsorted(skey, q, "right")]] for q in ks]))
        if len(cand) <= k:
            again.append(rows)
            continue
        lo = (np.floor(x[rows[0], :2] / tile) - 1) * tile
        for a in range(0, len(rows), chunk):
            rr = rows[a:a + chunk]
            nb, dk, dk1 = _knn_rows(x, rr, cand, k)
            margin = np.minimum(x[rr, :2] - lo, lo + 3 * tile - x[rr, :2]).min(1)
            safe = dk1 < (0.999 * margin) ** 2
            nbr[rr[safe]] = nb[safe]
            with np.errstate(invalid="ignore", divide="ignore"):
                gap[rr[safe]] = np.where(dk1[safe] > 0, (dk1[safe] - dk[safe]) / dk1[safe], 0.0)
            again.append(rr[~safe])
    rest = np.concatenate(again) if again else np.zeros(0, np.int64)
    for a in range(0, len(rest), chunk):
        rr = rest[a:a + chunk]
        nb, dk, dk1 = _knn_rows(x, rr, ok, k)
        nbr[rr] = nb
        with np.errstate(invalid="ignore", divide="ignore"):
            gap[rr] = np.where(np.isinf(dk1), np.inf, np.where(dk1 > 0, (dk1 - dk) / np.where(dk1 > 0, dk1, 1.0), 0.0))
    return nbr, gap


def covariance_one(pts64, eps):
    """(C_i [3, 3], eigen-gap (lambda_mid - lambda_min) / lambda_max, 0 for a zero matrix) of one neighbourhood"""
    k = len(pts64)
    mean = pts64.sum(0) / k
    d = pts64 - mean
    cov = (d.T @ d) / k
    lam, V = np.linalg.eigh(cov)
    nrm = V[:, 0]
    return np.eye(3) - (1.0 - eps) * np.outer(nrm, nrm), ((lam[1] - lam[0]) / lam[2] if lam[2] > 0 else 0.0)


def distributions_loops(xyz32, prm):
    x = np.asarray(xyz32, np.float32).astype(np.float64)
    nbr, gap = knn_loops(xyz32, prm["k_correspondences"])
    C = np.full((len(x), 3, 3), np.nan)
    eg = np.full(len(x), np.nan)
    for i in range(len(x)):
        if nbr[i, 0] >= 0:
            C[i], eg[i] = covariance_one(x[nbr[i]], prm["plane_epsilon"])
    return dict(nbr=nbr, gap=gap, C=C, eig_gap=eg)


def distributions(xyz32, prm):
    """dict(nbr [n, k], gap [n], C [n, 3, 3] (NaN for NaN points), eig_gap [n])"""
    x = np.asarray(xyz32, np.float32).astype(np.float64)
    nbr, gap = knn(xyz32, prm["k_correspondences"])
    ok = nbr[:, 0] >= 0
    k = nbr.shape[1]
    P = x[nbr[ok]]                                            # [m, k, 3]
    mean = P.sum(1) / k
    d = P - mean[:, None, :]
    cov = np.einsum("nki,nkj->nij", d, d) / k
    lam, V = np.linalg.eigh(cov)
    nrm = V[:, :, 0]
    C = np.full((len(x), 3, 3), np.nan)
    C[ok] = np.eye(3) - (1.0 - prm["plane_epsilon"]) * np.einsum("ni,nj->nij", nrm, nrm)
    eg = np.full(len(x), np.nan)
    eg[ok] = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / np.where(lam[:, 2] > 0, lam[:, 2], 1.0), 0.0)
    return dict(nbr=nbr, gap=gap, C=C, eig_gap=eg)


def cov6(C):
    """upper triangle (xx, xy, xz, yy, yz, zz) of [m, 3, 3]"""
    return np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], 1)


# ---- 2. target voxels ----------------------------------------------------------------------------------------------------------
def build_target(xyz32, prm, dist=None):
    xyz32 = np.ascontiguousarray(xyz32, np.float32)
    dist = dist or distributions(xyz32, prm)
    cell, dims, min_b = NR.voxel_cells(xyz32, prm["resolution"])
    order = np.argsort(cell, kind="stable")
    sc = cell[order]
    first = np.flatnonzero(np.r_[True, sc[1:] != sc[:-1]])
    last = np.r_[first[1:], len(sc)]
    ids, counts, means, covs = [], [], [], []
    x = xyz32.astype(np.float64)
    for a, b in zip(first, last):
        if sc[a] < 0:
            continue
        sel = order[a:b]
        ids.append(sc[a]); counts.append(b - a)
        means.append(x[sel].sum(0) / (b - a)); covs.append(dist["C"][sel].sum(0) / (b - a))
    return dict(resolution=float(prm["resolution"]), dims=dims, min_b=min_b, cell_ids=np.array(ids, np.int64),
                counts=np.array(counts, np.int64), means=np.array(means).reshape(-1, 3), covs=np.array(covs).reshape(-1, 3, 3),
                n_points=int((cell >= 0).sum()), dist=dist)


def prepare_source(xyz32, prm, dist=None):
    xyz32 = np.ascontiguousarray(np.asarray(xyz32, np.float32).reshape(-1, 3))
    dist = dist or distributions(xyz32, prm)
    return dict(x=xyz32.astype(np.float64), C=dist["C"], ok=dist["nbr"][:, 0] >= 0, dist=dist)


# ---- SE(3) ---------------------------------------------------------------------------------------------------------------------
def skew(a):
    return np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])


def se3_exp(delta):
    """4 x 4 of delta = (omega, v): R = I + A K + B K^2, t = (I + B K + C K^2) v with A = sin th / th, B = (1 - cos th) / th^2,
    C = (th - sin th) / th^3; below th = 0.05 the three are their series up to th^6"""
    om, v = np.asarray(delta[:3], np.float64), np.asarray(delta[3:], np.float64)
    th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]
    th = np.sqrt(th2)
    if th < 0.05:
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0))
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0))
        Cc = 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0 * (1.0 - th2 / 72.0))
    else:
        A, B, Cc = np.sin(th) / th, (1.0 - np.cos(th)) / th2, (th - np.sin(th)) / (th2 * th)
    K = skew(om)
    K2 = K @ K
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + A * K + B * K2
    T[:3, 3] = (np.eye(3) + B * K + Cc * K2) @ v
    return T


def transform_points(T, x64):
    R, t = T[:3, :3], T[:3, 3]
    return ((R[:, 0] * x64[:, 0:1] + R[:, 1] * x64[:, 1:2]) + R[:, 2] * x64[:, 2:3]) + t


# ---- 3. one linearisation ------------------------------------------------------------------------------------------------------
def _table(tgt):
    if "_table" not in tgt:
        tab = np.full(int(np.prod(tgt["dims"])), -1, np.int64)
        tab[tgt["cell_ids"]] = np.arange(len(tgt["cell_ids"]))
        tgt["_table"] = tab
    return tgt["_table"]


def find_pairs(tgt, src, T):
    """(source index, voxel index) of every pair at T, and the smallest distance of a transformed point to a voxel face (metres)"""
    xt = transform_points(T, src["x"])
    s = xt * (1.0 / tgt["resolution"])
    f = np.floor(s) - tgt["min_b"]
    with np.errstate(invalid="ignore"):
        inb = src["ok"] & (f >= 0).all(1) & (f < tgt["dims"]).all(1)
    idx = np.flatnonzero(inb)
    c = f[idx].astype(np.int64)
    v = _table(tgt)[c[:, 0] + c[:, 1] * tgt["dims"][0] + c[:, 2] * tgt["dims"][0] * tgt["dims"][1]]
    keep = v >= 0
    fin = src["ok"] & np.isfinite(s).all(1)
    face = float(np.min(np.abs(s[fin] - np.round(s[fin]))) * tgt["resolution"]) if fin.any() else np.inf
    return idx[keep], v[keep], face


def _empty():
    return dict(out=np.zeros(28), abs=np.zeros(28), n_pairs=0, face=np.inf)


def linearize_loops(tgt, src, T, with_hessian=True):
    R, t = T[:3, :3], T[:3, 3]
    ev = _empty()
    tab = _table(tgt)
    inv = 1.0 / tgt["resolution"]
    for a in range(len(src["x"])):
        if not src["ok"][a]:
            continue
        p = src["x"][a]
        x = ((R[:, 0] * p[0] + R[:, 1] * p[1]) + R[:, 2] * p[2]) + t
        f = np.floor(x * inv) - tgt["min_b"]
        if not ((f >= 0).all() and (f < tgt["dims"]).all()):
            continue
        v = tab[int(f[0]) + int(f[1]) * tgt["dims"][0] + int(f[2]) * tgt["dims"][0] * tgt["dims"][1]]
        if v < 0:
            continue
        d = tgt["means"][v] - x
        M = np.linalg.inv(tgt["covs"][v] + R @ src["C"][a] @ R.T)
        w = np.sqrt(float(tgt["counts"][v]))
        J = np.hstack([skew(x), -np.eye(3)])
        Md = M @ d
        ev["n_pairs"] += 1
        ev["out"][0] += w * (d @ Md); ev["abs"][0] += abs(w * (d @ Md))
        for i in range(6):
            ev["out"][1 + i] += w * (J[:, i] @ Md); ev["abs"][1 + i] += abs(w * (J[:, i] @ Md))
        if with_hessian:
            MJ = M @ J
            for q, (i, j) in enumerate(TRI):
                ev["out"][7 + q] += w * (J[:, i] @ MJ[:, j]); ev["abs"][7 + q] += abs(w * (J[:, i] @ MJ[:, j]))
    return ev


def linearize(tgt, src, T, with_hessian=True, pairs=None, R_lin=None, means=None):
    """the vector form of linearize_loops.  pairs: a fixed (source index, voxel index) set; R_lin: the rotation M is formed with
    (default: T's); means: the pairs' target means (default: the voxels') — for the tests that difference e"""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    ev = _empty()
    if pairs is None:
        pi, vi, ev["face"] = find_pairs(tgt, src, T)
    else:
        pi, vi = pairs
    ev["n_pairs"] = len(pi)
    if len(pi) == 0:
        return ev
    x = transform_points(T, src["x"][pi])
    mu = tgt["means"][vi] if means is None else means
    d = mu - x
    Rl = R if R_lin is None else R_lin
    S = tgt["covs"][vi] + np.einsum("ij,njk,lk->nil", Rl, src["C"][pi], Rl)
    M = np.linalg.inv(S)
    w = np.sqrt(tgt["counts"][vi].astype(np.float64))
    J = np.zeros((len(pi), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = -x[:, 2], x[:, 1]
    J[:, 1, 0], J[:, 1, 2] = x[:, 2], -x[:, 0]
    J[:, 2, 0], J[:, 2, 1] = -x[:, 1], x[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    Md = np.einsum("nij,nj->ni", M, d)
    e = w * np.einsum("ni,ni->n", d, Md)
    ev["out"][0], ev["abs"][0] = e.sum(), np.abs(e).sum()
    bt = w[:, None] * np.einsum("nia,ni->na", J, Md)
    ev["out"][1:7], ev["abs"][1:7] = bt.sum(0), np.abs(bt).sum(0)
    if with_hessian:
        MJ = np.einsum("nij,nja->nia", M, J)
        Ht = w[:, None, None] * np.einsum("nia,nib->nab", J, MJ)
        for q, (i, j) in enumerate(TRI):
            ev["out"][7 + q], ev["abs"][7 + q] = Ht[:, i, j].sum(), np.abs(Ht[:, i, j]).sum()
    return ev


def unpack(out):
    H = np.zeros((6, 6))
    for q, (i, j) in enumerate(TRI):
        H[i, j] = H[j, i] = out[7 + q]
    return out[0], np.array(out[1:7]), H


# ---- 4. the optimiser ----------------------------------------------------------------------------------------------------------
class Margins:
    """the smallest margins by which the comparisons of a run were decided"""

    def __init__(self):
        self.rho = self.conv = self.face = np.inf
        self.log = []                # what became of every trial
        self.lams = []               # the damping of every trial


def delta_converged(delta, prm, mg=None):
    E = se3_exp(delta)
    r = np.abs(E[:3, :3] - np.eye(3)).max() / prm["rotation_epsilon"]
    t = np.abs(E[:3, 3]).max() / prm["transformation_epsilon"]
    if mg is not None:
        mg.conv = min(mg.conv, abs(r - 1.0), abs(t - 1.0))
    return bool(r < 1.0 and t < 1.0)


def solve_damped(H, b, lam):
    """delta of (H + lam I) delta = -b, or None if the matrix is not finite or not positive definite"""
    A = H + lam * np.eye(6)
    if not (np.isfinite(A).all() and np.isfinite(b).all()):
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    y = np.linalg.solve(L, -b)
    d = np.linalg.solve(L.T, y)
    return d if np.isfinite(d).all() else None


def lm_optimise(lin, err, T0, prm, mg=None):
    """the LM loop on any least-squares problem: lin(T) -> (e, b, H, n_pairs), err(T) -> (e, n_pairs).  Returns the result dict."""
    mg = mg or Margins()
    T = np.array(T0, np.float64)
    e, b, H, pairs = lin(T)
    res = dict(converged=0, iters=0, n_evals=1, n_rejected=0)
    lam = 0.0
    if pairs > 0:
        lam = prm["lm_init_lambda_factor"] * np.abs(np.diag(H)).max()
        for it in range(prm["max_iters"]):
            if it:
                e, b, H, pairs = lin(T)
                res["n_evals"] += 1
            res["iters"] = it + 1
            nu, stop, accepted = 2.0, False, False
            for _ in range(prm["lm_max_iterations"]):
                mg.lams.append(lam)
                delta = solve_damped(H, b, lam)
                if delta is None:
                    mg.log.append("not positive definite")
                    stop = True
                    break
                Tn = se3_exp(delta) @ T
                en, pairs = err(Tn)
                res["n_evals"] += 1
                den = float(delta @ (lam * delta - b))
                with np.errstate(invalid="ignore", divide="ignore"):
                    rho = np.float64(e - en) / np.float64(den)
                mg.rho = min(mg.rho, abs(e - en) / e if e > 0 else np.inf)
                dconv = delta_converged(delta, prm, mg)
                if not rho >= 0:
                    res["n_rejected"] += 1
                    if dconv:
                        mg.log.append("rejected while converged")
                        res["converged"], stop = 1, True
                        break
                    mg.log.append("rejected")
                    lam, nu = nu * lam, 2.0 * nu
                    continue
                T, e = Tn, en
                lam = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)
                accepted = True
                mg.log.append("accepted")
                if dconv:
                    res["converged"], stop = 1, True
                break
            if not accepted and not stop:
                mg.log.append("trials exhausted")
                stop = True
            if stop:
                break
    res.update(T=T, error=float(e), lam=float(lam), n_pairs_last=int(pairs))
    return res


def align(tgt, src, prm, guess=None, mg=None):
    """the whole registration of a prepared source (prepare_source) against a target (build_target)"""
    mg = mg or Margins()
    T0 = np.eye(4) if guess is None else np.asarray(guess, np.float32).reshape(4, 4).astype(np.float64)

    def lin(T):
        ev = linearize(tgt, src, T, True)
        mg.face = min(mg.face, ev["face"])
        e, b, H = unpack(ev["out"])
        return e, b, H, ev["n_pairs"]

    def err(T):
        ev = linearize(tgt, src, T, False)
        mg.face = min(mg.face, ev["face"])
        return ev["out"][0], ev["n_pairs"]

    r = lm_optimise(lin, err, T0, prm, mg)
    r.update(margin_rho=mg.rho, margin_conv=mg.conv, margin_face=mg.face, log=list(mg.log))
    return r


# ---- the scenes of the tests ---------------------------------------------------------------------------------------------------
def scene(scan_seed=1000, trans=0.3, rot_deg=2.0):
    """(target xyz float32, source xyz float32 — not subsampled, guess 4x4 float32, T_true 4x4 float64)"""
    from lisreg import synth
    c = synth.make_case(h=16, w=225, m_points=300000, scan_seed=scan_seed, local_radius=12, trans=trans, rot_deg=rot_deg, pose_xy=(32, 31))
    tgt = np.concatenate([synth.pcl_xyz(c["tgt_corner"]), synth.pcl_xyz(c["tgt_surf"])])
    src = np.concatenate([synth.pcl_xyz(c["src_corner"]), synth.pcl_xyz(c["src_surf"])])
    return (np.ascontiguousarray(tgt, np.float32), np.ascontiguousarray(src, np.float32), synth.pose_matrix(c["T_init"]).astype(np.float32),
            synth.pose_matrix(c["T_true"].astype(np.float64)))


PLANTED_K = 20


def planted_cloud(n_base=600):
    """(xyz float32, groups): a random base cloud in a 6 m box, a cluster of 10 points 30 m from everything else, a coplanar patch, a
    collinear run, 25 identical points and NaN points, shuffled.  groups: name -> indices into xyz"""
    rng = np.random.default_rng(2771)
    parts = dict(base=rng.uniform(0.0, 6.0, (n_base, 3)),
                 cluster=np.array([36.0, 0.0, 1.0]) + rng.uniform(0.0, 1.0, (10, 3)) * np.array([0.4, 6.0, 0.4]),
                 coplanar=np.c_[8.0 + rng.uniform(0, 1.5, (60, 2)), np.full(60, 2.5)],
                 collinear=np.c_[np.linspace(0.0, 3.0, 40), np.full(40, -3.0), np.full(40, 1.25)],
                 identical=np.repeat(np.array([[3.5, 9.5, 0.75]]), 25, 0),
                 nan=np.array([[np.nan] * 3, [np.nan, 1.0, 1.0], [1.0, np.nan, 1.0], [2.0, 2.0, np.nan], [np.nan] * 3]))
    xyz = np.concatenate(list(parts.values())).astype(np.float32)
    tag = np.concatenate([np.full(len(v), i) for i, v in enumerate(parts.values())])
    perm = rng.permutation(len(xyz))
    xyz, tag = np.ascontiguousarray(xyz[perm]), tag[perm]
    return xyz, {name: np.flatnonzero(tag == i) for i, name in enumerate(parts)}


def small_cloud(n, seed=5):
    """n random points (the sizes 20, 21, 64, 65 of the tests)"""
    return np.random.default_rng(seed + n).uniform(-2.0, 2.0, (n, 3)).astype(np.float32)


# ---- the expected outputs kept in tests/golden/vgicp (tests/golden/make_golden_vgicp.py writes them) --------------------------------
LIN_SIZES = (1, 63, 64, 65, 257, 0)                # source sizes of the one-linearisation cases; 0: the whole source
ALIGN_CASES = ((1000, 0.3, 2.0, 5.0e-4), (1001, 0.5, 3.0, 5.0e-4), (1005, 0.5, 3.0, 5.0e-4), (1000, 0.3, 2.0, 0.01))   # seed, trans, rot_deg, transformation_epsilon


def lin_poses(guess, T_true):
    """the guess, the true pose, a pose 100 m away (no pairs)"""
    far = np.array(T_true, np.float64)
    far[0, 3] += 100.0
    return np.stack([np.asarray(guess, np.float64), np.asarray(T_true, np.float64), far])


_WORLD = {}


def world(seed=1000, trans=0.3, rot_deg=2.0):
    """scene + restatement target + prepared source of one seed, made once per process"""
    key = (seed, trans, rot_deg)
    if key not in _WORLD:
        tgt, src, guess, T_true = scene(seed, trans, rot_deg)
        prm = params()
        tkey = ("target", tgt.tobytes())                       # the seeds of the tests share one submap: its restatement is made once
        if tkey not in _WORLD:
            _WORLD[tkey] = build_target(tgt, prm)
        _WORLD[key] = dict(tgt=tgt, src=src, guess=guess, T_true=T_true, T=_WORLD[tkey], S=prepare_source(src, prm))
    return _WORLD[key]


def golden_cases():
    out = {}
    W = world()
    T, S = W["T"], W["S"]
    out["scene_dims"] = np.r_[T["dims"], len(T["cell_ids"]), T["n_points"]].astype(np.int64)
    out["scene_cell_ids"], out["scene_counts"] = T["cell_ids"].astype(np.int32), T["counts"].astype(np.int32)
    out["scene_means"], out["scene_cov6"] = T["means"][::8], cov6(T["covs"])[::8]
    out["scene_nbr_sum"] = T["dist"]["nbr"].sum(1).astype(np.int64)[::8]          # a check sum of every eighth neighbour row
    poses = lin_poses(W["guess"], W["T_true"])
    out["lin_T"] = poses
    sums, absum, pairs = [], [], []
    for P in poses:
        for n in LIN_SIZES:
            m = n or len(W["src"])
            Sm = dict(x=S["x"][:m], C=S["C"][:m], ok=S["ok"][:m])
            for hess in (1, 0):
                ev = linearize(T, Sm, P, bool(hess))
                sums.append(ev["out"]); absum.append(ev["abs"]); pairs.append(ev["n_pairs"])
    out["lin_out"], out["lin_abs"], out["lin_pairs"] = np.array(sums), np.array(absum), np.array(pairs, np.int64)
    rows, Ts, fig = [], [], []
    for seed, trans, rot, eps in ALIGN_CASES:
        Wk = world(seed, trans, rot)
        r = align(Wk["T"], Wk["S"], params(transformation_epsilon=eps), Wk["guess"])
        et, er = pose_error(r["T"], Wk["T_true"])
        et0, er0 = pose_error(Wk["guess"], Wk["T_true"])
        rows.append([r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], len(Wk["src"])])
        Ts.append(r["T"])
        fig.append([r["error"], r["lam"], r["margin_rho"], r["margin_conv"], r["margin_face"], float(Wk["T"]["dist"]["gap"].min()),
                    float(Wk["S"]["dist"]["gap"].min()), et, er, et0, er0])
    out["align_counts"], out["align_T"], out["align_fig"] = np.array(rows, np.int64), np.array(Ts), np.array(fig)
    return out
