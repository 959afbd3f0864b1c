"""The definition of lisreg_fgicp_* : FastGICP registration (generalised ICP with fast_gicp's Levenberg-Marquardt optimiser), restated in
numpy float64.

select_registration_method("FAST_GICP") (src/core/registration.cpp:157-166 of the reference: FastGICP, transformation epsilon 0.01, 50
iterations, max correspondence distance 5, correspondence randomness 20) is the one verifier of the fast_gicp family that tests/vgicp_ref.py
does not cover.  fast_gicp's source is not available to this project, so this file restates FastGICP + LsqRegistration from the papers and
from memory, on top of what vgicp_ref already defines (distributions, SE(3), the LM loop).  What is written here is the definition the GPU
code is tested against — it is not "fast_gicp's".

Readings picked (each one a possible departure from the fast_gicp a user has installed), besides those vgicp_ref lists for the
distributions, the perturbation and the optimiser:
  * target: every finite point gets its C_b from vgicp_ref.distributions with the target's own k_correspondences and plane_epsilon; NaN
    points are no points: never a correspondent, in no pair;
  * correspondence at T: the source point is transformed in DOUBLE from its float coordinates, x' = ((R0 a0 + R1 a1) + R2 a2) + t; its
    correspondent is the finite target point with the smallest ((dx dx + dy dy) + dz dz), in double from the float target coordinates,
    ties to the lower index in the caller's cloud (fast_gicp transforms in FLOAT and asks a kd-tree, whose tie order is unspecified and
    whose distances are float);
  * it is a pair iff that squared distance is < max_correspondence_distance^2 — strict, as fast_gicp's
    k_sq_dists[0] < corr_dist_threshold_^2 is remembered;
  * per pair: M = (C_b + R C_a R^T)^-1 of the 3 x 3, d = b - x', J = [skew(x') | -I]; e = sum d^T M d, b = sum J^T M d, H = sum J^T M J;
    no weight;
  * a linearisation searches and forms the pairs and their M; an error evaluation inside the LM trial loop REUSES the pairs and the M of
    the last linearisation and recomputes only x', d and e (what fast_gicp's compute_error is remembered to do with correspondences_ /
    mahalanobis_) — so the trial's model and its error share one pair set, rho is well defined, and n_pairs_last is the pair count of
    the last linearisation;
  * the optimiser is vgicp_ref.lm_optimise, unchanged;
  * a source without a pair at the guess: converged = 0, iters = 0, n_evals = 1, the guess;
  * defaults, kind 0: the reference's commented block plus fast_gicp's defaults as remembered; kind 1: the same with
    max_correspondence_distance = FLT_MAX, fast_gicp's own default (its square is finite in double: no special case).

Margins of a run, next to vgicp_ref's rho and conv: nn_gap, the smallest relative gap (d2 - d1) / d2 between the best and the second-best
squared distance over every search (0 if d2 == 0), and cut_gap, the smallest |d1 - max^2| / max^2.

The brute-force search, chunked, IS the definition; a kd-tree appears only in tests/test_fgicp_ref.py, as an independent check."""
import numpy as np

import vgicp_ref as V
from vgicp_ref import (distributions, prepare_source, se3_exp, transform_points, lm_optimise, scene, planted_cloud, small_cloud,  # noqa: F401
                       pose_error, skew, unpack, TRI)

FLT_MAX = 3.4028234663852886e38
DEFAULTS = dict(max_correspondence_distance=5.0, transformation_epsilon=0.01, rotation_epsilon=2.0e-3, lm_init_lambda_factor=1.0e-9,
                plane_epsilon=1.0e-3, k_correspondences=20, max_iters=50, lm_max_iterations=10)


def params(kind=0, **kw):
    p = dict(DEFAULTS)
    if kind == 1:
        p["max_correspondence_distance"] = FLT_MAX
    elif kind != 0:
        raise ValueError("kind")
    p.update(kw)
    return p


class Margins(V.Margins):
    """vgicp_ref's margins plus those of the searches"""

    def __init__(self):
        super().__init__()
        self.nn_gap = self.cut_gap = np.inf


# ---- 1. the target ---------------------------------------------------------------------------------------------------------------
def build_target(xyz32, prm, dist=None):
    xyz32 = np.ascontiguousarray(np.asarray(xyz32, np.float32).reshape(-1, 3))
    dist = dist or distributions(xyz32, prm)
    ok = dist["nbr"][:, 0] >= 0
    return dict(x=xyz32.astype(np.float64), C=dist["C"], ok=ok, idx=np.flatnonzero(ok), n_points=int(ok.sum()), dist=dist)


# ---- 2. the correspondences ------------------------------------------------------------------------------------------------------
def _gaps(d1, d2, max2):
    nn = (d2 - d1) / d2 if d2 > 0 else 0.0
    return nn, abs(d1 - max2) / max2


def search_loops(tgt, xt, max_d):
    """(index [n] in the caller's target cloud or -1, squared distance [n] or NaN, nn_gap [n], cut_gap [n]) of the queries xt [n, 3]
    (double); a query with a NaN coordinate has no correspondent and its gaps are inf"""
    max2 = float(max_d) * float(max_d)
    idx, sq = np.full(len(xt), -1, np.int64), np.full(len(xt), np.nan)
    nn_gap, cut_gap = np.full(len(xt), np.inf), np.full(len(xt), np.inf)
    for i, q in enumerate(xt):
        if np.isnan(q).any():
            continue
        best, bj, second = np.inf, -1, np.inf
        for j in tgt["idx"]:
            b = tgt["x"][j]
            dx, dy, dz = b[0] - q[0], b[1] - q[1], b[2] - q[2]
            d = (dx * dx + dy * dy) + dz * dz
            if d < best:                                      # strict: among equal distances the first (lowest) index stays
                best, bj, second = d, j, best
            elif d < second:
                second = d
        nn_gap[i], cut_gap[i] = _gaps(best, second, max2)
        if best < max2:
            idx[i], sq[i] = bj, best
    return idx, sq, nn_gap, cut_gap


def search(tgt, xt, max_d, chunk=256):
    """the vector form of search_loops"""
    max2 = float(max_d) * float(max_d)
    idx, sq = np.full(len(xt), -1, np.int64), np.full(len(xt), np.nan)
    nn_gap, cut_gap = np.full(len(xt), np.inf), np.full(len(xt), np.inf)
    b = tgt["x"][tgt["idx"]]
    rows = np.flatnonzero(~np.isnan(xt).any(1))
    for a in range(0, len(rows), chunk):
        rr = rows[a:a + chunk]
        q = xt[rr]
        dx, dy, dz = b[None, :, 0] - q[:, 0:1], b[None, :, 1] - q[:, 1:2], b[None, :, 2] - q[:, 2:3]
        d = (dx * dx + dy * dy) + dz * dz
        j = np.argmin(d, axis=1)                              # the first of equal minima: the lowest index (tgt["idx"] ascends)
        two = np.partition(d, 1, axis=1)[:, :2]
        d1, d2 = two[:, 0], two[:, 1]
        with np.errstate(invalid="ignore", divide="ignore"):
            nn_gap[rr] = np.where(d2 > 0, (d2 - d1) / np.where(d2 > 0, d2, 1.0), 0.0)
        cut_gap[rr] = np.abs(d1 - max2) / max2
        hit = d1 < max2
        idx[rr[hit]], sq[rr[hit]] = tgt["idx"][j[hit]], d1[hit]
    return idx, sq, nn_gap, cut_gap


def find_pairs(tgt, src, T, prm, mg=None, loops=False):
    """the pair set of a linearisation at T: dict(pi source indices, ti target indices (caller's), M [p, 3, 3]; idx, sq, row_nn, row_cut by
    source point; nn_gap, cut_gap = the smallest of the rows')"""
    T = np.asarray(T, np.float64)
    R = T[:3, :3]
    xt = transform_points(T, src["x"])
    xt[~src["ok"]] = np.nan
    idx, sq, row_nn, row_cut = (search_loops if loops else search)(tgt, xt, prm["max_correspondence_distance"])
    g1, g2 = float(row_nn.min()), float(row_cut.min())
    if mg is not None:
        mg.nn_gap, mg.cut_gap = min(mg.nn_gap, g1), min(mg.cut_gap, g2)
    pi = np.flatnonzero(idx >= 0)
    ti = idx[pi]
    if loops:
        M = np.array([np.linalg.inv(tgt["C"][t] + R @ src["C"][p] @ R.T) for p, t in zip(pi, ti)]).reshape(-1, 3, 3)
    else:
        M = np.linalg.inv(tgt["C"][ti] + np.einsum("ij,njk,lk->nil", R, src["C"][pi], R)) if len(pi) else np.zeros((0, 3, 3))
    return dict(pi=pi, ti=ti, M=M, idx=idx, sq=sq, row_nn=row_nn, row_cut=row_cut, nn_gap=g1, cut_gap=g2)


# ---- 3. the sums over a pair set ---------------------------------------------------------------------------------------------------
def _empty():
    return dict(out=np.zeros(28), abs=np.zeros(28), n_pairs=0)


def sums_loops(tgt, src, pairs, T, with_hessian=True):
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    ev = _empty()
    for p, j, M in zip(pairs["pi"], pairs["ti"], pairs["M"]):
        a = src["x"][p]
        x = ((R[:, 0] * a[0] + R[:, 1] * a[1]) + R[:, 2] * a[2]) + t
        d = tgt["x"][j] - x
        J = np.hstack([skew(x), -np.eye(3)])
        Md = M @ d
        ev["n_pairs"] += 1
        ev["out"][0] += d @ Md; ev["abs"][0] += abs(d @ Md)
        for i in range(6):
            ev["out"][1 + i] += J[:, i] @ Md; ev["abs"][1 + i] += abs(J[:, i] @ Md)
        if with_hessian:
            MJ = M @ J
            for q, (i, k) in enumerate(TRI):
                ev["out"][7 + q] += J[:, i] @ MJ[:, k]; ev["abs"][7 + q] += abs(J[:, i] @ MJ[:, k])
    return ev


def sums(tgt, src, pairs, T, with_hessian=True, per_pair=False):
    """the vector form of sums_loops: x', d and the 28 sums at T over the pair set and the M it carries"""
    T = np.asarray(T, np.float64)
    ev = _empty()
    pi, ti, M = pairs["pi"], pairs["ti"], pairs["M"]
    ev["n_pairs"] = len(pi)
    if len(pi) == 0:
        return ev
    x = transform_points(T, src["x"][pi])
    d = tgt["x"][ti] - x
    J = np.zeros((len(pi), 3, 6))
    J[:, 0, 1], J[:, 0, 2] = -x[:, 2], x[:, 1]
    J[:, 1, 0], J[:, 1, 2] = x[:, 2], -x[:, 0]
    J[:, 2, 0], J[:, 2, 1] = -x[:, 1], x[:, 0]
    J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
    Md = np.einsum("nij,nj->ni", M, d)
    e = np.einsum("ni,ni->n", d, Md)
    ev["out"][0], ev["abs"][0] = e.sum(), np.abs(e).sum()
    bt = np.einsum("nia,ni->na", J, Md)
    ev["out"][1:7], ev["abs"][1:7] = bt.sum(0), np.abs(bt).sum(0)
    if with_hessian:
        MJ = np.einsum("nij,nja->nia", M, J)
        Ht = np.einsum("nia,nib->nab", J, MJ)
        for q, (i, k) in enumerate(TRI):
            ev["out"][7 + q], ev["abs"][7 + q] = Ht[:, i, k].sum(), np.abs(Ht[:, i, k]).sum()
        if per_pair:
            ev["H_terms"] = Ht
    return ev


def linearize(tgt, src, T_pairs, prm, with_hessian=True, T_eval=None, mg=None, loops=False):
    """pairs and M from T_pairs, the sums at T_eval (None: T_pairs).  The returned dict also carries the pair set ("pairs")."""
    pairs = find_pairs(tgt, src, T_pairs, prm, mg, loops)
    ev = (sums_loops if loops else sums)(tgt, src, pairs, T_pairs if T_eval is None else T_eval, with_hessian)
    ev["pairs"] = pairs
    return ev


# ---- 4. the whole registration -----------------------------------------------------------------------------------------------------
def align(tgt, src, prm, guess=None, mg=None):
    """a prepared source (vgicp_ref.prepare_source) against a target (build_target)"""
    mg = mg or Margins()
    T0 = np.eye(4) if guess is None else np.asarray(guess, np.float32).reshape(4, 4).astype(np.float64)
    held = {}

    def lin(T):
        ev = linearize(tgt, src, T, prm, True, mg=mg)
        held["pairs"] = ev["pairs"]
        e, b, H = unpack(ev["out"])
        return e, b, H, ev["n_pairs"]

    def err(T):
        ev = sums(tgt, src, held["pairs"], T, False)
        return ev["out"][0], ev["n_pairs"]

    r = lm_optimise(lin, err, T0, prm, mg)
    r.update(margin_rho=mg.rho, margin_conv=mg.conv, margin_nn=mg.nn_gap, margin_cut=mg.cut_gap, log=list(mg.log))
    return r


# ---- the expected outputs kept in tests/golden/fgicp (tests/golden/make_golden_fgicp.py writes them) ---------------------------------
# seed, trans, rot_deg, transformation_epsilon: vgicp_ref.ALIGN_CASES with the first case's seed replaced — with seed 1000 and epsilon 5e-4
# the last step's rho is decided by 2.4e-7 of the error, under the 1e-6 bar of the tests (tests/test_fgicp_ref.py asserts the bars)
ALIGN_CASES = ((1006, 0.3, 2.0, 5.0e-4),) + tuple(V.ALIGN_CASES[1:])
lin_poses = V.lin_poses
_WORLD = {}


def world(seed=1000, trans=0.3, rot_deg=2.0):
    """vgicp_ref's scene of one seed (clouds, guess, truth, prepared source) with this file's target, made once per process"""
    key = (seed, trans, rot_deg)
    if key not in _WORLD:
        W = V.world(seed, trans, rot_deg)
        tkey = ("target", W["tgt"].tobytes())
        if tkey not in _WORLD:
            _WORLD[tkey] = build_target(W["tgt"], params(), W["T"]["dist"])
        _WORLD[key] = dict(tgt=W["tgt"], src=W["src"], guess=W["guess"], T_true=W["T_true"], T=_WORLD[tkey], S=W["S"])
    return _WORLD[key]


def golden_cases():
    out = {}
    W = world()
    T, S, prm = W["T"], W["S"], params()
    poses = lin_poses(W["guess"], W["T_true"])
    out["lin_T"] = poses
    idx, sums_, absum, npairs, gaps = [], [], [], [], []
    # the guess, the truth, the pose without a pair; then pairs from the guess with the sums at the truth
    for Tp, Te in ((poses[0], None), (poses[1], None), (poses[2], None), (poses[0], poses[1])):
        for hess in (1, 0):
            ev = linearize(T, S, Tp, prm, bool(hess), T_eval=Te)
            sums_.append(ev["out"]); absum.append(ev["abs"]); npairs.append(ev["n_pairs"])
        idx.append(ev["pairs"]["idx"][::8])
        gaps.append([ev["pairs"]["nn_gap"], ev["pairs"]["cut_gap"]])
    out["corr_idx"] = np.array(idx[:3], np.int32)             # every eighth correspondence row of the three poses
    out["corr_gaps"] = np.array(gaps[:3])
    out["lin_out"], out["lin_abs"], out["lin_pairs"] = np.array(sums_), np.array(absum), np.array(npairs, np.int64)
    rows, Ts, fig = [], [], []
    for seed, trans, rot, eps in ALIGN_CASES:
        Wk = world(seed, trans, rot)
        r = align(Wk["T"], Wk["S"], params(transformation_epsilon=eps), Wk["guess"])
        et, er = pose_error(r["T"], Wk["T_true"])
        et0, er0 = pose_error(Wk["guess"], Wk["T_true"])
        rows.append([r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], len(Wk["src"])])
        Ts.append(r["T"])
        fig.append([r["error"], r["lam"], r["margin_rho"], r["margin_conv"], r["margin_nn"], r["margin_cut"], et, er, et0, er0])
    out["align_counts"], out["align_T"], out["align_fig"] = np.array(rows, np.int64), np.array(Ts), np.array(fig)
    return out
