"""The definition of lisreg_vgicp_params.neighbor_search: the voxel neighbourhoods DIRECT1 / DIRECT7 / DIRECT27 of VGICP,
restated in numpy float64 over tests/vgicp_ref.py, which this file imports as R and does not change.  Only the PAIRING is written here;
the terms of a pair (linearize(..., pairs=...)), the Levenberg-Marquardt loop (lm_optimise), se3_exp, build_target and prepare_source are
R's.

For a finite source point a with x' = R a + t (double, R's operation order):
  * f = floor(x' * (1 / resolution)) - min_b, in double;
  * the offsets of a mode are the (dx, dy, dz) in {-1, 0, 1}^3 it keeps: DIRECT1 only (0, 0, 0); DIRECT7 those with
    |dx| + |dy| + |dz| <= 1; DIRECT27 all of them.  They are walked in ascending cell id (dz outermost, dx innermost);
  * every offset is tested on its own: g = f + o must satisfy 0 <= g < dims component-wise, in the floating-point domain before any
    integer is made of it.  So a point whose own cell lies one cell outside the grid still pairs with the voxels inside it, and a point
    with a non-finite f pairs with nothing;
  * every g whose table entry is a voxel is one pair (a, voxel), with exactly DIRECT1's terms for that voxel: d = mu_v - x',
    M = (C_v + R C_a R^T)^-1, weight sqrt(N_v), J = [skew(x') | -I];
  * the 28 sums run over all pairs, and the pair count and n_pairs_last count pairs, not points;
  * the LM loop, the convergence test, the "no pair at the guess" rule and the fitness score of the batch do not change.

fast_gicp's source is not available to this project (as for the rest of VGICP, §7k), so two readings cannot be verified against it:
  * the order of the offsets, which decides only the last bits of a sum;
  * whether fast_gicp skips a point whose own cell holds no voxel.  Here it does not: every offset stands on its own.

  python tests/vgicp_nb_ref.py --write      writes tests/golden/vgicp/vgicp_nb_cases.npz"""
import os
import sys

import numpy as np

if __name__ == "__main__":                      # run as a script: the package lies next to tests/ (under pytest, tests/conftest.py says so)
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lis-slam_amd"))

import vgicp_ref as R  # noqa: E402

MODES = (1, 7, 27)
NB_MODES = (7, 27)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgicp", "vgicp_nb_cases.npz")
COARSE = (1001, 2.0, 10.0)                     # the coarse guess of §7w: DIRECT1 "converges" 2.4 m from the truth, DIRECT27 2.5 mm


def offsets(mode):
    """[m, 3] integer offsets (dx, dy, dz) of a mode in ascending cell id"""
    if mode not in MODES:
        raise ValueError("neighbor_search is none of 1, 7, 27")
    keep = {1: 0, 7: 1, 27: 3}[mode]
    return np.array([(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if abs(dx) + abs(dy) + abs(dz) <= keep],
                    np.int64).reshape(-1, 3)


def _cells(tgt, src, T):
    xt = R.transform_points(T, src["x"])
    s = xt * (1.0 / tgt["resolution"])
    return s, np.floor(s) - tgt["min_b"]


def find_pairs(tgt, src, T, mode):
    """(source index, voxel index) of every pair at T, by source point and within a point in the order of offsets(mode), and the
    smallest distance of a transformed point to a voxel face (metres), as R.find_pairs"""
    s, f = _cells(tgt, src, T)
    tab, dims = R._table(tgt), tgt["dims"]
    pi, vi, rank = [], [], []
    for k, o in enumerate(offsets(mode)):
        g = f + o
        with np.errstate(invalid="ignore"):
            inb = src["ok"] & (g >= 0).all(1) & (g < dims).all(1)
        idx = np.flatnonzero(inb)
        c = g[idx].astype(np.int64)
        v = tab[c[:, 0] + c[:, 1] * dims[0] + c[:, 2] * dims[0] * dims[1]]
        keep = v >= 0
        pi.append(idx[keep]); vi.append(v[keep]); rank.append(np.full(int(keep.sum()), k))
    pi, vi, rank = np.concatenate(pi), np.concatenate(vi), np.concatenate(rank)
    order = np.lexsort((rank, pi))
    fin = src["ok"] & np.isfinite(s).all(1)
    face = float(np.min(np.abs(s[fin] - np.round(s[fin]))) * tgt["resolution"]) if fin.any() else np.inf
    return pi[order], vi[order], face


def find_pairs_loops(tgt, src, T, mode):
    """the loop form of find_pairs: (source indices, voxel indices)"""
    Rm, t = T[:3, :3], T[:3, 3]
    tab, dims, inv = R._table(tgt), tgt["dims"], 1.0 / tgt["resolution"]
    pi, vi = [], []
    for a in range(len(src["x"])):
        if not src["ok"][a]:
            continue
        p = src["x"][a]
        x = ((Rm[:, 0] * p[0] + Rm[:, 1] * p[1]) + Rm[:, 2] * p[2]) + t
        f = np.floor(x * inv) - tgt["min_b"]
        for o in offsets(mode):
            g = f + o
            if not ((g >= 0).all() and (g < dims).all()):
                continue
            v = tab[int(g[0]) + int(g[1]) * dims[0] + int(g[2]) * dims[0] * dims[1]]
            if v >= 0:
                pi.append(a); vi.append(int(v))
    return np.array(pi, np.int64), np.array(vi, np.int64)


def linearize(tgt, src, T, mode, with_hessian=True):
    """the vector form: R.linearize over the pairs of the mode"""
    T = np.asarray(T, np.float64)
    pi, vi, face = find_pairs(tgt, src, T, mode)
    ev = R.linearize(tgt, src, T, with_hessian, pairs=(pi, vi))
    ev["face"] = face
    return ev


def linearize_loops(tgt, src, T, mode, with_hessian=True):
    """the loop form: the terms of R.linearize_loops, pair by pair"""
    T = np.asarray(T, np.float64)
    Rm, t = T[:3, :3], T[:3, 3]
    ev = R._empty()
    for a, v in zip(*find_pairs_loops(tgt, src, T, mode)):
        p = src["x"][a]
        x = ((Rm[:, 0] * p[0] + Rm[:, 1] * p[1]) + Rm[:, 2] * p[2]) + t
        d = tgt["means"][v] - x
        M = np.linalg.inv(tgt["covs"][v] + Rm @ src["C"][a] @ Rm.T)
        w = np.sqrt(float(tgt["counts"][v]))
        J = np.hstack([R.skew(x), -np.eye(3)])
        Md = M @ d
        ev["n_pairs"] += 1
        ev["out"][0] += w * (d @ Md); ev["abs"][0] += abs(w * (d @ Md))
        for i in range(6):
            ev["out"][1 + i] += w * (J[:, i] @ Md); ev["abs"][1 + i] += abs(w * (J[:, i] @ Md))
        if with_hessian:
            MJ = M @ J
            for q, (i, j) in enumerate(R.TRI):
                ev["out"][7 + q] += w * (J[:, i] @ MJ[:, j]); ev["abs"][7 + q] += abs(w * (J[:, i] @ MJ[:, j]))
    return ev


def align(tgt, src, prm, mode, guess=None, mg=None):
    """R.align with the pairs of the mode"""
    mg = mg or R.Margins()
    T0 = np.eye(4) if guess is None else np.asarray(guess, np.float32).reshape(4, 4).astype(np.float64)

    def lin(T):
        ev = linearize(tgt, src, T, mode, True)
        mg.face = min(mg.face, ev["face"])
        e, b, H = R.unpack(ev["out"])
        return e, b, H, ev["n_pairs"]

    def err(T):
        ev = linearize(tgt, src, T, mode, False)
        mg.face = min(mg.face, ev["face"])
        return ev["out"][0], ev["n_pairs"]

    r = R.lm_optimise(lin, err, T0, prm, mg)
    r.update(margin_rho=mg.rho, margin_conv=mg.conv, margin_face=mg.face, log=list(mg.log))
    return r


def census(tgt, src, T, mode):
    """what the neighbour walk meets at T: points (finite, with a finite cell) whose own cell is outside the grid but that pair; points
    whose own cell is inside and that have an offset out of range; pairs"""
    _, f = _cells(tgt, src, T)
    with np.errstate(invalid="ignore"):
        fin = src["ok"] & np.isfinite(f).all(1)
        own_in = fin & (f >= 0).all(1) & (f < tgt["dims"]).all(1)
        clipped = np.zeros(len(f), bool)
        for o in offsets(mode):
            g = f + o
            clipped |= ~((g >= 0).all(1) & (g < tgt["dims"]).all(1))
    pi, _, _ = find_pairs(tgt, src, T, mode)
    has = np.zeros(len(f), bool)
    has[pi] = True
    return dict(outside_pairing=int((fin & ~own_in & has).sum()), inside_clipped=int((own_in & clipped).sum()), pairs=len(pi),
                outside=int((fin & ~own_in).sum()))


# ---- the cases of the tests ------------------------------------------------------------------------------------------------------
def lin_source(src, n):
    """the source of a one-linearisation case of R.LIN_SIZES: the first n points (0: all).  n = 1 is the one-pair construction of
    tests/test_vgicp.py: a source of k points of which one lies on the map, the others 200 m above it"""
    if n == 1:
        one = src[:R.PLANTED_K].copy()
        one[1:] = one[0] + (one[1:] - one[0]) * np.float32([50, 50, 1]) + np.float32([0, 0, 200])
        return one
    return src[: n or len(src)]


_CUT = {}


def lin_sources():
    """size -> (xyz, prepared source) of the scene's source cut to R.LIN_SIZES, made once per process"""
    if not _CUT:
        W = R.world()
        for n in R.LIN_SIZES:
            xyz = lin_source(W["src"], n)
            _CUT[n] = (xyz, W["S"] if n == 0 else R.prepare_source(xyz, R.params()))
    return _CUT


def border_poses(tgt, src, T):
    """name -> pose: T moved by whole cells along one axis so that the farthest layer of the source's cells lies exactly one cell
    (`+x1`, `-x1`, ...) or two cells (`+x2`, ...) outside the target's grid beyond that face.  Chosen from min_b, dims and the extent of
    the source's cells at T alone."""
    _, f = _cells(tgt, src, np.asarray(T, np.float64))
    f = f[src["ok"] & np.isfinite(f).all(1)]
    lo, hi = f.min(0), f.max(0)
    out = {}
    for ax, name in enumerate("xyz"):
        for sign, cells in (("+", tgt["dims"][ax] - hi[ax]), ("-", -1.0 - lo[ax])):
            for far in (1, 2):
                P = np.array(T, np.float64)
                P[ax, 3] += (cells + (far - 1) * (1 if sign == "+" else -1)) * tgt["resolution"]
                out[f"{sign}{name}{far}"] = P
    return out


_FLAT = {}


def flat_world():
    """a target one voxel thick along z (dims[2] == 1): the points of the scene's target in the layer of cells that holds most of them"""
    if "T" not in _FLAT:
        W = R.world()
        cell, dims, _ = R.NR.voxel_cells(W["tgt"], 1.0)
        kz = cell // (int(dims[0]) * int(dims[1]))
        layer = np.bincount(kz[cell >= 0]).argmax()
        xyz = np.ascontiguousarray(W["tgt"][(cell >= 0) & (kz == layer)])
        _FLAT.update(tgt=xyz, T=R.build_target(xyz, R.params()))
    return _FLAT


def nan_source():
    """the first 257 points of the scene's source with NaN coordinates planted: (xyz, prepared source)"""
    if "nan" not in _FLAT:
        xyz = R.world()["src"][:257].copy()
        xyz[5, 0] = xyz[64, 1] = xyz[200, 2] = np.nan
        xyz[130] = np.nan
        _FLAT["nan"] = (xyz, R.prepare_source(xyz, R.params()))
    return _FLAT["nan"]


def far_pose(T, metres=200.0):
    P = np.array(T, np.float64)
    P[0, 3] += metres
    return P


def align_case(k):
    """(world, params) of alignment case k: R.ALIGN_CASES, then COARSE"""
    if k < len(R.ALIGN_CASES):
        seed, trans, rot, eps = R.ALIGN_CASES[k]
        return R.world(seed, trans, rot), R.params(transformation_epsilon=eps)
    return R.world(*COARSE), R.params()


ALIGN_RUNS = tuple((k, m) for k in range(len(R.ALIGN_CASES)) for m in NB_MODES) + ((len(R.ALIGN_CASES), 27),)     # (case, mode)


def golden_cases():
    out = {}
    W = R.world()
    poses = R.lin_poses(W["guess"], W["T_true"])
    out["lin_T"] = poses
    sums, absum, pairs = [], [], []
    for mode in NB_MODES:
        for P in poses:
            for n in R.LIN_SIZES:
                for hess in (1, 0):
                    ev = linearize(W["T"], lin_sources()[n][1], P, mode, bool(hess))
                    sums.append(ev["out"]); absum.append(ev["abs"]); pairs.append(ev["n_pairs"])
    out["lin_out"], out["lin_abs"], out["lin_pairs"] = np.array(sums), np.array(absum), np.array(pairs, np.int64)
    rows, Ts, fig = [], [], []
    for k, mode in ALIGN_RUNS:
        Wk, prm = align_case(k)
        r = align(Wk["T"], Wk["S"], prm, mode, Wk["guess"])
        et, er = R.pose_error(r["T"], Wk["T_true"])
        rows.append([r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], len(Wk["src"]), k, mode])
        Ts.append(r["T"])
        fig.append([r["error"], r["lam"], r["margin_rho"], r["margin_conv"], r["margin_face"], et, er])
    out["align_counts"], out["align_T"], out["align_fig"] = np.array(rows, np.int64), np.array(Ts), np.array(fig)
    return out


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        np.savez_compressed(GOLDEN, **golden_cases())
        print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
    else:
        print(__doc__)
