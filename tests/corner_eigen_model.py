"""CPU model of the corner fit's eigen-solver (no GPU): the production cyclic Jacobi of `eigen_sym3` (lisreg_assoc.hip) and the closed
form that replaces it, both restated in numpy float32 and run on the 5-neighbour scatter matrices the default benchmark's corner
queries meet: `synth.make_submap` corner target, `synth.make_scan` corner points under `perturb_pose` and under the true pose,
brute-force 5-NN with the `sqDist[4] < tau` test.
    python tests/corner_eigen_model.py [--scans 8] [--points 200000] [--h 64] [--w 1800] [--tau 1.0] [--line-ratio 3.0]
It prints
  * the distribution of Jacobi sweeps per neighbourhood and of the maximum over 64 consecutive queries (a wavefront runs as many
    sweeps as its slowest lane);
  * for the closed form: the share of lanes / of 64-lane groups handed back to the Jacobi (guard band, residual certificate), the
    accept-flag disagreements with the Jacobi with and without the guard band, the angle between the two directions, the eigenvalue
    errors of both against numpy's float64 `eigh` in units of the bound, and that `corner_eval`'s (la, lb, lc, ld2) do not depend on
    the direction's sign.
The float32 restatements round every operation on its own (no FMA contraction, IEEE division and square root instead of the 1-ulp
hardware forms), so they are the device code up to last bits, which is what a count over many neighbourhoods needs.

The closed form and its error bound (u = 2^-24, T = trace):
  1. lambda ~ largest root of the characteristic polynomial of the trace-shifted, scaled matrix (A - T/3 I) / p, 6 p^2 = |A - T/3 I|_F^2:
     y^3 - 3 y - 2 r = 0 with r = det / 2 in [-1, 1], root 2 cos(acos(r) / 3) in [1, 2]; Newton from 1 + sqrt((1 + r) / 2) (exact at both
     ends, 3.2e-2 off at worst) is at 1.6e-3, 5e-6, 8e-11 after one, two, three steps (two steps: 2.7e-7 for r >= 0, where every accepted neighbourhood of ratio 3
     lies (r >= 0.54); the 5e-6 is met near r = -1, l0 ~ l1); lambda = T/3 + p y;
  2. v = the largest of the three cross products of rows of A - lambda I, normalised; u1 = the first row of that pair, normalised;
     u2 = v x u1: Q = [v u1 u2] is orthonormal up to eta = |Q^T Q - I| <= 32 u + 2 |v . u1|;
  3. rho = v.Av, B = [u1 u2]^T A [u1 u2] (2 x 2, eigenvalues mu1 >= mu2 from the stable (mean +- hypot) form), c = [u1 u2]^T A v.
  Q^T A Q = diag(rho, B) + offdiag(c), so by Ostrowski (eta T), Weyl (|c|), the rounding of the nine 3-term dot products
  (|F|_2 <= 3 * 12 u T) and of the 2 x 2 solve (4 u T), the sorted {rho, mu1, mu2} are within
        delta_cf = (eta + 36 u + 4 u) T + |c|   <=   kDeltaCf u T   with |v . u1| <= 8 u (+ 3 u of its own rounding) and max |c_i| <= 45 u T (|c| <= 64 u T)
  of A's eigenvalues — whatever step 1 and 2 did: a poor lambda or v shows in |c| and |v . u1|, and the lane goes to the Jacobi.
  The Jacobi's own eigenvalues carry <= kDeltaJacobi u T (18 rotations of <= 6 u |A| backward error each, plus the 3e-30 it may leave).
  The accept test l0 > r l1 is therefore the Jacobi's wherever |rho - r mu1| > (1 + r) (kDeltaCf + kDeltaJacobi + 1) u T.
"""
import argparse
import os
import sys

import numpy as np

f32 = np.float32
U = 2.0 ** -24
K_E = 8.0                     # bar on |v . u1| in units of u
K_C = 64.0                    # bar on |c| in units of u T ...
K_CI = 45.0                   # ... asked of either component (45 sqrt(2) < 64: no squares, which could underflow)
K_DELTA_CF = 32 + 2 * (K_E + 3) + 36 + 4 + K_C          # = 158
K_DELTA_JACOBI = 128.0
K_GUARD = K_DELTA_CF + K_DELTA_JACOBI + 1                # in units of (1 + r) u T
K_GAP = 0.125                 # accepted lanes need rho - mu1 >= K_GAP T for the direction (sin(angle) <= |c| / gap)
NEWTON_STEPS = 2


def scatter(nb):
    """centroid and the six scatter sums / 5 of nb[n, 5, 3] float32, in corner_model's order of operations"""
    nb = nb.astype(f32)
    c = np.zeros((len(nb), 3), f32)
    for j in range(5):
        c = c + nb[:, j]
    c = c * f32(0.2)
    a = np.zeros((6, len(nb)), f32)
    for j in range(5):
        d = nb[:, j] - c
        for k, (p, q) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            a[k] = a[k] + d[:, p] * d[:, q]
    return c, a * f32(0.2)


def _hypot(a, b):
    a, b = np.abs(a), np.abs(b)
    mx, mn = np.maximum(a, b), np.minimum(a, b)
    with np.errstate(all="ignore"):
        r = mn * (f32(1) / mx)
        return np.where(mx > 0, mx * np.sqrt(f32(1) + r * r), f32(0)).astype(f32)


def jacobi(a):
    """the production branch of eigen_sym3 on a[6, n]: (l0, l1, v[n, 3], sweeps[n])"""
    a11, a12, a13, a22, a23, a33 = (x.copy() for x in a.astype(f32))
    n = a.shape[1]
    w = [a11, a22, a33]
    off = {(0, 1): a12, (0, 2): a13, (1, 2): a23}
    V = [[np.full(n, f32(i == j), f32) for j in range(3)] for i in range(3)]
    sweeps = np.zeros(n, np.int64)
    for _ in range(6):
        live = np.abs(off[0, 1]) + np.abs(off[0, 2]) + np.abs(off[1, 2]) > f32(1e-30)
        if not live.any():
            break
        sweeps += live
        for (k, l), (o1, o2) in (((0, 1), ((0, 2), (1, 2))), ((0, 2), ((0, 1), (1, 2))), ((1, 2), ((0, 1), (0, 2)))):
            p = off[k, l]
            m = live & (np.abs(p) > 0)
            y = (w[l] - w[k]) * f32(0.5)
            with np.errstate(all="ignore"):
                t = np.abs(y) + _hypot(p, y)
                s = _hypot(p, t)
                c = t * (f32(1) / s)
                s = p * (f32(1) / s)
                t = p * (f32(1) / t) * p
            s = np.where(y < 0, -s, s); t = np.where(y < 0, -t, t)

            def rot(x0, x1):
                return np.where(m, x0 * c - x1 * s, x0), np.where(m, x0 * s + x1 * c, x1)
            off[k, l] = np.where(m, f32(0), p)
            w[k] = np.where(m, w[k] - t, w[k]); w[l] = np.where(m, w[l] + t, w[l])
            off[o1], off[o2] = rot(off[o1], off[o2])
            for j in range(3):
                V[k][j], V[l][j] = rot(V[k][j], V[l][j])
    e0, e1, e2 = w
    v = np.stack(V[0], 1)
    sw = e1 > e0
    e0, e1 = np.where(sw, e1, e0), np.where(sw, e0, e1); v = np.where(sw[:, None], np.stack(V[1], 1), v)
    sw = e2 > e0
    e0, e2 = np.where(sw, e2, e0), np.where(sw, e0, e2); v = np.where(sw[:, None], np.stack(V[2], 1), v)
    return e0.astype(f32), np.maximum(e1, e2).astype(f32), v.astype(f32), sweeps


def closed_form(a, ratio, newton_steps=NEWTON_STEPS):
    """the closed form on a[6, n]: dict(rho, mu1, mu2, v, accept, fallback, guard (fallback by the guard band alone), resid, e)"""
    a11, a12, a13, a22, a23, a33 = a.astype(f32)
    ratio = f32(ratio)
    with np.errstate(all="ignore"):
        T = a11 + a22 + a33
        qs = T * f32(1.0 / 3.0)
        d1, d2, d3 = a11 - qs, a22 - qs, a33 - qs
        p2 = ((d1 * d1 + d2 * d2 + d3 * d3) + f32(2) * (a12 * a12 + a13 * a13 + a23 * a23)) * f32(1.0 / 6.0)
        det = d1 * (d2 * d3 - a23 * a23) - a12 * (a12 * d3 - a13 * a23) + a13 * (a12 * a23 - a13 * d2)
        p = np.sqrt(p2)
        rr = det * (f32(0.5) / (p2 * p))
        y = f32(1) + np.sqrt(np.maximum(f32(0.5) + f32(0.5) * rr, f32(0)))
        for _ in range(newton_steps):
            y2 = y * y
            y = y - ((y2 - f32(3)) * y - f32(2) * rr) * (f32(1) / (f32(3) * y2 - f32(3)))
        x = qs + p * y
        r = [np.stack([a11 - x, a12, a13], 1), np.stack([a12, a22 - x, a23], 1), np.stack([a13, a23, a33 - x], 1)]
        cr = [np.cross(r[0], r[1]).astype(f32), np.cross(r[0], r[2]).astype(f32), np.cross(r[1], r[2]).astype(f32)]
        nn = [np.sum(c * c, 1, dtype=f32) for c in cr]
        v, n2, ra = cr[0], nn[0], r[0]
        pick = nn[1] > n2
        v = np.where(pick[:, None], cr[1], v); n2 = np.where(pick, nn[1], n2)
        pick = nn[2] > n2
        v = np.where(pick[:, None], cr[2], v); n2 = np.where(pick, nn[2], n2); ra = np.where(pick[:, None], r[1], ra)
        v = v * (f32(1) / np.sqrt(n2))[:, None]
        u1 = ra * (f32(1) / np.sqrt(np.sum(ra * ra, 1, dtype=f32)))[:, None]
        u2 = np.cross(v, u1).astype(f32)

        def mul(z):
            return np.stack([a11 * z[:, 0] + a12 * z[:, 1] + a13 * z[:, 2], a12 * z[:, 0] + a22 * z[:, 1] + a23 * z[:, 2],
                             a13 * z[:, 0] + a23 * z[:, 1] + a33 * z[:, 2]], 1).astype(f32)

        def dot(p, q):
            return (p[:, 0] * q[:, 0] + p[:, 1] * q[:, 1] + p[:, 2] * q[:, 2]).astype(f32)
        Av, Au1, Au2 = mul(v), mul(u1), mul(u2)
        rho, b11, b12, b22 = dot(v, Av), dot(u1, Au1), dot(u2, Au1), dot(u2, Au2)
        cc1, cc2, e = dot(u1, Av), dot(u2, Av), dot(v, u1)
        mean, h = (b11 + b22) * f32(0.5), (b11 - b22) * f32(0.5)
        s = np.sqrt(h * h + b12 * b12)
        mu1, mu2 = mean + s, mean - s
        top = np.maximum(rho, mu1); second = np.maximum(np.minimum(rho, mu1), mu2)
        uT = f32(U) * T
        certified = (np.maximum(np.abs(cc1), np.abs(cc2)) <= f32(K_CI) * uT) & (np.abs(e) <= f32(K_E * U)) & (T >= f32(1e-12)) & (T <= f32(1e12))
        margin = top - ratio * second
        band = (f32(1) + ratio) * f32(K_GUARD) * uT
        clear = np.abs(margin) > band
        accept = margin > 0
        direction_ok = (rho - mu1 >= f32(K_GAP) * T)               # only asked of accepted lanes (it implies rho is the top)
        fallback = ~(certified & clear & (~accept | direction_ok))
    return dict(rho=top, mu1=second, v=v, accept=accept, fallback=fallback, guard=certified & ~clear,
                resid=np.sqrt(cc1.astype(np.float64) ** 2 + cc2.astype(np.float64) ** 2), e=e, T=T)


def corner_eval(c, v, q):
    """(la, lb, lc, ld2) of corner_eval for centroids c, directions v, queries q (float32, the double promotions as in the kernel)"""
    p1 = (c.astype(np.float64) + 0.1 * v.astype(np.float64)).astype(f32); p2 = (c.astype(np.float64) - 0.1 * v.astype(np.float64)).astype(f32)
    x0, y0, z0 = q.astype(f32).T; x1, y1, z1 = p1.T; x2, y2, z2 = p2.T
    m11 = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)
    m22 = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)
    m33 = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)
    a012 = np.sqrt(m11 * m11 + m22 * m22 + m33 * m33)
    l12 = np.sqrt((x1 - x2) ** 2 + (y1 - y2) ** 2 + (z1 - z2) ** 2)
    inv = f32(1) / (a012 * l12)
    return np.stack([((y1 - y2) * m11 + (z1 - z2) * m22) * inv, -((x1 - x2) * m11 - (z1 - z2) * m33) * inv,
                     -((x1 - x2) * m22 + (y1 - y2) * m33) * inv, a012 / l12], 1)


def eigh64(a):
    a11, a12, a13, a22, a23, a33 = a.astype(np.float64)
    M = np.stack([np.stack([a11, a12, a13], 1), np.stack([a12, a22, a23], 1), np.stack([a13, a23, a33], 1)], 1)
    w, V = np.linalg.eigh(M)
    return w[:, 2], w[:, 1], V[:, :, 2]


def knn5(tgt, q, tau, chunk=2048):
    """brute-force 5-NN of q in tgt (float64 distances): indices [n, 5] ascending, and which queries have sqDist[4] < tau"""
    idx = np.zeros((len(q), 5), np.int64); ok = np.zeros(len(q), bool)
    t2 = (tgt * tgt).sum(1)
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        d = (qq * qq).sum(1)[:, None] - 2.0 * qq @ tgt.T + t2[None]
        part = np.argpartition(d, 5, axis=1)[:, :5]
        dd = np.take_along_axis(d, part, 1); o = np.argsort(dd, 1)
        idx[s:s + chunk] = np.take_along_axis(part, o, 1); ok[s:s + chunk] = np.take_along_axis(dd, o, 1)[:, 4] < tau
    return idx, ok


def report(name, nb, q, ratio, found):
    c, a = scatter(nb)
    l0, l1, vj, sweeps = jacobi(a)
    acc_j = l0 > f32(ratio) * l1
    n = len(nb)
    print(f"{name}: {n} neighbourhoods, Jacobi accepts {acc_j.mean():.4f}")
    print("    Jacobi sweeps per neighbourhood:", {int(k): round(float((sweeps == k).mean()), 4) for k in np.unique(sweeps)}, f"mean {sweeps.mean():.3f}")
    g = sweeps[: n // 64 * 64].reshape(-1, 64).max(1)
    print("    maximum over 64 consecutive queries:", {int(k): round(float((g == k).mean()), 4) for k in np.unique(g)}, f"mean {g.mean():.3f}")
    for steps in (1, 2, 3, 4):
        r = closed_form(a, ratio, steps)
        fb = r["fallback"] & found; gf = fb[: n // 64 * 64].reshape(-1, 64).any(1)
        print(f"    closed form, {steps} Newton steps: lanes to the Jacobi {fb.mean():.5f} (guard band alone {r['guard'].mean():.5f}), 64-lane groups with one {gf.mean():.4f}")
    r = closed_form(a, ratio)
    fb = r["fallback"] & found                   # (lanes without five neighbours never reach the fit)
    diff_raw = int((r["accept"] != acc_j).sum()); diff_guard = int(((r["accept"] != acc_j) & ~fb).sum())
    print(f"    accept flag differs from the Jacobi's: {diff_raw} of {n} without the guard band, {diff_guard} with it")
    keep = ~fb & acc_j & found
    ang = np.arcsin(np.clip(np.linalg.norm(np.cross(r["v"][keep].astype(np.float64), vj[keep].astype(np.float64)), axis=1), 0, 1))
    if keep.any():
        print(f"    direction (accepted, closed-form lanes): angle to the Jacobi's max {ang.max():.2e} rad, median {np.median(ang):.1e}")
    t0, t1, vt = eigh64(a)
    uT = U * r["T"].astype(np.float64)
    ok = ~fb & found
    for nm, x0, x1, msk in (("closed form", r["rho"], r["mu1"], ok), ("Jacobi", l0, l1, found)):
        e0 = (np.abs(x0 - t0) / np.where(uT > 0, uT, 1))[msk]; e1 = (np.abs(x1 - t1) / np.where(uT > 0, uT, 1))[msk]
        if msk.any():
            print(f"    {nm}: |l0 - eigh64| max {e0.max():.1f} u T, |l1 - eigh64| max {e1.max():.1f} u T   (bounds {K_DELTA_CF:.0f} / {K_DELTA_JACOBI:.0f})")
    ca = corner_eval(c[keep], r["v"][keep], q[keep]); cb = corner_eval(c[keep], -r["v"][keep], q[keep])
    print(f"    corner_eval with v and with -v: max |difference| of (la, lb, lc, ld2) = {np.abs(ca - cb).max() if keep.any() else 0.0:.2e}")
    return sweeps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=8); ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--h", type=int, default=64); ap.add_argument("--w", type=int, default=1800)
    ap.add_argument("--tau", type=float, default=1.0); ap.add_argument("--line-ratio", type=float, default=3.0)
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lis-slam_amd"))
    from lisreg import synth
    tgt = synth.pcl_xyz(synth.make_submap(a.points)[0])
    print(f"corner target: {len(tgt)} points")
    for name, at_truth in (("initial (perturbed) pose", False), ("true pose", True)):
        nbs, qs, oks = [], [], []
        for i in range(a.scans):
            s = synth.make_scan(a.h, a.w, 1000 + i)
            T = s["T_true"] if at_truth else synth.perturb_pose(s["T_true"], np.random.default_rng(1000 + i + 7919))
            M = synth.pose_matrix(np.asarray(T, np.float64))
            q = (synth.pcl_xyz(s["corner"]).astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(f32)
            idx, ok = knn5(tgt.astype(np.float64), q.astype(np.float64), a.tau)
            # queries without five neighbours stay in (their lanes are idle: zero sweeps), as a zero matrix
            nb = tgt[idx]; nb[~ok] = 0
            nbs.append(nb); qs.append(q); oks.append(ok)
        report(name, np.concatenate(nbs), np.concatenate(qs), a.line_ratio, np.concatenate(oks))


if __name__ == "__main__":
    main()
