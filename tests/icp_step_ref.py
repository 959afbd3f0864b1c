"""Planted clouds and a float64 reference for ONE step of point-to-point ICP (tests/test_icp_step.py).  No library code is imported.

Every coordinate is a multiple of GRID = 2^-10 m below 256 m, so with an identity guess (or a signed axis permutation with an integer
translation) the first iteration's 17 sums — count, sum p, sum q, sum q p^T, sum d^2 — are integers in units of 2^-10 / 2^-20: they are
formed here in integer arithmetic, they fit a double's 53 bits, and any summation order on any machine gives the same bits.  The target
sits on a shuffled lattice (pitch >= 2 m, jitter <= 0.25 m), source point i is target point pi(i) minus a small planted offset, so the
nearest neighbour of every source point is known and is nearest by a margin that rounding cannot bridge.

state codes: 0 not converged, 1 iterations, 2 transform, 3 absolute MSE, 4 relative MSE, 5 no correspondences (PCL's order of exits)."""
from fractions import Fraction

import numpy as np
from scipy.spatial import cKDTree

GRID = 2.0 ** -10
LIMIT = 256.0
MARGIN = 0.25                                  # second-nearest minus nearest distance, at least
DBL_MAX = np.finfo(np.float64).max
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
f32 = np.float32


def to_grid(x):
    return np.round(np.asarray(x, np.float64) / GRID) * GRID


def assert_dyadic(*clouds):
    for c in clouds:
        c = np.asarray(c, np.float64)
        ok = np.isfinite(c)
        k = c[ok] / GRID
        assert np.array_equal(k, np.round(k)), "a coordinate is no multiple of 2^-10"
        assert np.all(np.abs(c[ok]) < LIMIT), "a coordinate of 256 m or more"
        assert np.array_equal(c[ok], c[ok].astype(f32).astype(np.float64))


def rot(axis, deg):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = np.deg2rad(deg)
    return np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * (K @ K)


def rot_angle(R):
    R = np.asarray(R, np.float64)
    v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    return float(np.arctan2(np.linalg.norm(v), (np.trace(R) - 1) / 2))


def pose_diff(A, B):
    A, B = np.asarray(A, np.float64), np.asarray(B, np.float64)
    return rot_angle(A[:3, :3].T @ B[:3, :3]), float(np.abs(A[:3, 3] - B[:3, 3]).max())


# ---------------------------------------------------------------- pairs, exact totals, Kabsch
def pairs(tgt, cur, cap2, margin=MARGIN, tree=None):
    """nearest target of every finite row of cur within sqrt(cap2) (d^2 <= cap2 pairs); asserts the nearest is nearest by `margin`"""
    tgt = np.asarray(tgt, np.float64); cur = np.asarray(cur, np.float64)
    fin = np.isfinite(cur).all(1)
    idx = np.full(len(cur), -1); d2 = np.full(len(cur), np.inf)
    if fin.any() and len(tgt):
        if tree is None:
            tree = cKDTree(tgt)
        k = min(2, tree.n)
        d, j = tree.query(cur[fin], k=k)
        d, j = d.reshape(-1, k), j.reshape(-1, k)
        if k == 2 and margin is not None:
            near = d[:, 0] ** 2 <= 1.01 * cap2                          # beyond the gate nothing pairs, whichever point is nearest
            gap = d[near, 1] - d[near, 0]
            assert np.all(gap >= margin), f"nearest-neighbour margin {float(gap.min()):.4f} m"
        idx[fin] = j[:, 0]
        diff = cur[fin] - tree.data[j[:, 0]]
        d2[fin] = (diff * diff).sum(1)                                  # exact on the grid (multiples of 2^-20 below 2^33)
    ok = d2 <= cap2
    return idx, d2, ok


def exact_totals(p, q):
    """the 17 sums of the pairs (p source, q target), formed in integers: exact, and below 2^53 so they are exact doubles too"""
    P = np.round(np.asarray(p, np.float64) / GRID).astype(np.int64); Q = np.round(np.asarray(q, np.float64) / GRID).astype(np.int64)
    assert np.array_equal(P * GRID, p) and np.array_equal(Q * GRID, q)
    n = len(P)
    sp, sq = P.sum(0), Q.sum(0)
    sqp = Q.T @ P                                                       # |entry| < n * 2^36 <= 2^52 for n <= 2^16
    D = P - Q
    sd2 = int((D * D).sum())
    big = max(int(np.abs(sqp).max()) if n else 0, sd2)
    assert n <= 1 << 16 and big < 1 << 53
    return dict(n=n, sp=[int(v) for v in sp], sq=[int(v) for v in sq], sqp=[[int(v) for v in r] for r in sqp], sd2=sd2,
                bits=big.bit_length())


def totals_as_doubles(tot):
    """count, sum p, sum q, sum q p^T (row-major), sum d^2 in metres — every one exact"""
    return np.array([tot["n"]] + [v * GRID for v in tot["sp"]] + [v * GRID for v in tot["sq"]]
                    + [v * GRID * GRID for r in tot["sqp"] for v in r] + [tot["sd2"] * GRID * GRID])


def mse_of(tot):
    """sum d^2 / count, one correctly rounded division"""
    return float(Fraction(tot["sd2"], tot["n"] << 20))


def kabsch_from_totals(tot):
    """float64 Umeyama (no scale) from exact totals: sigma = (n sum q p^T - sum q sum p^T) / n^2 is rounded once per entry"""
    n = tot["n"]
    sig = np.array([[float(Fraction(n * tot["sqp"][r][c] - tot["sq"][r] * tot["sp"][c], n * n << 20)) for c in range(3)] for r in range(3)])
    ms = np.array([float(Fraction(v, n << 10)) for v in tot["sp"]]); md = np.array([float(Fraction(v, n << 10)) for v in tot["sq"]])
    U, S, Vt = np.linalg.svd(sig)
    s = np.sign(np.linalg.det(U) * np.linalg.det(Vt))
    R = U @ np.diag([1.0, 1.0, s]) @ Vt
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = md - R @ ms
    return T, S, float(s), sig


def first_step(tgt, src, max_corr, guess=None, margin=MARGIN):
    """the float64 answer of one ICP step from `guess` (identity, or a signed permutation with an integer translation: exact)"""
    tgt = np.asarray(tgt, np.float64); src = np.asarray(src, np.float64)
    G = np.eye(4) if guess is None else np.asarray(guess, np.float64)
    cur = src @ G[:3, :3].T + G[:3, 3]
    assert_dyadic(tgt, cur)
    idx, d2, ok = pairs(tgt, cur, max_corr * max_corr, margin)
    out = dict(idx=idx, ok=ok, n_corr=int(ok.sum()), cur=cur, guess=G)
    if out["n_corr"] < 3:
        out.update(state=NO_CORRESPONDENCES, T=G.copy(), Tm=None)
        return out
    tot = exact_totals(cur[ok], tgt[idx[ok]])
    Tm, S, s, sig = kabsch_from_totals(tot)
    out.update(tot=tot, Tm=Tm, T=Tm @ G, S=S, s=s, sigma=sig, mse=mse_of(tot), state=None)
    return out


def fitness(tgt, src, T, work=np.float64):
    """getFitnessScore: mean squared nearest distance of the source under T (every finite point, no gate), in double; work = float32
    forms the moved points in float32 first, as pcl::transformPointCloud does"""
    tgt = np.asarray(tgt, np.float64); src = np.asarray(src, np.float64)
    src = src[np.isfinite(src).all(1)].astype(work)
    T = np.asarray(T, work)
    w = [((T[r, 0] * src[:, 0] + T[r, 1] * src[:, 1]) + T[r, 2] * src[:, 2]) + T[r, 3] for r in range(3)]
    d, _ = cKDTree(tgt).query(np.stack(w, 1).astype(np.float64))
    return float((d * d).mean())


# ---------------------------------------------------------------- the loop (pcl::IterativeClosestPoint + DefaultConvergenceCriteria)
def _far(value, threshold, what, rel=1e-3):
    assert abs(value - threshold) >= rel * abs(threshold), f"borderline {what}: {value!r} against {threshold!r}"


def icp_loop(tgt, src, max_corr=10.0, max_iters=30, eps_t=1e-4, eps_mse=1e-4, prev_mse=DBL_MAX, guess=None, work=np.float64, fma=False,
             margin=MARGIN, exact=()):
    """Plain numpy ICP.  work = float64: all double.  work = float32: the working copy, the step Tm and the accumulated F are rounded to
    float32 as a float implementation holds them, the transform is evaluated in float32 — with every product rounded (fma False) or
    fused into the following addition (fma True).  Pairs come from a cKDTree in double; every nearest-neighbour margin and every
    stopping quantity is asserted clear of its decision (names in `exact` are planted on a threshold and are not).
    Returns dict(T, iters, state, converged, prev_mse, n_corr, trace)."""
    tgt = np.asarray(tgt, np.float64)
    tree = cKDTree(tgt)
    cap2 = max_corr * max_corr
    F = (np.eye(4) if guess is None else np.asarray(guess, np.float64)).astype(work)

    def move(M, x):
        if work == np.float64:
            return x @ M[:3, :3].T + M[:3, 3]
        M = M.astype(f32); x = x.astype(f32)
        cols = []
        for r in range(3):
            if fma:
                a = M[r, 0].astype(np.float64) * x[:, 0]
                a = (M[r, 1].astype(np.float64) * x[:, 1] + a).astype(f32)
                a = (M[r, 2].astype(np.float64) * x[:, 2] + a).astype(f32)
                cols.append((a.astype(np.float64) + M[r, 3]).astype(f32))
            else:
                cols.append(((M[r, 0] * x[:, 0] + M[r, 1] * x[:, 1]) + M[r, 2] * x[:, 2]) + M[r, 3])
        return np.stack(cols, 1)

    fin = np.isfinite(np.asarray(src, np.float64)).all(1)
    cur = move(F, np.asarray(src, np.float64)[fin].astype(work))
    iters, trace, n_corr = 0, [], 0
    while True:
        c64 = cur.astype(np.float64)
        idx, d2, ok = pairs(tgt, c64, cap2, margin, tree)
        if "gate" not in exact:
            assert not np.any(np.abs(d2[np.isfinite(d2)] - cap2) < 1e-3 * cap2), "borderline gate"
        n_corr = int(ok.sum())
        if n_corr < 3:
            return dict(T=F.astype(np.float64), iters=iters, state=NO_CORRESPONDENCES, converged=False, prev_mse=prev_mse, n_corr=n_corr, trace=trace)
        p, q = c64[ok], tgt[idx[ok]]
        ms, md = p.mean(0), q.mean(0)
        sig = (q - md).T @ (p - ms) / n_corr
        U, S, Vt = np.linalg.svd(sig)
        R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))]) @ Vt
        Tm = np.eye(4); Tm[:3, :3] = R; Tm[:3, 3] = md - R @ ms
        Tm = Tm.astype(work)
        cur = move(Tm, cur)
        F = (Tm @ F).astype(work) if work == np.float64 else (Tm.astype(f32) @ F.astype(f32))
        iters += 1
        mse = float(d2[ok].sum() / n_corr)
        Td = Tm.astype(np.float64)
        cos_angle = 0.5 * (np.trace(Td[:3, :3]) - 1.0); tr2 = float(Td[:3, 3] @ Td[:3, 3])
        trace.append(dict(n_corr=n_corr, S=S, mse=mse, cos_angle=cos_angle, tr2=tr2, prev_mse=prev_mse))
        done = lambda st: dict(T=F.astype(np.float64), iters=iters, state=st, converged=True, prev_mse=prev_mse, n_corr=n_corr, trace=trace)
        if iters >= max_iters:
            return done(ITERATIONS)
        if "transform" not in exact:
            _far(1.0 - cos_angle, eps_t, "rotation test"); _far(tr2, eps_t, "translation test")
        if cos_angle >= 1.0 - eps_t and tr2 <= eps_t:
            return done(TRANSFORM)
        diff = abs(mse - prev_mse)
        if "abs" not in exact:
            _far(diff, 1e-12, "absolute MSE test")
        if diff < 1e-12:
            return done(ABS_MSE)
        if "rel" not in exact and prev_mse > 0:
            _far(diff / prev_mse, eps_mse, "relative MSE test")
        if prev_mse > 0 and diff / prev_mse < eps_mse:
            return done(REL_MSE)
        prev_mse = mse


# ---------------------------------------------------------------- generators
def lattice(dims, pitch, rng, jitter=0.25, basis=None):
    """all sites of a dims[0] x dims[1] x dims[2] lattice centred on the origin, shuffled, each moved by a grid jitter; basis (3 integer
    row vectors) maps lattice coordinates to space (default: the axes)"""
    dims = np.asarray(dims)
    ijk = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3)
    ijk = ijk[rng.permutation(len(ijk))]
    c = (ijk - (dims - 1) // 2) * float(pitch)
    if jitter > 0:
        c = c + to_grid(rng.uniform(-jitter, jitter, c.shape)) * (dims > 1)
    if basis is not None:
        c = c @ np.asarray(basis, np.float64)
    return c


def plant(n, seed, shape="cube", motion=(3.0, (0.25, -0.125, 0.375)), holes=None, max_corr=10.0, order=(0, 1, 2), pitch=None):
    """A planted case: dict(tgt, src, pi, ans) with ans = first_step(tgt, src, max_corr) — and the assertions of this module made.

    shape   cube: n sites of the smallest cube lattice that holds them, pitch 4 m.  box: extents (2, 8, 32) m along the axes `order`,
            pitch 2 m (n = 170).  product: the full 3 x 5 x 9 lattice without jitter, axes `order`, offsets 0.25 sign(x) per axis — sigma
            is exactly diagonal.  plane_z / plane_xy / plane_111: z = const, x = y, x + y + z = 0, offsets in the plane (rank 2).
            line_x / line_111: points and offsets on a line (rank 1).  slab_mirror: |z| <= 0.25 m, target = source mirrored in z.
    motion  (angle in degrees, translation): offset d = to_grid((R - I) x + t) of target point x, R about a fixed oblique axis (the normal
            for a plane).  The angle is cut so that |d| stays inside what the lattice's pitch leaves for a 0.25 m margin.
    holes   dict(far=indices, nan=indices): source points pushed beyond max_corr / given a NaN coordinate."""
    rng = np.random.default_rng(seed)
    ang, t = motion
    t = np.asarray(t, np.float64)
    inv = np.argsort(order)
    if shape == "cube":
        pitch = pitch or 4.0
        side = 1
        while side ** 3 < n:
            side += 1
        tgt = lattice((side,) * 3, pitch, rng)[:n]
        axis = (0.3, -0.5, 0.8)
    elif shape == "box":
        pitch = 2.0
        tgt = lattice(np.array((2, 5, 17))[inv], pitch, rng)
        axis = (0.3, -0.5, 0.8)
    elif shape == "product":
        pitch = 2.0
        tgt = lattice(np.array((3, 5, 9))[inv], pitch, rng, jitter=0.0)
    elif shape == "plane_z":
        pitch = 4.0
        side = int(np.ceil(np.sqrt(n)))
        tgt = lattice((side, side, 1), pitch, rng)[:n] + np.array([0.0, 0.0, 1.5])
        axis, e1, e2 = (0, 0, 1), np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    elif shape == "plane_xy":
        pitch = 4.0
        side = int(np.ceil(np.sqrt(n)))
        tgt = lattice((side, side, 1), pitch, rng, basis=[[1, 1, 0], [0, 0, 1], [0, 0, 0]])[:n]
        axis, e1, e2 = (1, -1, 0), np.array([1.0, 1, 0]), np.array([0, 0, 1.0])
    elif shape == "plane_111":
        pitch = 2.0
        side = int(np.ceil(np.sqrt(n)))
        tgt = lattice((side, side, 1), pitch, rng, jitter=0.0625, basis=[[1, -1, 0], [1, 1, -2], [0, 0, 0]])[:n]
        axis, e1, e2 = (1, 1, 1), np.array([1.0, -1, 0]), np.array([1.0, 1, -2])
    elif shape in ("line_x", "line_111"):
        pitch = 2.0
        u = np.array([1.0, 0, 0]) if shape == "line_x" else np.array([1.0, 1, 1])
        tgt = lattice((n, 1, 1), pitch, rng)[:, :1] * u
    elif shape == "slab_mirror":
        pitch = 4.0
        tgt = lattice((9, 5, 1), pitch, rng)
        z = to_grid(rng.uniform(0.0625, 0.25, len(tgt))) * rng.choice([-1.0, 1.0], len(tgt))
        tgt[:, 2] = z
    else:
        raise ValueError(shape)
    n = len(tgt)
    # the planted offset d: source = target - d
    room = 0.5 * (pitch - 2 * 0.25 - MARGIN) - 0.05
    if shape == "product":
        d = 0.25 * np.sign(tgt)
    elif shape in ("line_x", "line_111"):
        d = to_grid(rng.uniform(-0.25, 0.25, (n, 1))) * u
    elif shape == "slab_mirror":
        d = np.zeros_like(tgt); d[:, 2] = 2 * tgt[:, 2]                   # source z = -target z
    else:
        rmax = float(np.linalg.norm(tgt, axis=1).max())
        a = min(np.deg2rad(ang), max(room - np.linalg.norm(t), 0.0) / max(rmax, 1e-9))
        want = tgt @ (rot(axis, np.rad2deg(a)) - np.eye(3)).T + t
        if shape.startswith("plane"):
            # an offset in the plane, exactly: grid multiples of the plane's two integer directions
            d = np.outer(to_grid(want @ e1 / (e1 @ e1)), e1) + np.outer(to_grid(want @ e2 / (e2 @ e2)), e2)
        else:
            d = to_grid(want)
    src = tgt - d
    pi = rng.permutation(n)
    src = src[pi]
    planted = pi.copy()
    if holes:
        far = np.asarray(holes.get("far", ()), int); nan = np.asarray(holes.get("nan", ()), int)
        src = src.copy()
        src[far, 0] += 128.0                                             # beyond max_corr of every target point, still on the grid
        src[nan, rng.integers(0, 3, len(nan))] = np.nan
        planted[far] = -1; planted[nan] = -1
    ans = first_step(tgt, src, max_corr)
    assert np.array_equal(np.where(ans["ok"], ans["idx"], -1), planted), "the planted neighbour is not the nearest"
    return dict(tgt=tgt, src=src, pi=planted, ans=ans, max_corr=max_corr, shape=shape)


def assert_distinct(S, k=3):
    """the first k singular values differ by at least 1 % of the largest"""
    for i in range(k - 1):
        assert S[i] - S[i + 1] >= 0.01 * S[0], S


def hole_sets(n):
    """the index sets of the holes group: one wavefront at four lanes per query (16 queries), one workgroup row at four lanes = one
    wavefront at one lane (64 queries), all four rows of a 256-query row, the last partial row, every odd query"""
    last = (n - 1) // 256 * 256
    return {"wavefront": np.arange(272, 288), "row": np.arange(64, 128), "row_256": np.arange(512, 768), "last_partial": np.arange(last, n),
            "odd": np.arange(1, n, 2)}


# ---------------------------------------------------------------- OptimizedICPGN: one Gauss-Newton step from the identity
def gn_step(tgt, src, max_corr_sq):
    """H, B of registration.cpp:19-115 at T = I in integers (exact), the float64 solve, the pose after the step."""
    tgt = np.asarray(tgt, np.float64); src = np.asarray(src, np.float64)
    idx, d2, ok = pairs(tgt, src, max_corr_sq)
    n = int(ok.sum())
    out = dict(n_corr=n, ok=ok)
    P = np.round(src[ok] / GRID).astype(np.int64); Q = np.round(tgt[idx[ok]] / GRID).astype(np.int64)
    E = P - Q
    Z = np.zeros(n, np.int64)
    # A = -hat(p): rows (0, pz, -py), (-pz, 0, px), (py, -px, 0)
    A = np.stack([np.stack([Z, P[:, 2], -P[:, 1]], 1), np.stack([-P[:, 2], Z, P[:, 0]], 1), np.stack([P[:, 1], -P[:, 0], Z], 1)], 1)   # [n, r, c]
    sA = A.sum(0); sAA = np.einsum("nra,nrb->ab", A, A); sAe = np.einsum("nra,nr->a", A, E); sE = E.sum(0)
    assert max(int(np.abs(sAA).max()) if n else 0, 1) < 1 << 53
    H = np.zeros((6, 6)); B = np.zeros(6)
    H[:3, :3] = n * np.eye(3); H[:3, 3:] = sA * GRID; H[3:, :3] = sA.T * GRID; H[3:, 3:] = sAA * GRID * GRID
    B[:3] = -sE * GRID; B[3:] = -sAe * GRID * GRID
    out.update(H=H, B=B)
    if n == 0 or np.linalg.matrix_rank(H) < 6:
        out.update(delta=None, T=np.eye(4))
        return out
    delta = np.linalg.solve(H, B)
    w = delta[3:]; th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + (np.sin(th) / th) * K + ((1 - np.cos(th)) / (th * th)) * (K @ K) if th > 0 else np.eye(3)
    T = np.eye(4); T[:3, :3] = R; T[:3, 3] = delta[:3]
    out.update(delta=delta, T=T, cond=float(np.linalg.cond(H)))
    return out


def gn_error_K(T_got, g):
    """largest entry difference of the pose after the step, in units of cond(H) 2^-24 |delta|"""
    err = float(np.abs(np.asarray(T_got, np.float64)[:3] - g["T"][:3]).max())
    return err / (g["cond"] * 2.0 ** -24 * float(np.linalg.norm(g["delta"])))


# ---------------------------------------------------------------- the correspondence gate
GATE = 0.25                                    # max_corr_dist of the gate cases: dyadic, and so is its square


def plant_gate(seed, at=0, above=0, offsets=None, n=300):
    """n lattice points whose offsets are (0.5, 0, 0) — beyond max_corr_dist = 0.25 m — except: the first `at` source points have
    |d|^2 == 0.25^2 exactly (along x, -y, z in turn), the next `above` have d = (0.25, 2^-10, 0), the next distance the grid can
    express; offsets = {source index: d} overrides.  The target is listed in the source's order (pi is the identity)."""
    rng = np.random.default_rng(seed)
    tgt = lattice((7, 7, 7), 4.0, rng)[:n]
    d = np.tile([0.5, 0.0, 0.0], (n, 1))
    on = [np.array([GATE, 0, 0]), np.array([0, -GATE, 0]), np.array([0, 0, GATE])]
    for k in range(at):
        d[k] = on[k % 3]
    for k in range(at, at + above):
        d[k] = [GATE, GRID, 0.0]
    for k, v in (offsets or {}).items():
        d[k] = v
    src = tgt - d
    ans = first_step(tgt, src, GATE)
    return dict(tgt=tgt, src=src, ans=ans, max_corr=GATE, d=d)


def plant_dropout(seed=5):
    """Three pairs at the first iteration, two at the second: three points in a row along x with offsets +0.25, -0.25, +0.25 m along x.
    The best rigid motion is a shift of 1/12 m, which leaves the middle point 1/3 m away — outside the gate."""
    rng = np.random.default_rng(seed)
    tgt = lattice((7, 7, 7), 4.0, rng)[:300]
    row = [int(np.argmin(np.linalg.norm(tgt - np.array([x, 0.0, 0.0]), axis=1))) for x in (-8.0, 0.0, 8.0)]
    assert len(set(row)) == 3
    d = np.tile([0.5, 0.0, 0.0], (300, 1))
    for k, s in zip(row, (1.0, -1.0, 1.0)):
        d[k] = [s * GATE, 0.0, 0.0]
    src = tgt - d
    ans = first_step(tgt, src, GATE)
    assert ans["n_corr"] == 3
    return dict(tgt=tgt, src=src, ans=ans, max_corr=GATE, d=d)
