"""The ICP step, exactly (tests/icp_step_ref.py holds the planted clouds and the float64 reference; profiles/icp_step.md the figures).

On the dyadic clouds planted here the first iteration's sums are exact in any order, so `max_iters = 1` and `params.prev_mse` expose the
totals (count, MSE = sum d^2 / count), the closed-form step (every branch of svd3, the reflection sign, Tm * F) and every exit of
DefaultConvergenceCriteria through the public entry points, against numpy's SVD in double.

CPU: self-tests of the reference.  GPU: lisreg_icp_align, lisreg_icp_align_batch, lisreg_icp_gn_match, lisreg_icp_gn_match_batch."""
import numpy as np
import pytest

import icp_step_ref as ref

f32 = np.float32
DBL_MAX = ref.DBL_MAX
SMALL = (3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
REGIME = tuple(256 * k + d for k in (31, 32, 33, 96, 97, 128, 129, 225) for d in (-1, 0, 1))
GN_SIZES = (3, 64, 65, 257, 24577, 24833, 33025)
T_SMALL = (0.125, -0.0625, 0.1875)             # leaves a 2.8 degree rotation on a cloud of +-16 m
# 4 x the largest K of the oracle's float Gauss-Newton step over GN_SIZES and four holes cases: 0.287 (test_oracle_gn_step_K measures it)
GN_K_MAX = 1.15
_cache = {}


def case(n, seed=None, **kw):
    key = (n, seed, tuple(sorted((k, repr(v)) for k, v in kw.items())))
    if key not in _cache:
        kw.setdefault("motion", (3.0, T_SMALL))
        _cache[key] = ref.plant(n, n if seed is None else seed, **kw)
    return _cache[key]


def cloud(xyz):
    from lisreg import synth
    return synth.to_pcl(np.asarray(xyz, f32))


def ulp(x):
    return float(np.spacing(f32(abs(x))))


def params(max_corr=10.0, max_iters=1, prev_mse=DBL_MAX):
    import lisreg
    p = lisreg.icp_default_params(0)
    p.max_corr_dist, p.max_iters, p.prev_mse = max_corr, max_iters, prev_mse
    return p


def same(a, b):
    return (a["T"].tobytes() == b["T"].tobytes() and a["iters"] == b["iters"] and a["state"] == b["state"] and a["converged"] == b["converged"]
            and a["n_corr_last"] == b["n_corr_last"] and a["fitness"] == b["fitness"] and a["prev_mse"] == b["prev_mse"])


def check_matrix(T, want, n_ulp=2, scale_t=None):
    """every entry within n_ulp float32 ulps of the float64 answer: the ulp at max(|entry|, 1) for the rotation, at |t| (the length of
    the translation) for the translation; row 3 exactly 0 0 0 1"""
    T = np.asarray(T); want = np.asarray(want, np.float64)
    assert T.dtype == f32 and np.array_equal(T[3], [0, 0, 0, 1])
    worst = 0.0
    for r in range(3):
        for c in range(3):
            worst = max(worst, abs(float(T[r, c]) - want[r, c]) / ulp(max(abs(want[r, c]), 1.0)))
    ut = ulp(scale_t if scale_t is not None else np.linalg.norm(want[:3, 3]))
    for r in range(3):
        worst = max(worst, abs(float(T[r, 3]) - want[r, 3]) / ut)
    assert worst <= n_ulp, f"{worst:.2f} ulps from the float64 answer"
    return worst


def check_first_step(r, c, a=None):
    """one iteration of `c` from its guess: count, iteration count, state, matrix and fitness"""
    import lisreg
    a = a or c["ans"]
    assert r["n_corr_last"] == a["n_corr"] and r["iters"] == 1 and r["state"] == lisreg.ICP_ITERATIONS and r["converged"]
    worst = check_matrix(r["T"], a["T"])
    fit = ref.fitness(c["tgt"], c["src"], r["T"], work=f32)
    assert abs(r["fitness"] - fit) <= 1e-6 * fit, (r["fitness"], fit, ref.fitness(c["tgt"], c["src"], r["T"]))
    return worst


# ---------------------------------------------------------------- CPU: the reference checks itself
def test_ref_sums_are_exact_under_permutation():
    """float64 sums of the 17 terms in three different orders equal the integer totals to the bit; the float32 d^2 equals the double"""
    for n in (3, 64, 257, 33025):
        c = case(n)
        a = c["ans"]
        p, q = a["cur"][a["ok"]], c["tgt"][a["idx"][a["ok"]]]
        want = ref.totals_as_doubles(a["tot"])
        assert a["tot"]["bits"] <= 48                                      # of a double's 53 (47 at the largest size, 57 601)
        rng = np.random.default_rng(n)
        for order in (np.arange(len(p)), np.arange(len(p))[::-1], rng.permutation(len(p))):
            P, Q = p[order], q[order]
            got = [float(len(P))] + [float(np.cumsum(P[:, k])[-1]) for k in range(3)] + [float(np.cumsum(Q[:, k])[-1]) for k in range(3)]
            got += [float(np.cumsum(Q[:, r] * P[:, k])[-1]) for r in range(3) for k in range(3)]
            got += [float(np.cumsum(((P - Q) ** 2).sum(1))[-1])]
            assert np.array_equal(np.array(got), want)
        d = p.astype(f32) - q.astype(f32)
        d2f = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert d2f.dtype == f32 and np.array_equal(d2f.astype(np.float64), ((p - q) ** 2).sum(1))
        assert a["mse"] == want[16] / want[0]


def test_ref_planted_neighbour_is_brute_force_nearest():
    for n in (3, 64, 257):
        c = case(n)
        fin = np.isfinite(c["src"]).all(1)
        D = np.linalg.norm(c["src"][fin, None, :] - c["tgt"][None, :, :], axis=2)
        assert np.array_equal(D.argmin(1), c["pi"][fin])
        if n > 1:
            s = np.sort(D, 1)
            assert (s[:, 1] - s[:, 0]).min() >= 1.0
    for holes in ref.hole_sets(1025).values():
        for kind in ("far", "nan"):
            c = case(1025, holes={kind: holes})
            assert c["ans"]["n_corr"] == 1025 - len(holes)


def assert_kabsch_is_the_optimum(c):
    """the reference's step is a proper rotation at which the pairs exert no torque, no nearby rotation does better, and t = md - R ms"""
    a = c["ans"]
    p, q = a["cur"][a["ok"]], c["tgt"][a["idx"][a["ok"]]]
    pc, qc = p - p.mean(0), q - q.mean(0)
    R, t = a["Tm"][:3, :3], a["Tm"][:3, 3]
    assert abs(np.linalg.det(R) - 1) < 1e-12 and np.abs(R @ R.T - np.eye(3)).max() < 1e-12
    assert np.abs(t - (q.mean(0) - R @ p.mean(0))).max() < 1e-12
    scale = float((np.linalg.norm(pc, axis=1) * np.linalg.norm(qc, axis=1)).sum())
    assert np.abs(np.cross(pc @ R.T, qc).sum(0)).max() <= 1e-12 * scale
    cost = lambda M: float(((pc @ M.T - qc) ** 2).sum())
    rng = np.random.default_rng(1)
    for _ in range(20):
        w = rng.normal(size=3)
        for deg in (0.05, 1.0, 30.0, 180.0):
            assert cost(R) <= cost(ref.rot(w, deg) @ R) * (1 + 1e-12)


def test_ref_kabsch_rank2_reflection_and_census():
    """Kabsch from the exact totals is the optimum on the rank-2, the three-pair and the reflection cases; the planted ranks hold"""
    for shape in ("plane_z", "plane_xy", "plane_111"):
        c = case(200, 7, shape=shape, motion=(3.0, (0.0625, -0.03125, 0.0625)))
        a = c["ans"]
        assert a["S"][2] <= 1e-12 * a["S"][0] and a["S"][1] - a["S"][2] >= 0.01 * a["S"][0]
        assert ref.rot_angle(a["Tm"][:3, :3]) > 5e-3
        assert_kabsch_is_the_optimum(c)
    assert_kabsch_is_the_optimum(ref.plant_gate(8, at=3, above=4))
    assert_kabsch_is_the_optimum(case(257))
    c = case(0, 3, shape="slab_mirror")
    a = c["ans"]
    assert a["s"] == -1.0
    assert_kabsch_is_the_optimum(c)
    ref.assert_distinct(a["S"])
    assert ref.rot_angle(a["Tm"][:3, :3]) < 0.01                       # the mirror cannot be undone: the best rotation leaves the slab where it is
    for shape in ("line_x", "line_111"):
        a = case(100, 7, shape=shape)["ans"]
        assert a["S"][1] <= 1e-12 * a["S"][0]
    seen = set()
    for order in [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]:
        a = case(0, 3, shape="box", order=order, motion=(3.0, (0.0625, -0.03125, 0.0625)))["ans"]
        ref.assert_distinct(a["S"])
        a = case(0, 3, shape="product", order=order)["ans"]
        ref.assert_distinct(a["S"])
        assert np.array_equal(a["sigma"], np.diag(np.diag(a["sigma"]))) and np.array_equal(a["Tm"], np.eye(4))
        seen.add(tuple(np.argsort(-np.diag(a["sigma"]))))
    assert len(seen) == 6                                              # every order of the three singular values along the axes


def test_ref_loop_decisions_are_not_borderline():
    """the whole-alignment cases: the loop's own assertions (margins at every iteration, every stopping quantity 1e-3 clear of its
    threshold) hold in double and in both float variants, which agree on state, iterations and count"""
    for c in whole_cases():
        runs = whole_runs(c)
        assert len({(r["state"], r["iters"], r["n_corr"]) for r in runs.values()}) == 1
    c = ref.plant_dropout()
    r = ref.icp_loop(c["tgt"], c["src"], max_corr=ref.GATE, exact=("gate",))
    assert (r["state"], r["iters"], r["n_corr"]) == (ref.NO_CORRESPONDENCES, 1, 2)


def whole_cases():
    return [case(300, 11), case(700, 12), case(200, 13, shape="plane_z")]


def whole_runs(c):
    return {k: ref.icp_loop(c["tgt"], c["src"], work=w, fma=f) for k, (w, f) in
            {"double": (np.float64, False), "float": (f32, False), "float_fma": (f32, True)}.items()}


def float_effect(runs):
    """largest pose difference among the reference's variants: what float storage of the working copy and the matrices costs"""
    ks = list(runs)
    d = [ref.pose_diff(runs[a]["T"], runs[b]["T"]) for i, a in enumerate(ks) for b in ks[i + 1:]]
    return max(x[0] for x in d), max(x[1] for x in d)


def gn_cases():
    out = [case(n) for n in GN_SIZES]
    for n in (1025, 24833):
        hs = ref.hole_sets(n)
        out += [case(n, holes={"far": hs["odd"]}), case(n, holes={"nan": hs["row_256"]})]
    return out


def test_oracle_gn_step_K(oracle):
    """the oracle's OptimizedICPGN step (float 6 x 6 inverse, as the reference) against the float64 solve of the exact H and B: K, the
    error in units of cond(H) 2^-24 |delta|, stays below GN_K_MAX / 4 — the bar of the GPU test is 4 x the largest K"""
    worst = 0.0
    for c in gn_cases():
        g = ref.gn_step(c["tgt"], c["src"], 4.0)
        r = oracle.icp_gn_match(cloud(c["tgt"]), cloud(c["src"]), 1, 4.0, np.eye(4, dtype=f32))
        assert r["steps_applied"] == 1 and r["n_corr_last"] == g["n_corr"]
        K = ref.gn_error_K(r["T"], g)
        print(f"oracle GN n={len(c['src'])} n_corr={g['n_corr']} cond={g['cond']:.3g} |delta|={np.linalg.norm(g['delta']):.3g} K={K:.4f}")
        worst = max(worst, K)
    print(f"largest K of the oracle: {worst:.4f}")
    assert worst <= GN_K_MAX / 4


# ---------------------------------------------------------------- GPU
_slots = {}


def slot_of(ctx, c):
    """the map index of a case's target, built once per context"""
    key = (id(ctx), id(c["tgt"]))
    if key not in _slots:
        _slots[key] = (300 + len(_slots), c["tgt"])                      # (the array is kept: its id stays its own)
        ctx.map_index_set(_slots[key][0], cloud(c["tgt"]))
    return _slots[key][0]


def align(ctx, c, p, guess=None, src=None):
    return ctx.icp_align(slot_of(ctx, c), cloud(c["src"] if src is None else src), p, guess=guess)


def both_lanes(ctx, monkeypatch, c, p, guess=None, src=None):
    out = {}
    for q in ("1", "4"):
        monkeypatch.setenv("LISREG_NN1_Q", q)
        out[q] = align(ctx, c, p, guess, src)
    monkeypatch.delenv("LISREG_NN1_Q")
    assert same(out["1"], out["4"]), (out["1"], out["4"])
    return out["4"]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL + REGIME)
def test_first_step_exact_totals(gpu_ctx, monkeypatch, n):
    c = case(n)
    r = both_lanes(gpu_ctx, monkeypatch, c, params())
    worst = check_first_step(r, c)
    print(f"n={n} worst {worst:.2f} ulp, fitness {r['fitness']:.6g}")
    # MSE = sum d^2 / count of the first iteration, to the bit: a second iteration is allowed, so the first one's value is kept
    r2 = align(gpu_ctx, c, params(max_iters=2, prev_mse=0.0))
    assert r2["prev_mse"] == c["ans"]["mse"] and r2["iters"] == 2


@pytest.mark.gpu
def test_first_step_in_a_batch_equals_single_calls(gpu_ctx):
    """a case twice with other cases in between: the same bytes as the single call (a batch under and one over the 500 k source points
    at which a batch goes to one lane per query)"""
    p = params()
    for sizes in ((3, 1025, 65, 3, 7937, 256, 1025), REGIME[::3] + (57601, 24833) + REGIME[1::3] + (57601,) + REGIME[2::3] + (24833, 57600) * 3):
        cs = [case(n) for n in sizes]
        rb = gpu_ctx.icp_align_batch([(slot_of(gpu_ctx, c), cloud(c["src"]), None) for c in cs], p)
        seen = {}
        for c, r in zip(cs, rb):
            n = len(c["src"])
            if n not in seen:
                seen[n] = align(gpu_ctx, c, p)
                check_first_step(seen[n], c)
            assert same(r, seen[n]), (n, r, seen[n])
    assert sum(sizes) >= 500000


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1025, 24833))
@pytest.mark.parametrize("kind", ("far", "nan"))
@pytest.mark.parametrize("which", ("wavefront", "row", "row_256", "last_partial", "odd"))
def test_first_step_with_holes(gpu_ctx, monkeypatch, n, kind, which):
    c = case(n, holes={kind: ref.hole_sets(n)[which]})
    assert c["ans"]["n_corr"] == n - len(ref.hole_sets(n)[which])
    r = both_lanes(gpu_ctx, monkeypatch, c, params())
    if kind == "nan":
        # a NaN point has no neighbour and no distance: count, matrix and state as planted; the fitness over the finite points
        import lisreg
        assert r["n_corr_last"] == c["ans"]["n_corr"] and r["iters"] == 1 and r["state"] == lisreg.ICP_ITERATIONS
        check_matrix(r["T"], c["ans"]["T"])
    else:
        check_first_step(r, c)
    r2 = align(gpu_ctx, c, params(max_iters=2, prev_mse=0.0))
    assert r2["prev_mse"] == c["ans"]["mse"]


@pytest.mark.gpu
def test_correspondence_gate(gpu_ctx, monkeypatch):
    import lisreg
    # |d|^2 == max_corr_dist^2 pairs, the next distance above does not
    c = ref.plant_gate(3, at=10, above=10)
    assert c["ans"]["n_corr"] == 10
    r = both_lanes(gpu_ctx, monkeypatch, c, params(ref.GATE))
    assert r["n_corr_last"] == 10 and r["state"] == lisreg.ICP_ITERATIONS
    check_matrix(r["T"], c["ans"]["T"])
    # a max_corr_dist whose square is no float: D = 0.25^2 + 2^-20 is the d^2 of the ten points above; m * m < D in double, but rounds
    # to D in float — PCL compares in double, so they must stay out; with m * m >= D they pair
    D = ref.GATE ** 2 + 2.0 ** -20
    lo = np.sqrt(D)
    while lo * lo >= D:
        lo = np.nextafter(lo, 0.0)
    hi = np.sqrt(D)
    while hi * hi < D:
        hi = np.nextafter(hi, 1.0)
    assert float(f32(lo * lo)) == D and lo * lo < D <= hi * hi
    assert both_lanes(gpu_ctx, monkeypatch, c, params(float(lo)))["n_corr_last"] == 10
    assert both_lanes(gpu_ctx, monkeypatch, c, params(float(hi)))["n_corr_last"] == 20
    # 0, 1, 2 surviving pairs: no correspondences, nothing moved; 3: solved (three points: rank 2)
    G = np.eye(4, dtype=f32); G[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]; G[:3, 3] = [4, -8, 12]
    for k in (0, 1, 2):
        c = ref.plant_gate(4 + k, at=k, above=4)
        for guess in (None, G):
            src = c["src"] if guess is None else (c["src"] - G[:3, 3].astype(np.float64)) @ G[:3, :3].astype(np.float64)
            r = both_lanes(gpu_ctx, monkeypatch, c, params(ref.GATE, max_iters=30), guess, src)
            assert r["state"] == lisreg.ICP_NO_CORRESPONDENCES and not r["converged"] and r["iters"] == 0 and r["n_corr_last"] == k
            assert np.array_equal(r["T"], np.eye(4, dtype=f32) if guess is None else G)
    c = ref.plant_gate(8, at=3, above=4)
    a = c["ans"]
    assert a["n_corr"] == 3 and a["S"][2] <= 1e-12 * a["S"][0] and a["S"][1] >= 0.01 * a["S"][0]
    r = both_lanes(gpu_ctx, monkeypatch, c, params(ref.GATE))
    assert r["n_corr_last"] == 3 and r["iters"] == 1 and r["state"] == lisreg.ICP_ITERATIONS
    check_matrix(r["T"], a["T"])


def check_rotation_properties(r, c):
    """where the best rotation is not unique: a finite proper rotation whose residual is the float64 optimum's"""
    a = c["ans"]
    T = r["T"].astype(np.float64)
    assert np.all(np.isfinite(T)) and np.array_equal(r["T"][3], [0, 0, 0, 1])
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-6
    p, q = a["cur"][a["ok"]], c["tgt"][a["idx"][a["ok"]]]
    rms = lambda M: float(np.sqrt((((p @ M[:3, :3].T + M[:3, 3]) - q) ** 2).sum(1).mean()))
    assert abs(rms(T) - rms(a["Tm"])) < 1e-6, (rms(T), rms(a["Tm"]))


@pytest.mark.gpu
def test_svd_branches(gpu_ctx, monkeypatch):
    p = params()
    small = (3.0, (0.0625, -0.03125, 0.0625))
    for order in [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]:
        c = case(0, 3, shape="box", order=order, motion=small)                  # U and V re-ordered together
        check_first_step(both_lanes(gpu_ctx, monkeypatch, c, p), c)
        c = case(0, 3, shape="product", order=order)                            # sigma diagonal: no Jacobi rotation at all
        r = both_lanes(gpu_ctx, monkeypatch, c, p)
        assert np.array_equal(r["T"], np.eye(4, dtype=f32)) and r["n_corr_last"] == 135
    for shape in ("plane_z", "plane_xy", "plane_111"):                          # rank 2: the third column of U is completed
        c = case(200, 7, shape=shape, motion=small)
        check_first_step(both_lanes(gpu_ctx, monkeypatch, c, p), c)
    c = case(0, 3, shape="slab_mirror")                                         # det U det V < 0
    check_first_step(both_lanes(gpu_ctx, monkeypatch, c, p), c)
    for shape in ("line_x", "line_111"):                                        # rank 1
        c = case(100, 7, shape=shape)
        r = both_lanes(gpu_ctx, monkeypatch, c, p)
        assert r["n_corr_last"] == 100 and r["iters"] == 1
        check_rotation_properties(r, c)
    # rank 0: every source point pairs with one target point / every source point is the same point
    base = case(64)
    y = base["tgt"][5]
    rng = np.random.default_rng(9)
    cluster = y + ref.to_grid(rng.uniform(-0.75, 0.75, (40, 3)))
    for src in (cluster, np.tile(cluster[:1], (40, 1))):
        a = ref.first_step(base["tgt"], src, 10.0)
        assert a["n_corr"] == 40 and np.all(a["idx"] == 5) and np.all(a["sigma"] == 0)
        c = dict(base, src=src, ans=a)
        r = both_lanes(gpu_ctx, monkeypatch, c, p)
        assert r["n_corr_last"] == 40 and r["iters"] == 1
        check_rotation_properties(r, c)


@pytest.mark.gpu
def test_composition_is_step_times_guess(gpu_ctx, monkeypatch):
    c = case(257)
    G = np.eye(4); G[:3, :3] = [[0, 0, -1], [1, 0, 0], [0, -1, 0]]; G[:3, 3] = [8, -4, 2]
    src = (c["src"] - G[:3, 3]) @ G[:3, :3]                                     # G^-1 of the planted source: exact
    a = ref.first_step(c["tgt"], src, 10.0, guess=G)
    assert np.array_equal(a["cur"], c["src"]) and np.array_equal(a["Tm"], c["ans"]["Tm"])
    want, other = a["Tm"] @ G, G @ a["Tm"]
    assert np.abs(want - other).max() > 1e-2
    r = both_lanes(gpu_ctx, monkeypatch, c, params(), G.astype(f32), src)
    assert r["n_corr_last"] == 257 and r["iters"] == 1
    terms = np.abs(a["Tm"][:3, :3]) @ np.abs(G[:3, 3])
    worst = check_matrix(r["T"], want, n_ulp=4, scale_t=max(float(terms.max()), float(np.abs(want[:3, 3]).max())))
    print(f"composition: {worst:.2f} ulp")
    assert np.abs(r["T"].astype(np.float64) - other).max() > 1e-2


def stop_items():
    """(case, source or None, params kwargs, expected state, iterations, returned prev_mse) of the stopping-rule group"""
    c = case(257)
    m = c["ans"]["mse"]
    sub = dict(c, src=c["tgt"][::3].copy())
    sub["ans"] = ref.first_step(sub["tgt"], sub["src"], 10.0)
    assert sub["ans"]["mse"] == 0.0
    eps = 1e-4
    up = m * (1 + 2 * eps)
    mid = m * (1 + 1.5 * eps)
    assert abs((m + 2e-12) - m) >= 1e-12 and abs(m - up) / up > eps * 1.5 and abs(m - mid) < 0.9 * eps and abs(m - mid) / mid > 1.4 * eps
    return c, sub, [
        (c, dict(max_iters=30, prev_mse=m), ref.ABS_MSE, 1, m),
        (c, dict(max_iters=30, prev_mse=m + 2e-12), ref.REL_MSE, 1, m + 2e-12),
        (c, dict(max_iters=2, prev_mse=up), ref.ITERATIONS, 2, m),
        (c, dict(max_iters=2, prev_mse=mid), ref.ITERATIONS, 2, m),                   # |difference| below eps, the RELATIVE one above it
        (sub, dict(max_iters=30, prev_mse=DBL_MAX), ref.TRANSFORM, 1, DBL_MAX),
        (sub, dict(max_iters=30, prev_mse=0.0), ref.TRANSFORM, 1, 0.0),             # the transform exit comes before both MSE exits
        (sub, dict(max_iters=1, prev_mse=DBL_MAX), ref.ITERATIONS, 1, DBL_MAX),      # and the iteration exit before it
        (c, dict(max_iters=1, prev_mse=m), ref.ITERATIONS, 1, m),
        (c, dict(max_iters=2, prev_mse=0.0), ref.ITERATIONS, 2, m),
        (c, dict(max_iters=2, prev_mse=DBL_MAX), ref.ITERATIONS, 2, m),
    ]


@pytest.mark.gpu
def test_stopping_rules(gpu_ctx, monkeypatch):
    import lisreg
    assert (lisreg.ICP_ITERATIONS, lisreg.ICP_TRANSFORM, lisreg.ICP_ABS_MSE, lisreg.ICP_REL_MSE, lisreg.ICP_NO_CORRESPONDENCES) == \
        (ref.ITERATIONS, ref.TRANSFORM, ref.ABS_MSE, ref.REL_MSE, ref.NO_CORRESPONDENCES)
    c, sub, items = stop_items()
    for cs, kw, state, iters, prev in items:
        want = ref.icp_loop(cs["tgt"], cs["src"], max_iters=kw["max_iters"], prev_mse=kw["prev_mse"], exact=("abs", "rel", "transform"))
        assert (want["state"], want["iters"], want["prev_mse"]) == (state, iters, prev), (kw, want["state"], want["iters"], want["prev_mse"])
        r = both_lanes(gpu_ctx, monkeypatch, cs, params(**kw))
        assert (r["state"], r["iters"], r["prev_mse"], r["converged"]) == (state, iters, prev, True), (kw, r)
        if iters == 1:
            check_matrix(r["T"], cs["ans"]["T"], scale_t=max(np.linalg.norm(cs["ans"]["T"][:3, 3]), 2.0 ** -10))
    # fewer than three pairs at the SECOND iteration: state 5 at one iteration, F that of the first
    d = ref.plant_dropout()
    r = both_lanes(gpu_ctx, monkeypatch, d, params(ref.GATE, max_iters=30))
    assert (r["state"], r["iters"], r["converged"], r["n_corr_last"]) == (ref.NO_CORRESPONDENCES, 1, False, 2), r
    check_matrix(r["T"], d["ans"]["T"], n_ulp=4)
    assert r["prev_mse"] == d["ans"]["mse"] == 0.0625


@pytest.mark.gpu
def test_stopping_rules_chained_batch(gpu_ctx):
    """lisreg_icp_align_batch with chain_prev_mse = 1: the value the item before leaves behind makes the first comparison"""
    c, sub, _ = stop_items()
    m = c["ans"]["mse"]
    near = dict(c, src=c["src"].copy())
    near["src"][0, 0] += ref.GRID                                       # one offset a grid step longer: an MSE ~1e-6 relative away
    near["ans"] = ref.first_step(near["tgt"], near["src"], 10.0)
    m2 = near["ans"]["mse"]
    assert 1e-12 < abs(m2 - m) and abs(m2 - m) / m < 1e-5
    other = case(300, 11)
    mo = other["ans"]["mse"]
    assert abs(mo - m) / m > 1e-2
    seq = [(c, ref.ITERATIONS, 2, m), (c, ref.ABS_MSE, 1, m), (near, ref.REL_MSE, 1, m), (other, ref.ITERATIONS, 2, mo),
           (sub, ref.TRANSFORM, 1, mo), (other, ref.ABS_MSE, 1, mo), (c, ref.ITERATIONS, 2, m)]
    p = params(max_iters=2)
    items = [(slot_of(gpu_ctx, cs), cloud(cs["src"]), None) for cs, _, _, _ in seq]
    rb = gpu_ctx.icp_align_batch(items, p, chain_prev_mse=True)
    carry = DBL_MAX
    for k, ((cs, state, iters, prev), r) in enumerate(zip(seq, rb)):
        assert (r["state"], r["iters"], r["prev_mse"], r["converged"]) == (state, iters, prev, True), (k, r)
        one = align(gpu_ctx, cs, params(max_iters=2, prev_mse=carry))           # the sequential loop through the single entry point
        assert same(r, one), (k, r, one)
        carry = one["prev_mse"]
    # unchained: every item starts from params.prev_mse
    ru = gpu_ctx.icp_align_batch(items, params(max_iters=2, prev_mse=m), chain_prev_mse=False)
    assert [r["state"] for r in ru] == [ref.ABS_MSE, ref.ABS_MSE, ref.REL_MSE, ref.ITERATIONS, ref.TRANSFORM, ref.ITERATIONS, ref.ABS_MSE]


@pytest.mark.gpu
def test_whole_alignments(gpu_ctx, monkeypatch):
    """default parameters, to their own end: state, iterations and count of the float64 loop; the pose within 4 x the float effect the
    reference's own variants show (profiles/icp_step.md)"""
    import lisreg
    for c in whole_cases():
        runs = whole_runs(c)
        want = runs["double"]
        eff_r, eff_t = float_effect(runs)
        p = lisreg.icp_default_params(0)
        r = both_lanes(gpu_ctx, monkeypatch, c, p)
        dr, dt = ref.pose_diff(r["T"], want["T"])
        print(f"whole n={len(c['src'])} {c['shape']}: state {r['state']} iters {r['iters']} float effect {eff_r:.3g} rad {eff_t:.3g} m, "
              f"GPU against double {dr:.3g} rad {dt:.3g} m")
        assert (r["state"], r["iters"], r["n_corr_last"], r["converged"]) == (want["state"], want["iters"], want["n_corr"], True)
        assert dr <= 4 * eff_r and dt <= 4 * eff_t, (dr, dt, eff_r, eff_t)


def check_gn(r, g):
    assert r["n_corr_last"] == g["n_corr"] and r["steps_applied"] == 1
    K = ref.gn_error_K(r["T"], g)
    assert np.array_equal(r["T"][3], [0, 0, 0, 1]) and K <= GN_K_MAX, K
    return K


@pytest.mark.gpu
def test_icp_gn_first_step(gpu_ctx, monkeypatch):
    import lisreg
    cs = gn_cases()
    I4 = np.eye(4, dtype=f32)
    singles = []
    for c in cs:
        g = ref.gn_step(c["tgt"], c["src"], 4.0)
        out = {}
        for q in ("1", "4"):
            monkeypatch.setenv("LISREG_NN1_Q", q)
            out[q] = gpu_ctx.icp_gn_match(slot_of(gpu_ctx, c), cloud(c["src"]), 1, 4.0, I4)
        monkeypatch.delenv("LISREG_NN1_Q")
        K = check_gn(out["4"], g)
        assert check_gn(out["1"], g) <= GN_K_MAX
        print(f"GN n={len(c['src'])} n_corr={g['n_corr']} cond={g['cond']:.3g} K={K:.4f}")
        singles.append(gpu_ctx.icp_gn_match(slot_of(gpu_ctx, c), cloud(c["src"]), 1, 4.0, I4))
    items = [lisreg.IcpGnItem(k, slot_of(gpu_ctx, c), None) for k, c in enumerate(cs)]
    rb, _ = gpu_ctx.icp_gn_match_batch([cloud(c["src"]) for c in cs], items, 1, 4.0)
    for c, r, s in zip(cs, rb, singles):
        check_gn(r, ref.gn_step(c["tgt"], c["src"], 4.0))
        assert r["T"].tobytes() == s["T"].tobytes() and r["n_corr_last"] == s["n_corr_last"]
    # a singular H: no pair at all, and three identical pairs (rank 3) — no step, the pose untouched
    base = case(64)
    P0 = np.eye(4, dtype=f32); P0[:3, 3] = [1, -2, 3]
    far = base["src"] + np.array([128.0, 0, 0])
    r = gpu_ctx.icp_gn_match(slot_of(gpu_ctx, base), cloud(far), 1, 4.0, P0)
    assert r["steps_applied"] == 0 and r["n_corr_last"] == 0 and np.array_equal(r["T"], P0)
    tgt3 = np.array([[2.0, 4.0, -8.0], [40.0, 0, 0], [0, 40.0, 0], [0, 0, 40.0]])
    src3 = np.tile([[2.5, 4.0, -8.0]], (3, 1))
    c3 = dict(tgt=tgt3, src=src3)
    g = ref.gn_step(tgt3, src3, 4.0)
    assert g["n_corr"] == 3 and g["delta"] is None
    r = gpu_ctx.icp_gn_match(slot_of(gpu_ctx, c3), cloud(src3), 1, 4.0, I4)
    assert r["steps_applied"] == 0 and r["n_corr_last"] == 3 and np.array_equal(r["T"], I4)
    rb, _ = gpu_ctx.icp_gn_match_batch([cloud(src3), cloud(far)], [lisreg.IcpGnItem(0, slot_of(gpu_ctx, c3), None),
                                                                     lisreg.IcpGnItem(1, slot_of(gpu_ctx, base), P0)], 1, 4.0)
    assert rb[0]["steps_applied"] == 0 and np.array_equal(rb[0]["T"], I4) and rb[1]["steps_applied"] == 0 and np.array_equal(rb[1]["T"], P0)
