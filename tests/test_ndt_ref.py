"""tests/ndt_ref.py, the definition of lisreg_ndt_*, checked against itself and against numpy on the CPU: the loop form equals the
vector form, the derivatives are those of the score, the voxel statistics are numpy's, and the line search returns steps that satisfy
the strong Wolfe conditions on functions with a known minimiser, through each of its four cases and three updates."""
import numpy as np
import pytest

import ndt_ref as R


@pytest.fixture(scope="module")
def small():
    """a few hundred target points in a corner of a room, a few source points near it"""
    rng = np.random.default_rng(3)
    n = 1500
    floor = np.stack([rng.uniform(0, 4, n), rng.uniform(0, 4, n), rng.normal(0, 0.02, n)], 1)
    wall = np.stack([rng.normal(0, 0.02, n), rng.uniform(0, 4, n), rng.uniform(0, 3, n)], 1)
    wall2 = np.stack([rng.uniform(0, 4, n), rng.normal(4, 0.02, n), rng.uniform(0, 3, n)], 1)
    stray = np.array([2.5, 2.5, 2.5]) + rng.uniform(-0.3, 0.3, (4, 3))          # a voxel of four points: no Gaussian
    tgt = np.concatenate([floor, wall, wall2, stray]).astype(np.float32) + np.float32(10.0)
    src = tgt[rng.choice(len(tgt), 80, replace=False)] + rng.normal(0, 0.01, (80, 3)).astype(np.float32)
    src[7] = np.nan
    prm = R.params()
    return R.build_target(tgt, prm), tgt, np.ascontiguousarray(src, np.float32), prm


P_TEST = np.array([0.11, -0.07, 0.05, 0.013, -0.021, 0.017])


def test_loop_form_equals_vector_form(small):
    T, _, src, prm = small
    for p in (P_TEST, np.zeros(6), np.array([0.1, 0, 0, 5e-5, -2e-5, 9e-5]), np.array([500.0, 0, 0, 0, 0, 0])):
        for hess in (True, False):
            a, b = R.evaluate_loops(T, src, p, prm, hess), R.evaluate(T, src, p, prm, hess)
            assert a["n_pairs"] == b["n_pairs"]
            assert np.allclose(a["abs"], b["abs"], rtol=1e-12, atol=0)
            assert np.all(np.abs(a["out"] - b["out"]) <= 1e-13 * a["abs"])
            if not hess:
                assert not a["out"][7:].any() and not b["out"][7:].any()
    assert R.evaluate(T, src, P_TEST, prm)["n_pairs"] > 100
    assert R.evaluate(T, src, np.array([500.0, 0, 0, 0, 0, 0]), prm)["n_pairs"] == 0


def test_gradient_and_hessian_are_the_scores_derivatives(small):
    T, _, src, prm = small
    # pairs enter and leave the radius as p moves, which steps the score: the derivatives are those of the score over a FIXED pair set
    pairs = R.find_pairs(T, R.transform_points(P_TEST, src), prm["resolution"])
    f = lambda p: R.evaluate(T, src, p, prm, False, pairs)["out"]
    ev = R.evaluate(T, src, P_TEST, prm)
    assert ev["n_pairs"] == len(pairs[0])
    score, g, H = R.unpack(ev["out"])
    h = 1e-6
    for i in range(6):
        e = np.zeros(6); e[i] = h
        up, dn = f(P_TEST + e), f(P_TEST - e)
        assert abs((up[0] - dn[0]) / (2 * h) - g[i]) <= 1e-6 * ev["abs"][1 + i], i
        assert np.all(np.abs((up[1:7] - dn[1:7]) / (2 * h) - H[i]) <= 1e-5 * np.abs(H).max()), i
    assert np.allclose(H, H.T)


def test_small_angle_shortcut_touches_the_derivatives_only():
    p = np.array([1.0, 2.0, 3.0, 5e-5, -9.9e-5, 2e-5])
    Rm, dR, ddR = R.pose_matrices(p)
    R0, dR0, ddR0 = R.pose_matrices(np.array([1.0, 2.0, 3.0, 0, 0, 0]))
    assert np.array_equal(dR, dR0) and np.array_equal(ddR, ddR0)
    assert not np.array_equal(Rm, R0) and np.allclose(Rm, R0, atol=2e-4)
    q = np.array([0.3, -0.2, 0.1, 0.4, -0.5, 0.6])
    assert np.allclose(R.p_from_matrix(R.matrix_from_p(q)), q, atol=1e-12)
    # the analytic derivative matrices against differences of R
    Rq, dRq, ddRq = R.pose_matrices(q)
    for k in range(3):
        e = np.zeros(6); e[3 + k] = 1e-6
        assert np.allclose((R.pose_matrices(q + e)[0] - R.pose_matrices(q - e)[0]) / 2e-6, dRq[k], atol=1e-8)
        for l in range(k, 3):
            assert np.allclose((R.pose_matrices(q + e)[1][l] - R.pose_matrices(q - e)[1][l]) / 2e-6, ddRq[R.ANG_PAIR[(k, l)]], atol=1e-8)


def test_voxel_statistics_are_numpys(small):
    T, tgt, _, prm = small
    cell, dims, min_b = R.voxel_cells(tgt, 1.0)
    assert np.array_equal(cell, (np.floor(tgt[:, 0]) - min_b[0] + (np.floor(tgt[:, 1]) - min_b[1]) * dims[0]
                                 + (np.floor(tgt[:, 2]) - min_b[2]) * dims[0] * dims[1]).astype(np.int64))
    assert len(T["cell_ids"]) > 20 and np.all(np.diff(T["cell_ids"]) > 0)
    for k, cid in enumerate(T["cell_ids"]):
        pts = tgt[cell == cid].astype(np.float64)
        assert len(pts) == T["counts"][k] >= 6
        assert np.allclose(T["means"][k], pts.mean(0), rtol=0, atol=1e-12 * 14)
        cov = np.cov(pts.T)
        lam, V = np.linalg.eigh(cov)
        lam = np.maximum(lam, 0.01 * lam[2])
        ic = np.linalg.inv((V * lam) @ V.T)
        assert np.allclose(T["icov"][k], ic, rtol=0, atol=1e-9 * np.abs(ic).max())
        assert np.linalg.cond(T["icov"][k]) <= 100 * (1 + 1e-9)
    few = [cid for cid in np.unique(cell) if (cell == cid).sum() < 6]
    assert few and not set(few) & set(T["cell_ids"])


def test_planted_voxels():
    xyz = R.planted_cloud()
    T = R.build_target(xyz, R.params())
    cell, dims, _ = R.voxel_cells(xyz, 1.0)
    assert (cell < 0).sum() == 5 and list(dims) == [5, 3, 3]
    by = dict(zip(T["cell_ids"].tolist(), range(len(T["cell_ids"]))))
    cid = lambda i, j, k: i + j * 5 + k * 15
    assert cid(0, 0, 0) not in by                                   # five points (and two NaN records that belong to no voxel)
    assert T["counts"][by[cid(2, 0, 0)]] == 6
    assert cid(4, 2, 0) not in by                                   # six identical points
    assert T["counts"][by[cid(0, 0, 2)]] == 3000
    flat, line = T["icov"][by[cid(0, 2, 0)]], T["icov"][by[cid(2, 2, 0)]]
    lam_f, lam_l = np.linalg.eigvalsh(np.linalg.inv(flat)), np.linalg.eigvalsh(np.linalg.inv(line))
    assert np.isclose(lam_f[0], 0.01 * lam_f[2]) and lam_f[1] > 0.02 * lam_f[2]           # one eigenvalue raised
    assert np.isclose(lam_l[0], 0.01 * lam_l[2]) and np.isclose(lam_l[1], 0.01 * lam_l[2])  # two
    assert T["n_voxels"] == 10 and len(T["cell_ids"]) == 8


# phi(a) = -a / (a^2 + c) + w sin(8 a): for w = 0 the minimiser is sqrt(c)
def _phi(c, w):
    return lambda a: (-(a / (a * a + c)) + w * np.sin(8 * a), -((c - a * a) / (a * a + c) ** 2) + 8 * w * np.cos(8 * a))


def test_line_search_on_scalar_functions():
    seen = set()
    n_wolfe = 0
    for c in (0.004, 2.0, 0.3, 30.0):
        for w in (0.0, 0.01, 0.05):
            f = _phi(c, w)
            phi_0, d_0 = f(0.0)
            for step_init in (1e-3, 0.05, 0.5, 3.0, 40.0):
                for step_max in (0.1, 1.0, 100.0):
                    D = R.Decisions()
                    a, trials = R.line_search_mt(f, phi_0, d_0, step_init, step_max, 0.005, D)
                    seen |= set(D.log)
                    assert np.isfinite(a) and 0.005 <= a <= step_max and trials <= R.MAX_TRIALS
                    ended = {"degenerate", "no trial"} & set(D.log)
                    if not ended and trials < R.MAX_TRIALS:
                        # the search ended because the strong Wolfe conditions hold
                        phi_a, d_a = f(a)
                        assert phi_a <= phi_0 + R.MU * a * d_0 and abs(d_a) <= R.NU * abs(d_0), (c, w, step_init, step_max)
                        n_wolfe += 1
                        if w == 0.0 and step_max >= np.sqrt(c) * 4 and trials:
                            assert abs(f(a)[1]) <= R.NU * abs(d_0)
    assert {"case1", "case2", "case3", "case4", "U1", "U2", "U3", "degenerate"} <= seen, seen
    assert n_wolfe > 50
    # a known minimiser: phi = (a - 2)^2, every trial of a quadratic is exact from case 2 on
    q = lambda a: ((a - 2.0) ** 2, 2.0 * (a - 2.0))
    a, trials = R.line_search_mt(q, 4.0, -4.0, 5.0, 100.0, 1e-3)
    assert trials >= 1 and abs(a - 2.0) <= 0.9 * 2.0 and abs(q(a)[1]) <= R.NU * 4.0


def test_solve_step_is_the_pseudo_inverse():
    rng = np.random.default_rng(1)
    A = rng.normal(size=(6, 6)); H = A + A.T; g = rng.normal(size=6)
    assert np.allclose(R.solve_step(H, g), np.linalg.solve(H, -g))
    H[:, 5] = H[5, :] = 0.0
    d = R.solve_step(H, g)
    assert d[5] == 0 and np.allclose(H[:5, :5] @ d[:5], -g[:5])
    assert not R.solve_step(np.zeros((6, 6)), np.zeros(6)).any()
    assert np.isnan(R.solve_step(np.full((6, 6), np.nan), g)).all()


def test_align_on_the_small_scene_and_no_nan_reaches_p(small):
    T, tgt, src, prm = small
    guess = R.matrix_from_p(np.array([0.2, -0.15, 0.1, 0.02, -0.01, 0.03])).astype(np.float32)
    for ls in (1, 0):
        hist = []
        r = R.align(T, src, R.params(line_search=ls), guess, history=hist)
        assert np.isfinite(r["p"]).all() and r["converged"] == 1 and r["iters"] >= 2
        assert hist[-1][1] > hist[0][1]                              # the score went up
    far = R.matrix_from_p(np.array([500.0, 0, 0, 0, 0, 0])).astype(np.float32)
    r = R.align(T, src, prm, far)
    assert (r["converged"], r["iters"], r["n_evals"], r["n_pairs_last"]) == (1, 0, 1, 0)
    assert np.array_equal(r["T"], far)
    m, where = R.smallest_margin(T, src, prm, guess)
    assert 0 < m < np.inf and isinstance(where, str)
