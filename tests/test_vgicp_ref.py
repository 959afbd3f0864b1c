"""tests/vgicp_ref.py, the definition of lisreg_vgicp_*, against itself and against independent computations — no GPU:
the loop forms against the vector forms, the neighbour sets against scipy's kd-tree, the regularised covariances' eigenvalues, b and H
against central differences of the error, the SE(3) exponential against its series, every branch of the Levenberg-Marquardt loop on a
scripted problem, the scene's alignments and their decision margins, the structs and symbols of include/lisreg.h, the golden file."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vgicp_ref as R
from test_ndt import _header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vgicp", "vgicp_cases.npz")
SYMBOLS = ("lisreg_vgicp_default_params", "lisreg_vgicp_set_target", "lisreg_vgicp_align", "lisreg_vgicp_covariances",
           "lisreg_vgicp_get_voxels", "lisreg_vgicp_linearize")


@pytest.fixture(scope="module")
def now():
    """the golden cases made afresh: once, for the tests that read them"""
    return R.golden_cases()


def test_loop_form_equals_vector_form():
    prm = R.params()
    xyz, groups = R.planted_cloud(n_base=220)
    a, b = R.distributions_loops(xyz, prm), R.distributions(xyz, prm)
    assert np.array_equal(a["nbr"], b["nbr"])                                  # ties included: both forms order by (distance, index)
    assert np.array_equal(np.isinf(a["gap"]), np.isinf(b["gap"])) and np.allclose(a["gap"][np.isfinite(a["gap"])], b["gap"][np.isfinite(b["gap"])], rtol=0, atol=0)
    fin = a["nbr"][:, 0] >= 0
    assert np.isnan(b["C"][~fin]).all() and set(np.flatnonzero(~fin)) == set(groups["nan"])
    well = fin & (a["eig_gap"] >= 1e-3)
    assert np.abs(a["C"][well] - b["C"][well]).max() <= 1e-12 and np.allclose(a["eig_gap"][fin], b["eig_gap"][fin], rtol=0, atol=1e-9)
    for n in (20, 21, 65):
        x = R.small_cloud(n)
        assert np.array_equal(R.knn_loops(x, 20)[0], R.knn(x, 20)[0]), n
    with pytest.raises(ValueError):
        R.knn(R.small_cloud(19), 20)
    # one linearisation: the scene's target, 150 source points with the whole source's distributions
    W = R.world()
    S = dict(x=W["S"]["x"][:150], C=W["S"]["C"][:150], ok=W["S"]["ok"][:150])
    for T in R.lin_poses(W["guess"], W["T_true"]):
        for hess in (True, False):
            u, v = R.linearize_loops(W["T"], S, T, hess), R.linearize(W["T"], S, T, hess)
            assert u["n_pairs"] == v["n_pairs"]
            assert np.all(np.abs(u["out"] - v["out"]) <= 1e-12 * np.maximum(u["abs"], 1e-300)) and np.allclose(u["abs"], v["abs"], rtol=1e-12, atol=0)
    assert v["n_pairs"] == 0 and not v["out"].any()                           # the pose 100 m away


def test_neighbour_sets_equal_the_kd_trees_on_the_scene():
    from scipy.spatial import cKDTree
    W = R.world()
    for xyz, D in ((W["tgt"], W["T"]["dist"]), (W["src"], W["S"]["dist"])):
        x = xyz.astype(np.float64)
        _, idx = cKDTree(x).query(x, k=20)
        assert np.array_equal(np.sort(idx, 1), np.sort(D["nbr"], 1))
        assert (D["nbr"][:, 0] == np.arange(len(x))).all()                     # a point is its own nearest neighbour


def test_regularised_covariances_have_the_plane_eigenvalues():
    W = R.world()
    xyz, _ = R.planted_cloud()
    for C3 in (W["T"]["dist"]["C"], W["S"]["dist"]["C"], R.distributions(xyz, R.params())["C"]):
        C3 = C3[~np.isnan(C3).any((1, 2))]
        assert np.abs(C3 - np.transpose(C3, (0, 2, 1))).max() == 0
        assert np.abs(np.linalg.eigvalsh(C3) - np.array([1e-3, 1.0, 1.0])).max() <= 1e-12


def test_b_and_h_against_central_differences_of_the_error():
    W = R.world()
    T0 = W["guess"].astype(np.float64)
    pi, vi, _ = R.find_pairs(W["T"], W["S"], T0)
    pairs, Rl = (pi[::5], vi[::5]), T0[:3, :3]
    ev = R.linearize(W["T"], W["S"], T0, True, pairs=pairs)
    e0, b, H = R.unpack(ev["out"])

    def err(delta, means=None):
        return R.linearize(W["T"], W["S"], R.se3_exp(delta) @ T0, False, pairs=pairs, R_lin=Rl, means=means)["out"][0]
    # e over a fixed pair set with M frozen: its gradient at delta = 0 is 2 b
    h = 1e-5
    g = np.array([(err(h * np.eye(6)[k]) - err(-h * np.eye(6)[k])) / (2 * h) for k in range(6)])
    assert np.abs(g - 2 * b).max() <= 1e-6 * np.abs(ev["abs"][1:7]).max()
    # with every target mean moved onto its transformed point the residuals vanish and the second differences of e are 2 H exactly
    # (the curvature of exp() enters through d only)
    means = R.transform_points(T0, W["S"]["x"][pairs[0]])
    assert err(np.zeros(6), means) == 0.0
    h = 1e-3
    E = np.eye(6)
    H2 = np.array([[(err(h * (E[i] + E[j]), means) - err(h * (E[i] - E[j]), means) - err(h * (E[j] - E[i]), means) + err(-h * (E[i] + E[j]), means))
                    / (4 * h * h) for j in range(6)] for i in range(6)])
    assert np.abs(H2 - 2 * H).max() <= 1e-5 * np.abs(H).max()
    assert np.abs(H - H.T).max() == 0 and np.linalg.eigvalsh(H).min() > 0


def test_se3_exp_against_its_series():
    rng = np.random.default_rng(3)
    deltas = [np.zeros(6), np.r_[0.0499999, 0, 0, 1, 2, 3], np.r_[0, 0.0500001, 0, 1, 2, 3]]
    deltas += [rng.normal(0, s, 6) for s in (1e-9, 1e-6, 1e-3, 0.02, 0.03, 0.1, 0.5, 1.5) for _ in range(6)]
    for d in deltas:
        A = np.zeros((4, 4))
        A[:3, :3], A[:3, 3] = R.skew(d[:3]), d[3:]
        S, term = np.eye(4), np.eye(4)
        for n in range(1, 40):
            term = term @ A / n
            S = S + term
        E = R.se3_exp(d)
        assert np.abs(E - S).max() <= 2e-15 * max(1.0, np.abs(S).max()), d
        assert np.abs(E[:3, :3] @ E[:3, :3].T - np.eye(3)).max() <= 1e-15 and np.array_equal(E[3], [0, 0, 0, 1])


def _point_problem(wall):
    """a point-to-point problem (M = I) whose error function adds `wall` inside 0.05 m of the optimum's translation: steps into it are
    rejected whatever the model promises"""
    rng = np.random.default_rng(9)
    x = rng.uniform(-3, 3, (40, 3))
    T_opt = R.se3_exp(np.r_[0.02, -0.03, 0.05, 0.4, -0.2, 0.1])
    mu = R.transform_points(T_opt, x)

    def terms(T):
        xt = R.transform_points(T, x)
        d = mu - xt
        J = np.zeros((len(x), 3, 6))
        J[:, 0, 1], J[:, 0, 2], J[:, 1, 0], J[:, 1, 2], J[:, 2, 0], J[:, 2, 1] = -xt[:, 2], xt[:, 1], xt[:, 2], -xt[:, 0], -xt[:, 1], xt[:, 0]
        J[:, 0, 3] = J[:, 1, 4] = J[:, 2, 5] = -1.0
        return d, J

    def err(T):
        d, _ = terms(T)
        return float((d * d).sum()) + (wall if np.linalg.norm(T[:3, 3] - T_opt[:3, 3]) < 0.05 else 0.0), len(x)

    def lin(T):
        d, J = terms(T)
        return float((d * d).sum()), np.einsum("nia,ni->a", J, d), np.einsum("nia,nib->ab", J, J), len(x)
    return lin, err, T_opt


def test_lm_steps_reach_every_branch():
    prm = R.params(transformation_epsilon=1e-3, rotation_epsilon=1e-3)
    # no wall: Gauss-Newton steps, all accepted, lambda falls by 1/3 per step, converged
    lin, err, T_opt = _point_problem(0.0)
    mg = R.Margins()
    r = R.lm_optimise(lin, err, np.eye(4), prm, mg)
    assert r["converged"] == 1 and r["n_rejected"] == 0 and set(mg.log) == {"accepted"} and r["n_evals"] == 2 * r["iters"]
    assert np.abs(r["T"] - T_opt).max() <= 1e-6
    assert np.allclose(mg.lams[1:], np.array(mg.lams[:-1]) / 3.0, rtol=1e-12) and mg.lams[0] == 1e-9 * np.abs(np.diag(lin(np.eye(4))[2])).max()
    # a wall around the optimum: the full step is rejected, lambda grows by 2, 4, 8, ... within the iteration until a step stays outside
    lin, err, T_opt = _point_problem(1.0e3)
    mg = R.Margins()
    r = R.lm_optimise(lin, err, np.eye(4), R.params(transformation_epsilon=1e-3, rotation_epsilon=1e-3, lm_max_iterations=60), mg)
    assert "rejected" in mg.log and "accepted" in mg.log and r["converged"] == 1
    assert r["n_rejected"] == mg.log.count("rejected") + mg.log.count("rejected while converged") and r["n_evals"] == r["iters"] + len(mg.log)
    assert 0.05 <= np.linalg.norm(r["T"][:3, 3] - T_opt[:3, 3]) < 0.2                  # it stayed outside the wall
    # an error function that reports 1e-3 more than the linearisation's: near the optimum no step earns that much, a trial is rejected,
    # and once its step is short enough to count as converged the alignment stops there, converged
    lin0, err0, _ = _point_problem(0.0)
    mg2 = R.Margins()
    r2 = R.lm_optimise(lin0, lambda T: (err0(T)[0] + 1.0e-3, 40), np.eye(4), R.params(transformation_epsilon=1e-3, rotation_epsilon=1e-3, lm_max_iterations=60), mg2)
    assert mg2.log[-1] == "rejected while converged" and "accepted" in mg2.log and r2["converged"] == 1
    assert r2["n_rejected"] == mg2.log.count("rejected") + 1 and np.abs(r2["T"] - T_opt).max() <= 1e-3
    i = mg.log.index("rejected")
    run = 0
    while mg.log[i + run] == "rejected":
        run += 1
    assert run >= 2 and np.allclose(np.array(mg.lams[i + 1:i + run + 1]) / np.array(mg.lams[i:i + run]), 2.0 ** np.arange(1, run + 1), rtol=1e-12)
    # the same wall with two trials per iteration: the trials run out, the alignment ends unconverged where it was
    mg = R.Margins()
    r = R.lm_optimise(lin, err, np.eye(4), R.params(transformation_epsilon=1e-3, rotation_epsilon=1e-3, lm_max_iterations=2), mg)
    assert mg.log[-3:] == ["rejected", "rejected", "trials exhausted"] and r["converged"] == 0 and np.isfinite(r["T"]).all()
    # no pair at the start: nothing is solved; a system that is not positive definite ends the alignment without a NaN
    r = R.lm_optimise(lambda T: (0.0, np.zeros(6), np.zeros((6, 6)), 0), err, np.eye(4), prm)
    assert (r["converged"], r["iters"], r["n_evals"]) == (0, 0, 1) and np.array_equal(r["T"], np.eye(4))
    mg = R.Margins()
    r = R.lm_optimise(lambda T: (1.0, np.ones(6), -np.eye(6), 5), err, np.eye(4), prm, mg)
    assert mg.log == ["not positive definite"] and r["converged"] == 0 and np.array_equal(r["T"], np.eye(4))
    assert R.solve_damped(np.full((6, 6), np.nan), np.ones(6), 1.0) is None
    # a NaN rho (e' = NaN) is a rejection
    r = R.lm_optimise(lin, lambda T: (np.nan, 40), np.eye(4), R.params(lm_max_iterations=3), R.Margins())
    assert r["n_rejected"] == 3 and r["converged"] == 0 and np.array_equal(r["T"], np.eye(4))


def test_scene_alignments_and_their_margins(now):
    for (seed, trans, rot, eps), c, f in zip(R.ALIGN_CASES, now["align_counts"], now["align_fig"]):
        assert c[0] == 1, seed
        assert f[9] >= 10.0 * f[7], (seed, f[9], f[7])                        # ends at least ten times closer in translation
        assert f[5] >= 1e-6 and f[6] >= 1e-6, (seed, "a 20 / 21 neighbour gap under the bar")
        assert f[4] >= 1e-9, (seed, "a transformed point within 1e-9 m of a voxel face")
        assert f[2] >= 1e-6 and f[3] >= 1e-6, (seed, "a rho-sign or convergence comparison decided by less than 1e-6")
    assert [tuple(c[:4]) for c in now["align_counts"]] == [(1, 7, 23, 10), (1, 11, 29, 8), (1, 5, 17, 8), (1, 4, 8, 0)]
    W = R.world()
    assert W["T"]["dist"]["gap"].min() >= 1e-6 and np.nanmin(W["T"]["dist"]["eig_gap"]) >= 7e-3 and np.nanmin(W["S"]["dist"]["eig_gap"]) >= 1e-2
    assert list(now["scene_dims"]) == [23, 24, 14, 1821, 25401] and len(W["src"]) == 2939


def test_structs_match_the_header():
    import lisreg
    for name, mine, size in (("lisreg_vgicp_params", lisreg.VgicpParams, 56), ("lisreg_vgicp_info", lisreg.VgicpInfo, 20),
                             ("lisreg_vgicp_result", lisreg.VgicpResult, 168)):
        theirs = _header_struct(name)
        assert [(getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert [n.rstrip("_") for n, _ in mine._fields_] == [n for n, _ in theirs._fields_], name       # ("lambda" is a Python keyword)
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name


def test_library_exports_the_vgicp_symbols_and_defaults():
    import lisreg
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lisreg.ABI_SYMBOLS, s
        assert re.search(r"^\s*int\s+%s\s*\(" % s, hdr, re.M), s
    p = lisreg.vgicp_default_params()
    assert {n: getattr(p, n) for n, _ in p._fields_ if n != "reserved"} == R.DEFAULTS
    assert L.lisreg_vgicp_default_params(1, C.byref(p)) == lisreg.ERR_ARG and L.lisreg_vgicp_default_params(0, None) == lisreg.ERR_ARG
    assert L.lisreg_vgicp_set_target(None, 0, None, 0, 0, 0, C.byref(p), None) == lisreg.ERR_ARG
    assert L.lisreg_vgicp_align(None, 0, None, 0, 0, 0, C.byref(p), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_vgicp_covariances(None, None, 0, 0, 0, 20, None, None, 0.0) == lisreg.ERR_ARG
    for text in ("registration.cpp:156-187", "subMapOptmizationNode.cpp:2771", "lisreg_nearest", "tests/vgicp_ref.py"):
        assert text in hdr, text


def test_golden_file_regenerates_from_the_restatement(now):
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    assert sorted(now) == sorted(g.files)
    for k in g.files:
        a, b = g[k], now[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind in "iu":
            assert np.array_equal(a, b), k
    # doubles: LAPACK / BLAS builds may add in another order; everything else is the same arithmetic
    assert np.allclose(g["scene_means"], now["scene_means"], rtol=1e-13, atol=0)
    assert np.allclose(g["scene_cov6"], now["scene_cov6"], rtol=0, atol=1e-11)
    assert np.array_equal(g["lin_T"], now["lin_T"])
    assert np.all(np.abs(g["lin_out"] - now["lin_out"]) <= 1e-11 * g["lin_abs"]) and np.allclose(g["lin_abs"], now["lin_abs"], rtol=1e-11, atol=0)
    assert np.allclose(g["align_T"], now["align_T"], rtol=0, atol=1e-8)
    assert np.allclose(g["align_fig"][:, [0, 1]], now["align_fig"][:, [0, 1]], rtol=1e-6, atol=0)
    assert np.allclose(g["align_fig"][:, 2:], now["align_fig"][:, 2:], rtol=1e-3, atol=1e-12)
    pairs = g["lin_pairs"].reshape(3, len(R.LIN_SIZES), 2)
    assert (pairs[2] == 0).all() and (pairs[:2, -1] > 2900).all() and (pairs[:, :, 0] == pairs[:, :, 1]).all()
