"""tests/gicp_ref.py, the definition of lisreg_gicp_* (PCL's GICP), against itself and against independent
computations — no GPU: the moment form of f and its gradient against PCL's per-pair sums at every state the scene runs' BFGS visits,
the gradient against central differences, Fletcher's line search and the BFGS on scripted problems with known minimisers, a census of
every branch, the scene's alignments and their decision margins, the structs and symbols of include/lisreg.h, the golden file.

The bars of the first test are measured, not chosen: over the 1 243 states the five ALIGN_CASES runs visit, the moment form differs from
the per-pair float64 form by at most 6.36e-14 relative in f and 1.20e-8 of max |grad f| in the gradient (the gradient cancels near the
optimum in both forms: the worst visits are the last, where max |grad f| is below 1e-2 of its start; the per-pair form itself rounds
coordinates of tens of metres, 1e-14 m per residual).  The test asserts 100 times that — the room for another summation order (the
GPU's) and other scenes — and prints what it measures."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import gicp_ref as R
from test_ndt import _header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "gicp", "gicp_cases.npz")
SYMBOLS = ("lisreg_gicp_default_params", "lisreg_gicp_align", "lisreg_gicp_moments", "lisreg_gicp_inner")
MOMENT_F_BAR, MOMENT_GRAD_BAR = 100 * 6.36e-14, 100 * 1.20e-8         # 100 x the measured worst (see above); tests/test_gicp.py reuses the first
BAR_DECISION, BAR_SEARCH = 1e-6, 1e-9                                  # the family's bars (tests/test_fgicp_ref.py)
BAR_STABLE = 1e-7                                                      # a tenth of the 1e-6 tests/test_gicp.py allows the GPU


@pytest.fixture(scope="module")
def now():
    """the golden cases made afresh: once, for the tests that read them"""
    return R.golden_cases()


def test_moment_form_equals_pair_form_at_every_visited_state():
    worst_f = worst_g = 0.0
    n = 0
    for k, case in enumerate(R.ALIGN_CASES):
        r, W = R.case_run(k), R.world(*case[:3])
        for rec, xk, ps, visited in zip(r["recs"], r["xks"], r["pair_sets"], r["visits"]):
            for x in visited:
                f, g = R.fdf(rec, r["c"], xk, x, True)
                f2, g2 = R.pair_form(W["T"], W["S"], ps, r["G"], x)
                worst_f = max(worst_f, abs(f - f2) / abs(f2))
                worst_g = max(worst_g, float(np.abs(np.array(g) - g2).max() / np.abs(g2).max()))
                n += 1
    print(f"[gicp_ref] moment form against per-pair form at {n} visited states: worst {worst_f:.3e} relative in f, {worst_g:.3e} of max |grad|")
    assert n == sum(R.case_run(k)["n_evals"] for k in range(len(R.ALIGN_CASES))) > 1000
    assert worst_f <= MOMENT_F_BAR and worst_g <= MOMENT_GRAD_BAR


def test_moments_of_no_pairs_are_zero_and_theta_vanishes_at_the_iterate():
    W = R.world()
    far = R.lin_poses(W["guess"], W["T_true"])[2]
    rec, ab = R.moments(W["T"], W["S"], R.find_pairs(W["T"], W["S"], far, R.params()), far, R.centre(W["T"]))
    assert not rec.any() and not ab.any()
    x = [0.3, -0.2, 0.1, 0.02, -0.03, 0.05]
    th = R.theta_of(x, x, [1.0, 2.0, 3.0])                        # E = R R^T - I, d = E (c - t): a few roundings of sums of size 1, times |c - t| <= 6
    assert max(abs(th[4 * a + b]) for a in range(3) for b in range(3)) <= 4 * 2.3e-16 and max(abs(th[4 * a + 3]) for a in range(3)) <= 24 * 2.3e-16
    # X(x) is a rotation, applyState's order: yaw about z applied last
    Rm = np.array(R.euler_R([0, 0, 0, 0.0, 0.0, math.pi / 2])).reshape(3, 3)
    assert np.allclose(Rm @ [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], atol=1e-15)
    Rm = np.array(R.euler_R(x)).reshape(3, 3)
    assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(Rm) - 1.0) <= 1e-15
    rz = lambda a: np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
    ry = lambda a: np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    rx = lambda a: np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    assert np.allclose(Rm, rz(x[5]) @ ry(x[4]) @ rx(x[3]), atol=1e-15)


def test_gradient_against_central_differences():
    """on scripted states around the first and the last outer iterate of the first case: steps of 1e-1 .. 1e-5 of (0.3 m, 2 deg)"""
    r = R.case_run(0)
    rng = np.random.default_rng(3)
    worst = 0.0
    for it in (0, len(r["recs"]) - 1):
        rec, xk = r["recs"][it], r["xks"][it]
        for scale in (1e-1, 1e-3, 1e-5):
            x = [xk[j] + scale * (0.3 if j < 3 else math.radians(2.0)) * rng.uniform(-1, 1) for j in range(6)]
            f, g = R.fdf(rec, r["c"], xk, x, True)
            assert R.fdf(rec, r["c"], xk, x, False)[0] == f
            for j in range(6):
                h = 1e-5 if j < 3 else 1e-6
                xp, xm = list(x), list(x)
                xp[j] += h; xm[j] -= h
                num = (R.fdf(rec, r["c"], xk, xp, False)[0] - R.fdf(rec, r["c"], xk, xm, False)[0]) / (xp[j] - xm[j])
                worst = max(worst, abs(num - g[j]) / max(abs(v) for v in g))
    print(f"[gicp_ref] gradient against central differences: worst {worst:.3e} of max |grad|")
    # truncation h^2 f''' / 6 and rounding eps f / h of the difference quotient, against gradients of 0.1 .. 10: both below 1e-6
    assert worst <= 1e-6


# ---- scripted problems -----------------------------------------------------------------------------------------------------------
def _quartic_1d(x, want_grad):
    d = x[0] - 2.0
    return d * d + 0.1 * d ** 4 + 1.0, ([2.0 * d + 0.4 * d ** 3] if want_grad else None)


_A6 = None


def _quadratic_6d(x, want_grad):
    global _A6
    if _A6 is None:
        q = np.linalg.qr(np.random.default_rng(11).normal(size=(6, 6)))[0]
        _A6 = (q * np.array([1.0, 3.0, 10.0, 30.0, 100.0, 300.0])) @ q.T
    d = np.asarray(x) - np.arange(1.0, 7.0)
    return float(0.5 * d @ _A6 @ d), (list(_A6 @ d) if want_grad else None)


def _rosenbrock_6d(x, want_grad):
    f, g = 0.0, [0.0] * 6
    for i in range(5):
        a, b = x[i + 1] - x[i] * x[i], 1.0 - x[i]
        f += 100.0 * a * a + b * b
        g[i] += -400.0 * a * x[i] - 2.0 * b
        g[i + 1] += 200.0 * a
    return f, (g if want_grad else None)


def _flat_1d(x, want_grad):
    return 1e-20 * x[0] * x[0], ([2e-20 * x[0]] if want_grad else None)


def _wolfe_holds(out, prm):
    for f0, fp0, alpha, f, fp in out["wolfe"]:
        assert fp0 < 0 and alpha > 0
        assert f <= f0 + prm["rho"] * alpha * fp0 and abs(fp) <= -prm["sigma"] * fp0, (f0, fp0, alpha, f, fp)
    fs = [w[0] for w in out["wolfe"]] + [out["f"]]
    assert all(b <= a for a, b in zip(fs, fs[1:]))                          # f never rises over the accepted steps


def test_line_search_and_bfgs_on_scripted_problems():
    # (GSL's no-progress test is absolute, (a - alpha) f'(a) <= eps: slopes far below 1e-6 end a search that way, so 1e-6 is the tolerance)
    tight = R.params(gradient_tol=1e-6, max_inner_iters=500)
    mg = R.Margins()
    o = R.bfgs_minimise(_quartic_1d, [0.0], tight, mg)
    assert o["exit"] == R.EXIT_GRADIENT and abs(o["x"][0] - 2.0) <= 1e-6 and "linesearch:limit" not in mg.events
    _wolfe_holds(o, tight)
    o = R.bfgs_minimise(_quadratic_6d, [0.0] * 6, tight, mg)                # eigenvalues 1 .. 300: |x - x*| <= |g| / 1
    assert o["exit"] == R.EXIT_GRADIENT and np.abs(np.array(o["x"]) - np.arange(1.0, 7.0)).max() <= 1e-6
    _wolfe_holds(o, tight)
    o = R.bfgs_minimise(_rosenbrock_6d, [-1.2, 1.0, -1.2, 1.0, -1.2, 1.0], R.params(gradient_tol=1e-4, max_inner_iters=5000), mg)
    assert o["exit"] == R.EXIT_GRADIENT and o["f"] <= 1e-8 and np.abs(np.array(o["x"]) - 1.0).max() <= 1e-3 and "linesearch:limit" not in mg.events
    _wolfe_holds(o, tight)
    assert o["n_f"] + o["n_df"] >= 2 * o["iters"]
    # the iteration cap: the same problem, 3 steps
    o3 = R.bfgs_minimise(_rosenbrock_6d, [-1.2, 1.0, -1.2, 1.0, -1.2, 1.0], R.params(gradient_tol=1e-4, max_inner_iters=3), mg)
    assert o3["exit"] == R.EXIT_CAP and o3["iters"] == 3
    # no progress: a start at the minimiser (a zero gradient), and a function whose slopes are below the rounding of the test
    flat = R.Margins()
    o0 = R.bfgs_minimise(_quartic_1d, [2.0], tight, flat)
    assert o0["exit"] == R.EXIT_NOPROGRESS and o0["x"] == [2.0] and o0["iters"] == 1 and flat.events == {"step:degenerate": 1, "inner:noprogress": 1}
    of = R.bfgs_minimise(_flat_1d, [1.0], tight, flat)
    assert of["exit"] == R.EXIT_NOPROGRESS and flat.events.get("section:noprogress") == 1
    assert of["x"] == [1.0] or of["f"] <= 1e-20                             # a NoProgress step leaves x where the step began
    # interpolate: the minimiser of the cubic through two points with slopes, clipped to the interval it is given
    assert abs(R.interpolate(0.0, 1.0, -2.0, 2.0, 1.0, 2.0, 0.1, 1.9, 3) - 1.0) <= 1e-15          # (x - 1)^2: symmetric data
    assert R.interpolate(0.0, 1.0, -2.0, 2.0, 1.0, 2.0, 1.2, 1.9, 3) == 1.2                         # the minimiser lies left of the interval
    assert abs(R.interpolate(0.0, 1.0, -2.0, 2.0, 1.0, math.nan, 0.1, 1.9, 3) - 1.0) <= 1e-15      # no slope at b: the quadratic
    assert R.solve_quadratic(1.0, -3.0, 2.0) == (2, 1.0, 2.0) and R.solve_quadratic(0.0, 2.0, -4.0)[:2] == (1, 2.0)
    assert R.solve_quadratic(1.0, 0.0, 1.0)[0] == 0 and R.solve_quadratic(0.0, 0.0, 1.0)[0] == 0 and R.solve_quadratic(1.0, 2.0, 1.0) == (2, -1.0, -1.0)


def test_census_every_branch_occurs():
    """the project's habit (tests/feature_sweeps.py): a branch no test takes is a branch nobody has checked"""
    seen = {}
    for k in range(len(R.ALIGN_CASES)):
        for name, cnt in R.case_run(k)["events"].items():
            seen[name] = seen.get(name, 0) + cnt
    W = R.world()
    capped = R.align(W["T"], W["S"], R.params(max_iters=2), W["guess"])
    assert (capped["converged"], capped["iters"], capped["n_rounds"]) == (1, 2, 2) and capped["last_delta"] >= 1.0
    far = np.array(W["guess"], np.float32)
    far[0, 3] += 100.0
    none = R.align(W["T"], W["S"], R.params(), far)
    assert (none["converged"], none["iters"], none["n_rounds"], none["n_pairs_last"], none["inner_exit"]) == (0, 0, 1, 0, -1)
    assert np.array_equal(none["T"], far.astype(np.float64))
    mg = R.Margins()
    R.bfgs_minimise(_flat_1d, [1.0], R.params(), mg)
    R.bfgs_minimise(_rosenbrock_6d, [-1.2, 1.0, -1.2, 1.0, -1.2, 1.0], R.params(gradient_tol=1e-4, max_inner_iters=5000), mg)
    for events in (capped["events"], none["events"], mg.events):
        for name, cnt in events.items():
            seen[name] = seen.get(name, 0) + cnt
    print("[gicp_ref] census:", dict(sorted(seen.items())))
    for name in ("inner:gradient", "inner:cap", "inner:noprogress", "bracket:rho", "bracket:sigma", "bracket:slope", "bracket:extend",
                 "section:shrink", "section:sigma", "section:flip", "section:advance", "section:noprogress", "outer:delta",
                 "outer:max_iters", "outer:few_pairs"):
        assert seen.get(name, 0) >= 1, name
    assert "linesearch:limit" not in seen                                   # no scene run spends its 100 trials


def test_scene_alignments_and_their_margins(now):
    assert len(R.ALIGN_CASES) >= 5 and R.ALIGN_CASES[0][3] == R.DEFAULTS["transformation_epsilon"] == 1e-6
    for k, ((seed, trans, rot, eps), c, f) in enumerate(zip(R.ALIGN_CASES, now["align_counts"], now["align_fig"])):
        dec = R.case_run(k)["decisions"]
        print(f"[gicp_ref] seed {seed} eps {eps}: counts {c.tolist()}, delta {f[1]:.3f}, conv {f[2]:.2e} nn {f[3]:.2e} cut {f[4]:.2e} "
              f"decisions {({a: float('%.2e' % b) for a, b in dec.items()})} f comparisons decided by >= {f[6]:.2e} eps |f|, "
              f"{1e3 * f[7]:.2f} mm from the truth (guess {1e3 * f[9]:.0f} mm)")
        assert c[0] == 1 and c[4] == c[1], seed                                # converged; one round per outer iteration
        assert f[9] >= 10.0 * f[7], (seed, f[9], f[7])                         # ends at least ten times closer in translation
        assert f[3] >= BAR_SEARCH and f[4] >= BAR_SEARCH, (seed, "a nearest neighbour or a cut-off decided by less than 1e-9")
        assert f[2] >= BAR_DECISION and min(dec.values()) >= BAR_DECISION and f[5] == min(dec.values()), (seed, dec)
        assert f[6] >= 1e3, (seed, "an f comparison within a thousand roundings of f")
    # the reference's own epsilon 1e-6 does NOT run its 30 iterations on these scenes: the inner loops end on gradient_tol after a few
    # steps once the pairs settle, and the 4th (3rd) outer iteration moves the state by 0.79e-6 (0.80e-6).  The looser epsilons end the
    # same trajectories earlier (case 4 is case 0 cut after its 3rd iteration)
    counts = [tuple(int(v) for v in c[:7]) for c in now["align_counts"]]
    assert counts == [(1, 4, 53, 261, 4, 2939, 0), (1, 4, 47, 232, 4, 2934, 0), (1, 3, 34, 168, 3, 2936, 0), (1, 5, 66, 337, 5, 2939, 0),
                      (1, 3, 50, 245, 3, 2939, 0)], counts
    assert all(f[1] < 1.0 for f in now["align_fig"])                           # every case ends by delta < 1


@pytest.mark.parametrize("case", range(len(R.ALIGN_CASES)))
def test_alignment_cases_are_stable_under_the_rounding_of_their_moments(case):
    """the bar a case must pass before a GPU is compared with it: every sum of every record moved by a random share of PERTURB_EPS of
    its sum of |term| (what another summation order and another rounding of M do), twice — the same counts, the pose within 1e-7
    and the error within 1e-7 relative.  (The family's 0.3 m / 2 degree guesses end 4e-5 .. 4e-4 apart: gicp_ref.ALIGN_CASES' comment.)"""
    seed, trans, rot, eps = R.ALIGN_CASES[case]
    W, base = R.world(seed, trans, rot), R.case_run(case)
    key = lambda r: tuple(int(r[k]) for k in ("converged", "iters", "inner_iters", "n_evals", "n_rounds", "n_pairs_last", "inner_exit"))
    for s in (0, 1):
        r = R.align(W["T"], W["S"], R.params(transformation_epsilon=eps), W["guess"], perturb=(R.PERTURB_EPS, s))
        dT, de = float(np.abs(r["T"] - base["T"]).max()), abs(r["error"] - base["error"]) / base["error"]
        print(f"[gicp_ref] seed {seed} eps {eps}, moments perturbed by {R.PERTURB_EPS} (draw {s}): |dT| {dT:.2e}, error off by {de:.2e}, counts {key(r)}")
        assert key(r) == key(base) and dT <= BAR_STABLE and de <= BAR_STABLE, (seed, s, dT, de)


def test_structs_match_the_header():
    import lisreg
    for name, mine, size in (("lisreg_gicp_params", lisreg.GicpParams, 104), ("lisreg_gicp_result", lisreg.GicpResult, 176)):
        theirs = _header_struct(name)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name


def test_library_exports_the_gicp_symbols_and_defaults():
    import lisreg
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lisreg.ABI_SYMBOLS, s
        assert re.search(r"^\s*int\s+%s\s*\(" % s, hdr, re.M), s
    assert "lisreg_gicp_set_target" not in hdr and not hasattr(L, "lisreg_gicp_set_target")         # the target is a FastGICP slot
    for kind in (0, 1):
        p = lisreg.gicp_default_params(kind)
        want = R.params(kind)
        want.pop("plane_epsilon")
        assert {n: getattr(p, n) for n, _ in p._fields_} == want, kind
    assert R.params(0) == dict(R.DEFAULTS, plane_epsilon=1e-3) and R.params(1)["transformation_epsilon"] == 1e-4
    f = lisreg.fgicp_default_params()
    assert (p.k_correspondences, p.gicp_epsilon) == (f.k_correspondences, f.plane_epsilon)          # a GICP target is a FastGICP target
    assert lisreg.gicp_default_params(transformation_epsilon=5e-4).transformation_epsilon == 5e-4
    with pytest.raises(AttributeError):
        lisreg.gicp_default_params(lm_max_iterations=3)
    assert L.lisreg_gicp_default_params(2, C.byref(p)) == lisreg.ERR_ARG and L.lisreg_gicp_default_params(0, None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_align(None, 0, None, 0, 0, 0, C.byref(p), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_moments(None, 0, None, 0, 0, 0, C.byref(p), None, None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_inner(None, None, None, C.byref(p), None, None, None) == lisreg.ERR_ARG
    for text in ("registration.cpp:137-146", "subMapOptmizationNode.cpp:2765-2769", "lisreg_nearest", "tests/gicp_ref.py", "lisreg_fgicp_set_target"):
        assert text in hdr[hdr.index("§7q"):hdr.index("loop-closure candidate detection: FEPSC")], text


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
    assert np.array_equal(g["mom_T"], now["mom_T"]) and np.array_equal(g["centre"], now["centre"])
    assert np.all(np.abs(g["mom_rec"] - now["mom_rec"]) <= 1e-11 * g["mom_abs"]) and np.allclose(g["mom_abs"], now["mom_abs"], rtol=1e-11, atol=0)
    assert np.allclose(g["align_T"], now["align_T"], rtol=0, atol=1e-8)
    assert np.allclose(g["align_fig"][:, :2], now["align_fig"][:, :2], rtol=1e-5, atol=0)
    assert np.allclose(g["inner_x1"], now["inner_x1"], rtol=0, atol=1e-8) and g["inner_rec"].shape == (19, 74)
    assert list(g["mom_rec"][:, 73]) == [2939.0, 2939.0, 0.0] and not g["mom_rec"][2].any()
