"""The corner fit's closed-form eigen-solver on the device (`eigen_top_closed` in lisreg_assoc.hip, with its hand-back to the cyclic
Jacobi), through `lisreg_test_fit_models`: kind 0 = `corner_model` + `corner_eval` as the correspondence kernel inlines them, kind 2 = the
solver's own outputs (two eigenvalues, direction, which of the two solvers produced them).  tests/corner_eigen_model.py is the numpy
restatement and derives the bound used here.

Cases (<= 2 000 neighbourhoods each, seeded): the three distance rings of test_fit_device.py's line test (10 / 100 / 1 000 m), l0 / l1
straddling line_ratio by +-1e-6 ... +-1e-2 relative, two equal largest eigenvalues (regular pentagons), two equal smallest (a line with
the same spread in both directions across it), exactly collinear points, five identical points, axis-aligned lines (a scatter matrix that
is already diagonal), coordinates scaled by 1e-3 and 1e3.

Criteria:
  * accept flag against the oracle: no more differences than the production build of the commit before this solver (cyclic Jacobi for
    every lane) shows on the same inputs — PARENT_FLAG_DIFFS, measured on an MI355X with that build;
  * point-to-line distance at the query against the oracle within the bars of test_fit_device.py (2e-5 / 3e-5 / 4e-4 m by ring; the
    constructed cases sit at 10 m: 2e-5);
  * eigenvalues against numpy's float64 `eigh` of the float32 scatter matrix within the derived bound: (158 + 16) u T for a certified
    closed-form lane, (128 + 16) u T for a Jacobi lane (u = 2^-24, T = trace; the 16 u T cover forming the matrix with and without FMA
    contraction: six sums of five products, <= 5 u T per entry); direction within 2 * that bound / (l0 - l1) where the neighbourhood is
    accepted (l0 - l1 >= T / 8);
  * the exact-arithmetic build is untouched: its flags and coefficients equal the oracle's to the bit, and it never reports the closed form.
"""
import numpy as np
import pytest

from corner_eigen_model import K_DELTA_CF, K_DELTA_JACOBI, U, eigh64, scatter
from helpers import copy_params
from test_fit_device import dist_and_normal, oracle_corner

f32 = np.float32

# accept flags that differ from the oracle's in the production build of the parent commit (cyclic Jacobi only), same seeded inputs
PARENT_FLAG_DIFFS = {"ring10": 0, "ring100": 0, "ring1000": 0, "straddle": 5, "equal_top": 0, "equal_low": 0, "collinear": 0,
                     "identical": 0, "diagonal": 0, "scale1e-3": 550, "scale1e3": 0}
DIST_BAR = {"ring10": 2e-5, "ring100": 3e-5, "ring1000": 4e-4, "straddle": 2e-5, "equal_low": 2e-5, "collinear": 2e-5, "diagonal": 2e-5}

T5 = np.array([-2.0, -1.0, 0.0, 1.0, 2.0])                  # along the line; W1, W2 across it: all three orthogonal to each other and to 1
W1 = np.array([1.0, -1.0, 0.0, -1.0, 1.0]); W2 = np.array([1.0, -2.0, 0.0, 2.0, -1.0]) * np.sqrt(0.4)       # |W1|^2 = |W2|^2 = 4, |T5|^2 = 10


def _frame(rng):
    d = rng.normal(0, 1, 3); d /= np.linalg.norm(d)
    a = np.cross(d, rng.normal(0, 1, 3)); a /= np.linalg.norm(a)
    return d, a, np.cross(d, a)


def _centre(rng, dist):
    c = rng.normal(0, 1, 3)
    return c * dist / np.linalg.norm(c)


def ring(dist, n=1500, seed=5):
    """the neighbourhoods of test_device_line_fit_matches_oracle: one generator drawn ring after ring"""
    rng = np.random.default_rng(seed)
    for dd in (10.0, 100.0, 1000.0):
        nb = np.zeros((n, 5, 3), f32); q = np.zeros((n, 3), f32)
        for i in range(n):
            centre = rng.normal(0, 1, 3); centre *= dd / np.linalg.norm(centre)
            d = rng.normal(0, 1, 3); d /= np.linalg.norm(d)
            off = np.cross(d, rng.normal(0, 1, 3)); off /= np.linalg.norm(off)
            p = centre + np.outer(rng.uniform(-0.6, 0.6, 5), d) + rng.normal(0, 0.01, (5, 3))
            nb[i] = p.astype(f32); q[i] = (centre + 0.08 * off + 0.1 * d).astype(f32)
        if dd == dist:
            return nb, q
    raise ValueError(dist)


def shaped(seed, n, k1, k2, dist=10.0, step=0.15, axis_aligned=False):
    """centre + step * (T5 d + k1[i] W1 a + k2[i] W2 b): scatter eigenvalues step^2 / 5 * (10, 4 k1^2, 4 k2^2) before rounding to float32"""
    rng = np.random.default_rng(seed)
    nb = np.zeros((n, 5, 3), f32); q = np.zeros((n, 3), f32)
    for i in range(n):
        d, a, b = (np.eye(3)[rng.permutation(3)] if axis_aligned else _frame(rng))
        c = np.round(_centre(rng, dist) * 64) / 64 if axis_aligned else _centre(rng, dist)
        p = c + step * (np.outer(T5, d) + k1[i] * np.outer(W1, a) + k2[i] * np.outer(W2, b))
        nb[i] = p.astype(f32); q[i] = (c + 0.08 * a + 0.05 * d).astype(f32)
    return nb, q


def build_cases():
    cases = {f"ring{int(d)}": ring(d) for d in (10.0, 100.0, 1000.0)}
    # l0 / l1 = 3 (1 + e): 4 k1^2 = 10 / (3 (1 + e)); the third eigenvalue between 0 and l1
    rng = np.random.default_rng(11)
    n = 2000
    e = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6, -2, n)
    k1 = np.sqrt(10.0 / (12.0 * (1.0 + e)))
    cases["straddle"] = shaped(12, n, k1, k1 * rng.uniform(0.0, 1.0, n))
    # regular pentagons of radius 0.3 m: l0 = l1, l2 = 0
    rng = np.random.default_rng(13)
    nb = np.zeros((500, 5, 3), f32); q = np.zeros((500, 3), f32)
    ang = 2 * np.pi * np.arange(5) / 5
    for i in range(500):
        d, a, b = _frame(rng); c = _centre(rng, 10.0)
        nb[i] = (c + 0.3 * (np.outer(np.cos(ang), a) + np.outer(np.sin(ang), b))).astype(f32); q[i] = (c + 0.05 * d).astype(f32)
    cases["equal_top"] = (nb, q)
    rng = np.random.default_rng(14)
    k = 10.0 ** rng.uniform(-4, -0.5, 1000)
    cases["equal_low"] = shaped(15, 1000, k, k)
    # exactly collinear in float32: multiples of 1/64 throughout
    rng = np.random.default_rng(16)
    nb = np.zeros((500, 5, 3), f32); q = np.zeros((500, 3), f32)
    for i in range(500):
        c = np.round(_centre(rng, 10.0) * 64) / 64; d = rng.integers(-8, 9, 3) / 64.0
        if not d.any():
            d[0] = 1 / 64.0
        nb[i] = (c + np.outer(rng.permutation(np.arange(-2, 3)) * 2.0, d)).astype(f32); q[i] = (c + [0.05, 0.03, -0.04]).astype(f32)
    cases["collinear"] = (nb, q)
    cases["identical"] = (np.tile(np.array([[3.0, 4.0, 5.0]], f32), (64, 5, 1)), np.tile(np.array([[3.0, 4.0, 5.05]], f32), (64, 1)))
    rng = np.random.default_rng(17)
    cases["diagonal"] = shaped(18, 600, np.where(np.arange(600) < 200, 0.0, 10.0 ** rng.uniform(-3, -0.3, 600)),
                               np.where(np.arange(600) < 400, 0.0, 10.0 ** rng.uniform(-3, -0.3, 600)), step=0.125, axis_aligned=True)
    nb, q = cases["ring10"]
    for name, s in (("scale1e-3", 1e-3), ("scale1e3", 1e3)):
        cases[name] = ((nb[:1000].astype(np.float64) * s).astype(f32), (q[:1000].astype(np.float64) * s).astype(f32))
    return cases


@pytest.fixture(scope="module")
def cases():
    return build_cases()


def run_case(ctx, oc, lisreg, nb, q):
    po = oc.default_params(1); pl = copy_params(po, lisreg.Params)
    dev = ctx.test_fit_models(0, nb, q, pl); eig = ctx.test_fit_models(2, nb, q, pl)
    ex = ctx.test_fit_models(0, nb, q, pl, exact=True); ex_eig = ctx.test_fit_models(2, nb, q, pl, exact=True)
    cfo, oko = oracle_corner(oc, nb, q, po)
    return dict(dev=dev, eig=eig, ex=ex, ex_eig=ex_eig, cfo=cfo, oko=oko, ratio=float(po.line_ratio))


NAMES = ["ring10", "ring100", "ring1000", "straddle", "equal_top", "equal_low", "collinear", "identical", "diagonal", "scale1e-3", "scale1e3"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_corner_eigen_case(gpu_ctx, oracle, cases, name):
    """Measured on an MI355X, accept flags differing from the oracle's, PARENT build (cyclic Jacobi only) / this build: rings 0 / 0, 0 / 0,
    0 / 0; straddle 5 / 5; equal_top, equal_low, collinear, identical, diagonal, scale1e3 0 / 0; scale1e-3 550 / 550 (scatter entries of
    1e-7 m^2 are under cv::eigen's FLT_EPSILON pivot threshold: the reference does not rotate there, neither build follows it).  Parent and
    this build agree lane for lane.  Worst eigenvalue error 8.1 u T (bound 174 / 144), direction 2.8e-7 off eigh64's, point-to-line
    distance against the oracle 3.1e-6 / 1.3e-5 / 8.2e-5 m by ring: profiles/r07_corner_eigen.md section 3."""
    import lisreg
    nb, q = cases[name]
    r = run_case(gpu_ctx, oracle, lisreg, nb, q)
    dev, eig, oko = r["dev"], r["eig"], r["oko"]
    n = len(nb)
    closed = eig[:, 5] == 1
    # --- accept flag against the oracle, capped by the parent build's count
    diff = int((dev[:, 9] != oko).sum())
    print(f"{name}: {n} neighbourhoods, closed form on {int(closed.sum())}, accept flags differ from the oracle's in {diff} (parent build: {PARENT_FLAG_DIFFS[name]})")
    assert np.array_equal(dev[:, 9], eig[:, 9])
    # --- eigenvalues (and direction) against float64 eigh of the float32 scatter matrix
    _, a = scatter(nb)
    t0, t1, vt = eigh64(a)
    T = (a[0].astype(np.float64) + a[3] + a[5])
    bound = np.where(closed, K_DELTA_CF + 16, K_DELTA_JACOBI + 16) * U * T
    e0 = np.abs(eig[:, 0] - t0); e1 = np.abs(eig[:, 1] - t1)
    pos = T > 0
    if pos.any():
        print(f"    |l0 - eigh64| max {np.max(e0[pos] / (U * T[pos])):.1f} u T, |l1 - eigh64| max {np.max(e1[pos] / (U * T[pos])):.1f} u T "
              f"(bound {K_DELTA_CF + 16:.0f} closed form / {K_DELTA_JACOBI + 16:.0f} Jacobi)")
    if closed.any():
        print(f"    closed-form direction: | |v| - 1 | max {np.abs(np.linalg.norm(eig[closed, 2:5].astype(np.float64), axis=1) - 1).max() / U:.2f} u (bound 4)")
    lam_ok = eig[:, 6] == 1
    sep = lam_ok & (t0 - t1 >= T / 8) & pos
    if sep.any():
        sin_ang = np.linalg.norm(np.cross(eig[sep, 2:5].astype(np.float64), vt[sep]), axis=1)
        print(f"    direction (accepted by the ratio test): sin(angle to eigh64's) max {sin_ang.max():.2e}, bound's max {(2 * bound[sep] / (t0 - t1)[sep]).max():.2e}")
    # --- point-to-line distance against the oracle
    both = (dev[:, 9] == 1) & (oko == 1)
    if name in DIST_BAR and both.any():
        d_dev, _ = dist_and_normal(dev[:, 5:9]); d_orc, _ = dist_and_normal(r["cfo"])
        e = np.abs(d_dev - d_orc)[both]
        print(f"    point-to-line distance at the query, {int(both.sum())} accepted by both: max |device - oracle| {e.max():.2e} (bar {DIST_BAR[name]:.0e})")
    assert diff <= PARENT_FLAG_DIFFS[name], (diff, PARENT_FLAG_DIFFS[name])
    assert (e0 <= bound).all() and (e1 <= bound).all(), (np.max(e0[pos] / (U * T[pos])), np.max(e1[pos] / (U * T[pos])))
    if sep.any():
        assert (sin_ang <= 2 * bound[sep] / (t0 - t1)[sep]).all()
    if closed.any():
        # the closed form's direction is a unit vector to 4 u, which its bound relies on: 3 u on the three-term sum of squares (1.5 u after
        # the root), 2 u for the 1-ulp reciprocal square root, 0.5 u for the products (the Jacobi's, eighteen rotations on, is not held to that)
        assert np.abs(np.linalg.norm(eig[closed, 2:5].astype(np.float64), axis=1) - 1).max() <= 4 * U
    if name in DIST_BAR:
        assert both.sum() >= (0.9 * n if name.startswith("ring") else 1)
        assert e.max() <= DIST_BAR[name]
    # --- what the cases are for
    if name.startswith("ring") or name in ("equal_low", "collinear", "diagonal"):
        assert closed.mean() >= 0.99 and lam_ok.mean() >= 0.99                    # lines: certified and passed
    if name == "equal_top":
        assert not lam_ok.any()
    if name == "identical":
        assert not closed.any() and not lam_ok.any() and (eig[:, 0] == 0).all() and (eig[:, 1] == 0).all()      # T = 0: the Jacobi's zeros
    if name == "straddle":
        # relative distance of l0 / l1 from the ratio, from float64: lanes inside the guard band ran the Jacobi, lanes well outside did not
        rel = np.abs(t0 / t1 / r["ratio"] - 1)
        assert not closed[rel < 1e-5].any() and closed[rel > 1e-3].all()
        assert (rel < 1e-5).sum() >= 100 and (rel > 1e-3).sum() >= 100
    # --- the exact-arithmetic build IS the oracle, and has no closed form
    ex = r["ex"]
    assert np.array_equal(ex[:, 9].astype(np.int32), oko)
    acc = oko == 1
    assert np.array_equal(ex[acc, 5:9].view(np.uint32), r["cfo"][acc].view(np.uint32))
    assert not (r["ex_eig"][:, 5] == 1).any()
