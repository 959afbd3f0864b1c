"""The definition of lisreg_gicp_* : PCL's GeneralizedIterativeClosestPoint (Segal et al. 2009, with PCL's BFGS optimiser), restated in
Python float64.

select_registration_method("GICP") (src/core/registration.cpp:137-146 of the reference: max correspondence distance 10, 30 iterations,
transformation epsilon 1e-6, Euclidean fitness epsilon 1e-3, RANSAC 0) is the fifth loop-closure verifier the reference names.  PCL's
source is not available to this project, so this file restates gicp.hpp / bfgs.h (= GSL's vector_bfgs2 and its linear_minimize.c) from
the paper and from memory, on top of fgicp_ref / vgicp_ref (distributions, search, find_pairs, margins, scenes).  What is written here
is the definition the GPU code is tested against — it is not "PCL's".

Readings picked (each one a possible departure from the PCL a user has installed):
  * distributions: k_correspondences 20 and gicp_epsilon 1e-3 are vgicp_ref.distributions with plane_epsilon = gicp_epsilon (eigenvalues
    replaced by 1, 1, epsilon), so a GICP target is a FastGICP target (PCL computes the covariance in one pass and multiplies U diag V^T
    of an SVD; the same matrix up to rounding);
  * the state is x = (tx, ty, tz, roll, pitch, yaw); X(x) is applyState's matrix, R = Rz(yaw) Ry(pitch) Rx(roll), translation x[0:3];
    the pose of outer iteration k is T_k = X(x_k) G with G the float guess widened to double; x_0 = 0 and x is carried from one outer
    iteration to the next (PCL reads x back from its matrix with atan2 / asin at every outer iteration: the same numbers up to rounding);
  * outer loop (computeTransformation): pairs and M_i = (C_b + R_k C_a R_k^T)^-1 at T_k by fgicp_ref.find_pairs — in DOUBLE, ties to the
    lower index, strict cut-off (PCL transforms and searches in float with a kd-tree, whose tie order is unspecified); fewer than 4 pairs
    is PCL's "need at least 4 points" throw: converged = 0 and the pose of that iteration's start; otherwise the inner minimisation from
    x_k; delta = max over the entries of |X(x_k) - X(x_k+1)|, rotation entries scaled by 1 / rotation_epsilon (2e-3), translation
    entries by 1 / transformation_epsilon; the loop stops when nr_iterations >= max_iters or delta < 1 and BOTH set converged = 1 —
    PCL 1.8's behaviour, which the reference's ROS Melodic install implies (later releases report the iteration cap as not converged);
  * inner minimisation (BFGS<> of bfgs.h = gsl_multimin_fdfminimizer_vector_bfgs2): the first direction is -g / |g|; a step's first
    trial is step_size (0.01) on the first step and min(1, 2 max(-delta_f, 10 eps |f0|) / -fp0) afterwards; Fletcher's line search
    (bracketing, then sectioning, `interpolate` of order 3 with gsl_poly_solve_quadratic) with rho 0.01, sigma 0.01, tau1 9, tau2 0.05,
    tau3 0.5; ONE counter runs through both loops, as GSL's `minimize` is remembered: at most 100 trials of bracketing and sectioning
    together, which keeps both limits of 100; the direction update is the memoryless p = g - A dx - B dg, renormalised and sign-fixed;
    testGradient(1e-2) (|g| < 1e-2) after every step; max_inner_iterations 20; NoProgress, Success or the iteration cap accept x (a
    NoProgress step leaves x where the step began);
  * the function BFGS sees is f(x) = (1/m) sum (X(x) p_i - q_i)^T M_i (X(x) p_i - q_i) with p_i = G a_i — and its DEFINITION here is the
    moment form below, an exact quadratic in the 12 entries of (R, t); PCL's per-pair sums (pair_form) are kept beside it as an
    independent check and are never the definition;
  * the Euler derivatives are computeRDerivative's, chained through theta(x);
  * defaults, kind 0: the reference's block plus PCL's defaults; kind 1: the settings of src/node/subMapOptmizationNode.cpp:2765-2769
    read for GICP (the commented :2764 puts a GICP object under them): transformation epsilon 1e-4, the rest the same.

The moments.  With T_k fixed, x'_i = T_k a_i, c = (b0 + b1) / 2 the centre of the target's finite bounding box (in double from the float
corners), y_i = x'_i - c, yt_i = (y_i, 1), r_i = x'_i - b_i:  X(x) p_i - q_i = r_i + E y_i + d with E = R(x) R(x_k)^T - I and
d = E (c - t_k) + (t(x) - t_k), t_k = x_k[0:3].  Theta = [E | d] (3 x 4), so  m f = c0 + 2 sum g[a][b] Theta[a][b] + sum Theta[a][b]
S[(a, a')][(b, b')] Theta[a'][b'].  The record of one outer iteration is 74 doubles:
    rec[0]              c0 = sum r^T M r
    rec[1 + 4 a + b]    g[a][b] = sum (M r)[a] yt[b]                                  a < 3, b < 4
    rec[13 + 10 p + q]  S[p][q] = sum M[P6[p]] yt[Q10[q][0]] yt[Q10[q][1]]             P6 = xx xy xz yy yz zz, Q10 = 00 01 02 03 11 12 13 22 23 33
    rec[73]             the pair count m
Every term is a displacement about the current pose: nothing cancels against coordinates.

A run is only as reproducible as its inner minimisations are stable: ALIGN_CASES' comment says what that means for the scenes.

Margins of a run (the smallest over the run, kept in a Margins): nn_gap and cut_gap of fgicp_ref; conv = |delta - 1|; and one per
comparison the optimiser branches on, each the distance between the two sides RELATIVE TO THE SIZE OF WHAT THE TEST WEIGHS: rho
(f(alpha) > f0 + rho alpha fp0) and prev (f(alpha) >= f(alpha_prev) / f(a)) compare CHANGES of f along the line, so their scale is the
largest of |f(alpha) - f0|, |f(other) - f0| and |alpha fp0| — not |f|: a converging minimiser's changes of f vanish against f itself,
and f0 is common to both sides; sigma (|f'(alpha)| <= -sigma fp0) and sign (f'(alpha) >= 0, and the sectioning's sign test) are
relative to |fp0|; noprog ((a - alpha) f'(a) <= eps) to |(b - a) f'(a)|; grad (|g| < gradient_tol) to the larger side.  f_ulps says
what the f comparisons leave out: the smallest |lhs - rhs| of a rho or prev test in units of eps |f0|, the rounding of ONE value of f —
the two sides are computed from the same 74 doubles, so a device record that differs in its last bits moves them by a few such units.
log keeps what became of every trial."""
import math

import numpy as np

import fgicp_ref as F
import vgicp_ref as V
from fgicp_ref import find_pairs, world, small_cloud, pose_error, prepare_source, build_target, transform_points  # noqa: F401

DBL_EPSILON = 2.220446049250313e-16
N_REC = 74
P6 = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
Q10 = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3))
SYM3 = ((0, 1, 2), (1, 3, 4), (2, 4, 5))
SYM4 = ((0, 1, 2, 3), (1, 4, 5, 6), (2, 5, 7, 8), (3, 6, 8, 9))
EXIT_GRADIENT, EXIT_CAP, EXIT_NOPROGRESS = 0, 1, 2
EXIT_NAMES = ("gradient", "cap", "noprogress")

DEFAULTS = dict(max_correspondence_distance=10.0, transformation_epsilon=1.0e-6, rotation_epsilon=2.0e-3, gicp_epsilon=1.0e-3,
                k_correspondences=20, max_iters=30, max_inner_iters=20, rho=0.01, sigma=0.01, tau1=9.0, tau2=0.05, tau3=0.5,
                step_size=0.01, order=3, gradient_tol=1.0e-2)


def params(kind=0, **kw):
    p = dict(DEFAULTS)
    if kind == 1:
        p["transformation_epsilon"] = 1.0e-4
    elif kind != 0:
        raise ValueError("kind")
    p.update(kw)
    p["plane_epsilon"] = p["gicp_epsilon"]                    # the name vgicp_ref.distributions reads
    return p


class Margins(F.Margins):
    """fgicp_ref's margins (nn_gap, cut_gap, conv, log) plus one per comparison of the BFGS; events: the census of what happened"""
    KEYS = ("m_rho", "m_sigma", "m_sign", "m_prev", "m_noprog", "m_grad")

    def __init__(self):
        super().__init__()
        for k in self.KEYS:
            setattr(self, k, np.inf)
        self.f_ulps = np.inf
        self.events = {}

    def see(self, key, lhs, rhs, scale=None):
        s = max(abs(lhs), abs(rhs)) if scale is None else scale
        if s > 0 and math.isfinite(lhs) and math.isfinite(rhs):
            setattr(self, key, min(getattr(self, key), abs(lhs - rhs) / s))

    def see_f(self, key, lhs, rhs, f0, lin):
        """a comparison of two values of f along a line: relative to the larger of their changes from f0 and of the linear term lin;
        f_ulps: the same distance in units of eps |f0|, the rounding of one value of f"""
        self.see(key, lhs, rhs, max(abs(lhs - f0), abs(rhs - f0), abs(lin)))
        if f0 != 0.0:
            self.f_ulps = min(self.f_ulps, abs(lhs - rhs) / (DBL_EPSILON * abs(f0)))

    def event(self, name):
        self.events[name] = self.events.get(name, 0) + 1
        self.log.append(name)

    def decisions(self):
        return {k: getattr(self, k) for k in self.KEYS}


# ---- 1. x <-> X(x) -----------------------------------------------------------------------------------------------------------------
def euler_R(x):
    """R = Rz(yaw) Ry(pitch) Rx(roll), row-major [9]"""
    cr, sr, cp, sp, cy, sy = math.cos(x[3]), math.sin(x[3]), math.cos(x[4]), math.sin(x[4]), math.cos(x[5]), math.sin(x[5])
    return [cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
            sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr,
            -sp, cp * sr, cp * cr]


def euler_dR(x):
    """(dR/droll, dR/dpitch, dR/dyaw), each row-major [9]: computeRDerivative's matrices"""
    cr, sr, cp, sp, cy, sy = math.cos(x[3]), math.sin(x[3]), math.cos(x[4]), math.sin(x[4]), math.cos(x[5]), math.sin(x[5])
    d_roll = [0.0, cy * sp * cr + sy * sr, sy * cr - cy * sp * sr,
              0.0, sy * sp * cr - cy * sr, -sy * sp * sr - cy * cr,
              0.0, cp * cr, -cp * sr]
    d_pitch = [-cy * sp, cy * cp * sr, cy * cp * cr,
               -sy * sp, sy * cp * sr, sy * cp * cr,
               -cp, -sp * sr, -sp * cr]
    d_yaw = [-sy * cp, -sy * sp * sr - cy * cr, cy * sr - sy * sp * cr,
             cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr,
             0.0, 0.0, 0.0]
    return d_roll, d_pitch, d_yaw


def state_matrix(x):
    """X(x), row-major [16]"""
    R = euler_R(x)
    return [R[0], R[1], R[2], x[0], R[3], R[4], R[5], x[1], R[6], R[7], R[8], x[2], 0.0, 0.0, 0.0, 1.0]


def compose(X, G):
    """X G of two row-major [16], every entry ((X0 G0 + X1 G1) + X2 G2) + X3 G3"""
    T = [0.0] * 16
    for i in range(4):
        for j in range(4):
            T[4 * i + j] = ((X[4 * i] * G[j] + X[4 * i + 1] * G[4 + j]) + X[4 * i + 2] * G[8 + j]) + X[4 * i + 3] * G[12 + j]
    return T


def pose_of(x, G):
    """T = X(x) G as a [4, 4] array"""
    return np.array(compose(state_matrix(x), [float(v) for v in np.asarray(G, np.float64).reshape(16)])).reshape(4, 4)


def outer_delta(xa, xb, prm):
    """max over the entries of |X(xa) - X(xb)|, rotation entries / rotation_epsilon, translation entries / transformation_epsilon"""
    A, B = state_matrix(xa), state_matrix(xb)
    delta = 0.0
    for i in range(3):
        for j in range(4):
            d = abs(A[4 * i + j] - B[4 * i + j])
            d = d / prm["rotation_epsilon"] if j < 3 else d / prm["transformation_epsilon"]
            if d > delta:
                delta = d
    return delta


# ---- 2. the moments and what BFGS sees ---------------------------------------------------------------------------------------------
def centre(tgt):
    """c = (b0 + b1) / 2 of the target's finite bounding box, in double from the float corners"""
    pts = tgt["x"][tgt["idx"]]
    return [float(v) for v in (pts.min(0) + pts.max(0)) / 2.0]


def moments(tgt, src, pairs, T_k, c):
    """(rec [74], abs [74]: the sums of the terms' magnitudes) of a pair set (fgicp_ref.find_pairs at T_k)"""
    rec, ab = np.zeros(N_REC), np.zeros(N_REC)
    pi, ti, M = pairs["pi"], pairs["ti"], pairs["M"]
    if len(pi) == 0:
        return rec, ab
    xp = transform_points(np.asarray(T_k, np.float64), src["x"][pi])
    y = xp - np.asarray(c, np.float64)
    yt = np.concatenate([y, np.ones((len(pi), 1))], 1)
    r = xp - tgt["x"][ti]
    Mr = np.stack([(M[:, a, 0] * r[:, 0] + M[:, a, 1] * r[:, 1]) + M[:, a, 2] * r[:, 2] for a in range(3)], 1)
    terms = np.zeros((len(pi), N_REC))
    terms[:, 0] = (r[:, 0] * Mr[:, 0] + r[:, 1] * Mr[:, 1]) + r[:, 2] * Mr[:, 2]
    for a in range(3):
        for b in range(4):
            terms[:, 1 + 4 * a + b] = Mr[:, a] * yt[:, b]
    for p, (a, a2) in enumerate(P6):
        for q, (b, b2) in enumerate(Q10):
            terms[:, 13 + 10 * p + q] = M[:, a, a2] * (yt[:, b] * yt[:, b2])
    terms[:, 73] = 1.0
    return terms.sum(0), np.abs(terms).sum(0)


def theta_of(x, xk, c):
    """Theta = [E | d] row-major [12]: E = R(x) R(xk)^T - I, d = E (c - t_k) + (t(x) - t_k)"""
    R, Rk = euler_R(x), euler_R(xk)
    v = [c[0] - xk[0], c[1] - xk[1], c[2] - xk[2]]
    th = [0.0] * 12
    for a in range(3):
        for b in range(3):
            e = (R[3 * a] * Rk[3 * b] + R[3 * a + 1] * Rk[3 * b + 1]) + R[3 * a + 2] * Rk[3 * b + 2]
            th[4 * a + b] = e - 1.0 if a == b else e
        th[4 * a + 3] = ((th[4 * a] * v[0] + th[4 * a + 1] * v[1]) + th[4 * a + 2] * v[2]) + (x[a] - xk[a])
    return th


def fdf(rec, c, xk, x, want_grad=True):
    """(f, grad [6] or None) at x from the record of the outer iterate xk: the function BFGS minimises"""
    m = rec[73]
    th = theta_of(x, xk, c)
    W = [0.0] * 12                                            # W[a][b] = sum over a', b' of S[(a, a')][(b, b')] Theta[a'][b']
    for a in range(3):
        for b in range(4):
            s = 0.0
            for a2 in range(3):
                base = 13 + 10 * SYM3[a][a2]
                for b2 in range(4):
                    s += rec[base + SYM4[b][b2]] * th[4 * a2 + b2]
            W[4 * a + b] = s
    mf = rec[0]
    for k in range(12):
        mf += th[k] * (2.0 * rec[1 + k] + W[k])
    f = mf / m
    if not want_grad:
        return f, None
    Gt = [2.0 * (rec[1 + k] + W[k]) for k in range(12)]       # d(m f) / dTheta
    Rk = euler_R(xk)
    v = [c[0] - xk[0], c[1] - xk[1], c[2] - xk[2]]
    grad = [Gt[3] / m, Gt[7] / m, Gt[11] / m, 0.0, 0.0, 0.0]
    for j, dR in enumerate(euler_dR(x)):
        s = 0.0
        for a in range(3):
            D = [0.0] * 3                                     # row a of dR R(xk)^T
            for b in range(3):
                D[b] = (dR[3 * a] * Rk[3 * b] + dR[3 * a + 1] * Rk[3 * b + 1]) + dR[3 * a + 2] * Rk[3 * b + 2]
            dv = (D[0] * v[0] + D[1] * v[1]) + D[2] * v[2]
            s += ((Gt[4 * a] * D[0] + Gt[4 * a + 1] * D[1]) + Gt[4 * a + 2] * D[2]) + Gt[4 * a + 3] * dv
        grad[3 + j] = s / m
    return f, grad


def pair_form(tgt, src, pairs, G, x):
    """PCL's literal sums over the pairs at x: (f, grad [6]) with p_i = G a_i, res = R(x) p + t(x) - q, g[0:3] = 2/m sum M res,
    g[3 + j] = 2/m sum (dR_j p) . (M res).  The independent check of fdf; never the definition."""
    pi, ti, M = pairs["pi"], pairs["ti"], pairs["M"]
    m = float(len(pi))
    p = transform_points(np.asarray(G, np.float64).reshape(4, 4), src["x"][pi])
    R = np.array(euler_R(x)).reshape(3, 3)
    res = p @ R.T + np.asarray(x[:3]) - tgt["x"][ti]
    Mres = np.einsum("nij,nj->ni", M, res)
    f = float(np.einsum("ni,ni->", res, Mres)) / m
    g = np.zeros(6)
    g[:3] = 2.0 * Mres.sum(0) / m
    for j, dR in enumerate(euler_dR(x)):
        g[3 + j] = 2.0 * float(np.einsum("ni,ni->", p @ np.array(dR).reshape(3, 3).T, Mres)) / m
    return f, g


# ---- 3. Fletcher's line search and the BFGS (GSL's vector_bfgs2 as remembered) -----------------------------------------------------
def solve_quadratic(a, b, c):
    """gsl_poly_solve_quadratic: (number of roots, x0 <= x1)"""
    if a == 0.0:
        if b == 0.0:
            return 0, 0.0, 0.0
        return 1, -c / b, 0.0
    disc = b * b - 4.0 * a * c
    if disc > 0.0:
        if b == 0.0:
            r = math.sqrt(-c / a)
            return 2, -r, r
        sgnb = 1.0 if b > 0.0 else -1.0
        temp = -0.5 * (b + sgnb * math.sqrt(disc))
        r1, r2 = temp / a, c / temp
        return (2, r1, r2) if r1 < r2 else (2, r2, r1)
    if disc == 0.0:
        return 2, -0.5 * b / a, -0.5 * b / a
    return 0, 0.0, 0.0


def interp_quad(f0, fp0, f1, zl, zh):
    fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0))
    fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0))
    c = 2.0 * (f1 - f0 - fp0)
    zmin, fmin = zl, fl
    if fh < fmin:
        zmin, fmin = zh, fh
    if c > 0.0:
        z = -fp0 / c
        if z > zl and z < zh:
            f = f0 + z * (fp0 + z * (f1 - f0 - fp0))
            if f < fmin:
                zmin, fmin = z, f
    return zmin


def _cubic(c0, c1, c2, c3, z):
    return c0 + z * (c1 + z * (c2 + z * c3))


def interp_cubic(f0, fp0, f1, fp1, zl, zh):
    eta = 3.0 * (f1 - f0) - 2.0 * fp0 - fp1
    xi = fp0 + fp1 - 2.0 * (f1 - f0)
    c0, c1, c2, c3 = f0, fp0, eta, xi
    zmin, fmin = zl, _cubic(c0, c1, c2, c3, zl)
    y = _cubic(c0, c1, c2, c3, zh)
    if y < fmin:
        zmin, fmin = zh, y
    n, z0, z1 = solve_quadratic(3.0 * c3, 2.0 * c2, c1)
    if n >= 1 and z0 > zl and z0 < zh:
        y = _cubic(c0, c1, c2, c3, z0)
        if y < fmin:
            zmin, fmin = z0, y
    if n == 2 and z1 > zl and z1 < zh:
        y = _cubic(c0, c1, c2, c3, z1)
        if y < fmin:
            zmin, fmin = z1, y
    return zmin


def interpolate(a, fa, fpa, b, fb, fpb, xmin, xmax, order):
    zmin, zmax = (xmin - a) / (b - a), (xmax - a) / (b - a)
    if zmin > zmax:
        zmin, zmax = zmax, zmin
    if order > 2 and math.isfinite(fpb):
        z = interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax)
    else:
        z = interp_quad(fa, fpa * (b - a), fb, zmin, zmax)
    return a + z * (b - a)


LS_SUCCESS, LS_NOPROGRESS = 0, 1


def line_search(f_at, df_at, f0, fp0, alpha1, prm, mg=None):
    """GSL's `minimize`: (status, alpha).  f_at(alpha), df_at(alpha): the function and its slope along the direction"""
    rho, sigma, tau1, tau2, tau3, order = prm["rho"], prm["sigma"], prm["tau1"], prm["tau2"], prm["tau3"], prm["order"]
    alpha, alpha_prev = alpha1, 0.0
    falpha_prev, fpalpha_prev = f0, fp0
    a, b, fa, fb, fpa, fpb = 0.0, alpha, f0, 0.0, fp0, 0.0
    i = 0
    while i < 100:                                            # bracketing
        i += 1
        falpha = f_at(alpha)
        if mg:
            mg.see_f("m_rho", falpha, f0 + alpha * rho * fp0, f0, alpha * fp0)
            mg.see_f("m_prev", falpha, falpha_prev, f0, 0.0)
        if falpha > f0 + alpha * rho * fp0 or falpha >= falpha_prev:
            if mg:
                mg.event("bracket:rho")
            a, fa, fpa = alpha_prev, falpha_prev, fpalpha_prev
            b, fb, fpb = alpha, falpha, math.nan
            break
        fpalpha = df_at(alpha)
        if mg:
            mg.see("m_sigma", abs(fpalpha), -sigma * fp0, abs(fp0))
        if abs(fpalpha) <= -sigma * fp0:
            if mg:
                mg.event("bracket:sigma")
            return LS_SUCCESS, alpha
        if mg:
            mg.see("m_sign", fpalpha, 0.0, abs(fp0))
        if fpalpha >= 0.0:
            if mg:
                mg.event("bracket:slope")
            a, fa, fpa = alpha, falpha, fpalpha
            b, fb, fpb = alpha_prev, falpha_prev, fpalpha_prev
            break
        if mg:
            mg.event("bracket:extend")
        delta = alpha - alpha_prev
        alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta, alpha + tau1 * delta, order)
        alpha_prev, falpha_prev, fpalpha_prev = alpha, falpha, fpalpha
        alpha = alpha_next
    while i < 100:                                            # sectioning of [a, b]; the counter runs on
        i += 1
        delta = b - a
        alpha = interpolate(a, fa, fpa, b, fb, fpb, a + tau2 * delta, b - tau3 * delta, order)
        falpha = f_at(alpha)
        if mg:
            mg.see("m_noprog", (a - alpha) * fpa, DBL_EPSILON, abs(delta * fpa))
        if (a - alpha) * fpa <= DBL_EPSILON:
            if mg:
                mg.event("section:noprogress")
            return LS_NOPROGRESS, alpha
        if mg:
            mg.see_f("m_rho", falpha, f0 + rho * alpha * fp0, f0, alpha * fp0)
            mg.see_f("m_prev", falpha, fa, f0, 0.0)
        if falpha > f0 + rho * alpha * fp0 or falpha >= fa:
            if mg:
                mg.event("section:shrink")
            b, fb, fpb = alpha, falpha, math.nan
        else:
            fpalpha = df_at(alpha)
            if mg:
                mg.see("m_sigma", abs(fpalpha), -sigma * fp0, abs(fp0))
            if abs(fpalpha) <= -sigma * fp0:
                if mg:
                    mg.event("section:sigma")
                return LS_SUCCESS, alpha
            if mg:
                mg.see("m_sign", fpalpha, 0.0, abs(fp0))
            if (b - a >= 0.0 and fpalpha >= 0.0) or (b - a <= 0.0 and fpalpha <= 0.0):
                if mg:
                    mg.event("section:flip")
                b, fb, fpb = a, fa, fpa
                a, fa, fpa = alpha, falpha, fpalpha
            else:
                if mg:
                    mg.event("section:advance")
                a, fa, fpa = alpha, falpha, fpalpha
    if mg:
        mg.event("linesearch:limit")
    return LS_SUCCESS, alpha


def _norm(v):
    s = 0.0
    for k in range(len(v)):
        s += v[k] * v[k]
    return math.sqrt(s)


def _dot(u, v):
    s = 0.0
    for k in range(len(u)):
        s += u[k] * v[k]
    return s


def bfgs_minimise(fun, x_start, prm, mg=None):
    """PCL's inner loop over BFGS<>: fun(x, want_grad) -> (f, grad or None).  Returns dict(x, f, iters, n_f, n_df, exit, wolfe): n_f
    counts the evaluations of f (with or without the gradient), n_df those of the gradient alone; wolfe: per successful step
    (f0, fp0, alpha, f(alpha), f'(alpha))"""
    n = len(x_start)
    cnt = dict(n_f=0, n_df=0)
    x = list(x_start)
    f, g = fun(x, True)
    cnt["n_f"] += 1
    x0, g0 = list(x), list(g)
    g0norm = _norm(g0)
    p = [0.0] * n
    if g0norm > 0.0:
        for k in range(n):
            p[k] = g[k] * (-1.0 / g0norm)
    pnorm = _norm(p)
    fp0 = -g0norm
    delta_f = 0.0
    iters, exit_code, wolfe = 0, EXIT_CAP, []
    cache = {}

    def x_at(alpha):
        return [x0[k] + alpha * p[k] for k in range(n)]

    def f_at(alpha):
        if cache.get("fa") == alpha:
            return cache["f"]
        fa, _ = fun(x_at(alpha), False)
        cnt["n_f"] += 1
        cache["fa"], cache["f"] = alpha, fa
        return fa

    def g_at(alpha):
        if cache.get("ga") != alpha:
            fa, ga = fun(x_at(alpha), True)
            if cache.get("fa") == alpha:
                cnt["n_df"] += 1
            else:
                cnt["n_f"] += 1
            cache["fa"], cache["f"], cache["ga"], cache["g"] = alpha, fa, alpha, ga
        return cache["g"]

    def df_at(alpha):
        return _dot(g_at(alpha), p)

    while True:
        iters += 1
        # ---- minimizeOneStep
        f0 = f
        if pnorm == 0.0 or g0norm == 0.0 or fp0 == 0.0:
            if mg:
                mg.event("step:degenerate")
            exit_code = EXIT_NOPROGRESS
            break
        if delta_f < 0.0:
            dl = max(-delta_f, 10.0 * DBL_EPSILON * abs(f0))
            alpha1 = min(1.0, 2.0 * dl / (-fp0))
        else:
            alpha1 = abs(prm["step_size"])
        cache.clear()
        cache["fa"], cache["f"], cache["ga"], cache["g"] = 0.0, f0, 0.0, g0
        status, alpha = line_search(f_at, df_at, f0, fp0, alpha1, prm, mg)
        if status != LS_SUCCESS:
            exit_code = EXIT_NOPROGRESS
            break
        g = list(g_at(alpha))                                 # updatePosition
        f = f_at(alpha)
        x = x_at(alpha)
        wolfe.append((f0, fp0, alpha, f, _dot(g, p)))
        delta_f = f - f0
        dx0 = [x[k] - x0[k] for k in range(n)]
        dg0 = [g[k] - g0[k] for k in range(n)]
        dxg, dgg, dxdg, dgnorm = _dot(dx0, g), _dot(dg0, g), _dot(dx0, dg0), _norm(dg0)
        if dxdg != 0.0:
            B = dxg / dxdg
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg
        else:
            B = A = 0.0
        for k in range(n):
            p[k] = (g[k] - A * dx0[k]) - B * dg0[k]
        g0, x0 = list(g), list(x)
        g0norm, pnorm = _norm(g0), _norm(p)
        pg = _dot(p, g)
        direction = -1.0 if pg >= 0.0 else 1.0
        if pnorm > 0.0:
            for k in range(n):
                p[k] = p[k] * (direction / pnorm)
        pnorm = _norm(p)
        fp0 = _dot(p, g0)
        # ---- testGradient
        if mg:
            mg.see("m_grad", g0norm, prm["gradient_tol"])
        if g0norm < prm["gradient_tol"]:
            exit_code = EXIT_GRADIENT
            break
        if iters >= prm["max_inner_iters"]:
            exit_code = EXIT_CAP
            break
    if mg:
        mg.event("inner:" + EXIT_NAMES[exit_code])
    return dict(x=x, f=f, iters=iters, n_f=cnt["n_f"], n_df=cnt["n_df"], exit=exit_code, wolfe=wolfe)


def inner(rec, c, xk, prm, mg=None, on_eval=None):
    """the inner minimisation of one outer iteration from the 74 doubles alone"""
    def fun(x, want_grad):
        if on_eval:
            on_eval(x)
        return fdf(rec, c, xk, x, want_grad)
    return bfgs_minimise(fun, xk, prm, mg)


# ---- 4. the whole registration -----------------------------------------------------------------------------------------------------
def align(tgt, src, prm, guess=None, mg=None, keep=False, perturb=None):
    """a prepared source (vgicp_ref.prepare_source) against a target (fgicp_ref.build_target).  keep: also the records, the pair sets
    and the visited states of every outer iteration.  perturb = (eps, seed): every sum of every record is moved by a random share of
    eps times its sum of |term| (the pair count stays) — what another summation order or another rounding of M does to it; the
    stability margin of a case is how far such a run ends from the plain one"""
    mg = mg or Margins()
    rng = np.random.default_rng(perturb[1]) if perturb else None
    G = np.eye(4) if guess is None else np.asarray(guess, np.float32).reshape(4, 4).astype(np.float64)
    c = centre(tgt)
    x = [0.0] * 6
    res = dict(converged=0, iters=0, inner_iters=0, n_evals=0, n_rounds=0, n_pairs_last=0, error=0.0, last_delta=0.0, inner_exit=-1)
    recs, xks, outs, psets, visits = [], [], [], [], []
    while True:
        T_k = pose_of(x, G)
        pairs = find_pairs(tgt, src, T_k, prm, mg)
        rec, ab = moments(tgt, src, pairs, T_k, c)
        if perturb:
            rec[:73] += perturb[0] * ab[:73] * rng.uniform(-1.0, 1.0, 73)
        res["n_rounds"] += 1
        res["n_pairs_last"] = int(rec[73])
        if rec[73] < 4:
            mg.event("outer:few_pairs")
            res["error"] = float(rec[0] / rec[73]) if rec[73] > 0 else 0.0
            break
        seen = []
        r = inner(rec, c, x, prm, mg, seen.append if keep else None)
        if keep:
            recs.append(rec); xks.append(list(x)); outs.append(r); psets.append(pairs); visits.append(seen)
        delta = outer_delta(x, r["x"], prm)
        mg.conv = min(mg.conv, abs(delta - 1.0))
        x = r["x"]
        res["iters"] += 1
        res["inner_iters"] += r["iters"]
        res["n_evals"] += r["n_f"] + r["n_df"]
        res.update(error=float(r["f"]), last_delta=float(delta), inner_exit=r["exit"])
        if res["iters"] >= prm["max_iters"] or delta < 1.0:
            mg.event("outer:delta" if delta < 1.0 else "outer:max_iters")
            res["converged"] = 1
            break
    res.update(T=pose_of(x, G), x=list(x), margin_conv=mg.conv, margin_nn=mg.nn_gap, margin_cut=mg.cut_gap, decisions=mg.decisions(), f_ulps=mg.f_ulps,
               events=dict(mg.events), log=list(mg.log))
    if keep:
        res.update(recs=recs, xks=xks, inners=outs, pair_sets=psets, visits=visits, G=G, c=c)
    return res


# ---- the expected outputs kept in tests/golden/gicp (tests/golden/make_golden_gicp.py writes them) -----------------------------------
# seed, trans, rot_deg, transformation_epsilon.  The seeds are vgicp_ref.ALIGN_CASES' and fgicp_ref's; the guesses are NOT the family's
# 0.3 m / 2 degrees and 0.5 m / 3 degrees: from that far the first inner minimisations spend their 20 steps unconverged, and 20 steps of
# a memoryless BFGS with an inexact line search amplify a change of 1e-12 of a moment's sum of |term| to 1e-4 in the final pose (measured
# with align(perturb=...) on all four seeds: 4e-5 .. 4e-4, and other iteration counts) — no two summation orders, this file's and a
# GPU's among them, agree on such a run to the 1e-6 the family's tests ask for.  From 0.05 m / 0.3 degrees and closer the runs below end
# within 1e-8 of themselves under that perturbation (tests/test_gicp_ref.py asserts 1e-7 and equal counts); a seed or a guess that misses
# is replaced.  tests/test_gicp.py still aligns the family's 0.3 m / 2 degree scene, against the truth instead of against this file.
ALIGN_CASES = ((1000, 0.05, 0.3, 1.0e-6), (1006, 0.05, 0.3, 1.0e-4), (1001, 0.02, 0.1, 1.0e-6), (1005, 0.05, 0.3, 5.0e-4), (1000, 0.05, 0.3, 0.01))
PERTURB_EPS = 1.0e-12             # of a sum's sum of |term|: M = S^-1 with condition 1 / gicp_epsilon = 1e3 rounds to 1e3 eps = 2e-13 per term
lin_poses = V.lin_poses
_RUNS = {}


def case_run(k):
    """the kept run (align(..., keep=True)) of ALIGN_CASES[k], made once per process"""
    if k not in _RUNS:
        seed, trans, rot, eps = ALIGN_CASES[k]
        W = world(seed, trans, rot)
        _RUNS[k] = align(W["T"], W["S"], params(transformation_epsilon=eps), W["guess"], keep=True)
    return _RUNS[k]


def golden_cases():
    out = {}
    W = world()
    T, S, prm = W["T"], W["S"], params()
    poses = lin_poses(W["guess"], W["T_true"])
    c = centre(T)
    out["centre"], out["mom_T"] = np.array(c), poses
    recs, absum = [], []
    for P in poses:
        rec, ab = moments(T, S, find_pairs(T, S, P, prm), P, c)
        recs.append(rec); absum.append(ab)
    out["mom_rec"], out["mom_abs"] = np.array(recs), np.array(absum)
    counts, Ts, fig, in_rec, in_x0, in_x1, in_cnt, in_case, in_c = [], [], [], [], [], [], [], [], []
    for k, (seed, trans, rot, eps) in enumerate(ALIGN_CASES):
        Wk = world(seed, trans, rot)
        r = case_run(k)
        et, er = pose_error(r["T"], Wk["T_true"])
        et0, er0 = pose_error(Wk["guess"], Wk["T_true"])
        counts.append([r["converged"], r["iters"], r["inner_iters"], r["n_evals"], r["n_rounds"], r["n_pairs_last"], r["inner_exit"], len(Wk["src"])])
        Ts.append(r["T"])
        fig.append([r["error"], r["last_delta"], r["margin_conv"], r["margin_nn"], r["margin_cut"], min(r["decisions"].values()), r["f_ulps"], et, er, et0, er0])
        for rec, xk, o in zip(r["recs"], r["xks"], r["inners"]):
            in_rec.append(rec); in_x0.append(xk); in_x1.append(o["x"]); in_cnt.append([o["iters"], o["n_f"], o["n_df"], o["exit"]])
            in_case.append(k); in_c.append(r["c"])
    out["align_counts"], out["align_T"], out["align_fig"] = np.array(counts, np.int64), np.array(Ts), np.array(fig)
    out["inner_rec"], out["inner_x0"], out["inner_x1"] = np.array(in_rec), np.array(in_x0), np.array(in_x1)
    out["inner_counts"], out["inner_case"], out["inner_centre"] = np.array(in_cnt, np.int64), np.array(in_case, np.int64), np.array(in_c)
    return out
