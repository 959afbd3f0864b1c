// lisreg_gicp_host.hpp — the host half of PCL's GICP (lisreg_gicp.hip): the Euler algebra x <-> X(x), the function and
// the gradient BFGS sees from the 74 moments of one outer iteration, Fletcher's line search and the BFGS loop (GSL's vector_bfgs2 as
// remembered), in double, statement by statement what tests/gicp_ref.py defines — the same operations in the same order, so that both
// give the same bits from the same 74 doubles.  Plain C++ (no HIP, no state outside its structs), so that it can be compiled and
// checked on its own (host/gicp_bfgs_check.cpp).  Not installed.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace lisreg {
namespace gicp_host {

constexpr int kRec = 74;          // c0, g [3][4], S [6][10], pairs (tests/gicp_ref.py lists the order)
constexpr double kEps = 2.220446049250313e-16;
constexpr int kSym3[3][3] = { { 0, 1, 2 }, { 1, 3, 4 }, { 2, 4, 5 } };
constexpr int kSym4[4][4] = { { 0, 1, 2, 3 }, { 1, 4, 5, 6 }, { 2, 5, 7, 8 }, { 3, 6, 8, 9 } };
enum { kExitGradient = 0, kExitCap = 1, kExitNoProgress = 2 };
enum { kLsSuccess = 0, kLsNoProgress = 1 };

struct BfgsParams {
    double rho, sigma, tau1, tau2, tau3, step_size, gradient_tol;
    int    order, max_inner_iters;
};
template <class Params>
inline BfgsParams bfgs_params_of(const Params& P)
{
    return BfgsParams{ P.rho, P.sigma, P.tau1, P.tau2, P.tau3, P.step_size, P.gradient_tol, P.order, P.max_inner_iters };
}

// what happened, for the checks (optional everywhere): the census of the branches and the record of every successful step
enum Event {
    kBracketRho, kBracketSigma, kBracketSlope, kBracketExtend, kSectionNoProgress, kSectionShrink, kSectionSigma, kSectionFlip,
    kSectionAdvance, kLineSearchLimit, kStepDegenerate, kInnerGradient, kInnerCap, kInnerNoProgress, kEvents
};
struct Step { double f0, fp0, alpha, f, fp; int trials; };
struct Census {
    long events[kEvents] = {};
    int  max_trials = 0;          // the most trials one line search took
    int  n_steps = 0;             // successful steps of the last bfgs_minimise (the first kMaxSteps are kept)
    static constexpr int kMaxSteps = 64;
    Step steps[kMaxSteps];
    void see(Event e) { ++events[e]; }
};
inline void note(Census* cs, Event e) { if (cs) cs->see(e); }

// ---- x <-> X(x) ----------------------------------------------------------------------------------------------------------------------
struct Trig { double cr, sr, cp, sp, cy, sy; };
inline Trig trig_of(const double x[6]) { return Trig{ cos(x[3]), sin(x[3]), cos(x[4]), sin(x[4]), cos(x[5]), sin(x[5]) }; }

// R = Rz(yaw) Ry(pitch) Rx(roll), row-major
inline void euler_R(const double x[6], double R[9])
{
    const Trig t = trig_of(x);
    R[0] = t.cy * t.cp; R[1] = t.cy * t.sp * t.sr - t.sy * t.cr; R[2] = t.cy * t.sp * t.cr + t.sy * t.sr;
    R[3] = t.sy * t.cp; R[4] = t.sy * t.sp * t.sr + t.cy * t.cr; R[5] = t.sy * t.sp * t.cr - t.cy * t.sr;
    R[6] = -t.sp;       R[7] = t.cp * t.sr;                      R[8] = t.cp * t.cr;
}

// dR/droll, dR/dpitch, dR/dyaw
inline void euler_dR(const double x[6], double D[3][9])
{
    const Trig t = trig_of(x);
    const double roll[9] = { 0.0, t.cy * t.sp * t.cr + t.sy * t.sr, t.sy * t.cr - t.cy * t.sp * t.sr,
                             0.0, t.sy * t.sp * t.cr - t.cy * t.sr, -t.sy * t.sp * t.sr - t.cy * t.cr,
                             0.0, t.cp * t.cr, -t.cp * t.sr };
    const double pitch[9] = { -t.cy * t.sp, t.cy * t.cp * t.sr, t.cy * t.cp * t.cr,
                              -t.sy * t.sp, t.sy * t.cp * t.sr, t.sy * t.cp * t.cr,
                              -t.cp, -t.sp * t.sr, -t.sp * t.cr };
    const double yaw[9] = { -t.sy * t.cp, -t.sy * t.sp * t.sr - t.cy * t.cr, t.cy * t.sr - t.sy * t.sp * t.cr,
                            t.cy * t.cp, t.cy * t.sp * t.sr - t.sy * t.cr, t.cy * t.sp * t.cr + t.sy * t.sr,
                            0.0, 0.0, 0.0 };
    memcpy(D[0], roll, sizeof roll); memcpy(D[1], pitch, sizeof pitch); memcpy(D[2], yaw, sizeof yaw);
}

inline void state_matrix(const double x[6], double X[16])
{
    double R[9];
    euler_R(x, R);
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) X[4 * i + j] = R[3 * i + j]; X[4 * i + 3] = x[i]; }
    X[12] = X[13] = X[14] = 0.0; X[15] = 1.0;
}

// T = X(x) G, every entry ((X0 G0 + X1 G1) + X2 G2) + X3 G3
inline void pose_of_state(const double x[6], const double G[16], double T[16])
{
    double X[16];
    state_matrix(x, X);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            T[4 * i + j] = ((X[4 * i] * G[j] + X[4 * i + 1] * G[4 + j]) + X[4 * i + 2] * G[8 + j]) + X[4 * i + 3] * G[12 + j];
}

// max over the entries of |X(xa) - X(xb)|, rotation entries / rotation_epsilon, translation entries / transformation_epsilon
inline double outer_delta(const double xa[6], const double xb[6], double rotation_epsilon, double transformation_epsilon)
{
    double A[16], B[16];
    state_matrix(xa, A);
    state_matrix(xb, B);
    double delta = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            double d = fabs(A[4 * i + j] - B[4 * i + j]);
            d = j < 3 ? d / rotation_epsilon : d / transformation_epsilon;
            if (d > delta) delta = d;
        }
    return delta;
}

// ---- the moments -> f, grad -------------------------------------------------------------------------------------------------------------
// Theta = [E | d] row-major [12]: E = R(x) R(xk)^T - I, d = E (c - t_k) + (t(x) - t_k)
inline void theta_of(const double x[6], const double xk[6], const double c[3], double th[12])
{
    double R[9], Rk[9];
    euler_R(x, R);
    euler_R(xk, Rk);
    const double v[3] = { c[0] - xk[0], c[1] - xk[1], c[2] - xk[2] };
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) {
            const double e = (R[3 * a] * Rk[3 * b] + R[3 * a + 1] * Rk[3 * b + 1]) + R[3 * a + 2] * Rk[3 * b + 2];
            th[4 * a + b] = a == b ? e - 1.0 : e;
        }
        th[4 * a + 3] = ((th[4 * a] * v[0] + th[4 * a + 1] * v[1]) + th[4 * a + 2] * v[2]) + (x[a] - xk[a]);
    }
}

// f (and grad [6] if wanted) at x from the record of the outer iterate xk
inline double fdf(const double rec[kRec], const double c[3], const double xk[6], const double x[6], double* grad)
{
    const double m = rec[73];
    double th[12], W[12];
    theta_of(x, xk, c, th);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 4; ++b) {
            double s = 0.0;
            for (int a2 = 0; a2 < 3; ++a2) {
                const int base = 13 + 10 * kSym3[a][a2];
                for (int b2 = 0; b2 < 4; ++b2) s += rec[base + kSym4[b][b2]] * th[4 * a2 + b2];
            }
            W[4 * a + b] = s;
        }
    double mf = rec[0];
    for (int k = 0; k < 12; ++k) mf += th[k] * (2.0 * rec[1 + k] + W[k]);
    const double f = mf / m;
    if (!grad) return f;
    double Gt[12], Rk[9], dR[3][9];
    for (int k = 0; k < 12; ++k) Gt[k] = 2.0 * (rec[1 + k] + W[k]);
    euler_R(xk, Rk);
    euler_dR(x, dR);
    const double v[3] = { c[0] - xk[0], c[1] - xk[1], c[2] - xk[2] };
    grad[0] = Gt[3] / m; grad[1] = Gt[7] / m; grad[2] = Gt[11] / m;
    for (int j = 0; j < 3; ++j) {
        double s = 0.0;
        for (int a = 0; a < 3; ++a) {
            double D[3];
            for (int b = 0; b < 3; ++b)
                D[b] = (dR[j][3 * a] * Rk[3 * b] + dR[j][3 * a + 1] * Rk[3 * b + 1]) + dR[j][3 * a + 2] * Rk[3 * b + 2];
            const double dv = (D[0] * v[0] + D[1] * v[1]) + D[2] * v[2];
            s += ((Gt[4 * a] * D[0] + Gt[4 * a + 1] * D[1]) + Gt[4 * a + 2] * D[2]) + Gt[4 * a + 3] * dv;
        }
        grad[3 + j] = s / m;
    }
    return f;
}

// ---- Fletcher's line search (GSL's linear_minimize.c as remembered) --------------------------------------------------------------------
// gsl_poly_solve_quadratic: the number of roots, x0 <= x1
inline int solve_quadratic(double a, double b, double c, double& x0, double& x1)
{
    x0 = x1 = 0.0;
    if (a == 0.0) {
        if (b == 0.0) return 0;
        x0 = -c / b;
        return 1;
    }
    const double disc = b * b - 4.0 * a * c;
    if (disc > 0.0) {
        if (b == 0.0) {
            const double r = sqrt(-c / a);
            x0 = -r; x1 = r;
            return 2;
        }
        const double sgnb = b > 0.0 ? 1.0 : -1.0;
        const double temp = -0.5 * (b + sgnb * sqrt(disc));
        const double r1 = temp / a, r2 = c / temp;
        if (r1 < r2) { x0 = r1; x1 = r2; } else { x0 = r2; x1 = r1; }
        return 2;
    }
    if (disc == 0.0) {
        x0 = x1 = -0.5 * b / a;
        return 2;
    }
    return 0;
}

inline double interp_quad(double f0, double fp0, double f1, double zl, double zh)
{
    const double fl = f0 + zl * (fp0 + zl * (f1 - f0 - fp0));
    const double fh = f0 + zh * (fp0 + zh * (f1 - f0 - fp0));
    const double c = 2.0 * (f1 - f0 - fp0);
    double zmin = zl, fmin = fl;
    if (fh < fmin) { zmin = zh; fmin = fh; }
    if (c > 0.0) {
        const double z = -fp0 / c;
        if (z > zl && z < zh) {
            const double f = f0 + z * (fp0 + z * (f1 - f0 - fp0));
            if (f < fmin) { zmin = z; fmin = f; }
        }
    }
    return zmin;
}

inline double cubic(double c0, double c1, double c2, double c3, double z) { return c0 + z * (c1 + z * (c2 + z * c3)); }

inline double interp_cubic(double f0, double fp0, double f1, double fp1, double zl, double zh)
{
    const double eta = 3.0 * (f1 - f0) - 2.0 * fp0 - fp1;
    const double xi = fp0 + fp1 - 2.0 * (f1 - f0);
    const double c0 = f0, c1 = fp0, c2 = eta, c3 = xi;
    double zmin = zl, fmin = cubic(c0, c1, c2, c3, zl);
    double y = cubic(c0, c1, c2, c3, zh);
    if (y < fmin) { zmin = zh; fmin = y; }
    double z0, z1;
    const int n = solve_quadratic(3.0 * c3, 2.0 * c2, c1, z0, z1);
    if (n >= 1 && z0 > zl && z0 < zh) {
        y = cubic(c0, c1, c2, c3, z0);
        if (y < fmin) { zmin = z0; fmin = y; }
    }
    if (n == 2 && z1 > zl && z1 < zh) {
        y = cubic(c0, c1, c2, c3, z1);
        if (y < fmin) { zmin = z1; fmin = y; }
    }
    return zmin;
}

inline double interpolate(double a, double fa, double fpa, double b, double fb, double fpb, double xmin, double xmax, int order)
{
    double zmin = (xmin - a) / (b - a), zmax = (xmax - a) / (b - a);
    if (zmin > zmax) std::swap(zmin, zmax);
    double z;
    if (order > 2 && std::isfinite(fpb)) z = interp_cubic(fa, fpa * (b - a), fb, fpb * (b - a), zmin, zmax);
    else                                 z = interp_quad(fa, fpa * (b - a), fb, zmin, zmax);
    return a + z * (b - a);
}

// GSL's `minimize`.  L has f_at(alpha) and df_at(alpha), the function and its slope along the direction.  One counter runs through
// bracketing and sectioning: at most 100 trials together.
template <class Line>
inline int line_search(Line& L, double f0, double fp0, double alpha1, const BfgsParams& P, double& alpha_out, Census* cs, int* trials)
{
    const double rho = P.rho, sigma = P.sigma, tau1 = P.tau1, tau2 = P.tau2, tau3 = P.tau3;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    double alpha = alpha1, alpha_prev = 0.0;
    double falpha, fpalpha, falpha_prev = f0, fpalpha_prev = fp0;
    double a = 0.0, b = alpha, fa = f0, fb = 0.0, fpa = fp0, fpb = 0.0;
    int i = 0;
    while (i < 100) {                                                // bracketing
        ++i;
        falpha = L.f_at(alpha);
        if (falpha > f0 + alpha * rho * fp0 || falpha >= falpha_prev) {
            note(cs, kBracketRho);
            a = alpha_prev; fa = falpha_prev; fpa = fpalpha_prev;
            b = alpha; fb = falpha; fpb = nan;
            break;
        }
        fpalpha = L.df_at(alpha);
        if (fabs(fpalpha) <= -sigma * fp0) {
            note(cs, kBracketSigma);
            alpha_out = alpha; *trials = i;
            return kLsSuccess;
        }
        if (fpalpha >= 0.0) {
            note(cs, kBracketSlope);
            a = alpha; fa = falpha; fpa = fpalpha;
            b = alpha_prev; fb = falpha_prev; fpb = fpalpha_prev;
            break;
        }
        note(cs, kBracketExtend);
        const double delta = alpha - alpha_prev;
        const double alpha_next = interpolate(alpha_prev, falpha_prev, fpalpha_prev, alpha, falpha, fpalpha, alpha + delta, alpha + tau1 * delta, P.order);
        alpha_prev = alpha; falpha_prev = falpha; fpalpha_prev = fpalpha;
        alpha = alpha_next;
    }
    while (i < 100) {                                                // sectioning of [a, b]; the counter runs on
        ++i;
        const double delta = b - a;
        alpha = interpolate(a, fa, fpa, b, fb, fpb, a + tau2 * delta, b - tau3 * delta, P.order);
        falpha = L.f_at(alpha);
        if ((a - alpha) * fpa <= kEps) {
            note(cs, kSectionNoProgress);
            alpha_out = alpha; *trials = i;
            return kLsNoProgress;
        }
        if (falpha > f0 + rho * alpha * fp0 || falpha >= fa) {
            note(cs, kSectionShrink);
            b = alpha; fb = falpha; fpb = nan;
        } else {
            fpalpha = L.df_at(alpha);
            if (fabs(fpalpha) <= -sigma * fp0) {
                note(cs, kSectionSigma);
                alpha_out = alpha; *trials = i;
                return kLsSuccess;
            }
            if ((b - a >= 0.0 && fpalpha >= 0.0) || (b - a <= 0.0 && fpalpha <= 0.0)) {
                note(cs, kSectionFlip);
                b = a; fb = fa; fpb = fpa;
                a = alpha; fa = falpha; fpa = fpalpha;
            } else {
                note(cs, kSectionAdvance);
                a = alpha; fa = falpha; fpa = fpalpha;
            }
        }
    }
    (void)fb;
    note(cs, kLineSearchLimit);
    alpha_out = alpha; *trials = i;
    return kLsSuccess;
}

// ---- the BFGS (PCL's inner loop over BFGS<>) ------------------------------------------------------------------------------------------
template <int N>
inline double norm_of(const double v[N])
{
    double s = 0.0;
    for (int k = 0; k < N; ++k) s += v[k] * v[k];
    return sqrt(s);
}
template <int N>
inline double dot_of(const double u[N], const double v[N])
{
    double s = 0.0;
    for (int k = 0; k < N; ++k) s += u[k] * v[k];
    return s;
}

struct InnerCounts { int iters, n_f, n_df, exit; };

// the line through x0 along p with the cache of the last f and the last gradient (GSL's wrapper)
template <int N, class Fun>
struct LineOf {
    Fun&         fun;
    InnerCounts& cnt;
    double x0[N], p[N];
    double fa, f, ga, g[N];
    void x_at(double alpha, double x[N]) const { for (int k = 0; k < N; ++k) x[k] = x0[k] + alpha * p[k]; }
    double f_at(double alpha)
    {
        if (fa == alpha) return f;
        double x[N];
        x_at(alpha, x);
        const double v = fun(x, (double*)nullptr);
        ++cnt.n_f;
        fa = alpha; f = v;
        return v;
    }
    const double* g_at(double alpha)
    {
        if (ga != alpha) {
            double x[N], gn[N];
            x_at(alpha, x);
            const double v = fun(x, gn);
            if (fa == alpha) ++cnt.n_df; else ++cnt.n_f;
            fa = alpha; f = v; ga = alpha;
            memcpy(g, gn, sizeof gn);
        }
        return g;
    }
    double df_at(double alpha) { return dot_of<N>(g_at(alpha), p); }
};

// fun(x, grad or nullptr) -> f.  x: the start, then the result.  Returns f at the result.
template <int N, class Fun>
inline double bfgs_minimise(Fun& fun, double x[N], const BfgsParams& P, InnerCounts* counts, Census* cs = nullptr)
{
    InnerCounts cnt = { 0, 0, 0, kExitCap };
    LineOf<N, Fun> L{ fun, cnt, {}, {}, 0.0, 0.0, 0.0, {} };
    double g[N], g0[N];
    double f = fun(x, g);
    ++cnt.n_f;
    memcpy(L.x0, x, sizeof g); memcpy(g0, g, sizeof g);
    double g0norm = norm_of<N>(g0);
    for (int k = 0; k < N; ++k) L.p[k] = g0norm > 0.0 ? g[k] * (-1.0 / g0norm) : 0.0;
    double pnorm = norm_of<N>(L.p);
    double fp0 = -g0norm, delta_f = 0.0;
    if (cs) cs->n_steps = 0;
    for (;;) {
        ++cnt.iters;
        const double f0 = f;
        if (pnorm == 0.0 || g0norm == 0.0 || fp0 == 0.0) {
            note(cs, kStepDegenerate);
            cnt.exit = kExitNoProgress;
            break;
        }
        double alpha1;
        if (delta_f < 0.0) {
            const double dl = std::max(-delta_f, 10.0 * kEps * fabs(f0));
            alpha1 = std::min(1.0, 2.0 * dl / (-fp0));
        } else {
            alpha1 = fabs(P.step_size);
        }
        L.fa = 0.0; L.f = f0; L.ga = 0.0;
        memcpy(L.g, g0, sizeof g0);
        double alpha = 0.0;
        int trials = 0;
        const int status = line_search(L, f0, fp0, alpha1, P, alpha, cs, &trials);
        if (cs) cs->max_trials = std::max(cs->max_trials, trials);
        if (status != kLsSuccess) {
            cnt.exit = kExitNoProgress;
            break;
        }
        memcpy(g, L.g_at(alpha), sizeof g);                          // updatePosition
        f = L.f_at(alpha);
        L.x_at(alpha, x);
        if (cs) {
            if (cs->n_steps < Census::kMaxSteps) cs->steps[cs->n_steps] = Step{ f0, fp0, alpha, f, dot_of<N>(g, L.p), trials };
            ++cs->n_steps;
        }
        delta_f = f - f0;
        double dx0[N], dg0[N];
        for (int k = 0; k < N; ++k) { dx0[k] = x[k] - L.x0[k]; dg0[k] = g[k] - g0[k]; }
        const double dxg = dot_of<N>(dx0, g), dgg = dot_of<N>(dg0, g), dxdg = dot_of<N>(dx0, dg0), dgnorm = norm_of<N>(dg0);
        double A = 0.0, B = 0.0;
        if (dxdg != 0.0) {
            B = dxg / dxdg;
            A = -(1.0 + dgnorm * dgnorm / dxdg) * B + dgg / dxdg;
        }
        for (int k = 0; k < N; ++k) L.p[k] = (g[k] - A * dx0[k]) - B * dg0[k];
        memcpy(g0, g, sizeof g); memcpy(L.x0, x, sizeof g);
        g0norm = norm_of<N>(g0);
        pnorm = norm_of<N>(L.p);
        const double pg = dot_of<N>(L.p, g);
        const double direction = pg >= 0.0 ? -1.0 : 1.0;
        if (pnorm > 0.0)
            for (int k = 0; k < N; ++k) L.p[k] = L.p[k] * (direction / pnorm);
        pnorm = norm_of<N>(L.p);
        fp0 = dot_of<N>(L.p, g0);
        if (g0norm < P.gradient_tol) {                               // testGradient
            cnt.exit = kExitGradient;
            break;
        }
        if (cnt.iters >= P.max_inner_iters) {
            cnt.exit = kExitCap;
            break;
        }
    }
    note(cs, cnt.exit == kExitGradient ? kInnerGradient : cnt.exit == kExitCap ? kInnerCap : kInnerNoProgress);
    *counts = cnt;
    return f;
}

// the inner minimisation of one outer iteration from the 74 doubles alone: x = x_k on entry, the accepted state on return
inline double inner(const double rec[kRec], const double c[3], double x[6], const BfgsParams& P, InnerCounts* counts, Census* cs = nullptr)
{
    double xk[6];
    memcpy(xk, x, sizeof xk);
    auto fun = [&](const double* at, double* grad) { return fdf(rec, c, xk, at, grad); };
    return bfgs_minimise<6>(fun, x, P, counts, cs);
}

}  // namespace gicp_host
}  // namespace lisreg
