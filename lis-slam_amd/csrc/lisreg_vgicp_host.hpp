// lisreg_vgicp_host.hpp — the host half of the VGICP registration (lisreg_vgicp.hip): the SE(3) exponential, the damped 6 x 6 solve and
// the Levenberg-Marquardt bookkeeping, in double, statement by statement what tests/vgicp_ref.py defines.  Plain C++ (no HIP), so that
// it can be compiled and checked on its own.  Not installed.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

namespace lisreg {
namespace vgicp_host {

constexpr int kOut = 29;          // e, b [6], upper triangle of H row by row [21], pairs

// E (row-major 4 x 4) of delta = (omega, v): R = I + A K + B K^2, t = (I + B K + C K^2) v
inline void se3_exp(const double d[6], double E[16])
{
    const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const double th = sqrt(th2);
    double A, B, C;
    if (th < 0.05) {                                                // the series up to th^6: the next terms are below 1e-16
        A = 1.0 - th2 / 6.0 * (1.0 - th2 / 20.0 * (1.0 - th2 / 42.0));
        B = 0.5 - th2 / 24.0 * (1.0 - th2 / 30.0 * (1.0 - th2 / 56.0));
        C = 1.0 / 6.0 - th2 / 120.0 * (1.0 - th2 / 42.0 * (1.0 - th2 / 72.0));
    } else {
        A = sin(th) / th; B = (1.0 - cos(th)) / th2; C = (th - sin(th)) / (th2 * th);
    }
    const double K[9] = { 0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0 };
    double K2[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
    for (int i = 0; i < 3; ++i) {
        double t = 0.0;
        for (int j = 0; j < 3; ++j) {
            const double id = i == j ? 1.0 : 0.0;
            E[4 * i + j] = (id + A * K[3 * i + j]) + B * K2[3 * i + j];
            t += ((id + B * K[3 * i + j]) + C * K2[3 * i + j]) * d[3 + j];
        }
        E[4 * i + 3] = t;
    }
    E[12] = E[13] = E[14] = 0.0; E[15] = 1.0;
}

// C = A B for rigid 4 x 4 (last row 0 0 0 1)
inline void mul_rigid(const double A[16], const double B[16], double C[16])
{
    double out[16];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 4; ++j)
            out[4 * i + j] = (A[4 * i] * B[j] + A[4 * i + 1] * B[4 + j]) + A[4 * i + 2] * B[8 + j];
        out[4 * i + 3] += A[4 * i + 3];
    }
    out[12] = out[13] = out[14] = 0.0; out[15] = 1.0;
    memcpy(C, out, sizeof out);
}

// (H + lam I) delta = -b by Cholesky; false: the matrix is not finite or not positive definite (delta untouched)
inline bool solve_damped(const double H[36], const double b[6], double lam, double delta[6])
{
    double L[6][6];
    for (int i = 0; i < 6; ++i) {
        if (!std::isfinite(b[i])) return false;
        for (int j = 0; j <= i; ++j) {
            double s = H[6 * i + j] + (i == j ? lam : 0.0);
            if (!std::isfinite(s)) return false;
            for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
            if (i == j) {
                if (!(s > 0.0)) return false;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
    }
    double y[6], x[6];
    for (int i = 0; i < 6; ++i) { double s = -b[i]; for (int k = 0; k < i; ++k) s -= L[i][k] * y[k]; y[i] = s / L[i][i]; }
    for (int i = 5; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < 6; ++k) s -= L[k][i] * x[k]; x[i] = s / L[i][i]; }
    for (int i = 0; i < 6; ++i) if (!std::isfinite(x[i])) return false;
    memcpy(delta, x, sizeof x);
    return true;
}

// max|exp(delta).R - I| / rotation_epsilon < 1 and max|exp(delta).t| / transformation_epsilon < 1, entry-wise maxima
inline bool delta_converged(const double delta[6], double rotation_epsilon, double transformation_epsilon)
{
    double E[16];
    se3_exp(delta, E);
    double r = 0.0, t = 0.0;
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) r = std::max(r, fabs(E[4 * i + j] - (i == j ? 1.0 : 0.0)));
        t = std::max(t, fabs(E[4 * i + 3]));
    }
    return r / rotation_epsilon < 1.0 && t / transformation_epsilon < 1.0;
}

struct LmParams { double transformation_epsilon, rotation_epsilon, init_lambda_factor; int max_iters, lm_max_iterations; };
struct LmResult {
    double T[16];
    int    converged, iters, n_evals, n_rejected;
    long long n_pairs_last;
    double error, lambda;
};

// The Levenberg-Marquardt loop of LsqRegistration::step_lm as tests/vgicp_ref.py restates it.  eval(T, with_hessian, out[29]) -> 0 or an
// error code (returned at once).  lambda starts at init_lambda_factor max|diag H| of the first linearisation and is carried across the
// outer iterations; NOT (rho >= 0) is a rejection; a trial loop that runs out, or a system that is not positive definite, ends the
// alignment unconverged.  No NaN can reach T: a step is applied only after solve_damped vouched for a finite delta.
template <class Eval>
int lm_optimise(Eval&& eval, const double T0[16], const LmParams& P, LmResult* res)
{
    double T[16], out[kOut];
    memcpy(T, T0, sizeof T);
    int rc = eval(T, true, out);
    if (rc) return rc;
    res->converged = 0; res->iters = 0; res->n_evals = 1; res->n_rejected = 0;
    double e = out[0], lam = 0.0;
    long long pairs = (long long)out[28];
    if (pairs > 0) {
        for (int k = 0, q = 7; k < 6; q += 6 - k, ++k) lam = std::max(lam, fabs(out[q]));         // the diagonal of the packed triangle
        lam *= P.init_lambda_factor;
        for (int it = 0; it < P.max_iters; ++it) {
            if (it) {
                rc = eval(T, true, out);
                if (rc) return rc;
                ++res->n_evals;
                e = out[0]; pairs = (long long)out[28];
            }
            res->iters = it + 1;
            double H[36], b[6];
            for (int k = 0; k < 6; ++k) b[k] = out[1 + k];
            for (int i = 0, q = 7; i < 6; ++i)
                for (int j = i; j < 6; ++j, ++q) H[6 * i + j] = H[6 * j + i] = out[q];
            double nu = 2.0;
            bool stop = false, accepted = false;
            for (int trial = 0; trial < P.lm_max_iterations; ++trial) {
                double delta[6], E[16], Tn[16], o2[kOut];
                if (!solve_damped(H, b, lam, delta)) { stop = true; break; }
                se3_exp(delta, E);
                mul_rigid(E, T, Tn);
                rc = eval(Tn, false, o2);
                if (rc) return rc;
                ++res->n_evals;
                const double en = o2[0];
                pairs = (long long)o2[28];
                double den = 0.0;
                for (int k = 0; k < 6; ++k) den += delta[k] * (lam * delta[k] - b[k]);
                const double rho = (e - en) / den;
                const bool dconv = delta_converged(delta, P.rotation_epsilon, P.transformation_epsilon);
                if (!(rho >= 0.0)) {
                    ++res->n_rejected;
                    if (dconv) { res->converged = 1; stop = true; break; }
                    lam = nu * lam; nu = 2.0 * nu;
                    continue;
                }
                memcpy(T, Tn, sizeof T);
                e = en;
                const double c = 2.0 * rho - 1.0;
                lam = lam * std::max(1.0 / 3.0, 1.0 - c * c * c);
                accepted = true;
                if (dconv) { res->converged = 1; stop = true; }
                break;
            }
            if (!accepted) stop = true;                             // rejected while converged, not positive definite, or out of trials
            if (stop) break;
        }
    }
    memcpy(res->T, T, sizeof T);
    res->error = e; res->lambda = lam; res->n_pairs_last = pairs;
    return 0;
}

}  // namespace vgicp_host
}  // namespace lisreg
