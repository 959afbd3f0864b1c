// lisreg_vgicp_host.hpp — the host half of the VGICP registration (lisreg_vgicp.hip): the SE(3) exponential, the damped 6 x 6 solve, the
// convergence test and the parameter / result records of the Levenberg-Marquardt loop (the loop itself: lisreg_lm_stepper.hpp), in
// double, statement by statement what tests/vgicp_ref.py defines, and the small conversions the family's entry points share.  Plain C++
// (no HIP), so that it can be compiled and checked on its own.  Not installed.
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

// ---- what the four entry points of the fast_gicp family (the two aligners and their batch forms) do around the loop ---------------
// the start of a run: the caller's row-major 4 x 4 (NULL: the identity) in double, the last row forced to 0 0 0 1
inline void guess_to_T0(const float* guess, double T0[16])
{
    for (int k = 0; k < 16; ++k) T0[k] = guess ? (double)guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
    T0[12] = T0[13] = T0[14] = 0.0; T0[15] = 1.0;
}

// R[9], t[3] of a row-major 4 x 4 (VgPose, FgPose)
template <class Pose>
inline Pose pose_of(const double T[16])
{
    Pose P;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) P.R[3 * i + j] = T[4 * i + j]; P.t[i] = T[4 * i + 3]; }
    return P;
}

// lisreg_vgicp_params / lisreg_fgicp_params -> LmParams, LmResult -> lisreg_vgicp_result / lisreg_fgicp_result
template <class Params>
inline LmParams lm_params_of(const Params& P)
{
    return LmParams{ P.transformation_epsilon, P.rotation_epsilon, P.lm_init_lambda_factor, P.max_iters, P.lm_max_iterations };
}

template <class Result>
inline void lm_result_to(const LmResult& lr, Result* res)
{
    memcpy(res->final_transform, lr.T, sizeof lr.T);
    res->converged = lr.converged; res->iters = lr.iters; res->n_evals = lr.n_evals; res->n_rejected = lr.n_rejected;
    res->n_pairs_last = lr.n_pairs_last; res->error = lr.error; res->lambda = lr.lambda;
}

}  // namespace vgicp_host
}  // namespace lisreg
