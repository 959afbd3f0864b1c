// lisreg_ndt_host.hpp — the host half of the NDT registration (lisreg_ndt.hip): pose matrices, the 6 x 6 pseudo-inverse solve and the
// pieces of the More-Thuente line search that hold no state (the trial value, the interval update), in double, statement by statement
// what tests/ndt_ref.py defines; the loop that drives them is lisreg_ndt_stepper.hpp.  Plain C++ (no HIP), so that it can be compiled
// and checked on its own.  Not installed.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

namespace lisreg {
namespace ndt_host {

struct NdtPose { double R[9], t[3], dR[27], ddR[54]; };       // R: true trigonometry; dR [3], ddR [aa, ab, ac, bb, bc, cc]: small-angle shortcut

inline void mat3(const double A[9], const double B[9], double C[9])
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}
inline void elem(int axis, double c, double s, double M[9], double M1[9], double M2[9])
{
    if (axis == 0) {
        const double a[9] = { 1, 0, 0, 0, c, -s, 0, s, c }, b[9] = { 0, 0, 0, 0, -s, -c, 0, c, -s }, d[9] = { 0, 0, 0, 0, -c, s, 0, -s, -c };
        memcpy(M, a, sizeof a); memcpy(M1, b, sizeof b); memcpy(M2, d, sizeof d);
    } else if (axis == 1) {
        const double a[9] = { c, 0, s, 0, 1, 0, -s, 0, c }, b[9] = { -s, 0, c, 0, 0, 0, -c, 0, -s }, d[9] = { -c, 0, -s, 0, 0, 0, s, 0, -c };
        memcpy(M, a, sizeof a); memcpy(M1, b, sizeof b); memcpy(M2, d, sizeof d);
    } else {
        const double a[9] = { c, -s, 0, s, c, 0, 0, 0, 1 }, b[9] = { -s, -c, 0, c, -s, 0, 0, 0, 0 }, d[9] = { -c, s, 0, -s, -c, 0, 0, 0, 0 };
        memcpy(M, a, sizeof a); memcpy(M1, b, sizeof b); memcpy(M2, d, sizeof d);
    }
}
inline void prod3(const double A[9], const double B[9], const double C[9], double out[9]) { double t[9]; mat3(A, B, t); mat3(t, C, out); }

inline void pose_matrices(const double p[6], NdtPose* P)
{
    double X[9], Y[9], Z[9], X1[9], Y1[9], Z1[9], X2[9], Y2[9], Z2[9];
    elem(0, cos(p[3]), sin(p[3]), X, X1, X2); elem(1, cos(p[4]), sin(p[4]), Y, Y1, Y2); elem(2, cos(p[5]), sin(p[5]), Z, Z1, Z2);
    prod3(X, Y, Z, P->R);
    for (int k = 0; k < 3; ++k) P->t[k] = p[k];
    double cs[3][2];
    for (int k = 0; k < 3; ++k) {                                  // the small-angle shortcut of the derivatives
        const bool small = fabs(p[3 + k]) < 10e-5;
        cs[k][0] = small ? 1.0 : cos(p[3 + k]); cs[k][1] = small ? 0.0 : sin(p[3 + k]);
    }
    elem(0, cs[0][0], cs[0][1], X, X1, X2); elem(1, cs[1][0], cs[1][1], Y, Y1, Y2); elem(2, cs[2][0], cs[2][1], Z, Z1, Z2);
    prod3(X1, Y, Z, P->dR); prod3(X, Y1, Z, P->dR + 9); prod3(X, Y, Z1, P->dR + 18);
    prod3(X2, Y, Z, P->ddR); prod3(X1, Y1, Z, P->ddR + 9); prod3(X1, Y, Z1, P->ddR + 18);
    prod3(X, Y2, Z, P->ddR + 27); prod3(X, Y1, Z1, P->ddR + 36); prod3(X, Y, Z2, P->ddR + 45);
}

inline void p_from_matrix(const float* M, double p[6])
{
    if (!M) { for (int k = 0; k < 6; ++k) p[k] = 0.0; return; }
    p[0] = M[3]; p[1] = M[7]; p[2] = M[11];
    p[3] = atan2(-(double)M[6], (double)M[10]);
    p[4] = asin(std::min(1.0, std::max(-1.0, (double)M[2])));
    p[5] = atan2(-(double)M[1], (double)M[0]);
}

// delta = H^+ (-g): one-sided Jacobi SVD (H V = U S), singular values <= 6 eps s_max dropped
inline void solve_step(const double Hm[36], const double g[6], double delta[6])
{
    double A[6][6], V[6][6];
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < 6; ++j) { A[i][j] = Hm[6 * i + j]; V[i][j] = i == j ? 1.0 : 0.0; }
    for (int i = 0; i < 36; ++i)
        if (!std::isfinite(Hm[i])) { for (int k = 0; k < 6; ++k) delta[k] = NAN; return; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                double al = 0, be = 0, ga = 0;
                for (int k = 0; k < 6; ++k) { al += A[k][p] * A[k][p]; be += A[k][q] * A[k][q]; ga += A[k][p] * A[k][q]; }
                if (ga == 0.0 || fabs(ga) <= 1.0e-16 * sqrt(al * be)) continue;
                rotated = true;
                const double ze = (be - al) / (2.0 * ga);
                const double t = (ze >= 0.0 ? 1.0 : -1.0) / (fabs(ze) + sqrt(1.0 + ze * ze));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int k = 0; k < 6; ++k) {
                    const double a = A[k][p], b = A[k][q]; A[k][p] = cs * a - sn * b; A[k][q] = sn * a + cs * b;
                    const double u = V[k][p], w = V[k][q]; V[k][p] = cs * u - sn * w; V[k][q] = sn * u + cs * w;
                }
            }
        if (!rotated) break;
    }
    double s[6], smax = 0;
    for (int j = 0; j < 6; ++j) { double a = 0; for (int k = 0; k < 6; ++k) a += A[k][j] * A[k][j]; s[j] = sqrt(a); smax = std::max(smax, s[j]); }
    for (int k = 0; k < 6; ++k) delta[k] = 0.0;
    for (int j = 0; j < 6; ++j) {
        if (!(s[j] > 6.0 * DBL_EPSILON * smax)) continue;
        double y = 0;                                                 // u_j . (-g) / s_j, u_j = A[:, j] / s_j
        for (int k = 0; k < 6; ++k) y += A[k][j] * -g[k];
        y /= s[j] * s[j];
        for (int k = 0; k < 6; ++k) delta[k] += V[k][j] * y;
    }
}

constexpr double kMu = 1.0e-4, kNu = 0.9;
constexpr int kMaxTrials = 10;

inline bool cubic_min(double a_e, double f_e, double g_e, double a_t, double f_t, double g_t, double* out)
{
    const double z = 3.0 * (f_t - f_e) / (a_t - a_e) - g_t - g_e;
    const double disc = z * z - g_t * g_e;
    if (!(disc >= 0)) return false;
    const double w = sqrt(disc), den = g_t - g_e + 2.0 * w;
    if (den == 0) return false;
    *out = a_e + (a_t - a_e) * (w - g_e - z) / den;
    return std::isfinite(*out);
}

// I = a_l, f_l, g_l, a_u, f_u, g_u; false: no finite value (the search ends)
inline bool trial_value(const double I[6], double a_t, double f_t, double g_t, double* out)
{
    const double a_l = I[0], f_l = I[1], g_l = I[2], a_u = I[3], f_u = I[4], g_u = I[5];
    double a_c = 0;
    if (f_t > f_l) {                                                                       // case 1
        const bool hc = cubic_min(a_l, f_l, g_l, a_t, f_t, g_t, &a_c);
        const double a_q = a_l - 0.5 * (a_l - a_t) * g_l / (g_l - (f_l - f_t) / (a_l - a_t));
        if (!hc) { *out = a_q; return std::isfinite(a_q); }
        if (!std::isfinite(a_q)) { *out = a_c; return true; }
        *out = fabs(a_c - a_l) < fabs(a_q - a_l) ? a_c : 0.5 * (a_q + a_c);
        return true;
    }
    if (g_t * g_l < 0.0) {                                                                 // case 2
        const bool hc = cubic_min(a_l, f_l, g_l, a_t, f_t, g_t, &a_c);
        const double a_s = a_l - (a_l - a_t) / (g_l - g_t) * g_l;
        if (!hc) { *out = a_s; return std::isfinite(a_s); }
        *out = fabs(a_c - a_t) >= fabs(a_s - a_t) ? a_c : a_s;
        return true;
    }
    if (fabs(g_t) <= fabs(g_l)) {                                                          // case 3
        const bool hc = cubic_min(a_l, f_l, g_l, a_t, f_t, g_t, &a_c);
        const double a_s = g_l != g_t ? a_l - (a_l - a_t) / (g_l - g_t) * g_l : INFINITY;
        const double guard = a_t + 0.66 * (a_u - a_t);
        double nxt;
        if (hc && std::isfinite(a_s)) nxt = fabs(a_c - a_t) < fabs(a_s - a_t) ? a_c : a_s;
        else if (hc) nxt = a_c;
        else if (std::isfinite(a_s)) nxt = a_s;
        else { *out = guard; return true; }
        *out = a_t > a_l ? std::min(guard, nxt) : std::max(guard, nxt);
        return true;
    }
    if (a_t == a_u) return false;                                                          // case 4
    return cubic_min(a_u, f_u, g_u, a_t, f_t, g_t, out);
}

inline bool update_interval(double I[6], double a_t, double f_t, double g_t)
{
    if (f_t > I[1]) { I[3] = a_t; I[4] = f_t; I[5] = g_t; return false; }                // U1
    const double s = g_t * (I[0] - a_t);
    if (s > 0) { I[0] = a_t; I[1] = f_t; I[2] = g_t; return false; }                      // U2
    if (s < 0) { I[3] = I[0]; I[4] = I[1]; I[5] = I[2]; I[0] = a_t; I[1] = f_t; I[2] = g_t; return false; }   // U3
    return true;
}

inline void gauss_constants(double o, double res, double* g1, double* g2)
{
    const double c1 = 10.0 * (1.0 - o), c2 = o / (res * res * res);
    const double d3 = -log(c2);
    *g1 = -log(c1 + c2) - d3;
    *g2 = -2.0 * log((-log(c1 * exp(-0.5) + c2) - d3) / *g1);
}

}  // namespace ndt_host
}  // namespace lisreg
