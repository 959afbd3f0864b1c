// lisreg_icp_step.hpp — the closed-form step of pcl::IterativeClosestPoint on the device, shared by every ICP kernel:
// svd3 (3x3 one-sided Jacobi), det3, and icp_solve_step (TransformationEstimationSVD + final_transformation_ update +
// DefaultConvergenceCriteria::hasConverged).  Device functions only; each translation unit gets its own copy.
#pragma once
#include "lisreg_internal.hpp"

namespace lisreg {
namespace {

// 3x3 SVD by one-sided Jacobi (double); U S V^T = A, singular values descending, U completed to an orthogonal matrix
__device__ void svd3(const double* Ain, double* U, double* S, double* V)
{
    double A[9];
    for (int i = 0; i < 9; ++i) { A[i] = Ain[i]; V[i] = (i % 4 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double a = 0, b = 0, c = 0;
                for (int r = 0; r < 3; ++r) { a += A[3 * r + p] * A[3 * r + p]; b += A[3 * r + q] * A[3 * r + q]; c += A[3 * r + p] * A[3 * r + q]; }
                if (fabs(c) <= 1e-300 || fabs(c) <= 1e-15 * sqrt(a * b)) continue;
                off += fabs(c);
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < 3; ++r) {
                    double x = A[3 * r + p], y = A[3 * r + q];
                    A[3 * r + p] = cs * x - sn * y; A[3 * r + q] = sn * x + cs * y;
                    x = V[3 * r + p]; y = V[3 * r + q];
                    V[3 * r + p] = cs * x - sn * y; V[3 * r + q] = sn * x + cs * y;
                }
            }
        if (off == 0) break;
    }
    double nrm[3];
    int ord[3] = { 0, 1, 2 };
    for (int j = 0; j < 3; ++j) nrm[j] = sqrt(A[j] * A[j] + A[3 + j] * A[3 + j] + A[6 + j] * A[6 + j]);
    for (int i = 0; i < 2; ++i) for (int j = i + 1; j < 3; ++j) if (nrm[ord[j]] > nrm[ord[i]]) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
    double Vs[9];
    for (int j = 0; j < 3; ++j) {
        S[j] = nrm[ord[j]];
        for (int r = 0; r < 3; ++r) { Vs[3 * r + j] = V[3 * r + ord[j]]; U[3 * r + j] = S[j] > 0 ? A[3 * r + ord[j]] / S[j] : 0.0; }
    }
    for (int i = 0; i < 9; ++i) V[i] = Vs[i];
    const double tiny = 1e-12 * (S[0] > 0 ? S[0] : 1.0);
    if (S[1] <= tiny) {
        if (S[0] <= 0) { U[0] = 1; U[3] = 0; U[6] = 0; }
        const double u0[3] = { U[0], U[3], U[6] };
        const int k = fabs(u0[0]) < fabs(u0[1]) ? (fabs(u0[0]) < fabs(u0[2]) ? 0 : 2) : (fabs(u0[1]) < fabs(u0[2]) ? 1 : 2);
        double e[3] = { 0, 0, 0 }; e[k] = 1;
        const double d = u0[k];
        double u1[3] = { e[0] - d * u0[0], e[1] - d * u0[1], e[2] - d * u0[2] };
        const double n1 = sqrt(u1[0] * u1[0] + u1[1] * u1[1] + u1[2] * u1[2]);
        for (int r = 0; r < 3; ++r) U[3 * r + 1] = u1[r] / n1;
    }
    if (S[2] <= tiny) {
        U[2] = U[3] * U[7] - U[6] * U[4];
        U[5] = U[6] * U[1] - U[0] * U[7];
        U[8] = U[0] * U[4] - U[3] * U[1];
    }
}

__device__ __forceinline__ double det3(const double* M)
{
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// estimateRigidTransformation (Umeyama, no scale) + final_transformation_ update + DefaultConvergenceCriteria::hasConverged
__device__ void icp_solve_step(const double* tot, IcpState* st, int max_iters, double eps_t, double eps_mse)
{
    const double cnt = tot[0];
    st->n_corr = (int)cnt;
    if (cnt < 3.0) { st->state = LISREG_ICP_NO_CORRESPONDENCES; st->converged = 0; st->done = 1; return; }    // icp.hpp: min_number_correspondences_
    const double inv = 1.0 / cnt;
    const double ms[3] = { tot[1] * inv, tot[2] * inv, tot[3] * inv }, md[3] = { tot[4] * inv, tot[5] * inv, tot[6] * inv };
    double sg[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) sg[3 * r + c] = tot[7 + 3 * r + c] * inv - md[r] * ms[c];
    double U[9], S[3], V[9], R[9];
    svd3(sg, U, S, V);
    const double s2 = det3(U) * det3(V) < 0 ? -1.0 : 1.0;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c)
        R[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1] + s2 * U[3 * r + 2] * V[3 * c + 2];
    float Tm[16];
    for (int i = 0; i < 16; ++i) Tm[i] = (i % 5 == 0) ? 1.f : 0.f;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Tm[4 * r + c] = (float)R[3 * r + c];
        Tm[4 * r + 3] = (float)(md[r] - (R[3 * r] * ms[0] + R[3 * r + 1] * ms[1] + R[3 * r + 2] * ms[2]));
    }
    float Fn[16];
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c)
        Fn[4 * r + c] = ((Tm[4 * r] * st->F[c] + Tm[4 * r + 1] * st->F[4 + c]) + Tm[4 * r + 2] * st->F[8 + c]) + Tm[4 * r + 3] * st->F[12 + c];
    for (int i = 0; i < 16; ++i) { st->F[i] = Fn[i]; st->Tm[i] = Tm[i]; }
    const int iters = ++st->iters;
    st->state = LISREG_ICP_NOT_CONVERGED;
    if (iters >= max_iters) { st->state = LISREG_ICP_ITERATIONS; st->converged = 1; st->done = 1; return; }
    const double cos_angle = 0.5 * ((double)Tm[0] + (double)Tm[5] + (double)Tm[10] - 1.0);
    const double tr2 = (double)Tm[3] * Tm[3] + (double)Tm[7] * Tm[7] + (double)Tm[11] * Tm[11];
    if (cos_angle >= 1.0 - eps_t && tr2 <= eps_t) { st->state = LISREG_ICP_TRANSFORM; st->converged = 1; st->done = 1; return; }
    // calculateMSE divides (default_convergence_criteria.hpp): tot[16] * inv is up to one ulp off it, which decides the absolute test
    // when an alignment starts from the value the one before it left behind
    const double cur = tot[16] / cnt, prev = st->prev_mse;
    st->cur_mse = cur;
    if (iters == 1) st->first_mse = cur;                 // the MSE test of the first iteration was reached (chained batches)
    // chained batch (the reference's `static` ICP object, subMapOptmizationNode.cpp:2763): this item's correspondences_prev_mse_ is the
    // value the item before it leaves behind, unknown while both run together — the first comparison is made by the host afterwards
    if (iters == 1 && st->defer_first) { st->prev_mse = cur; return; }
    if (fabs(cur - prev) < 1e-12) { st->state = LISREG_ICP_ABS_MSE; st->converged = 1; st->done = 1; return; }
    if (fabs(cur - prev) / prev < eps_mse) { st->state = LISREG_ICP_REL_MSE; st->converged = 1; st->done = 1; return; }
    st->prev_mse = cur;
}

}  // namespace
}  // namespace lisreg
