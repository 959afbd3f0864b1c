// lisreg_ndt_lane.hpp — what one lane of the NDT evaluation kernels computes, shared by the single call (k_ndt_eval,
// lisreg_ndt.hip) and the batch (k_ndt_eval_batch, lisreg_ndt_batch.hip, §7o): the transform of one source record, the walk over the 27
// voxels around it, its 28 terms and its pair count.  Both units are built with -ffp-contract=off and inline this body, so a lane of
// either computes the same bits from the same input.  Also the few host helpers of lisreg_ndt.hip that the batch shares.  Not installed.
#pragma once
#include "lisreg_fp64_sums.hpp"
#include "lisreg_ndt_stepper.hpp"

namespace lisreg {

static_assert(ndt_host::kNdtOut == kEvalOut, "one evaluation is 29 doubles in every family");

using ndt_host::NdtPose;                                        // R, t, dR [3], ddR [6]: plain doubles, read by the lanes as they are
struct NdtGauss { double r2, g1, g2; };                         // resolution^2, the Gaussian constants d1, d2

// One source record per lane: acc[28] = its terms of the score, the gradient and (HESS) the upper triangle of the Hessian, pairs = its
// (point, voxel) pairs, as this lane's own sums (the caller adds the wavefront's).  live = false, or a NaN coordinate: zeros.  G, K and
// P are read at constant offsets only: behind a wave-uniform address they stay scalar.
template <bool HESS>
__device__ __forceinline__ void ndt_eval_lane(bool live, const float4* __restrict__ src_i, const VoxelView& G, const NdtGauss& K, const NdtPose& P,
                                              double acc[28], double& pairs)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    pairs = 0.0;
    double x0 = 0, x1 = 0, x2 = 0;
    if (live) { const float4 s = *src_i; x0 = (double)s.x; x1 = (double)s.y; x2 = (double)s.z; }
    const double t0 = ((P.R[0] * x0 + P.R[1] * x1) + P.R[2] * x2) + P.t[0];
    const double t1 = ((P.R[3] * x0 + P.R[4] * x1) + P.R[5] * x2) + P.t[1];
    const double t2 = ((P.R[6] * x0 + P.R[7] * x1) + P.R[8] * x2) + P.t[2];
    live = live && t0 == t0 && t1 == t1 && t2 == t2;
    if (live) {
        double J[6][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 }, { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };
        double Hv[6][3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int r = 0; r < 3; ++r) J[3 + k][r] = (P.dR[9 * k + 3 * r] * x0 + P.dR[9 * k + 3 * r + 1] * x1) + P.dR[9 * k + 3 * r + 2] * x2;
        if (HESS) {
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int r = 0; r < 3; ++r) Hv[k][r] = (P.ddR[9 * k + 3 * r] * x0 + P.ddR[9 * k + 3 * r + 1] * x1) + P.ddR[9 * k + 3 * r + 2] * x2;
        }
        const long long c0 = (long long)fmin(fmax(floor(t0 * G.inv_res), -2.0e9), 2.0e9) - G.m0;
        const long long c1 = (long long)fmin(fmax(floor(t1 * G.inv_res), -2.0e9), 2.0e9) - G.m1;
        const long long c2 = (long long)fmin(fmax(floor(t2 * G.inv_res), -2.0e9), 2.0e9) - G.m2;
        for (int dz = -1; dz <= 1; ++dz) {
            const long long z = c2 + dz;
            if (z < 0 || z >= G.d2) continue;
            for (int dy = -1; dy <= 1; ++dy) {
                const long long y = c1 + dy;
                if (y < 0 || y >= G.d1) continue;
                for (int dx = -1; dx <= 1; ++dx) {
                    const long long x = c0 + dx;
                    if (x < 0 || x >= G.d0) continue;
                    const int v = G.table[x + y * G.d0 + z * (long long)G.d0 * G.d1];
                    if (v < 0) continue;
                    const double* __restrict__ rec = G.stats + (size_t)v * kVoxelRec;
                    const double q0 = t0 - rec[0], q1 = t1 - rec[1], q2 = t2 - rec[2];
                    if (!((q0 * q0 + q1 * q1) + q2 * q2 <= K.r2)) continue;
                    const double C[3][3] = { { rec[3], rec[4], rec[5] }, { rec[4], rec[6], rec[7] }, { rec[5], rec[7], rec[8] } };
                    double cq[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) cq[r] = (C[r][0] * q0 + C[r][1] * q1) + C[r][2] * q2;
                    const double e = exp(-K.g2 * ((q0 * cq[0] + q1 * cq[1]) + q2 * cq[2]) / 2.0);
                    pairs += 1.0;
                    acc[0] += -K.g1 * e;
                    double w = K.g2 * e;
                    if (w > 1.0 || w < 0.0 || w != w) continue;
                    w *= K.g1;
                    double cJ[6];
#pragma unroll
                    for (int a = 0; a < 6; ++a) cJ[a] = (cq[0] * J[a][0] + cq[1] * J[a][1]) + cq[2] * J[a][2];
#pragma unroll
                    for (int a = 0; a < 6; ++a) acc[1 + a] += w * cJ[a];
                    if (HESS) {
                        double CJ[6][3];
#pragma unroll
                        for (int a = 0; a < 6; ++a)
#pragma unroll
                            for (int r = 0; r < 3; ++r) CJ[a][r] = (C[r][0] * J[a][0] + C[r][1] * J[a][1]) + C[r][2] * J[a][2];
#pragma unroll
                        for (int a = 0; a < 6; ++a)
#pragma unroll
                            for (int b = a; b < 6; ++b) {
                                double t = -K.g2 * cJ[a] * cJ[b] + ((J[b][0] * CJ[a][0] + J[b][1] * CJ[a][1]) + J[b][2] * CJ[a][2]);
                                if (a >= 3) {
                                    const int h = a == 3 ? b - 3 : (a == 4 ? b - 1 : 5);          // aa ab ac | bb bc | cc
                                    t += (cq[0] * Hv[h][0] + cq[1] * Hv[h][1]) + cq[2] * Hv[h][2];
                                }
                                acc[7 + a * 6 - a * (a - 1) / 2 + (b - a)] += w * t;
                            }
                    }
                }
            }
        }
    }
}

// the wavefront's sums of the lanes' terms, stored by lane 0 as one partial record
__device__ __forceinline__ void ndt_store_partial(double acc[28], double pairs, double* __restrict__ o)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = wave_sum(acc[k]);
    pairs = wave_sum(pairs);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 28; ++k) o[k] = acc[k];
        o[28] = pairs;
    }
}

// ---- lisreg_ndt.hip: the host checks of every NDT entry point (one copy) ----------------------------------------------------------------
int ndt_check_params(lisreg_ctx* c, const lisreg_ndt_params* P, const char* who);
int ndt_find_target(lisreg_ctx* c, int slot, const lisreg_ndt_params* P, const char* who, NdtTarget** out);
// lisreg_ndt_result of a finished run (final_transform = the float image of pose_matrices(p))
void ndt_result_to(const ndt_host::NdtLoopResult& lr, lisreg_ndt_result* res);
// what the loop reads of lisreg_ndt_params
inline ndt_host::NdtLoopParams ndt_loop_params_of(const lisreg_ndt_params& P)
{
    return ndt_host::NdtLoopParams{ P.step_size, P.transformation_epsilon, P.max_iters, P.line_search };
}

}  // namespace lisreg
