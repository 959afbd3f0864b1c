// lisreg_vgicp_lane.hpp — what one lane of a VGICP linearisation computes, shared by the single alignment
// (lisreg_vgicp.hip) and the batch (lisreg_vgicp_batch.hip, §7n): the transform of one source point, its voxel, the matrix of the pair,
// the 28 terms and the wavefront sums (lisreg_fp64_sums.hpp).  Both units are built with -ffp-contract=off and inline this body, so a
// lane of either computes the same bits from the same input.  Also the few host helpers of lisreg_vgicp.hip that the batch shares.  Not
// installed.
#pragma once
#include "lisreg_fp64_sums.hpp"
#include "lisreg_vgicp_host.hpp"

#include <string>

namespace lisreg {

static_assert(vgicp_host::kOut == kEvalOut, "one evaluation is 29 doubles in every family");

struct VgPose { double R[9], t[3]; };

// The neighbourhoods DIRECT7 / DIRECT27 (tests/vgicp_nb_ref.py): bit o = (dx + 1) + 3 (dy + 1) + 9 (dz + 1) of the mask is
// set where the neighbourhood keeps the offset (dx, dy, dz); ascending o is ascending cell id.
template <int NB> struct VgNeighbourhood;
template <> struct VgNeighbourhood<7>  { static constexpr unsigned kMask = (1u << 4) | (1u << 10) | (1u << 12) | (1u << 13) | (1u << 14) | (1u << 16) | (1u << 22); };
template <> struct VgNeighbourhood<27> { static constexpr unsigned kMask = (1u << 27) - 1u; };

// One source point per lane, paired with every voxel among the NB cells around its own (NB = 7 or 27).  What depends on the point alone
// is made once: x', the cell f in the floating-point domain, R C_a R^T and J.  Per cell: the bounds test of f + o (in the floating-point
// domain, every offset on its own, so a point whose own cell lies outside the grid still pairs with the voxels inside), one table load
// and, for a voxel, the terms of vg_linearize_lane's one pair.  A lane's term is the left-to-right sum over its pairs in ascending cell
// id; pairs counts them.  A non-finite f fails every comparison.  The cells are walked by a loop, so the Hessian block exists once.
template <bool HESS, int NB>
__device__ __forceinline__ void vg_linearize_lane_nb(bool live, const float4* __restrict__ src_i, const double* __restrict__ ca, const VoxelView& G,
                                                     const VgPose& P, double acc[28], double& pairs)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    pairs = 0.0;
    if (live) {
        const float4 s = *src_i;
        const double a0 = (double)s.x, a1 = (double)s.y, a2 = (double)s.z;
        const double x0 = ((P.R[0] * a0 + P.R[1] * a1) + P.R[2] * a2) + P.t[0];
        const double x1 = ((P.R[3] * a0 + P.R[4] * a1) + P.R[5] * a2) + P.t[1];
        const double x2 = ((P.R[6] * a0 + P.R[7] * a1) + P.R[8] * a2) + P.t[2];
        const double f0 = floor(x0 * G.inv_res) - (double)G.m0, f1 = floor(x1 * G.inv_res) - (double)G.m1, f2 = floor(x2 * G.inv_res) - (double)G.m2;
        const double C[3][3] = { { ca[0], ca[1], ca[2] }, { ca[1], ca[3], ca[4] }, { ca[2], ca[4], ca[5] } };
        double RC[3][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) RC[r][c] = (P.R[3 * r] * C[0][c] + P.R[3 * r + 1] * C[1][c]) + P.R[3 * r + 2] * C[2][c];
        auto rcr = [&](int r, int c) { return (RC[r][0] * P.R[3 * c] + RC[r][1] * P.R[3 * c + 1]) + RC[r][2] * P.R[3 * c + 2]; };
        const double r00 = rcr(0, 0), r01 = rcr(0, 1), r02 = rcr(0, 2), r11 = rcr(1, 1), r12 = rcr(1, 2), r22 = rcr(2, 2);
        // J = [skew(x) | -I], column by column
        const double J[6][3] = { { 0.0, x2, -x1 }, { -x2, 0.0, x0 }, { x1, -x0, 0.0 }, { -1.0, 0.0, 0.0 }, { 0.0, -1.0, 0.0 }, { 0.0, 0.0, -1.0 } };
        const long long row = G.d0, slab = (long long)G.d0 * G.d1;
#pragma clang loop unroll(disable)
        for (int o = 0; o < 27; ++o) {
            if (!((VgNeighbourhood<NB>::kMask >> o) & 1u)) continue;
            const double g0 = f0 + (double)(o % 3 - 1), g1 = f1 + (double)(o / 3 % 3 - 1), g2 = f2 + (double)(o / 9 - 1);
            int v = -1;
            if (g0 >= 0.0 && g0 < (double)G.d0 && g1 >= 0.0 && g1 < (double)G.d1 && g2 >= 0.0 && g2 < (double)G.d2)
                v = G.table[(long long)g0 + (long long)g1 * row + (long long)g2 * slab];
            if (v < 0) continue;
            const double* __restrict__ rec = G.stats + (size_t)v * kVoxelRec;
            const double d[3] = { rec[0] - x0, rec[1] - x1, rec[2] - x2 };
            const double s00 = rec[3] + r00, s01 = rec[4] + r01, s02 = rec[5] + r02;
            const double s11 = rec[6] + r11, s12 = rec[7] + r12, s22 = rec[8] + r22;
            // M = S^-1, closed form, as vg_linearize_lane's
            const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
            const double det = (s00 * c00 + s01 * c01) + s02 * c02;
            const double id = 1.0 / det;
            const double M[3][3] = { { c00 * id, c01 * id, c02 * id },
                                     { c01 * id, (s00 * s22 - s02 * s02) * id, (s01 * s02 - s00 * s12) * id },
                                     { c02 * id, (s01 * s02 - s00 * s12) * id, (s00 * s11 - s01 * s01) * id } };
            const double w = sqrt(rec[9]);
            double Md[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) Md[r] = (M[r][0] * d[0] + M[r][1] * d[1]) + M[r][2] * d[2];
            pairs += 1.0;
            acc[0] += w * ((d[0] * Md[0] + d[1] * Md[1]) + d[2] * Md[2]);
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[1 + a] += w * ((J[a][0] * Md[0] + J[a][1] * Md[1]) + J[a][2] * Md[2]);
            if (HESS) {
                double MJ[6][3];
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int r = 0; r < 3; ++r) MJ[a][r] = (M[r][0] * J[a][0] + M[r][1] * J[a][1]) + M[r][2] * J[a][2];
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b)
                        acc[7 + a * 6 - a * (a - 1) / 2 + (b - a)] += w * ((J[a][0] * MJ[b][0] + J[a][1] * MJ[b][1]) + J[a][2] * MJ[b][2]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = wave_sum(acc[k]);
    pairs = wave_sum(pairs);
}

// One source point per lane: the 28 terms of its pair at P (zeros without one, and on a lane past the source's end: !live) and its 1.0
// or 0.0 for the pair count.  src_i / ca: the lane's point and the six entries of its covariance (read only if live).  The wavefront's
// sums of them are left in acc[28] and pairs on every lane.  This is DIRECT1, the voxel the point falls into; the kernels choose between
// it and vg_linearize_lane_nb above at compile time, so nothing of the neighbour walk reaches it.
template <bool HESS>
__device__ __forceinline__ void vg_linearize_lane(bool live, const float4* __restrict__ src_i, const double* __restrict__ ca, const VoxelView& G,
                                                  const VgPose& P, double acc[28], double& pairs)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    pairs = 0.0;
    if (live) {
        const float4 s = *src_i;
        const double a0 = (double)s.x, a1 = (double)s.y, a2 = (double)s.z;
        const double x0 = ((P.R[0] * a0 + P.R[1] * a1) + P.R[2] * a2) + P.t[0];
        const double x1 = ((P.R[3] * a0 + P.R[4] * a1) + P.R[5] * a2) + P.t[1];
        const double x2 = ((P.R[6] * a0 + P.R[7] * a1) + P.R[8] * a2) + P.t[2];
        // the cell in the floating-point domain first: a point far off the map, a huge or a NaN coordinate fails a comparison here and
        // never becomes an integer
        const double f0 = floor(x0 * G.inv_res) - (double)G.m0, f1 = floor(x1 * G.inv_res) - (double)G.m1, f2 = floor(x2 * G.inv_res) - (double)G.m2;
        int v = -1;
        if (f0 >= 0.0 && f0 < (double)G.d0 && f1 >= 0.0 && f1 < (double)G.d1 && f2 >= 0.0 && f2 < (double)G.d2)
            v = G.table[(long long)f0 + (long long)f1 * G.d0 + (long long)f2 * (long long)G.d0 * G.d1];
        if (v >= 0) {
            const double* __restrict__ rec = G.stats + (size_t)v * kVoxelRec;
            const double d[3] = { rec[0] - x0, rec[1] - x1, rec[2] - x2 };
            const double C[3][3] = { { ca[0], ca[1], ca[2] }, { ca[1], ca[3], ca[4] }, { ca[2], ca[4], ca[5] } };
            double RC[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) RC[r][c] = (P.R[3 * r] * C[0][c] + P.R[3 * r + 1] * C[1][c]) + P.R[3 * r + 2] * C[2][c];
            auto rcr = [&](int r, int c) { return (RC[r][0] * P.R[3 * c] + RC[r][1] * P.R[3 * c + 1]) + RC[r][2] * P.R[3 * c + 2]; };
            const double s00 = rec[3] + rcr(0, 0), s01 = rec[4] + rcr(0, 1), s02 = rec[5] + rcr(0, 2);
            const double s11 = rec[6] + rcr(1, 1), s12 = rec[7] + rcr(1, 2), s22 = rec[8] + rcr(2, 2);
            // M = S^-1, closed form (S is symmetric positive definite with eigenvalues between 2 plane_epsilon and 2)
            const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
            const double det = (s00 * c00 + s01 * c01) + s02 * c02;
            const double id = 1.0 / det;
            const double M[3][3] = { { c00 * id, c01 * id, c02 * id },
                                     { c01 * id, (s00 * s22 - s02 * s02) * id, (s01 * s02 - s00 * s12) * id },
                                     { c02 * id, (s01 * s02 - s00 * s12) * id, (s00 * s11 - s01 * s01) * id } };
            const double w = sqrt(rec[9]);
            double Md[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) Md[r] = (M[r][0] * d[0] + M[r][1] * d[1]) + M[r][2] * d[2];
            // J = [skew(x) | -I], column by column
            const double J[6][3] = { { 0.0, x2, -x1 }, { -x2, 0.0, x0 }, { x1, -x0, 0.0 }, { -1.0, 0.0, 0.0 }, { 0.0, -1.0, 0.0 }, { 0.0, 0.0, -1.0 } };
            pairs = 1.0;
            acc[0] = w * ((d[0] * Md[0] + d[1] * Md[1]) + d[2] * Md[2]);
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[1 + a] = w * ((J[a][0] * Md[0] + J[a][1] * Md[1]) + J[a][2] * Md[2]);
            if (HESS) {
                double MJ[6][3];
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int r = 0; r < 3; ++r) MJ[a][r] = (M[r][0] * J[a][0] + M[r][1] * J[a][1]) + M[r][2] * J[a][2];
#pragma unroll
                for (int a = 0; a < 6; ++a)
#pragma unroll
                    for (int b = a; b < 6; ++b)
                        acc[7 + a * 6 - a * (a - 1) / 2 + (b - a)] = w * ((J[a][0] * MJ[b][0] + J[a][1] * MJ[b][1]) + J[a][2] * MJ[b][2]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = wave_sum(acc[k]);
    pairs = wave_sum(pairs);
}

// neighbor_search of a parameter struct: its last int, which keeps the member name `reserved` (include/lisreg.h says why)
inline int vg_neighbor_search(const lisreg_vgicp_params& P) { return P.reserved; }

// ---- lisreg_vgicp.hip: the host checks of every VGICP entry point (one copy) -----------------------------------------------------------
// P may be null in vg_find_target: the slot's resolution is then not compared
int vg_check_params(lisreg_ctx* c, const lisreg_vgicp_params* P, const char* who);
int vg_find_target(lisreg_ctx* c, int slot, const lisreg_vgicp_params* P, const char* who, VgicpTarget** out);

}  // namespace lisreg
