// lisreg_fgicp_lane.hpp — what one lane of the FastGICP kernels computes, shared by the single alignment
// (lisreg_fgicp.hip) and the batch (lisreg_fgicp_batch.hip, §7m): the search of one query, the matrix of one pair, the 28 terms of one
// pair and the wavefront sums (lisreg_fp64_sums.hpp).  Both units are built with -ffp-contract=off and inline these bodies, so a lane
// of either computes the same bits from the same input.  Also the few host helpers of lisreg_fgicp.hip that the batch shares.  Not
// installed.
#pragma once
#include "lisreg_fp64_sums.hpp"
#include "lisreg_vgicp_host.hpp"

#include <string>

namespace lisreg {

struct FgTarget {
    const float4* sorted;       // [m] by grid cell; .w = index among the finite points (ascending with the caller's index)
    const int*    cell_start;   // [nx * ny * nz + 1], cell = (ix * ny + iy) * nz + iz
    const double* cov;          // [m][6] by index among the finite points
    float  ox, oy, oz, cell;
    int    nx, ny, nz;
    double b0[3], b1[3];        // the finite bounding box
};
struct FgPose { double R[9], t[3]; };

static_assert(vgicp_host::kOut == kEvalOut, "one evaluation is 29 doubles in every family");

__device__ __forceinline__ void fg_transform(const FgPose& P, const float4 s, double& x0, double& x1, double& x2)
{
    const double a0 = (double)s.x, a1 = (double)s.y, a2 = (double)s.z;
    x0 = ((P.R[0] * a0 + P.R[1] * a1) + P.R[2] * a2) + P.t[0];
    x1 = ((P.R[3] * a0 + P.R[4] * a1) + P.R[5] * a2) + P.t[1];
    x2 = ((P.R[6] * a0 + P.R[7] * a1) + P.R[8] * a2) + P.t[2];
}

// the grid coordinate of a query along one axis, clamped to the grid while it is still a double
__device__ __forceinline__ int fg_cell(double v, float origin, double inv_cell, int n)
{
    double c = floor((v - (double)origin) * inv_cell);
    c = c < 0.0 ? 0.0 : (c > (double)(n - 1) ? (double)(n - 1) : c);
    return (int)c;
}

// The nearest finite target point of the query (qx, qy, qz), exactly.  Shells of cells are walked outward from the (clamped) cell of the
// query as k_vg_knn walks them; the best (squared distance, sorted position) lives in two registers, a tie is decided by the points'
// indices.  The walk ends when the best squared distance is no larger than the square of the distance to the nearest face with unvisited
// cells behind it (less 1e-3 cell: a point's cell comes from float arithmetic, so a point of an unvisited cell can lie that little inside
// the face), when that bound alone reaches max_d (nothing further out can be a pair), or when the whole grid has been visited: the
// result does not depend on the cell edge.  A query outside the grid's box starts from the border cell; the face bounds are distances to
// planes the query lies on the visited side of, so they hold there too.  A NaN or huge query fails the first comparison and never
// becomes an integer.  bd = the squared distance of the nearest point found (HUGE_VAL: none), bj = its sorted position (-1: none); the
// caller applies the cut-off (bd < max2, strict).
__device__ __forceinline__ void fg_search_lane(const FgTarget& A, double qx, double qy, double qz, double max_d, double max2, double& bd, int& bj)
{
    // the distance to the target's bounding box: no point of the target is nearer
    const double e0 = fmax(fmax(A.b0[0] - qx, qx - A.b1[0]), 0.0), e1 = fmax(fmax(A.b0[1] - qy, qy - A.b1[1]), 0.0),
                 e2 = fmax(fmax(A.b0[2] - qz, qz - A.b1[2]), 0.0);
    const double box2 = (e0 * e0 + e1 * e1) + e2 * e2;
    bd = HUGE_VAL;
    bj = -1;
    if (qx == qx && qy == qy && qz == qz && box2 < max2) {
        const double cell = (double)A.cell, inv_cell = 1.0 / cell, slack = 1.0e-3 * cell;
        const int cx = fg_cell(qx, A.ox, inv_cell, A.nx), cy = fg_cell(qy, A.oy, inv_cell, A.ny), cz = fg_cell(qz, A.oz, inv_cell, A.nz);
        const int rmax = max(max(A.nx, A.ny), A.nz);
        for (int r = 0; r <= rmax; ++r) {
            const int x0 = max(cx - r, 0), x1 = min(cx + r, A.nx - 1);
            const int y0 = max(cy - r, 0), y1 = min(cy + r, A.ny - 1);
            const int z0 = max(cz - r, 0), z1 = min(cz + r, A.nz - 1);
            for (int ix = x0; ix <= x1; ++ix)
                for (int iy = y0; iy <= y1; ++iy) {
                    const int base = (ix * A.ny + iy) * A.nz;
                    const bool rim = ix == cx - r || ix == cx + r || iy == cy - r || iy == cy + r;
                    // a rim column is new over its whole z range; inside the rim only the two caps are (r >= 1 there)
                    for (int part = 0; part < (rim ? 1 : 2); ++part) {
                        const int za = rim ? z0 : (part == 0 ? cz - r : cz + r), zb = rim ? z1 : za;
                        if (za < 0 || zb >= A.nz) continue;
                        const int ja = A.cell_start[base + za], jb = A.cell_start[base + zb + 1];
                        for (int j = ja; j < jb; ++j) {
                            const float4 p = A.sorted[j];
                            const double dx = (double)p.x - qx, dy = (double)p.y - qy, dz = (double)p.z - qz;
                            const double d = (dx * dx + dy * dy) + dz * dz;
                            if (d < bd) { bd = d; bj = j; }
                            else if (d == bd && __float_as_int(p.w) < __float_as_int(A.sorted[bj].w)) bj = j;     // (d == bd: bj >= 0)
                        }
                    }
                }
            double lim = HUGE_VAL;                                  // distance to the nearest face with unvisited cells behind it
            if (cx - r > 0)        lim = fmin(lim, qx - ((double)A.ox + (double)(cx - r) * cell));
            if (cx + r < A.nx - 1) lim = fmin(lim, ((double)A.ox + (double)(cx + r + 1) * cell) - qx);
            if (cy - r > 0)        lim = fmin(lim, qy - ((double)A.oy + (double)(cy - r) * cell));
            if (cy + r < A.ny - 1) lim = fmin(lim, ((double)A.oy + (double)(cy + r + 1) * cell) - qy);
            if (cz - r > 0)        lim = fmin(lim, qz - ((double)A.oz + (double)(cz - r) * cell));
            if (cz + r < A.nz - 1) lim = fmin(lim, ((double)A.oz + (double)(cz + r + 1) * cell) - qz);
            if (lim == HUGE_VAL) break;                             // the whole grid has been visited
            lim -= slack;
            if (lim > 0.0 && (bd <= lim * lim || lim >= max_d)) break;
        }
    }
}

// M = (C_b + R C_a R^T)^-1 of the pair (source point with covariance ca[6], target point at sorted position bj), written to o[6] as
// xx, xy, xz, yy, yz, zz
__device__ __forceinline__ void fg_pair_matrix_lane(const FgTarget& A, const FgPose& P, int bj, const double* __restrict__ ca, double* __restrict__ o)
{
    const double* __restrict__ cb = A.cov + (size_t)__float_as_int(A.sorted[bj].w) * 6;
    const double C[3][3] = { { ca[0], ca[1], ca[2] }, { ca[1], ca[3], ca[4] }, { ca[2], ca[4], ca[5] } };
    double RC[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) RC[r][c] = (P.R[3 * r] * C[0][c] + P.R[3 * r + 1] * C[1][c]) + P.R[3 * r + 2] * C[2][c];
    auto rcr = [&](int r, int c) { return (RC[r][0] * P.R[3 * c] + RC[r][1] * P.R[3 * c + 1]) + RC[r][2] * P.R[3 * c + 2]; };
    const double s00 = cb[0] + rcr(0, 0), s01 = cb[1] + rcr(0, 1), s02 = cb[2] + rcr(0, 2);
    const double s11 = cb[3] + rcr(1, 1), s12 = cb[4] + rcr(1, 2), s22 = cb[5] + rcr(2, 2);
    // M = S^-1, closed form (S is symmetric positive definite with eigenvalues between 2 plane_epsilon and 2), as k_vgicp_linearize's
    const double c00 = s11 * s22 - s12 * s12, c01 = s02 * s12 - s01 * s22, c02 = s01 * s12 - s02 * s11;
    const double det = (s00 * c00 + s01 * c01) + s02 * c02;
    const double id = 1.0 / det;
    o[0] = c00 * id; o[1] = c01 * id; o[2] = c02 * id;
    o[3] = (s00 * s22 - s02 * s02) * id; o[4] = (s01 * s02 - s00 * s12) * id; o[5] = (s00 * s11 - s01 * s01) * id;
}

// One source point per lane: its pair at P and the pair's M.  pair = sorted position of the correspondent or -1; m6 = the 6 doubles of M
// (written for pairs only); d2 (may be null) = the squared distance, NaN without a pair.
__device__ __forceinline__ void fg_pairs_lane(const float4 s, const double* __restrict__ ca, const FgTarget& A, const FgPose& P, double max_d,
                                              double max2, int* __restrict__ pair, double* __restrict__ m6, double* __restrict__ d2)
{
    double qx, qy, qz;
    fg_transform(P, s, qx, qy, qz);
    double bd;
    int    bj;
    fg_search_lane(A, qx, qy, qz, max_d, max2, bd, bj);
    const bool hit = bj >= 0 && bd < max2;                          // strict
    *pair = hit ? bj : -1;
    if (d2) *d2 = hit ? bd : (double)NAN;
    if (!hit) return;
    fg_pair_matrix_lane(A, P, bj, ca, m6);
}

// The 28 terms of one lane's pair at P (zeros without one: j < 0) and its 1.0 or 0.0 for the pair count: x' and d are recomputed, the
// pair and its M are read.  The wavefront's sums of them are left in acc[28] and pairs on every lane.
template <bool HESS>
__device__ __forceinline__ void fg_sums_lane(int j, const float4* __restrict__ src_i, const double* __restrict__ m, const float4* __restrict__ tgt_sorted,
                                             const FgPose& P, double acc[28], double& pairs)
{
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = 0.0;
    pairs = 0.0;
    if (j >= 0) {
        double x0, x1, x2;
        fg_transform(P, *src_i, x0, x1, x2);
        const float4 b = tgt_sorted[j];
        const double d[3] = { (double)b.x - x0, (double)b.y - x1, (double)b.z - x2 };
        const double M[3][3] = { { m[0], m[1], m[2] }, { m[1], m[3], m[4] }, { m[2], m[4], m[5] } };
        double Md[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) Md[r] = (M[r][0] * d[0] + M[r][1] * d[1]) + M[r][2] * d[2];
        // J = [skew(x) | -I], column by column
        const double J[6][3] = { { 0.0, x2, -x1 }, { -x2, 0.0, x0 }, { x1, -x0, 0.0 }, { -1.0, 0.0, 0.0 }, { 0.0, -1.0, 0.0 }, { 0.0, 0.0, -1.0 } };
        pairs = 1.0;
        acc[0] = (d[0] * Md[0] + d[1] * Md[1]) + d[2] * Md[2];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[1 + a] = (J[a][0] * Md[0] + J[a][1] * Md[1]) + J[a][2] * Md[2];
        if (HESS) {
            double MJ[6][3];
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int r = 0; r < 3; ++r) MJ[a][r] = (M[r][0] * J[a][0] + M[r][1] * J[a][1]) + M[r][2] * J[a][2];
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int c = a; c < 6; ++c)
                    acc[7 + a * 6 - a * (a - 1) / 2 + (c - a)] = (J[a][0] * MJ[c][0] + J[a][1] * MJ[c][1]) + J[a][2] * MJ[c][2];
        }
    }
#pragma unroll
    for (int k = 0; k < 28; ++k) acc[k] = wave_sum(acc[k]);
    pairs = wave_sum(pairs);
}

// ---- lisreg_fgicp.hip: the host checks of every FastGICP entry point (one copy) --------------------------------------------------------
int fg_check_params(lisreg_ctx* c, const lisreg_fgicp_params* P, const char* who);
int fg_find_target(lisreg_ctx* c, int slot, const char* who, FgicpTarget** out);
// the kernels' view of a slot's target
FgTarget fg_target_view(const FgicpTarget& G);

}  // namespace lisreg
