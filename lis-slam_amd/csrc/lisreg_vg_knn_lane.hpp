// lisreg_vg_knn_lane.hpp — what one lane of the distribution kernel computes: the k nearest points of one point within
// its own cloud by an exact shell walk over the cloud's search grid, then mean, covariance and the plane regularisation, fp64.  Shared by
// the single call's kernel (k_vg_knn, lisreg_vgicp.hip) and the batched target build (k_ft_knn, lisreg_fgicp_target_batch.hip, §7t).
// Both units are built with -ffp-contract=off and inline this body, so a lane of either computes the same bits from the same input.  Not
// installed.
#pragma once
#include "lisreg_jacobi3.hpp"

namespace lisreg {

struct VgKnn {
    const float4* sorted;       // [m] by grid cell, ascending index inside a cell; .w = index among the finite points
    const int*    cell_start;   // [nx * ny * nz + 1], cell = (ix * ny + iy) * nz + iz
    const float4* pts;          // [m] the finite points in input order
    const int*    orig;         // [m] -> index in the caller's cloud
    int    m, k;
    float  ox, oy, oz, cell, inv_cell;
    int    nx, ny, nz;
    double plane_eps;
    double* cov;                // [m][6] upper triangle of C_i, by index among the finite points
    int*    nbr;                // [n][k] by the CALLER's index, ascending (distance, index); may be null
};

__device__ __forceinline__ int vg_cell(float v, float origin, float inv_cell, int n)
{
    int c = (int)floorf((v - origin) * inv_cell);                  // the arithmetic of the index build (cell_coord)
    return c < 0 ? 0 : (c >= n ? n - 1 : c);
}

// The query at sorted position s < A.m.  The KT best (distance, index) pairs live in registers: the list is only ever touched through
// fully unrolled loops, so no entry is addressed dynamically.  Shells of cells are walked outward from the query's cell — shell r is the
// surface of the (2 r + 1)^3 block, clipped to the grid; the z runs of a column are contiguous in the sorted array — until the k-th best
// distance is no larger than the distance from the query to the nearest face of the visited block that still has cells behind it.  That
// distance is reduced by 1e-3 cell: a point's cell comes from float arithmetic ((x - origin) * inv_cell, relative error about 1e-7 of
// at most 2048 cells per axis), so a point of an unvisited cell can lie that little inside the face.  The result therefore does not
// depend on the cell edge: it is the k smallest (distance, index) pairs of the whole cloud.
template <int KT>
__device__ __forceinline__ void vg_knn_lane(const VgKnn& A, int s)
{
    const float4 q = A.sorted[s];
    const int self = __float_as_int(q.w);
    const double qx = (double)q.x, qy = (double)q.y, qz = (double)q.z;
    const int cx = vg_cell(q.x, A.ox, A.inv_cell, A.nx), cy = vg_cell(q.y, A.oy, A.inv_cell, A.ny), cz = vg_cell(q.z, A.oz, A.inv_cell, A.nz);
    double bd[KT];
    int    bi[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) { bd[j] = HUGE_VAL; bi[j] = 0x7fffffff; }
    double wd = HUGE_VAL;                                           // the k-th best so far
    int    wi = 0x7fffffff;
    const int k = A.k;
    const double cell = (double)A.cell, slack = 1.0e-3 * (double)A.cell;

    auto scan = [&](int a, int b) {
        for (int j = a; j < b; ++j) {
            const float4 p = A.sorted[j];
            const double dx = (double)p.x - qx, dy = (double)p.y - qy, dz = (double)p.z - qz;
            const double d = (dx * dx + dy * dy) + dz * dz;
            const int id = __float_as_int(p.w);
            if (!(d < wd || (d == wd && id < wi))) continue;
#pragma unroll
            for (int e = KT - 1; e >= 1; --e) {
                const bool lt_prev = d < bd[e - 1] || (d == bd[e - 1] && id < bi[e - 1]);
                const bool lt_cur  = d < bd[e] || (d == bd[e] && id < bi[e]);
                const double nd = lt_prev ? bd[e - 1] : (lt_cur ? d : bd[e]);
                const int    ni = lt_prev ? bi[e - 1] : (lt_cur ? id : bi[e]);
                bd[e] = nd; bi[e] = ni;
            }
            if (d < bd[0] || (d == bd[0] && id < bi[0])) { bd[0] = d; bi[0] = id; }
#pragma unroll
            for (int e = 0; e < KT; ++e)
                if (e == k - 1) { wd = bd[e]; wi = bi[e]; }
        }
    };

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
                    scan(A.cell_start[base + za], A.cell_start[base + zb + 1]);
                }
            }
        double lim = HUGE_VAL;                                      // distance to the nearest face with unvisited cells behind it
        if (cx - r > 0)        lim = fmin(lim, qx - ((double)A.ox + (double)(cx - r) * cell));
        if (cx + r < A.nx - 1) lim = fmin(lim, ((double)A.ox + (double)(cx + r + 1) * cell) - qx);
        if (cy - r > 0)        lim = fmin(lim, qy - ((double)A.oy + (double)(cy - r) * cell));
        if (cy + r < A.ny - 1) lim = fmin(lim, ((double)A.oy + (double)(cy + r + 1) * cell) - qy);
        if (cz - r > 0)        lim = fmin(lim, qz - ((double)A.oz + (double)(cz - r) * cell));
        if (cz + r < A.nz - 1) lim = fmin(lim, ((double)A.oz + (double)(cz + r + 1) * cell) - qz);
        if (lim == HUGE_VAL) break;                                 // the whole grid has been visited
        lim -= slack;
        if (lim > 0.0 && wd <= lim * lim) break;
    }

    // the k points again: two passes, in the list's order
    if (A.nbr) {
        int* row = A.nbr + (size_t)A.orig[self] * (size_t)k;
#pragma unroll
        for (int e = 0; e < KT; ++e)
            if (e < k) row[e] = A.orig[bi[e]];
    }
    double m0 = 0, m1 = 0, m2 = 0;
#pragma unroll
    for (int e = 0; e < KT; ++e)
        if (e < k) { const float4 p = A.pts[bi[e]]; m0 += (double)p.x; m1 += (double)p.y; m2 += (double)p.z; }
    const double kk = (double)k;
    m0 /= kk; m1 /= kk; m2 /= kk;
    double a00 = 0, a01 = 0, a02 = 0, a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
    for (int e = 0; e < KT; ++e)
        if (e < k) {
            const float4 p = A.pts[bi[e]];
            const double d0 = (double)p.x - m0, d1 = (double)p.y - m1, d2 = (double)p.z - m2;
            a00 += d0 * d0; a01 += d0 * d1; a02 += d0 * d2; a11 += d1 * d1; a12 += d1 * d2; a22 += d2 * d2;
        }
    a00 /= kk; a01 /= kk; a02 /= kk; a11 /= kk; a12 /= kk; a22 /= kk;
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
    jacobi3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    // the eigenvector of the smallest eigenvalue (the first of equal ones: any unit vector of a degenerate neighbourhood will do)
    const bool s1 = a11 < a00;
    const double l01 = s1 ? a11 : a00;
    const bool s2 = a22 < l01;
    double n0 = s2 ? v02 : (s1 ? v01 : v00), n1 = s2 ? v12 : (s1 ? v11 : v10), n2 = s2 ? v22 : (s1 ? v21 : v20);
    const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    n0 /= nn; n1 /= nn; n2 /= nn;
    const double f = 1.0 - A.plane_eps;
    double* o = A.cov + (size_t)self * 6;
    o[0] = 1.0 - f * n0 * n0; o[1] = -f * n0 * n1; o[2] = -f * n0 * n2;
    o[3] = 1.0 - f * n1 * n1; o[4] = -f * n1 * n2; o[5] = 1.0 - f * n2 * n2;
}

}  // namespace lisreg
