// lisreg_vg_voxel_lane.hpp — the statistics of one VGICP target voxel: the mean of its points and the mean of their
// covariances, fp64, the record, the cell id and the dense table's entry.  Shared by the single call's kernels (VgBuild::voxel,
// lisreg_vgicp.hip) and the batched target build (VtBuild::voxel, lisreg_vgicp_target_batch.hip).  Both units are built with
// -ffp-contract=off and inline this body, so a voxel gets the same sums in the same order from either: sequential in input order by one
// lane, or lanes j, j + 64, ... and the wave_sum butterfly by a wavefront.  Not installed.
#pragma once
#include "lisreg_fp64_sums.hpp"

namespace lisreg {

// The voxel whose points are order[a .. b) (indices among the target's finite points `pts`, covariances `cov` [.][6]), sidx[a] its cell
// id.  rec: the voxel's record of kVoxelRec doubles; cell_out: its cell id; table[cell id] = v, the voxel's number within its target.
// WAVE: the 64 lanes of a wavefront share the voxel (every lane ends up with the same sums: the butterfly adds the same pairs everywhere)
template <bool WAVE>
__device__ __forceinline__ void vg_voxel_lane(const float4* __restrict__ pts, const double* __restrict__ cov, const int* __restrict__ order,
                                              const uint32_t* __restrict__ sidx, int a, int b, int lane, int v, long long n_cells,
                                              double* __restrict__ rec, int* __restrict__ cell_out, int* __restrict__ table)
{
    const int step = WAVE ? 64 : 1;
    double s[9];
#pragma unroll
    for (int e = 0; e < 9; ++e) s[e] = 0.0;
    for (int j = a + lane; j < b; j += step) {
        const int i = order[j];
        const float4 p = pts[i];
        const double* c = cov + (size_t)i * 6;
        s[0] += (double)p.x; s[1] += (double)p.y; s[2] += (double)p.z;
#pragma unroll
        for (int e = 0; e < 6; ++e) s[3 + e] += c[e];
    }
    if (WAVE) {
#pragma unroll
        for (int e = 0; e < 9; ++e) s[e] = wave_sum(s[e]);
    }
    if (lane != 0) return;
    const double cnt = (double)(b - a);
    const uint32_t cid = sidx[a];
#pragma unroll
    for (int e = 0; e < 9; ++e) rec[e] = s[e] / cnt;
    rec[9] = cnt;
    *cell_out = (int)cid;
    if ((long long)cid < n_cells) table[cid] = v;
}

}  // namespace lisreg
