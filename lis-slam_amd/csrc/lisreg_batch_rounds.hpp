// lisreg_batch_rounds.hpp — what the rounds of the two batch verifiers share on the device (lisreg_fgicp_batch.hip, DESIGN.md §7m, and
// lisreg_vgicp_batch.hip, §7n): how a workgroup finds its entry in the round's work table, and the fixed-order totals of an entry's
// partial records.  One source for both units; the anonymous namespace gives each unit a kernel of its own in its own code object.
// Not installed.
#pragma once
#include "lisreg_fgicp_lane.hpp"

namespace lisreg {
namespace {

// the entry of workgroup g: the last e in [lo, hi) with wg_start[e] <= g.  g comes from blockIdx alone: the walk is scalar
__device__ __forceinline__ int fg_entry_of(const int* __restrict__ wg_start, int lo, int hi, int g)
{
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (wg_start[mid] <= g) lo = mid; else hi = mid;
    }
    return __builtin_amdgcn_readfirstlane(lo);
}

// One wavefront per entry: its partial records of W doubles added in k_vgicp_total's order (lane l takes records l, l + 64, ... one
// after the other, then the butterfly from 32 down to 1)
template <int W>
__global__ __launch_bounds__(64) void k_fgicp_total_batch(const double* __restrict__ part, const int* __restrict__ wg_start, double* __restrict__ out)
{
    const int e = blockIdx.x;
    const int p0 = wg_start[e], n_part = wg_start[e + 1] - p0;
    double acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.0;
    for (int b = (int)threadIdx.x; b < n_part; b += 64)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += part[(size_t)(p0 + b) * W + k];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = fg_wave_sum(acc[k]);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < W; ++k) out[(size_t)e * W + k] = acc[k];
}

}  // namespace
}  // namespace lisreg
