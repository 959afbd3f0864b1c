// lisreg_batch_rounds.hpp — what the rounds of the batch verifiers share on the device (lisreg_fgicp_batch.hip, DESIGN.md §7m,
// lisreg_vgicp_batch.hip, §7n, lisreg_ndt_batch.hip, §7o, and lisreg_gicp_batch.hip, §7r): how a workgroup finds its entry in the round's
// work table, the fixed-order totals of an entry's partial records (of the family's width), and the fitness search.  One source for the units; the anonymous namespace gives each unit a kernel of its own in
// its own code object.  The host side of the rounds is lisreg_batch_driver.hpp.  Not installed.
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

// One wavefront per entry: its partial records of W doubles added by the single call's sum_records (lisreg_fp64_sums.hpp: lane l takes
// records l, l + 64, ... one after the other, then the butterfly from 32 down to 1)
template <int W>
__global__ __launch_bounds__(64) void k_fgicp_total_batch(const double* __restrict__ part, const int* __restrict__ wg_start, double* __restrict__ out)
{
    const int e = blockIdx.x;
    const int p0 = wg_start[e], n_part = wg_start[e + 1] - p0;
    double acc[W];
    sum_records<W>(part + (size_t)p0 * W, n_part, acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < W; ++k) out[(size_t)e * W + k] = acc[k];
}

// One item at its final pose, for the fitness pass of either family: the search grid of its target (the search reads the points and the
// cells only: cov may be null)
struct FgFitWork {
    FgTarget  A;
    FgPose    P;
    long long src_off;     // the source's first finite point in the batch's point buffer
    int       n;           // finite points of the source
    int       reserved;
};

// The fitness pass: the nearest finite target point of every finite source point at the item's final pose, without a cut-off; the
// wavefront's sum of the squared distances goes to the workgroup's partial.
__global__ __launch_bounds__(64) void k_fgicp_fitness_batch(const FgFitWork* __restrict__ work, const int* __restrict__ wg_start, int n_entries,
                                                            const float4* __restrict__ src, double* __restrict__ part)
{
    const int g = blockIdx.x;
    const int e = fg_entry_of(wg_start, 0, n_entries, g);
    const FgFitWork* __restrict__ w = work + e;
    const int n = w->n;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    double d2 = 0.0;
    if (i < n) {
        const FgTarget A = w->A;
        const FgPose   P = w->P;
        double qx, qy, qz, bd;
        int    bj;
        fg_transform(P, src[(size_t)w->src_off + (size_t)i], qx, qy, qz);
        fg_search_lane(A, qx, qy, qz, HUGE_VAL, HUGE_VAL, bd, bj);
        d2 = bj >= 0 ? bd : 0.0;
    }
    d2 = wave_sum(d2);
    if (threadIdx.x == 0) part[g] = d2;
}

}  // namespace
}  // namespace lisreg
