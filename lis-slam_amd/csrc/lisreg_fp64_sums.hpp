// lisreg_fp64_sums.hpp — the fp64 reductions the NDT, VGICP and FastGICP verifiers and their batch forms share: the
// wavefront butterfly, the fixed-order total of partial records, the round trip of one total, and the launch shell of the voxel
// statistics.  Each exists once: "an item of a batch gets the bits of the single call" rests on every unit adding in THIS order.  Every
// unit that includes the header is built with -ffp-contract=off.  Not installed.
#pragma once
#include "lisreg_ctx.hpp"

#include <cstring>

namespace lisreg {

constexpr int kEvalOut = 29;           // doubles of one evaluation: the value, the gradient [6], the Hessian's upper triangle [21], pairs
constexpr int kVoxelBig = 48;          // voxels with more points get a wavefront each (k_voxel_stats_big), the others a lane

// the sum over the wavefront, on every lane: the butterfly adds the same pairs everywhere
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// acc[W] = the n_part records of W doubles added in a fixed order by one wavefront: lane l takes records l, l + 64, ... one after the
// other, then the butterfly from 32 down to 1.  The sums are left on every lane.
template <int W>
__device__ __forceinline__ void sum_records(const double* __restrict__ part, int n_part, double acc[W])
{
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = 0.0;
    for (int b = (int)threadIdx.x; b < n_part; b += 64)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += part[(size_t)b * W + k];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = wave_sum(acc[k]);
}

// One round trip of fixed-order totals: launch(part) writes nb partial records of W doubles on the context's stream (and opens its
// profiling interval, if it has one; close_mark: the interval ends behind the total), total(part, nb, out, stream) adds them with
// sum_records<W>, out = the total, waited for.  One set of buffers serves every family (an evaluation of the NDT, VGICP and FastGICP
// verifiers is W = kEvalOut, PCL's GICP takes W = 74 moments): a context is single-threaded and every round trip ends in the wait.
template <int W, class Launch, class Total>
int record_totals(lisreg_ctx* c, int nb, Launch launch, Total total, bool close_mark, double out[W])
{
    hipStream_t st = c->stream;
    HIPCHK(c, c->eval_part.ensure(sizeof(double) * W * (size_t)nb));
    HIPCHK(c, c->eval_out.ensure(sizeof(double) * W));
    HIPCHK(c, c->eval_host.ensure(sizeof(double) * W, sizeof(double) * (W > 64 ? W : 64)));
    launch(c->eval_part.as<double>());
    total(c->eval_part.as<double>(), nb, c->eval_out.as<double>(), st);
    if (close_mark) ctx_prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->eval_host.p, c->eval_out.p, sizeof(double) * W, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    memcpy(out, c->eval_host.p, sizeof(double) * W);
    return LISREG_OK;
}

// one evaluation's round trip: records of kEvalOut doubles, added by launch_eval_total
template <class Launch>
int eval_totals(lisreg_ctx* c, int nb, Launch launch, bool close_mark, double out[kEvalOut])
{
    return record_totals<kEvalOut>(c, nb, launch, launch_eval_total, close_mark, out);
}

// The statistics of the n_vox voxels of a sorted cloud: a lane per voxel up to kVoxelBig points, a wavefront per voxel above.  Build is
// the family's record (by value: n_vox, vstart[n_vox + 1] and what its body reads and writes) with the body as a static member,
// Build::voxel<WAVE>(B, v, lane); the 64 lanes of the wavefront form share voxel v.
template <class Build>
__global__ __launch_bounds__(256) void k_voxel_stats_small(Build B)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= B.n_vox) return;
    if (B.vstart[v + 1] - B.vstart[v] > kVoxelBig) return;     // k_voxel_stats_big
    Build::template voxel<false>(B, v, 0);
}

template <class Build>
__global__ __launch_bounds__(64) void k_voxel_stats_big(Build B)
{
    const int v = blockIdx.x;
    if (v >= B.n_vox) return;
    if (B.vstart[v + 1] - B.vstart[v] <= kVoxelBig) return;    // the whole wavefront leaves together
    Build::template voxel<true>(B, v, (int)threadIdx.x);
}

template <class Build>
void launch_voxel_stats(const Build& B, hipStream_t st)
{
    k_voxel_stats_small<Build><<<(B.n_vox + 255) / 256, 256, 0, st>>>(B);
    k_voxel_stats_big<Build><<<B.n_vox, 64, 0, st>>>(B);
}

// The same for the voxels of a whole batch of targets, whose number only the device knows (*B.n_vox, device memory): fixed grids that
// stride.  Build is the family's record with the same static body, Build::voxel<WAVE>(B, v, lane), which finds voxel v's target itself.
// Voxels above kVoxelBig points go into a list (an int counter, zero on entry; the list's order is irrelevant: every voxel has its own
// output) that a fixed grid of wavefronts loops over; the voxel number is made wave-uniform, so what the body loads by it is scalar.
template <class Build>
__global__ __launch_bounds__(256) void k_voxel_stats_small_dev(Build B, int* __restrict__ big_count, int* __restrict__ big_list)
{
    const int n_vox = *B.n_vox;
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n_vox; v += gridDim.x * 256) {
        if (B.vstart[v + 1] - B.vstart[v] > kVoxelBig) { big_list[atomicAdd(big_count, 1)] = v; continue; }
        Build::template voxel<false>(B, v, 0);
    }
}

template <class Build>
__global__ __launch_bounds__(64) void k_voxel_stats_big_dev(Build B, const int* __restrict__ big_count, const int* __restrict__ big_list)
{
    const int n_big = *big_count;
    for (int i = blockIdx.x; i < n_big; i += gridDim.x) {
        const int v = __builtin_amdgcn_readfirstlane(big_list[i]);
        Build::template voxel<true>(B, v, (int)threadIdx.x);
    }
}

// points: an upper bound of the voxels (every voxel holds a point); big_list has room for points / (kVoxelBig + 1) + 1 entries
constexpr int kVoxelDevMaxBlocks = 4096, kVoxelDevMaxBigBlocks = 2048;
inline int voxel_stats_big_capacity(int points) { return points / (kVoxelBig + 1) + 1; }
template <class Build>
void launch_voxel_stats_dev(const Build& B, int points, int* big_count, int* big_list, hipStream_t st)
{
    const int nb = std::max(1, std::min(kVoxelDevMaxBlocks, (points + 255) / 256));
    const int nw = std::max(1, std::min(kVoxelDevMaxBigBlocks, voxel_stats_big_capacity(points)));
    k_voxel_stats_small_dev<Build><<<nb, 256, 0, st>>>(B, big_count, big_list);
    k_voxel_stats_big_dev<Build><<<nw, 64, 0, st>>>(B, big_count, big_list);
}

}  // namespace lisreg
