// lisreg_ndt_voxel_lane.hpp — the Gaussian of one NDT target voxel: the mean of its finite points, the inverse of
// their inflated covariance, fp64, the record, the flag, the cell id, the dense table's entry and the two counts.  Shared by the single
// call's kernels (NdtBuild::voxel, lisreg_ndt.hip) and the batched target build (NtBuild::voxel, lisreg_ndt_target_batch.hip).  Both
// units are built with -ffp-contract=off and inline this body, so a voxel gets the same sums in the same order from either: sequential
// in sorted order by one lane, or lanes j, j + 64, ... and the wave_sum butterfly by a wavefront.  Not installed.
#pragma once
#include "lisreg_fp64_sums.hpp"
#include "lisreg_jacobi3.hpp"

namespace lisreg {

// the Gaussian of one voxel from its mean-centred second moments S (already divided by n - 1): eigen-decomposition, the two smaller
// eigenvalues raised to mult * the largest, inverse = V diag(1 / lambda) V^T.  False: not a valid voxel.
__device__ inline bool ndt_gaussian(double a00, double a01, double a02, double a11, double a12, double a22, double mult, double ic[6])
{
    double v00, v01, v02, v10, v11, v12, v20, v21, v22;
    jacobi3(a00, a01, a02, a11, a12, a22, v00, v01, v02, v10, v11, v12, v20, v21, v22);
    const double lmax = fmax(a00, fmax(a11, a22));
    if (a00 < 0.0 || a11 < 0.0 || a22 < 0.0 || !(lmax > 0.0)) return false;
    const double fl = mult * lmax;
    const double i0 = 1.0 / fmax(a00, fl), i1 = 1.0 / fmax(a11, fl), i2 = 1.0 / fmax(a22, fl);
    ic[0] = (i0 * v00 * v00 + i1 * v01 * v01) + i2 * v02 * v02;
    ic[1] = (i0 * v00 * v10 + i1 * v01 * v11) + i2 * v02 * v12;
    ic[2] = (i0 * v00 * v20 + i1 * v01 * v21) + i2 * v02 * v22;
    ic[3] = (i0 * v10 * v10 + i1 * v11 * v11) + i2 * v12 * v12;
    ic[4] = (i0 * v10 * v20 + i1 * v11 * v21) + i2 * v12 * v22;
    ic[5] = (i0 * v20 * v20 + i1 * v21 * v21) + i2 * v22 * v22;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) fin = fin && isfinite(ic[k]);
    return fin;
}

// Which records of a voxel's run belong to no voxel.  The single call sorts a cleaned copy of the cloud (k_ndt_clean: a record with a
// NaN coordinate sits on the box's minimum corner, marked in .w); the batch sorts the caller's records where they lie and a NaN record
// carries the key of that corner's cell.  Either way the record is in cell 0's run, counts towards the run's length and is left out
// of every sum.
struct NdtSkipMarked { static __device__ __forceinline__ bool skip(const float4 p) { return p.w != 0.0f; } };
struct NdtSkipNaN    { static __device__ __forceinline__ bool skip(const float4 p) { return p.x != p.x || p.y != p.y || p.z != p.z; } };

// *p += 1 for every lane that calls with `flag` set, by integer atomics.  The lanes of a wavefront that name the first active lane's
// counter send ONE atomic with their number; a lane that names another counter (a wavefront of the batch that lies across two targets)
// sends its own.  Thousands of voxels count into the two words of one target: an atomic per voxel makes the statistics kernel wait
// for the one memory channel that holds them (3.0 ms of 4.0 ms for 16 targets of 200 000 points, profiles/ndt_target_batch.md).
__device__ __forceinline__ void ndt_count(int* p, bool flag)
{
    const unsigned long long a = (unsigned long long)p;
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(a >> 32));
    const bool same = a == (((unsigned long long)hi << 32) | lo);
    const unsigned long long together = __ballot(flag && same);
    if (flag && !same) atomicAdd(p, 1);
    else if (flag && (int)__lane_id() == __ffsll((long long)together) - 1) atomicAdd(p, __popcll(together));
}

// The voxel whose records are order[a .. b) (indices into `pts`), sidx[a] its cell id, v its number within its target.  rec: the
// voxel's record of kVoxelRec doubles; vflag_out: became a Gaussian; cell_out: its cell id; table[cell id] = v for a valid voxel;
// counters[0] += 1 for a voxel with a finite point, counters[1] += 1 for a valid one (ndt_count: integer atomics, their order and
// grouping cannot change a sum of ones).  WAVE: the 64 lanes of a wavefront share the voxel (every lane ends up with the same sums:
// the butterfly adds the same pairs everywhere)
template <bool WAVE, class Skip>
__device__ __forceinline__ void ndt_voxel_lane(const float4* __restrict__ pts, const int* __restrict__ order, const uint32_t* __restrict__ sidx,
                                               int a, int b, int lane, int v, long long n_cells, int min_pts, double mult,
                                               double* __restrict__ rec_out, int* __restrict__ vflag_out, int* __restrict__ cell_out,
                                               int* __restrict__ table, int* __restrict__ counters)
{
    const int step = WAVE ? 64 : 1;
    double s0 = 0, s1 = 0, s2 = 0, cnt = 0;
    for (int k = a + lane; k < b; k += step) {
        const float4 p = pts[order[k]];
        if (Skip::skip(p)) continue;
        s0 += (double)p.x; s1 += (double)p.y; s2 += (double)p.z; cnt += 1.0;
    }
    if (WAVE) { s0 = wave_sum(s0); s1 = wave_sum(s1); s2 = wave_sum(s2); cnt = wave_sum(cnt); }
    const int n = (int)cnt;
    const uint32_t cid = sidx[a];
    double rec[kVoxelRec];
#pragma unroll
    for (int k = 0; k < kVoxelRec; ++k) rec[k] = 0.0;
    rec[9] = cnt;
    bool ok = n >= min_pts && n >= 2;
    if (ok) {                                                  // uniform across the wavefront: no lane leaves the shuffles below alone
        const double m0 = s0 / cnt, m1 = s1 / cnt, m2 = s2 / cnt;
        double c00 = 0, c01 = 0, c02 = 0, c11 = 0, c12 = 0, c22 = 0;
        for (int k = a + lane; k < b; k += step) {
            const float4 p = pts[order[k]];
            if (Skip::skip(p)) continue;
            const double d0 = (double)p.x - m0, d1 = (double)p.y - m1, d2 = (double)p.z - m2;
            c00 += d0 * d0; c01 += d0 * d1; c02 += d0 * d2; c11 += d1 * d1; c12 += d1 * d2; c22 += d2 * d2;
        }
        if (WAVE) { c00 = wave_sum(c00); c01 = wave_sum(c01); c02 = wave_sum(c02); c11 = wave_sum(c11); c12 = wave_sum(c12); c22 = wave_sum(c22); }
        const double inv = 1.0 / (cnt - 1.0);
        double ic[6];
        ok = ndt_gaussian(c00 * inv, c01 * inv, c02 * inv, c11 * inv, c12 * inv, c22 * inv, mult, ic);
        rec[0] = m0; rec[1] = m1; rec[2] = m2;
#pragma unroll
        for (int k = 0; k < 6; ++k) rec[3 + k] = ok ? ic[k] : 0.0;
    }
    if (lane != 0) return;
#pragma unroll
    for (int k = 0; k < kVoxelRec; ++k) rec_out[k] = rec[k];
    *vflag_out = ok ? 1 : 0;
    *cell_out = (int)cid;
    ndt_count(&counters[0], n > 0);
    ndt_count(&counters[1], ok);
    if (ok && (long long)cid < n_cells) table[cid] = v;
}

}  // namespace lisreg
