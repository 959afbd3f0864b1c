// lisreg_voxel_shared.hpp — what the three forms of the voxel grid (lisreg_voxel_downsample, _multi, _batch) have in common, one copy each:
// pcl::VoxelGrid's geometry from a bounding box (host and device: the batch form makes it on the device) and the per-voxel arithmetic
// of the centroid kernels (device).  A cloud of a batch gets the bits of the single call because both run these functions.
#pragma once
#include "lisreg_internal.hpp"

#include <math.h>

namespace lisreg {

// pcl::VoxelGrid's min_b_ and div_b_ (voxel_grid.hpp) of the box `bb` at the inverse leaf size `inv`
__host__ __device__ inline void voxel_bounds(const float bb[6], float inv, int min_b[3], long long div_b[3])
{
    for (int k = 0; k < 3; ++k) {
        min_b[k] = (int)floorf(bb[k] * inv);
        div_b[k] = (long long)floorf(bb[3 + k] * inv) - min_b[k] + 1;
    }
}

// pcl::VoxelGrid's geometry (voxel_grid.hpp) of a cloud with bounding box `bb`: the voxel index of a point and the number of voxels the
// box spans.  d->span is left to the sort (it follows from how many buckets it may use).  false: "Leaf size is too small for the
// input dataset" — the index would overflow int32.  Every voxel entry point takes its geometry from here: that is what makes the multi
// and the batch form's results those of K single calls.  (No product feeds a sum here, so contraction settings cannot change a bit.)
__host__ __device__ inline bool voxel_geometry(const float bb[6], float leaf, VoxelDesc* d, long long* total)
{
    const float inv = 1.0f / leaf;
    const long long dx = (long long)((bb[3] - bb[0]) * inv) + 1, dy = (long long)((bb[4] - bb[1]) * inv) + 1,
                    dz = (long long)((bb[5] - bb[2]) * inv) + 1;
    if (dx * dy * dz > 2147483647LL) return false;
    int min_b[3];
    long long div_b[3];
    voxel_bounds(bb, inv, min_b, div_b);
    d->inv_leaf = inv; d->min_b0 = min_b[0]; d->min_b1 = min_b[1]; d->min_b2 = min_b[2];
    d->mul1 = (int)div_b[0]; d->mul2 = (int)(div_b[0] * div_b[1]);
    *total = div_b[0] * div_b[1] * div_b[2];
    return true;
}

#if defined(__HIPCC__)

// PCL's voxel index of a point: ijk = static_cast<int>(floor(p * inverse_leaf) - static_cast<float>(min_b)), idx = ijk . divb_mul
__device__ __forceinline__ uint32_t voxel_index(const float4 p, const VoxelDesc& d)
{
    const int i0 = (int)(floorf(p.x * d.inv_leaf) - (float)d.min_b0);
    const int i1 = (int)(floorf(p.y * d.inv_leaf) - (float)d.min_b1);
    const int i2 = (int)(floorf(p.z * d.inv_leaf) - (float)d.min_b2);
    return (uint32_t)(i0 + i1 * d.mul1 + i2 * d.mul2);
}

constexpr int kVoteBig = 24;            // voxels with more points are summed and voted by one wavefront each (voxel_centroid_wave)

// CentroidPoint (common/impl/accumulators.hpp) of the voxel whose points are order[a .. b), b - a <= kVoteBig, by ONE thread: xyz and
// intensity = sequential float sums / n, label = most frequent (smallest on ties).  The loads of four points are in flight together, the
// sums stay strictly in input order (that order is part of the result).
// w_mode 0: .w is an intensity (averaged), labels (if any) in `labels`; w_mode 1: .w is a lisreg_dpoint payload whose
// low 16 bits are the label (majority-voted into the output payload).
__device__ __forceinline__ float4 voxel_centroid_thread(int a, int b, const float4* __restrict__ pts, const uint32_t* __restrict__ labels,
                                                        int w_mode, const int* __restrict__ order, uint32_t* best_out)
{
    const bool vote = w_mode == 1 || labels;
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    // AccumulatorLabel through up to 8 distinct (label, count) slots held in registers (compile-time indices); a voxel with more
    // distinct labels than that falls back to the quadratic count below
    uint32_t sl[8]; int sc[8]; int ns = 0; bool overflow = false;
#pragma unroll
    for (int s = 0; s < 8; ++s) { sl[s] = 0xffffffffu; sc[s] = 0; }
#define LISREG_VOX_ADD(q_, e_) do { \
        sx += (q_).x; sy += (q_).y; sz += (q_).z; \
        if (w_mode == 0) sw += (q_).w; \
        if (vote && !overflow) { \
            const uint32_t lp_ = (w_mode == 1 ? __float_as_uint((q_).w) : labels[e_]) & 0xffffu; \
            bool hit_ = false; \
            _Pragma("unroll") for (int s = 0; s < 8; ++s) if (sl[s] == lp_) { ++sc[s]; hit_ = true; } \
            if (!hit_) { \
                if (ns < 8) { _Pragma("unroll") for (int s = 0; s < 8; ++s) if (s == ns) { sl[s] = lp_; sc[s] = 1; } ++ns; } \
                else overflow = true; \
            } \
        } } while (0)
    int p = a;
    for (; p + 4 <= b; p += 4) {
        const int e0 = order[p], e1 = order[p + 1], e2 = order[p + 2], e3 = order[p + 3];
        const float4 q0 = pts[e0], q1 = pts[e1], q2 = pts[e2], q3 = pts[e3];
        LISREG_VOX_ADD(q0, e0); LISREG_VOX_ADD(q1, e1); LISREG_VOX_ADD(q2, e2); LISREG_VOX_ADD(q3, e3);
    }
    for (; p < b; ++p) { const int e = order[p]; const float4 q = pts[e]; LISREG_VOX_ADD(q, e); }
#undef LISREG_VOX_ADD
    const float cnt = (float)(b - a);
    uint32_t best = 0u;
    if (vote) {
        int bestc = 0;
        if (!overflow) {
#pragma unroll
            for (int s = 0; s < 8; ++s)
                if (sc[s] > bestc || (sc[s] == bestc && sc[s] > 0 && sl[s] < best)) { bestc = sc[s]; best = sl[s]; }
        } else {
            for (int p2 = a; p2 < b; ++p2) {
                const int e = order[p2];
                const uint32_t lp = (w_mode == 1 ? __float_as_uint(pts[e].w) : labels[e]) & 0xffffu;
                int c = 0;
                for (int m = a; m < b; ++m) {
                    const int em = order[m];
                    c += (((w_mode == 1 ? __float_as_uint(pts[em].w) : labels[em]) & 0xffffu) == lp) ? 1 : 0;
                }
                if (c > bestc || (c == bestc && lp < best)) { bestc = c; best = lp; }
            }
        }
    }
    *best_out = best;
    return make_float4(sx / cnt, sy / cnt, sz / cnt, w_mode == 1 ? __uint_as_float(best) : sw / cnt);
}

// The same voxel by ONE WAVEFRONT (more than kVoteBig points: the cells next to the sensor hold hundreds to thousands, and one lane
// walking through them — a dependent gather per point — was most of a grid's time).  Centroid: the lanes fetch 64 points at a time into
// s_q (LDS, 64 records) and lane 0 adds them up in input order, so the float sums are the serial ones bit for bit.  Label: one pass per
// DISTINCT label in ascending order; every pass counts the current label and finds the next larger one (lanes stride over the points,
// wave reductions), so the most frequent label — the smallest among equals, as the serial vote keeps it — falls out without any table.
// The result is lane 0's; *best_out is every lane's.
__device__ __forceinline__ float4 voxel_centroid_wave(int a, int b, int lane, float4* s_q, const float4* __restrict__ pts,
                                                      const uint32_t* __restrict__ labels, int w_mode, const int* __restrict__ order,
                                                      uint32_t* best_out)
{
    const bool vote = w_mode == 1 || labels;
    float sx = 0.f, sy = 0.f, sz = 0.f, sw = 0.f;
    unsigned cur = 0xffffffffu;
    for (int p0 = a; p0 < b; p0 += 64) {
        const int p = p0 + lane;
        if (p < b) {
            const int e = order[p];
            const float4 q = pts[e];
            s_q[lane] = q;
            if (vote) cur = min(cur, (w_mode == 1 ? __float_as_uint(q.w) : labels[e]) & 0xffffu);
        }
        __builtin_amdgcn_wave_barrier();                       // one wavefront: its LDS operations execute in order
        if (lane == 0) {
            const int m = min(64, b - p0);
            for (int i = 0; i < m; ++i) {
                const float4 q = s_q[i];
                sx += q.x; sy += q.y; sz += q.z;
                if (w_mode == 0) sw += q.w;
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    unsigned best = 0u;
    if (vote) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) cur = min(cur, (unsigned)__shfl_xor((int)cur, d));
        int bestc = 0;
        while (cur != 0xffffffffu) {
            int c = 0; unsigned nxt = 0xffffffffu;
            for (int p = a + lane; p < b; p += 64) {
                const int e = order[p];
                const unsigned lp = (w_mode == 1 ? __float_as_uint(pts[e].w) : labels[e]) & 0xffffu;
                c += lp == cur ? 1 : 0;
                if (lp > cur) nxt = min(nxt, lp);
            }
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) { c += __shfl_xor(c, d); nxt = min(nxt, (unsigned)__shfl_xor((int)nxt, d)); }
            if (c > bestc) { bestc = c; best = cur; }              // ascending labels: a later equal count does not replace
            cur = nxt;
        }
    }
    *best_out = best;
    const float cnt = (float)(b - a);
    return make_float4(sx / cnt, sy / cnt, sz / cnt, w_mode == 1 ? __uint_as_float(best) : sw / cnt);
}

#endif  // __HIPCC__

}  // namespace lisreg
