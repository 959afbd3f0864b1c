// lisreg_voxel_sort_batch.hpp — the voxel sort of a whole batch of targets, one copy for the two units that run
// it: lisreg_vgicp_set_target_batch (lisreg_vgicp_target_batch.hip) and lisreg_ndt_set_target_batch (lisreg_ndt_target_batch.hip).  ONE
// sort over the records of all targets, keyed by (target, the target's own pcl::VoxelGrid index): every target owns a range of buckets,
// so the sorted sequence is target by target, each "ascending cell id, ties by index" — the total order launch_voxel_sort gives the
// single call.  Then the voxels' heads, their scan, the targets' first voxels and voxel counts, the voxels' starts; and one launch
// that fills every dense table with -1.
//
// The kernels are templates over the unit's target record Tg, which says where a target's records come from and how a record's key is
// made.  Tg has: int pbase (the target's first sorted position: the targets' records end to end), int m (its records in the sort;
// 0: dropped), VoxelDesc d (geometry + bucket span), int bucket_base, n_buckets, and
//     static __device__ uint32_t key(const Tg& T, int e)     the voxel index of the target's record e (0 <= e < m)
// VGICP sorts a target's finite points (compacted by phase B), NDT the caller's records with a NaN record in cell 0.
// A workgroup of a per-record kernel is one block of one target (a host-made BlockDesc table: item = target, start, count), so it
// never spans two targets and loads its target's record as scalars; no workgroup waits for another.  Everything is in an unnamed
// namespace: each unit compiles its own kernels from this one text.  Not installed.
#pragma once
#include "lisreg_internal.hpp"
#include "lisreg_voxel_shared.hpp"

#include <algorithm>

namespace {

using namespace lisreg;

// The bucket budget of the voxel sort, as lisreg_voxel_downsample_batch's (lisreg_voxel_batch_plan.hpp): a target of m records asks
// for kVtBucketsPerPoint * m buckets (at least kVtMinBuckets, never more than its grid has cells); only if the batch asks for more than
// kVtBucketCap in all does every share shrink in proportion.  The rank pass is quadratic inside a bucket, so the share per POINT is what
// matters, and that does not shrink with n_targets until the cap binds (2 M points).
constexpr long long kVtBucketsPerPoint = 8;
constexpr long long kVtMinBuckets      = 64;
constexpr long long kVtBucketCap       = 1LL << 24;
constexpr int       kVtFillChunk       = 8192;        // table entries one workgroup of k_vt_fill sets

struct VtChunk { int* p; int count, pad_; };
static_assert(sizeof(VtChunk) == 16, "table layout");

// the buckets a target of m records over `total` cells asks for
inline long long vt_buckets_wanted(long long total, long long m) { return std::min(total, std::max(kVtMinBuckets, kVtBucketsPerPoint * m)); }
// its share once the batch's wishes are known, as the span of cell ids per bucket; *n_buckets: the buckets that span makes
inline uint32_t vt_bucket_span(long long total, long long want, long long want_all, int* n_buckets)
{
    long long share = want;
    if (want_all > kVtBucketCap) share = std::max(1LL, share * kVtBucketCap / want_all);
    const long long span = (total + share - 1) / share;
    *n_buckets = (int)((total + span - 1) / span);
    return (uint32_t)span;
}

// sort keys: bucket = the target's first bucket + index / span, sub-key = the target's own voxel index; and the record's arrival rank in its
// bucket, drawn from the histogram's counter here so that the scatter needs no atomic (k_vb_keys' scheme: a run of equal buckets among
// neighbouring lanes sends ONE integer atomic; which rank a record draws is irrelevant, the rank pass fixes the order inside a bucket)
template <class Tg>
__global__ __launch_bounds__(kBlockQ) void k_vt_keys(const BlockDesc* __restrict__ blocks, const Tg* __restrict__ tg,
                                                     uint32_t* __restrict__ elem_bucket, uint32_t* __restrict__ elem_sub,
                                                     int* __restrict__ elem_rank, int* __restrict__ hist)
{
    const BlockDesc bd = blocks[blockIdx.x];
    const Tg& T = tg[bd.item];
    const int lane = threadIdx.x & 63;
    const bool valid = (int)threadIdx.x < bd.count;
    const int e = bd.start + (int)threadIdx.x;
    uint32_t b = 0xffffffffu - (uint32_t)lane, idx = 0u;            // a lane without a record: a bucket no other lane names
    if (valid) {
        idx = Tg::key(T, e);
        uint32_t lb = idx / T.d.span;
        if (lb >= (uint32_t)T.n_buckets) lb = (uint32_t)T.n_buckets - 1u;      // (cannot happen: a finite point lies inside its box)
        b = (uint32_t)T.bucket_base + lb;
    }
    const uint32_t left = (uint32_t)__shfl_up((int)b, 1);
    const bool first = lane == 0 || left != b;                      // first lane of a run of equal buckets
    const unsigned long long firsts = __ballot(first);
    const int start = 63 - __clzll((long long)(firsts & ((2ull << lane) - 1ull)));          // my run's first lane
    const unsigned long long above = lane == 63 ? 0ull : firsts >> (lane + 1);
    const int behind = above ? __ffsll((long long)above) - 1 : 63 - lane;                   // lanes of my run behind me
    int base = 0;
    if (first && valid) base = atomicAdd(&hist[b], 1 + behind);
    base = __shfl(base, start);
    if (!valid) return;
    const int i = T.pbase + e;
    elem_bucket[i] = b;
    elem_sub[i] = idx;
    elem_rank[i] = base + (lane - start);
}

// scatter into the buckets at the rank drawn above; the record's index within its target travels along
template <class Tg>
__global__ __launch_bounds__(kBlockQ) void k_vt_scatter(const BlockDesc* __restrict__ blocks, const Tg* __restrict__ tg,
                                                        const uint32_t* __restrict__ elem_bucket, const uint32_t* __restrict__ elem_sub,
                                                        const int* __restrict__ elem_rank, const int* __restrict__ bucket_start,
                                                        uint32_t* __restrict__ tmp_bucket, uint32_t* __restrict__ tmp_sub, int* __restrict__ tmp_idx)
{
    const BlockDesc bd = blocks[blockIdx.x];
    if ((int)threadIdx.x >= bd.count) return;
    const int e = bd.start + (int)threadIdx.x, i = tg[bd.item].pbase + e;
    const uint32_t b = elem_bucket[i];
    const int pos = bucket_start[b] + elem_rank[i];
    tmp_bucket[pos] = b;
    tmp_sub[pos] = elem_sub[i];
    tmp_idx[pos] = e;
}

// final position inside the bucket: rank by (cell id, index) — a bucket holds records of one target only, so the sorted sequence is,
// target by target, "ascending cell id, ties by index within the target"
__global__ __launch_bounds__(256) void k_vt_rank(int n, const uint32_t* __restrict__ tmp_bucket, const uint32_t* __restrict__ tmp_sub,
                                                 const int* __restrict__ tmp_idx, const int* __restrict__ bucket_start,
                                                 int* __restrict__ order, uint32_t* __restrict__ sidx)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t b = tmp_bucket[p];
    const int s = bucket_start[b], e = bucket_start[b + 1];
    const uint32_t sub = tmp_sub[p];
    const int idx = tmp_idx[p];
    int rank = 0;
#pragma unroll 8
    for (int j = s; j < e; ++j) {
        const uint32_t sj = tmp_sub[j];
        const int ij = tmp_idx[j];
        rank += (sj < sub || (sj == sub && ij < idx)) ? 1 : 0;
    }
    order[s + rank] = idx;
    sidx[s + rank] = sub;
}

// a voxel begins where a target begins or the cell id changes
template <class Tg>
__global__ __launch_bounds__(kBlockQ) void k_vt_heads(const BlockDesc* __restrict__ blocks, const Tg* __restrict__ tg,
                                                      const uint32_t* __restrict__ sidx, int* __restrict__ head)
{
    const BlockDesc bd = blocks[blockIdx.x];
    if ((int)threadIdx.x >= bd.count) return;
    const int e = bd.start + (int)threadIdx.x, p = tg[bd.item].pbase + e;
    head[p] = (e == 0 || sidx[p] != sidx[p - 1]) ? 1 : 0;
}

// One thread per target (and one more), after the scan of the heads (slot[p] = voxels in front of sorted position p, slot[n_points] =
// all of them): the target's first voxel in the batch-wide numbering and its voxel count; vox_base[n_targets] = the voxels of the
// batch, which the statistics launches read; the end of the last voxel; the counter of the wavefront voxels' list back to zero
template <class Tg>
__global__ __launch_bounds__(256) void k_vt_finish(int n_targets, int n_points, const Tg* __restrict__ tg, const int* __restrict__ slot,
                                                   int* __restrict__ vox_base, int* __restrict__ n_vox, int* __restrict__ vstart,
                                                   int* __restrict__ big_count)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t == n_targets) { const int all = slot[n_points]; vox_base[t] = all; vstart[all] = n_points; *big_count = 0; }
    if (t >= n_targets) return;
    const Tg& T = tg[t];
    const int base = slot[T.pbase];
    vox_base[t] = base;
    n_vox[t] = slot[T.pbase + T.m] - base;
}

template <class Tg>
__global__ __launch_bounds__(kBlockQ) void k_vt_starts(const BlockDesc* __restrict__ blocks, const Tg* __restrict__ tg,
                                                       const int* __restrict__ head, const int* __restrict__ slot, int* __restrict__ vstart)
{
    const BlockDesc bd = blocks[blockIdx.x];
    if ((int)threadIdx.x >= bd.count) return;
    const int p = tg[bd.item].pbase + bd.start + (int)threadIdx.x;
    if (head[p]) vstart[slot[p]] = p;
}

// every dense table all -1: one workgroup per chunk of one table.  A chunk starts at a multiple of kVtFillChunk entries of an
// allocation, so its first entry is 16-byte aligned
__global__ __launch_bounds__(256) void k_vt_fill(const VtChunk* __restrict__ chunks)
{
    const VtChunk ch = chunks[blockIdx.x];
    int4* q = reinterpret_cast<int4*>(ch.p);
    const int n4 = ch.count >> 2;
    for (int i = threadIdx.x; i < n4; i += 256) q[i] = make_int4(-1, -1, -1, -1);
    const int rest = (n4 << 2) + (int)threadIdx.x;
    if (rest < ch.count) ch.p[rest] = -1;
}

// the voxel of the batch-wide number v belongs to the last target whose first voxel is not behind v (targets without voxels share the
// next one's base and lose)
__device__ __forceinline__ int vt_target_of(const int* __restrict__ vox_base, int n_targets, int v)
{
    int lo = 0, hi = n_targets - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (vox_base[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// What a call enqueues for the sort, in order: the keys, the scan of the histogram, the scatter, the rank pass, the heads, their scan,
// the finish, the starts — 8 enqueues, which the caller counts.  n: the records of all live targets; n_buckets: their buckets in all
// (sb.hist cleared over that extent by the caller).  `head` serves as the ranks until the heads are made.
template <class Tg>
inline void launch_voxel_sort_targets(const BlockDesc* blk, int nb, const Tg* d_tg, int n_targets, int n, int n_buckets, const SortBuffers& sb,
                                      int* order, uint32_t* sidx, int* head, int* slot, int* vstart, int* vox_base, int* n_vox, int* big_count,
                                      hipStream_t st)
{
    k_vt_keys<Tg><<<nb, kBlockQ, 0, st>>>(blk, d_tg, sb.elem_bucket, sb.elem_sub, head, sb.hist);
    launch_exclusive_scan(sb.hist, sb.bucket_start, sb.scan_tmp, n_buckets, st);
    k_vt_scatter<Tg><<<nb, kBlockQ, 0, st>>>(blk, d_tg, sb.elem_bucket, sb.elem_sub, head, sb.bucket_start, sb.tmp_bucket, sb.tmp_sub, sb.tmp_idx);
    k_vt_rank<<<(n + 255) / 256, 256, 0, st>>>(n, sb.tmp_bucket, sb.tmp_sub, sb.tmp_idx, sb.bucket_start, order, sidx);
    k_vt_heads<Tg><<<nb, kBlockQ, 0, st>>>(blk, d_tg, sidx, head);
    launch_exclusive_scan(head, slot, sb.scan_tmp, n, st);
    k_vt_finish<Tg><<<(n_targets + 256) / 256, 256, 0, st>>>(n_targets, n, d_tg, slot, vox_base, n_vox, vstart, big_count);
    k_vt_starts<Tg><<<nb, kBlockQ, 0, st>>>(blk, d_tg, head, slot, vstart);
}
constexpr int kVtSortEnqueues = 8;

}  // namespace
