// lisreg_voxel_batch_plan.hpp — the decisions of lisreg_voxel_downsample_batch that need no device (lisreg_voxel_batch.hip): argument
// validation, the overlap test, the clouds' offsets, the chunk table, the bucket budget, the launch sizes and the scratch sizes.  Plain
// C++: no HIP header, no HIP call.  Everything here is a function of n_clouds, the jobs' n / leaf / pointers / capacities and the
// constants below — never of a count the device makes — so the call sizes its allocations and launches before the first kernel runs.
// host/voxel_batch_plan_check.cpp compares these functions with brute-force restatements on random batches.
#pragma once
#include "../../include/lisreg.h"

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace lisreg {

constexpr int       kVbChunk           = 256;          // points of one chunk: every chunk belongs to one cloud (the BlockDesc pattern)
constexpr int       kVbRecordBytes     = 16;           // sizeof(lisreg_dpoint)
constexpr long long kVbMaxPoints       = 2000000000LL;
// The bucket budget.  A cloud of n points asks for kVbBucketsPerPoint * n sort buckets (at least kVbMinBuckets); if the batch asks for
// more than kVbBucketCap in all, every cloud's share shrinks in proportion (at least one bucket).  The device divides each cloud's voxel
// index space by its share to get the cloud's span (indices per bucket).  The rank pass is quadratic inside a bucket, so the share per
// POINT is what matters, and that does not shrink with n_clouds until the cap binds (2 M points); the histogram the cap allows
// (64 MiB) is zeroed and scanned at HBM speed in well under the time one more host round trip would cost.
constexpr long long kVbBucketsPerPoint = 8;
constexpr long long kVbMinBuckets      = 64;
constexpr long long kVbBucketCap       = 1LL << 24;
constexpr int       kVbVoteBig         = 24;           // = kVoteBig (lisreg_voxel_shared.hpp; the unit asserts it)
constexpr int       kVbMaxVoxelBlocks  = 4096;         // workgroups of the kernels that stride over a device-side voxel count
constexpr int       kVbMaxBigBlocks    = 2048;         // wavefronts that loop over the list of big voxels

// One cloud of the batch as the kernels read it (uploaded; 48 bytes)
struct VbCloud {
    const void* in;            // n records
    void*       out;           // cap records
    int         off;           // first point in the batch-wide numbering (the sorted sequence is cloud by cloud: also its first sorted position)
    int         n;
    float       leaf;
    int         cap;
    int         bucket_base;   // first sort bucket
    int         n_buckets;     // its share of the budget (0: an empty cloud)
    int         chunk0;        // first chunk
    int         n_chunks;
};
// One workgroup of the kernels that run over input points
struct VbChunk {
    int cloud;
    int start;                 // first point of the chunk, relative to the cloud
    int count;                 // <= kVbChunk
    int pad_;
};

struct VbPlan {
    std::vector<VbCloud> clouds;
    std::vector<VbChunk> chunks;
    int n_points  = 0;
    int n_buckets = 0;
};

// do the byte ranges [a, a + na) and [b, b + nb) meet?  (an empty range meets nothing)
inline bool vb_ranges_meet(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return na != 0 && nb != 0 && a < b + nb && b < a + na; }

// The overlap rule: no job's `out` range (out_capacity records) may meet any job's `in` range (n records; its own included: the batch
// form does no in-place grids) or another job's `out` range.  Inputs may meet each other.  One sort and one sweep (1024 jobs would be
// a million pairs otherwise, per call).  false: *job names a job whose `out` is in conflict.
inline bool vb_check_overlap(int n_clouds, const lisreg_voxel_job* jobs, int* job)
{
    struct Range { uintptr_t lo, hi; int job; int is_out; };
    std::vector<Range> r;
    r.reserve(2 * (size_t)n_clouds);
    for (int s = 0; s < n_clouds; ++s) {
        const lisreg_voxel_job& j = jobs[s];
        if (j.n > 0 && j.in) r.push_back({ (uintptr_t)j.in, (uintptr_t)j.in + (size_t)j.n * kVbRecordBytes, s, 0 });
        if (j.out_capacity > 0 && j.out) r.push_back({ (uintptr_t)j.out, (uintptr_t)j.out + (size_t)j.out_capacity * kVbRecordBytes, s, 1 });
    }
    std::sort(r.begin(), r.end(), [](const Range& a, const Range& b) { return a.lo != b.lo ? a.lo < b.lo : a.job < b.job; });
    // the furthest end among the ranges in front (all start at or before this one's start), of any kind and of the outputs alone
    uintptr_t end_any = 0, end_out = 0;
    int job_out = -1;
    for (const Range& x : r) {
        if (x.is_out && end_any > x.lo) { *job = x.job; return false; }
        if (!x.is_out && end_out > x.lo) { *job = job_out; return false; }
        end_any = std::max(end_any, x.hi);
        if (x.is_out && x.hi > end_out) { end_out = x.hi; job_out = x.job; }
    }
    return true;
}

// The argument checks of the entry point, in the order it names them.  true: the batch may run.  false: *why is the text for
// lisreg_last_error (it names the job where there is one).
inline bool vb_validate(int n_clouds, const lisreg_voxel_job* jobs, int fmt, std::string* why)
{
    const std::string who = "voxel_downsample_batch: ";
    if (n_clouds < 0 || n_clouds > LISREG_VOXEL_BATCH_MAX) { *why = who + "n_clouds outside 0 .. " + std::to_string(LISREG_VOXEL_BATCH_MAX); return false; }
    if (fmt != LISREG_FMT_DEVICE && fmt != LISREG_FMT_DEVICE_XYZI) { *why = who + "device records only (LISREG_FMT_DEVICE / _DEVICE_XYZI)"; return false; }
    if (n_clouds > 0 && !jobs) { *why = who + "jobs is NULL"; return false; }
    long long total = 0;
    for (int s = 0; s < n_clouds; ++s) {
        const lisreg_voxel_job& j = jobs[s];
        const std::string at = who + "job " + std::to_string(s) + ": ";
        if (j.n < 0) { *why = at + "n < 0"; return false; }
        if (!(j.leaf > 0.f)) { *why = at + "the leaf is not > 0"; return false; }
        if (j.out_capacity < 0) { *why = at + "out_capacity < 0"; return false; }
        if (j.n > 0 && (!j.in || !j.out)) { *why = at + "NULL cloud with n > 0"; return false; }
        if (j.out_capacity > 0 && !j.out) { *why = at + "NULL out with out_capacity > 0"; return false; }
        total += j.n;
    }
    if (total > kVbMaxPoints) { *why = who + "more than 2e9 points in all"; return false; }
    int job = -1;
    if (!vb_check_overlap(n_clouds, jobs, &job)) {
        *why = who + "job " + std::to_string(job) + ": its out range overlaps an in range or another job's out range (no in-place grids here)";
        return false;
    }
    return true;
}

// offsets, chunk table and bucket shares of a validated batch
inline void vb_plan(int n_clouds, const lisreg_voxel_job* jobs, VbPlan* P)
{
    P->clouds.assign((size_t)n_clouds, VbCloud{});
    P->chunks.clear();
    long long want_all = 0;
    for (int s = 0; s < n_clouds; ++s)
        if (jobs[s].n > 0) want_all += std::max(kVbMinBuckets, kVbBucketsPerPoint * (long long)jobs[s].n);
    long long off = 0, nb = 0;
    for (int s = 0; s < n_clouds; ++s) {
        const lisreg_voxel_job& j = jobs[s];
        VbCloud& c = P->clouds[(size_t)s];
        c.in = j.in; c.out = j.out; c.off = (int)off; c.n = j.n; c.leaf = j.leaf; c.cap = j.out_capacity;
        long long share = 0;
        if (j.n > 0) {
            share = std::max(kVbMinBuckets, kVbBucketsPerPoint * (long long)j.n);
            if (want_all > kVbBucketCap) share = std::max(1LL, share * kVbBucketCap / want_all);      // (< 2^58: 1.6e10 * 2^24)
        }
        c.bucket_base = (int)nb; c.n_buckets = (int)share;
        c.chunk0 = (int)P->chunks.size(); c.n_chunks = (j.n + kVbChunk - 1) / kVbChunk;
        for (int b = 0; b < c.n_chunks; ++b) P->chunks.push_back({ s, b * kVbChunk, std::min(kVbChunk, j.n - b * kVbChunk), 0 });
        off += j.n; nb += share;
    }
    P->n_points = (int)off;
    P->n_buckets = (int)nb;
}

// launch sizes of the two kernels that stride over counts only the device knows (voxels of the batch; voxels of more than kVbVoteBig
// points): upper bounds of those counts from the point count, capped
inline int vb_voxel_blocks(int n_points) { return std::max(1, std::min(kVbMaxVoxelBlocks, (n_points + 255) / 256)); }
inline int vb_big_capacity(int n_points) { return n_points / (kVbVoteBig + 1) + 1; }              // entries of the list
inline int vb_big_blocks(int n_points) { return std::max(1, std::min(kVbMaxBigBlocks, vb_big_capacity(n_points))); }

// bytes of the context's scratch a call uses
struct VbSizes {
    size_t hist, bucket_start, scan_tmp, per_point /* elem_bucket, elem_sub, tmp_bucket, tmp_sub, tmp_idx, order, sidx */, head, slot, vstart,
           part, big, tab_upload, tab_state, tab_result;
};
constexpr size_t kVbStateBytes = 48;      // sizeof(VbState) (lisreg_voxel_batch.hip asserts it)
inline VbSizes vb_sizes(const VbPlan& P)
{
    const size_t N = (size_t)P.n_points, B = (size_t)P.n_buckets, K = P.clouds.size(), C = P.chunks.size();
    VbSizes z;
    z.hist = 4 * (B + 1); z.bucket_start = 4 * (B + 2); z.scan_tmp = 4 * (std::max(B, N + 1) / 2048 + 4);
    z.per_point = 4 * (N + 1); z.head = 4 * (N + 1); z.slot = 4 * (N + 2); z.vstart = 4 * (N + 2);
    z.part = 4 * 6 * std::max<size_t>(C, 1);
    z.big = 16 + 8 * (size_t)vb_big_capacity(P.n_points);      // the counter (16 bytes), then (voxel, cloud) pairs
    z.tab_upload = sizeof(VbCloud) * K + sizeof(VbChunk) * C;
    z.tab_state = kVbStateBytes * K;
    z.tab_result = 2 * sizeof(int) * K;
    return z;
}

}  // namespace lisreg
