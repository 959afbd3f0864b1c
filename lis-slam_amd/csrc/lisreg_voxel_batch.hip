// lisreg_voxel_batch.hip — lisreg_voxel_downsample_batch: pcl::VoxelGrid of up to LISREG_VOXEL_BATCH_MAX device clouds (the corner and
// surface clouds of a sweep batch, currentCloudInit, odomEstimationNode.cpp:260-281; the class clouds of key frames,
// subMapOptmizationNode.cpp:806-821) in ONE launch sequence whose length does not depend on the number of clouds, with one host
// synchronisation.  DESIGN.md §7g-8.
//
// What differs from the multi form (lisreg_api_cloud.hip, at most 8 clouds):
//  - per-cloud state lives in device tables (VbCloud uploaded, VbState made on the device), not in kernel arguments; a point finds its
//    cloud through the chunk table (every workgroup of a per-point kernel is one chunk of one cloud), a voxel by a binary search;
//  - the grid geometry is made on the device from the device bounding boxes (voxel_geometry, lisreg_voxel_shared.hpp: the function the
//    single call runs on the host), together with each cloud's status and bucket span: no round trip;
//  - there is no joint voxel index: the sort key is (cloud, the cloud's own 32-bit index) — every cloud owns a range of buckets, so the
//    sorted sequence is cloud by cloud, cloud s at sorted positions [off, off + n), and a head is where the index changes or a cloud begins;
//  - the clouds are read where they lie (no concatenation) and every voxel is written straight into its cloud's `out` once the device has
//    checked that the cloud's voxels fit;
//  - the kernels over voxels read the voxel count from device memory and stride; voxels of more than kVoteBig points go into a list that
//    a fixed grid of wavefronts loops over.
// The per-voxel arithmetic is the single call's (voxel_centroid_thread / voxel_centroid_wave), so a cloud of a batch gets its bits.
#include "lisreg_ctx.hpp"
#include "lisreg_voxel_shared.hpp"
#include "lisreg_voxel_batch_plan.hpp"

#include <cstring>

using namespace lisreg;

namespace {

static_assert(kVbVoteBig == kVoteBig, "the plan sizes the list of big voxels by kVoteBig");
static_assert(kVbRecordBytes == sizeof(float4), "device records are 16 bytes");

// What the device makes of one cloud
struct VbState {
    VoxelDesc d;               // geometry + bucket span (k_vb_geometry)
    int       gstat;           // 0: gridded; 1: the index would overflow int32 (the input is copied); 2: a non-finite bounding box
    int       vox_base;        // first voxel of the cloud in the batch-wide numbering (k_vb_finish)
    int       mode;            // 0: nothing is written; 1: centroids; 2: copy of the input
    int       pad_[2];
};
static_assert(sizeof(VbState) == kVbStateBytes, "lisreg_voxel_batch_plan.hpp sizes the table");
static_assert(sizeof(VbCloud) == 48 && sizeof(VbChunk) == 16, "table layout");

enum { kGridded = 0, kOverflow = 1, kNonFinite = 2 };

// bounding box of every chunk: part[chunk][6] = min xyz, max xyz
__global__ __launch_bounds__(kVbChunk) void k_vb_bbox(const VbCloud* __restrict__ clouds, const VbChunk* __restrict__ chunks,
                                                      float* __restrict__ part)
{
    __shared__ float s[4][6];
    const VbChunk ch = chunks[blockIdx.x];
    const float4* pts = static_cast<const float4*>(clouds[ch.cloud].in) + ch.start;
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    if ((int)threadIdx.x < ch.count) {
        const float4 p = pts[threadIdx.x];
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], d));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d));
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) for (int k = 0; k < 3; ++k) { s[wave][k] = lo[k]; s[wave][3 + k] = hi[k]; }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) v = threadIdx.x < 3 ? fminf(v, s[w][threadIdx.x]) : fmaxf(v, s[w][threadIdx.x]);
        part[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
}

// One wavefront per cloud: the cloud's box from its chunks' boxes, then what the single call decides on the host between its first and
// second round trip — the status of the box, pcl::VoxelGrid's geometry, the bucket span
__global__ __launch_bounds__(64) void k_vb_geometry(const VbCloud* __restrict__ clouds, const float* __restrict__ part, VbState* __restrict__ state)
{
    const VbCloud c = clouds[blockIdx.x];
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    for (int b = threadIdx.x; b < c.n_chunks; b += 64) {
        const float* r = part + (size_t)(c.chunk0 + b) * 6;
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], r[k]); hi[k] = fmaxf(hi[k], r[3 + k]); }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d)); }
    if (threadIdx.x != 0) return;
    VbState st;
    memset(&st, 0, sizeof st);
    st.d.span = 1u;
    if (c.n > 0) {
        const float bb[6] = { lo[0], lo[1], lo[2], hi[0], hi[1], hi[2] };
        bool finite = true;
        for (int k = 0; k < 6; ++k) finite = finite && isfinite(bb[k]);
        long long total = 0;
        if (!finite) st.gstat = kNonFinite;
        else if (!voxel_geometry(bb, c.leaf, &st.d, &total)) st.gstat = kOverflow;
        // a cloud that is not gridded is still part of the sort (the launches are sized before this is known): its key is the point's
        // own index, spread evenly over the cloud's buckets, so it costs a pass and every point is a "voxel" of its own
        if (st.gstat != kGridded) total = c.n;
        const long long nb = c.n_buckets > 0 ? c.n_buckets : 1;
        const long long span = (total + nb - 1) / nb;
        st.d.span = (uint32_t)(span < 1 ? 1 : span > 0xffffffffLL ? 0xffffffffLL : span);      // (k_vb_keys divides by it)
    }
    state[blockIdx.x] = st;
}

// sort keys: bucket = the cloud's first bucket + index / span, sub-key = the cloud's own 32-bit voxel index; and the point's arrival rank
// in its bucket, drawn from the histogram's atomic counter here so that the scatter needs no atomic of its own (which rank a point draws
// is irrelevant: the rank pass fixes the order inside a bucket).  Consecutive points of a sweep fall into the same bucket dozens at a
// time, and a million atomics on a few thousand hot addresses were half of the call: every run of equal buckets among neighbouring
// lanes sends ONE atomic, for the run's length, and hands its members consecutive ranks.
__global__ __launch_bounds__(kVbChunk) void k_vb_keys(const VbCloud* __restrict__ clouds, const VbChunk* __restrict__ chunks,
                                                      const VbState* __restrict__ state, uint32_t* __restrict__ elem_bucket,
                                                      uint32_t* __restrict__ elem_sub, int* __restrict__ elem_rank, int* __restrict__ hist)
{
    const VbChunk ch = chunks[blockIdx.x];
    const VbCloud c = clouds[ch.cloud];
    const int lane = threadIdx.x & 63;
    const bool valid = (int)threadIdx.x < ch.count;
    const int e = ch.start + (int)threadIdx.x;
    uint32_t b = 0xffffffffu - (uint32_t)lane, idx = 0u;        // a lane without a point: a bucket no other lane names
    if (valid) {
        const VbState& st = state[ch.cloud];
        const VoxelDesc d = st.d;
        idx = st.gstat == kGridded ? voxel_index(static_cast<const float4*>(c.in)[e], d) : (uint32_t)e;
        // (an index outside the cloud's range can only come from a NaN coordinate: its bucket is clamped into the cloud's own)
        uint32_t lb = idx / d.span;
        if (lb >= (uint32_t)c.n_buckets) lb = (uint32_t)c.n_buckets - 1u;
        b = (uint32_t)c.bucket_base + lb;
    }
    const uint32_t left = (uint32_t)__shfl_up((int)b, 1);
    const bool first = lane == 0 || left != b;                  // first lane of a run of equal buckets
    const unsigned long long firsts = __ballot(first);
    const int start = 63 - __clzll((long long)(firsts & ((2ull << lane) - 1ull)));          // my run's first lane
    const unsigned long long above = lane == 63 ? 0ull : firsts >> (lane + 1);
    const int behind = above ? __ffsll((long long)above) - 1 : 63 - lane;                   // lanes of my run behind me
    int base = 0;
    if (first && valid) base = atomicAdd(&hist[b], 1 + behind);
    base = __shfl(base, start);
    if (!valid) return;
    elem_bucket[c.off + e] = b;
    elem_sub[c.off + e] = idx;
    elem_rank[c.off + e] = base + (lane - start);
}

// scatter into the buckets at the rank drawn by k_vb_keys (arbitrary order inside a bucket); the element's index WITHIN its cloud
// travels along
__global__ __launch_bounds__(kVbChunk) void k_vb_scatter(const VbCloud* __restrict__ clouds, const VbChunk* __restrict__ chunks,
                                                         const uint32_t* __restrict__ elem_bucket, const uint32_t* __restrict__ elem_sub,
                                                         const int* __restrict__ elem_rank, const int* __restrict__ bucket_start,
                                                         uint32_t* __restrict__ tmp_bucket, uint32_t* __restrict__ tmp_sub, int* __restrict__ tmp_idx)
{
    const VbChunk ch = chunks[blockIdx.x];
    if ((int)threadIdx.x >= ch.count) return;
    const int e = ch.start + (int)threadIdx.x, i = clouds[ch.cloud].off + e;
    const uint32_t b = elem_bucket[i];
    const int pos = bucket_start[b] + elem_rank[i];
    tmp_bucket[pos] = b;
    tmp_sub[pos] = elem_sub[i];
    tmp_idx[pos] = e;
}

// final position inside the bucket: rank by (voxel index, input index) — a bucket holds points of one cloud only, so the sorted
// sequence is, cloud by cloud, "ascending voxel index, ties by input index": PCL's output order with the summation order fixed
__global__ __launch_bounds__(256) void k_vb_rank(int n, const uint32_t* __restrict__ tmp_bucket, const uint32_t* __restrict__ tmp_sub,
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

// a voxel begins where a cloud begins or the cloud's index changes (two consecutive clouds may both end and begin at index 0)
__global__ __launch_bounds__(kVbChunk) void k_vb_heads(const VbCloud* __restrict__ clouds, const VbChunk* __restrict__ chunks,
                                                       const uint32_t* __restrict__ sidx, int* __restrict__ head)
{
    const VbChunk ch = chunks[blockIdx.x];
    if ((int)threadIdx.x >= ch.count) return;
    const int e = ch.start + (int)threadIdx.x, p = clouds[ch.cloud].off + e;
    head[p] = (e == 0 || sidx[p] != sidx[p - 1]) ? 1 : 0;
}

// One thread per cloud, after the scan of the heads (slot[p] = voxels in front of sorted position p, slot[n_points] = all of them):
// the cloud's voxel count, and with it what the single call decides after its second round trip; the result table
__global__ __launch_bounds__(256) void k_vb_finish(int n_clouds, int n_points, const VbCloud* __restrict__ clouds, VbState* __restrict__ state,
                                                   const int* __restrict__ slot, int* __restrict__ vstart, int2* __restrict__ result)
{
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s == 0) vstart[slot[n_points]] = n_points;
    if (s >= n_clouds) return;
    const VbCloud c = clouds[s];
    const int gstat = state[s].gstat;
    const int base = slot[c.off], nv = slot[c.off + c.n] - base;
    int mode = 0, n_out = 0, status = LISREG_OK;
    if (c.n == 0) { }
    else if (gstat == kNonFinite) status = LISREG_ERR_ARG;
    else if (gstat == kOverflow) {                                  // "Leaf size is too small for the input dataset": output = input
        n_out = c.n;
        if (c.n > c.cap) status = LISREG_ERR_ARG; else { status = LISREG_LEAF_TOO_SMALL; mode = 2; }
    } else {
        n_out = nv;
        if (nv > c.cap) status = LISREG_ERR_ARG; else mode = 1;
    }
    state[s].vox_base = base;
    state[s].mode = mode;
    result[s] = make_int2(n_out, status);
}

__global__ __launch_bounds__(kVbChunk) void k_vb_starts(const VbCloud* __restrict__ clouds, const VbChunk* __restrict__ chunks,
                                                        const int* __restrict__ head, const int* __restrict__ slot, int* __restrict__ vstart)
{
    const VbChunk ch = chunks[blockIdx.x];
    if ((int)threadIdx.x >= ch.count) return;
    const int p = clouds[ch.cloud].off + ch.start + (int)threadIdx.x;
    if (head[p]) vstart[slot[p]] = p;
}

// the cloud of voxel v: the last one whose first voxel is not behind v (clouds without voxels in front of it share its base and lose)
__device__ __forceinline__ int vb_cloud_of_voxel(const VbState* __restrict__ state, int n_clouds, int v)
{
    int lo = 0, hi = n_clouds - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (state[mid].vox_base <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// One thread per voxel, striding over the voxel count the device holds (slot[n_points]): the centroid of a voxel of at most kVoteBig
// points straight into its cloud's `out`; bigger ones into the list of k_vb_big; the records of a cloud that is copied
__global__ __launch_bounds__(256) void k_vb_centroids(int n_clouds, int n_points, const VbCloud* __restrict__ clouds,
                                                      const VbState* __restrict__ state, int w_mode, const int* __restrict__ order,
                                                      const int* __restrict__ slot, const int* __restrict__ vstart,
                                                      int* __restrict__ big_count, int2* __restrict__ big_list)
{
    const int n_vox = slot[n_points];
    for (int v = blockIdx.x * 256 + threadIdx.x; v < n_vox; v += gridDim.x * 256) {
        const int s = vb_cloud_of_voxel(state, n_clouds, v);
        const int mode = state[s].mode;
        if (mode == 0) continue;
        const VbCloud c = clouds[s];
        const float4* pts = static_cast<const float4*>(c.in);
        float4* out = static_cast<float4*>(c.out) + (v - state[s].vox_base);
        const int a = vstart[v], b = vstart[v + 1];
        if (mode == 2) { *out = pts[order[a]]; continue; }
        if (b - a > kVoteBig) { big_list[atomicAdd(big_count, 1)] = make_int2(v, s); continue; }
        uint32_t best;
        *out = voxel_centroid_thread(a, b, pts, nullptr, w_mode, order, &best);
    }
}

// a fixed grid of wavefronts loops over the list of big voxels (in whatever order the list came to be: every voxel has its own output)
__global__ __launch_bounds__(64) void k_vb_big(const VbCloud* __restrict__ clouds, const VbState* __restrict__ state, int w_mode,
                                               const int* __restrict__ order, const int* __restrict__ vstart,
                                               const int* __restrict__ big_count, const int2* __restrict__ big_list)
{
    __shared__ float4 s_q[64];
    const int n_big = *big_count;
    for (int i = blockIdx.x; i < n_big; i += gridDim.x) {
        const int2 vs = big_list[i];
        const VbCloud c = clouds[vs.y];
        uint32_t best;
        const float4 o = voxel_centroid_wave(vstart[vs.x], vstart[vs.x + 1], (int)threadIdx.x, s_q, static_cast<const float4*>(c.in), nullptr,
                                             w_mode, order, &best);
        if (threadIdx.x == 0) static_cast<float4*>(c.out)[vs.x - state[vs.y].vox_base] = o;
        __builtin_amdgcn_wave_barrier();                       // s_q is the next voxel's too
    }
}

}  // namespace

extern "C" int lisreg_voxel_downsample_batch(lisreg_ctx* c, int n_clouds, lisreg_voxel_job* jobs, int fmt)
{
    if (!c) return LISREG_ERR_ARG;
    std::string why;
    if (!vb_validate(n_clouds, jobs, fmt, &why)) return bad(c, why);
    VbPlan P;
    vb_plan(n_clouds, jobs, &P);
    for (int s = 0; s < n_clouds; ++s) { jobs[s].n_out = 0; jobs[s].status = LISREG_OK; }
    if (P.n_points == 0) return LISREG_OK;                     // nothing but empty clouds
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int N = P.n_points, B = P.n_buckets, K = n_clouds, C = (int)P.chunks.size();
    const VbSizes z = vb_sizes(P);
    // ---- scratch: the sort's and the single call's buffers, the tables --------------------------------------------------------------
    HIPCHK(c, c->hist.ensure(z.hist));
    HIPCHK(c, c->bucket_start.ensure(z.bucket_start));
    HIPCHK(c, c->scan_tmp.ensure(z.scan_tmp));
    HIPCHK(c, c->elem_bucket.ensure(z.per_point));
    HIPCHK(c, c->elem_sub.ensure(z.per_point));
    HIPCHK(c, c->tmp_bucket.ensure(z.per_point));
    HIPCHK(c, c->tmp_sub.ensure(z.per_point));
    HIPCHK(c, c->tmp_idx.ensure(z.per_point));
    HIPCHK(c, c->vox_order.ensure(z.per_point));
    HIPCHK(c, c->vox_sidx.ensure(z.per_point));
    HIPCHK(c, c->vox_head.ensure(z.head));
    HIPCHK(c, c->vox_slot.ensure(z.slot));
    HIPCHK(c, c->vox_start.ensure(z.vstart));
    HIPCHK(c, c->vb_part.ensure(z.part));
    HIPCHK(c, c->vb_big.ensure(z.big));
    HIPCHK(c, c->vb_tab.ensure(z.tab_upload + z.tab_state + z.tab_result));
    const size_t host_bytes = z.tab_upload + z.tab_result;
    HIPCHK(c, c->vb_host.ensure(host_bytes, host_bytes + host_bytes / 2 + 4096));
    char* h = c->vb_host.as<char>();
    memcpy(h, P.clouds.data(), sizeof(VbCloud) * (size_t)K);
    memcpy(h + sizeof(VbCloud) * (size_t)K, P.chunks.data(), sizeof(VbChunk) * (size_t)C);
    char* t = c->vb_tab.as<char>();
    const VbCloud* clouds = reinterpret_cast<const VbCloud*>(t);
    const VbChunk* chunks = reinterpret_cast<const VbChunk*>(t + sizeof(VbCloud) * (size_t)K);
    VbState* state = reinterpret_cast<VbState*>(t + z.tab_upload);
    int2* result = reinterpret_cast<int2*>(t + z.tab_upload + z.tab_state);
    int* big_count = c->vb_big.as<int>();
    int2* big_list = reinterpret_cast<int2*>(c->vb_big.as<char>() + 16);
    int *hist = c->hist.as<int>(), *bucket_start = c->bucket_start.as<int>(), *scan_tmp = c->scan_tmp.as<int>();
    uint32_t *elem_bucket = c->elem_bucket.as<uint32_t>(), *elem_sub = c->elem_sub.as<uint32_t>();
    uint32_t *tmp_bucket = c->tmp_bucket.as<uint32_t>(), *tmp_sub = c->tmp_sub.as<uint32_t>(), *sidx = c->vox_sidx.as<uint32_t>();
    int *tmp_idx = c->tmp_idx.as<int>(), *order = c->vox_order.as<int>(), *head = c->vox_head.as<int>(), *slot = c->vox_slot.as<int>(),
        *vstart = c->vox_start.as<int>();
    const int w_mode = fmt == LISREG_FMT_DEVICE ? 1 : 0;       // label vote on the payload, else .w averaged
    // ---- one launch sequence, whatever n_clouds ------------------------------------------------------------------------------------------
    HIPCHK(c, hipMemcpyAsync(t, h, z.tab_upload, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(hist, 0, sizeof(int) * (size_t)B, st));          // the extent this call uses
    HIPCHK(c, hipMemsetAsync(big_count, 0, 16, st));
    k_vb_bbox<<<C, kVbChunk, 0, st>>>(clouds, chunks, c->vb_part.as<float>());
    k_vb_geometry<<<K, 64, 0, st>>>(clouds, c->vb_part.as<float>(), state);
    k_vb_keys<<<C, kVbChunk, 0, st>>>(clouds, chunks, state, elem_bucket, elem_sub, head /* the ranks, until the heads are made */, hist);
    launch_exclusive_scan(hist, bucket_start, scan_tmp, B, st);
    k_vb_scatter<<<C, kVbChunk, 0, st>>>(clouds, chunks, elem_bucket, elem_sub, head, bucket_start, tmp_bucket, tmp_sub, tmp_idx);
    k_vb_rank<<<(N + 255) / 256, 256, 0, st>>>(N, tmp_bucket, tmp_sub, tmp_idx, bucket_start, order, sidx);
    k_vb_heads<<<C, kVbChunk, 0, st>>>(clouds, chunks, sidx, head);
    launch_exclusive_scan(head, slot, scan_tmp, N, st);
    k_vb_finish<<<(K + 255) / 256, 256, 0, st>>>(K, N, clouds, state, slot, vstart, result);
    k_vb_starts<<<C, kVbChunk, 0, st>>>(clouds, chunks, head, slot, vstart);
    k_vb_centroids<<<vb_voxel_blocks(N), 256, 0, st>>>(K, N, clouds, state, w_mode, order, slot, vstart, big_count, big_list);
    k_vb_big<<<vb_big_blocks(N), 64, 0, st>>>(clouds, state, w_mode, order, vstart, big_count, big_list);
    HIPCHK(c, hipGetLastError());
    // ---- the one round trip: n_out and status of every cloud; the outputs are complete with it ----------------------------------------------
    int* hr = reinterpret_cast<int*>(h + z.tab_upload);
    HIPCHK(c, hipMemcpyAsync(hr, result, z.tab_result, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int s = 0; s < K; ++s) { jobs[s].n_out = hr[2 * s]; jobs[s].status = hr[2 * s + 1]; }
    return LISREG_OK;
}
