// lisreg_semantic_batch.hip — lisreg_semantic_split_batch: categoryMapping (semanticFusionNode.cpp:173-189) for the labelled clouds of
// up to LISREG_SEMANTIC_BATCH_MAX key frames in THREE launches, whatever the number of frames, behind one table upload and with one
// read-back and one host synchronisation; and lisreg_concat_device_batch, the other per-frame step of the semantic chain, as one launch.
// DESIGN.md §7g-9.
//
// What differs from the single call (lisreg_features.hip, k_sem_flags / scan / k_sem_write / k_sem_gather): no [5][n] flag array, no
// scan over 5 n ints and no index lists.  The host cuts every frame into tiles of kSbTile points (lisreg_semantic_batch_plan.hpp) and
//   1. k_sb_count    a workgroup per tile: the tile's five class counts, from 64-bit ballots, the four wavefronts combined through LDS;
//   2. k_sb_offsets  a workgroup per frame: its tiles' counts, in tile order, become exclusive bases (a block scan with five carried
//                    sums, 256 tiles a round); the frame's five totals, its status against cap[] / cloud[], its result record;
//   3. k_sb_scatter  a workgroup per tile of a frame that passed: a lane's place in its class is the tile's base + the counts of the
//                    (round, wavefront) groups in front of it in the tile + the lanes of its class below it in its ballot; the record
//                    goes straight to out.cloud[k][place] as one 16-byte store.
// The order of a class is the input order by construction (ballots and sums in a fixed order; no atomic anywhere), no workgroup waits
// for another (the launch boundary orders the passes), and every loop runs to a count the host put into the tables.
// Two 16-byte reads and one 16-byte write per point, plus 16 + 32 bytes of tables per tile.
#include "lisreg_ctx.hpp"
#include "lisreg_semantic_batch_plan.hpp"

#include <cstring>

using namespace lisreg;

namespace {

static_assert(kSbRecordBytes == sizeof(float4), "device records are 16 bytes");
static_assert(sizeof(SbFrame) == 80 && sizeof(SbTile) == 16 && sizeof(CbJob) == 112, "table layout");
static_assert(kSbThreads == 256 && kSbTile == kSbThreads * kSbRounds, "four wavefronts, kSbRounds records a lane");
static_assert(kSbPartInts >= 5 && kSbResultInts >= 6, "five counts a tile; five counts and a status a frame");
static_assert(sizeof(lisreg_semantic_job) == 104 && sizeof(lisreg_semantic_out) == 80, "the ABI the header states");

constexpr int kWaves = kSbThreads / 64;

__device__ __forceinline__ int sb_class(const SbClassMap& m, uint32_t payload)
{
    const uint32_t l = payload & 31u;
    return (int)(((l & 16u ? m.nib[1] : m.nib[0]) >> (4u * (l & 15u))) & 7u);
}

// The records of a tile a lane owns, here and in k_sb_scatter: round r, wavefront w, lane l -> point r * 256 + w * 64 + l of the tile;
// class -1 past the tile's end, so that all 64 lanes stay in every ballot
__global__ __launch_bounds__(kSbThreads) void k_sb_count(const SbFrame* __restrict__ frames, const SbTile* __restrict__ tiles, SbClassMap map,
                                                         int* __restrict__ part)
{
    __shared__ int s_cnt[kWaves][5];
    const SbTile t = tiles[blockIdx.x];
    const float4* pts = static_cast<const float4*>(frames[t.frame].in) + t.start;
    int cls[kSbRounds];
#pragma unroll
    for (int r = 0; r < kSbRounds; ++r) {
        const int i = r * kSbThreads + (int)threadIdx.x;
        cls[r] = i < t.count ? sb_class(map, __float_as_uint(pts[i].w)) : -1;
    }
    int cnt[5] = { 0, 0, 0, 0, 0 };
#pragma unroll
    for (int r = 0; r < kSbRounds; ++r)
#pragma unroll
        for (int k = 0; k < 5; ++k) cnt[k] += __popcll(__ballot(cls[r] == k));
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k) s_cnt[w][k] = cnt[k];
    __syncthreads();
    if (threadIdx.x < 5) {
        int sum = 0;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) sum += s_cnt[q][threadIdx.x];
        part[(size_t)blockIdx.x * kSbPartInts + threadIdx.x] = sum;
    }
}

// One workgroup per frame.  part[tile][0..5): counts in, exclusive bases out (a thread reads and writes its own tile only).
__global__ __launch_bounds__(256) void k_sb_offsets(const SbFrame* __restrict__ frames, int* __restrict__ part, int* __restrict__ result)
{
    __shared__ int s_wave[kWaves][5];
    const SbFrame f = frames[blockIdx.x];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int carry[5] = { 0, 0, 0, 0, 0 };
    for (int b0 = 0; b0 < f.n_tiles; b0 += 256) {                  // n_tiles: the host's
        const int b = b0 + (int)threadIdx.x;
        int* mine = part + (size_t)(f.tile0 + b) * kSbPartInts;
        int v[5], inc[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) inc[k] = v[k] = b < f.n_tiles ? mine[k] : 0;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1)
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const int up = __shfl_up(inc[k], d, 64);
                if (lane >= d) inc[k] += up;
            }
        if (lane == 63)
#pragma unroll
            for (int k = 0; k < 5; ++k) s_wave[w][k] = inc[k];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            int front = carry[k], all = 0;
#pragma unroll
            for (int q = 0; q < kWaves; ++q) { if (q < w) front += s_wave[q][k]; all += s_wave[q][k]; }
            if (b < f.n_tiles) mine[k] = front + inc[k] - v[k];
            carry[k] += all;
        }
        __syncthreads();                                           // s_wave is the next round's too
    }
    if (threadIdx.x == 0) {
        int status = LISREG_OK;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (f.cloud[k] && carry[k] > f.cap[k]) status = LISREG_ERR_ARG;
            result[(size_t)blockIdx.x * kSbResultInts + k] = carry[k];
        }
        result[(size_t)blockIdx.x * kSbResultInts + 5] = status;
    }
}

__global__ __launch_bounds__(kSbThreads) void k_sb_scatter(const SbFrame* __restrict__ frames, const SbTile* __restrict__ tiles, SbClassMap map,
                                                           const int* __restrict__ part, const int* __restrict__ result)
{
    __shared__ int s_grp[kSbRounds][kWaves][5];                    // counts of the (round, wavefront) groups, then their exclusive bases
    const SbTile t = tiles[blockIdx.x];
    if (result[(size_t)t.frame * kSbResultInts + 5] != LISREG_OK) return;      // the whole workgroup: a frame that failed writes nothing
    const SbFrame f = frames[t.frame];
    const float4* pts = static_cast<const float4*>(f.in) + t.start;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float4 rec[kSbRounds];
    int cls[kSbRounds], below[kSbRounds];
#pragma unroll
    for (int r = 0; r < kSbRounds; ++r) {
        const int i = r * kSbThreads + (int)threadIdx.x;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < t.count) v = pts[i];
        rec[r] = v;
        cls[r] = i < t.count ? sb_class(map, __float_as_uint(v.w)) : -1;
    }
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < kSbRounds; ++r) {
        below[r] = 0;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const unsigned long long bal = __ballot(cls[r] == k);
            if (cls[r] == k) below[r] = __popcll(bal & lanes_below);
            if (lane == 0) s_grp[r][w][k] = __popcll(bal);
        }
    }
    __syncthreads();
    if (threadIdx.x < 5) {                                         // groups in (round, wavefront) order = input order
        int run = part[(size_t)blockIdx.x * kSbPartInts + threadIdx.x];
#pragma unroll
        for (int r = 0; r < kSbRounds; ++r)
#pragma unroll
            for (int q = 0; q < kWaves; ++q) { const int c = s_grp[r][q][threadIdx.x]; s_grp[r][q][threadIdx.x] = run; run += c; }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kSbRounds; ++r) {
        const int k = cls[r];
        void* o = k == 0 ? f.cloud[0] : (k == 1 ? f.cloud[1] : (k == 2 ? f.cloud[2] : (k == 3 ? f.cloud[3] : f.cloud[4])));   // (no indexed table)
        if (k >= 0 && o) static_cast<float4*>(o)[s_grp[r][w][k] + below[r]] = rec[r];
    }
}

// lisreg_concat_device_batch: a job per blockIdx.y, plain 16-byte copies
__global__ __launch_bounds__(256) void k_concat_batch(const CbJob* __restrict__ jobs)
{
    const CbJob* __restrict__ j = jobs + blockIdx.y;               // (read in place: a lane's own source is an indexed load, not a private copy)
    float4* out = static_cast<float4*>(j->out);
    const int total = j->off[8], k = j->k;
    for (int t = blockIdx.x * 256 + threadIdx.x; t < total; t += gridDim.x * 256) {
        int s = 0;
#pragma unroll
        for (int q = 1; q < 8; ++q) if (q < k && t >= j->off[q]) s = q;
        out[t] = static_cast<const float4*>(j->in[s])[t - j->off[s]];
    }
}

}  // namespace

extern "C" int lisreg_semantic_split_batch(lisreg_ctx* c, int n_frames, lisreg_semantic_job* jobs, const uint32_t* using_label)
{
    if (!c) return LISREG_ERR_ARG;
    std::string why;
    if (!sb_validate(n_frames, jobs, &why)) return bad(c, why);
    SbPlan P;
    sb_plan(n_frames, jobs, &P);
    for (int s = 0; s < n_frames; ++s) {
        for (int k = 0; k < 5; ++k) jobs[s].out.n[k] = 0;
        jobs[s].status = LISREG_OK;
    }
    if (P.n_points == 0) return LISREG_OK;                     // no frame, or nothing but empty frames
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int K = n_frames, C = (int)P.tiles.size();
    const SbSizes z = sb_sizes(P);
    const SbClassMap map = sb_class_map(using_label);
    HIPCHK(c, c->sb_tab.ensure(z.tab_upload + z.tab_part + z.tab_result));
    const size_t host_bytes = z.tab_upload + z.tab_result;
    HIPCHK(c, c->sb_host.ensure(host_bytes, host_bytes + host_bytes / 2 + 4096));
    char* h = c->sb_host.as<char>();
    memcpy(h, P.frames.data(), sizeof(SbFrame) * (size_t)K);
    memcpy(h + sizeof(SbFrame) * (size_t)K, P.tiles.data(), sizeof(SbTile) * (size_t)C);
    char* t = c->sb_tab.as<char>();
    const SbFrame* frames = reinterpret_cast<const SbFrame*>(t);
    const SbTile* tiles = reinterpret_cast<const SbTile*>(t + sizeof(SbFrame) * (size_t)K);
    int* part = reinterpret_cast<int*>(t + z.tab_upload);
    int* result = reinterpret_cast<int*>(t + z.tab_upload + z.tab_part);
    // ---- one upload, three launches, one read-back, one synchronisation ----------------------------------------------------------------
    HIPCHK(c, hipMemcpyAsync(t, h, z.tab_upload, hipMemcpyHostToDevice, st));
    k_sb_count<<<C, kSbThreads, 0, st>>>(frames, tiles, map, part);
    k_sb_offsets<<<K, 256, 0, st>>>(frames, part, result);
    k_sb_scatter<<<C, kSbThreads, 0, st>>>(frames, tiles, map, part, result);
    HIPCHK(c, hipGetLastError());
    int* hr = reinterpret_cast<int*>(h + z.tab_upload);
    HIPCHK(c, hipMemcpyAsync(hr, result, z.tab_result, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int s = 0; s < K; ++s) {
        for (int k = 0; k < 5; ++k) jobs[s].out.n[k] = hr[(size_t)s * kSbResultInts + k];
        jobs[s].status = hr[(size_t)s * kSbResultInts + 5];
    }
    return LISREG_OK;
}

extern "C" int lisreg_concat_device_batch(lisreg_ctx* c, int n_jobs, lisreg_concat_job* jobs)
{
    if (!c) return LISREG_ERR_ARG;
    std::string why;
    if (!cb_validate(n_jobs, jobs, &why)) return bad(c, why);
    std::vector<CbJob> tab;
    int max_total = 0;
    cb_plan(n_jobs, jobs, &tab, &max_total);
    for (int s = 0; s < n_jobs; ++s) jobs[s].n_out = tab[(size_t)s].off[8];
    if (max_total == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, c->cb_tab.ensure(sizeof(CbJob) * (size_t)n_jobs));
    HIPCHK(c, hipMemcpyAsync(c->cb_tab.p, tab.data(), sizeof(CbJob) * (size_t)n_jobs, hipMemcpyHostToDevice, st));
    k_concat_batch<<<dim3((unsigned)cb_blocks_x(max_total), (unsigned)n_jobs), 256, 0, st>>>(c->cb_tab.as<CbJob>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));                               // `tab` is a local
    return LISREG_OK;
}
