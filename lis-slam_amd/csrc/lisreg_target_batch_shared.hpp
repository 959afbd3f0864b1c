// lisreg_target_batch_shared.hpp — phases A and B of a batched target build, one copy for the three units that
// run them: lisreg_fgicp_set_target_batch (lisreg_fgicp_target_batch.hip), lisreg_vgicp_set_target_batch
// (lisreg_vgicp_target_batch.hip) and lisreg_ndt_set_target_batch (lisreg_ndt_target_batch.hip), which leaves the distributions out.  Phase A: the finite count and the bounding box of every target, one read-back.  The host between the
// phases: every target's verdict and search grid (vg_grid_geometry, the single call's function), one table of descriptors.  Phase B: the
// finite points compacted in input order, all search grids in one bucket sort (launch_build_targets_batched) and the distributions of
// all targets in one launch (vg_knn_lane, the single kernel's body).  Where the sorted points, the cells, the indices and the
// covariances of a target go is the caller's choice (ft_add_target): a FastGICP slot keeps all four, a VGICP slot the first two.
//
// Per-target state lives in device tables: a workgroup of a per-point kernel is one tile of one target (host-made tile table) and loads
// its target's record as scalars; no workgroup waits for another, no float atomics.  Both units are built with -ffp-contract=off.
// Everything is in an unnamed namespace: each unit compiles its own kernels from this one text.  Not installed.
#pragma once
#include "lisreg_fgicp_lane.hpp"
#include "lisreg_vg_knn_lane.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace {

using namespace lisreg;

constexpr int kFtTile = 256;                         // points of one target per workgroup of the per-point kernels
// cells one sort sequence covers: 16 grids of the largest size (kVgGridMaxCells).  A batch whose grids need more is sorted in as many
// sequences (the targets in order, each sequence as many as fit); the workload's 16 targets always fit one
constexpr long long kFtMaxSortCells = 16 * kVgGridMaxCells;

struct FtJob  { const float4* cloud; int n, off, tile0, n_tiles; };      // off: the target's first record in the batch-wide numbering
struct FtTile { int job, start, count, pad_; };
struct FtStat { int m; float bb[6]; int pad_; };                          // what phase A makes of one target
struct FtDesc {                                                           // what phase B needs of one target; A.m == 0: dropped
    VgKnn   A;
    float4* pts_out;           // = A.pts
    int*    orig_out;          // = A.orig
};
static_assert(sizeof(FtJob) == 24 && sizeof(FtTile) == 16 && sizeof(FtStat) == 32, "table layout");

__device__ __forceinline__ bool ft_finite(const float4 p) { return p.x == p.x && p.y == p.y && p.z == p.z; }     // (k_vg_flag's test)

// ---- phase A -----------------------------------------------------------------------------------------------------------------------
// One tile: its number of finite points and its bounding box, each coordinate's minimum and maximum on its own as launch_bbox makes
// them (a NaN coordinate is skipped, an infinite one shows: +inf in a maximum, -inf in a minimum)
__global__ __launch_bounds__(kFtTile) void k_ft_tiles(const FtJob* __restrict__ jobs, const FtTile* __restrict__ tiles,
                                                      int* __restrict__ tile_cnt, float* __restrict__ tile_bb)
{
    __shared__ float s[4][6];
    __shared__ int s_cnt[4];
    const FtTile t = tiles[blockIdx.x];
    const float4* pts = jobs[t.job].cloud + t.start;
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    bool fin = false;
    if ((int)threadIdx.x < t.count) {
        const float4 p = pts[threadIdx.x];
        fin = ft_finite(p);
        lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
        hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
    }
    const unsigned long long mask = __ballot(fin);
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], d));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d));
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        for (int k = 0; k < 3; ++k) { s[wave][k] = lo[k]; s[wave][3 + k] = hi[k]; }
        s_cnt[wave] = __popcll(mask);
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s[0][threadIdx.x];
        for (int w = 1; w < 4; ++w) v = threadIdx.x < 3 ? fminf(v, s[w][threadIdx.x]) : fmaxf(v, s[w][threadIdx.x]);
        tile_bb[(size_t)blockIdx.x * 6 + threadIdx.x] = v;
    }
    if (threadIdx.x == 6) tile_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// One wavefront per target: its box from its tiles' boxes, the exclusive scan of its tiles' counts (tile_base: finite points of the
// target in front of the tile) and its finite count
__global__ __launch_bounds__(64) void k_ft_stats(const FtJob* __restrict__ jobs, const int* __restrict__ tile_cnt,
                                                 const float* __restrict__ tile_bb, int* __restrict__ tile_base, FtStat* __restrict__ stat)
{
    const FtJob j = jobs[blockIdx.x];
    const int lane = threadIdx.x;
    float lo[3] = { 3.0e38f, 3.0e38f, 3.0e38f }, hi[3] = { -3.0e38f, -3.0e38f, -3.0e38f };
    int running = 0;
    for (int b0 = 0; b0 < j.n_tiles; b0 += 64) {
        const int b = b0 + lane;
        const bool live = b < j.n_tiles;
        int v = 0;
        if (live) {
            v = tile_cnt[j.tile0 + b];
            const float* r = tile_bb + (size_t)(j.tile0 + b) * 6;
#pragma unroll
            for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], r[k]); hi[k] = fmaxf(hi[k], r[3 + k]); }
        }
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (live) tile_base[j.tile0 + b] = running + incl - v;
        running += __shfl(incl, 63);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) { lo[k] = fminf(lo[k], __shfl_xor(lo[k], d)); hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], d)); }
    if (lane != 0) return;
    FtStat st;
    st.m = running;
    for (int k = 0; k < 3; ++k) { st.bb[k] = lo[k]; st.bb[3 + k] = hi[k]; }
    st.pad_ = 0;
    stat[blockIdx.x] = st;
}

// ---- phase B -----------------------------------------------------------------------------------------------------------------------
// One tile: its finite points, in input order, behind those of the target's tiles in front of it; their indices in the caller's cloud
// go to the descriptor's `orig_out` (if it has one).  Tiles of a dropped target return at once.
__global__ __launch_bounds__(kFtTile) void k_ft_compact(const FtJob* __restrict__ jobs, const FtTile* __restrict__ tiles,
                                                        const FtDesc* __restrict__ descs, const int* __restrict__ tile_base)
{
    __shared__ int s_cnt[4];
    const FtTile t = tiles[blockIdx.x];
    const FtDesc& D = descs[t.job];
    if (D.A.m == 0) return;
    float4* pts_out = D.pts_out;
    int* orig_out = D.orig_out;
    const int m = D.A.m;
    const float4* pts = jobs[t.job].cloud + t.start;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    bool fin = false;
    if ((int)threadIdx.x < t.count) { p = pts[threadIdx.x]; fin = ft_finite(p); }
    const unsigned long long mask = __ballot(fin);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    if (!fin) return;
    int dst = tile_base[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) dst += s_cnt[w];
    if (dst >= m) return;                                           // (cannot happen: m is the sum of the counts this repeats)
    pts_out[dst] = p;
    if (orig_out) orig_out[dst] = t.start + (int)threadIdx.x;   // (null: a family that keeps no indices, lisreg_ndt_set_target_batch)
}

// The distributions of all targets: one query per lane, 64-lane workgroups, four of them to a 256-point block of one target (the sort's
// block table), so a workgroup never spans two targets and its target's record is wave-uniform: scalar loads
template <int KT>
__global__ __launch_bounds__(64) void k_ft_knn(const BlockDesc* __restrict__ blocks, const FtDesc* __restrict__ descs)
{
    const BlockDesc bd = blocks[blockIdx.x >> 2];
    const int e = (int)((blockIdx.x & 3u) * 64u + threadIdx.x);
    if (e >= bd.count) return;
    const VgKnn A = descs[bd.item].A;
    vg_knn_lane<KT>(A, bd.start + e);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct FtEnq { int* n; void operator()(int k = 1) const { *n += k; } };        // counts what a call enqueues

// The tables of one call.  Pinned host side: [jobs | tiles] up, [stats] down, then [descs | tsegs | blocks] up; the device table
// (c->ft_tab) has the same layout.  A context is single-threaded and both families' calls end in a wait, so they share the buffers.
struct FtBatch {
    int N = 0, n_tiles = 0, n_points = 0;
    std::vector<FtJob> hj;
    size_t o_tiles = 0, o_stat = 0, o_desc = 0, o_tseg = 0, o_blk = 0, z_stat = 0, z_desc = 0;
    char *h = nullptr, *d = nullptr;
    const FtJob* d_jobs = nullptr; const FtTile* d_tiles = nullptr; const FtDesc* d_desc = nullptr; const TargetSeg* d_tseg = nullptr;
    const BlockDesc* d_blk = nullptr;
    int* tile_base = nullptr;
    const FtStat* hs = nullptr;                                     // valid behind ft_phase_a
    FtDesc* hd = nullptr; TargetSeg* hseg = nullptr; BlockDesc* hb = nullptr;
    struct Group { int seg0, n_segs, blk0, n_blks, elems; long long cells; };
    std::vector<Group> groups;                                      // the sort sequences
    std::vector<int> seg_job;                                       // the targets that passed, in order
    int n_seg = 0, n_blk = 0;

    void add_job(const void* cloud, int n)
    {
        FtJob j;
        j.cloud = static_cast<const float4*>(cloud); j.n = n; j.off = n_points; j.tile0 = n_tiles; j.n_tiles = (n + kFtTile - 1) / kFtTile;
        n_tiles += j.n_tiles; n_points += n; ++N;
        hj.push_back(j);
    }
};

// Phase A of the jobs added to F: three enqueues and the read-back, whatever the number of targets.  Afterwards F.hs[t] holds target
// t's finite count and box, c->vg_pts has room for the finite points of all targets (target t's at F.hj[t].off).
inline int ft_phase_a(lisreg_ctx* c, const char* who, FtBatch& F, FtEnq enq, int* syncs)
{
    hipStream_t st = c->stream;
    const int N = F.N, n_tiles = F.n_tiles, n_points = F.n_points;
    const size_t z_jobs = sizeof(FtJob) * (size_t)N, z_tiles = sizeof(FtTile) * (size_t)n_tiles;
    F.z_stat = sizeof(FtStat) * (size_t)N; F.z_desc = sizeof(FtDesc) * (size_t)N;
    const size_t z_tseg = sizeof(TargetSeg) * (size_t)N;
    const size_t z_blk = sizeof(BlockDesc) * ((size_t)n_points / kBlockQ + (size_t)N);
    F.o_tiles = (z_jobs + 15) & ~(size_t)15; F.o_stat = F.o_tiles + z_tiles; F.o_desc = F.o_stat + F.z_stat; F.o_tseg = F.o_desc + F.z_desc;
    F.o_blk = F.o_tseg + z_tseg;
    const size_t z_all = F.o_blk + z_blk;
    HIPCHK(c, c->ft_host.ensure(z_all, z_all + z_all / 2 + 4096));
    HIPCHK(c, c->ft_tab.ensure(z_all));
    HIPCHK(c, c->ft_part.ensure((sizeof(int) * 2 + sizeof(float) * 6) * (size_t)n_tiles));
    HIPCHK(c, c->vg_pts.ensure(sizeof(float4) * (size_t)n_points));
    char* h = F.h = c->ft_host.as<char>();
    char* d = F.d = c->ft_tab.as<char>();
    memcpy(h, F.hj.data(), z_jobs);
    FtTile* ht = reinterpret_cast<FtTile*>(h + F.o_tiles);
    for (int t = 0, i = 0; t < N; ++t)
        for (int b = 0; b < F.hj[(size_t)t].n_tiles; ++b, ++i)
            ht[i] = FtTile{ t, b * kFtTile, std::min(kFtTile, F.hj[(size_t)t].n - b * kFtTile), 0 };
    F.d_jobs = reinterpret_cast<const FtJob*>(d);
    F.d_tiles = reinterpret_cast<const FtTile*>(d + F.o_tiles);
    FtStat* d_stat = reinterpret_cast<FtStat*>(d + F.o_stat);
    F.d_desc = reinterpret_cast<const FtDesc*>(d + F.o_desc);
    F.d_tseg = reinterpret_cast<const TargetSeg*>(d + F.o_tseg);
    F.d_blk = reinterpret_cast<const BlockDesc*>(d + F.o_blk);
    int* tile_cnt = c->ft_part.as<int>();
    F.tile_base = tile_cnt + n_tiles;
    float* tile_bb = reinterpret_cast<float*>(F.tile_base + n_tiles);
    HIPCHK(c, hipMemcpyAsync(d, h, F.o_stat, hipMemcpyHostToDevice, st)); enq();
    k_ft_tiles<<<n_tiles, kFtTile, 0, st>>>(F.d_jobs, F.d_tiles, tile_cnt, tile_bb); enq();
    k_ft_stats<<<N, 64, 0, st>>>(F.d_jobs, tile_cnt, tile_bb, F.tile_base, d_stat); enq();
    HIPCHK(c, hipGetLastError());
    F.hs = reinterpret_cast<const FtStat*>(h + F.o_stat);
    HIPCHK(c, hipMemcpyAsync(h + F.o_stat, d_stat, F.z_stat, hipMemcpyDeviceToHost, st)); enq();
    HIPCHK(c, hipStreamSynchronize(st)); ++*syncs;
    for (int t = 0; t < N; ++t)
        if (F.hs[t].m < 0 || F.hs[t].m > F.hj[(size_t)t].n)
            return ctx_fail(c, LISREG_ERR_HIP, std::string(who) + ": the compaction returned an impossible count");
    F.hd = reinterpret_cast<FtDesc*>(h + F.o_desc);
    F.hseg = reinterpret_cast<TargetSeg*>(h + F.o_tseg);
    F.hb = reinterpret_cast<BlockDesc*>(h + F.o_blk);
    memset(F.hd, 0, F.z_desc);
    return LISREG_OK;
}

// the single call's first two checks, in its order (vg_distributions, vg_search_grid); null: the target passes them
inline const char* ft_verdict(const FtStat& S, int k)
{
    for (int e = 0; e < 6; ++e) if (std::isinf(S.bb[e])) return "the cloud has infinite coordinates";
    if (S.m < k || !(S.bb[0] <= S.bb[3] && S.bb[1] <= S.bb[4] && S.bb[2] <= S.bb[5]))
        return "the cloud has fewer finite points than k_correspondences";
    return nullptr;
}

// Target t passed: its descriptor, its sort segment and its blocks.  The search grid vg goes to sorted / cells, the indices in the
// caller's cloud to orig, the covariances to cov (by index among the finite points); the finite points to c->vg_pts at the target's offset.
inline void ft_add_target(lisreg_ctx* c, FtBatch& F, int t, const VgGrid& vg, int k, double plane_eps, float4* sorted, int* cells, int* orig,
                          double* cov)
{
    const int m = F.hs[t].m, n_cells = vg.nx * vg.ny * vg.nz;
    if (F.groups.empty() || F.groups.back().cells + n_cells > kFtMaxSortCells) F.groups.push_back(FtBatch::Group{ F.n_seg, 0, F.n_blk, 0, 0, 0 });
    FtBatch::Group& g = F.groups.back();
    FtDesc& D = F.hd[t];
    D.pts_out = c->vg_pts.as<float4>() + F.hj[(size_t)t].off;
    D.orig_out = orig;
    D.A.sorted = sorted; D.A.cell_start = cells; D.A.pts = D.pts_out; D.A.orig = D.orig_out;
    D.A.m = m; D.A.k = k; D.A.ox = vg.ox; D.A.oy = vg.oy; D.A.oz = vg.oz; D.A.cell = vg.cell; D.A.inv_cell = vg.inv_cell;
    D.A.nx = vg.nx; D.A.ny = vg.ny; D.A.nz = vg.nz; D.A.plane_eps = plane_eps; D.A.cov = cov; D.A.nbr = nullptr;
    TargetSeg& ts = F.hseg[F.n_seg];
    memset(&ts, 0, sizeof ts);
    ts.raw = D.pts_out; ts.sorted_out = sorted; ts.cell_start_out = cells;
    ts.n = m; ts.n_cells = n_cells; ts.flat_base = g.elems; ts.bucket_base = (int)g.cells;
    ts.ox = vg.ox; ts.oy = vg.oy; ts.oz = vg.oz; ts.inv_cell = vg.inv_cell; ts.nx = vg.nx; ts.ny = vg.ny; ts.nz = vg.nz;
    for (int s0 = 0; s0 < m; s0 += kBlockQ) F.hb[F.n_blk++] = BlockDesc{ g.n_segs, s0, std::min(kBlockQ, m - s0), t };
    g.n_blks = F.n_blk - g.blk0;
    g.elems += m; g.cells += n_cells; ++g.n_segs; ++F.n_seg;
    F.seg_job.push_back(t);
}

// the search grid of the single call in a slot's GridIndex (vg_search_grid's)
inline void ft_grid_index(const VgGrid& vg, int m, const float4* sorted, const int* cells, GridIndex* g)
{
    memset(g, 0, sizeof *g);
    g->n = m; g->ox = vg.ox; g->oy = vg.oy; g->oz = vg.oz; g->cell = vg.cell; g->inv_cell = vg.inv_cell;
    g->nx = vg.nx; g->ny = vg.ny; g->nz = vg.nz;
    g->pts = sorted; g->cell_start = cells;
}

// Phase B of the targets added (at least one): one table up, the compaction, one sort per sequence, the distributions (k == 0: none,
// and orig / cov of ft_add_target may be null); nothing is waited for.  lisreg_get_timing: "index" opens in front of the compaction (the caller closes it)
inline int ft_phase_b(lisreg_ctx* c, FtBatch& F, int k, FtEnq enq)
{
    hipStream_t st = c->stream;
    int max_elems = 0; long long max_cells = 0;
    for (const FtBatch::Group& g : F.groups) { max_elems = std::max(max_elems, g.elems); max_cells = std::max(max_cells, g.cells); }
    const int rc = ensure_sort_scratch(c, (size_t)max_elems, (size_t)max_cells + 1);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(F.d + F.o_desc, F.h + F.o_desc, F.o_blk + sizeof(BlockDesc) * (size_t)F.n_blk - F.o_desc, hipMemcpyHostToDevice, st)); enq();
    ctx_prof_mark(c, 2);                                           // lisreg_get_timing: "index" = the compaction, the sort, the distributions
    k_ft_compact<<<F.n_tiles, kFtTile, 0, st>>>(F.d_jobs, F.d_tiles, F.d_desc, F.tile_base); enq();
    for (const FtBatch::Group& g : F.groups) {
        launch_build_targets_batched(F.d_blk + g.blk0, g.n_blks, F.d_tseg + g.seg0, g.n_segs, g.elems, (int)g.cells, sort_buffers(c), st);
        enq();
    }
    if (k == 0) return LISREG_OK;                                  // a family without distributions: the search grids are all it wants
    if (k <= 20) k_ft_knn<20><<<F.n_blk * 4, 64, 0, st>>>(F.d_blk, F.d_desc);
    else         k_ft_knn<32><<<F.n_blk * 4, 64, 0, st>>>(F.d_blk, F.d_desc);
    enq();
    return LISREG_OK;
}

}  // namespace
