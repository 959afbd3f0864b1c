// lisreg_fgicp_target_batch.hip — lisreg_fgicp_set_target_batch: the FastGICP targets of a whole candidate list
// (detectLoopClosureForSubMap, src/node/subMapOptmizationNode.cpp:2779-2846: setInputTarget at :2793 inside the candidate loop) in one
// launch sequence whose length does not depend on the number of targets, with two host synchronisations.  Every slot ends up, byte for
// byte, as lisreg_fgicp_set_target leaves it for its cloud alone.
//
// What differs from the single call (lisreg_fgicp.hip over vg_distributions, lisreg_vgicp.hip):
//  - per-target state lives in device tables: a workgroup of a per-point kernel is one tile of one target (host-made tile table) and
//    loads its target's record as scalars; no workgroup waits for another, no float atomics;
//  - phase A (finite counts, bounding boxes, the tiles' bases) ends in ONE read-back of every target's (m, bb[6]); the host then chooses
//    each grid with the single call's function (vg_grid_geometry), marks and drops the targets that fail, sizes the slots' buffers and
//    uploads one table of descriptors;
//  - phase B compacts the finite points (their indices straight into the slot's `orig`), sorts all grids in one bucket sort
//    (launch_build_targets_batched: its order inside a cell is the single build's, ascending index) straight into the slots' `sorted` /
//    `cells`, and makes the distributions of all targets in one launch (vg_knn_lane, the single kernel's body) straight into the slots'
//    `cov`: no device-to-device copy;
//  - a failure (fewer finite points than k_correspondences, an infinite coordinate, an empty box) stays with its target.
#include "lisreg_fgicp_lane.hpp"
#include "lisreg_vg_knn_lane.hpp"

#include <cmath>
#include <cstring>
#include <set>
#include <vector>

using namespace lisreg;

namespace {

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
// go straight into the slot's `orig`.  Tiles of a dropped target return at once.
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
    orig_out[dst] = t.start + (int)threadIdx.x;
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

struct Enq { lisreg_ctx* c; void operator()(int n = 1) const { c->ft_enqueues += n; } };

}  // namespace

extern "C" {

int lisreg_fgicp_grid_geometry(const float bb[6], int n_points, float cell_edge, int dims[3], float cell[2])
{
    if (!bb || !dims || !cell || n_points <= 0 || !(cell_edge >= 0.f) || !std::isfinite(cell_edge)) return LISREG_ERR_ARG;
    for (int k = 0; k < 6; ++k) if (!std::isfinite(bb[k])) return LISREG_ERR_ARG;
    if (!(bb[0] <= bb[3] && bb[1] <= bb[4] && bb[2] <= bb[5])) return LISREG_ERR_ARG;
    VgGrid g;
    vg_grid_geometry(bb, n_points, cell_edge, &g);
    dims[0] = g.nx; dims[1] = g.ny; dims[2] = g.nz; cell[0] = g.cell; cell[1] = g.inv_cell;
    return LISREG_OK;
}

int lisreg_fgicp_target_batch_counts(const lisreg_ctx* c, int* enqueues, int* synchronisations)
{
    if (!c || !enqueues || !synchronisations) return LISREG_ERR_ARG;
    *enqueues = c->ft_enqueues; *synchronisations = c->ft_syncs;
    return LISREG_OK;
}

int lisreg_fgicp_set_target_batch(lisreg_ctx* c, int n_targets, lisreg_fgicp_target_job* jobs, const lisreg_fgicp_params* P)
{
    if (!c) return LISREG_ERR_ARG;
    const char* who = "fgicp_set_target_batch";
    // ---- whole-call refusals: nothing is touched ----------------------------------------------------------------------------------------
    if (n_targets < 0 || n_targets > LISREG_FGICP_TARGET_BATCH_MAX)
        return bad(c, std::string(who) + ": n_targets outside 0 .. " + std::to_string(LISREG_FGICP_TARGET_BATCH_MAX));
    if (n_targets > 0 && !jobs) return bad(c, std::string(who) + ": NULL jobs with n_targets > 0");
    int rc = fg_check_params(c, P, who);
    if (rc) return rc;
    long long total = 0;
    {
        std::set<int> seen;
        for (int t = 0; t < n_targets; ++t) {
            const lisreg_fgicp_target_job& J = jobs[t];
            const std::string job = std::string(who) + ": job " + std::to_string(t);
            if (J.slot < 0 || J.slot > 65535) return bad(c, job + ": bad slot");
            if (!seen.insert(J.slot).second) return bad(c, job + ": its slot is named twice in this call");
            if (J.n <= 0) return bad(c, job + ": n <= 0");
            if (!J.cloud) return bad(c, job + ": NULL cloud with n > 0");
            if (!(J.cell_edge >= 0.f) || !std::isfinite(J.cell_edge)) return bad(c, job + ": cell_edge < 0");
            total += J.n;
        }
    }
    if (total > (long long)LISREG_FGICP_TARGET_BATCH_MAX_POINTS)
        return bad(c, std::string(who) + ": more than " + std::to_string(LISREG_FGICP_TARGET_BATCH_MAX_POINTS) + " points in all");
    c->ft_enqueues = 0; c->ft_syncs = 0;
    if (n_targets == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const Enq enq{ c };
    const int N = n_targets, k = P->k_correspondences;
    std::vector<FgicpTarget*> T((size_t)N);
    for (int t = 0; t < N; ++t) {
        T[(size_t)t] = &c->fgicp[jobs[t].slot];
        T[(size_t)t]->valid = false;
        jobs[t].status = LISREG_OK;
        memset(&jobs[t].info, 0, sizeof jobs[t].info);
    }
    // ---- the tables of phase A ------------------------------------------------------------------------------------------------------------
    std::vector<FtJob> hj((size_t)N);
    int n_tiles = 0, off = 0;
    for (int t = 0; t < N; ++t) {
        FtJob& j = hj[(size_t)t];
        j.cloud = static_cast<const float4*>(jobs[t].cloud); j.n = jobs[t].n; j.off = off; j.tile0 = n_tiles;
        j.n_tiles = (j.n + kFtTile - 1) / kFtTile;
        n_tiles += j.n_tiles; off += j.n;
    }
    const int n_points = off;
    // pinned host side: [jobs | tiles] up, [stats] down, then [descs | tsegs | blocks] up; the device table has the same layout
    const size_t z_jobs = sizeof(FtJob) * (size_t)N, z_tiles = sizeof(FtTile) * (size_t)n_tiles, z_stat = sizeof(FtStat) * (size_t)N;
    const size_t z_desc = sizeof(FtDesc) * (size_t)N, z_tseg = sizeof(TargetSeg) * (size_t)N;
    const size_t z_blk = sizeof(BlockDesc) * ((size_t)n_points / kBlockQ + (size_t)N);
    const size_t o_tiles = (z_jobs + 15) & ~(size_t)15, o_stat = o_tiles + z_tiles, o_desc = o_stat + z_stat, o_tseg = o_desc + z_desc,
                 o_blk = o_tseg + z_tseg, z_all = o_blk + z_blk;
    HIPCHK(c, c->ft_host.ensure(z_all, z_all + z_all / 2 + 4096));
    HIPCHK(c, c->ft_tab.ensure(z_all));
    HIPCHK(c, c->ft_part.ensure((sizeof(int) * 2 + sizeof(float) * 6) * (size_t)n_tiles));
    HIPCHK(c, c->vg_pts.ensure(sizeof(float4) * (size_t)n_points));
    char* h = c->ft_host.as<char>();
    char* d = c->ft_tab.as<char>();
    memcpy(h, hj.data(), z_jobs);
    FtTile* ht = reinterpret_cast<FtTile*>(h + o_tiles);
    for (int t = 0, i = 0; t < N; ++t)
        for (int b = 0; b < hj[(size_t)t].n_tiles; ++b, ++i)
            ht[i] = FtTile{ t, b * kFtTile, std::min(kFtTile, hj[(size_t)t].n - b * kFtTile), 0 };
    const FtJob* d_jobs = reinterpret_cast<const FtJob*>(d);
    const FtTile* d_tiles = reinterpret_cast<const FtTile*>(d + o_tiles);
    FtStat* d_stat = reinterpret_cast<FtStat*>(d + o_stat);
    const FtDesc* d_desc = reinterpret_cast<const FtDesc*>(d + o_desc);
    const TargetSeg* d_tseg = reinterpret_cast<const TargetSeg*>(d + o_tseg);
    const BlockDesc* d_blk = reinterpret_cast<const BlockDesc*>(d + o_blk);
    int* tile_cnt = c->ft_part.as<int>();
    int* tile_base = tile_cnt + n_tiles;
    float* tile_bb = reinterpret_cast<float*>(tile_base + n_tiles);
    // ---- phase A: three enqueues and the read-back, whatever n_targets ---------------------------------------------------------------------
    HIPCHK(c, hipMemcpyAsync(d, h, o_stat, hipMemcpyHostToDevice, st)); enq();
    k_ft_tiles<<<n_tiles, kFtTile, 0, st>>>(d_jobs, d_tiles, tile_cnt, tile_bb); enq();
    k_ft_stats<<<N, 64, 0, st>>>(d_jobs, tile_cnt, tile_bb, tile_base, d_stat); enq();
    HIPCHK(c, hipGetLastError());
    const FtStat* hs = reinterpret_cast<const FtStat*>(h + o_stat);
    HIPCHK(c, hipMemcpyAsync(h + o_stat, d_stat, z_stat, hipMemcpyDeviceToHost, st)); enq();
    HIPCHK(c, hipStreamSynchronize(st)); ++c->ft_syncs;
    // ---- the host between the phases: every target's verdict, grid and buffers ------------------------------------------------------------------
    for (int t = 0; t < N; ++t)
        if (hs[t].m < 0 || hs[t].m > jobs[t].n) return ctx_fail(c, LISREG_ERR_HIP, std::string(who) + ": the compaction returned an impossible count");
    FtDesc* hd = reinterpret_cast<FtDesc*>(h + o_desc);
    TargetSeg* hseg = reinterpret_cast<TargetSeg*>(h + o_tseg);
    BlockDesc* hb = reinterpret_cast<BlockDesc*>(h + o_blk);
    memset(hd, 0, z_desc);
    struct Group { int seg0, n_segs, blk0, n_blks, elems; long long cells; };
    std::vector<Group> groups;
    std::vector<int> seg_job;
    std::string first_failure;
    int n_seg = 0, n_blk = 0;
    for (int t = 0; t < N; ++t) {
        const FtStat& S = hs[t];
        const char* why = nullptr;                                  // the single call's checks, in its order (vg_distributions, vg_search_grid)
        for (int e = 0; e < 6; ++e) if (std::isinf(S.bb[e])) why = "the cloud has infinite coordinates";
        if (!why && (S.m < k || !(S.bb[0] <= S.bb[3] && S.bb[1] <= S.bb[4] && S.bb[2] <= S.bb[5])))
            why = "the cloud has fewer finite points than k_correspondences";
        if (why) {
            jobs[t].status = LISREG_ERR_ARG;
            if (first_failure.empty()) first_failure = std::string(who) + ": job " + std::to_string(t) + ": fgicp_set_target: " + why;
            continue;
        }
        FgicpTarget& G = *T[(size_t)t];
        VgGrid vg;
        vg_grid_geometry(S.bb, S.m, jobs[t].cell_edge, &vg);
        const int m = S.m, n_cells = vg.nx * vg.ny * vg.nz;
        HIPCHK(c, G.sorted.ensure(sizeof(float4) * (size_t)m));
        HIPCHK(c, G.cells.ensure(sizeof(int) * ((size_t)n_cells + 1)));
        HIPCHK(c, G.orig.ensure(sizeof(int) * (size_t)m));
        HIPCHK(c, G.cov.ensure(sizeof(double) * 6 * (size_t)m));
        memset(&G.grid, 0, sizeof G.grid);
        G.grid.n = m; G.grid.ox = vg.ox; G.grid.oy = vg.oy; G.grid.oz = vg.oz; G.grid.cell = vg.cell; G.grid.inv_cell = vg.inv_cell;
        G.grid.nx = vg.nx; G.grid.ny = vg.ny; G.grid.nz = vg.nz;
        G.grid.pts = G.sorted.as<float4>(); G.grid.cell_start = G.cells.as<int>();
        for (int e = 0; e < 6; ++e) G.bb[e] = S.bb[e];
        G.n_points = m;
        if (groups.empty() || groups.back().cells + n_cells > kFtMaxSortCells) groups.push_back(Group{ n_seg, 0, n_blk, 0, 0, 0 });
        Group& g = groups.back();
        FtDesc& D = hd[t];
        D.pts_out = c->vg_pts.as<float4>() + hj[(size_t)t].off;
        D.orig_out = G.orig.as<int>();
        D.A.sorted = G.sorted.as<float4>(); D.A.cell_start = G.cells.as<int>(); D.A.pts = D.pts_out; D.A.orig = D.orig_out;
        D.A.m = m; D.A.k = k; D.A.ox = vg.ox; D.A.oy = vg.oy; D.A.oz = vg.oz; D.A.cell = vg.cell; D.A.inv_cell = vg.inv_cell;
        D.A.nx = vg.nx; D.A.ny = vg.ny; D.A.nz = vg.nz; D.A.plane_eps = P->plane_epsilon; D.A.cov = G.cov.as<double>(); D.A.nbr = nullptr;
        TargetSeg& ts = hseg[n_seg];
        memset(&ts, 0, sizeof ts);
        ts.raw = D.pts_out; ts.sorted_out = G.sorted.as<float4>(); ts.cell_start_out = G.cells.as<int>();
        ts.n = m; ts.n_cells = n_cells; ts.flat_base = g.elems; ts.bucket_base = (int)g.cells;
        ts.ox = vg.ox; ts.oy = vg.oy; ts.oz = vg.oz; ts.inv_cell = vg.inv_cell; ts.nx = vg.nx; ts.ny = vg.ny; ts.nz = vg.nz;
        for (int s0 = 0; s0 < m; s0 += kBlockQ) hb[n_blk++] = BlockDesc{ g.n_segs, s0, std::min(kBlockQ, m - s0), t };
        g.n_blks = n_blk - g.blk0;
        g.elems += m; g.cells += n_cells; ++g.n_segs; ++n_seg;
        seg_job.push_back(t);
    }
    if (!first_failure.empty()) c->err = first_failure;
    // ---- phase B: one table, the compaction, the sort and the distributions ---------------------------------------------------------------------
    if (n_seg > 0) {
        int max_elems = 0; long long max_cells = 0;
        for (const Group& g : groups) { max_elems = std::max(max_elems, g.elems); max_cells = std::max(max_cells, g.cells); }
        rc = ensure_sort_scratch(c, (size_t)max_elems, (size_t)max_cells + 1);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(d + o_desc, h + o_desc, o_blk + sizeof(BlockDesc) * (size_t)n_blk - o_desc, hipMemcpyHostToDevice, st)); enq();
        ctx_prof_mark(c, 2);                                       // lisreg_get_timing: "index" = the compaction, the sort, the distributions
        k_ft_compact<<<n_tiles, kFtTile, 0, st>>>(d_jobs, d_tiles, d_desc, tile_base); enq();
        for (const Group& g : groups) {
            launch_build_targets_batched(d_blk + g.blk0, g.n_blks, d_tseg + g.seg0, g.n_segs, g.elems, (int)g.cells, sort_buffers(c), st);
            enq();
        }
        if (k <= 20) k_ft_knn<20><<<n_blk * 4, 64, 0, st>>>(d_blk, d_desc);
        else         k_ft_knn<32><<<n_blk * 4, 64, 0, st>>>(d_blk, d_desc);
        enq();
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st)); ++c->ft_syncs;
        ctx_prof_collect(c);
    }
    for (int t : seg_job) {
        FgicpTarget& G = *T[(size_t)t];
        jobs[t].info.grid_dims[0] = G.grid.nx; jobs[t].info.grid_dims[1] = G.grid.ny; jobs[t].info.grid_dims[2] = G.grid.nz;
        jobs[t].info.n_points = G.n_points;
        G.valid = true;
    }
    return LISREG_OK;
}

int lisreg_fgicp_get_target(lisreg_ctx* c, int slot, lisreg_fgicp_info* info, float geom[11], float* sorted_xyzw, int* cell_start, int* orig,
                            double* cov6, int capacity_points, int capacity_cells)
{
    if (!c) return LISREG_ERR_ARG;
    FgicpTarget* G = nullptr;
    int rc = fg_find_target(c, slot, "fgicp_get_target", &G);
    if (rc) return rc;
    const GridIndex& g = G->grid;
    const int m = G->n_points, n_cells = g.nx * g.ny * g.nz;
    if (info) { info->grid_dims[0] = g.nx; info->grid_dims[1] = g.ny; info->grid_dims[2] = g.nz; info->n_points = m; }
    if (geom) {
        geom[0] = g.ox; geom[1] = g.oy; geom[2] = g.oz; geom[3] = g.cell; geom[4] = g.inv_cell;
        for (int e = 0; e < 6; ++e) geom[5 + e] = G->bb[e];
    }
    if (capacity_points < 0 || capacity_cells < 0) return bad(c, "fgicp_get_target: negative capacity");
    if ((sorted_xyzw || orig || cov6) && capacity_points < m) return bad(c, "fgicp_get_target: capacity_points < the target's points");
    if (cell_start && capacity_cells < n_cells + 1) return bad(c, "fgicp_get_target: capacity_cells < the grid's cells + 1");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (sorted_xyzw) HIPCHK(c, hipMemcpyAsync(sorted_xyzw, G->sorted.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (cell_start) HIPCHK(c, hipMemcpyAsync(cell_start, G->cells.p, sizeof(int) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost, st));
    if (orig) HIPCHK(c, hipMemcpyAsync(orig, G->orig.p, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (cov6) HIPCHK(c, hipMemcpyAsync(cov6, G->cov.p, sizeof(double) * 6 * (size_t)m, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

}  // extern "C"
