// lisreg_vgicp_target_batch.hip — lisreg_vgicp_set_target_batch: the VGICP targets of a whole candidate list
// (detectLoopClosureForSubMap, src/node/subMapOptmizationNode.cpp:2779-2846: setInputTarget at :2793 inside the candidate loop) in one
// launch sequence whose length does not depend on the number of targets, with two host synchronisations.  Every slot ends up, byte for
// byte, as lisreg_vgicp_set_target leaves it for its cloud alone.
//
// The first half of a VGICP target is a FastGICP target's: phases A and B of lisreg_target_batch_shared.hpp (finite points, boxes, search
// grids, distributions), with the search grid straight into the slot's `sorted` / `cells` and the covariances into the context's scratch.
// What this unit adds is the voxel half:
//  - the host decides every target's voxel geometry between the phases with the single call's function (voxel_table_geometry), so the
//    third per-target failure (a grid beyond 2^26 cells) needs no device work either;
//  - ONE voxel sort over the finite points of all targets (lisreg_voxel_sort_batch.hpp, which lisreg_ndt_set_target_batch runs over all
//    records of its targets), keyed by (target, the target's own pcl::VoxelGrid index): every target owns a
//    range of buckets, so the sorted sequence is target by target, each "ascending cell id, ties by index among the finite points" — the
//    total order launch_voxel_sort gives the single call;
//  - one launch fills every dense table with -1 (a table of (pointer, length) chunks; no workgroup spans two targets);
//  - the statistics of all voxels of all targets in one pair of launches that read the voxel count from device memory
//    (launch_voxel_stats_dev over VtBuild, whose body is the single kernels': vg_voxel_lane);
//  - `stats` / `cell` of a slot are sized by min(finite points, grid cells), an upper bound of its voxels, so the voxel counts are read
//    back only at the end: two synchronisations instead of three (§7u gives the memory this costs).
#include "lisreg_vgicp_lane.hpp"
#include "lisreg_target_batch_shared.hpp"
#include "lisreg_vg_voxel_lane.hpp"
#include "lisreg_voxel_sort_batch.hpp"

#include <algorithm>
#include <set>

using namespace lisreg;

namespace {

// One target of the batch as the voxel kernels read it (by job index; m == 0: dropped)
struct VtTarget {
    const float4* pts;         // its finite points, input order
    const double* cov;         // [m][6]
    double*       stats;       // the slot's: [cap][kVoxelRec]
    int*          cell;        // [cap]
    int*          table;       // [n_cells]
    long long     n_cells;
    VoxelDesc     d;           // geometry + bucket span
    int           pbase, m;    // first sorted position (the live targets' finite points end to end), finite points
    int           bucket_base, n_buckets;
    int           cap;         // records `stats` / `cell` hold: min(m, n_cells)
    // the sort's key of the target's finite point e (lisreg_voxel_sort_batch.hpp)
    static __device__ __forceinline__ uint32_t key(const VtTarget& T, int e) { return voxel_index(T.pts[e], T.d); }
};
static_assert(sizeof(VtTarget) == 96, "table layout");

// The family's record for launch_voxel_stats_dev (lisreg_fp64_sums.hpp): voxel v of the batch belongs to the last target whose first voxel
// is not behind v (targets without voxels share the next one's base and lose); the body is the single kernels'
struct VtBuild {
    const VtTarget* tg;
    int             n_targets;
    const int*      vox_base;   // [n_targets + 1]
    const int*      n_vox;      // = vox_base + n_targets
    const int*      vstart;
    const int*      order;
    const uint32_t* sidx;
    template <bool WAVE> static __device__ __forceinline__ void voxel(const VtBuild& B, int v, int lane)
    {
        const int lo = vt_target_of(B.vox_base, B.n_targets, v);
        const VtTarget& T = B.tg[lo];
        const int vl = v - B.vox_base[lo];
        if (vl >= T.cap) return;                                    // (cannot happen: a target has at most min(m, n_cells) voxels)
        vg_voxel_lane<WAVE>(T.pts, T.cov, B.order, B.sidx, B.vstart[v], B.vstart[v + 1], lane, vl, T.n_cells,
                            T.stats + (size_t)vl * kVoxelRec, T.cell + vl, T.table);
    }
};

}  // namespace

extern "C" {

int lisreg_vgicp_target_batch_counts(const lisreg_ctx* c, int* enqueues, int* synchronisations)
{
    if (!c || !enqueues || !synchronisations) return LISREG_ERR_ARG;
    *enqueues = c->vt_enqueues; *synchronisations = c->vt_syncs;
    return LISREG_OK;
}

int lisreg_vgicp_set_target_batch(lisreg_ctx* c, int n_targets, lisreg_vgicp_target_job* jobs, const lisreg_vgicp_params* P)
{
    if (!c) return LISREG_ERR_ARG;
    const char* who = "vgicp_set_target_batch";
    // ---- whole-call refusals: nothing is touched ----------------------------------------------------------------------------------------
    if (n_targets < 0 || n_targets > LISREG_VGICP_TARGET_BATCH_MAX)
        return bad(c, std::string(who) + ": n_targets outside 0 .. " + std::to_string(LISREG_VGICP_TARGET_BATCH_MAX));
    if (n_targets > 0 && !jobs) return bad(c, std::string(who) + ": NULL jobs with n_targets > 0");
    int rc = vg_check_params(c, P, who);
    if (rc) return rc;
    long long total_n = 0;
    {
        std::set<int> seen;
        for (int t = 0; t < n_targets; ++t) {
            const lisreg_vgicp_target_job& J = jobs[t];
            const std::string job = std::string(who) + ": job " + std::to_string(t);
            if (J.slot < 0 || J.slot > 65535) return bad(c, job + ": bad slot");
            if (!seen.insert(J.slot).second) return bad(c, job + ": its slot is named twice in this call");
            if (J.n <= 0) return bad(c, job + ": n <= 0");
            if (!J.cloud) return bad(c, job + ": NULL cloud with n > 0");
            total_n += J.n;
        }
    }
    if (total_n > (long long)LISREG_VGICP_TARGET_BATCH_MAX_POINTS)
        return bad(c, std::string(who) + ": more than " + std::to_string(LISREG_VGICP_TARGET_BATCH_MAX_POINTS) + " points in all");
    c->vt_enqueues = 0; c->vt_syncs = 0;
    if (n_targets == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const FtEnq enq{ &c->vt_enqueues };
    const int N = n_targets, k = P->k_correspondences;
    std::vector<VgicpTarget*> T((size_t)N);
    FtBatch F;
    for (int t = 0; t < N; ++t) {
        T[(size_t)t] = &c->vgicp[jobs[t].slot];
        T[(size_t)t]->valid = false;
        jobs[t].status = LISREG_OK;
        memset(&jobs[t].info, 0, sizeof jobs[t].info);
        F.add_job(jobs[t].cloud, jobs[t].n);
    }
    // ---- phase A: three enqueues and the read-back, whatever n_targets ---------------------------------------------------------------------
    rc = ft_phase_a(c, who, F, enq, &c->vt_syncs);
    if (rc) return rc;
    // ---- the host between the phases: every target's verdict (the single call's three checks, in its order) and voxel geometry ----------------
    struct Plan { bool live; int min_b[3], dims[3]; VoxelDesc d; long long total; int pbase; long long want; };
    std::vector<Plan> plan((size_t)N);
    std::string first_failure;
    long long M = 0, want_all = 0, n_chunks = 0;
    for (int t = 0; t < N; ++t) {
        Plan& p = plan[(size_t)t];
        p.live = false; p.pbase = (int)M;
        const FtStat& S = F.hs[t];
        std::string why;
        if (const char* w = ft_verdict(S, k)) why = w;
        else voxel_table_geometry(S.bb, P->resolution, "voxel table", p.min_b, p.dims, &p.d, &p.total, &why);
        if (!why.empty()) {
            jobs[t].status = LISREG_ERR_ARG;
            if (first_failure.empty()) first_failure = std::string(who) + ": job " + std::to_string(t) + ": vgicp_set_target: " + why;
            continue;
        }
        p.live = true;
        p.want = vt_buckets_wanted(p.total, S.m);
        want_all += p.want;
        n_chunks += (p.total + kVtFillChunk - 1) / kVtFillChunk;
        M += S.m;
    }
    if (!first_failure.empty()) c->err = first_failure;
    if (M > 0) {
        // ---- scratch and tables: everything is sized before phase B is enqueued (a buffer that grows waits for the device) ---------------------
        const size_t z_tg = sizeof(VtTarget) * (size_t)N, z_ch = sizeof(VtChunk) * (size_t)n_chunks, z_res = sizeof(int) * (2 * (size_t)N + 1);
        const size_t z_up = z_tg + z_ch;
        HIPCHK(c, c->vt_host.ensure(z_up + z_res, z_up + z_res + (z_up + z_res) / 2 + 4096));
        HIPCHK(c, c->vt_tab.ensure(z_up + z_res));
        HIPCHK(c, c->vg_idx.ensure(sizeof(int) * (size_t)F.n_points));
        HIPCHK(c, c->vg_cov.ensure(sizeof(double) * 6 * (size_t)M));
        VtTarget* ht = reinterpret_cast<VtTarget*>(c->vt_host.as<char>());
        VtChunk* hc = reinterpret_cast<VtChunk*>(c->vt_host.as<char>() + z_tg);
        const int* hres = reinterpret_cast<const int*>(c->vt_host.as<char>() + z_up);
        const VtTarget* d_tg = reinterpret_cast<const VtTarget*>(c->vt_tab.as<char>());
        const VtChunk* d_ch = reinterpret_cast<const VtChunk*>(c->vt_tab.as<char>() + z_tg);
        int* vox_base = reinterpret_cast<int*>(c->vt_tab.as<char>() + z_up);
        int* n_vox = vox_base + N + 1;
        memset(ht, 0, z_tg);
        long long n_buckets = 0, ic = 0;
        for (int t = 0; t < N; ++t) {
            Plan& p = plan[(size_t)t];
            VtTarget& V = ht[t];
            V.pbase = p.pbase; V.bucket_base = (int)n_buckets;
            if (!p.live) continue;
            const FtStat& S = F.hs[t];
            VgicpTarget& G = *T[(size_t)t];
            const int m = S.m;
            // the search grid: the single call's choice, straight into the slot
            VgGrid vg;
            vg_grid_geometry(S.bb, m, 0.f, &vg);
            const size_t n_grid_cells = (size_t)vg.nx * (size_t)vg.ny * (size_t)vg.nz;
            const size_t cap = (size_t)std::min((long long)m, p.total);
            HIPCHK(c, G.sorted.ensure(sizeof(float4) * (size_t)m));
            HIPCHK(c, G.cells.ensure(sizeof(int) * (n_grid_cells + 1)));
            HIPCHK(c, G.stats.ensure(sizeof(double) * kVoxelRec * cap));
            HIPCHK(c, G.cell.ensure(sizeof(int) * cap));
            HIPCHK(c, G.table.ensure(sizeof(int) * (size_t)p.total));
            ft_grid_index(vg, m, G.sorted.as<float4>(), G.cells.as<int>(), &G.grid);
            for (int e = 0; e < 6; ++e) G.bb[e] = S.bb[e];
            for (int e = 0; e < 3; ++e) { G.dims[e] = p.dims[e]; G.min_b[e] = p.min_b[e]; }
            G.resolution = P->resolution; G.n_points = m; G.n_voxels = 0;
            double* cov = c->vg_cov.as<double>() + 6 * (size_t)p.pbase;
            ft_add_target(c, F, t, vg, k, P->plane_epsilon, G.sorted.as<float4>(), G.cells.as<int>(), c->vg_idx.as<int>() + F.hj[(size_t)t].off, cov);
            // the voxel sort's share of the buckets and the span that follows from it
            int nbk = 0;
            p.d.span = vt_bucket_span(p.total, p.want, want_all, &nbk);
            V.pts = F.hd[t].pts_out; V.cov = cov; V.stats = G.stats.as<double>(); V.cell = G.cell.as<int>(); V.table = G.table.as<int>();
            V.n_cells = p.total; V.d = p.d; V.m = m; V.n_buckets = nbk; V.cap = (int)cap;
            n_buckets += V.n_buckets;
            for (long long s0 = 0; s0 < p.total; s0 += kVtFillChunk)
                hc[ic++] = VtChunk{ V.table + s0, (int)std::min((long long)kVtFillChunk, p.total - s0), 0 };
        }
        const int Mi = (int)M, B = (int)n_buckets, big_cap = voxel_stats_big_capacity(Mi);
        rc = ensure_sort_scratch(c, (size_t)Mi, (size_t)std::max(B, Mi) + 1);
        if (rc) return rc;
        HIPCHK(c, c->vox_order.ensure(sizeof(int) * (size_t)Mi));
        HIPCHK(c, c->vox_sidx.ensure(sizeof(uint32_t) * (size_t)Mi));
        HIPCHK(c, c->vox_head.ensure(sizeof(int) * ((size_t)Mi + 1)));
        HIPCHK(c, c->vox_slot.ensure(sizeof(int) * ((size_t)Mi + 2)));
        HIPCHK(c, c->vox_start.ensure(sizeof(int) * ((size_t)Mi + 2)));
        HIPCHK(c, c->vt_big.ensure(16 + sizeof(int) * (size_t)big_cap));
        // ---- phase B: the compaction, the search grids, the distributions ---------------------------------------------------------------------
        rc = ft_phase_b(c, F, k, enq);
        if (rc) return rc;
        // ---- the voxel half: one table up, one fill, one sort, one pair of statistics launches -----------------------------------------------------
        const SortBuffers sb = sort_buffers(c);
        int *order = c->vox_order.as<int>(), *head = c->vox_head.as<int>(), *slot = c->vox_slot.as<int>(), *vstart = c->vox_start.as<int>();
        uint32_t* sidx = c->vox_sidx.as<uint32_t>();
        int* big_count = c->vt_big.as<int>();
        int* big_list = big_count + 4;
        const BlockDesc* blk = F.d_blk;
        const int nb = F.n_blk;
        ctx_prof_mark(c, 1);                                       // lisreg_get_timing: "solve" = the voxel sort and statistics
        HIPCHK(c, hipMemcpyAsync(c->vt_tab.p, c->vt_host.p, z_up, hipMemcpyHostToDevice, st)); enq();
        HIPCHK(c, hipMemsetAsync(sb.hist, 0, sizeof(int) * (size_t)B, st)); enq();          // the extent this call uses, once
        k_vt_fill<<<(unsigned)n_chunks, 256, 0, st>>>(d_ch); enq();
        launch_voxel_sort_targets(blk, nb, d_tg, N, Mi, B, sb, order, sidx, head, slot, vstart, vox_base, n_vox, big_count, st);
        enq(kVtSortEnqueues);
        VtBuild Bd;
        Bd.tg = d_tg; Bd.n_targets = N; Bd.vox_base = vox_base; Bd.n_vox = vox_base + N; Bd.vstart = vstart; Bd.order = order; Bd.sidx = sidx;
        launch_voxel_stats_dev(Bd, Mi, big_count, big_list, st); enq(2);
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        // ---- the end: every target's voxel count ---------------------------------------------------------------------------------------------
        HIPCHK(c, hipMemcpyAsync(c->vt_host.as<char>() + z_up, vox_base, z_res, hipMemcpyDeviceToHost, st)); enq();
        HIPCHK(c, hipStreamSynchronize(st)); ++c->vt_syncs;
        ctx_prof_collect(c);
        for (int t : F.seg_job) {
            const int nv = hres[N + 1 + t];
            if (nv < 1 || nv > ht[t].cap) return ctx_fail(c, LISREG_ERR_HIP, std::string(who) + ": the voxel sort returned an impossible voxel count");
        }
        for (int t : F.seg_job) {
            VgicpTarget& G = *T[(size_t)t];
            G.n_voxels = hres[N + 1 + t];
            for (int e = 0; e < 3; ++e) jobs[t].info.dims[e] = G.dims[e];
            jobs[t].info.n_voxels = G.n_voxels; jobs[t].info.n_points = G.n_points;
            G.valid = true;
        }
    }
    return LISREG_OK;
}

int lisreg_vgicp_get_target(lisreg_ctx* c, int slot, lisreg_vgicp_info* info, int voxel_dims[3], int voxel_min_b[3], double* resolution,
                            float geom[11], int grid_dims[3], float* sorted_xyzw, int* cell_start, int* table, int capacity_points,
                            int capacity_cells, int capacity_table)
{
    if (!c) return LISREG_ERR_ARG;
    VgicpTarget* G = nullptr;
    int rc = vg_find_target(c, slot, nullptr, "vgicp_get_target", &G);
    if (rc) return rc;
    const GridIndex& g = G->grid;
    const int m = G->n_points, n_cells = g.nx * g.ny * g.nz;
    const long long n_table = (long long)G->dims[0] * G->dims[1] * G->dims[2];
    if (info) { for (int e = 0; e < 3; ++e) info->dims[e] = G->dims[e]; info->n_voxels = G->n_voxels; info->n_points = m; }
    if (voxel_dims) for (int e = 0; e < 3; ++e) voxel_dims[e] = G->dims[e];
    if (voxel_min_b) for (int e = 0; e < 3; ++e) voxel_min_b[e] = G->min_b[e];
    if (resolution) *resolution = G->resolution;
    if (geom) {
        geom[0] = g.ox; geom[1] = g.oy; geom[2] = g.oz; geom[3] = g.cell; geom[4] = g.inv_cell;
        for (int e = 0; e < 6; ++e) geom[5 + e] = G->bb[e];
    }
    if (grid_dims) { grid_dims[0] = g.nx; grid_dims[1] = g.ny; grid_dims[2] = g.nz; }
    if (capacity_points < 0 || capacity_cells < 0 || capacity_table < 0) return bad(c, "vgicp_get_target: negative capacity");
    if (sorted_xyzw && capacity_points < m) return bad(c, "vgicp_get_target: capacity_points < the target's points");
    if (cell_start && capacity_cells < n_cells + 1) return bad(c, "vgicp_get_target: capacity_cells < the grid's cells + 1");
    if (table && (long long)capacity_table < n_table) return bad(c, "vgicp_get_target: capacity_table < the voxel grid's cells");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (sorted_xyzw) HIPCHK(c, hipMemcpyAsync(sorted_xyzw, G->sorted.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (cell_start) HIPCHK(c, hipMemcpyAsync(cell_start, G->cells.p, sizeof(int) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost, st));
    if (table) HIPCHK(c, hipMemcpyAsync(table, G->table.p, sizeof(int) * (size_t)n_table, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

}  // extern "C"
