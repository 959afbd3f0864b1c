// lisreg_ndt_target_batch.hip — lisreg_ndt_set_target_batch: the NDT targets of a whole candidate list
// (detectLoopClosureForSubMap, src/node/subMapOptmizationNode.cpp:2779-2846: setInputTarget at :2793 inside the candidate loop) in one
// launch sequence whose length does not depend on the number of targets, with two host synchronisations.  Every slot ends up, byte for
// byte, as lisreg_ndt_set_target leaves it for its cloud alone.
//
// The search grid of an NDT target is a FastGICP target's without the distributions: phases A and B of lisreg_target_batch_shared.hpp
// with k = 0 (finite points, boxes, search grids straight into the slot's `sorted` / `cells`; no indices, no covariances).  The voxel
// half is the VGICP batch's sort (lisreg_voxel_sort_batch.hpp) with two differences that are NDT's own:
//  - the sort runs over ALL records of a target, not its finite points: the single call sorts a cleaned copy of the whole cloud in which
//    a record with a NaN coordinate sits on the box's minimum corner, so such records are in cell 0's run, give cell 0 a voxel record even
//    when it holds no finite point (which shifts every voxel number of the table) and count towards the run length that decides between
//    the lane and the wavefront path.  Here the key of a NaN record is cell 0 and the records are read where the caller keeps them: no
//    cleaned copy;
//  - the per-voxel body is the single kernels' (ndt_voxel_lane, lisreg_ndt_voxel_lane.hpp), with the occupied and the valid voxels
//    counted per target in a device table the call clears once.
// `stats` / `cell` / `vflag` of a slot are sized by min(records, grid cells), an upper bound of its voxel records, so the three counts of
// every target are read back only at the end (§7v gives the memory this costs).
#include "lisreg_ndt_lane.hpp"
#include "lisreg_ndt_voxel_lane.hpp"
#include "lisreg_target_batch_shared.hpp"
#include "lisreg_voxel_sort_batch.hpp"

#include <algorithm>
#include <set>

using namespace lisreg;

namespace {

// One target of the batch as the voxel kernels read it (by job index; m == 0: dropped)
struct NtTarget {
    const float4* pts;         // the caller's records
    double*       stats;       // the slot's: [cap][kVoxelRec]
    int*          cell;        // [cap]
    int*          vflag;       // [cap]
    int*          table;       // [n_cells]
    long long     n_cells;
    VoxelDesc     d;           // geometry + bucket span
    int           pbase, m;    // first sorted position (the live targets' records end to end), records
    int           bucket_base, n_buckets;
    int           cap;         // records `stats` / `cell` / `vflag` hold: min(m, n_cells)
    // the sort's key of the target's record e (lisreg_voxel_sort_batch.hpp): its voxel; a record with a NaN coordinate belongs to no
    // voxel and goes where k_ndt_clean puts it, the box's minimum corner — cell 0
    static __device__ __forceinline__ uint32_t key(const NtTarget& T, int e)
    {
        const float4 p = T.pts[e];
        return NdtSkipNaN::skip(p) ? 0u : voxel_index(p, T.d);
    }
};
static_assert(sizeof(NtTarget) == 96, "table layout");

// The family's record for launch_voxel_stats_dev (lisreg_fp64_sums.hpp); the body is the single kernels'
struct NtBuild {
    const NtTarget* tg;
    int             n_targets;
    const int*      vox_base;   // [n_targets + 1]
    const int*      n_vox;      // = vox_base + n_targets
    const int*      vstart;
    const int*      order;
    const uint32_t* sidx;
    int*            counters;   // [n_targets][2]: voxels with a finite point, valid voxels
    int             min_pts;
    double          mult;
    template <bool WAVE> static __device__ __forceinline__ void voxel(const NtBuild& B, int v, int lane)
    {
        const int lo = vt_target_of(B.vox_base, B.n_targets, v);
        const NtTarget& T = B.tg[lo];
        const int vl = v - B.vox_base[lo];
        if (vl >= T.cap) return;                                    // (cannot happen: a target has at most min(m, n_cells) voxel records)
        ndt_voxel_lane<WAVE, NdtSkipNaN>(T.pts, B.order, B.sidx, B.vstart[v], B.vstart[v + 1], lane, vl, T.n_cells, B.min_pts, B.mult,
                                         T.stats + (size_t)vl * kVoxelRec, T.vflag + vl, T.cell + vl, T.table, B.counters + 2 * lo);
    }
};

}  // namespace

extern "C" {

int lisreg_ndt_target_batch_counts(const lisreg_ctx* c, int* enqueues, int* synchronisations)
{
    if (!c || !enqueues || !synchronisations) return LISREG_ERR_ARG;
    *enqueues = c->nt_enqueues; *synchronisations = c->nt_syncs;
    return LISREG_OK;
}

int lisreg_ndt_set_target_batch(lisreg_ctx* c, int n_targets, lisreg_ndt_target_job* jobs, const lisreg_ndt_params* P)
{
    if (!c) return LISREG_ERR_ARG;
    const char* who = "ndt_set_target_batch";
    c->nt_enqueues = 0; c->nt_syncs = 0;                           // (a refused call enqueues nothing and waits for nothing)
    // ---- whole-call refusals: no slot and no job field is touched ----------------------------------------------------------------------------------------
    if (n_targets < 0 || n_targets > LISREG_NDT_TARGET_BATCH_MAX)
        return bad(c, std::string(who) + ": n_targets outside 0 .. " + std::to_string(LISREG_NDT_TARGET_BATCH_MAX));
    if (n_targets > 0 && !jobs) return bad(c, std::string(who) + ": NULL jobs with n_targets > 0");
    int rc = ndt_check_params(c, P, who);
    if (rc) return rc;
    long long total_n = 0;
    {
        std::set<int> seen;
        for (int t = 0; t < n_targets; ++t) {
            const lisreg_ndt_target_job& J = jobs[t];
            const std::string job = std::string(who) + ": job " + std::to_string(t);
            if (J.slot < 0 || J.slot > 65535) return bad(c, job + ": bad slot");
            if (!seen.insert(J.slot).second) return bad(c, job + ": its slot is named twice in this call");
            if (J.n <= 0) return bad(c, job + ": n <= 0");
            if (!J.cloud) return bad(c, job + ": NULL cloud with n > 0");
            total_n += J.n;
        }
    }
    if (total_n > (long long)LISREG_NDT_TARGET_BATCH_MAX_POINTS)
        return bad(c, std::string(who) + ": more than " + std::to_string(LISREG_NDT_TARGET_BATCH_MAX_POINTS) + " points in all");
    if (n_targets == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const FtEnq enq{ &c->nt_enqueues };
    const int N = n_targets;
    std::vector<NdtTarget*> T((size_t)N);
    FtBatch F;
    for (int t = 0; t < N; ++t) {
        T[(size_t)t] = &c->ndt[jobs[t].slot];
        T[(size_t)t]->valid = false;
        jobs[t].status = LISREG_OK;
        memset(&jobs[t].info, 0, sizeof jobs[t].info);
        F.add_job(jobs[t].cloud, jobs[t].n);
    }
    // ---- phase A: three enqueues and the read-back, whatever n_targets ---------------------------------------------------------------------
    rc = ft_phase_a(c, who, F, enq, &c->nt_syncs);
    if (rc) return rc;
    // ---- the host between the phases: every target's verdict (the single call's first four checks, in its order) and voxel geometry ---------
    struct Plan { bool live; int min_b[3], dims[3]; VoxelDesc d; long long total; int pbase; long long want; };
    std::vector<Plan> plan((size_t)N);
    std::vector<std::string> failure((size_t)N);
    long long M = 0, want_all = 0, n_chunks = 0, n_vblk = 0;
    for (int t = 0; t < N; ++t) {
        Plan& p = plan[(size_t)t];
        p.live = false; p.pbase = (int)M;
        const FtStat& S = F.hs[t];
        std::string& why = failure[(size_t)t];
        bool inf = false;
        for (int e = 0; e < 6; ++e) inf = inf || std::isinf(S.bb[e]);
        if (inf) why = "the cloud has infinite coordinates";
        else if (!(S.bb[0] <= S.bb[3] && S.bb[1] <= S.bb[4] && S.bb[2] <= S.bb[5])) why = "the cloud has no finite point: no valid voxel";
        else if (S.m < 1) why = "the cloud has fewer finite points than k_correspondences";      // (vg_search_grid's text)
        else voxel_table_geometry(S.bb, P->resolution, "cell table", p.min_b, p.dims, &p.d, &p.total, &why);
        if (!why.empty()) { jobs[t].status = LISREG_ERR_ARG; continue; }
        p.live = true;
        const long long n = F.hj[(size_t)t].n;
        p.want = vt_buckets_wanted(p.total, n);
        want_all += p.want;
        n_chunks += (p.total + kVtFillChunk - 1) / kVtFillChunk;
        n_vblk += (n + kBlockQ - 1) / kBlockQ;
        M += n;
    }
    auto report = [&]() {
        for (int t = 0; t < N; ++t)
            if (!failure[(size_t)t].empty()) { c->err = std::string(who) + ": job " + std::to_string(t) + ": ndt_set_target: " + failure[(size_t)t]; return; }
    };
    if (M == 0) { report(); return LISREG_OK; }
    // ---- scratch and tables: everything is sized before phase B is enqueued (a buffer that grows waits for the device) -------------------------
    const size_t z_tg = sizeof(NtTarget) * (size_t)N, z_ch = sizeof(VtChunk) * (size_t)n_chunks, z_bl = sizeof(BlockDesc) * (size_t)n_vblk;
    const size_t z_up = z_tg + z_ch + z_bl, z_res = sizeof(int) * (4 * (size_t)N + 1);
    HIPCHK(c, c->vt_host.ensure(z_up + z_res, z_up + z_res + (z_up + z_res) / 2 + 4096));
    HIPCHK(c, c->vt_tab.ensure(z_up + z_res));
    NtTarget* ht = reinterpret_cast<NtTarget*>(c->vt_host.as<char>());
    VtChunk* hc = reinterpret_cast<VtChunk*>(c->vt_host.as<char>() + z_tg);
    BlockDesc* hb = reinterpret_cast<BlockDesc*>(c->vt_host.as<char>() + z_tg + z_ch);
    const int* hres = reinterpret_cast<const int*>(c->vt_host.as<char>() + z_up);
    const NtTarget* d_tg = reinterpret_cast<const NtTarget*>(c->vt_tab.as<char>());
    const VtChunk* d_ch = reinterpret_cast<const VtChunk*>(c->vt_tab.as<char>() + z_tg);
    const BlockDesc* d_vblk = reinterpret_cast<const BlockDesc*>(c->vt_tab.as<char>() + z_tg + z_ch);
    int* vox_base = reinterpret_cast<int*>(c->vt_tab.as<char>() + z_up);       // [N + 1], then the voxel records [N], then the counters [N][2]
    int* n_vox = vox_base + N + 1;
    int* counters = n_vox + N;
    memset(ht, 0, z_tg);
    long long n_buckets = 0, ic = 0, ib = 0;
    for (int t = 0; t < N; ++t) {
        Plan& p = plan[(size_t)t];
        NtTarget& V = ht[t];
        V.pbase = p.pbase; V.bucket_base = (int)n_buckets;
        if (!p.live) continue;
        const FtStat& S = F.hs[t];
        NdtTarget& G = *T[(size_t)t];
        const int m = S.m, n = F.hj[(size_t)t].n;
        // the search grid: the single call's choice, straight into the slot
        VgGrid vg;
        vg_grid_geometry(S.bb, m, 0.f, &vg);
        const size_t n_grid_cells = (size_t)vg.nx * (size_t)vg.ny * (size_t)vg.nz;
        const size_t cap = (size_t)std::min((long long)n, p.total);
        HIPCHK(c, G.sorted.ensure(sizeof(float4) * (size_t)m));
        HIPCHK(c, G.cells.ensure(sizeof(int) * (n_grid_cells + 1)));
        HIPCHK(c, G.stats.ensure(sizeof(double) * kVoxelRec * cap));
        HIPCHK(c, G.cell.ensure(sizeof(int) * cap));
        HIPCHK(c, G.vflag.ensure(sizeof(int) * cap));
        HIPCHK(c, G.table.ensure(sizeof(int) * (size_t)p.total));
        ft_grid_index(vg, m, G.sorted.as<float4>(), G.cells.as<int>(), &G.grid);
        for (int e = 0; e < 6; ++e) G.bb[e] = S.bb[e];
        for (int e = 0; e < 3; ++e) { G.dims[e] = p.dims[e]; G.min_b[e] = p.min_b[e]; }
        G.resolution = P->resolution; G.n_points = m; G.n_voxels = 0; G.n_occupied = 0; G.n_valid = 0;
        ft_add_target(c, F, t, vg, 0, 0.0, G.sorted.as<float4>(), G.cells.as<int>(), nullptr, nullptr);
        // the voxel sort's share of the buckets and the span that follows from it
        int nbk = 0;
        p.d.span = vt_bucket_span(p.total, p.want, want_all, &nbk);
        V.pts = F.hj[(size_t)t].cloud; V.stats = G.stats.as<double>(); V.cell = G.cell.as<int>(); V.vflag = G.vflag.as<int>();
        V.table = G.table.as<int>();
        V.n_cells = p.total; V.d = p.d; V.m = n; V.n_buckets = nbk; V.cap = (int)cap;
        n_buckets += nbk;
        for (long long s0 = 0; s0 < p.total; s0 += kVtFillChunk)
            hc[ic++] = VtChunk{ V.table + s0, (int)std::min((long long)kVtFillChunk, p.total - s0), 0 };
        for (int s0 = 0; s0 < n; s0 += kBlockQ) hb[ib++] = BlockDesc{ 0, s0, std::min(kBlockQ, n - s0), t };
    }
    const int Mi = (int)M, B = (int)n_buckets, nb = (int)n_vblk, big_cap = voxel_stats_big_capacity(Mi);
    rc = ensure_sort_scratch(c, (size_t)Mi, (size_t)std::max(B, Mi) + 1);
    if (rc) return rc;
    HIPCHK(c, c->vox_order.ensure(sizeof(int) * (size_t)Mi));
    HIPCHK(c, c->vox_sidx.ensure(sizeof(uint32_t) * (size_t)Mi));
    HIPCHK(c, c->vox_head.ensure(sizeof(int) * ((size_t)Mi + 1)));
    HIPCHK(c, c->vox_slot.ensure(sizeof(int) * ((size_t)Mi + 2)));
    HIPCHK(c, c->vox_start.ensure(sizeof(int) * ((size_t)Mi + 2)));
    HIPCHK(c, c->vt_big.ensure(16 + sizeof(int) * (size_t)big_cap));
    // ---- phase B without the distributions: the compaction and the search grids ----------------------------------------------------------------
    rc = ft_phase_b(c, F, 0, enq);
    if (rc) return rc;
    // ---- the voxel half: one table up, two clears, one fill, one sort, one pair of statistics launches ----------------------------------------
    const SortBuffers sb = sort_buffers(c);
    int *order = c->vox_order.as<int>(), *head = c->vox_head.as<int>(), *slot = c->vox_slot.as<int>(), *vstart = c->vox_start.as<int>();
    uint32_t* sidx = c->vox_sidx.as<uint32_t>();
    int* big_count = c->vt_big.as<int>();
    int* big_list = big_count + 4;
    ctx_prof_mark(c, 1);                                           // lisreg_get_timing: "solve" = the voxel sort and the Gaussians
    HIPCHK(c, hipMemcpyAsync(c->vt_tab.p, c->vt_host.p, z_up, hipMemcpyHostToDevice, st)); enq();
    HIPCHK(c, hipMemsetAsync(sb.hist, 0, sizeof(int) * (size_t)B, st)); enq();              // the extent this call uses, once
    HIPCHK(c, hipMemsetAsync(counters, 0, sizeof(int) * 2 * (size_t)N, st)); enq();         // every target's two counts, once
    k_vt_fill<<<(unsigned)n_chunks, 256, 0, st>>>(d_ch); enq();
    launch_voxel_sort_targets(d_vblk, nb, d_tg, N, Mi, B, sb, order, sidx, head, slot, vstart, vox_base, n_vox, big_count, st);
    enq(kVtSortEnqueues);
    NtBuild Bd;
    Bd.tg = d_tg; Bd.n_targets = N; Bd.vox_base = vox_base; Bd.n_vox = vox_base + N; Bd.vstart = vstart; Bd.order = order; Bd.sidx = sidx;
    Bd.counters = counters; Bd.min_pts = P->min_points_per_voxel; Bd.mult = P->min_covar_eigvalue_mult;
    launch_voxel_stats_dev(Bd, Mi, big_count, big_list, st); enq(2);
    ctx_prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    // ---- the end: every target's three counts ----------------------------------------------------------------------------------------------
    HIPCHK(c, hipMemcpyAsync(c->vt_host.as<char>() + z_up, vox_base, z_res, hipMemcpyDeviceToHost, st)); enq();
    HIPCHK(c, hipStreamSynchronize(st)); ++c->nt_syncs;
    ctx_prof_collect(c);
    const int* h_nvox = hres + N + 1;
    const int* h_cnt = h_nvox + N;
    for (int t : F.seg_job) {
        const int nv = h_nvox[t], occ = h_cnt[2 * t], val = h_cnt[2 * t + 1];
        if (nv < 1 || nv > ht[t].cap || occ < 0 || occ > nv || val < 0 || val > occ)
            return ctx_fail(c, LISREG_ERR_HIP, std::string(who) + ": the voxel sort returned an impossible voxel count");
    }
    for (int t : F.seg_job) {
        NdtTarget& G = *T[(size_t)t];
        G.n_voxels = h_nvox[t]; G.n_occupied = h_cnt[2 * t]; G.n_valid = h_cnt[2 * t + 1];
        lisreg_ndt_info& I = jobs[t].info;
        for (int e = 0; e < 3; ++e) I.dims[e] = G.dims[e];
        I.n_voxels = G.n_occupied; I.n_valid = G.n_valid; I.reserved = 0;
        if (G.n_valid < 1) {
            jobs[t].status = LISREG_ERR_ARG;
            failure[(size_t)t] = "the target has no valid voxel (min_points_per_voxel points with a positive-definite covariance)";
            continue;
        }
        G.valid = true;
    }
    report();
    return LISREG_OK;
}

int lisreg_ndt_get_target(lisreg_ctx* c, int slot, lisreg_ndt_info* info, int voxel_dims[3], int voxel_min_b[3], double* resolution,
                          float geom[11], int grid_dims[3], int* n_points, int* n_records, float* sorted_xyzw, int* cell_start, int* table,
                          int* record_cells, int* record_flags, double* records, int capacity_points, int capacity_cells,
                          int capacity_table, int capacity_records)
{
    if (!c) return LISREG_ERR_ARG;
    NdtTarget* G = nullptr;
    int rc = ndt_find_target(c, slot, nullptr, "ndt_get_target", &G);
    if (rc) return rc;
    const GridIndex& g = G->grid;
    const int m = G->n_points, n_cells = g.nx * g.ny * g.nz, nv = G->n_voxels;
    const long long n_table = (long long)G->dims[0] * G->dims[1] * G->dims[2];
    if (info) { for (int e = 0; e < 3; ++e) info->dims[e] = G->dims[e]; info->n_voxels = G->n_occupied; info->n_valid = G->n_valid; info->reserved = 0; }
    if (voxel_dims) for (int e = 0; e < 3; ++e) voxel_dims[e] = G->dims[e];
    if (voxel_min_b) for (int e = 0; e < 3; ++e) voxel_min_b[e] = G->min_b[e];
    if (resolution) *resolution = G->resolution;
    if (geom) {
        geom[0] = g.ox; geom[1] = g.oy; geom[2] = g.oz; geom[3] = g.cell; geom[4] = g.inv_cell;
        for (int e = 0; e < 6; ++e) geom[5 + e] = G->bb[e];
    }
    if (grid_dims) { grid_dims[0] = g.nx; grid_dims[1] = g.ny; grid_dims[2] = g.nz; }
    if (n_points) *n_points = m;
    if (n_records) *n_records = nv;
    if (capacity_points < 0 || capacity_cells < 0 || capacity_table < 0 || capacity_records < 0) return bad(c, "ndt_get_target: negative capacity");
    if (sorted_xyzw && capacity_points < m) return bad(c, "ndt_get_target: capacity_points < the target's points");
    if (cell_start && capacity_cells < n_cells + 1) return bad(c, "ndt_get_target: capacity_cells < the grid's cells + 1");
    if (table && (long long)capacity_table < n_table) return bad(c, "ndt_get_target: capacity_table < the voxel grid's cells");
    if ((record_cells || record_flags || records) && capacity_records < nv) return bad(c, "ndt_get_target: capacity_records < the target's voxel records");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (sorted_xyzw) HIPCHK(c, hipMemcpyAsync(sorted_xyzw, G->sorted.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, st));
    if (cell_start) HIPCHK(c, hipMemcpyAsync(cell_start, G->cells.p, sizeof(int) * ((size_t)n_cells + 1), hipMemcpyDeviceToHost, st));
    if (table) HIPCHK(c, hipMemcpyAsync(table, G->table.p, sizeof(int) * (size_t)n_table, hipMemcpyDeviceToHost, st));
    if (record_cells) HIPCHK(c, hipMemcpyAsync(record_cells, G->cell.p, sizeof(int) * (size_t)nv, hipMemcpyDeviceToHost, st));
    if (record_flags) HIPCHK(c, hipMemcpyAsync(record_flags, G->vflag.p, sizeof(int) * (size_t)nv, hipMemcpyDeviceToHost, st));
    if (records) HIPCHK(c, hipMemcpyAsync(records, G->stats.p, sizeof(double) * kVoxelRec * (size_t)nv, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

}  // extern "C"
