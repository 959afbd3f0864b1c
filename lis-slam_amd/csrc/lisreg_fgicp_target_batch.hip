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
// The kernels and the host code of both phases are in lisreg_target_batch_shared.hpp, which lisreg_vgicp_set_target_batch (§7u) runs too:
// this unit chooses where a target's sorted points, cells, indices and covariances go (the FastGICP slot) and keeps the entry points.
#include "lisreg_fgicp_lane.hpp"
#include "lisreg_vg_knn_lane.hpp"
#include "lisreg_target_batch_shared.hpp"      // phases A and B (k_ft_tiles, k_ft_stats, k_ft_compact, k_ft_knn over vg_knn_lane<KT>): shared with the VGICP twin

#include <cmath>
#include <cstring>
#include <set>
#include <vector>

using namespace lisreg;

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
    const FtEnq enq{ &c->ft_enqueues };
    const int N = n_targets, k = P->k_correspondences;
    std::vector<FgicpTarget*> T((size_t)N);
    FtBatch F;
    for (int t = 0; t < N; ++t) {
        T[(size_t)t] = &c->fgicp[jobs[t].slot];
        T[(size_t)t]->valid = false;
        jobs[t].status = LISREG_OK;
        memset(&jobs[t].info, 0, sizeof jobs[t].info);
        F.add_job(jobs[t].cloud, jobs[t].n);
    }
    // ---- phase A: three enqueues and the read-back, whatever n_targets ---------------------------------------------------------------------
    rc = ft_phase_a(c, who, F, enq, &c->ft_syncs);
    if (rc) return rc;
    // ---- the host between the phases: every target's verdict, grid and buffers ------------------------------------------------------------------
    std::string first_failure;
    for (int t = 0; t < N; ++t) {
        const FtStat& S = F.hs[t];
        if (const char* why = ft_verdict(S, k)) {                   // the single call's checks, in its order
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
        ft_grid_index(vg, m, G.sorted.as<float4>(), G.cells.as<int>(), &G.grid);
        for (int e = 0; e < 6; ++e) G.bb[e] = S.bb[e];
        G.n_points = m;
        ft_add_target(c, F, t, vg, k, P->plane_epsilon, G.sorted.as<float4>(), G.cells.as<int>(), G.orig.as<int>(), G.cov.as<double>());
    }
    if (!first_failure.empty()) c->err = first_failure;
    // ---- phase B: one table, the compaction, the sort and the distributions ---------------------------------------------------------------------
    if (F.n_seg > 0) {
        rc = ft_phase_b(c, F, k, enq);
        if (rc) return rc;
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st)); ++c->ft_syncs;
        ctx_prof_collect(c);
    }
    for (int t : F.seg_job) {
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
