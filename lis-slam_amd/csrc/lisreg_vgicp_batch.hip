// lisreg_vgicp_batch.hip — VGICP verification of a loop-closure candidate list as one call: the loop of
// detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) aligns one key-frame cloud against every candidate submap
// and picks the winner by getFitnessScore() and hasConverged(), with the verifier its authors wrote down last
// (select_registration_method("FAST_VGICP"), :2771).  The definition is tests/vgicp_batch_ref.py: the loop of single alignments plus the
// fitness score and the `best` rule of §7m.  Every item of a batch gets the bits lisreg_vgicp_align returns for it alone: the lanes run
// the same body (lisreg_vgicp_lane.hpp) over the same partition of the source into wavefronts, the partial records are added in
// the single call's order (sum_records of lisreg_fp64_sums.hpp), and the Levenberg-Marquardt loop is the single aligner's (lisreg_lm_stepper.hpp).
// What the batch saves: a source's distributions are made once per call, and the outstanding evaluations of ALL unfinished items are
// answered by one round of launches and one synchronisation.  VGICP derives its pairs again at every evaluation, so an item owns no
// device memory.  The fitness score searches the grid lisreg_vgicp_set_target keeps with the slot, with FastGICP's search
// (lisreg_fgicp_lane.hpp).  This unit holds the linearising kernel and what it launches per round; the host side of a call is the
// driver the batch units share (lisreg_batch_driver.hpp).  No LDS, no atomics, no CPU fallback.
#include "lisreg_batch_rounds.hpp"
#include "lisreg_vgicp_lane.hpp"
#include "lisreg_batch_driver.hpp"

using namespace lisreg;
using namespace lisreg::vgicp_host;

namespace {

// One evaluation of one item.  The entries of a round sit in one array, the linearising ones first; wg_start[e] is the first workgroup
// of entry e over the whole round (wg_start[n_entries] = their number), so a workgroup's number is also the number of its partial record.
struct VgWork {
    VoxelView    G;
    VgPose    P;
    long long src_off;     // the source's first finite point in the batch's point / covariance buffers
    int       n;           // finite points of the source
    int       reserved;
};

// The evaluations of the entries [e_lo, e_hi) of the round (the linearising ones with HESS, the error evaluations without): lanes
// 64 b .. 64 b + 63 of the entry's source, one partial record per workgroup, as k_vgicp_linearize.  Launched over the workgroups
// wg_start[e_lo] .. wg_start[e_hi].  NB: the neighbourhood of the batch (1, 7 or 27 cells, §7w).
template <bool HESS, int NB>
__global__ __launch_bounds__(64) void k_vgicp_linearize_batch(const VgWork* __restrict__ work, const int* __restrict__ wg_start, int e_lo, int e_hi,
                                                              const float4* __restrict__ src, const double* __restrict__ cov,
                                                              double* __restrict__ part)
{
    const int g = wg_start[e_lo] + (int)blockIdx.x;
    const int e = fg_entry_of(wg_start, e_lo, e_hi, g);
    const VgWork* __restrict__ w = work + e;
    const int n = w->n;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    const VoxelView G = w->G;
    const VgPose P = w->P;
    const size_t s = (size_t)w->src_off + (size_t)i;
    double acc[28], pairs;
    if constexpr (NB == 1) vg_linearize_lane<HESS>(i < n, src + s, cov + s * 6, G, P, acc, pairs);
    else                   vg_linearize_lane_nb<HESS, NB>(i < n, src + s, cov + s * 6, G, P, acc, pairs);
    if (threadIdx.x == 0) {
        double* o = part + (size_t)g * kOut;
#pragma unroll
        for (int k = 0; k < 28; ++k) o[k] = acc[k];
        o[28] = pairs;
    }
}

// ---- host: what VGICP supplies to the driver of lisreg_batch_driver.hpp -------------------------------------------------------------------
struct VgBatch : LmBatchFamily<lisreg_vgicp_params, lisreg_vgicp_result> {
    static constexpr const char* kWho = "vgicp_align_batch";
    using Params = lisreg_vgicp_params;
    using ItemC  = lisreg_vgicp_item;
    using Result = lisreg_vgicp_result;
    using Info   = lisreg_vgicp_batch_info;
    using Target = VgicpTarget;
    using Work   = VgWork;
    static constexpr bool kFitnessTotalsApart = false;             // the fitness pass: "solve" = the search with its totals, one interval

    static BatchBufs& bufs(lisreg_ctx* c) { return c->vgb; }
    static int check_params(lisreg_ctx* c, const Params* P) { return vg_check_params(c, P, kWho); }
    // (with P: params->resolution must be the resolution of EVERY named slot)
    static int find_target(lisreg_ctx* c, int slot, const Params* P, Target** T) { return vg_find_target(c, slot, P, kWho, T); }
    static hipError_t ensure_lanes(lisreg_ctx*, long long) { return hipSuccess; }      // an item owns no device memory

    // the search's view of the grid a slot keeps (cov = nullptr: the search reads the points and the cells only)
    static FgTarget fit_view(const Target& G)
    {
        FgTarget A;
        A.sorted = G.sorted.as<float4>(); A.cell_start = G.cells.as<int>(); A.cov = nullptr;
        A.ox = G.grid.ox; A.oy = G.grid.oy; A.oz = G.grid.oz; A.cell = G.grid.cell; A.nx = G.grid.nx; A.ny = G.grid.ny; A.nz = G.grid.nz;
        for (int k = 0; k < 3; ++k) { A.b0[k] = (double)G.bb[k]; A.b1[k] = (double)G.bb[3 + k]; }
        return A;
    }

    static void fill(const Target& T, const Params&, const Stepper& lm, long long src_off, long long, int n, Work* w)
    {
        w->G = voxel_table_view(T);
        w->P = vgicp_host::pose_of<VgPose>(lm.req_T);
        w->src_off = src_off; w->n = n; w->reserved = 0;
    }

    template <int NB>
    static void launch_round_nb(const BatchRound<Work>& r)
    {
        if (r.n_lin) k_vgicp_linearize_batch<true, NB><<<r.g_lin, 64, 0, r.st>>>(r.work, r.start, 0, r.n_lin, r.src, r.cov, r.part);
        if (r.ne > r.n_lin) k_vgicp_linearize_batch<false, NB><<<r.g - r.g_lin, 64, 0, r.st>>>(r.work, r.start, r.n_lin, r.ne, r.src, r.cov, r.part);
    }

    // a batch has one neighbourhood, that of its params
    static void launch_round(lisreg_ctx* c, const Params& P, const BatchRound<Work>& r)
    {
        ctx_prof_mark(c, 0);                                       // lisreg_get_timing: "assoc" = the evaluations of a round (with the totals), one interval
        switch (vg_neighbor_search(P)) {
        case LISREG_VGICP_DIRECT7:  launch_round_nb<7>(r); break;
        case LISREG_VGICP_DIRECT27: launch_round_nb<27>(r); break;
        default:                    launch_round_nb<1>(r); break;                                 // 0 and 1 (vg_check_params)
        }
    }
};

}  // namespace

extern "C" int lisreg_vgicp_align_batch(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt,
                                        const lisreg_vgicp_item* items, int n_items, const lisreg_vgicp_params* P,
                                        lisreg_vgicp_result* results, double* fitness, lisreg_vgicp_batch_info* info)
{
    return batch_align<VgBatch>(c, sources, n, n_sources, stride, fmt, items, n_items, P, results, fitness, info);
}
