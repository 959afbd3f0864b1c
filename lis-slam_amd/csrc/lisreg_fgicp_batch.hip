// lisreg_fgicp_batch.hip — FastGICP verification of a loop-closure candidate list as one call: the loop of
// detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) aligns one key-frame cloud against every candidate submap
// and picks the winner by getFitnessScore() and hasConverged().  The definition is tests/fgicp_batch_ref.py: the loop of single
// alignments plus the fitness score and the `best` rule.  Every item of a batch gets the bits lisreg_fgicp_align returns for it alone:
// the lanes run the same bodies (lisreg_fgicp_lane.hpp) over the same partition of the source into wavefronts, the partial records are
// added in the single call's order (sum_records of lisreg_fp64_sums.hpp), and the Levenberg-Marquardt loop is the single aligner's (lisreg_lm_stepper.hpp).  What the batch
// saves: a source's distributions are made once per call, and the outstanding evaluations of ALL unfinished items are answered by one
// round of launches and one synchronisation.  This unit holds the search and sum kernels and what they are launched with per round; the
// host side of a call is the driver the batch units share (lisreg_batch_driver.hpp).  No LDS, no atomics, no CPU fallback.
#include "lisreg_batch_rounds.hpp"
#include "lisreg_batch_driver.hpp"

using namespace lisreg;
using namespace lisreg::vgicp_host;

namespace {

// One evaluation of one item.  The entries of a round sit in one array, the linearising ones first; wg_start[e] is the first workgroup
// of entry e over the whole round (wg_start[n_entries] = their number), so a workgroup's number is also the number of its partial record.
struct FgWork {
    FgTarget  A;
    FgPose    P;
    long long src_off;     // the source's first finite point in the batch's point / covariance buffers
    long long lane_off;    // the item's first lane in the batch's pair / M buffers
    int       n;           // finite points of the source
    int       reserved;
};

// The search of every linearising entry (entries [0, n_lin) of the round): lanes 64 b .. 64 b + 63 of the entry's source, as k_fgicp_pairs
__global__ __launch_bounds__(64) void k_fgicp_pairs_batch(const FgWork* __restrict__ work, const int* __restrict__ wg_start, int n_lin,
                                                          const float4* __restrict__ src, const double* __restrict__ scov, double max_d, double max2,
                                                          int* __restrict__ pair, double* __restrict__ M6)
{
    const int g = blockIdx.x;
    const int e = fg_entry_of(wg_start, 0, n_lin, g);
    const FgWork* __restrict__ w = work + e;
    const int n = w->n;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    if (i >= n) return;
    const FgTarget A = w->A;
    const FgPose   P = w->P;
    const size_t s = (size_t)w->src_off + (size_t)i, l = (size_t)w->lane_off + (size_t)i;
    fg_pairs_lane(src[s], scov + s * 6, A, P, max_d, max2, pair + l, M6 + l * 6, nullptr);
}

// The sums of the entries [e_lo, e_hi) of the round (the linearising ones with HESS, the error evaluations without), over the pairs and
// the M their items hold: one partial record per workgroup, as k_fgicp_sums.  Launched over the workgroups wg_start[e_lo] .. wg_start[e_hi].
template <bool HESS>
__global__ __launch_bounds__(64) void k_fgicp_sums_batch(const FgWork* __restrict__ work, const int* __restrict__ wg_start, int e_lo, int e_hi,
                                                         const float4* __restrict__ src, const int* __restrict__ pair, const double* __restrict__ M6,
                                                         double* __restrict__ part)
{
    const int g = wg_start[e_lo] + (int)blockIdx.x;
    const int e = fg_entry_of(wg_start, e_lo, e_hi, g);
    const FgWork* __restrict__ w = work + e;
    const int n = w->n;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    const FgPose P = w->P;
    const size_t s = (size_t)w->src_off + (size_t)i, l = (size_t)w->lane_off + (size_t)i;
    double acc[28], pairs;
    const int j = i < n ? pair[l] : -1;
    fg_sums_lane<HESS>(j, src + s, M6 + l * 6, w->A.sorted, P, acc, pairs);
    if (threadIdx.x == 0) {
        double* o = part + (size_t)g * kOut;
#pragma unroll
        for (int k = 0; k < 28; ++k) o[k] = acc[k];
        o[28] = pairs;
    }
}

// ---- host: what FastGICP supplies to the driver of lisreg_batch_driver.hpp ---------------------------------------------------------------
struct FgBatch : LmBatchFamily<lisreg_fgicp_params, lisreg_fgicp_result> {
    static constexpr const char* kWho = "fgicp_align_batch";
    using Params = lisreg_fgicp_params;
    using ItemC  = lisreg_fgicp_item;
    using Result = lisreg_fgicp_result;
    using Info   = lisreg_fgicp_batch_info;
    using Target = FgicpTarget;
    using Work   = FgWork;
    static constexpr bool kFitnessTotalsApart = true;              // the fitness pass: "solve" = the search, "assoc" = its totals

    static BatchBufs& bufs(lisreg_ctx* c) { return c->fgb; }
    static int check_params(lisreg_ctx* c, const Params* P) { return fg_check_params(c, P, kWho); }
    static int find_target(lisreg_ctx* c, int slot, const Params*, Target** T) { return fg_find_target(c, slot, kWho, T); }
    static FgTarget fit_view(const Target& T) { return fg_target_view(T); }

    // the items' storage: 4 + 48 bytes per (item, finite source point)
    static hipError_t ensure_lanes(lisreg_ctx* c, long long lanes)
    {
        const hipError_t e = c->fgb_pair.ensure(sizeof(int) * (size_t)lanes);
        return e != hipSuccess ? e : c->fgb_M.ensure(sizeof(double) * 6 * (size_t)lanes);
    }

    static void fill(const Target& T, const Params&, const Stepper& lm, long long src_off, long long lane_off, int n, Work* w)
    {
        w->A = fg_target_view(T);
        w->P = vgicp_host::pose_of<FgPose>(lm.req_T);
        w->src_off = src_off; w->lane_off = lane_off; w->n = n; w->reserved = 0;
    }

    static void launch_round(lisreg_ctx* c, const Params& P, const BatchRound<Work>& r)
    {
        const double max_d = P.max_correspondence_distance;
        int* const    pair = c->fgb_pair.as<int>();
        double* const M6 = c->fgb_M.as<double>();
        if (r.n_lin) {
            ctx_prof_mark(c, 1);                                   // lisreg_get_timing: "solve" = the search launches, one interval each
            k_fgicp_pairs_batch<<<r.g_lin, 64, 0, r.st>>>(r.work, r.start, r.n_lin, r.src, r.cov, max_d, max_d * max_d, pair, M6);
        }
        ctx_prof_mark(c, 0);                                       // "assoc" = the sum launches of a round (with the totals), one interval
        if (r.n_lin) k_fgicp_sums_batch<true><<<r.g_lin, 64, 0, r.st>>>(r.work, r.start, 0, r.n_lin, r.src, pair, M6, r.part);
        if (r.ne > r.n_lin) k_fgicp_sums_batch<false><<<r.g - r.g_lin, 64, 0, r.st>>>(r.work, r.start, r.n_lin, r.ne, r.src, pair, M6, r.part);
    }
};

}  // namespace

extern "C" int lisreg_fgicp_align_batch(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt,
                                        const lisreg_fgicp_item* items, int n_items, const lisreg_fgicp_params* P,
                                        lisreg_fgicp_result* results, double* fitness, lisreg_fgicp_batch_info* info)
{
    return batch_align<FgBatch>(c, sources, n, n_sources, stride, fmt, items, n_items, P, results, fitness, info);
}
