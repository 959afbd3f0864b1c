// lisreg_gicp_batch.hip — PCL's GICP verification of a loop-closure candidate list as one call: the loop of
// detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) aligns one key-frame cloud against every candidate submap
// and picks the winner by getFitnessScore() and hasConverged(), with the one verifier whose block is live in
// select_registration_method ("GICP", src/core/registration.cpp:137-146).  The definition is tests/gicp_batch_ref.py: the loop of single
// alignments plus the fitness score and the `best` rule of §7m.  Every item of a batch gets the bits lisreg_gicp_align returns for it
// alone: the lanes run the same body (lisreg_gicp_lane.hpp) over the same partition of the source's finite points into wavefronts, the
// partial records are added in the single call's order (sum_records of lisreg_fp64_sums.hpp), and the outer loop with its host BFGS is
// the single aligner's (lisreg_gicp_stepper.hpp).  What the batch saves: a source's distributions are made once per call, and the
// outstanding outer iteration of ALL unfinished items is answered by one moments launch, one totals launch and one synchronisation.
// Nothing per pair goes to memory, so an item owns no device memory.  This unit holds the moments kernel and its launch per round; the
// host side of a call is the driver the batch units share (lisreg_batch_driver.hpp).  No LDS, no read-modify-write on memory, no CPU
// fallback.
#include "lisreg_batch_rounds.hpp"
#include "lisreg_gicp_lane.hpp"
#include "lisreg_gicp_stepper.hpp"
#include "lisreg_batch_driver.hpp"

using namespace lisreg;
using namespace lisreg::gicp_host;

namespace {

// One outer iteration of one item (its address is the same on every lane of a workgroup).  wg_start[e] is the first workgroup of entry
// e over the whole round (wg_start[n_entries] = their number), so a workgroup's number is also the number of its partial record.
struct GicpWork {
    FgTarget   A;
    FgPose     P;
    GicpCentre C;
    long long  src_off;    // the source's first finite point in the batch's point / covariance buffers
    int        n;          // finite points of the source
    int        reserved;
};

// The search and the moments of every entry of the round: lanes 64 b .. 64 b + 63 of the entry's finite source points in input order,
// one partial record of 74 doubles per workgroup, as k_gicp_moments of the single call.  A lane past the end reads the entry's point 0
// and drops it (n >= k_correspondences >= 4).
__global__ __launch_bounds__(64) void k_gicp_moments_batch(const GicpWork* __restrict__ work, const int* __restrict__ wg_start, int n_entries,
                                                           const float4* __restrict__ src, const double* __restrict__ scov, double max_d, double max2,
                                                           double* __restrict__ part)
{
    const int g = blockIdx.x;
    const int e = fg_entry_of(wg_start, 0, n_entries, g);
    const GicpWork* __restrict__ w = work + e;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    const bool live = i < w->n;
    const size_t at = (size_t)w->src_off + (size_t)(live ? i : 0);
    const FgTarget   A = w->A;
    const FgPose     P = w->P;
    const GicpCentre C = w->C;
    gicp_moments_lane(live, src[at], scov + at * 6, A, P, max_d, max2, C, part + (size_t)g * kGicpRec);
}

// ---- host: what GICP supplies to the driver of lisreg_batch_driver.hpp -----------------------------------------------------------------
struct GcBatch : DistributionSources {
    static constexpr const char* kWho = "gicp_align_batch";
    using Params  = lisreg_gicp_params;
    using ItemC   = lisreg_gicp_item;
    using Result  = lisreg_gicp_result;
    using Info    = lisreg_gicp_batch_info;
    using Target  = FgicpTarget;
    using Work    = GicpWork;
    using Stepper = GicpStepper;
    static constexpr int  kRec = kGicpRec;                         // one record per outer iteration: the 74 moments
    static constexpr bool kFitnessTotalsApart = true;              // the fitness pass: "solve" = the search, "assoc" = its totals

    static BatchBufs& bufs(lisreg_ctx* c) { return c->gcb; }
    static int check_params(lisreg_ctx* c, const Params* P) { return gc_check_params(c, P, kWho); }
    static int find_target(lisreg_ctx* c, int slot, const Params*, Target** T) { return fg_find_target(c, slot, kWho, T); }
    static FgTarget fit_view(const Target& T) { return fg_target_view(T); }
    static hipError_t ensure_lanes(lisreg_ctx*, long long) { return hipSuccess; }      // an item owns no device memory

    static void start(Stepper& s, const Target& T, const float* guess, const Params& P, int)
    {
        double G[16];
        vgicp_host::guess_to_T0(guess, G);
        s.start(G, gicp_loop_params_of(P), gicp_centre_of(T).c);
    }
    static int stage_source(lisreg_ctx* c, const char* who, const Params& P, const void* cloud, int n, int stride, int fmt, BatchBufs& B, long long off,
                            bool, int* m_out, int* n_finite)
    {
        return stage_distributions(c, who, P.k_correspondences, P.gicp_epsilon, cloud, n, stride, fmt, B, off, m_out, n_finite);
    }
    // the score is taken at the double final_transform T = X(x) G
    static FgPose fit_pose(const GicpLoopResult& lr) { return vgicp_host::pose_of<FgPose>(lr.T); }
    static void result_to(const GicpLoopResult& lr, Result* res) { gicp_result_to(lr, res); }

    static void fill(const Target& T, const Params&, const Stepper& s, long long src_off, long long, int n, Work* w)
    {
        w->A = fg_target_view(T);
        w->P = vgicp_host::pose_of<FgPose>(s.req_T);
        w->C = gicp_centre_of(T);
        w->src_off = src_off; w->n = n; w->reserved = 0;
    }

    // every request of a round is of one kind: r.n_lin == r.ne, r.g_lin == r.g
    static void launch_round(lisreg_ctx* c, const Params& P, const BatchRound<Work>& r)
    {
        const double max_d = P.max_correspondence_distance;
        ctx_prof_mark(c, 1);                                       // lisreg_get_timing: "solve" = the search-and-moments launch of a round
        k_gicp_moments_batch<<<r.g, 64, 0, r.st>>>(r.work, r.start, r.ne, r.src, r.cov, max_d, max_d * max_d, r.part);
        ctx_prof_mark(c, 0);                                       // "assoc" = its fixed-order totals (the driver launches them)
    }
};

}  // namespace

extern "C" int lisreg_gicp_align_batch(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt,
                                       const lisreg_gicp_item* items, int n_items, const lisreg_gicp_params* P, lisreg_gicp_result* results,
                                       double* fitness, lisreg_gicp_batch_info* info)
{
    return batch_align<GcBatch>(c, sources, n, n_sources, stride, fmt, items, n_items, P, results, fitness, info);
}
