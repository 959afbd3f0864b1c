// lisreg_ndt_batch.hip — NDT verification of a loop-closure candidate list as one call: the loop of
// detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) aligns one key-frame cloud against every candidate submap
// and picks the winner by getFitnessScore() and hasConverged(), with the verifier the reference names first
// (select_registration_method("NDT"), src/core/registration.cpp:147-155).  The definition is tests/ndt_batch_ref.py: the loop of single
// alignments plus the fitness score and the `best` rule of §7m.  Every item of a batch gets the bits lisreg_ndt_align returns for it
// alone: the lanes run the same body (lisreg_ndt_lane.hpp) over the same partition of the source's RECORDS into wavefronts (NaN records
// keep their lanes, as in the single call), the partial records are added in the single call's order (sum_records of
// lisreg_fp64_sums.hpp), and the Newton loop with its line search is the single aligner's (lisreg_ndt_stepper.hpp).  What the batch
// saves: a source is uploaded once per call, and the outstanding evaluations of ALL unfinished items are answered by one round of
// launches and one synchronisation.  NDT derives its pairs again at every evaluation, so an item owns no device memory.  The fitness
// score searches the grid lisreg_ndt_set_target keeps with the slot, with FastGICP's search (lisreg_fgicp_lane.hpp).  This unit holds
// the evaluation kernel and what it launches per round; the host side of a call is the driver the batch units share
// (lisreg_batch_driver.hpp).  No LDS, no atomics, no CPU fallback.
#include "lisreg_batch_rounds.hpp"
#include "lisreg_ndt_lane.hpp"
#include "lisreg_batch_driver.hpp"

using namespace lisreg;
using namespace lisreg::ndt_host;

namespace {

// One evaluation of one item (about 0.8 KB; its address is the same on every lane of a workgroup).  The entries of a round sit in one
// array, those with the Hessian first; wg_start[e] is the first workgroup of entry e over the whole round (wg_start[n_entries] = their
// number), so a workgroup's number is also the number of its partial record.
struct NdtWork {
    VoxelView G;
    NdtGauss  K;
    NdtPose   P;
    long long src_off;     // the source's first record in the batch's record buffer
    int       n;           // records of the source
    int       reserved;
};

// The evaluations of the entries [e_lo, e_hi) of the round (those with the Hessian, those without): lanes 64 b .. 64 b + 63 of the
// entry's source by RECORD, one partial record per workgroup, as k_ndt_eval.  Launched over the workgroups wg_start[e_lo] ..
// wg_start[e_hi].  The entry is read in place: the lane's body takes its 96 doubles of pose at constant offsets from one address.
template <bool HESS>
__global__ __launch_bounds__(64) void k_ndt_eval_batch(const NdtWork* __restrict__ work, const int* __restrict__ wg_start, int e_lo, int e_hi,
                                                       const float4* __restrict__ src, double* __restrict__ part)
{
    const int g = wg_start[e_lo] + (int)blockIdx.x;
    const int e = fg_entry_of(wg_start, e_lo, e_hi, g);
    const NdtWork* __restrict__ w = work + e;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    double acc[28], pairs;
    ndt_eval_lane<HESS>(i < w->n, src + ((size_t)w->src_off + (size_t)i), w->G, w->K, w->P, acc, pairs);
    ndt_store_partial(acc, pairs, part + (size_t)g * kEvalOut);
}

// the finite records among src[0, n): one wavefront, exact in double
__global__ __launch_bounds__(64) void k_ndt_count_finite(const float4* __restrict__ src, int n, int* __restrict__ out)
{
    double cnt = 0.0;
    for (int i = (int)threadIdx.x; i < n; i += 64) {
        const float4 p = src[i];
        cnt += (p.x == p.x && p.y == p.y && p.z == p.z) ? 1.0 : 0.0;
    }
    cnt = wave_sum(cnt);
    if (threadIdx.x == 0) *out = (int)cnt;
}

// ---- host: what NDT supplies to the driver of lisreg_batch_driver.hpp ---------------------------------------------------------------------
struct NdBatch {
    static constexpr const char* kWho = "ndt_align_batch";
    using Params  = lisreg_ndt_params;
    using ItemC   = lisreg_ndt_item;
    using Result  = lisreg_ndt_result;
    using Info    = lisreg_ndt_batch_info;
    using Target  = NdtTarget;
    using Work    = NdtWork;
    using Stepper = NdtStepper;
    static constexpr int  kRec = kNdtOut;
    static constexpr bool kFitnessTotalsApart = false;             // the fitness pass: "solve" = the search with its totals, one interval

    static BatchBufs& bufs(lisreg_ctx* c) { return c->ndb; }
    static int check_params(lisreg_ctx* c, const Params* P) { return ndt_check_params(c, P, kWho); }
    // (params->resolution must be the resolution of EVERY named slot; a slot without a target refuses the batch as an argument error)
    static int find_target(lisreg_ctx* c, int slot, const Params* P, Target** T)
    {
        const int rc = ndt_find_target(c, slot, P, kWho, T);
        return rc == LISREG_ERR_NO_TARGET ? bad(c, std::string(kWho) + ": no NDT target in this slot (lisreg_ndt_set_target)") : rc;
    }
    static hipError_t ensure_lanes(lisreg_ctx*, long long) { return hipSuccess; }      // an item owns no device memory

    static void start(Stepper& s, const Target&, const float* guess, const Params& P, int n_records)
    {
        double p0[6];
        p_from_matrix(guess, p0);
        s.start(p0, ndt_loop_params_of(P), n_records);
    }

    // a source is its raw records, NaN ones included (the single call partitions the records into wavefronts): no covariances
    static hipError_t ensure_sources(BatchBufs& B, size_t records) { return B.src.ensure(sizeof(float4) * records); }
    static int stage_source(lisreg_ctx* c, const char*, const Params&, const void* cloud, int n, int stride, int fmt, BatchBufs& B, long long off,
                            bool want_finite, int* m_out, int* n_finite)
    {
        hipStream_t st = c->stream;
        const float4* raw = nullptr;
        const int rc = stage_records(c, cloud, n, stride, fmt, c->ndt_src, &raw);
        if (rc) return rc;
        float4* dst = B.src.as<float4>() + off;
        HIPCHK(c, hipMemcpyAsync(dst, raw, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, st));
        *m_out = n; *n_finite = n;
        if (want_finite) {                                         // the fitness mean is over the finite points
            HIPCHK(c, c->ndt_cnt.ensure(sizeof(int) * 4));
            k_ndt_count_finite<<<1, 64, 0, st>>>(dst, n, c->ndt_cnt.as<int>());
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(n_finite, c->ndt_cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
        }
        return LISREG_OK;
    }

    // the search's view of the grid a slot keeps (cov = nullptr: the search reads the points and the cells only)
    static FgTarget fit_view(const Target& G)
    {
        FgTarget A;
        A.sorted = G.sorted.as<float4>(); A.cell_start = G.cells.as<int>(); A.cov = nullptr;
        A.ox = G.grid.ox; A.oy = G.grid.oy; A.oz = G.grid.oz; A.cell = G.grid.cell; A.nx = G.grid.nx; A.ny = G.grid.ny; A.nz = G.grid.nz;
        for (int k = 0; k < 3; ++k) { A.b0[k] = (double)G.bb[k]; A.b1[k] = (double)G.bb[3 + k]; }
        return A;
    }
    // the score is taken at the pose the evaluations use: R, t of pose_matrices(p) in double, not the float final_transform
    static FgPose fit_pose(const NdtLoopResult& lr)
    {
        NdtPose Pm;
        pose_matrices(lr.p, &Pm);
        FgPose P;
        memcpy(P.R, Pm.R, sizeof P.R); memcpy(P.t, Pm.t, sizeof P.t);
        return P;
    }
    static void result_to(const NdtLoopResult& lr, Result* res) { ndt_result_to(lr, res); }

    static void fill(const Target& T, const Params& P, const Stepper& s, long long src_off, long long, int n, Work* w)
    {
        w->G = voxel_table_view(T);
        double g1, g2;
        gauss_constants(P.outlier_ratio, P.resolution, &g1, &g2);
        w->K = NdtGauss{ T.resolution * T.resolution, g1, g2 };
        pose_matrices(s.req_p, &w->P);
        w->src_off = src_off; w->n = n; w->reserved = 0;
    }

    static void launch_round(lisreg_ctx* c, const Params&, const BatchRound<Work>& r)
    {
        ctx_prof_mark(c, 0);                                       // lisreg_get_timing: "assoc" = the evaluations of a round (with the totals), one interval
        if (r.n_lin) k_ndt_eval_batch<true><<<r.g_lin, 64, 0, r.st>>>(r.work, r.start, 0, r.n_lin, r.src, r.part);
        if (r.ne > r.n_lin) k_ndt_eval_batch<false><<<r.g - r.g_lin, 64, 0, r.st>>>(r.work, r.start, r.n_lin, r.ne, r.src, r.part);
    }
};

}  // namespace

extern "C" int lisreg_ndt_align_batch(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt,
                                      const lisreg_ndt_item* items, int n_items, const lisreg_ndt_params* P, lisreg_ndt_result* results,
                                      double* fitness, lisreg_ndt_batch_info* info)
{
    return batch_align<NdBatch>(c, sources, n, n_sources, stride, fmt, items, n_items, P, results, fitness, info);
}
