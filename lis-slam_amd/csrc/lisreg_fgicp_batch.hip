// lisreg_fgicp_batch.hip — FastGICP verification of a loop-closure candidate list as one call: the loop of
// detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) aligns one key-frame cloud against every candidate submap
// and picks the winner by getFitnessScore() and hasConverged().  The definition is tests/fgicp_batch_ref.py: the loop of single
// alignments plus the fitness score and the `best` rule.  Every item of a batch gets the bits lisreg_fgicp_align returns for it alone:
// the lanes run the same bodies (lisreg_fgicp_lane.hpp) over the same partition of the source into wavefronts, the partial records are
// added in k_vgicp_total's order, and the Levenberg-Marquardt loop is lm_optimise turned inside out (lisreg_lm_stepper.hpp).  What the
// batch saves: a source's distributions are made once per call, and the outstanding evaluations of ALL unfinished items are answered by
// one round of launches and one synchronisation.  No LDS, no atomics, no CPU fallback.
#include "lisreg_batch_rounds.hpp"
#include "lisreg_lm_stepper.hpp"

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

using namespace lisreg;
using namespace lisreg::vgicp_host;

namespace {

// One evaluation of one item (LM phase), or one item at its final pose (fitness pass).  The entries of a round sit in one array, the
// linearising ones first; wg_start[e] is the first workgroup of entry e over the whole round (wg_start[n_entries] = their number), so
// a workgroup's number is also the number of its partial record.
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

// The fitness pass: the same search at the item's final pose without a cut-off, over every finite source point.  The squared distance
// of lane i goes to the head of the item's M storage (its M is no longer needed), the wavefront's sum to the workgroup's partial.
__global__ __launch_bounds__(64) void k_fgicp_fitness_batch(const FgWork* __restrict__ work, const int* __restrict__ wg_start, int n_entries,
                                                            const float4* __restrict__ src, double* __restrict__ M6, double* __restrict__ part)
{
    const int g = blockIdx.x;
    const int e = fg_entry_of(wg_start, 0, n_entries, g);
    const FgWork* __restrict__ w = work + e;
    const int n = w->n;
    const int i = (g - wg_start[e]) * 64 + (int)threadIdx.x;
    double d2 = 0.0;
    if (i < n) {
        const FgTarget A = w->A;
        const FgPose   P = w->P;
        double qx, qy, qz, bd;
        int    bj;
        fg_transform(P, src[(size_t)w->src_off + (size_t)i], qx, qy, qz);
        fg_search_lane(A, qx, qy, qz, HUGE_VAL, HUGE_VAL, bd, bj);
        d2 = bj >= 0 ? bd : 0.0;
        M6[(size_t)w->lane_off * 6 + (size_t)i] = bj >= 0 ? bd : (double)NAN;
    }
    d2 = fg_wave_sum(d2);
    if (threadIdx.x == 0) part[g] = d2;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
constexpr const char* kWho = "fgicp_align_batch";

struct Source { bool used = false; int m = 0; long long off = 0; };
struct Item { LmStepper lm; const FgicpTarget* T = nullptr; long long lane_off = 0; int src = 0, nb = 0; };

// where the work table of a round lives in its buffer: the entries, then the n_entries + 1 workgroup starts
size_t starts_offset(int n_items) { return sizeof(FgWork) * (size_t)n_items; }
size_t table_bytes(int n_items) { return starts_offset(n_items) + sizeof(int) * ((size_t)n_items + 1); }

}  // namespace

extern "C" int lisreg_fgicp_align_batch(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt,
                                        const lisreg_fgicp_item* items, int n_items, const lisreg_fgicp_params* P,
                                        lisreg_fgicp_result* results, double* fitness, lisreg_fgicp_batch_info* info)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || n_sources < 0) return bad(c, std::string(kWho) + ": n_items < 0 or n_sources < 0");
    if (info) *info = lisreg_fgicp_batch_info{ -1, 0, 0, 0 };
    if (n_items == 0) return LISREG_OK;
    // ---- every refusal that needs no device, for the whole batch ----------------------------------------------------------------
    if (!items || !results || !sources || !n) return bad(c, std::string(kWho) + ": NULL items / results / sources / n");
    int rc = fg_check_params(c, P, kWho);
    if (rc) return rc;
    std::vector<Source> S((size_t)n_sources);
    std::vector<Item>   I((size_t)n_items);
    for (int k = 0; k < n_items; ++k) {
        if (items[k].source < 0 || items[k].source >= n_sources) return bad(c, std::string(kWho) + ": an item's source index is out of range");
        FgicpTarget* T = nullptr;
        rc = fg_find_target(c, items[k].slot, kWho, &T);
        if (rc) return rc;
        I[k].T = T; I[k].src = items[k].source;
        S[items[k].source].used = true;
    }
    size_t cap = 0;
    for (int s = 0; s < n_sources; ++s) {
        if (!S[s].used) continue;                                  // a source no item names is neither checked nor staged
        rc = check_cloud(c, kWho, sources[s], n[s], stride, fmt, kFmtPackable, false);
        if (rc) return rc;
        cap += (size_t)n[s];
    }
    // ---- the sources' distributions, once each; a cloud they refuse (too few finite points, an infinite coordinate) ends the call
    // before any alignment work, with `results` untouched.  The context's scratch is overwritten by the next source: the batch keeps copies
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, c->fgb_src.ensure(sizeof(float4) * cap));
    HIPCHK(c, c->fgb_cov.ensure(sizeof(double) * 6 * cap));
    long long off = 0;
    int n_staged = 0;
    for (int s = 0; s < n_sources; ++s) {
        if (!S[s].used) continue;
        const float4* raw = nullptr;
        rc = stage_records(c, sources[s], n[s], stride, fmt, c->vg_raw, &raw);
        if (rc) return rc;
        float bb[6];
        int m = 0;
        rc = vg_distributions(c, kWho, raw, n[s], P->k_correspondences, P->plane_epsilon, 0.f, bb, &m, nullptr, nullptr);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->fgb_src.as<float4>() + off, c->vg_pts.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->fgb_cov.as<double>() + 6 * off, c->vg_cov.p, sizeof(double) * 6 * (size_t)m, hipMemcpyDeviceToDevice, st));
        S[s].m = m; S[s].off = off;
        off += m;
        ++n_staged;
    }
    // ---- the items' storage: 4 + 48 bytes per (item, finite source point) ----------------------------------------------------------
    long long lanes = 0, wgs = 0;
    for (int k = 0; k < n_items; ++k) {
        I[k].lane_off = lanes; I[k].nb = (S[I[k].src].m + 63) / 64;
        lanes += S[I[k].src].m; wgs += I[k].nb;
    }
    if (wgs > (long long)INT_MAX / kOut) return bad(c, std::string(kWho) + ": the batch is too large (items x source points)");
    HIPCHK(c, c->fgb_pair.ensure(sizeof(int) * (size_t)lanes));
    HIPCHK(c, c->fgb_M.ensure(sizeof(double) * 6 * (size_t)lanes));
    HIPCHK(c, c->fgb_part.ensure(sizeof(double) * kOut * (size_t)wgs));
    HIPCHK(c, c->fgb_out.ensure(sizeof(double) * kOut * (size_t)n_items));
    HIPCHK(c, c->fgb_work.ensure(table_bytes(n_items)));
    HIPCHK(c, c->fgb_host_work.ensure(table_bytes(n_items), table_bytes(n_items) + table_bytes(n_items) / 2));
    HIPCHK(c, c->fgb_host_out.ensure(sizeof(double) * kOut * (size_t)n_items, sizeof(double) * kOut * ((size_t)n_items + (size_t)n_items / 2)));
    FgWork* const  h_work = c->fgb_host_work.as<FgWork>();
    int* const     h_start = reinterpret_cast<int*>(static_cast<char*>(c->fgb_host_work.p) + starts_offset(n_items));
    const FgWork*  d_work = c->fgb_work.as<FgWork>();
    const int*     d_start = reinterpret_cast<const int*>(static_cast<const char*>(c->fgb_work.p) + starts_offset(n_items));
    const float4*  d_src = c->fgb_src.as<float4>();
    auto entry = [&](int k, const double T[16], FgWork* w) {
        w->A = fg_target_view(*I[k].T);
        for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) w->P.R[3 * i + j] = T[4 * i + j]; w->P.t[i] = T[4 * i + 3]; }
        w->src_off = S[I[k].src].off; w->lane_off = I[k].lane_off; w->n = S[I[k].src].m; w->reserved = 0;
    };
    // the table of a round goes up in one copy: the entries and, behind them, the starts (the gap between them is not read)
    auto upload = [&](int ne) -> hipError_t {
        hipError_t e = hipMemcpyAsync(c->fgb_work.p, h_work, sizeof(FgWork) * (size_t)ne, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(const_cast<int*>(d_start), h_start, sizeof(int) * ((size_t)ne + 1), hipMemcpyHostToDevice, st);
    };
    // ---- the LM phase, in lockstep rounds: every unfinished item has one request outstanding -----------------------------------------
    const LmParams lp{ P->transformation_epsilon, P->rotation_epsilon, P->lm_init_lambda_factor, P->max_iters, P->lm_max_iterations };
    for (int k = 0; k < n_items; ++k) {
        const float* guess = items[k].guess;
        double T0[16];
        for (int q = 0; q < 16; ++q) T0[q] = guess ? (double)guess[q] : (q % 5 == 0 ? 1.0 : 0.0);
        T0[12] = T0[13] = T0[14] = 0.0; T0[15] = 1.0;
        I[k].lm.start(T0, lp);
    }
    const double max_d = P->max_correspondence_distance;
    std::vector<int> order((size_t)n_items);
    int n_rounds = 0;
    for (;;) {
        int ne = 0, n_lin = 0;
        for (int k = 0; k < n_items; ++k) if (!I[k].lm.finished() && I[k].lm.req_hessian) order[ne++] = k;
        n_lin = ne;
        for (int k = 0; k < n_items; ++k) if (!I[k].lm.finished() && !I[k].lm.req_hessian) order[ne++] = k;
        if (!ne) break;
        int g = 0;
        for (int e = 0; e < ne; ++e) { entry(order[e], I[order[e]].lm.req_T, h_work + e); h_start[e] = g; g += I[order[e]].nb; }
        h_start[ne] = g;
        const int g_lin = h_start[n_lin];
        HIPCHK(c, upload(ne));
        if (n_lin) {
            ctx_prof_mark(c, 1);                                   // lisreg_get_timing: "solve" = the search launches, one interval each
            k_fgicp_pairs_batch<<<g_lin, 64, 0, st>>>(d_work, d_start, n_lin, d_src, c->fgb_cov.as<double>(), max_d, max_d * max_d,
                                                      c->fgb_pair.as<int>(), c->fgb_M.as<double>());
        }
        ctx_prof_mark(c, 0);                                       // "assoc" = the sum launches of a round (with the totals), one interval
        if (n_lin) k_fgicp_sums_batch<true><<<g_lin, 64, 0, st>>>(d_work, d_start, 0, n_lin, d_src, c->fgb_pair.as<int>(), c->fgb_M.as<double>(),
                                                                   c->fgb_part.as<double>());
        if (ne > n_lin) k_fgicp_sums_batch<false><<<g - g_lin, 64, 0, st>>>(d_work, d_start, n_lin, ne, d_src, c->fgb_pair.as<int>(),
                                                                            c->fgb_M.as<double>(), c->fgb_part.as<double>());
        k_fgicp_total_batch<kOut><<<ne, 64, 0, st>>>(c->fgb_part.as<double>(), d_start, c->fgb_out.as<double>());
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->fgb_host_out.p, c->fgb_out.p, sizeof(double) * kOut * (size_t)ne, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        const double* out = c->fgb_host_out.as<double>();
        for (int e = 0; e < ne; ++e) I[order[e]].lm.feed(out + (size_t)e * kOut);
        ++n_rounds;
    }
    // ---- the fitness pass: every item at its final pose, converged or not -------------------------------------------------------------
    std::vector<double> fit;
    if (fitness) {
        int g = 0;
        for (int k = 0; k < n_items; ++k) { entry(k, I[k].lm.res.T, h_work + k); h_start[k] = g; g += I[k].nb; }
        h_start[n_items] = g;
        HIPCHK(c, upload(n_items));
        ctx_prof_mark(c, 1);
        k_fgicp_fitness_batch<<<g, 64, 0, st>>>(d_work, d_start, n_items, d_src, c->fgb_M.as<double>(), c->fgb_part.as<double>());
        ctx_prof_mark(c, 0);
        k_fgicp_total_batch<1><<<n_items, 64, 0, st>>>(c->fgb_part.as<double>(), d_start, c->fgb_out.as<double>());
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->fgb_host_out.p, c->fgb_out.p, sizeof(double) * (size_t)n_items, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        fit.assign(c->fgb_host_out.as<double>(), c->fgb_host_out.as<double>() + n_items);
        for (int k = 0; k < n_items; ++k) fit[k] /= (double)S[I[k].src].m;
    } else {
        HIPCHK(c, hipStreamSynchronize(st));                       // (a batch whose items all end at once has made no round)
    }
    ctx_prof_collect(c);
    // ---- nothing can fail any more: the results, and the winner as subMapOptmizationNode.cpp:2834-2840 picks it -------------------------
    int best = -1;
    double best_score = DBL_MAX;
    for (int k = 0; k < n_items; ++k) {
        const LmResult& lr = I[k].lm.res;
        lisreg_fgicp_result* res = results + k;
        memcpy(res->final_transform, lr.T, sizeof lr.T);
        res->converged = lr.converged; res->iters = lr.iters; res->n_evals = lr.n_evals; res->n_rejected = lr.n_rejected;
        res->n_pairs_last = lr.n_pairs_last; res->error = lr.error; res->lambda = lr.lambda;
        if (!fitness) continue;
        fitness[k] = fit[k];
        if (lr.converged == 0 || fit[k] > best_score) continue;
        best_score = fit[k];
        best = k;
    }
    if (info) *info = lisreg_fgicp_batch_info{ best, n_rounds, n_staged, 0 };
    return LISREG_OK;
}
