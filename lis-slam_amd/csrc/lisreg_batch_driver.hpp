// lisreg_batch_driver.hpp — what the four batch verifiers share on the host (lisreg_fgicp_batch.hip, DESIGN.md §7m,
// lisreg_vgicp_batch.hip, §7n, lisreg_ndt_batch.hip, §7o, and lisreg_gicp_batch.hip, §7r): the refusals, the staging of every named
// source, the work table of a round and its upload, the lockstep rounds of the items' resumable loops (the Levenberg-Marquardt stepper of
// lisreg_lm_stepper.hpp for the fast_gicp family, the Newton / More-Thuente stepper of lisreg_ndt_stepper.hpp for NDT, the outer loop
// of lisreg_gicp_stepper.hpp for PCL's GICP), the fitness pass, the `best` rule and the copy-out.  A family F (a struct of static
// members, no virtual call) supplies
//   kWho, Params / ItemC / Result / Info (its types of include/lisreg.h), Target (what a slot holds), Work (one entry of a round's table);
//   kRec: the doubles of one evaluation's record (29 for the fast_gicp family and NDT, 74 for GICP's moments);
//   bufs(c): its BatchBufs;  check_params(c, P);  find_target(c, slot, P, &T);
//   Stepper: one item's loop (start / finished / req_hessian / feed / res);  start(stepper, target, guess, P, n_records);
//   ensure_sources(B, records): the batch's source buffers for that many records;
//   stage_source(c, who, P, cloud, n, stride, fmt, B, off, want_finite, &m, &n_finite): one named source into the batch's buffers at `off`;
//   m = the lanes of one evaluation of it (the finite points of the fast_gicp family, the records of NDT), n_finite = the points the
//   fitness mean divides by (computed only if want_finite where that costs anything);
//   ensure_lanes(c, lanes): the storage its items own per (item, lane), if any;
//   fill(target, P, stepper, src_off, lane_off, m, Work*): one entry for the stepper's request;  fit_view(target): the grid the fitness
//   search reads;  fit_pose(res): the pose it runs at;  result_to(res, Result*);
//   launch_round(c, P, BatchRound<Work>): the evaluations of a round into r.part, with their profiling marks (the driver adds the totals
//   and closes the interval);  kFitnessTotalsApart: the fitness pass's totals are an interval of their own.
// One source for the four units, like lisreg_batch_rounds.hpp.  Not installed.
#pragma once
#include "lisreg_batch_rounds.hpp"
#include "lisreg_lm_stepper.hpp"

#include <cfloat>
#include <climits>
#include <vector>

namespace lisreg {
namespace {

// A round as its family's launches see it.  The entries sit in one array, the linearising ones first: [0, n_lin) of ne.  start[e] is
// the first workgroup of entry e over the whole round (start[ne] = g, their number; start[n_lin] = g_lin), so a workgroup's number is
// also the number of its partial record
template <class Work>
struct BatchRound {
    const Work*   work;
    const int*    start;
    const float4* src;     // the batch's point / covariance buffers
    const double* cov;
    double*       part;
    int           n_lin, ne, g_lin, g;
    hipStream_t   st;
};

// A source staged as the distributions of its finite points (points and covariances, one lane per finite point), for every family
// whose lanes read them: the fast_gicp kind and PCL's GICP.  epsilon: the family's regularisation of a covariance (plane_epsilon,
// gicp_epsilon)
struct DistributionSources {
    static hipError_t ensure_sources(BatchBufs& B, size_t records)
    {
        const hipError_t e = B.src.ensure(sizeof(float4) * records);
        return e != hipSuccess ? e : B.cov.ensure(sizeof(double) * 6 * records);
    }
    static int stage_distributions(lisreg_ctx* c, const char* who, int k_correspondences, double epsilon, const void* cloud, int n, int stride, int fmt,
                                   BatchBufs& B, long long off, int* m_out, int* n_finite)
    {
        hipStream_t st = c->stream;
        const float4* raw = nullptr;
        int rc = stage_records(c, cloud, n, stride, fmt, c->vg_raw, &raw);
        if (rc) return rc;
        float bb[6];
        int m = 0;
        rc = vg_distributions(c, who, raw, n, k_correspondences, epsilon, 0.f, bb, &m, nullptr, nullptr);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(B.src.as<float4>() + off, c->vg_pts.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipMemcpyAsync(B.cov.as<double>() + 6 * off, c->vg_cov.p, sizeof(double) * 6 * (size_t)m, hipMemcpyDeviceToDevice, st));
        *m_out = *n_finite = m;
        return LISREG_OK;
    }
};

// What the two families of the fast_gicp kind supply alike: the Levenberg-Marquardt stepper started from the guess matrix, a source
// staged as its distributions, the pose and the result of an LmResult
template <class Params, class Result>
struct LmBatchFamily : DistributionSources {
    using Stepper = vgicp_host::LmStepper;
    static constexpr int kRec = vgicp_host::kOut;

    template <class Target>
    static void start(Stepper& lm, const Target&, const float* guess, const Params& P, int)
    {
        double T0[16];
        vgicp_host::guess_to_T0(guess, T0);
        lm.start(T0, vgicp_host::lm_params_of(P));
    }
    static int stage_source(lisreg_ctx* c, const char* who, const Params& P, const void* cloud, int n, int stride, int fmt, BatchBufs& B, long long off,
                            bool, int* m_out, int* n_finite)
    {
        return stage_distributions(c, who, P.k_correspondences, P.plane_epsilon, cloud, n, stride, fmt, B, off, m_out, n_finite);
    }
    static FgPose fit_pose(const vgicp_host::LmResult& lr) { return vgicp_host::pose_of<FgPose>(lr.T); }
    static void result_to(const vgicp_host::LmResult& lr, Result* res) { vgicp_host::lm_result_to(lr, res); }
};

template <class F>
int batch_align(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt, const typename F::ItemC* items,
                int n_items, const typename F::Params* P, typename F::Result* results, double* fitness, typename F::Info* info)
{
    using namespace vgicp_host;
    using Work = typename F::Work;
    constexpr int kOut = F::kRec;                                  // the doubles of one record: the family's, not vgicp_host's
    struct Source { bool used = false; int m = 0, n_finite = 0; long long off = 0; };
    struct Item { typename F::Stepper lm; const typename F::Target* T = nullptr; long long lane_off = 0; int src = 0, nb = 0; };
    constexpr const char* kWho = F::kWho;
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || n_sources < 0) return bad(c, std::string(kWho) + ": n_items < 0 or n_sources < 0");
    if (info) *info = typename F::Info{ -1, 0, 0, 0 };
    if (n_items == 0) return LISREG_OK;
    // ---- every refusal that needs no device, for the whole batch ----------------------------------------------------------------
    if (!items || !results || !sources || !n) return bad(c, std::string(kWho) + ": NULL items / results / sources / n");
    int rc = F::check_params(c, P);
    if (rc) return rc;
    std::vector<Source> S((size_t)n_sources);
    std::vector<Item>   I((size_t)n_items);
    for (int k = 0; k < n_items; ++k) {
        if (items[k].source < 0 || items[k].source >= n_sources) return bad(c, std::string(kWho) + ": an item's source index is out of range");
        typename F::Target* T = nullptr;
        rc = F::find_target(c, items[k].slot, P, &T);
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
    // ---- the sources, once each; a cloud the staging refuses (for the fast_gicp family: too few finite points, an infinite coordinate)
    // ends the call before any alignment work, with `results` untouched.  The context's scratch is overwritten by the next source: the
    // batch keeps copies
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    BatchBufs& B = F::bufs(c);
    HIPCHK(c, F::ensure_sources(B, cap));
    long long off = 0;
    int n_staged = 0;
    for (int s = 0; s < n_sources; ++s) {
        if (!S[s].used) continue;
        int m = 0, n_finite = 0;
        rc = F::stage_source(c, kWho, *P, sources[s], n[s], stride, fmt, B, off, fitness != nullptr, &m, &n_finite);
        if (rc) return rc;
        S[s].m = m; S[s].n_finite = n_finite; S[s].off = off;
        off += m;
        ++n_staged;
    }
    // ---- the round's storage: what the items own, one partial record per workgroup, one total per item; the work table: the entries
    // (of the larger of the two kinds), then the n_entries + 1 workgroup starts --------------------------------------------------------
    long long lanes = 0, wgs = 0;
    for (int k = 0; k < n_items; ++k) {
        I[k].lane_off = lanes; I[k].nb = (S[I[k].src].m + 63) / 64;
        lanes += S[I[k].src].m; wgs += I[k].nb;
    }
    if (wgs > (long long)INT_MAX / kOut) return bad(c, std::string(kWho) + ": the batch is too large (items x source points)");
    constexpr size_t kEntryBytes = sizeof(Work) > sizeof(FgFitWork) ? sizeof(Work) : sizeof(FgFitWork);
    const size_t starts_offset = kEntryBytes * (size_t)n_items, table_bytes = starts_offset + sizeof(int) * ((size_t)n_items + 1);
    HIPCHK(c, F::ensure_lanes(c, lanes));
    HIPCHK(c, B.part.ensure(sizeof(double) * kOut * (size_t)wgs));
    HIPCHK(c, B.out.ensure(sizeof(double) * kOut * (size_t)n_items));
    HIPCHK(c, B.work.ensure(table_bytes));
    HIPCHK(c, B.host_work.ensure(table_bytes, table_bytes + table_bytes / 2));
    HIPCHK(c, B.host_out.ensure(sizeof(double) * kOut * (size_t)n_items, sizeof(double) * kOut * ((size_t)n_items + (size_t)n_items / 2)));
    int* const     h_start = reinterpret_cast<int*>(static_cast<char*>(B.host_work.p) + starts_offset);
    const int*     d_start = reinterpret_cast<const int*>(static_cast<const char*>(B.work.p) + starts_offset);
    const float4*  d_src = B.src.as<float4>();
    double* const  d_part = B.part.as<double>();
    // the table of a round goes up in two copies: the entries and, behind them, the starts (the gap between them is not read)
    auto upload = [&](int ne, size_t entry_bytes) -> hipError_t {
        hipError_t e = hipMemcpyAsync(B.work.p, B.host_work.p, entry_bytes * (size_t)ne, hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(const_cast<int*>(d_start), h_start, sizeof(int) * ((size_t)ne + 1), hipMemcpyHostToDevice, st);
    };
    // ---- the alignment phase, in lockstep rounds: every unfinished item has one request outstanding ----------------------------------
    for (int k = 0; k < n_items; ++k) F::start(I[k].lm, *I[k].T, items[k].guess, *P, n[I[k].src]);
    Work* const h_work = B.host_work.as<Work>();
    std::vector<int> order((size_t)n_items);
    int n_rounds = 0;
    for (;;) {
        int ne = 0, n_lin = 0;
        for (int k = 0; k < n_items; ++k) if (!I[k].lm.finished() && I[k].lm.req_hessian) order[ne++] = k;
        n_lin = ne;
        for (int k = 0; k < n_items; ++k) if (!I[k].lm.finished() && !I[k].lm.req_hessian) order[ne++] = k;
        if (!ne) break;
        int g = 0;
        for (int e = 0; e < ne; ++e) {
            const Item& it = I[order[e]];
            F::fill(*it.T, *P, it.lm, S[it.src].off, it.lane_off, S[it.src].m, h_work + e);
            h_start[e] = g; g += it.nb;
        }
        h_start[ne] = g;
        HIPCHK(c, upload(ne, sizeof(Work)));
        F::launch_round(c, *P, BatchRound<Work>{ B.work.as<Work>(), d_start, d_src, B.cov.as<double>(), d_part, n_lin, ne,
                                                 h_start[n_lin], g, st });
        k_fgicp_total_batch<kOut><<<ne, 64, 0, st>>>(d_part, d_start, B.out.as<double>());
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(B.host_out.p, B.out.p, sizeof(double) * kOut * (size_t)ne, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        const double* out = B.host_out.as<double>();
        for (int e = 0; e < ne; ++e) I[order[e]].lm.feed(out + (size_t)e * kOut);
        ++n_rounds;
    }
    // ---- the fitness pass: every item at its final pose, converged or not -------------------------------------------------------------
    std::vector<double> fit;
    if (fitness) {
        FgFitWork* const h_fit = B.host_work.as<FgFitWork>();
        int g = 0;
        for (int k = 0; k < n_items; ++k) {
            FgFitWork* w = h_fit + k;
            w->A = F::fit_view(*I[k].T);
            w->P = F::fit_pose(I[k].lm.res);
            w->src_off = S[I[k].src].off; w->n = S[I[k].src].m; w->reserved = 0;
            h_start[k] = g; g += I[k].nb;
        }
        h_start[n_items] = g;
        HIPCHK(c, upload(n_items, sizeof(FgFitWork)));
        ctx_prof_mark(c, 1);                                       // lisreg_get_timing: "solve" = the fitness search, one interval
        k_fgicp_fitness_batch<<<g, 64, 0, st>>>(B.work.as<FgFitWork>(), d_start, n_items, d_src, d_part);
        if (F::kFitnessTotalsApart) ctx_prof_mark(c, 0);
        k_fgicp_total_batch<1><<<n_items, 64, 0, st>>>(d_part, d_start, B.out.as<double>());
        ctx_prof_mark(c, -1);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(B.host_out.p, B.out.p, sizeof(double) * (size_t)n_items, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        fit.assign(B.host_out.as<double>(), B.host_out.as<double>() + n_items);
        for (int k = 0; k < n_items; ++k) fit[k] /= (double)S[I[k].src].n_finite;
    } else {
        HIPCHK(c, hipStreamSynchronize(st));                       // (a batch whose items all end at once has made no round)
    }
    ctx_prof_collect(c);
    // ---- nothing can fail any more: the results, and the winner as subMapOptmizationNode.cpp:2834-2840 picks it -------------------------
    int best = -1;
    double best_score = DBL_MAX;
    for (int k = 0; k < n_items; ++k) {
        const auto& lr = I[k].lm.res;
        F::result_to(lr, results + k);
        if (!fitness) continue;
        fitness[k] = fit[k];
        if (lr.converged == 0 || fit[k] > best_score) continue;
        best_score = fit[k];
        best = k;
    }
    if (info) *info = typename F::Info{ best, n_rounds, n_staged, 0 };
    return LISREG_OK;
}

}  // namespace
}  // namespace lisreg
