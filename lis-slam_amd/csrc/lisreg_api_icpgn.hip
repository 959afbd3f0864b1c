// lisreg_api_icpgn.hip — lisreg_icp_gn_match_batch: the candidate loop of detectLoopClosureForSubMapICP
// (src/node/subMapOptmizationNode.cpp:2496-2621: SetTargetCloud / Match / GetFitnessScore / HasConverged per candidate of a static
// OptimizedICPGN, then the `best` rule) as one call.  OptimizedICPGN has no convergence test, so every item runs exactly max_iterations
// iterations: the whole batch is max_iterations x (correspondence launch per lane class, one solve launch) + the fitness launches on one
// stream, with nothing for the host to decide in between.  Kernels: lisreg_nn1.hip (k_icpgn_assoc_b, k_icpgn_solve_b, k_icpgn_fit_b,
// k_icpgn_fit_reduce_b — the per-lane body and the step of the single call).  DESIGN.md section 7s.
#include "lisreg_ctx.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

using namespace lisreg;

namespace {

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

// :2551-2558 — `if (score > bestScore) continue; bestScore = score; best = k;` over the float scores compared in double
int icpgn_best(const lisreg_icpgn_result* r, int n)
{
    double best_score = DBL_MAX;
    int best = -1;
    for (int k = 0; k < n; ++k) {
        const double s = (double)r[k].fitness;
        if (s > best_score) continue;
        best_score = s; best = k;
    }
    return best;
}

}  // namespace

extern "C" {

int lisreg_icp_gn_match_batch(lisreg_ctx* c, const void* const* sources, const int* n, int n_sources, int stride, int fmt,
                              const lisreg_icpgn_item* items, int n_items, unsigned max_iterations, float max_correspond_distance,
                              lisreg_icpgn_result* results, lisreg_icpgn_batch_info* info)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0) return bad(c, "icp_gn_match_batch: n_items < 0");
    if (n_items > 0 && (!items || !results || !sources || !n)) return bad(c, "icp_gn_match_batch: NULL items / results / sources / n");
    if (max_iterations > 100000u) return bad(c, "icp_gn_match_batch: max_iterations out of range");
    if (n_items == 0) {
        if (info) *info = lisreg_icpgn_batch_info{ -1, 0, 0, 0 };
        return LISREG_OK;
    }
    // ---- what the single call would refuse, for every item, before anything is staged ------------------------------------------------
    std::vector<char> used((size_t)std::max(n_sources, 1), 0);
    for (int k = 0; k < n_items; ++k) {
        if (items[k].source < 0 || items[k].source >= n_sources) return bad(c, "icp_gn_match_batch: an item's source index is out of range");
        used[(size_t)items[k].source] = 1;
    }
    for (int k = 0; k < n_items; ++k)
        if (items[k].slot < 0 || c->maps.count(items[k].slot) == 0 || !c->maps[items[k].slot].valid)
            return ctx_fail(c, LISREG_ERR_NO_TARGET, "icp_gn_match_batch: an item names a slot without a map index (SetTargetCloud)");
    int n_staged = 0;
    size_t host_points = 0;
    for (int s = 0; s < n_sources; ++s) {
        if (!used[(size_t)s]) continue;
        const int rc = check_cloud(c, "icp_gn_match_batch", sources[s], n[s], stride, fmt, kFmtPackable, true);
        if (rc) return rc;
        ++n_staged;
        if (fmt != LISREG_FMT_DEVICE) host_points += (size_t)n[s];
    }
    // ---- the table: items by lane class (each keeps the lanes per query of its own size), blocks per class, rows over the batch ---------
    std::vector<int> order; order.reserve((size_t)n_items);
    IcpGnClasses cls;
    long long rows = 0, points = 0, cls_blocks[3] = { 0, 0, 0 };
    for (int cl = 0; cl < 3; ++cl) {
        cls.first[cl] = (int)order.size();
        for (int k = 0; k < n_items; ++k) {
            const int q = icp_lanes(n[items[k].source]);
            if ((q == 1 ? 0 : (q == 4 ? 1 : 2)) != cl) continue;
            order.push_back(k);
            cls_blocks[cl] += icp_blocks(n[items[k].source]);
        }
        rows += cls_blocks[cl];
    }
    cls.first[3] = (int)order.size();
    for (int k = 0; k < n_items; ++k) points += n[items[k].source];
    if (rows > 0x7fffffffLL || points > 0x7fffffffLL)
        return bad(c, "icp_gn_match_batch: the batch's workgroups / partial rows / source points over all items do not fit 32-bit counts");
    for (int cl = 0; cl < 3; ++cl) cls.blocks[cl] = (int)cls_blocks[cl];

    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // one pinned block [states | table | packed host sources] and its device twin, one upload
    const size_t o_tab = align16(sizeof(IcpState) * (size_t)n_items), o_src = o_tab + align16(sizeof(IcpGnItem) * (size_t)n_items);
    const size_t bytes = o_src + sizeof(lisreg_dpoint) * host_points;
    HIPCHK(c, c->gnb_host.ensure(bytes, bytes + bytes / 4));
    HIPCHK(c, c->gnb_tab.ensure(bytes));
    HIPCHK(c, c->gnb_part.ensure(sizeof(double) * 22 * (size_t)std::max<long long>(rows, 1)));
    HIPCHK(c, c->gnb_nn.ensure(sizeof(int) * (size_t)std::max<long long>(points, 1)));
    char* hb = c->gnb_host.as<char>();
    char* db = c->gnb_tab.as<char>();
    IcpState* hs = reinterpret_cast<IcpState*>(hb);
    IcpGnItem* hi = reinterpret_cast<IcpGnItem*>(hb + o_tab);
    IcpState* sd = reinterpret_cast<IcpState*>(db);
    const IcpGnItem* di = reinterpret_cast<const IcpGnItem*>(db + o_tab);
    std::vector<const float4*> src_dev((size_t)n_sources, nullptr);
    {
        size_t off = 0;
        for (int s = 0; s < n_sources; ++s) {
            if (!used[(size_t)s]) continue;
            if (fmt == LISREG_FMT_DEVICE) { src_dev[(size_t)s] = static_cast<const float4*>(sources[s]); continue; }
            pack_cloud(sources[s], n[s], stride, fmt, reinterpret_cast<lisreg_dpoint*>(hb + o_src) + off);
            src_dev[(size_t)s] = reinterpret_cast<const float4*>(db + o_src) + off;
            off += (size_t)n[s];
        }
    }
    memset(hs, 0, sizeof(IcpState) * (size_t)n_items);
    for (int k = 0; k < n_items; ++k)
        for (int j = 0; j < 16; ++j) hs[k].F[j] = items[k].predict_pose ? items[k].predict_pose[j] : ((j % 5 == 0) ? 1.f : 0.f);
    {
        int row = 0, nn_off = 0;
        for (int cl = 0; cl < 3; ++cl) {
            int blk = 0;
            for (int e = cls.first[cl]; e < cls.first[cl + 1]; ++e) {
                const int k = order[(size_t)e], s = items[k].source;
                IcpGnItem& d = hi[e];
                d.src = src_dev[(size_t)s]; d.nn = c->gnb_nn.as<int>() + nn_off; d.grid = c->maps[items[k].slot].g_dev.as<GridIndex>();
                d.n = n[s]; d.blk0 = blk; d.nblk = icp_blocks(n[s]); d.row0 = row; d.state = k; d.pad_ = 0;
                blk += d.nblk; row += d.nblk; nn_off += n[s];
            }
        }
    }
    HIPCHK(c, hipMemcpyAsync(db, hb, bytes, hipMemcpyHostToDevice, st));
    // registration.cpp:50 compares the SQUARED distance with max_correspond_distance itself
    const float cap2 = max_correspond_distance >= 0.f ? std::min(max_correspond_distance, 3.0e38f) : -1.f;
    double* part = c->gnb_part.as<double>();
    int n_syncs = 0;
    const bool iterate = cap2 >= 0.f && max_iterations > 0;
    if (iterate)
        for (unsigned it = 0; it < max_iterations; ++it) {
            launch_icpgn_batch_iteration(di, n_items, cls, sd, cap2, it == 0, part, st);
            if ((it & 63u) == 63u) { HIPCHK(c, hipGetLastError()); HIPCHK(c, hipStreamSynchronize(st)); ++n_syncs; }      // keep the queue bounded for long runs
        }
    HIPCHK(c, hipGetLastError());
    launch_icpgn_batch_fitness(di, n_items, cls, sd, iterate, part, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(hs, sd, sizeof(IcpState) * (size_t)n_items, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st)); ++n_syncs;
    for (int k = 0; k < n_items; ++k) {
        const IcpState& h = hs[k];
        lisreg_icpgn_result* res = &results[k];
        memcpy(res->final_transform, h.F, sizeof h.F);
        res->steps_applied = h.iters; res->n_corr_last = h.n_corr; res->reserved = 0;
        res->fitness = h.fit_n > 0 ? (float)(h.fit_sum / (double)h.fit_n) : FLT_MAX;
    }
    if (info) *info = lisreg_icpgn_batch_info{ icpgn_best(results, n_items), n_staged, n_syncs, 0 };
    return LISREG_OK;
}

}  // extern "C"
