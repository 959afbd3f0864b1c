// lisreg_api.hip — C-ABI host layer of liblisreg.so (declared in include/lisreg.h): context lifecycle, registration targets and their
// search indices, options, diagnostics, test hooks, profiling.  Batch prepare / run / fetch / align are in lisreg_api_batch.hip, the
// other subsystems have a unit each (lisreg_api_{cloud,features,feed,map,localmap,comm}.hip); what they all share is in lisreg_api_ctx.hip.
//
// Creates the seam the reference lacks: each entry point replaces a piece of
// scan2SubMapOptimization() — /root/reference/src/node/odomEstimationNode.cpp:596-626 and the copies at
// src/node/subMapOptmizationNode.cpp:1509-1541, 4485-4540.  A
// context is single-threaded and owns its stream, so several contexts run concurrently (callers #2/#3).
// There is deliberately NO CPU fallback: without a HIP device every compute entry point fails with
// LISREG_ERR_HIP.
#include "lisreg_batch_plan.hpp"

#include <algorithm>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace lisreg;

DevParams lisreg::make_dev_params(const lisreg_params& p)
{
    DevParams d;
    memset(&d, 0, sizeof d);
    d.tau = p.knn_sq_thresh; d.line_ratio = p.line_ratio; d.plane_tol = p.plane_tol; d.accept_s = p.accept_s;
    d.conv_deg = p.conv_deg; d.conv_cm = p.conv_cm; d.eig_thresh = p.eig_thresh;
    d.min_corr = p.min_corr; d.use_label = p.use_label_weight; d.emulate_shadow = p.emulate_matp_shadow;
    d.skip_empty = p.skip_empty_target; d.fixed_iters = p.fixed_iters;
    d.bound = p.fixed_iters > 0 ? p.fixed_iters : p.max_iters;
    d.edge_min = p.edge_min; d.surf_min = p.surf_min; d.use_imu = p.use_imu_blend;
    d.imu_w = p.imu_rpy_weight; d.rot_tol = p.rotation_tol; d.z_tol = p.z_tol;
    for (int i = 0; i < 32; ++i) d.wtab[i] = (float)(2.0 - (double)p.label_score[i]);   // subMapOptmizationNode.cpp:1671
    return d;
}

namespace {

constexpr int kCrowGridMargin = 2;

int build_target_kind(lisreg_ctx* c, Target& t, int k)
{
    const int n = t.n[k];
    HIPCHK(c, t.cell_start[k].ensure(sizeof(int) * ((size_t)t.n_cells[k] + 2)));
    HIPCHK(c, t.sorted[k].ensure(sizeof(float4) * (size_t)std::max(n, 1)));
    int rc = ensure_sort_scratch(c, (size_t)std::max(n, 1), (size_t)t.n_cells[k]);
    if (rc) return rc;
    t.g[k].pts = t.sorted[k].as<float4>();
    t.g[k].cell_start = t.cell_start[k].as<int>();
    launch_build_target(t.raw_ptr[k], n, t.g[k], t.sorted[k].as<float4>(), t.cell_start[k].as<int>(), t.n_cells[k],
                        sort_buffers(c), c->stream);
    HIPCHK(c, hipGetLastError());
    return LISREG_OK;
}

}  // namespace

// search_mode 3: neighbour lists of target kind k (the index itself must already be enqueued on the stream)
int lisreg::ensure_graph(lisreg_ctx* c, Target& t, int k, bool launch)
{
    const size_t n = (size_t)std::max(t.n[k], 1);
    HIPCHK(c, t.nbr[k].ensure(sizeof(float4) * kGraphK * n));
    HIPCHK(c, t.nbr_meta[k].ensure(sizeof(float2) * n));
    t.g[k].nbr = t.nbr[k].as<float4>();
    t.g[k].nbr_meta = t.nbr_meta[k].as<float2>();
    if (launch && !t.graph_valid[k]) {
        launch_build_graph_one(t.g[k], c->stream);
        HIPCHK(c, hipGetLastError());
        t.graph_valid[k] = true;
    }
    return LISREG_OK;
}

// search_mode 5: cell rows of target kind k (the index itself must already be enqueued on the stream).  The row count depends on the
// data, so the first build of a target classifies its cells, reads the count back (one host round trip, at set / prepare time) and sizes the
// buffers; rebuilds inside a run (rebuild_targets_each_run) reuse that capacity — a cell that does not fit gets no row and its queries walk.
// "row_reach" = 2, `near`: the target has a point within P cells of the cell (Chebyshev, like the 5 x 5 x 5 count).  P is half a metre in
// cells — in metres, like the dilation: the queries' path from their initial pose to the surface does not shrink with the cells.
// P = 1 (cells of 0.5 m and more) is the 3 x 3 x 3 count the classification makes for it; P = 2 (smaller cells: never under 0.25 m,
// make_grid) IS the 5 x 5 x 5 count every cell with rows has anyway, so such grids keep the rows of "row_reach" = 1.
static int crow_near_cells(float cell) { return std::max(1, (int)std::ceil(0.5f / cell - 1e-3f)); }

lisreg::CrowBuffers lisreg::crow_buffers(Target& t, int k, bool with_reach, bool near_only)
{
    lisreg::CrowBuffers cb;
    cb.need = t.crow_need[k].as<int>(); cb.omask = t.crow_omask[k].as<int>(); cb.scan = t.crow_scan[k].as<int>(); cb.scan_tmp = t.crow_scan_tmp[k].as<int>();
    cb.cap_rows = t.crow_cap[k];
    cb.reach = with_reach && t.g[k].qmark ? t.crow_reach[k].as<unsigned>() : nullptr;      // (never for the classification that SIZES the row buffers)
    const int P = crow_near_cells(t.g[k].cell);
    assert(P <= 2);
    cb.qmark = cb.reach && near_only && P == 1 ? t.g[k].qmark : nullptr;
    return cb;
}

// option "row_reach": mark and reach words of target kind k (one bit per grid cell, lisreg_internal.hpp) — made when a batch that rebuilds its
// targets takes the cell rows; the pointer travels in the GridIndex (the device table is refreshed when it changes)
int lisreg::ensure_reach(lisreg_ctx* c, Target& t, int k, bool on)
{
    unsigned* want = nullptr;
    int w = 0;
    if (on && t.n[k] > 0 && t.g[k].crow_tab) {
        w = (t.g[k].nz + 31) / 32;
        const size_t words = (size_t)t.g[k].nx * (size_t)t.g[k].ny * (size_t)w;
        HIPCHK(c, t.crow_qmark[k].ensure(sizeof(unsigned) * (words + 8)));
        HIPCHK(c, t.crow_reach[k].ensure(sizeof(unsigned) * (words + 8)));
        want = t.crow_qmark[k].as<unsigned>();
    }
    if (t.g[k].qmark != want || t.g[k].qmark_w != w) { t.g[k].qmark = want; t.g[k].qmark_w = w; c->grids_dirty = true; }
    return LISREG_OK;
}

// may_decline (front-end chosen by auto): a target whose rows would not fit "cell_rows_max_mb" is left without them (crow_too_big) and the
// batch takes another front-end; with search_mode 5 set by the caller the buffers are capped there instead and the cells past them walk.
// rows_left (auto): rows the batch may still take under "cell_rows_max_mb" — the bound is on the batch's targets together, not on each
int lisreg::ensure_crows(lisreg_ctx* c, Target& t, int k, bool may_decline, long long* rows_left)
{
    if (t.crow_valid[k] && t.g[k].crow_tab) { if (rows_left) *rows_left -= t.crow_cap[k]; return LISREG_OK; }
    if (may_decline && t.crow_too_big[k]) return LISREG_OK;       // found too big before (the note is cleared when the target is set again)
    t.crow_too_big[k] = false;
    if (t.n[k] > 0 && t.grid_margin[k] < kCrowGridMargin) {
        // a wall that bounds the cloud has half of a not-yet-registered scan's points OUTSIDE the cloud's bounding box: the grid is
        // re-made two cells wider on every side (empty cells: four bytes of table each) and the index rebuilt on it, once per target
        t.grid_margin[k] = kCrowGridMargin;
        make_grid(t.bbox[k], t.n[k], &t.g[k], &t.n_cells[k], t.grid_margin[k]);
        int rc = build_target_kind(c, t, k);
        if (rc) return rc;
        t.graph_valid[k] = false;
        t.g[k].nbr = nullptr; t.g[k].nbr_meta = nullptr;
        // the geometry (origin, dims) and possibly the cell table's address have changed: a batch prepared against the old grid holds stale
        // copies of both (the device GridIndex table, the rebuild table h_tsegs) — it has to be prepared again (lisreg_batch_prepare calls
        // this before it reads any geometry; lisreg_get_target_cell_rows on a slot a prepared batch uses lands here too)
        c->batch.live.prepared = false;
        c->grids_dirty = true;
    }
    const size_t nc = (size_t)std::max(t.n_cells[k], 1);
    HIPCHK(c, t.crow_need[k].ensure(sizeof(int) * (nc + 8)));
    { const size_t before = t.crow_omask[k].cap; HIPCHK(c, t.crow_omask[k].ensure(sizeof(int) * (nc + 8))); if (t.crow_omask[k].cap != before) t.omask_zero[k] = 0; }     // (a new allocation: nothing known)
    HIPCHK(c, t.crow_scan[k].ensure(sizeof(int) * (nc + 8)));
    HIPCHK(c, t.crow_scan_tmp[k].ensure(sizeof(int) * (nc / 2048 + 8)));
    HIPCHK(c, t.crow_tab[k].ensure(sizeof(int) * (nc + 8)));
    t.g[k].crow_tab = t.crow_tab[k].as<int>();
    int rows = 0;
    if (t.n[k] > 0) {
        launch_crow_classify(t.g[k], t.n_cells[k], crow_buffers(t, k), c->stream, &t.omask_zero[k]);
        HIPCHK(c, hipMemcpyAsync(&rows, t.crow_scan[k].as<int>() + t.n_cells[k], sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    t.crow_cap[k] = std::max(rows, 1);
    {
        // (a cloud scattered through space instead of lying on surfaces — vegetation, rain — asks for up to 125 centre rows per point)
        long long budget = crow_row_budget(c->opt.cell_rows_max_mb);
        if (rows_left) budget = std::min(budget, std::max(*rows_left, 0LL));
        if ((long long)rows > budget) {
            if (may_decline) { t.crow_too_big[k] = true; t.g[k].crow_tab = nullptr; return LISREG_OK; }
            t.crow_cap[k] = (int)std::max(1LL, budget);
        }
    }
    if (const char* e = getenv("LISREG_CROW_CAP_PERCENT"))      // tests: under-size the row buffers (cells past the capacity get no row: their queries walk)
        t.crow_cap[k] = std::max(1, (int)((long long)t.crow_cap[k] * std::max(0, atoi(e)) / 100));
    if (getenv("LISREG_CROW_DEBUG")) fprintf(stderr, "[lisreg] cell rows of kind %d: %d rows for %d points in %d cells (%d x %d x %d of %.3f m)\n", k, rows, t.n[k], t.n_cells[k], t.g[k].nx, t.g[k].ny, t.g[k].nz, t.g[k].cell);
    {
        // (auto: a refused allocation — many own-target items, each under the bound — is a reason to take another front-end, not an error)
        const hipError_t e1 = t.crow[k].ensure(sizeof(float4) * kGraphK * (size_t)t.crow_cap[k]);
        const hipError_t e2 = e1 == hipSuccess ? t.crow_meta[k].ensure(sizeof(float2) * (size_t)t.crow_cap[k]) : e1;
        if (e2 != hipSuccess) {
            (void)hipGetLastError();
            t.crow[k].release(); t.crow_meta[k].release();      // (the half that was granted goes back now: the target lives on without rows)
            if (may_decline) { t.crow_too_big[k] = true; t.g[k].crow_tab = nullptr; return LISREG_OK; }
            return ctx_fail(c, LISREG_ERR_HIP, std::string("cell rows: ") + hipGetErrorString(e2));
        }
    }
    if (rows_left) *rows_left -= t.crow_cap[k];
    t.crow_chosen[k] = true;
    t.g[k].crow = t.crow[k].as<float4>();
    t.g[k].crow_meta = t.crow_meta[k].as<float2>();
    if (t.n[k] > 0) launch_crow_build(t.g[k], t.n_cells[k], crow_buffers(t, k), c->stream, &t.omask_zero[k]);
    else HIPCHK(c, hipMemsetAsync(t.crow_tab[k].p, 0xff, sizeof(int) * nc, c->stream));
    HIPCHK(c, hipGetLastError());
    t.crow_valid[k] = true;
    return LISREG_OK;
}

int lisreg::upload_grids(lisreg_ctx* c)
{
    std::vector<GridIndex> h(c->targets.size() * 2);
    for (size_t s = 0; s < c->targets.size(); ++s)
        for (int k = 0; k < 2; ++k) {
            if (c->targets[s].valid) h[s * 2 + k] = c->targets[s].g[k];
            else memset(&h[s * 2 + k], 0, sizeof(GridIndex));
        }
    HIPCHK(c, c->grids_dev.ensure(sizeof(GridIndex) * std::max<size_t>(h.size(), 1)));
    const size_t bytes = sizeof(GridIndex) * h.size();
    // through a pinned buffer of the context, guarded by an event: the copy is asynchronous and the host goes on building the batch's
    // tables while the stream still works on the target index it has just been given (a frame loop sets a target per frame: waiting
    // here meant an idle device for the rest of lisreg_batch_prepare)
    if (bytes > c->grids_host.cap) {
        if (c->grids_done) (void)hipEventSynchronize(c->grids_done);
        if (c->grids_host.ensure(bytes, 2 * bytes + 1024) != hipSuccess) (void)hipGetLastError();
    }
    if (!c->grids_done) (void)c->grids_done.create(hipEventDisableTiming);
    if (bytes && c->grids_host.p && c->grids_done) {
        HIPCHK(c, hipEventSynchronize(c->grids_done));          // (recorded by the previous upload: long past)
        memcpy(c->grids_host.p, h.data(), bytes);
        HIPCHK(c, hipMemcpyAsync(c->grids_dev.p, c->grids_host.p, bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipEventRecord(c->grids_done, c->stream));
    } else if (bytes) {
        HIPCHK(c, hipMemcpyAsync(c->grids_dev.p, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));     // h is a local
    }
    c->grids_dirty = false;
    return LISREG_OK;
}

namespace {

// (sidx 1: the mark goes on the side stream — the second half of an interleaved run, run_impl; an interval runs from a mark to the next mark
//  on the SAME stream)
void prof_mark(lisreg_ctx* c, int kind_of_next_interval, int sidx = 0)
{
    if (!c->profiling) return;
    Event e;
    if (e.create(hipEventDefault) != hipSuccess) return;
    (void)hipEventRecord(e, sidx ? c->side_stream : c->stream);
    c->ev.push_back(std::move(e));
    c->ev_kind.push_back(kind_of_next_interval);
    c->ev_sidx.push_back(sidx);
}

void prof_collect(lisreg_ctx* c)
{
    for (int i = 0; i < 5; ++i) c->timing[i] = 0;
    const bool dump = getenv("LISREG_PROF_DUMP") != nullptr;
    for (size_t i = 0; i + 1 < c->ev.size(); ++i) {
        float ms = 0;
        size_t j = i + 1;
        while (j < c->ev.size() && c->ev_sidx[j] != c->ev_sidx[i]) ++j;          // the next mark on the same stream
        if (j >= c->ev.size()) continue;
        if (c->ev_kind[i] >= 0 && hipEventElapsedTime(&ms, c->ev[i], c->ev[j]) == hipSuccess) {
            if (dump) fprintf(stderr, "[lisreg prof] interval %zu kind %d: %.4f ms\n", i, c->ev_kind[i], ms);
            if (c->ev_kind[i] == 0) { c->timing[0] += ms; c->timing[1] += 1; }
            else if (c->ev_kind[i] == 1) { c->timing[2] += ms; c->timing[3] += 1; }
            else if (c->ev_kind[i] == 2) c->timing[4] += ms;
        }
    }
    c->ev.clear(); c->ev_kind.clear(); c->ev_sidx.clear();
}

}  // namespace

// HIP-event marks for the other translation units (lisreg_set_profiling / lisreg_get_timing)
void lisreg::ctx_prof_mark(lisreg_ctx* c, int kind_of_next_interval, int sidx) { prof_mark(c, kind_of_next_interval, sidx); }
void lisreg::ctx_prof_collect(lisreg_ctx* c) { if (!c->ev.empty()) prof_collect(c); }

// =============================================================================================================
// the context of this process that enqueued the last batch run (lisreg_ctx.hpp: batch_runner_alone)
static std::atomic<const lisreg_ctx*> g_last_batch_runner{ nullptr };
namespace lisreg {
bool batch_runner_alone(const lisreg_ctx* c)
{
    const lisreg_ctx* before = g_last_batch_runner.exchange(c);
    return before == nullptr || before == c;
}
}  // namespace lisreg

extern "C" {

int lisreg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int lisreg_create(int device, lisreg_ctx** out)
{
    if (!out) return bad(nullptr, "lisreg_create: out is NULL");
    *out = nullptr;
    int n = lisreg_device_count();
    if (n <= 0) return ctx_fail(nullptr, LISREG_ERR_HIP, "lisreg_create: no HIP device visible (liblisreg has no CPU fallback)");
    if (device < 0 || device >= n) return bad(nullptr, "lisreg_create: bad device index");
    lisreg_ctx* c = new (std::nothrow) lisreg_ctx();
    if (!c) return ctx_fail(nullptr, LISREG_ERR_NOMEM, "lisreg_create: out of host memory");
    c->device = device;
    if (hipSetDevice(device) != hipSuccess || c->own_stream.create(hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return ctx_fail(nullptr, LISREG_ERR_HIP, "lisreg_create: hipSetDevice/hipStreamCreate failed");
    }
    c->stream = c->own_stream;
    c->targets.resize(1);
    (void)c->done_host.ensure(sizeof(int), sizeof(int));     // (a failure is tolerated: runs then do not stop early)
    if (c->done_dev.ensure(sizeof(int)) != hipSuccess) { lisreg_destroy(c); return ctx_fail(nullptr, LISREG_ERR_HIP, "lisreg_create: hipMalloc failed"); }
    lisreg_default_params(LISREG_VARIANT_ODOM, &c->batch.params);
    *out = c;
    return LISREG_OK;
}

void lisreg_destroy(lisreg_ctx* c)
{
    if (!c) return;
    { const lisreg_ctx* self = c; g_last_batch_runner.compare_exchange_strong(self, nullptr); }
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    // everything the context owns goes with `delete c`, in no particular order; what has to be over BEFORE that is said here:
    // no stream of the context still runs work that reads or writes its buffers, and no packing thread still writes pinned staging
    if (c->side_stream) (void)hipStreamSynchronize(c->side_stream);
    if (c->grids_done) (void)hipEventSynchronize(c->grids_done);
    lisreg_comm_destroy(c);
    feeder_stop(c);
    delete c;
}

int lisreg_set_stream(lisreg_ctx* c, void* s)
{
    if (!c) return LISREG_ERR_ARG;
    (void)hipStreamSynchronize(c->stream);
    c->stream = s ? (hipStream_t)s : c->own_stream;
    return LISREG_OK;
}

void* lisreg_get_stream(const lisreg_ctx* c) { return c ? (void*)c->stream : nullptr; }

int lisreg_default_params(int variant, lisreg_params* p)
{
    if (!p || variant < 1 || variant > 3) return LISREG_ERR_ARG;
    memset(p, 0, sizeof *p);
    static const float score[20] = { 1.0f, 1.0f, 0.6f, 0.5f, 0.8f, 0.5f, 0.5f, 0.5f, 0.5f, 1.2f,     // config/label.yaml:214-234
                                     1.2f, 1.2f, 0.5f, 1.0f, 0.8f, 0.5f, 1.3f, 0.5f, 1.5f, 1.5f };
    p->max_iters = variant == 1 ? 15 : (variant == 2 ? 20 : 30);
    p->fixed_iters = 0;
    p->knn_sq_thresh = variant == 1 ? 1.0f : 2.0f;
    p->conv_deg = variant == 1 ? 0.005f : (variant == 2 ? 0.003f : 0.002f);
    p->conv_cm = variant == 1 ? 0.05f : (variant == 2 ? 0.03f : 0.02f);
    p->min_corr = 50; p->eig_thresh = 100.f; p->edge_min = -1; p->surf_min = 100;
    p->line_ratio = 3.f; p->plane_tol = 0.2f; p->accept_s = 0.1f;
    p->use_label_weight = variant == 1 ? 0 : 1;
    for (int i = 0; i < 32; ++i) p->label_score[i] = i < 20 ? score[i] : 0.0f;    // a label the std::map does not hold reads as 0 (:1671)
    p->emulate_matp_shadow = 1;
    p->skip_empty_target = variant == 3 ? 1 : 0;
    p->use_imu_blend = variant == 3 ? 0 : 1;
    p->imu_rpy_weight = 0.1f; p->rotation_tol = 1000.f; p->z_tol = 1000.f;
    return LISREG_OK;
}

// transformUpdate, host form (odomEstimationNode.cpp:976-1006): tf's double-precision quaternion slerp of the
// single-axis roll / pitch rotations, then constraintTransformation (common.cpp:285-291).
void lisreg_transform_update(const lisreg_params* p, const lisreg_imu* imu, float T[6])
{
    auto blend = [](double a, double b, double w, bool is_pitch) {
        // slerp between two rotations about ONE axis by angles a and b: quaternions (sin(a/2), cos(a/2))
        double qa_s = sin(a * 0.5), qa_c = cos(a * 0.5), qb_s = sin(b * 0.5), qb_c = cos(b * 0.5);
        double d = qa_s * qb_s + qa_c * qb_c;
        double theta = d < 0 ? acos(-d) : acos(d);
        double rs = qa_s, rc = qa_c;
        if (theta != 0.0) {
            double dd = 1.0 / sin(theta), s0 = sin((1.0 - w) * theta), s1 = sin(w * theta), sg = d < 0 ? -1.0 : 1.0;
            rs = (qa_s * s0 + sg * qb_s * s1) * dd;
            rc = (qa_c * s0 + sg * qb_c * s1) * dd;
        }
        double n2 = rs * rs + rc * rc, s = 2.0 / n2;
        if (!is_pitch) {                       // rotation about X: m21 = 2wx, m22 = 1 - 2xx ; getRPY roll = atan2(m21, m22)
            return atan2(rc * rs * s, 1.0 - rs * rs * s);
        }
        double m20 = -(rc * rs * s);           // rotation about Y: m20 = xz - wy = -2wy
        if (fabs(m20) >= 1) return m20 < 0 ? M_PI / 2.0 : -M_PI / 2.0;
        return -asin(m20);
    };
    if (p->use_imu_blend && imu && imu->imu_available && fabsf(imu->imu_pitch_init) < 1.4f) {
        T[0] = (float)blend((double)T[0], (double)imu->imu_roll_init, (double)p->imu_rpy_weight, false);
        T[1] = (float)blend((double)T[1], (double)imu->imu_pitch_init, (double)p->imu_rpy_weight, true);
    }
    auto clampf = [](float v, float lim) { if (v < -lim) v = -lim; if (v > lim) v = lim; return v; };
    T[0] = clampf(T[0], p->rotation_tol);
    T[1] = clampf(T[1], p->rotation_tol);
    T[5] = clampf(T[5], p->z_tol);
}

// ---- target -------------------------------------------------------------------------------------------------
static int set_target_impl(lisreg_ctx* c, int slot, const void* clouds[2], const int counts[2], int stride, int fmt)
{
    if (!c) return LISREG_ERR_ARG;
    if (slot < 0 || slot > 65535) return bad(c, "set_target: bad slot");
    for (int k = 0; k < 2; ++k)          // (any fmt but DEVICE and XYZIL is read as XYZI structs)
        if (const int rc = check_cloud(c, "set_target", clouds[k], counts[k], stride, fmt == LISREG_FMT_DEVICE || fmt == LISREG_FMT_XYZIL ? fmt : LISREG_FMT_XYZI,
                                       fmt_bit(LISREG_FMT_DEVICE) | fmt_bit(LISREG_FMT_XYZI) | fmt_bit(LISREG_FMT_XYZIL), true)) return rc;
    for (int k = 0; k < 2; ++k)          // the kernels address a target's 16-byte records by 32-bit byte offsets from a scalar base
        if (counts[k] >= (1 << 28)) return bad(c, "set_target: a cloud of 2^28 points or more");
    HIPCHK(c, hipSetDevice(c->device));
    if ((size_t)slot >= c->targets.size()) c->targets.resize((size_t)slot + 1);
    Target& t = c->targets[(size_t)slot];
    t.gen = ++c->target_gen;
    float bb_dev[2][8] = { { 0 }, { 0 } };
    if (fmt == LISREG_FMT_DEVICE && (counts[0] > 0 || counts[1] > 0)) {          // both bounding boxes, one read-back
        HIPCHK(c, c->bbox_dev.ensure(sizeof(float) * 16));
        HIPCHK(c, c->bbox_scratch.ensure(sizeof(float) * 2 * 6 * 256));
        for (int k = 0; k < 2; ++k)
            if (counts[k] > 0)
                launch_bbox(static_cast<const float4*>(clouds[k]), counts[k], c->bbox_dev.as<float>() + 8 * k, c->bbox_scratch.as<float>() + 6 * 256 * k, c->stream);
        HIPCHK(c, hipMemcpyAsync(bb_dev, c->bbox_dev.p, sizeof bb_dev, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    for (int k = 0; k < 2; ++k) {
        const int n = counts[k];
        t.n[k] = n;
        float bb[6] = { 0, 0, 0, 0, 0, 0 };
        if (fmt == LISREG_FMT_DEVICE) {
            t.raw_external[k] = true;
            t.raw_ptr[k] = static_cast<const float4*>(clouds[k]);
            if (n > 0) memcpy(bb, bb_dev[k], sizeof bb);
        } else {
            std::vector<lisreg_dpoint> h((size_t)std::max(n, 1));
            if (n > 0) pack_cloud(clouds[k], n, stride, fmt, h.data());
            for (int d = 0; d < 3; ++d) { bb[d] = 3.0e38f; bb[3 + d] = -3.0e38f; }
            for (int i = 0; i < n; ++i) {
                const float v[3] = { h[(size_t)i].x, h[(size_t)i].y, h[(size_t)i].z };
                for (int d = 0; d < 3; ++d) { bb[d] = std::min(bb[d], v[d]); bb[3 + d] = std::max(bb[3 + d], v[d]); }
            }
            // on the context's stream: a run still queued there against this slot (it may re-read the raw records) reads the old
            // cloud; the null stream would order nothing against it
            if (const int rc = upload_packed(c, h.data(), (size_t)n, t.raw[k])) return rc;
            t.raw_external[k] = false;
            t.raw_ptr[k] = t.raw[k].as<float4>();
        }
        for (int d = 0; d < 6; ++d)
            if (n > 0 && !std::isfinite(bb[d])) return bad(c, "set_target: the cloud has infinite coordinates (NaN points are ignored, Inf is not indexable)");
        if (n > 0 && !(bb[0] <= bb[3] && bb[1] <= bb[4] && bb[2] <= bb[5]))
            return bad(c, "set_target: the cloud has no finite point (every coordinate is NaN)");
        // the cell rows (search front-end 5) want a grid that reaches two cells past the cloud; when the front-end is left to the batch
        // (auto), a target gets that margin only once a batch has chosen the cell rows for it (ensure_crow_margin)
        // — and keeps it from then on: a slot whose targets went through the cell rows last time (a frame stream re-sets its slot
        // every frame) is indexed with the margin straight away, instead of being built twice per set
        memcpy(t.bbox[k], bb, sizeof bb);
        t.grid_margin[k] = (c->opt.search_mode == 5 || (c->opt.search_mode == 4 && t.crow_chosen[k])) ? kCrowGridMargin : 0;
        make_grid(bb, n, &t.g[k], &t.n_cells[k], t.grid_margin[k]);
        prof_mark(c, 2);
        int rc = build_target_kind(c, t, k);
        t.graph_valid[k] = false;
        t.crow_valid[k] = false; t.crow_too_big[k] = false;
        t.g[k].crow = nullptr; t.g[k].crow_meta = nullptr; t.g[k].crow_tab = nullptr;
        if (!rc && c->opt.search_mode == 3) rc = ensure_graph(c, t, k, true);
        if (!rc && c->opt.search_mode == 5) rc = ensure_crows(c, t, k);
        prof_mark(c, -1);
        if (rc) return rc;
    }
    t.valid = true;
    c->grids_dirty = true;
    c->batch.live.prepared = false;
    return LISREG_OK;
}

int lisreg_set_target_slot(lisreg_ctx* c, int slot, const void* corner, int n_corner, const void* surf, int n_surf,
                           int stride, int fmt)
{
    const void* clouds[2] = { corner, surf };
    const int counts[2] = { n_corner, n_surf };
    return set_target_impl(c, slot, clouds, counts, stride, fmt);
}

int lisreg_set_target(lisreg_ctx* c, const void* corner, int n_corner, const void* surf, int n_surf, int stride, int fmt)
{
    return lisreg_set_target_slot(c, 0, corner, n_corner, surf, n_surf, stride, fmt);
}

int lisreg_target_from_classes(lisreg_ctx* c, int slot, const void* pole, int n_pole, const void* ground, int n_ground,
                               const void* building, int n_building, const void* dynamic, int n_dynamic,
                               int stride, int fmt)
{
    if (!c) return LISREG_ERR_ARG;
    if (fmt == LISREG_FMT_DEVICE) return bad(c, "target_from_classes: host clouds only");
    if (stride < 12) return bad(c, "target_from_classes: stride < 12");      // (the parts are copied by it below; lisreg_set_target_slot checks the rest)
    // surf = ground + building + dynamic, the concat order of extractSlidingCloud (subMapOptmizationNode.cpp:1408-1419)
    const void* parts[3] = { ground, building, dynamic };
    const int cnt[3] = { std::max(n_ground, 0), std::max(n_building, 0), std::max(n_dynamic, 0) };
    std::vector<unsigned char> surf((size_t)(cnt[0] + cnt[1] + cnt[2]) * (size_t)stride + 1);
    size_t off = 0;
    for (int i = 0; i < 3; ++i) if (cnt[i] > 0 && parts[i]) {
        memcpy(surf.data() + off, parts[i], (size_t)cnt[i] * (size_t)stride);
        off += (size_t)cnt[i] * (size_t)stride;
    }
    return lisreg_set_target_slot(c, slot, pole, pole ? std::max(n_pole, 0) : 0, surf.data(), (int)(off / (size_t)stride), stride, fmt);
}

// Options that are not part of the reference's parameter surface (kept out of lisreg_params on purpose).
int lisreg_set_option(lisreg_ctx* c, const char* name, int value)
{
    if (!c || !name) return LISREG_ERR_ARG;
    if (!strcmp(name, "rebuild_targets_each_run")) {
        c->opt.rebuild_targets_each_run = value != 0;
        if (c->batch.live.prepared && c->opt.rebuild_targets_each_run) {      // the rebuild needs its sort scratch
            int rc = ensure_sort_scratch(c, (size_t)std::max(c->batch.t_elems, 1), (size_t)std::max(c->batch.t_buckets, 1));
            if (rc) return rc;
        }
        return LISREG_OK;
    }
    if (!strcmp(name, "sort_sources")) { c->opt.sort_sources = value; c->mem.probe_items = -1; return LISREG_OK; }
    if (!strcmp(name, "cell_anchor_until")) { c->opt.cell_anchor_until = std::max(value, 0); return LISREG_OK; }
    if (!strcmp(name, "search_mode")) {
        if (value < 1 || value > 5 || value == 2) return bad(c, "search_mode: 1 cell walk, 3 k-NN graph scan, 4 auto, 5 cell rows");
        c->opt.search_mode = value; c->batch.live.prepared = false; return LISREG_OK;
    }
    if (!strcmp(name, "graph_min_ratio")) { c->opt.graph_min_ratio = value; c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "cell_min_ratio")) { c->opt.cell_min_ratio = value; c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "row_reach")) {
        if (value < 0 || value > 2) return bad(c, "row_reach: 0 all rows, 1 rows within a metre of the queries, 2 of those the cells near the target or a query");
        c->opt.row_reach = value; c->mem.reach_backoff = 0; c->batch.live.prepared = false; return LISREG_OK;
    }
    if (!strcmp(name, "cell_rows_max_mb")) {
        c->opt.cell_rows_max_mb = value; c->batch.live.prepared = false;
        for (auto& t : c->targets) for (int k = 0; k < 2; ++k) {        // a new bound: what was too big may fit now, what fitted may have to be capped
            t.crow_too_big[k] = false;
            if (t.crow_valid[k]) { t.crow_valid[k] = false; c->grids_dirty = true; }
        }
        return LISREG_OK;
    }
    if (!strcmp(name, "early_stop_chunk")) { c->opt.early_stop_chunk = value; return LISREG_OK; }
    if (!strcmp(name, "xcd_order")) { if (value < 0 || value > 2) return bad(c, "xcd_order: 0 off, 1 on, 2 auto"); c->opt.xcd_order = value; c->batch.live.xcd_cached = false; return LISREG_OK; }
    if (!strcmp(name, "index_build")) {
        if (value < 0 || value > 2) return bad(c, "index_build: 0 bucket sort, 1 strip form, 2 auto");
        c->opt.index_build = value; c->batch.live.prepared = false;
        return LISREG_OK;
    }
    if (!strcmp(name, "index_strip_cells")) { c->opt.strip_cells = std::max(value, 0); c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "index_strip_cap")) { c->opt.strip_cap = std::min(std::max(value, 64), 16384); c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "count_searches")) {
        c->opt.count_searches = value != 0;
        if (c->opt.count_searches) { HIPCHK(c, c->counters.ensure(128 * 8)); HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 128 * 8, c->stream)); }   // behind a counting run still queued
        return LISREG_OK;
    }
    if (!strcmp(name, "lanes_per_query")) { c->opt.lanes_per_query_auto = value != 1; c->batch.live.prepared = false; return LISREG_OK; }   // 1 forces one lane per query, anything else = auto
    if (!strcmp(name, "dump_neighbors")) { c->opt.dump_neighbors = value != 0; c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "exact_arithmetic")) { c->opt.exact = value != 0; c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "feeder_copy_engine")) { c->feeder_engine = value; return LISREG_OK; }
    if (!strcmp(name, "canonical_ties")) { c->opt.canonical_ties = value != 0; c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "first_pass_mm")) {          // (a negative radius would square to the positive one: refused rather than taken as that)
        if (value < 0) return bad(c, "first_pass_mm: a radius in millimetres, >= 0");
        c->opt.first_pass_r = 1e-3f * (float)value; return LISREG_OK;
    }
    if (!strcmp(name, "trace_cap")) { c->opt.trace_cap = std::max(0, value); c->batch.live.prepared = false; return LISREG_OK; }
    if (!strcmp(name, "feeder_threads")) { c->feeder_threads = std::min(std::max(value, 0), 64); return LISREG_OK; }
    if (!strcmp(name, "feeder_numa")) { c->feeder_numa = value != 0; return LISREG_OK; }       // takes effect when the thread pool is created
    if (!strcmp(name, "interleave_min_blocks")) { c->opt.interleave_min_blocks = std::max(value, 2); return LISREG_OK; }
    if (!strcmp(name, "interleave")) { if (value < 0 || value > 2) return bad(c, "interleave: 0 off, 1 alternating halves, 2 free-running halves"); c->opt.interleave = value; return LISREG_OK; }
    return bad(c, std::string("set_option: unknown option ") + name);
}

int lisreg_get_option(const lisreg_ctx* c, const char* name, int* value)
{
    if (!c || !name || !value) return LISREG_ERR_ARG;
    if (!strcmp(name, "search_mode")) { *value = c->opt.search_mode; return LISREG_OK; }
    if (!strcmp(name, "exact_arithmetic")) { *value = c->opt.exact ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "feeder_chunks_by_copy_engine")) { *value = c->pack_stolen; return LISREG_OK; }
    if (!strcmp(name, "feeder_chunks")) { *value = c->pack_chunks_n; return LISREG_OK; }
    if (!strcmp(name, "canonical_ties")) { *value = (c->opt.canonical_ties || c->opt.exact) ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "index_build")) { *value = c->opt.index_build; return LISREG_OK; }
    if (!strcmp(name, "index_build_now")) { *value = c->batch.strip_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "front_end")) { *value = c->batch.mode_now; return LISREG_OK; }
    if (!strcmp(name, "lanes_per_query")) { *value = c->batch.lanes_q; return LISREG_OK; }          // what the prepared batch runs (auto resolved)
    if (!strcmp(name, "sort_sources")) { *value = c->opt.sort_sources; return LISREG_OK; }
    if (!strcmp(name, "cell_anchor_until")) { *value = c->opt.cell_anchor_until; return LISREG_OK; }
    if (!strcmp(name, "feeder_threads")) { *value = c->feeder_threads; return LISREG_OK; }
    if (!strcmp(name, "feeder_numa_node")) { *value = c->feeder_node; return LISREG_OK; }
    if (!strcmp(name, "feeder_numa_cpus")) { *value = c->feeder_cpus; return LISREG_OK; }
    if (!strcmp(name, "comm_nranks")) { *value = c->comm ? c->comm_nranks : 0; return LISREG_OK; }
    if (!strcmp(name, "sorted_now")) { *value = c->batch.sort_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "rebuild_targets_each_run")) { *value = c->opt.rebuild_targets_each_run ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "graph_min_ratio")) { *value = c->opt.graph_min_ratio; return LISREG_OK; }
    if (!strcmp(name, "cell_min_ratio")) { *value = c->opt.cell_min_ratio; return LISREG_OK; }
    if (!strcmp(name, "row_reach")) { *value = c->opt.row_reach; return LISREG_OK; }
    if (!strcmp(name, "row_reach_now")) { *value = c->last.reach_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "row_reach_misses")) { *value = c->last.reach_miss_last; return LISREG_OK; }
    if (!strcmp(name, "cell_rows_max_mb")) { *value = c->opt.cell_rows_max_mb; return LISREG_OK; }
    if (!strcmp(name, "xcd_order")) { *value = c->opt.xcd_order; return LISREG_OK; }
    if (!strcmp(name, "xcd_order_now")) { *value = c->last.xcd_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "interleave")) { *value = c->opt.interleave; return LISREG_OK; }
    if (!strcmp(name, "interleaved_now")) { *value = c->last.interleaved_now ? 1 : 0; return LISREG_OK; }
    // size of the search index of the prepared batch's targets, in KiB (what the front-end in use reads), and their points:
    //   index_kib_grid: sorted records + cell table; index_kib_front_end: k-NN graph rows (front-end 3) or cell rows + their table (front-end 5)
    if (!strcmp(name, "index_kib_front_end_built")) {
        // the cell rows the LAST run actually built (option "row_reach" leaves out the cells no query comes near): row counts read back from the
        // device (a synchronous diagnostic); other front-ends: what "index_kib_front_end" says
        if (c->batch.mode_now != 5) return lisreg_get_option(c, "index_kib_front_end", value);
        unsigned long long fe = 0;
        for (int slot : c->batch.batch_slots) {
            if (slot < 0 || (size_t)slot >= c->targets.size()) continue;
            const lisreg::Target& t = c->targets[(size_t)slot];
            for (int k = 0; k < 2; ++k) {
                if (t.n[k] <= 0 || !t.crow_scan[k].p) continue;
                int rows = 0;
                if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
                    hipMemcpy(&rows, t.crow_scan[k].as<int>() + t.n_cells[k], sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return LISREG_ERR_HIP;
                rows = std::min(std::max(rows, 0), t.crow_cap[k]);
                fe += (unsigned long long)rows * lisreg::kCrowRowBytes + (unsigned long long)t.n_cells[k] * sizeof(int);
            }
        }
        *value = (int)std::min<unsigned long long>((fe + 1023) / 1024, 0x7fffffffULL);
        return LISREG_OK;
    }
    if (!strcmp(name, "index_kib_grid") || !strcmp(name, "index_kib_front_end") || !strcmp(name, "index_target_points")) {
        unsigned long long grid = 0, fe = 0, pts = 0;
        for (int slot : c->batch.batch_slots) {
            if (slot < 0 || (size_t)slot >= c->targets.size()) continue;
            const lisreg::Target& t = c->targets[(size_t)slot];
            for (int k = 0; k < 2; ++k) {
                if (t.n[k] <= 0) continue;
                pts += (unsigned long long)t.n[k];
                grid += (unsigned long long)t.n[k] * sizeof(float4) + ((unsigned long long)t.n_cells[k] + 1) * sizeof(int);
                if (c->batch.mode_now == 3) fe += (unsigned long long)t.n[k] * lisreg::kCrowRowBytes;
                if (c->batch.mode_now == 5) fe += (unsigned long long)t.crow_cap[k] * lisreg::kCrowRowBytes +
                                            (unsigned long long)t.n_cells[k] * sizeof(int);
            }
        }
        const unsigned long long v = !strcmp(name, "index_target_points") ? pts : ((!strcmp(name, "index_kib_grid") ? grid : fe) + 1023) / 1024;
        *value = (int)std::min<unsigned long long>(v, 0x7fffffffULL);
        return LISREG_OK;
    }
    return LISREG_ERR_ARG;
}

int lisreg_get_trace(lisreg_ctx* c, float* buf, int max_iters)
{
    if (!c || !buf || max_iters <= 0) return 0;
    const int n = std::min(max_iters, c->mem.last_trace_n);
    if (n > 0) memcpy(buf, c->mem.last_trace.data(), sizeof(float) * kTraceStride * (size_t)n);
    return n;
}

int lisreg_get_counters(lisreg_ctx* c, unsigned long long* out, int n)
{
    if (!c || !out || n < 0) return LISREG_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = 0;
    if (!c->counters.p) return LISREG_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->counters.p, sizeof(unsigned long long) * (size_t)std::min(n, 128), hipMemcpyDeviceToHost));
    if (c->batch.mode_now == 3 || c->batch.mode_now == 5) {              // the graph scan packs (walked << 32 | valid) per GN iteration: unpack to the pair layout
        unsigned long long tmp[64] = { 0 };
        for (int i = 0; i < 32 && 2 * i + 1 < n; ++i) { tmp[2 * i] = out[i] >> 32; tmp[2 * i + 1] = out[i] & 0xffffffffull; }
        for (int i = 0; i < std::min(n, 64); ++i) out[i] = tmp[i];
    }
    return LISREG_OK;
}

int lisreg_get_target_index(lisreg_ctx* c, int slot, int kind, int* dims /* n, nx, ny, nz, n_cells */, float* geom /* ox, oy, oz, cell */,
                            float* sorted_out, int sorted_capacity, int* cell_start_out, int cell_capacity)
{
    if (!c || slot < 0 || (size_t)slot >= c->targets.size() || kind < 0 || kind > 1 || !c->targets[(size_t)slot].valid)
        return bad(c, "get_target_index: no such target");
    const Target& t = c->targets[(size_t)slot];
    const GridIndex& g = t.g[kind];
    if (dims) { dims[0] = t.n[kind]; dims[1] = g.nx; dims[2] = g.ny; dims[3] = g.nz; dims[4] = t.n_cells[kind]; }
    if (geom) { geom[0] = g.ox; geom[1] = g.oy; geom[2] = g.oz; geom[3] = g.cell; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (sorted_out) {
        if (sorted_capacity < t.n[kind]) return bad(c, "get_target_index: sorted_capacity too small");
        if (t.n[kind] > 0) HIPCHK(c, hipMemcpy(sorted_out, t.sorted[kind].p, sizeof(float4) * (size_t)t.n[kind], hipMemcpyDeviceToHost));
    }
    if (cell_start_out) {
        if (cell_capacity < t.n_cells[kind] + 1) return bad(c, "get_target_index: cell_capacity too small");
        HIPCHK(c, hipMemcpy(cell_start_out, t.cell_start[kind].p, sizeof(int) * ((size_t)t.n_cells[kind] + 1), hipMemcpyDeviceToHost));
    }
    return LISREG_OK;
}

int lisreg_get_target_graph(lisreg_ctx* c, int slot, int kind, int* k_out, float* rows_out, float* meta_out, int capacity_points)
{
    if (!c || slot < 0 || (size_t)slot >= c->targets.size() || kind < 0 || kind > 1 || !c->targets[(size_t)slot].valid)
        return bad(c, "get_target_graph: no such target");
    Target& t = c->targets[(size_t)slot];
    if (k_out) *k_out = kGraphK;
    if (!rows_out && !meta_out) return LISREG_OK;
    if (capacity_points < t.n[kind]) return bad(c, "get_target_graph: capacity_points too small");
    HIPCHK(c, hipSetDevice(c->device));
    if (!t.graph_valid[kind] || !t.g[kind].nbr) {            // build it now (it is built on demand otherwise)
        int rc = ensure_graph(c, t, kind, true);
        if (rc) return rc;
        c->grids_dirty = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)t.n[kind];
    if (rows_out && n) HIPCHK(c, hipMemcpy(rows_out, t.nbr[kind].p, sizeof(float4) * kGraphK * n, hipMemcpyDeviceToHost));
    if (meta_out && n) HIPCHK(c, hipMemcpy(meta_out, t.nbr_meta[kind].p, sizeof(float2) * n, hipMemcpyDeviceToHost));
    return LISREG_OK;
}

int lisreg_get_target_cell_rows(lisreg_ctx* c, int slot, int kind, int* n_rows, int* k_out, int* table_out, int capacity_cells,
                                float* rows_out, float* meta_out, int capacity_rows)
{
    if (!c || slot < 0 || (size_t)slot >= c->targets.size() || kind < 0 || kind > 1 || !c->targets[(size_t)slot].valid)
        return bad(c, "get_target_cell_rows: no such target");
    HIPCHK(c, hipSetDevice(c->device));
    Target& t = c->targets[(size_t)slot];
    if (k_out) *k_out = kGraphK;
    if (!t.crow_valid[kind] || !t.g[kind].crow_tab) {
        int rc = ensure_crows(c, t, kind);
        if (rc) return rc;
        c->grids_dirty = true;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int rows = 0;
    if (t.n[kind] > 0) HIPCHK(c, hipMemcpy(&rows, t.crow_scan[kind].as<int>() + t.n_cells[kind], sizeof(int), hipMemcpyDeviceToHost));
    rows = std::min(rows, t.crow_cap[kind]);
    if (n_rows) *n_rows = rows;
    if (table_out) {
        if (capacity_cells < t.n_cells[kind]) return bad(c, "get_target_cell_rows: capacity_cells too small");
        HIPCHK(c, hipMemcpy(table_out, t.crow_tab[kind].p, sizeof(int) * (size_t)t.n_cells[kind], hipMemcpyDeviceToHost));
    }
    if ((rows_out || meta_out) && capacity_rows < rows) return bad(c, "get_target_cell_rows: capacity_rows too small");
    if (rows_out && rows) {
        HIPCHK(c, hipMemcpy(rows_out, t.crow[kind].p, sizeof(float4) * kGraphK * (size_t)rows, hipMemcpyDeviceToHost));
    }
    if (meta_out && rows) HIPCHK(c, hipMemcpy(meta_out, t.crow_meta[kind].p, sizeof(float2) * (size_t)rows, hipMemcpyDeviceToHost));
    return LISREG_OK;
}

int lisreg_get_neighbors(lisreg_ctx* c, int* out, int n_elems)
{
    if (!c || !out || n_elems < 0) return LISREG_ERR_ARG;
    if (!c->opt.dump_neighbors || !c->dbg_nn.p || n_elems != c->batch.n_elems || (c->batch.mode_now != 1 && c->batch.mode_now != 3 && c->batch.mode_now != 5))
        return bad(c, "get_neighbors: set option dump_neighbors before preparing the batch (search modes 1, 3); n_elems must be the batch's source point count");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->dbg_nn.p, sizeof(int) * 6 * (size_t)n_elems, hipMemcpyDeviceToHost));
    return LISREG_OK;
}

// Host code only: nothing here is on the production path and no buffer is sized or cleared for it.  The partial rows outlive the run
// because nothing but the next correspondence launch writes them: k_solve reads them as const, and the finalize — on its own
// (k_finalize) or folded into the last solve (finalize_in_last_solve) — resets the registrations' ItemState and touches neither
// `partials` nor `coef` / `coef_ok`.  An interleaved run joins its side stream into the context's stream before it returns.
int lisreg_get_partial_rows(lisreg_ctx* c, int* n_blocks, int* blocks, double* rows, int capacity_blocks, float* coef, int* coef_ok,
                            int n_elems)
{
    if (!c || !n_blocks) return LISREG_ERR_ARG;
    const PreparedBatch& b = c->batch;
    if (!b.live.prepared) return bad(c, "get_partial_rows: no prepared batch");
    if (!c->opt.dump_neighbors || !c->dbg_nn.p || (b.mode_now != 1 && b.mode_now != 3 && b.mode_now != 5))
        return bad(c, "get_partial_rows: set option dump_neighbors before preparing the batch (search modes 1, 3, 5)");
    if ((blocks || rows) && capacity_blocks < b.n_blocks) return bad(c, "get_partial_rows: capacity_blocks too small");
    if (coef || coef_ok) {
        if (b.lanes_q <= 1) return bad(c, "get_partial_rows: the prepared batch runs one lane per query: it keeps no coefficients");
        if (n_elems != b.n_elems) return bad(c, "get_partial_rows: n_elems must be the batch's source point count");
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<BlockDesc> hb((size_t)b.n_blocks);
    std::vector<Segment> hs((size_t)b.n_segs);
    if (b.n_blocks) HIPCHK(c, hipMemcpy(hb.data(), c->blocks.p, sizeof(BlockDesc) * hb.size(), hipMemcpyDeviceToHost));
    if (b.n_segs) HIPCHK(c, hipMemcpy(hs.data(), c->segs.p, sizeof(Segment) * hs.size(), hipMemcpyDeviceToHost));
    for (const BlockDesc& d : hb)
        if (d.seg < 0 || d.seg >= b.n_segs) return ctx_fail(c, LISREG_ERR_HIP, "get_partial_rows: the device block table names no segment of the batch");
    if (rows && b.n_blocks) HIPCHK(c, hipMemcpy(rows, c->partials.p, sizeof(double) * kNumAcc * hb.size(), hipMemcpyDeviceToHost));
    if (coef && b.n_elems) HIPCHK(c, hipMemcpy(coef, c->coef.p, sizeof(float4) * (size_t)b.n_elems, hipMemcpyDeviceToHost));
    if (coef_ok && b.n_elems) HIPCHK(c, hipMemcpy(coef_ok, c->coef_ok.p, sizeof(int) * (size_t)b.n_elems, hipMemcpyDeviceToHost));
    // (copied as they are: for a segment whose target has fewer than five points k_assoc_walk leaves before it searches (g.n < 5) and
    // never writes its queries' coefficients — the buffers hold there whatever an earlier batch left, and include/lisreg.h says so)
    if (blocks)
        for (size_t i = 0; i < hb.size(); ++i) {
            const Segment& s = hs[(size_t)hb[i].seg];
            blocks[4 * i] = hb[i].item; blocks[4 * i + 1] = s.kind; blocks[4 * i + 2] = s.flat_base + hb[i].start; blocks[4 * i + 3] = hb[i].count;
        }
    *n_blocks = b.n_blocks;
    return LISREG_OK;
}

int lisreg_test_fit_models(lisreg_ctx* c, int kind, int n, const float* neighbours, const float* queries, const lisreg_params* params,
                           int exact, float* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (kind < 0 || kind > 2 || n < 0 || !params || (n > 0 && (!neighbours || !queries || !out)))
        return bad(c, "test_fit_models: bad arguments");
    if (n == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    DevBuf nb, q, o;
    HIPCHK(c, nb.ensure(sizeof(float) * 15 * (size_t)n));
    HIPCHK(c, q.ensure(sizeof(float) * 3 * (size_t)n));
    HIPCHK(c, o.ensure(sizeof(float) * 10 * (size_t)n));
    HIPCHK(c, hipMemcpyAsync(nb.p, neighbours, sizeof(float) * 15 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(q.p, queries, sizeof(float) * 3 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    DevParams prm = make_dev_params(*params);
    prm.exact = exact ? 1 : 0;
    if (exact) launch_test_fit_exact(kind, n, nb.as<float>(), q.as<float>(), prm, o.as<float>(), c->stream);
    else launch_test_fit(kind, n, nb.as<float>(), q.as<float>(), prm, o.as<float>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(out, o.p, sizeof(float) * 10 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

int lisreg_test_solve_steps(lisreg_ctx* c, int n_items, int n_steps, const int* n_rows, const double* rows, const float* T_init,
                            const int* degenerate_in, const int* n_sc, const int* n_ss, const lisreg_imu* imu,
                            const lisreg_params* params, float* trace_out, float* state_out, float* results_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || n_steps < 1 || n_steps > 64 || !params || (n_items > 0 && (!n_rows || !T_init)))
        return bad(c, "test_solve_steps: bad arguments");
    if (n_items == 0) return LISREG_OK;
    size_t total_rows = 0;
    for (int i = 0; i < n_items; ++i) {
        if (n_rows[i] < 0) return bad(c, "test_solve_steps: negative row count");
        total_rows += (size_t)n_rows[i];
    }
    if (total_rows > 0x7fffffffu || (total_rows > 0 && !rows)) return bad(c, "test_solve_steps: bad rows");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_items;
    DevParams prm = make_dev_params(*params);
    std::vector<ItemState> h_items(n);
    memset(h_items.data(), 0, sizeof(ItemState) * n);
    int blk = 0;
    prm.n_guard_failed = 0;
    for (size_t i = 0; i < n; ++i) {
        ItemState& it = h_items[i];
        for (int k = 0; k < 6; ++k) it.T_init[k] = T_init[6 * i + k];
        it.degenerate_in = degenerate_in ? degenerate_in[i] : 0;
        it.blk_begin = blk; it.blk_count = n_rows[i]; blk += n_rows[i];
        it.n_sc = n_sc ? n_sc[i] : prm.edge_min + 1;
        it.n_ss = n_ss ? n_ss[i] : prm.surf_min + 1;
        if (imu) it.imu = imu[i];
        if (!(it.n_sc > prm.edge_min && it.n_ss > prm.surf_min)) ++prm.n_guard_failed;
    }
    const size_t step_doubles = total_rows * kNumAcc, trace_floats = n * (size_t)n_steps * kTraceStride;
    DevBuf d_items, d_rows, d_trace, d_results, d_done;
    HIPCHK(c, d_items.ensure(sizeof(ItemState) * n));
    HIPCHK(c, d_rows.ensure(sizeof(double) * std::max<size_t>(step_doubles * (size_t)n_steps, 1)));
    HIPCHK(c, d_trace.ensure(sizeof(float) * trace_floats));
    HIPCHK(c, d_results.ensure(sizeof(float) * kResultSize * n));
    HIPCHK(c, d_done.ensure(sizeof(int)));
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(d_items.p, h_items.data(), sizeof(ItemState) * n, hipMemcpyHostToDevice, st));
    if (step_doubles) HIPCHK(c, hipMemcpyAsync(d_rows.p, rows, sizeof(double) * step_doubles * (size_t)n_steps, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(d_trace.p, 0, sizeof(float) * trace_floats, st));
    launch_reset_items(d_items.as<ItemState>(), n_items, prm, d_done.as<int>(), st);
    for (int s = 0; s < n_steps; ++s) {
        launch_solve(d_items.as<ItemState>(), n_items, prm, d_rows.as<double>() + step_doubles * (size_t)s, d_trace.as<float>(), n_steps,
                     d_done.as<int>(), st);
        HIPCHK(c, hipGetLastError());
        if (!state_out) continue;
        HIPCHK(c, hipMemcpyAsync(h_items.data(), d_items.p, sizeof(ItemState) * n, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        for (size_t i = 0; i < n; ++i) {
            const ItemState& it = h_items[i];
            float* o = state_out + (i * (size_t)n_steps + (size_t)s) * LISREG_SOLVE_STATE_STRIDE;
            for (int k = 0; k < 36; ++k) o[k] = it.P[k];
            for (int k = 0; k < 12; ++k) o[36 + k] = it.M[k];
            o[48] = (float)it.degenerate; o[49] = it.deltaR; o[50] = it.deltaT; o[51] = (float)it.n_corr;
            o[52] = (float)it.done; o[53] = (float)it.iters_out; o[54] = (float)it.any_solved; o[55] = (float)it.iter;
        }
    }
    launch_finalize(d_items.as<ItemState>(), n_items, prm, d_results.as<float>(), st);
    HIPCHK(c, hipGetLastError());
    if (trace_out) HIPCHK(c, hipMemcpyAsync(trace_out, d_trace.p, sizeof(float) * trace_floats, hipMemcpyDeviceToHost, st));
    if (results_out) HIPCHK(c, hipMemcpyAsync(results_out, d_results.p, sizeof(float) * kResultSize * n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

int lisreg_set_profiling(lisreg_ctx* c, int enable)
{
    if (!c) return LISREG_ERR_ARG;
    c->profiling = enable != 0;
    return LISREG_OK;
}

int lisreg_get_timing(lisreg_ctx* c, double out[5])
{
    if (!c || !out) return LISREG_ERR_ARG;
    for (int i = 0; i < 5; ++i) out[i] = c->timing[i];
    return LISREG_OK;
}

}  // extern "C"
