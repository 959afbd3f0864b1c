// lisreg_api.hip — C-ABI host layer of liblisreg.so (declared in include/lisreg.h): context lifecycle, registration targets, batch
// prepare / run / fetch / align, options, diagnostics, test hooks, profiling.  The other subsystems have a unit each
// (lisreg_api_{cloud,features,feed,map,localmap,comm}.hip); what they all share is in lisreg_api_ctx.hip.
//
// Creates the seam the reference lacks: each entry point replaces a piece of
// scan2SubMapOptimization() — /root/reference/src/node/odomEstimationNode.cpp:596-626 and the copies at
// src/node/subMapOptmizationNode.cpp:1509-1541, 4485-4540.  The GN loop is enqueued in full (optional index rebuild,
// optional source sort, `bound` x {correspondence kernel, solve kernel}, finalize) with no host synchronisation inside
// lisreg_batch_run (the synchronous entry points may stop launching early once every item has converged); a
// context is single-threaded and owns its stream, so several contexts run concurrently (callers #2/#3).
// There is deliberately NO CPU fallback: without a HIP device every compute entry point fails with
// LISREG_ERR_HIP.
#include "lisreg_ctx.hpp"

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

namespace {

DevParams make_dev_params(const lisreg_params& p)
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

// search_mode 3: neighbour lists of target kind k (the index itself must already be enqueued on the stream)
int ensure_graph(lisreg_ctx* c, Target& t, int k, bool launch)
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

lisreg::CrowBuffers crow_buffers(Target& t, int k, bool with_reach = false, bool near_only = false)
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
int ensure_reach(lisreg_ctx* c, Target& t, int k, bool on)
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
int ensure_crows(lisreg_ctx* c, Target& t, int k, bool may_decline = false, long long* rows_left = nullptr)
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
        c->prepared = false;
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
        long long budget = (long long)std::max(c->cell_rows_max_mb, 1) * 1048576LL / (long long)(sizeof(float4) * kGraphK + sizeof(float2));
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

int upload_grids(lisreg_ctx* c)
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
void lisreg::ctx_prof_mark(lisreg_ctx* c, int kind_of_next_interval) { prof_mark(c, kind_of_next_interval); }
void lisreg::ctx_prof_collect(lisreg_ctx* c) { if (!c->ev.empty()) prof_collect(c); }

// =============================================================================================================
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
    lisreg_default_params(LISREG_VARIANT_ODOM, &c->params);
    *out = c;
    return LISREG_OK;
}

void lisreg_destroy(lisreg_ctx* c)
{
    if (!c) return;
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
        t.grid_margin[k] = (c->search_mode == 5 || (c->search_mode == 4 && t.crow_chosen[k])) ? kCrowGridMargin : 0;
        make_grid(bb, n, &t.g[k], &t.n_cells[k], t.grid_margin[k]);
        prof_mark(c, 2);
        int rc = build_target_kind(c, t, k);
        t.graph_valid[k] = false;
        t.crow_valid[k] = false; t.crow_too_big[k] = false;
        t.g[k].crow = nullptr; t.g[k].crow_meta = nullptr; t.g[k].crow_tab = nullptr;
        if (!rc && c->search_mode == 3) rc = ensure_graph(c, t, k, true);
        if (!rc && c->search_mode == 5) rc = ensure_crows(c, t, k);
        prof_mark(c, -1);
        if (rc) return rc;
    }
    t.valid = true;
    c->grids_dirty = true;
    c->prepared = false;
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

// ---- batch --------------------------------------------------------------------------------------------------
static bool xcd_order_wanted(const lisreg_ctx* c);

int lisreg_batch_prepare(lisreg_ctx* c, int n_items, const lisreg_item* items, const lisreg_params* params,
                         const float* T_init)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || (n_items > 0 && (!items || !T_init)) || !params) return bad(c, "batch_prepare: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    c->prepared = false;
    c->params = *params;
    c->prm = make_dev_params(*params);
    c->prm.exact = c->exact ? 1 : 0;
    c->prm.ties = (c->canonical_ties || c->exact) ? 1 : 0;
    c->n_items = n_items;
    c->h_blocks.clear(); c->h_segs.clear(); c->h_items.assign((size_t)n_items, ItemState());
    c->batch_slots.clear();
    // front-end of this batch.  The k-NN graph costs ~1 ns per target point and saves ~0.015 ns per query-iteration
    // (MI355X): it pays for shared / long-lived targets (a batch of scans against one submap), not for
    // one-shot targets (a loop-closure candidate pair, a single odometry frame).
    {
        long long total_src = 0;
        double t_pts = 0;
        std::vector<int> seen;
        for (int i = 0; i < n_items; ++i) {
            total_src += (long long)std::max(items[i].n_corner, 0) + (long long)std::max(items[i].n_surf, 0);
            const int sl = items[i].target;
            if (sl >= 0 && (size_t)sl < c->targets.size() && std::find(seen.begin(), seen.end(), sl) == seen.end()) {
                seen.push_back(sl);
                t_pts += (double)c->targets[(size_t)sl].n[0] + (double)c->targets[(size_t)sl].n[1];
            }
        }
        if (total_src > 2000000000LL) return bad(c, "batch_prepare: more than 2e9 source points in one batch");
        c->mode_now = c->search_mode;
        if (c->search_mode == 4) {
            const double qi = (double)total_src * (double)c->prm.bound;
            c->mode_now = (t_pts > 0 && qi >= (double)c->graph_min_ratio * t_pts) ? 3 : 1;
            if (t_pts > 0 && qi >= (double)c->cell_min_ratio * t_pts && t_pts * 5120.0 <= (double)c->cell_rows_max_mb * 1048576.0) c->mode_now = 5;
        }
        // a batch this small cannot fill the chip with one lane per query: eight lanes share a query (k_assoc_walk<.., 8>)
        c->lanes_q = (c->mode_now == 1 && c->lanes_per_query_auto && total_src > 0 && total_src <= 131072) ? 8 : 1;
        // the cell rows re-make a target's grid with a margin the first time they are chosen for it: before anything below reads the geometry
        if (c->mode_now == 5) {
            bool declined = false;
            long long rows_left = (long long)std::max(c->cell_rows_max_mb, 1) * 1048576LL / (long long)(sizeof(float4) * kGraphK + sizeof(float2));
            for (int sl : seen)
                for (int k = 0; k < 2 && !declined; ++k) {
                    Target& t = c->targets[(size_t)sl];
                    if (!t.valid) continue;
                    const bool had = t.crow_valid[k] && t.g[k].crow_tab;
                    int rc = ensure_crows(c, t, k, c->search_mode == 4, c->search_mode == 4 ? &rows_left : nullptr);
                    if (rc) return rc;
                    if (!had) c->grids_dirty = true;
                    declined = c->search_mode == 4 && t.crow_too_big[k];
                }
            if (declined) {
                // (auto only) the rows of the batch's targets would not fit "cell_rows_max_mb" together: the graph scan — and the rows already
                // made for the batch's other targets go back (they would only hold memory)
                c->mode_now = 3;
                for (int sl : seen)
                    for (int k = 0; k < 2; ++k) {
                        Target& t = c->targets[(size_t)sl];
                        if (t.crow_valid[k]) { t.crow[k].release(); t.crow_meta[k].release(); t.crow_valid[k] = false; t.g[k].crow = nullptr; t.g[k].crow_meta = nullptr; t.g[k].crow_tab = nullptr; c->grids_dirty = true; }
                        t.crow_chosen[k] = false;         // (the next set_target of this slot builds its grid without the rows' two-cell margin again)
                    }
            }
        }
    }
    // (after the front-end choice: the cell rows re-make a target's grid with a margin, and the tile count follows the grids)
    // 2-D sort columns of the (optional) source sort: 0.25 m tiles over every item's target footprint.  The bucket count is kept
    // in 64 bits and the tile grows until the whole batch fits 2^26 buckets (km-scale submaps x large batches would otherwise
    // overflow the int32 bucket numbering and ask for gigabytes of histogram).
    float tile = 0.25f;
    for (;;) {
        long long total = 0;
        for (int i = 0; i < n_items; ++i) {
            if (items[i].target < 0 || (size_t)items[i].target >= c->targets.size()) continue;
            for (int k = 0; k < 2; ++k) {
                const GridIndex& g = c->targets[(size_t)items[i].target].g[k];
                total += (long long)std::max(1.0, std::ceil((double)g.nx * g.cell / tile)) * (long long)std::max(1.0, std::ceil((double)g.ny * g.cell / tile));
            }
        }
        if (total <= (1LL << 26)) break;
        tile *= 1.5f;
    }
    const int qpb = kBlockQ / c->lanes_q;                  // queries per workgroup of the kQ-lane search (h_blocks_q)
    c->h_blocks_q.clear();
    int flat = 0, bucket = 0;
    for (int i = 0; i < n_items; ++i) {
        const lisreg_item& in = items[i];
        if (in.fmt != LISREG_FMT_DEVICE) return bad(c, "batch_prepare: items must be LISREG_FMT_DEVICE (use lisreg_align_batch for host clouds)");
        if (in.n_corner < 0 || in.n_surf < 0 || (in.n_corner > 0 && !in.src_corner) || (in.n_surf > 0 && !in.src_surf))
            return bad(c, "batch_prepare: NULL source cloud with n > 0");
        if (in.target < 0 || (size_t)in.target >= c->targets.size() || !c->targets[(size_t)in.target].valid)
            return ctx_fail(c, LISREG_ERR_NO_TARGET, "batch_prepare: item refers to a target slot that was never set");
        if (std::find(c->batch_slots.begin(), c->batch_slots.end(), in.target) == c->batch_slots.end()) c->batch_slots.push_back(in.target);
        const Target& t = c->targets[(size_t)in.target];
        ItemState& st = c->h_items[(size_t)i];
        memset(&st, 0, sizeof st);
        memcpy(st.T_init, T_init + 6 * (size_t)i, 24);
        memcpy(st.T, st.T_init, 24);
        st.degenerate_in = in.degenerate_in;
        st.imu = in.imu;
        st.n_sc = in.n_corner; st.n_ss = in.n_surf;
        if (!(st.n_sc > c->prm.edge_min && st.n_ss > c->prm.surf_min)) ++c->prm.n_guard_failed;      // (:598; the done counter's value after a reset)
        st.blk_begin = (int)c->h_blocks.size();
        for (int k = 0; k < 2; ++k) {
            Segment sg;
            memset(&sg, 0, sizeof sg);
            sg.src = static_cast<const float4*>(k == 0 ? in.src_corner : in.src_surf);
            sg.n = k == 0 ? in.n_corner : in.n_surf;
            sg.item = i; sg.kind = k; sg.target = in.target * 2 + k;
            sg.flat_base = flat; sg.bucket_base = bucket;
            const GridIndex& g = t.g[k];
            sg.tox = g.ox; sg.toy = g.oy; sg.toz = g.oz;
            sg.inv_tile = 1.f / tile;
            sg.tnx = std::max(1, (int)ceilf(g.nx * g.cell / tile));
            sg.tny = std::max(1, (int)ceilf(g.ny * g.cell / tile));
            sg.tnz = 1;
            const int seg_id = (int)c->h_segs.size();
            c->h_segs.push_back(sg);
            for (int s = 0; s < sg.n; s += kBlockQ)
                c->h_blocks.push_back(BlockDesc{ seg_id, s, std::min(kBlockQ, sg.n - s), i });
            if (c->lanes_q > 1)
                for (int s = 0; s < sg.n; s += qpb)
                    c->h_blocks_q.push_back(BlockDesc{ seg_id, s, std::min(qpb, sg.n - s), i });
            flat += sg.n;
            bucket += sg.tnx * sg.tny;
        }
        st.blk_count = (int)c->h_blocks.size() - st.blk_begin;
    }
    c->n_blocks = (int)c->h_blocks.size();
    c->n_segs = (int)c->h_segs.size();
    c->n_elems = flat;
    c->n_buckets = std::max(bucket, 1);
    int rc = LISREG_OK;
    if (c->pack_pending) {                        // sources staged by lisreg_stage_host_items: the device waits for the uploads, the host does not
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->pack_pending, 0));
        c->pack_pending = nullptr;
        c->pack_in_use = c->pack_last;
    }
    HIPCHK(c, c->blocks.ensure(sizeof(BlockDesc) * (size_t)std::max(c->n_blocks, 1)));
    HIPCHK(c, c->segs.ensure(sizeof(Segment) * (size_t)std::max(c->n_segs, 1)));
    HIPCHK(c, c->items.ensure(sizeof(ItemState) * (size_t)std::max(n_items, 1)));
    HIPCHK(c, c->sorted_all.ensure(sizeof(float4) * (size_t)std::max(flat, 1)));
    HIPCHK(c, c->order_all.ensure(sizeof(int) * (size_t)std::max(flat, 1)));
    HIPCHK(c, c->nn.ensure(sizeof(int) * 5 * (size_t)std::max(flat, 1)));
    if (c->lanes_q > 1) {
        HIPCHK(c, c->blocks_q.ensure(sizeof(BlockDesc) * std::max<size_t>(c->h_blocks_q.size(), 1)));
        HIPCHK(c, c->coef.ensure(sizeof(float4) * (size_t)std::max(flat, 1)));
        HIPCHK(c, c->coef_ok.ensure(sizeof(int) * (size_t)std::max(flat, 1)));
    }
    if (c->dump_neighbors) {
        HIPCHK(c, c->dbg_nn.ensure(sizeof(int) * 6 * (size_t)std::max(flat, 1)));
        HIPCHK(c, hipMemsetAsync(c->dbg_nn.p, 0xff, sizeof(int) * 6 * (size_t)std::max(flat, 1), c->stream));
    }
    HIPCHK(c, c->partials.ensure(sizeof(double) * kNumAcc * (size_t)std::max(c->n_blocks, 1)));
    HIPCHK(c, c->results.ensure(sizeof(float) * kResultSize * ((size_t)std::max(n_items, 1) + 1)));      // (+ one record: the run's "row_reach" miss count)
    if (c->trace_cap > 0) HIPCHK(c, c->trace.ensure(sizeof(float) * kTraceStride * (size_t)c->trace_cap * (size_t)std::max(n_items, 1)));
    if (c->mode_now == 3)                        // the mode may have been chosen after the targets were set
        for (int slot : c->batch_slots)
            for (int k = 0; k < 2; ++k) {
                Target& t = c->targets[(size_t)slot];
                if (!t.graph_valid[k] || !t.g[k].nbr) { rc = ensure_graph(c, t, k, true); if (rc) return rc; c->grids_dirty = true; }
            }
    if (c->mode_now == 5)
        for (int slot : c->batch_slots)
            for (int k = 0; k < 2; ++k) {
                Target& t = c->targets[(size_t)slot];
                if (!t.crow_valid[k] || !t.g[k].crow_tab) { rc = ensure_crows(c, t, k); if (rc) return rc; c->grids_dirty = true; }
            }
    for (int slot : c->batch_slots)            // query marks for the row build of every run (option "row_reach"): buffers + the pointer in the grid
        for (int k = 0; k < 2; ++k) {
            rc = ensure_reach(c, c->targets[(size_t)slot], k, c->mode_now == 5 && c->rebuild_targets_each_run && c->row_reach != 0);
            if (rc) return rc;
        }
    if (c->grids_dirty) { rc = upload_grids(c); if (rc) return rc; }
    // table for rebuilding every target index of this batch in ONE launch sequence (rebuild_targets_each_run)
    c->h_tsegs.clear(); c->h_tblocks.clear(); c->h_tchunks.clear();
    int tflat = 0, tbucket = 0, tstrip = 0;
    c->t_max_units = 0; c->t_max_ucells = 0;
    bool strips_fit = true;
    for (int slot : c->batch_slots)
        for (int k = 0; k < 2; ++k) {
            Target& t = c->targets[(size_t)slot];
            TargetSeg ts;
            memset(&ts, 0, sizeof ts);
            ts.raw = t.raw_ptr[k]; ts.sorted_out = t.sorted[k].as<float4>(); ts.cell_start_out = t.cell_start[k].as<int>();
            ts.n = t.n[k]; ts.n_cells = t.n[k] > 0 ? t.n_cells[k] : 0;
            ts.flat_base = tflat; ts.bucket_base = tbucket;
            ts.ox = t.g[k].ox; ts.oy = t.g[k].oy; ts.oz = t.g[k].oz; ts.inv_cell = t.g[k].inv_cell;
            ts.nx = t.g[k].nx; ts.ny = t.g[k].ny; ts.nz = t.g[k].nz;
            ts.grid_id = slot * 2 + k;
            ts.strip_base = tstrip;
            // cells per strip: a batch of one or two targets (a shared submap: configs[1]) wants more, smaller strips than the 2048 cells that suit
            // a batch of hundreds — its strip build is a handful of workgroups (k_strip_build<true> 22 -> 15.6 us with 1024; configs[3] loses
            // 2.7 % with it): "index_strip_cells" = 0 (default) picks by the number of targets in the batch
            const int strip_cells = c->strip_cells > 0 ? c->strip_cells : (c->batch_slots.size() <= 2 ? 1024 : 2048);
            ts.ystrip = std::max(1, std::min(ts.ny, (strip_cells + ts.nz / 2) / std::max(ts.nz, 1)));
            // wide grids: fewer, longer strips so that nx * nstrips stays inside the partition histogram (kMaxStrips bins)
            if (ts.nx > 0 && ts.nx <= kMaxStrips) {
                const int max_nstrips = std::max(1, kMaxStrips / ts.nx);
                ts.ystrip = std::max(ts.ystrip, (ts.ny + max_nstrips - 1) / max_nstrips);
            }
            ts.nstrips = (ts.ny + ts.ystrip - 1) / ts.ystrip;
            const int id = (int)c->h_tsegs.size();
            c->h_tsegs.push_back(ts);
            for (int s = 0; s < ts.n; s += kBlockQ) c->h_tblocks.push_back(BlockDesc{ id, s, std::min(kBlockQ, ts.n - s), 0 });
            for (int s = 0; s < ts.n; s += kPartChunkHost) c->h_tchunks.push_back(BlockDesc{ id, s, std::min(kPartChunkHost, ts.n - s), 0 });
            tflat += ts.n; tbucket += ts.n_cells;
            if (ts.n > 0) {
                const int units = ts.nx * ts.nstrips;
                tstrip += units; c->t_max_units = std::max(c->t_max_units, units); c->t_max_ucells = std::max(c->t_max_ucells, ts.ystrip * ts.nz);
                strips_fit = strips_fit && units <= kMaxStrips;
            }
        }
    c->t_elems = tflat; c->t_buckets = std::max(tbucket, 1); c->t_strips = tstrip;
    strips_fit = strips_fit && ((size_t)c->t_max_ucells + 1) * 4 + (size_t)c->strip_cap * 6 + 8192 <= kStripLdsLarge;
    // auto = the strip form whenever the grids fit it: measured faster from 2 own-target items up (index 0.063 vs 0.078 ms) to 256
    // (2.2 vs 5.3 ms), and equal for the single shared submap of configs[1]
    c->strip_now = strips_fit && c->index_build != 0;
    if (c->index_build == 1 && !c->strip_now)
        return bad(c, "index_build 1: a target grid of this batch does not fit the strip form (strips per target or cells per strip)");
    HIPCHK(c, c->tchunk_dev.ensure(sizeof(BlockDesc) * std::max<size_t>(c->h_tchunks.size(), 1)));
    { const void* before = c->strip_tab.p; HIPCHK(c, c->strip_tab.ensure(sizeof(int) * (3 * ((size_t)tstrip + 4) + (size_t)tstrip / 2048 + 8))); if (c->strip_tab.p != before) c->strip_zero_ints = 0; }
    HIPCHK(c, c->tseg_dev.ensure(sizeof(TargetSeg) * std::max<size_t>(c->h_tsegs.size(), 1)));
    HIPCHK(c, c->tblk_dev.ensure(sizeof(BlockDesc) * std::max<size_t>(c->h_tblocks.size(), 1)));
    // every table crosses PCIe from ONE pinned staging buffer: five asynchronous copies, no host synchronisation
    // (pageable sources would make each hipMemcpyAsync a blocking staged copy — most of a single registration's latency)
    {
        struct Part { const void* src; size_t bytes; void* dst; };
        const Part parts[7] = {
            { c->h_tchunks.data(), sizeof(BlockDesc) * c->h_tchunks.size(), c->tchunk_dev.p },
            { c->h_blocks_q.data(), sizeof(BlockDesc) * c->h_blocks_q.size(), c->blocks_q.p },
            { c->h_blocks.data(), sizeof(BlockDesc) * (size_t)c->n_blocks, c->blocks.p },
            { c->h_segs.data(), sizeof(Segment) * (size_t)c->n_segs, c->segs.p },
            { c->h_items.data(), sizeof(ItemState) * (size_t)n_items, c->items.p },
            { c->h_tsegs.data(), sizeof(TargetSeg) * c->h_tsegs.size(), c->tseg_dev.p },
            { c->h_tblocks.data(), sizeof(BlockDesc) * c->h_tblocks.size(), c->tblk_dev.p } };
        size_t total = 0;
        for (const Part& pt : parts) total += (pt.bytes + 63) & ~(size_t)63;
        if (c->stage_done) HIPCHK(c, hipEventSynchronize(c->stage_done));      // the previous batch's copies have left the buffer
        else HIPCHK(c, c->stage_done.create(hipEventDisableTiming));
        HIPCHK(c, c->stage_host.ensure(total, total + total / 2 + 4096));
        unsigned char* stage = c->stage_host.as<unsigned char>();
        size_t off = 0;
        for (const Part& pt : parts) {
            if (pt.bytes) {
                memcpy(stage + off, pt.src, pt.bytes);
                HIPCHK(c, hipMemcpyAsync(pt.dst, stage + off, pt.bytes, hipMemcpyHostToDevice, c->stream));
            }
            off += (pt.bytes + 63) & ~(size_t)63;
        }
        HIPCHK(c, hipEventRecord(c->stage_done, c->stream));
    }
    // sort_sources: scan order and voxel-grid order are spatially coherent and beat a re-sort; an arbitrary order costs
    // the cell walk its L1 locality (2x slower), so in auto mode a cheap probe decides once per prepared batch.  Small batches
    // (a single odometry frame) skip the probe and its host round trip: a sort could not pay for itself there.
    c->sort_now = c->sort_sources == 1;
    // (the probe costs a pass over the sources and a host round trip — 0.15 ms in front of a pipelined batch: batches of the same shape as
    // the one last probed reuse its verdict, re-probed every 32nd; the verdict never changes the neighbours, only the order in which a
    // workgroup sums its rows — the last bits of the poses)
    if (c->sort_sources == 2 && c->n_elems >= 65536 && c->probe_items == n_items && c->probe_elems == c->n_elems && c->probe_age < 32) {
        ++c->probe_age;
        c->sort_now = c->probe_verdict;
    } else
    if (c->sort_sources == 2 && c->n_elems >= 65536) {
        launch_count_jumps(c->blocks.as<BlockDesc>(), c->n_blocks, c->segs.as<Segment>(), 1.5f, c->done_dev.as<int>(), c->stream);
        int jumps_stack = 0;
        int* jumps = c->done_host.p ? c->done_host.as<int>() : &jumps_stack;       // lisreg_create tolerates a failed pinned allocation
        HIPCHK(c, hipMemcpyAsync(jumps, c->done_dev.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->sort_now = (double)*jumps > 0.25 * (double)c->n_elems;
        c->probe_verdict = c->sort_now; c->probe_items = n_items; c->probe_elems = c->n_elems; c->probe_age = 0;
    }
    // scratch of the bucket sorts: the target rebuild (if the batch does that) and the source sort (only if it will run)
    {
        const size_t se = (size_t)std::max(c->rebuild_targets_each_run ? tflat : 1, c->sort_now ? flat : 1);
        const size_t sbk = (size_t)std::max(c->rebuild_targets_each_run ? c->t_buckets : 1, c->sort_now ? c->n_buckets : 1);
        rc = ensure_sort_scratch(c, se, sbk);
        if (rc) return rc;
    }
    // The registrations start reset (pose caches of the initial poses, done counter = the guard failures): every run leaves them reset again
    // for the next one (launch_finalize), so a run has no reset launch of its own.  The "row_reach" miss count is cumulative from here.
    launch_reset_items(c->items.as<ItemState>(), c->n_items, c->prm, c->done_dev.as<int>(), c->stream,
                       reinterpret_cast<int*>(c->results.as<float>() + (size_t)std::max(c->n_items, 1) * kResultSize));
    c->items_reset = true; c->reach_miss_seen = 0; c->runs_since_fetch = 0;
    // Query marks for the row builds of this batch's runs (option "row_reach"; cell rows, targets rebuilt inside every run).  A scan sees a
    // part of its map — the lidar's elevation span leaves the upper walls of the benchmark room unseen: a fifth of the cells that would
    // get rows — so every run builds rows only for the cells a query comes within a metre of under its INITIAL pose: one pass over the
    // batch's source points (k_query_marks: the cell each falls into), those marks grown by ceil(1 m / cell) cells (`reach`, read by the
    // classification of every run).  The mark words are cleared in front of the marking and kept: "row_reach" = 2 reads them as well (the
    // cells a query starts in).  Both depend on the sources and the initial poses — what this call is given — not on the target's points,
    // which a run may find changed.
    c->reach_ready = false;
    if (c->reach_backoff > 0) --c->reach_backoff;
    else if (c->mode_now == 5 && c->rebuild_targets_each_run && c->row_reach != 0 && c->lanes_q == 1 && c->n_blocks > 0) {
        bool any = false;
        for (int slot : c->batch_slots) for (int k = 0; k < 2; ++k) any = any || (c->targets[(size_t)slot].g[k].qmark != nullptr && c->targets[(size_t)slot].n[k] > 0);
        if (any) {
            for (int slot : c->batch_slots)
                for (int k = 0; k < 2; ++k) {
                    Target& t = c->targets[(size_t)slot];
                    if (!t.g[k].qmark || t.n[k] <= 0) continue;
                    HIPCHK(c, hipMemsetAsync(t.g[k].qmark, 0, sizeof(unsigned) * (size_t)t.g[k].nx * (size_t)t.g[k].ny * (size_t)t.g[k].qmark_w, c->stream));
                }
            launch_query_marks(c->blocks.as<BlockDesc>(), c->n_blocks, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(), c->items.as<ItemState>(), c->stream);
            for (int slot : c->batch_slots)
                for (int k = 0; k < 2; ++k) {
                    Target& t = c->targets[(size_t)slot];
                    if (!t.g[k].qmark || t.n[k] <= 0) continue;
                    launch_reach_dilate(t.g[k], t.crow_reach[k].as<unsigned>(), c->stream);
                }
            HIPCHK(c, hipGetLastError());
            c->reach_ready = true;
        }
    }
    // The dispatch order of the runs' correspondence launches (blocks ranked by the sector their queries fall into, one eighth per XCD) is a
    // function of the same inputs — block descriptors, sources, initial poses, grid geometry: made here once instead of by every run
    // (k_xcd_keys + a single-workgroup counting sort: 70 us per run on the side stream, which the shorter row build of "row_reach" had turned
    // into the tail of a run's index phase).  Runs that sort their sources or split the batch in halves keep making their own.
    c->xcd_cached = false;
    if (xcd_order_wanted(c) && !c->sort_now && !c->exact && c->n_blocks > 0) {
        HIPCHK(c, c->xcd_tab.ensure(sizeof(int) * 2 * (size_t)c->n_blocks));
        launch_xcd_order(c->blocks.as<BlockDesc>(), c->n_blocks, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(), c->items.as<ItemState>(),
                         nullptr, c->batch_slots.size() >= 8 && c->xcd_order == 1, c->xcd_tab.as<int>(), c->xcd_tab.as<int>() + c->n_blocks, c->stream);
        HIPCHK(c, hipGetLastError());
        c->xcd_cached = true;
    }
    c->prepared = true;
    return LISREG_OK;
}

// exact_arithmetic: the sine and cosine of the three pose angles are taken by the HOST's libm — the library the reference's
// pcl::getTransformation and LMOptimization call (cosf / sinf on x86-64) — because no device routine returns its last bit in every case
// (1 configuration in 100 showed a 1-ulp matrix entry, which swapped two candidates 8e-7 apart in squared distance).  One 24-byte-per-item
// round trip per Gauss-Newton iteration; only this build pays it.
static int exact_pose_caches(lisreg_ctx* c)
{
    const size_t n = (size_t)c->n_items;
    if (n == 0) return LISREG_OK;
    HIPCHK(c, c->exact_trig.ensure(sizeof(float) * 6 * n));
    std::vector<float> T(6 * n), trig(6 * n);
    launch_pose_gather(c->items.as<ItemState>(), c->n_items, c->exact_trig.as<float>(), c->stream);
    HIPCHK(c, hipMemcpyAsync(T.data(), c->exact_trig.p, sizeof(float) * 6 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        const float* t = &T[6 * i];
        float* g = &trig[6 * i];
        g[0] = cosf(t[2]); g[1] = sinf(t[2]); g[2] = cosf(t[1]); g[3] = sinf(t[1]); g[4] = cosf(t[0]); g[5] = sinf(t[0]);
    }
    HIPCHK(c, hipMemcpyAsync(c->exact_trig.p, trig.data(), sizeof(float) * 6 * n, hipMemcpyHostToDevice, c->stream));
    launch_pose_cache_from_trig(c->items.as<ItemState>(), c->n_items, c->exact_trig.as<float>(), c->stream);
    HIPCHK(c, hipStreamSynchronize(c->stream));          // `trig` is a local
    return LISREG_OK;
}

// GN iterations kWideFrom..kWideUntil walk centre-first (no seeds, or seeds a pose step off).  Batches searched with eight lanes per query
// (single frames, sequential use) start at kWideFromSmall: their first guess is usually a frame step off, and the radius-limited first pass of
// the plain walk then settles iteration 0 in 160-200 us instead of 230-310 (replay of configs[2]); 1 % slower on a single frame with a
// 2-degree error (configs[0] stand-in).  The graph scan (search_mode 3) runs the centre-first fall-back walk until kGraphWideUntil; the cell
// rows (search_mode 5) never do (1.4 % of the queries walk at iteration 0: the plain kernel's iteration 0 takes 317 us against 330 with the
// centre-first variant, iteration 1 201 against 205; same neighbours).
constexpr int kWideFrom = 0, kWideFromSmall = 1, kWideUntil = 2, kGraphWideUntil = 1;
constexpr int kGraphHops = 3;              // search_mode 3: neighbour lists scanned per query (anchor, then nearest found, ...) before the walk takes over

// XCD-aware dispatch order for the prepared batch? (see run_impl)
static bool xcd_order_wanted(const lisreg_ctx* c)
{
    const bool many_targets = c->batch_slots.size() >= 8 && c->xcd_order == 1;
    return c->lanes_q != 8 &&
           (((c->mode_now == 3 || c->mode_now == 5) && (c->xcd_order == 1 || (c->xcd_order == 2 && c->n_blocks >= 2048 && c->n_items >= 32))) ||
            (many_targets && c->xcd_order != 0 && c->n_blocks >= 2048));
}

// Enqueue one full pass.  early_stop (synchronous entry points only): after every few iterations the host reads a
// 4-byte "registrations finished" counter and stops launching once every item has converged — the reference's
// `break` at :617 — instead of launching no-op kernels up to max_iters.  Results are identical either way.
static int run_impl(lisreg_ctx* c, bool early_stop)
{
    if (!c->prepared) return bad(c, "batch_run: no prepared batch");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    // XCD-aware dispatch order (lisreg_assoc.hip, launch_xcd_order): two small launches per run, at the initial poses.  Auto: the graph
    // front-end with >= 32 registrations (measured: +2.5 % at 64 scans, +4.9 % at 256; with 8 big scans the sectors are unevenly loaded
    // and it costs 2 %; the walk front-end gains nothing)
    // Round 5: a batch whose registrations bring targets of their own (configs[3]: 256 candidate pairs, 256 x 6 MB of index) takes the order
    // by TARGET whatever the front-end — whole targets per XCD, so that an L2 holds the one or two targets its CUs are working on instead of
    // a slice of all eight-plus in flight.
    // (measured on configs[3], 256 own-target registrations through the cell walk: 13 539 reg/s against 13 716 in plain order — no gain, the walk
    //  is not bound by L2 misses either; the order by target is taken only with xcd_order = 1, profiles/r05_kernel_experiments.md)
    const bool many_targets = c->batch_slots.size() >= 8 && c->xcd_order == 1;
    c->xcd_now = xcd_order_wanted(c);
    if (c->xcd_now) HIPCHK(c, c->xcd_tab.ensure(sizeof(int) * 2 * (size_t)c->n_blocks));
    // Two halves of the batch on two streams (round 5).  The 6x6 solves are one workgroup per registration and ~13 us of dependent latency
    // between two correspondence launches: the chip idles through ten of them per step.  Registrations are independent, so the batch is cut
    // in two at an item boundary near the middle of the workgroups: the first half iterates on the context's stream, the second on the side
    // stream, and each half's solve (and launch gaps, and the thinning tail of its correspondence launch) runs underneath the other half's
    // correspondence launch.  Same kernels on the same data in the same order per registration: same results to the bit.  Only for runs
    // that do not stop early from the host (fixed iteration counts, lisreg_batch_run) and are big enough to fill the chip twice.
    const bool can_stop = early_stop && c->prm.fixed_iters <= 0 && c->done_host.p && c->early_stop_chunk != 0;
    int split_item = 0, split_blk = 0;
    if (c->interleave != 0 && !c->exact && !can_stop && c->lanes_q == 1 && c->n_items >= 2 && c->n_blocks >= c->interleave_min_blocks) {
        ensure_side_stream(c);
        if (c->side_stream && !c->ev_ab && (c->ev_ab.create(hipEventDisableTiming) != hipSuccess ||
                                            c->ev_ba.create(hipEventDisableTiming) != hipSuccess)) { c->ev_ab.reset(); c->ev_ba.reset(); }
        if (c->side_stream) {
            for (int i = 1; i < c->n_items; ++i)
                if (c->h_items[(size_t)i].blk_begin * 2 >= c->n_blocks) { split_item = i; split_blk = c->h_items[(size_t)i].blk_begin; break; }
            if (split_blk * 4 < c->n_blocks || (c->n_blocks - split_blk) * 4 < c->n_blocks) { split_item = 0; split_blk = 0; }     // (a lop-sided cut hides nothing)
        }
    }
    // Round 6, option "row_reach": the rows of this run are built only for the cells a query of the batch comes within a metre of under
    // its initial pose (`reach` words made by lisreg_batch_prepare: they depend on the sources and the initial poses alone, not on the target's
    // points).  A query that ends up in a cell without rows all the same takes the cell walk: results cannot depend on the marks.
    c->reach_now = c->rebuild_targets_each_run && c->mode_now == 5 && c->reach_ready && !c->exact;
    int* const miss_dev = reinterpret_cast<int*>(c->results.as<float>() + (size_t)std::max(c->n_items, 1) * kResultSize);
    c->prm.reach_miss = c->reach_now ? miss_dev : nullptr;
    // (the registrations are reset already — by lisreg_batch_prepare or by the run before, launch_finalize — unless a run ended in an error)
    const bool reset_done = c->items_reset;
    c->items_reset = false;
    if (c->rebuild_targets_each_run) {                 // the reference rebuilds both kd-trees per registration (:602-603)
        prof_mark(c, 2);
        if (c->strip_now) {
            StripBuffers sl;
            sl.cnt = c->strip_tab.as<int>(); sl.fill = sl.cnt + (c->t_strips + 1); sl.start = sl.fill + (c->t_strips + 1);
            sl.scan_tmp = sl.start + (c->t_strips + 2);
            sl.tmp_pts = c->tmp_pts.as<float4>(); sl.slot_idx = c->elem_bucket.as<uint32_t>(); sl.slot_pos = c->elem_sub.as<uint32_t>();
            ensure_side_stream(c);                    // failure just means the two variants run back to back
            sl.side = c->side_stream; sl.ev_fork = c->ev_fork; sl.ev_join = c->ev_join;
            if (launch_build_targets_strips(c->tchunk_dev.as<BlockDesc>(), (int)c->h_tchunks.size(), c->tseg_dev.as<TargetSeg>(),
                                            (int)c->h_tsegs.size(), c->t_strips, c->t_max_units, c->t_max_ucells, c->strip_cap, sl, st, &c->strip_zero_ints))
                return ctx_fail(c, LISREG_ERR_HIP, "strip index build: LDS configuration refused");
        } else
            launch_build_targets_batched(c->tblk_dev.as<BlockDesc>(), (int)c->h_tblocks.size(), c->tseg_dev.as<TargetSeg>(),
                                         (int)c->h_tsegs.size(), c->t_elems, c->t_buckets, sort_buffers(c), st);
        if (c->mode_now == 3)
            launch_build_graph(c->tblk_dev.as<BlockDesc>(), (int)c->h_tblocks.size(), c->tseg_dev.as<TargetSeg>(),
                               c->grids_dev.as<GridIndex>(), st);
        if (c->mode_now == 5) {
            // corner and surf target of a slot in ONE launch sequence on this stream (launch_crow_rows_pair): no side stream, no event hops
            for (int slot : c->batch_slots) {
                Target& t = c->targets[(size_t)slot];
                const GridIndex g2[2] = { t.g[0], t.g[1] };
                const int nc2[2] = { t.n_cells[0], t.n_cells[1] };
                const lisreg::CrowBuffers cb2[2] = { crow_buffers(t, 0, c->reach_now, c->row_reach == 2), crow_buffers(t, 1, c->reach_now, c->row_reach == 2) };
                int* oz2[2] = { &t.omask_zero[0], &t.omask_zero[1] };
                launch_crow_rows_pair(g2, nc2, cb2, st, oz2);
            }
        }
        prof_mark(c, -1);
    }
    if (!reset_done) launch_reset_items(c->items.as<ItemState>(), c->n_items, c->prm, c->done_dev.as<int>(), st);
    if (c->exact) { int rc = exact_pose_caches(c); if (rc) return rc; }
    prof_mark(c, 2);
    launch_sort_sources(c->blocks.as<BlockDesc>(), c->n_blocks, c->segs.as<Segment>(), c->n_segs, c->items.as<ItemState>(),
                        c->n_elems, c->sort_now ? c->n_buckets : 0, sort_buffers(c), c->sorted_all.as<float4>(), c->order_all.as<int>(), st);
    prof_mark(c, -1);
    if (c->xcd_now && !(c->xcd_cached && split_blk == 0)) {      // (after the source sort: the keys read the sorted records)
        // (an interleaved run dispatches its halves separately: one table per half, positions and ids relative to the half)
        const int nb0 = split_blk ? split_blk : c->n_blocks;
        launch_xcd_order(c->blocks.as<BlockDesc>(), nb0, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(), c->items.as<ItemState>(),
                         c->sort_now ? c->sorted_all.as<float4>() : nullptr, many_targets, c->xcd_tab.as<int>(), c->xcd_tab.as<int>() + c->n_blocks, st);
        if (split_blk) {
            launch_xcd_order(c->blocks.as<BlockDesc>() + split_blk, c->n_blocks - split_blk, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(),
                             c->items.as<ItemState>(), c->sort_now ? c->sorted_all.as<float4>() : nullptr, many_targets,
                             c->xcd_tab.as<int>() + split_blk, c->xcd_tab.as<int>() + c->n_blocks + split_blk, st);
            // the half tables have overwritten the batch's table from lisreg_batch_prepare: a later unsplit run of this batch (interleave
            // switched off, interleave_min_blocks raised) must make its own instead of reading half-relative ids as whole-batch ones
            c->xcd_cached = false;
        }
    }
    // how often the host looks at the "registrations finished" counter: a skipped launch of a big batch still dispatches tens of
    // thousands of workgroups (check every 3 iterations), a skipped launch of a single frame costs ~2 us (check every 6: one
    // round trip for the typical 3-6 iteration registration)
    const int chunk = c->early_stop_chunk > 0 ? c->early_stop_chunk : (c->n_blocks <= 1024 ? 6 : 3);
    // sequential use: the last batch fetched from this context needed `last_launches` iterations — frames of a drive converge alike, so the
    // first look is taken right there (a replay frame converges in 3: three no-op iterations, nine launches, not enqueued), later looks every 3
    int next_check = chunk;
    if (c->early_stop_chunk <= 0 && c->last_launches > 0) next_check = std::max(2, std::min(c->last_launches, chunk));
    c->prm.cell_anchor_until = c->cell_anchor_until;
    // one Gauss-Newton iteration of the items [i0, i0 + ni) = the workgroups [b0, b0 + nb) on stream s_ (sidx: which stream the profiling marks go on)
    // (after_assoc: an event recorded right behind the correspondence launch, for the alternation of an interleaved run)
    auto iteration = [&](int it, int i0, int ni, int b0, int nb, hipStream_t s_, int sidx, hipEvent_t after_assoc) {
        if (!after_assoc) prof_mark(c, 0, sidx);          // (an alternating run marks behind its wait for the other half)
        (c->exact ? launch_assoc_exact : launch_assoc)(
                     c->blocks.as<BlockDesc>() + b0, nb, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(),
                     c->items.as<ItemState>(), c->prm, c->sort_now ? c->sorted_all.as<float4>() : nullptr, c->partials.as<double>() + (size_t)b0 * kNumAcc,
                     c->mode_now, c->nn.as<int>(), c->n_elems, c->first_pass_r * c->first_pass_r,
                     c->mode_now != 5 && it >= (c->lanes_q == 8 ? kWideFromSmall : kWideFrom) && it <= (c->mode_now == 3 ? kGraphWideUntil : kWideUntil), kGraphHops,
                     c->count_searches ? c->counters.as<unsigned long long>() : nullptr,
                     c->dump_neighbors ? c->dbg_nn.as<int>() : nullptr, c->lanes_q,
                     c->blocks_q.as<BlockDesc>(), (int)c->h_blocks_q.size(), c->coef.as<float4>(), c->coef_ok.as<int>(),
                     c->xcd_now ? c->xcd_tab.as<int>() + c->n_blocks + b0 : nullptr, s_);
        if (after_assoc) (void)hipEventRecord(after_assoc, s_);
        prof_mark(c, 1, sidx);
        launch_solve(c->items.as<ItemState>() + i0, ni, c->prm, c->partials.as<double>(),
                     c->trace_cap > 0 ? c->trace.as<float>() + (size_t)i0 * (size_t)c->trace_cap * kTraceStride : nullptr, c->trace_cap, c->done_dev.as<int>(), s_);
        prof_mark(c, -1, sidx);
    };
    c->interleaved_now = false;
    if (split_blk > 0 && hipEventRecord(c->ev_fork, st) == hipSuccess && hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) == hipSuccess) {
        c->interleaved_now = true;
        // interleave 1: the two correspondence launches ALTERNATE (each waits for the other half's previous one through an event), so that
        // every launch has the chip to itself apart from the other half's solve — per-launch durations stay what they are for a launch
        // alone, which is what the roofline figures of bench.py and the profiler tables are made of; 2: free-running (the launches of the
        // two streams share the chip whenever both are ready: same throughput, launch durations no longer comparable)
        const bool alternate = c->interleave == 1 && c->ev_ab && c->ev_ba;
        // a failing event call must not leave work of the second half un-joined on the side stream (the caller's next fetch on `st` would race
        // with it): on any failure the side stream is drained by the HOST before the error is returned, and the run counts as not interleaved
        hipError_t ie = hipSuccess;
        for (int it = 0; it < c->prm.bound && ie == hipSuccess; ++it) {
            if (alternate && it > 0) ie = hipStreamWaitEvent(st, c->ev_ba, 0);                   // B's launch of the iteration before is through
            if (ie != hipSuccess) break;
            if (alternate) prof_mark(c, 0, 0);
            iteration(it, 0, split_item, 0, split_blk, st, 0, alternate ? c->ev_ab : nullptr);
            if (alternate) ie = hipStreamWaitEvent(c->side_stream, c->ev_ab, 0);                 // A's launch of this iteration is through
            if (ie != hipSuccess) break;
            if (alternate) prof_mark(c, 0, 1);
            iteration(it, split_item, c->n_items - split_item, split_blk, c->n_blocks - split_blk, c->side_stream, 1, alternate ? c->ev_ba : nullptr);
        }
        if (ie == hipSuccess) ie = hipEventRecord(c->ev_join, c->side_stream);
        if (ie == hipSuccess) ie = hipStreamWaitEvent(st, c->ev_join, 0);
        if (ie != hipSuccess) {
            (void)hipStreamSynchronize(c->side_stream);
            c->interleaved_now = false;
            return ctx_fail(c, LISREG_ERR_HIP, std::string("interleaved run: ") + hipGetErrorString(ie));
        }
    } else
    for (int it = 0; it < c->prm.bound; ++it) {
        iteration(it, 0, c->n_items, 0, c->n_blocks, st, 0, nullptr);
        if (c->exact && it + 1 < c->prm.bound) { int rc = exact_pose_caches(c); if (rc) return rc; }
        if (can_stop && it + 1 == next_check && it + 1 < c->prm.bound) {
            HIPCHK(c, hipMemcpyAsync(c->done_host.p, c->done_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (*c->done_host.as<int>() >= c->n_items) break;
            next_check += c->early_stop_chunk > 0 ? chunk : std::min(chunk, 3);
        }
    }
    launch_finalize(c->items.as<ItemState>(), c->n_items, c->prm, c->results.as<float>(), st, c->done_dev.as<int>());      // (+ reset for the next run)
    c->items_reset = true; ++c->runs_since_fetch;
    HIPCHK(c, hipGetLastError());
    if (c->pack_in_use >= 0 && c->pack_free[c->pack_in_use])      // the staged source buffer may be overwritten once this run is through
        HIPCHK(c, hipEventRecord(c->pack_free[c->pack_in_use], st));
    return LISREG_OK;
}

int lisreg_batch_run(lisreg_ctx* c)
{
    if (!c) return LISREG_ERR_ARG;
    return run_impl(c, false);
}

int lisreg_batch_fetch(lisreg_ctx* c, float* T, lisreg_stats* stats)
{
    if (!c) return LISREG_ERR_ARG;
    if (!c->prepared) return bad(c, "batch_fetch: no prepared batch");
    HIPCHK(c, hipSetDevice(c->device));
    // results (and, for lisreg_align, the trace) land in pinned memory: asynchronous copies, ONE synchronisation
    const size_t res_floats = ((size_t)std::max(c->n_items, 1) + 1) * kResultSize;
    const size_t trace_floats = c->fetch_trace_records > 0 ? (size_t)kTraceStride * (size_t)c->fetch_trace_records : 0;
    const size_t fetch_bytes = (res_floats + trace_floats) * sizeof(float);
    HIPCHK(c, c->fetch_host.ensure(fetch_bytes, fetch_bytes * 2 + 4096));
    float* fetched = c->fetch_host.as<float>();
    const bool with_miss = c->n_items > 0 && c->reach_now;
    if (c->n_items) HIPCHK(c, hipMemcpyAsync(fetched, c->results.p, sizeof(float) * kResultSize * ((size_t)c->n_items + (with_miss ? 1 : 0)), hipMemcpyDeviceToHost, c->stream));
    if (trace_floats && c->trace.p) HIPCHK(c, hipMemcpyAsync(fetched + res_floats, c->trace.p, sizeof(float) * trace_floats, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->h_results.assign(fetched, fetched + res_floats);
    if (with_miss) {
        // "row_reach" watches itself: the marks are the queries' cells under their INITIAL poses grown by a metre; a batch whose first steps move
        // its points farther than that sends queries into cells without rows, where they walk (exact, but slow: configs[4] with a 0.5 m
        // dilation ran 30 % longer).  More than one query-iteration in a thousand there: the prepared batch's later runs, and the next 32
        // batches prepared on this context, build all rows.
        int cum; memcpy(&cum, fetched + (size_t)c->n_items * kResultSize, sizeof cum);      // (cumulative since the batch was prepared)
        const int miss = cum - c->reach_miss_seen;
        c->reach_miss_seen = cum;
        c->reach_miss_last = miss;
        if ((long long)miss * 1000LL > (long long)c->n_elems * (long long)std::max(c->prm.bound, 1) * (long long)std::max(c->runs_since_fetch, 1)) { c->reach_ready = false; c->reach_backoff = 32; }
    }
    if (!c->ev.empty()) prof_collect(c);          // events of every profiled run since the last fetch (profiling may be off again by now)
    c->last_launches = 0;
    for (int i = 0; i < c->n_items; ++i) {
        const float* r = &c->h_results[(size_t)i * kResultSize];
        c->last_launches = std::max(c->last_launches, (int)r[6] + 1);
        if (T) memcpy(T + 6 * (size_t)i, r, 24);
        if (stats) {
            stats[i].iters = (int)r[6]; stats[i].deltaR = r[7]; stats[i].deltaT = r[8];
            stats[i].degenerate = (int)r[9]; stats[i].n_corr_last = (int)r[10]; stats[i].status = (int)r[11];
        }
    }
    c->runs_since_fetch = 0;
    return LISREG_OK;
}

void* lisreg_batch_result_device(const lisreg_ctx* c) { return c ? c->results.p : nullptr; }

// Options that are not part of the reference's parameter surface (kept out of lisreg_params on purpose).
int lisreg_set_option(lisreg_ctx* c, const char* name, int value)
{
    if (!c || !name) return LISREG_ERR_ARG;
    if (!strcmp(name, "rebuild_targets_each_run")) {
        c->rebuild_targets_each_run = value != 0;
        if (c->prepared && c->rebuild_targets_each_run) {      // the rebuild needs its sort scratch
            int rc = ensure_sort_scratch(c, (size_t)std::max(c->t_elems, 1), (size_t)std::max(c->t_buckets, 1));
            if (rc) return rc;
        }
        return LISREG_OK;
    }
    if (!strcmp(name, "sort_sources")) { c->sort_sources = value; c->probe_items = -1; return LISREG_OK; }
    if (!strcmp(name, "cell_anchor_until")) { c->cell_anchor_until = std::max(value, 0); return LISREG_OK; }
    if (!strcmp(name, "search_mode")) {
        if (value < 1 || value > 5 || value == 2) return bad(c, "search_mode: 1 cell walk, 3 k-NN graph scan, 4 auto, 5 cell rows");
        c->search_mode = value; c->prepared = false; return LISREG_OK;
    }
    if (!strcmp(name, "graph_min_ratio")) { c->graph_min_ratio = value; c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "cell_min_ratio")) { c->cell_min_ratio = value; c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "row_reach")) {
        if (value < 0 || value > 2) return bad(c, "row_reach: 0 all rows, 1 rows within a metre of the queries, 2 of those the cells near the target or a query");
        c->row_reach = value; c->reach_backoff = 0; c->prepared = false; return LISREG_OK;
    }
    if (!strcmp(name, "cell_rows_max_mb")) {
        c->cell_rows_max_mb = value; c->prepared = false;
        for (auto& t : c->targets) for (int k = 0; k < 2; ++k) {        // a new bound: what was too big may fit now, what fitted may have to be capped
            t.crow_too_big[k] = false;
            if (t.crow_valid[k]) { t.crow_valid[k] = false; c->grids_dirty = true; }
        }
        return LISREG_OK;
    }
    if (!strcmp(name, "early_stop_chunk")) { c->early_stop_chunk = value; return LISREG_OK; }
    if (!strcmp(name, "xcd_order")) { if (value < 0 || value > 2) return bad(c, "xcd_order: 0 off, 1 on, 2 auto"); c->xcd_order = value; c->xcd_cached = false; return LISREG_OK; }
    if (!strcmp(name, "index_build")) {
        if (value < 0 || value > 2) return bad(c, "index_build: 0 bucket sort, 1 strip form, 2 auto");
        c->index_build = value; c->prepared = false;
        return LISREG_OK;
    }
    if (!strcmp(name, "index_strip_cells")) { c->strip_cells = std::max(value, 0); c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "index_strip_cap")) { c->strip_cap = std::min(std::max(value, 64), 16384); c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "count_searches")) {
        c->count_searches = value != 0;
        if (c->count_searches) { HIPCHK(c, c->counters.ensure(128 * 8)); HIPCHK(c, hipMemsetAsync(c->counters.p, 0, 128 * 8, c->stream)); }   // behind a counting run still queued
        return LISREG_OK;
    }
    if (!strcmp(name, "lanes_per_query")) { c->lanes_per_query_auto = value != 1; c->prepared = false; return LISREG_OK; }   // 1 forces one lane per query, anything else = auto
    if (!strcmp(name, "dump_neighbors")) { c->dump_neighbors = value != 0; c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "exact_arithmetic")) { c->exact = value != 0; c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "feeder_copy_engine")) { c->feeder_engine = value; return LISREG_OK; }
    if (!strcmp(name, "canonical_ties")) { c->canonical_ties = value != 0; c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "first_pass_mm")) {          // (a negative radius would square to the positive one: refused rather than taken as that)
        if (value < 0) return bad(c, "first_pass_mm: a radius in millimetres, >= 0");
        c->first_pass_r = 1e-3f * (float)value; return LISREG_OK;
    }
    if (!strcmp(name, "trace_cap")) { c->trace_cap = std::max(0, value); c->prepared = false; return LISREG_OK; }
    if (!strcmp(name, "feeder_threads")) { c->feeder_threads = std::min(std::max(value, 0), 64); return LISREG_OK; }
    if (!strcmp(name, "feeder_numa")) { c->feeder_numa = value != 0; return LISREG_OK; }       // takes effect when the thread pool is created
    if (!strcmp(name, "interleave_min_blocks")) { c->interleave_min_blocks = std::max(value, 2); return LISREG_OK; }
    if (!strcmp(name, "interleave")) { if (value < 0 || value > 2) return bad(c, "interleave: 0 off, 1 alternating halves, 2 free-running halves"); c->interleave = value; return LISREG_OK; }
    return bad(c, std::string("set_option: unknown option ") + name);
}

int lisreg_get_option(const lisreg_ctx* c, const char* name, int* value)
{
    if (!c || !name || !value) return LISREG_ERR_ARG;
    if (!strcmp(name, "search_mode")) { *value = c->search_mode; return LISREG_OK; }
    if (!strcmp(name, "exact_arithmetic")) { *value = c->exact ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "feeder_chunks_by_copy_engine")) { *value = c->pack_stolen; return LISREG_OK; }
    if (!strcmp(name, "feeder_chunks")) { *value = c->pack_chunks_n; return LISREG_OK; }
    if (!strcmp(name, "canonical_ties")) { *value = (c->canonical_ties || c->exact) ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "index_build")) { *value = c->index_build; return LISREG_OK; }
    if (!strcmp(name, "index_build_now")) { *value = c->strip_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "front_end")) { *value = c->mode_now; return LISREG_OK; }
    if (!strcmp(name, "lanes_per_query")) { *value = c->lanes_q; return LISREG_OK; }          // what the prepared batch runs (auto resolved)
    if (!strcmp(name, "sort_sources")) { *value = c->sort_sources; return LISREG_OK; }
    if (!strcmp(name, "cell_anchor_until")) { *value = c->cell_anchor_until; return LISREG_OK; }
    if (!strcmp(name, "feeder_threads")) { *value = c->feeder_threads; return LISREG_OK; }
    if (!strcmp(name, "feeder_numa_node")) { *value = c->feeder_node; return LISREG_OK; }
    if (!strcmp(name, "feeder_numa_cpus")) { *value = c->feeder_cpus; return LISREG_OK; }
    if (!strcmp(name, "comm_nranks")) { *value = c->comm ? c->comm_nranks : 0; return LISREG_OK; }
    if (!strcmp(name, "sorted_now")) { *value = c->sort_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "rebuild_targets_each_run")) { *value = c->rebuild_targets_each_run ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "graph_min_ratio")) { *value = c->graph_min_ratio; return LISREG_OK; }
    if (!strcmp(name, "cell_min_ratio")) { *value = c->cell_min_ratio; return LISREG_OK; }
    if (!strcmp(name, "row_reach")) { *value = c->row_reach; return LISREG_OK; }
    if (!strcmp(name, "row_reach_now")) { *value = c->reach_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "row_reach_misses")) { *value = c->reach_miss_last; return LISREG_OK; }
    if (!strcmp(name, "cell_rows_max_mb")) { *value = c->cell_rows_max_mb; return LISREG_OK; }
    if (!strcmp(name, "xcd_order")) { *value = c->xcd_order; return LISREG_OK; }
    if (!strcmp(name, "xcd_order_now")) { *value = c->xcd_now ? 1 : 0; return LISREG_OK; }
    if (!strcmp(name, "interleave")) { *value = c->interleave; return LISREG_OK; }
    if (!strcmp(name, "interleaved_now")) { *value = c->interleaved_now ? 1 : 0; return LISREG_OK; }
    // size of the search index of the prepared batch's targets, in KiB (what the front-end in use reads), and their points:
    //   index_kib_grid: sorted records + cell table; index_kib_front_end: k-NN graph rows (front-end 3) or cell rows + their table (front-end 5)
    if (!strcmp(name, "index_kib_front_end_built")) {
        // the cell rows the LAST run actually built (option "row_reach" leaves out the cells no query comes near): row counts read back from the
        // device (a synchronous diagnostic); other front-ends: what "index_kib_front_end" says
        if (c->mode_now != 5) return lisreg_get_option(c, "index_kib_front_end", value);
        unsigned long long fe = 0;
        for (int slot : c->batch_slots) {
            if (slot < 0 || (size_t)slot >= c->targets.size()) continue;
            const lisreg::Target& t = c->targets[(size_t)slot];
            for (int k = 0; k < 2; ++k) {
                if (t.n[k] <= 0 || !t.crow_scan[k].p) continue;
                int rows = 0;
                if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess ||
                    hipMemcpy(&rows, t.crow_scan[k].as<int>() + t.n_cells[k], sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return LISREG_ERR_HIP;
                rows = std::min(std::max(rows, 0), t.crow_cap[k]);
                fe += (unsigned long long)rows * (sizeof(float4) * lisreg::kGraphK + sizeof(float2)) + (unsigned long long)t.n_cells[k] * sizeof(int);
            }
        }
        *value = (int)std::min<unsigned long long>((fe + 1023) / 1024, 0x7fffffffULL);
        return LISREG_OK;
    }
    if (!strcmp(name, "index_kib_grid") || !strcmp(name, "index_kib_front_end") || !strcmp(name, "index_target_points")) {
        unsigned long long grid = 0, fe = 0, pts = 0;
        for (int slot : c->batch_slots) {
            if (slot < 0 || (size_t)slot >= c->targets.size()) continue;
            const lisreg::Target& t = c->targets[(size_t)slot];
            for (int k = 0; k < 2; ++k) {
                if (t.n[k] <= 0) continue;
                pts += (unsigned long long)t.n[k];
                grid += (unsigned long long)t.n[k] * sizeof(float4) + ((unsigned long long)t.n_cells[k] + 1) * sizeof(int);
                if (c->mode_now == 3) fe += (unsigned long long)t.n[k] * (sizeof(float4) * lisreg::kGraphK + sizeof(float2));
                if (c->mode_now == 5) fe += (unsigned long long)t.crow_cap[k] * (sizeof(float4) * lisreg::kGraphK + sizeof(float2)) +
                                            (unsigned long long)t.n_cells[k] * sizeof(int);
            }
        }
        const unsigned long long v = !strcmp(name, "index_target_points") ? pts : ((!strcmp(name, "index_kib_grid") ? grid : fe) + 1023) / 1024;
        *value = (int)std::min<unsigned long long>(v, 0x7fffffffULL);
        return LISREG_OK;
    }
    return LISREG_ERR_ARG;
}

int lisreg_align_batch(lisreg_ctx* c, int n_items, const lisreg_item* items, const lisreg_params* params, float* T,
                       lisreg_stats* stats)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || (n_items > 0 && (!items || !T)) || !params) return bad(c, "align_batch: bad arguments");
    const auto t_in = std::chrono::steady_clock::now();
    HIPCHK(c, hipSetDevice(c->device));
    // stage host clouds into one device buffer of 16-B records; device items pass through
    size_t total = 0;
    for (int i = 0; i < n_items; ++i) {
        const lisreg_item& in = items[i];
        if (in.n_corner < 0 || in.n_surf < 0) return bad(c, "align_batch: negative count");
        if (in.fmt != LISREG_FMT_DEVICE) {
            if (in.stride_bytes < 12 || (in.fmt == LISREG_FMT_XYZIL && in.stride_bytes < 22)) return bad(c, "align_batch: bad stride");
            if ((in.n_corner > 0 && !in.src_corner) || (in.n_surf > 0 && !in.src_surf)) return bad(c, "align_batch: NULL cloud");
            total += (size_t)in.n_corner + (size_t)in.n_surf;
        }
    }
    std::vector<lisreg_item> dev_items((size_t)n_items);
    // Big host batches go through the feeder (lisreg_api_feed.hip): a few host threads pack the structs to 16-byte records in pinned
    // staging and the chunks are uploaded as they complete — half the bytes on the link, a few big copies instead of one per cloud.
    if (total >= 262144 && c->feeder_threads > 0) {
        int rc = lisreg_stage_host_items(c, n_items, items, dev_items.data());
        if (rc) return rc;
        rc = lisreg_batch_prepare(c, n_items, dev_items.data(), params, T);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        rc = run_impl(c, true);
        if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
        return lisreg_batch_fetch(c, T, stats);
    }
    // Small ones (a single odometry frame) cross PCIe as they are — the caller's structs, asynchronously on the context's stream —
    // and are packed to 16-byte records on the device: no thread is woken, nothing is repacked on the CPU.
    HIPCHK(c, c->src_upload.ensure(sizeof(lisreg_dpoint) * std::max<size_t>(total, 1)));
    size_t raw_bytes = 0;
    for (int i = 0; i < n_items; ++i)
        if (items[i].fmt != LISREG_FMT_DEVICE) raw_bytes += ((size_t)items[i].n_corner + (size_t)items[i].n_surf) * (size_t)items[i].stride_bytes + 32;
    HIPCHK(c, c->raw_upload.ensure(std::max<size_t>(raw_bytes, 16)));
    size_t off = 0, roff = 0;
    for (int i = 0; i < n_items; ++i) {
        dev_items[(size_t)i] = items[i];
        const lisreg_item& in = items[i];
        if (in.fmt == LISREG_FMT_DEVICE) continue;
        lisreg_item& d = dev_items[(size_t)i];
        const void* srcs[2] = { in.src_corner, in.src_surf };
        const int cnts[2] = { in.n_corner, in.n_surf };
        const void** dsts[2] = { &d.src_corner, &d.src_surf };
        for (int k = 0; k < 2; ++k) {
            lisreg_dpoint* dst = c->src_upload.as<lisreg_dpoint>() + off;
            *dsts[k] = dst;
            if (cnts[k] > 0) {
                unsigned char* rdst = static_cast<unsigned char*>(c->raw_upload.p) + roff;
                const size_t bytes = (size_t)cnts[k] * (size_t)in.stride_bytes;
                HIPCHK(c, hipMemcpyAsync(rdst, srcs[k], bytes, hipMemcpyHostToDevice, c->stream));
                launch_pack_cloud(rdst, (size_t)cnts[k], in.stride_bytes, in.fmt == LISREG_FMT_XYZIL, reinterpret_cast<float4*>(dst), c->stream);
                roff += (bytes + 15) & ~(size_t)15;
            }
            off += (size_t)cnts[k];
        }
        d.fmt = LISREG_FMT_DEVICE;
    }
    HIPCHK(c, hipGetLastError());
    static const bool host_prof = getenv("LISREG_HOST_PROF") != nullptr;      // where a synchronous call spends its host time
    auto now = [] { return std::chrono::steady_clock::now(); };
    const auto t0 = now();
    // a failure after uploads have been enqueued must not return while the DMA still reads the caller's (possibly pinned) buffers
    int rc = lisreg_batch_prepare(c, n_items, dev_items.data(), params, T);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    const auto t1 = now();
    rc = run_impl(c, true);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    const auto t2 = now();
    rc = lisreg_batch_fetch(c, T, stats);
    if (host_prof) {
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[lisreg host] upload %.1f us, prepare %.1f us, enqueue %.1f us, fetch (incl. GPU wait) %.1f us\n",
                us(t_in, t0), us(t0, t1), us(t1, t2), us(t2, now()));
    }
    return rc;
}

int lisreg_align(lisreg_ctx* c, const void* src_corner, int n_corner, const void* src_surf, int n_surf, int stride,
                 int fmt, const lisreg_params* params, const lisreg_imu* imu, float T[6], lisreg_stats* stats)
{
    if (!c) return LISREG_ERR_ARG;
    if (!params || !T) return bad(c, "align: params/T NULL");
    if (c->targets.empty() || !c->targets[0].valid) return ctx_fail(c, LISREG_ERR_NO_TARGET, "align: call lisreg_set_target first");
    lisreg_item item;
    memset(&item, 0, sizeof item);
    item.src_corner = src_corner; item.n_corner = n_corner;
    item.src_surf = src_surf; item.n_surf = n_surf;
    item.stride_bytes = stride; item.fmt = fmt; item.target = 0;
    item.degenerate_in = c->degenerate;
    if (imu) item.imu = *imu;
    const int bound = params->fixed_iters > 0 ? params->fixed_iters : params->max_iters;
    const int saved_cap = c->trace_cap;
    c->trace_cap = std::max(bound, 1);
    lisreg_stats st;
    memset(&st, 0, sizeof st);
    c->fetch_trace_records = c->trace_cap;             // the trace rides along with the result copy (one synchronisation)
    int rc = lisreg_align_batch(c, 1, &item, params, T, &st);
    c->fetch_trace_records = 0;
    if (rc == LISREG_OK) {
        c->degenerate = st.degenerate;
        c->last_trace_n = std::min(bound, st.iters + 1);
        if (st.status == LISREG_NOT_ENOUGH_FEATURES) c->last_trace_n = 0;
        c->last_trace.assign((size_t)kTraceStride * (size_t)std::max(c->last_trace_n, 1), 0.f);
        if (c->last_trace_n > 0 && c->fetch_host.p)
            memcpy(c->last_trace.data(), c->fetch_host.as<float>() + 2 * (size_t)kResultSize, sizeof(float) * kTraceStride * (size_t)c->last_trace_n);      // (one item + the "row_reach" record in front: lisreg_batch_fetch)
        if (stats) *stats = st;
        rc = st.status;
    }
    c->trace_cap = saved_cap;
    c->prepared = false;
    return rc;
}

int lisreg_get_trace(lisreg_ctx* c, float* buf, int max_iters)
{
    if (!c || !buf || max_iters <= 0) return 0;
    const int n = std::min(max_iters, c->last_trace_n);
    if (n > 0) memcpy(buf, c->last_trace.data(), sizeof(float) * kTraceStride * (size_t)n);
    return n;
}

int lisreg_get_counters(lisreg_ctx* c, unsigned long long* out, int n)
{
    if (!c || !out || n < 0) return LISREG_ERR_ARG;
    for (int i = 0; i < n; ++i) out[i] = 0;
    if (!c->counters.p) return LISREG_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->counters.p, sizeof(unsigned long long) * (size_t)std::min(n, 128), hipMemcpyDeviceToHost));
    if (c->mode_now == 3 || c->mode_now == 5) {              // the graph scan packs (walked << 32 | valid) per GN iteration: unpack to the pair layout
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
    if (!c->dump_neighbors || !c->dbg_nn.p || n_elems != c->n_elems || (c->mode_now != 1 && c->mode_now != 3 && c->mode_now != 5))
        return bad(c, "get_neighbors: set option dump_neighbors before preparing the batch (search modes 1, 3); n_elems must be the batch's source point count");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out, c->dbg_nn.p, sizeof(int) * 6 * (size_t)n_elems, hipMemcpyDeviceToHost));
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
