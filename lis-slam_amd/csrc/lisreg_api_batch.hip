// lisreg_api_batch.hip — the batch pipeline of liblisreg.so's C-ABI host layer: lisreg_batch_prepare / _run / _fetch, lisreg_align_batch and
// lisreg_align.  Every scan-to-submap registration goes through here.  The GN loop is enqueued in full (optional index rebuild, optional
// source sort, `bound` x {correspondence kernel, solve kernel}, finalize) with no host synchronisation inside lisreg_batch_run (the
// synchronous entry points may stop launching early once every item has converged).
//
// The host state is in four groups of the context (lisreg_ctx.hpp): the options `opt` (read only here, apart from lisreg_align's
// temporary trace_cap), the prepared batch `batch` (written by prepare; runs and fetches write its `live` block only), the last run's
// readouts `last` and the memory across batches `mem`.  What needs no device is decided in lisreg_batch_plan.hpp.
#include "lisreg_batch_plan.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace lisreg;

namespace {

// the context's targets as the plan reads them
struct CtxTargets {
    const std::vector<Target>& v;
    size_t size() const { return v.size(); }
    TargetView operator()(int slot) const
    {
        const Target& t = v[(size_t)slot];
        return TargetView{ t.valid, { t.n[0], t.n[1] }, { t.n_cells[0], t.n_cells[1] }, { &t.g[0], &t.g[1] }, { t.raw_ptr[0], t.raw_ptr[1] },
                           { t.sorted[0].as<float4>(), t.sorted[1].as<float4>() }, { t.cell_start[0].as<int>(), t.cell_start[1].as<int>() } };
    }
};

// fn(target, kind) -> return code, for both kinds of every slot in turn; the first code that is not LISREG_OK ends the walk and is returned
template <class Fn>
int for_each_target_kind(lisreg_ctx* c, const std::vector<int>& slots, Fn fn)
{
    for (int slot : slots)
        for (int k = 0; k < 2; ++k)
            if (const int rc = fn(c->targets[(size_t)slot], k)) return rc;
    return LISREG_OK;
}
template <class Fn>
int for_each_batch_target(lisreg_ctx* c, Fn fn) { return for_each_target_kind(c, c->batch.batch_slots, fn); }

// the "row_reach" miss counter of the prepared batch's runs: one record behind the items' results
int* reach_miss_counter(const lisreg_ctx* c)
{
    return reinterpret_cast<int*>(c->results.as<float>() + (size_t)std::max(c->batch.n_items, 1) * kResultSize);
}

// ---- lisreg_batch_prepare, phase by phase ------------------------------------------------------------------------------------------------

// Phase 1.  Reads the items' counts, the targets they name and the options; decides batch.mode_now and batch.lanes_q (plan_front_end).
// The cell rows re-make a target's grid with a margin the first time they are chosen for it — before anything later reads the geometry
// — so they are built here, for every valid target the items name.  (auto only) rows that would not fit "cell_rows_max_mb" together:
// the graph scan instead — and the rows already made for the batch's other targets go back (they would only hold memory).
int choose_front_end(lisreg_ctx* c, int n_items, const lisreg_item* items)
{
    const BatchOptions& o = c->opt;
    PreparedBatch& b = c->batch;
    std::vector<int> seen;
    if (plan_front_end(n_items, items, CtxTargets{ c->targets }, o, b.prm.bound, seen, &b.mode_now, &b.lanes_q) != kPlanOk)
        return bad(c, "batch_prepare: more than 2e9 source points in one batch");
    if (b.mode_now != 5) return LISREG_OK;
    const bool may_decline = o.search_mode == 4;
    bool declined = false;
    long long rows_left = crow_row_budget(o.cell_rows_max_mb);
    if (const int rc = for_each_target_kind(c, seen, [&](Target& t, int k) {
            if (declined || !t.valid) return (int)LISREG_OK;
            const bool had = t.crow_valid[k] && t.g[k].crow_tab;
            if (const int e = ensure_crows(c, t, k, may_decline, may_decline ? &rows_left : nullptr)) return e;
            if (!had) c->grids_dirty = true;
            declined = may_decline && t.crow_too_big[k];
            return (int)LISREG_OK;
        })) return rc;
    if (!declined) return LISREG_OK;
    b.mode_now = 3;
    return for_each_target_kind(c, seen, [&](Target& t, int k) {
        if (t.crow_valid[k]) { t.crow[k].release(); t.crow_meta[k].release(); t.crow_valid[k] = false; t.g[k].crow = nullptr; t.g[k].crow_meta = nullptr; t.g[k].crow_tab = nullptr; c->grids_dirty = true; }
        t.crow_chosen[k] = false;         // (the next set_target of this slot builds its grid without the rows' two-cell margin again)
        return (int)LISREG_OK;
    });
}

// Phase 3.  Reads the items, their initial poses, the targets' grids, the tile and batch.lanes_q; fills batch.h_items, h_segs, h_blocks,
// h_blocks_q and batch_slots and the counts that follow from them (plan_item_tables, which also makes the items' argument checks: a bad
// item is refused here, after the front-end choice may already have built rows).
int build_item_tables(lisreg_ctx* c, int n_items, const lisreg_item* items, const float* T_init, float tile)
{
    PreparedBatch& b = c->batch;
    b.h_blocks_q.clear();
    ItemTables tab{ b.h_items, b.h_segs, b.h_blocks, b.h_blocks_q, b.batch_slots, 0, 0 };
    switch (plan_item_tables(n_items, items, T_init, CtxTargets{ c->targets }, tile, b.lanes_q, b.prm, tab)) {
    case kPlanItemFormat: return bad(c, "batch_prepare: items must be LISREG_FMT_DEVICE (use lisreg_align_batch for host clouds)");
    case kPlanNullSource: return bad(c, "batch_prepare: NULL source cloud with n > 0");
    case kPlanNoTarget:   return ctx_fail(c, LISREG_ERR_NO_TARGET, "batch_prepare: item refers to a target slot that was never set");
    default: break;
    }
    b.n_blocks = (int)b.h_blocks.size();
    b.n_segs = (int)b.h_segs.size();
    b.n_elems = tab.n_elems;
    b.n_buckets = tab.n_buckets;
    return LISREG_OK;
}

// Phase 4.  Reads the counts of phase 3, batch.lanes_q and the options "dump_neighbors" / "trace_cap"; sizes the per-batch device
// buffers (grow-only).  Sources staged by lisreg_stage_host_items: the device waits for their uploads here, the host does not.
int size_batch_buffers(lisreg_ctx* c)
{
    const BatchOptions& o = c->opt;
    const PreparedBatch& b = c->batch;
    if (c->pack_pending) {
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->pack_pending, 0));
        c->pack_pending = nullptr;
        c->pack_in_use = c->pack_last;
    }
    const size_t flat = (size_t)std::max(b.n_elems, 1), n_items = (size_t)std::max(b.n_items, 1);
    HIPCHK(c, c->blocks.ensure(sizeof(BlockDesc) * (size_t)std::max(b.n_blocks, 1)));
    HIPCHK(c, c->segs.ensure(sizeof(Segment) * (size_t)std::max(b.n_segs, 1)));
    HIPCHK(c, c->items.ensure(sizeof(ItemState) * n_items));
    HIPCHK(c, c->sorted_all.ensure(sizeof(float4) * flat));
    HIPCHK(c, c->order_all.ensure(sizeof(int) * flat));
    HIPCHK(c, c->nn.ensure(sizeof(int) * 5 * flat));
    if (b.lanes_q > 1) {
        HIPCHK(c, c->blocks_q.ensure(sizeof(BlockDesc) * std::max<size_t>(b.h_blocks_q.size(), 1)));
        HIPCHK(c, c->coef.ensure(sizeof(float4) * flat));
        HIPCHK(c, c->coef_ok.ensure(sizeof(int) * flat));
    }
    if (o.dump_neighbors) {
        HIPCHK(c, c->dbg_nn.ensure(sizeof(int) * 6 * flat));
        HIPCHK(c, hipMemsetAsync(c->dbg_nn.p, 0xff, sizeof(int) * 6 * flat, c->stream));
    }
    HIPCHK(c, c->partials.ensure(sizeof(double) * kNumAcc * (size_t)std::max(b.n_blocks, 1)));
    HIPCHK(c, c->results.ensure(sizeof(float) * kResultSize * (n_items + 1)));      // (+ one record: the run's "row_reach" miss count)
    if (o.trace_cap > 0) HIPCHK(c, c->trace.ensure(sizeof(float) * kTraceStride * (size_t)o.trace_cap * n_items));
    return LISREG_OK;
}

// Phase 5.  Reads batch.mode_now and batch_slots; makes what the front-end reads of every target of the batch — the graph or the cell
// rows (the mode may have been chosen after the targets were set), the mark and reach words of option "row_reach" (buffers + the pointer
// in the grid; taken away again from a batch that does not want them) — and uploads the grid table if any of it changed.
int ensure_front_end_indices(lisreg_ctx* c)
{
    const PreparedBatch& b = c->batch;
    const bool marks = reach_marks_wanted(c->opt, b);
    const int rc = for_each_batch_target(c, [&](Target& t, int k) {
        int e = LISREG_OK;
        if (b.mode_now == 3 && !(t.graph_valid[k] && t.g[k].nbr)) { if ((e = ensure_graph(c, t, k, true))) return e; c->grids_dirty = true; }
        if (b.mode_now == 5 && !(t.crow_valid[k] && t.g[k].crow_tab)) { if ((e = ensure_crows(c, t, k))) return e; c->grids_dirty = true; }
        return e;
    });
    if (rc) return rc;
    if (const int e = for_each_batch_target(c, [&](Target& t, int k) { return ensure_reach(c, t, k, marks); })) return e;
    return c->grids_dirty ? upload_grids(c) : (int)LISREG_OK;
}

// Phase 6.  Reads batch_slots, their targets and the index-build options; fills batch.h_tsegs, h_tblocks, h_tchunks, the t_* totals
// and batch.strip_now (plan_target_tables), refuses "index_build" = 1 for grids that do not fit the strip form, and sizes the tables'
// device sides (a re-allocated strip table has no counters known to be zero).
int build_target_tables(lisreg_ctx* c)
{
    PreparedBatch& b = c->batch;
    b.h_tsegs.clear(); b.h_tblocks.clear(); b.h_tchunks.clear();
    TargetTables tab{ b.h_tsegs, b.h_tblocks, b.h_tchunks, 0, 0, 0, 0, 0, false };
    plan_target_tables(b.batch_slots, CtxTargets{ c->targets }, c->opt, tab);
    b.t_elems = tab.t_elems; b.t_buckets = tab.t_buckets; b.t_strips = tab.t_strips;
    b.t_max_units = tab.t_max_units; b.t_max_ucells = tab.t_max_ucells;
    b.strip_now = tab.strip_now;
    if (c->opt.index_build == 1 && !b.strip_now)
        return bad(c, "index_build 1: a target grid of this batch does not fit the strip form (strips per target or cells per strip)");
    HIPCHK(c, c->tchunk_dev.ensure(sizeof(BlockDesc) * std::max<size_t>(b.h_tchunks.size(), 1)));
    { const void* before = c->strip_tab.p; HIPCHK(c, c->strip_tab.ensure(sizeof(int) * (3 * ((size_t)b.t_strips + 4) + (size_t)b.t_strips / 2048 + 8))); if (c->strip_tab.p != before) c->mem.strip_zero_ints = 0; }
    HIPCHK(c, c->tseg_dev.ensure(sizeof(TargetSeg) * std::max<size_t>(b.h_tsegs.size(), 1)));
    HIPCHK(c, c->tblk_dev.ensure(sizeof(BlockDesc) * std::max<size_t>(b.h_tblocks.size(), 1)));
    return LISREG_OK;
}

// Phase 7.  Reads the seven host tables of phases 3 and 6.  Every table crosses PCIe from ONE pinned staging buffer: seven asynchronous
// copies, no host synchronisation (pageable sources would make each hipMemcpyAsync a blocking staged copy — most of a single
// registration's latency).
int upload_tables(lisreg_ctx* c)
{
    const PreparedBatch& b = c->batch;
    struct Part { const void* src; size_t bytes; void* dst; };
    const Part parts[7] = {
        { b.h_tchunks.data(), sizeof(BlockDesc) * b.h_tchunks.size(), c->tchunk_dev.p },
        { b.h_blocks_q.data(), sizeof(BlockDesc) * b.h_blocks_q.size(), c->blocks_q.p },
        { b.h_blocks.data(), sizeof(BlockDesc) * (size_t)b.n_blocks, c->blocks.p },
        { b.h_segs.data(), sizeof(Segment) * (size_t)b.n_segs, c->segs.p },
        { b.h_items.data(), sizeof(ItemState) * (size_t)b.n_items, c->items.p },
        { b.h_tsegs.data(), sizeof(TargetSeg) * b.h_tsegs.size(), c->tseg_dev.p },
        { b.h_tblocks.data(), sizeof(BlockDesc) * b.h_tblocks.size(), c->tblk_dev.p } };
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
    return LISREG_OK;
}

// Phase 8.  Reads "sort_sources", the batch's shape and the probe memory; decides batch.sort_now.  Scan order and voxel-grid order are
// spatially coherent and beat a re-sort; an arbitrary order costs the cell walk its L1 locality (2x slower), so in auto mode a cheap
// probe decides once per prepared batch.  Small batches (a single odometry frame) skip the probe and its host round trip: a sort could
// not pay for itself there.  (the probe costs a pass over the sources and a host round trip — 0.15 ms in front of a pipelined batch:
// batches of the same shape as the one last probed reuse its verdict, re-probed every 32nd; the verdict never changes the neighbours,
// only the order in which a workgroup sums its rows — the last bits of the poses)
int decide_sort(lisreg_ctx* c)
{
    const BatchOptions& o = c->opt;
    PreparedBatch& b = c->batch;
    BatchMemory& m = c->mem;
    b.sort_now = o.sort_sources == 1;
    if (o.sort_sources != 2 || b.n_elems < 65536) return LISREG_OK;
    if (m.probe_items == b.n_items && m.probe_elems == b.n_elems && m.probe_age < 32) {
        ++m.probe_age;
        b.sort_now = m.probe_verdict;
        return LISREG_OK;
    }
    launch_count_jumps(c->blocks.as<BlockDesc>(), b.n_blocks, c->segs.as<Segment>(), 1.5f, c->done_dev.as<int>(), c->stream);
    int jumps_stack = 0;
    int* jumps = c->done_host.p ? c->done_host.as<int>() : &jumps_stack;       // lisreg_create tolerates a failed pinned allocation
    HIPCHK(c, hipMemcpyAsync(jumps, c->done_dev.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b.sort_now = (double)*jumps > 0.25 * (double)b.n_elems;
    m.probe_verdict = b.sort_now; m.probe_items = b.n_items; m.probe_elems = b.n_elems; m.probe_age = 0;
    return LISREG_OK;
}

// Phase 9.  Reads the totals of phases 3 and 6, batch.sort_now and "rebuild_targets_each_run"; sizes the scratch of the bucket sorts:
// the target rebuild (if the batch does that) and the source sort (only if it will run).
int size_sort_scratch(lisreg_ctx* c)
{
    const PreparedBatch& b = c->batch;
    const bool rebuild = c->opt.rebuild_targets_each_run;
    const size_t se = (size_t)std::max(rebuild ? b.t_elems : 1, b.sort_now ? b.n_elems : 1);
    const size_t sbk = (size_t)std::max(rebuild ? b.t_buckets : 1, b.sort_now ? b.n_buckets : 1);
    return ensure_sort_scratch(c, se, sbk);
}

// Phase 10.  The registrations start reset (pose caches of the initial poses, done counter = the guard failures): every run leaves them
// reset again for the next one (launch_finalize), so a run has no reset launch of its own.  The "row_reach" miss count is cumulative
// from here.
void reset_items(lisreg_ctx* c)
{
    PreparedBatch& b = c->batch;
    launch_reset_items(c->items.as<ItemState>(), b.n_items, b.prm, c->done_dev.as<int>(), c->stream, reach_miss_counter(c));
    b.live.items_reset = true; b.live.reach_miss_seen = 0; b.live.runs_since_fetch = 0;
}

// Phase 11.  Query marks for the row builds of this batch's runs (option "row_reach"; cell rows, targets rebuilt inside every run).  A
// scan sees a part of its map — the lidar's elevation span leaves the upper walls of the benchmark room unseen: a fifth of the cells that
// would get rows — so every run builds rows only for the cells a query comes within a metre of under its INITIAL pose: one pass over the
// batch's source points (k_query_marks: the cell each falls into), those marks grown by ceil(1 m / cell) cells (`reach`, read by the
// classification of every run).  The mark words are cleared in front of the marking and kept: "row_reach" = 2 reads them as well (the
// cells a query starts in).  Both depend on the sources and the initial poses — what this call is given — not on the target's points,
// which a run may find changed.  Reads the marks' pointers in the grids (phase 5) and the back-off memory; decides live.reach_ready.
int make_reach_marks(lisreg_ctx* c)
{
    PreparedBatch& b = c->batch;
    b.live.reach_ready = false;
    if (c->mem.reach_backoff > 0) { --c->mem.reach_backoff; return LISREG_OK; }
    if (!reach_marks_wanted(c->opt, b) || b.lanes_q != 1 || b.n_blocks <= 0) return LISREG_OK;
    auto marked = [](const Target& t, int k) { return t.g[k].qmark != nullptr && t.n[k] > 0; };
    bool any = false;
    (void)for_each_batch_target(c, [&](Target& t, int k) { any = any || marked(t, k); return (int)LISREG_OK; });
    if (!any) return LISREG_OK;
    if (const int rc = for_each_batch_target(c, [&](Target& t, int k) {
            if (marked(t, k))
                HIPCHK(c, hipMemsetAsync(t.g[k].qmark, 0, sizeof(unsigned) * (size_t)t.g[k].nx * (size_t)t.g[k].ny * (size_t)t.g[k].qmark_w, c->stream));
            return (int)LISREG_OK;
        })) return rc;
    launch_query_marks(c->blocks.as<BlockDesc>(), b.n_blocks, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(), c->items.as<ItemState>(), c->stream);
    (void)for_each_batch_target(c, [&](Target& t, int k) {
        if (marked(t, k)) launch_reach_dilate(t.g[k], t.crow_reach[k].as<unsigned>(), c->stream);
        return (int)LISREG_OK;
    });
    HIPCHK(c, hipGetLastError());
    b.live.reach_ready = true;
    return LISREG_OK;
}

// Phase 12.  The dispatch order of the runs' correspondence launches (blocks ranked by the sector their queries fall into, one eighth per
// XCD) is a function of the same inputs — block descriptors, sources, initial poses, grid geometry: made here once instead of by every run
// (k_xcd_keys + a single-workgroup counting sort: 70 us per run on the side stream, which the shorter row build of "row_reach" had turned
// into the tail of a run's index phase).  Runs that sort their sources keep making their own; a run that splits the batch makes one table
// per part and leaves them to the runs after it (dispatch_order_tables).  Decides live.xcd_cached and live.xcd_split_blk.
// the dispatch-order table of the whole batch (split_blk 0), or one per part of a batch cut at workgroup split_blk: positions and ids
// relative to the part
void launch_order_tables(lisreg_ctx* c, int split_blk, const float4* sorted, hipStream_t st)
{
    const PreparedBatch& b = c->batch;
    const bool by_target = many_targets(c->opt, b);
    int* const pos = c->xcd_tab.as<int>();
    int* const ids = pos + b.n_blocks;
    const int nb0 = split_blk ? split_blk : b.n_blocks;
    launch_xcd_order(c->blocks.as<BlockDesc>(), nb0, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(), c->items.as<ItemState>(),
                     sorted, by_target, pos, ids, st);
    if (split_blk)
        launch_xcd_order(c->blocks.as<BlockDesc>() + split_blk, b.n_blocks - split_blk, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(),
                         c->items.as<ItemState>(), sorted, by_target, pos + split_blk, ids + split_blk, st);
}

int cache_xcd_order(lisreg_ctx* c)
{
    PreparedBatch& b = c->batch;
    b.live.xcd_cached = false;
    if (!xcd_order_wanted(c->opt, b) || b.sort_now || c->opt.exact || b.n_blocks <= 0) return LISREG_OK;
    HIPCHK(c, c->xcd_tab.ensure(sizeof(int) * 2 * (size_t)b.n_blocks));
    // the cut the batch's runs will take, as far as prepare can know it: a fixed iteration count never stops early from the host, whichever
    // entry point runs it, and the context is taken to be the only one running batches; any other batch gets the whole-batch table (a run
    // that cuts elsewhere makes its own, once)
    const int split_blk = b.prm.fixed_iters > 0 ? plan_run_split(c->opt, b, false, !b.live.one_shot).blk : 0;
    launch_order_tables(c, split_blk, nullptr, c->stream);
    HIPCHK(c, hipGetLastError());
    b.live.xcd_cached = true; b.live.xcd_split_blk = split_blk;
    return LISREG_OK;
}

// ---- run_impl, phase by phase ------------------------------------------------------------------------------------------------------------
// (nothing below writes the options or the prepared batch outside batch.live: they are read through these two)
struct RunView { const BatchOptions& o; const PreparedBatch& b; };
RunView view(const lisreg_ctx* c) { return RunView{ c->opt, c->batch }; }

// exact_arithmetic: the sine and cosine of the three pose angles are taken by the HOST's libm — the library the reference's
// pcl::getTransformation and LMOptimization call (cosf / sinf on x86-64) — because no device routine returns its last bit in every case
// (1 configuration in 100 showed a 1-ulp matrix entry, which swapped two candidates 8e-7 apart in squared distance).  One 24-byte-per-item
// round trip per Gauss-Newton iteration; only this build pays it.
int exact_pose_caches(lisreg_ctx* c)
{
    const size_t n = (size_t)c->batch.n_items;
    if (n == 0) return LISREG_OK;
    HIPCHK(c, c->exact_trig.ensure(sizeof(float) * 6 * n));
    std::vector<float> T(6 * n), trig(6 * n);
    launch_pose_gather(c->items.as<ItemState>(), (int)n, c->exact_trig.as<float>(), c->stream);
    HIPCHK(c, hipMemcpyAsync(T.data(), c->exact_trig.p, sizeof(float) * 6 * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) {
        const float* t = &T[6 * i];
        float* g = &trig[6 * i];
        g[0] = cosf(t[2]); g[1] = sinf(t[2]); g[2] = cosf(t[1]); g[3] = sinf(t[1]); g[4] = cosf(t[0]); g[5] = sinf(t[0]);
    }
    HIPCHK(c, hipMemcpyAsync(c->exact_trig.p, trig.data(), sizeof(float) * 6 * n, hipMemcpyHostToDevice, c->stream));
    launch_pose_cache_from_trig(c->items.as<ItemState>(), (int)n, c->exact_trig.as<float>(), c->stream);
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

// The split decision.  Two halves of the batch on two streams (round 5).  The 6x6 solves are one workgroup per registration and ~13 us of
// dependent latency between two correspondence launches: the chip idles through ten of them per step.  Registrations are independent, so
// the batch is cut in two at an item boundary (where: below): the first half iterates on the context's stream, the
// second on the side stream, and each half's solve (and launch gaps, and the thinning tail of its correspondence launch) runs underneath
// the other half's correspondence launch.  Same kernels on the same data in the same order per registration: same results to the bit.
// Only for runs that do not stop early from the host (fixed iteration counts, lisreg_batch_run) and are big enough to fill the chip
// twice.  Makes the side stream and the halves' events on first use; no split without them.
// Whether, in which form and where: plan_run_split (lisreg_batch_plan.hpp: "interleave" = 1 cuts at the middle, 2 and the library's own
// choice under the default 0 where plan_split_uneven says).
// The library's own choice (the `alone` of split_form) is for a prepared batch run through lisreg_batch_run by the only context of the
// process that runs batches: that is where it was measured to pay.  A synchronous lisreg_align_batch (prepare, one run, fetch; host clouds
// staged in front) read 5 % lower with it in four pairs of bench.py's `pcie_inclusive` leg, within that leg's noise but never ahead.
Split choose_split(lisreg_ctx* c, bool can_stop)
{
    const auto [o, b] = view(c);
    const bool alone = batch_runner_alone(c);
    const Split s = plan_run_split(o, b, can_stop, alone && !b.live.one_shot);
    if (s.blk <= 0) return Split();
    ensure_side_stream(c);
    if (c->side_stream && !c->ev_ab && (c->ev_ab.create(hipEventDisableTiming) != hipSuccess ||
                                        c->ev_ba.create(hipEventDisableTiming) != hipSuccess)) { c->ev_ab.reset(); c->ev_ba.reset(); }
    return c->side_stream ? s : Split();
}

// The index of every target of the batch, rebuilt from the caller's points in one launch sequence ("rebuild_targets_each_run": the
// reference rebuilds both kd-trees per registration, :602-603): the grid in strip or bucket-sort form (batch.strip_now), then the graph
// or the cell rows of the front-end — with last.reach_now, rows for the reached cells only.
int rebuild_targets(lisreg_ctx* c, hipStream_t st)
{
    const auto [o, b] = view(c);
    ctx_prof_mark(c, 2);
    if (b.strip_now) {
        StripBuffers sl;
        sl.cnt = c->strip_tab.as<int>(); sl.fill = sl.cnt + (b.t_strips + 1); sl.start = sl.fill + (b.t_strips + 1);
        sl.scan_tmp = sl.start + (b.t_strips + 2);
        sl.tmp_pts = c->tmp_pts.as<float4>(); sl.slot_idx = c->elem_bucket.as<uint32_t>(); sl.slot_pos = c->elem_sub.as<uint32_t>();
        ensure_side_stream(c);                    // failure just means the two variants run back to back
        sl.side = c->side_stream; sl.ev_fork = c->ev_fork; sl.ev_join = c->ev_join;
        if (launch_build_targets_strips(c->tchunk_dev.as<BlockDesc>(), (int)b.h_tchunks.size(), c->tseg_dev.as<TargetSeg>(),
                                        (int)b.h_tsegs.size(), b.t_strips, b.t_max_units, b.t_max_ucells, o.strip_cap, sl, st, &c->mem.strip_zero_ints))
            return ctx_fail(c, LISREG_ERR_HIP, "strip index build: LDS configuration refused");
    } else
        launch_build_targets_batched(c->tblk_dev.as<BlockDesc>(), (int)b.h_tblocks.size(), c->tseg_dev.as<TargetSeg>(),
                                     (int)b.h_tsegs.size(), b.t_elems, b.t_buckets, sort_buffers(c), st);
    if (b.mode_now == 3)
        launch_build_graph(c->tblk_dev.as<BlockDesc>(), (int)b.h_tblocks.size(), c->tseg_dev.as<TargetSeg>(),
                           c->grids_dev.as<GridIndex>(), st);
    if (b.mode_now == 5) {
        // corner and surf target of a slot in ONE launch sequence on this stream (launch_crow_rows_pair): no side stream, no event hops
        const bool reach = c->last.reach_now, near_only = o.row_reach == 2;
        for (int slot : b.batch_slots) {
            Target& t = c->targets[(size_t)slot];
            const GridIndex g2[2] = { t.g[0], t.g[1] };
            const int nc2[2] = { t.n_cells[0], t.n_cells[1] };
            const lisreg::CrowBuffers cb2[2] = { crow_buffers(t, 0, reach, near_only), crow_buffers(t, 1, reach, near_only) };
            int* oz2[2] = { &t.omask_zero[0], &t.omask_zero[1] };
            launch_crow_rows_pair(g2, nc2, cb2, st, oz2);
        }
    }
    ctx_prof_mark(c, -1);
    return LISREG_OK;
}

// The dispatch-order tables of this run (last.xcd_now), after the source sort: the keys read the sorted records.  An unsplit run of an
// unsorted batch reuses the table prepare cached.  An interleaved run dispatches its halves separately: one table per half, positions
// and ids relative to the half.
void dispatch_order_tables(lisreg_ctx* c, Split split, hipStream_t st)
{
    const auto [o, b] = view(c);
    PreparedBatch::Live& live = c->batch.live;
    if (!c->last.xcd_now || (live.xcd_cached && live.xcd_split_blk == split.blk)) return;
    // the tables are a function of what lisreg_batch_prepare was given (cache_xcd_order) unless the run sorts its sources: the ones made
    // here stay good for the later runs of this prepared batch that cut it at the same place (a split run made both of its tables anew
    // in front of every Gauss-Newton loop: 41 us of a 2.1 ms step on configs[1], profiles/interleave_uneven.md)
    live.xcd_cached = !b.sort_now && !o.exact;
    live.xcd_split_blk = split.blk;
    // (part tables overwrite the batch's table: live.xcd_split_blk says which the buffer holds, and a later run of this batch that is cut
    // elsewhere or not at all — interleave switched off, interleave_min_blocks raised — makes its own instead of reading part-relative ids
    // as whole-batch ones)
    launch_order_tables(c, split.blk, b.sort_now ? c->sorted_all.as<float4>() : nullptr, st);
}

// the part of the batch one stream iterates on: the items [i0, i0 + ni) = the workgroups [b0, b0 + nb) on stream s (sidx: which stream the
// profiling marks go on); after_assoc: an event recorded right behind the correspondence launch, for the alternation of an interleaved run
struct RunHalf { int i0, ni, b0, nb; hipStream_t s; int sidx; hipEvent_t after_assoc; };

// Does the last solve of this run do the finalize as well (launch_solve's finalize_results)?  Runs whose last iteration is known when it
// is enqueued and in which no registration finishes before it: a fixed iteration count, no early stop from the host.  One launch and one
// kernel boundary less at the end of a step — per part in an interleaved run, whose parts then need nothing behind their join.
bool finalize_in_last_solve(const DevParams& prm, bool can_stop) { return prm.fixed_iters > 0 && !can_stop; }

// one Gauss-Newton iteration of a half: the correspondence launch and the solve (last_folded: and this half's finalize inside that solve)
void iteration(lisreg_ctx* c, const DevParams& prm, int it, const RunHalf& h, bool last_folded)
{
    const auto [o, b] = view(c);
    if (!h.after_assoc) ctx_prof_mark(c, 0, h.sidx);          // (an alternating run marks behind its wait for the other half)
    (o.exact ? launch_assoc_exact : launch_assoc)(
                 c->blocks.as<BlockDesc>() + h.b0, h.nb, c->segs.as<Segment>(), c->grids_dev.as<GridIndex>(),
                 c->items.as<ItemState>(), prm, b.sort_now ? c->sorted_all.as<float4>() : nullptr, c->partials.as<double>() + (size_t)h.b0 * kNumAcc,
                 b.mode_now, c->nn.as<int>(), b.n_elems, o.first_pass_r * o.first_pass_r,
                 b.mode_now != 5 && it >= (b.lanes_q == 8 ? kWideFromSmall : kWideFrom) && it <= (b.mode_now == 3 ? kGraphWideUntil : kWideUntil), kGraphHops,
                 o.count_searches ? c->counters.as<unsigned long long>() : nullptr,
                 o.dump_neighbors ? c->dbg_nn.as<int>() : nullptr, b.lanes_q,
                 c->blocks_q.as<BlockDesc>(), (int)b.h_blocks_q.size(), c->coef.as<float4>(), c->coef_ok.as<int>(),
                 c->last.xcd_now ? c->xcd_tab.as<int>() + b.n_blocks + h.b0 : nullptr, h.s);
    if (h.after_assoc) (void)hipEventRecord(h.after_assoc, h.s);
    ctx_prof_mark(c, 1, h.sidx);
    launch_solve(c->items.as<ItemState>() + h.i0, h.ni, prm, c->partials.as<double>(),
                 o.trace_cap > 0 ? c->trace.as<float>() + (size_t)h.i0 * (size_t)o.trace_cap * kTraceStride : nullptr, o.trace_cap, c->done_dev.as<int>(), h.s,
                 last_folded ? c->results.as<float>() + (size_t)h.i0 * kResultSize : nullptr);
    ctx_prof_mark(c, -1, h.sidx);
}

// The plain loop: every iteration of the whole batch on the context's stream.  can_stop (synchronous entry points): after every few
// iterations the host reads the "registrations finished" counter and stops launching once every item has converged.  How often it
// looks: a skipped launch of a big batch still dispatches tens of thousands of workgroups (check every 3 iterations), a skipped launch
// of a single frame costs ~2 us (check every 6: one round trip for the typical 3-6 iteration registration).  Sequential use: the last
// batch fetched from this context needed `last_launches` iterations — frames of a drive converge alike, so the first look is taken
// right there (a replay frame converges in 3: three no-op iterations, nine launches, not enqueued), later looks every 3.
int run_plain(lisreg_ctx* c, const DevParams& prm, bool can_stop, hipStream_t st)
{
    const auto [o, b] = view(c);
    const int chunk = o.early_stop_chunk > 0 ? o.early_stop_chunk : (b.n_blocks <= 1024 ? 6 : 3);
    int next_check = chunk;
    if (o.early_stop_chunk <= 0 && c->mem.last_launches > 0) next_check = std::max(2, std::min(c->mem.last_launches, chunk));
    const RunHalf all{ 0, b.n_items, 0, b.n_blocks, st, 0, nullptr };
    const bool fold = finalize_in_last_solve(prm, can_stop);
    for (int it = 0; it < prm.bound; ++it) {
        iteration(c, prm, it, all, fold && it + 1 == prm.bound);
        if (o.exact && it + 1 < prm.bound) { int rc = exact_pose_caches(c); if (rc) return rc; }
        if (can_stop && it + 1 == next_check && it + 1 < prm.bound) {
            HIPCHK(c, hipMemcpyAsync(c->done_host.p, c->done_dev.p, sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            if (*c->done_host.as<int>() >= b.n_items) break;
            next_check += o.early_stop_chunk > 0 ? chunk : std::min(chunk, 3);
        }
    }
    return LISREG_OK;
}

// The interleaved loop (the side stream already waits for ev_fork).  "interleave" = 1: the two correspondence launches ALTERNATE (each
// waits for the other half's previous one through an event), so that every launch has the chip to itself apart from the other half's
// solve — per-launch durations stay what they are for a launch alone, which is what the roofline figures of bench.py and the profiler
// tables are made of; 2: free-running (the launches of the two streams share the chip whenever both are ready: same throughput, launch
// durations no longer comparable).  A failing event call must not leave work of the second half un-joined on the side stream (the
// caller's next fetch on `st` would race with it): on any failure the side stream is drained by the HOST before the error is returned,
// and the run counts as not interleaved.
int run_interleaved(lisreg_ctx* c, const DevParams& prm, Split split, hipStream_t st)
{
    const auto [o, b] = view(c);
    c->last.interleaved_now = true;
    const bool alternate = o.interleave == 1 && c->ev_ab && c->ev_ba;
    const RunHalf A{ 0, split.item, 0, split.blk, st, 0, alternate ? (hipEvent_t)c->ev_ab : nullptr };
    const RunHalf B{ split.item, b.n_items - split.item, split.blk, b.n_blocks - split.blk, c->side_stream, 1, alternate ? (hipEvent_t)c->ev_ba : nullptr };
    const bool fold = finalize_in_last_solve(prm, false);           // (a run that can stop early is never split)
    hipError_t ie = hipSuccess;
    for (int it = 0; it < prm.bound && ie == hipSuccess; ++it) {
        if (alternate && it > 0) ie = hipStreamWaitEvent(st, c->ev_ba, 0);                   // B's launch of the iteration before is through
        if (ie != hipSuccess) break;
        if (alternate) ctx_prof_mark(c, 0, 0);
        iteration(c, prm, it, A, fold && it + 1 == prm.bound);
        if (alternate) ie = hipStreamWaitEvent(c->side_stream, c->ev_ab, 0);                 // A's launch of this iteration is through
        if (ie != hipSuccess) break;
        if (alternate) ctx_prof_mark(c, 0, 1);
        iteration(c, prm, it, B, fold && it + 1 == prm.bound);
    }
    if (ie == hipSuccess) ie = hipEventRecord(c->ev_join, c->side_stream);
    if (ie == hipSuccess) ie = hipStreamWaitEvent(st, c->ev_join, 0);
    if (ie == hipSuccess) return LISREG_OK;
    (void)hipStreamSynchronize(c->side_stream);
    c->last.interleaved_now = false;
    return ctx_fail(c, LISREG_ERR_HIP, std::string("interleaved run: ") + hipGetErrorString(ie));
}

// Finalize: the results, and the registrations reset for the next run (done: by the last solve already, finalize_in_last_solve); the
// staged source buffer may be overwritten once this run is through
int finalize_run(lisreg_ctx* c, const DevParams& prm, hipStream_t st, bool done)
{
    if (!done) launch_finalize(c->items.as<ItemState>(), c->batch.n_items, prm, c->results.as<float>(), st, c->done_dev.as<int>());
    c->batch.live.items_reset = true; ++c->batch.live.runs_since_fetch;
    HIPCHK(c, hipGetLastError());
    if (c->pack_in_use >= 0 && c->pack_free[c->pack_in_use])
        HIPCHK(c, hipEventRecord(c->pack_free[c->pack_in_use], st));
    return LISREG_OK;
}

// Enqueue one full pass.  early_stop (synchronous entry points only): after every few iterations the host reads a
// 4-byte "registrations finished" counter and stops launching once every item has converged — the reference's
// `break` at :617 — instead of launching no-op kernels up to max_iters.  Results are identical either way.
int run_impl(lisreg_ctx* c, bool early_stop)
{
    if (!c->batch.live.prepared) return bad(c, "batch_run: no prepared batch");
    HIPCHK(c, hipSetDevice(c->device));
    const auto [o, b] = view(c);
    PreparedBatch::Live& live = c->batch.live;
    hipStream_t st = c->stream;
    c->last.xcd_now = xcd_order_wanted(o, b);
    if (c->last.xcd_now) HIPCHK(c, c->xcd_tab.ensure(sizeof(int) * 2 * (size_t)b.n_blocks));
    const bool can_stop = early_stop && b.prm.fixed_iters <= 0 && c->done_host.p && o.early_stop_chunk != 0;
    const Split split = choose_split(c, can_stop);
    // Round 6, option "row_reach": the rows of this run are built only for the cells a query of the batch comes within a metre of under
    // its initial pose (`reach` words made by lisreg_batch_prepare: they depend on the sources and the initial poses alone, not on the target's
    // points).  A query that ends up in a cell without rows all the same takes the cell walk: results cannot depend on the marks.
    c->last.reach_now = o.rebuild_targets_each_run && b.mode_now == 5 && live.reach_ready && !o.exact;
    DevParams prm = b.prm;                     // this run's copy: its miss counter and (below) its "cell_anchor_until"
    prm.reach_miss = c->last.reach_now ? reach_miss_counter(c) : nullptr;
    // (the registrations are reset already — by lisreg_batch_prepare or by the run before, launch_finalize — unless a run ended in an error)
    const bool reset_done = live.items_reset;
    live.items_reset = false;
    if (o.rebuild_targets_each_run) { int rc = rebuild_targets(c, st); if (rc) return rc; }
    if (!reset_done) launch_reset_items(c->items.as<ItemState>(), b.n_items, prm, c->done_dev.as<int>(), st);
    if (o.exact) { int rc = exact_pose_caches(c); if (rc) return rc; }
    ctx_prof_mark(c, 2);
    launch_sort_sources(c->blocks.as<BlockDesc>(), b.n_blocks, c->segs.as<Segment>(), b.n_segs, c->items.as<ItemState>(),
                        b.n_elems, b.sort_now ? b.n_buckets : 0, sort_buffers(c), c->sorted_all.as<float4>(), c->order_all.as<int>(), st);
    ctx_prof_mark(c, -1);
    dispatch_order_tables(c, split, st);
    prm.cell_anchor_until = o.cell_anchor_until;
    c->last.interleaved_now = false;
    int rc;
    if (split.blk > 0 && hipEventRecord(c->ev_fork, st) == hipSuccess && hipStreamWaitEvent(c->side_stream, c->ev_fork, 0) == hipSuccess)
        rc = run_interleaved(c, prm, split, st);
    else
        rc = run_plain(c, prm, can_stop, st);
    return rc ? rc : finalize_run(c, prm, st, finalize_in_last_solve(prm, can_stop) && prm.bound > 0);
}

// lisreg_batch_prepare; one_shot: for a synchronous entry point, which enqueues the batch's one run right behind
int prepare_impl(lisreg_ctx* c, int n_items, const lisreg_item* items, const lisreg_params* params, const float* T_init, bool one_shot)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || (n_items > 0 && (!items || !T_init)) || !params) return bad(c, "batch_prepare: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    PreparedBatch& b = c->batch;
    b.live.prepared = false; b.live.one_shot = one_shot;
    b.params = *params;
    b.prm = make_dev_params(*params);
    b.prm.exact = c->opt.exact ? 1 : 0;
    b.prm.ties = (c->opt.canonical_ties || c->opt.exact) ? 1 : 0;
    b.n_items = n_items;
    b.h_blocks.clear(); b.h_segs.clear(); b.h_items.assign((size_t)n_items, ItemState());
    b.batch_slots.clear();
    int rc;
    if ((rc = choose_front_end(c, n_items, items))) return rc;                                  // 1
    const float tile = plan_sort_tile(n_items, items, CtxTargets{ c->targets });                // 2
    if ((rc = build_item_tables(c, n_items, items, T_init, tile))) return rc;                   // 3
    if ((rc = size_batch_buffers(c))) return rc;                                                // 4
    if ((rc = ensure_front_end_indices(c))) return rc;                                          // 5
    if ((rc = build_target_tables(c))) return rc;                                               // 6
    if ((rc = upload_tables(c))) return rc;                                                     // 7
    if ((rc = decide_sort(c))) return rc;                                                       // 8
    if ((rc = size_sort_scratch(c))) return rc;                                                 // 9
    reset_items(c);                                                                             // 10
    if ((rc = make_reach_marks(c))) return rc;                                                  // 11
    if ((rc = cache_xcd_order(c))) return rc;                                                   // 12
    b.live.prepared = true;
    return LISREG_OK;
}

// lisreg_align_batch's tail, after the sources are on their way to the device: prepare, run with early stop, fetch.  A failure after
// uploads have been enqueued must not return while the DMA still reads the caller's (possibly pinned) buffers: the stream is drained
// first.  prof (null: no print): when the call came in and when its uploads were enqueued — where a synchronous call spends its host time.
using HostClock = std::chrono::steady_clock;
int prepare_run_fetch(lisreg_ctx* c, int n_items, const lisreg_item* dev_items, const lisreg_params* params, float* T, lisreg_stats* stats,
                      const HostClock::time_point* prof)
{
    int rc = prepare_impl(c, n_items, dev_items, params, T, true);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    const auto t1 = prof ? HostClock::now() : HostClock::time_point();
    rc = run_impl(c, true);
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }
    const auto t2 = prof ? HostClock::now() : HostClock::time_point();
    rc = lisreg_batch_fetch(c, T, stats);
    if (prof) {
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[lisreg host] upload %.1f us, prepare %.1f us, enqueue %.1f us, fetch (incl. GPU wait) %.1f us\n",
                us(prof[0], prof[1]), us(prof[1], t1), us(t1, t2), us(t2, HostClock::now()));
    }
    return rc;
}

}  // namespace

// =============================================================================================================
extern "C" {

int lisreg_batch_prepare(lisreg_ctx* c, int n_items, const lisreg_item* items, const lisreg_params* params,
                         const float* T_init)
{
    return prepare_impl(c, n_items, items, params, T_init, false);
}

int lisreg_batch_run(lisreg_ctx* c)
{
    if (!c) return LISREG_ERR_ARG;
    return run_impl(c, false);
}

int lisreg_batch_fetch(lisreg_ctx* c, float* T, lisreg_stats* stats)
{
    if (!c) return LISREG_ERR_ARG;
    if (!c->batch.live.prepared) return bad(c, "batch_fetch: no prepared batch");
    HIPCHK(c, hipSetDevice(c->device));
    const PreparedBatch& b = c->batch;
    PreparedBatch::Live& live = c->batch.live;
    // results (and, for lisreg_align, the trace) land in pinned memory: asynchronous copies, ONE synchronisation
    const size_t res_floats = ((size_t)std::max(b.n_items, 1) + 1) * kResultSize;
    const size_t trace_floats = c->opt.fetch_trace_records > 0 ? (size_t)kTraceStride * (size_t)c->opt.fetch_trace_records : 0;
    const size_t fetch_bytes = (res_floats + trace_floats) * sizeof(float);
    HIPCHK(c, c->fetch_host.ensure(fetch_bytes, fetch_bytes * 2 + 4096));
    float* fetched = c->fetch_host.as<float>();
    const bool with_miss = b.n_items > 0 && c->last.reach_now;
    if (b.n_items) HIPCHK(c, hipMemcpyAsync(fetched, c->results.p, sizeof(float) * kResultSize * ((size_t)b.n_items + (with_miss ? 1 : 0)), hipMemcpyDeviceToHost, c->stream));
    if (trace_floats && c->trace.p) HIPCHK(c, hipMemcpyAsync(fetched + res_floats, c->trace.p, sizeof(float) * trace_floats, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->last.h_results.assign(fetched, fetched + res_floats);
    if (with_miss) {
        // "row_reach" watches itself: the marks are the queries' cells under their INITIAL poses grown by a metre; a batch whose first steps move
        // its points farther than that sends queries into cells without rows, where they walk (exact, but slow: configs[4] with a 0.5 m
        // dilation ran 30 % longer).  More than one query-iteration in a thousand there: the prepared batch's later runs, and the next 32
        // batches prepared on this context, build all rows.
        int cum; memcpy(&cum, fetched + (size_t)b.n_items * kResultSize, sizeof cum);      // (cumulative since the batch was prepared)
        const int miss = cum - live.reach_miss_seen;
        live.reach_miss_seen = cum;
        c->last.reach_miss_last = miss;
        if ((long long)miss * 1000LL > (long long)b.n_elems * (long long)std::max(b.prm.bound, 1) * (long long)std::max(live.runs_since_fetch, 1)) { live.reach_ready = false; c->mem.reach_backoff = 32; }
    }
    ctx_prof_collect(c);          // events of every profiled run since the last fetch (profiling may be off again by now)
    c->mem.last_launches = 0;
    for (int i = 0; i < b.n_items; ++i) {
        const float* r = &c->last.h_results[(size_t)i * kResultSize];
        c->mem.last_launches = std::max(c->mem.last_launches, (int)r[6] + 1);
        if (T) memcpy(T + 6 * (size_t)i, r, 24);
        if (stats) {
            stats[i].iters = (int)r[6]; stats[i].deltaR = r[7]; stats[i].deltaT = r[8];
            stats[i].degenerate = (int)r[9]; stats[i].n_corr_last = (int)r[10]; stats[i].status = (int)r[11];
        }
    }
    live.runs_since_fetch = 0;
    return LISREG_OK;
}

void* lisreg_batch_result_device(const lisreg_ctx* c) { return c ? c->results.p : nullptr; }

int lisreg_align_batch(lisreg_ctx* c, int n_items, const lisreg_item* items, const lisreg_params* params, float* T,
                       lisreg_stats* stats)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_items < 0 || (n_items > 0 && (!items || !T)) || !params) return bad(c, "align_batch: bad arguments");
    const auto t_in = HostClock::now();
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
        return prepare_run_fetch(c, n_items, dev_items.data(), params, T, stats, nullptr);
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
    static const bool host_prof = getenv("LISREG_HOST_PROF") != nullptr;
    const HostClock::time_point stamps[2] = { t_in, HostClock::now() };
    return prepare_run_fetch(c, n_items, dev_items.data(), params, T, stats, host_prof ? stamps : nullptr);
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
    item.degenerate_in = c->mem.degenerate;
    if (imu) item.imu = *imu;
    const int bound = params->fixed_iters > 0 ? params->fixed_iters : params->max_iters;
    const int saved_cap = c->opt.trace_cap;
    c->opt.trace_cap = std::max(bound, 1);
    lisreg_stats st;
    memset(&st, 0, sizeof st);
    c->opt.fetch_trace_records = c->opt.trace_cap;             // the trace rides along with the result copy (one synchronisation)
    int rc = lisreg_align_batch(c, 1, &item, params, T, &st);
    c->opt.fetch_trace_records = 0;
    if (rc == LISREG_OK) {
        BatchMemory& m = c->mem;
        m.degenerate = st.degenerate;
        m.last_trace_n = std::min(bound, st.iters + 1);
        if (st.status == LISREG_NOT_ENOUGH_FEATURES) m.last_trace_n = 0;
        m.last_trace.assign((size_t)kTraceStride * (size_t)std::max(m.last_trace_n, 1), 0.f);
        if (m.last_trace_n > 0 && c->fetch_host.p)
            memcpy(m.last_trace.data(), c->fetch_host.as<float>() + 2 * (size_t)kResultSize, sizeof(float) * kTraceStride * (size_t)m.last_trace_n);      // (one item + the "row_reach" record in front: lisreg_batch_fetch)
        if (stats) *stats = st;
        rc = st.status;
    }
    c->opt.trace_cap = saved_cap;
    c->batch.live.prepared = false;
    return rc;
}

}  // extern "C"
