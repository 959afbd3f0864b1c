// lisreg_batch_plan.hpp — the decisions of lisreg_batch_prepare and run_impl that need no device (lisreg_api_batch.hip): pure functions
// of the items, of the grids and counts of the targets they refer to, of the options and of DevParams.  None takes a lisreg_ctx or makes
// a HIP call; their outputs are the batch's tables.  host/batch_plan_check.cpp holds the loops they were cut out of in closed form and
// compares the two on random batches.
#pragma once
#include "lisreg_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace lisreg {

// What the plan reads of one target slot.  `Targets` below is any callable slot -> TargetView with a size(): the context's target vector
// (lisreg_api_batch.hip) or the check program's plain arrays.
struct TargetView {
    bool             valid;
    int              n[2], n_cells[2];
    const GridIndex* g[2];
    const float4*    raw[2];
    float4*          sorted[2];
    int*             cell_start[2];
};

// bytes of one cell row (search_mode 5): kGraphK entries and the (rho^2, count) beside them
constexpr size_t kCrowRowBytes = sizeof(float4) * kGraphK + sizeof(float2);
// rows that fit "cell_rows_max_mb"
inline long long crow_row_budget(int max_mb) { return (long long)std::max(max_mb, 1) * 1048576LL / (long long)kCrowRowBytes; }

enum PlanError { kPlanOk = 0, kPlanTooManySources, kPlanItemFormat, kPlanNullSource, kPlanNoTarget };

// Phase 1, the front-end choice.  Reads the items' source counts, the point counts of the distinct target slots they name (`seen`, in
// order of first use; unset or out-of-range slots are passed over here: phase 3 refuses them) and the options; decides the front-end of
// the batch (*mode) and its lanes per query (*lanes_q).  The k-NN graph costs ~1 ns per target point and saves ~0.015 ns per
// query-iteration (MI355X): it pays for shared / long-lived targets (a batch of scans against one submap), not for one-shot
// targets (a loop-closure candidate pair, a single odometry frame).  A batch of at most 131072 source points cannot fill the chip with
// one lane per query: eight lanes share a query (k_assoc_walk<.., 8>).  Whether the rows chosen here fit together is the caller's to find
// out (choose_front_end builds them).
template <class Targets>
inline PlanError plan_front_end(int n_items, const lisreg_item* items, const Targets& targets, const BatchOptions& o, int bound,
                                std::vector<int>& seen, int* mode, int* lanes_q)
{
    long long total_src = 0;
    double t_pts = 0;
    seen.clear();
    for (int i = 0; i < n_items; ++i) {
        total_src += (long long)std::max(items[i].n_corner, 0) + (long long)std::max(items[i].n_surf, 0);
        const int sl = items[i].target;
        if (sl >= 0 && (size_t)sl < targets.size() && std::find(seen.begin(), seen.end(), sl) == seen.end()) {
            seen.push_back(sl);
            const TargetView t = targets(sl);
            t_pts += (double)t.n[0] + (double)t.n[1];
        }
    }
    if (total_src > 2000000000LL) return kPlanTooManySources;
    *mode = o.search_mode;
    if (o.search_mode == 4) {
        const double qi = (double)total_src * (double)bound;
        *mode = (t_pts > 0 && qi >= (double)o.graph_min_ratio * t_pts) ? 3 : 1;
        if (t_pts > 0 && qi >= (double)o.cell_min_ratio * t_pts && t_pts * 5120.0 <= (double)o.cell_rows_max_mb * 1048576.0) *mode = 5;
    }
    *lanes_q = (*mode == 1 && o.lanes_per_query_auto && total_src > 0 && total_src <= 131072) ? 8 : 1;
    return kPlanOk;
}

// Phase 2, the tile of the (optional) source sort.  Reads the grid dimensions of every item's target (after the front-end choice: the
// cell rows re-make a target's grid with a margin, and the tile count follows the grids).  2-D sort columns: 0.25 m tiles over every
// item's target footprint.  The bucket count is kept in 64 bits and the tile grows until the whole batch fits 2^26 buckets (km-scale
// submaps x large batches would otherwise overflow the int32 bucket numbering and ask for gigabytes of histogram).
template <class Targets>
inline float plan_sort_tile(int n_items, const lisreg_item* items, const Targets& targets)
{
    float tile = 0.25f;
    for (;;) {
        long long total = 0;
        for (int i = 0; i < n_items; ++i) {
            if (items[i].target < 0 || (size_t)items[i].target >= targets.size()) continue;
            const TargetView t = targets(items[i].target);
            for (int k = 0; k < 2; ++k) {
                const GridIndex& g = *t.g[k];
                total += (long long)std::max(1.0, std::ceil((double)g.nx * g.cell / tile)) * (long long)std::max(1.0, std::ceil((double)g.ny * g.cell / tile));
            }
        }
        if (total <= (1LL << 26)) return tile;
        tile *= 1.5f;
    }
}

// Phase 3, the item, segment and block tables.  Reads the items, their initial poses, the grids of their targets, the tile, the lanes
// per query and the feature-count guard of `prm`; fills the registrations' start states, one segment per (item, kind), the 256-query
// workgroups and (lanes_q > 1) the kBlockQ / lanes_q-query workgroups of the search kernel, the slots the batch uses in order of first
// use, and counts the items that fail the guard into prm.n_guard_failed (:598; the done counter's value after a reset).  The items'
// argument checks live here: the first bad item ends the loop with its error, the tables filled so far left as they are.
struct ItemTables {
    std::vector<ItemState>& items;        // sized n_items by the caller
    std::vector<Segment>&   segs;         // } empty on entry
    std::vector<BlockDesc>& blocks;       // }
    std::vector<BlockDesc>& blocks_q;     // }
    std::vector<int>&       slots;        // }
    int n_elems, n_buckets;               // out: source points of the batch, sort buckets (at least 1)
};
template <class Targets>
inline PlanError plan_item_tables(int n_items, const lisreg_item* items, const float* T_init, const Targets& targets, float tile, int lanes_q,
                                  DevParams& prm, ItemTables& out)
{
    const int qpb = kBlockQ / lanes_q;                  // queries per workgroup of the kQ-lane search (blocks_q)
    int flat = 0, bucket = 0;
    for (int i = 0; i < n_items; ++i) {
        const lisreg_item& in = items[i];
        if (in.fmt != LISREG_FMT_DEVICE) return kPlanItemFormat;
        if (in.n_corner < 0 || in.n_surf < 0 || (in.n_corner > 0 && !in.src_corner) || (in.n_surf > 0 && !in.src_surf)) return kPlanNullSource;
        if (in.target < 0 || (size_t)in.target >= targets.size() || !targets(in.target).valid) return kPlanNoTarget;
        if (std::find(out.slots.begin(), out.slots.end(), in.target) == out.slots.end()) out.slots.push_back(in.target);
        const TargetView t = targets(in.target);
        ItemState& st = out.items[(size_t)i];
        memset(&st, 0, sizeof st);
        memcpy(st.T_init, T_init + 6 * (size_t)i, 24);
        memcpy(st.T, st.T_init, 24);
        st.degenerate_in = in.degenerate_in;
        st.imu = in.imu;
        st.n_sc = in.n_corner; st.n_ss = in.n_surf;
        if (!(st.n_sc > prm.edge_min && st.n_ss > prm.surf_min)) ++prm.n_guard_failed;
        st.blk_begin = (int)out.blocks.size();
        for (int k = 0; k < 2; ++k) {
            Segment sg;
            memset(&sg, 0, sizeof sg);
            sg.src = static_cast<const float4*>(k == 0 ? in.src_corner : in.src_surf);
            sg.n = k == 0 ? in.n_corner : in.n_surf;
            sg.item = i; sg.kind = k; sg.target = in.target * 2 + k;
            sg.flat_base = flat; sg.bucket_base = bucket;
            const GridIndex& g = *t.g[k];
            sg.tox = g.ox; sg.toy = g.oy; sg.toz = g.oz;
            sg.inv_tile = 1.f / tile;
            sg.tnx = std::max(1, (int)ceilf(g.nx * g.cell / tile));
            sg.tny = std::max(1, (int)ceilf(g.ny * g.cell / tile));
            sg.tnz = 1;
            const int seg_id = (int)out.segs.size();
            out.segs.push_back(sg);
            for (int s = 0; s < sg.n; s += kBlockQ)
                out.blocks.push_back(BlockDesc{ seg_id, s, std::min(kBlockQ, sg.n - s), i });
            if (lanes_q > 1)
                for (int s = 0; s < sg.n; s += qpb)
                    out.blocks_q.push_back(BlockDesc{ seg_id, s, std::min(qpb, sg.n - s), i });
            flat += sg.n;
            bucket += sg.tnx * sg.tny;
        }
        st.blk_count = (int)out.blocks.size() - st.blk_begin;
    }
    out.n_elems = flat;
    out.n_buckets = std::max(bucket, 1);
    return kPlanOk;
}

// Phase 6, the table for rebuilding every target index of this batch in ONE launch sequence (rebuild_targets_each_run), and the
// strip-form verdict.  Reads the batch's slots, their targets' clouds, buffers and grids, and the options "index_strip_cells",
// "index_strip_cap" and "index_build"; fills one TargetSeg per (slot, kind) with its strip geometry, the targets' 256-point blocks and
// kPartChunkHost-point chunks, the totals, and decides whether every grid fits the strip form (strips per target, cells per strip).
// auto = the strip form whenever the grids fit it: measured faster from 2 own-target items up (index 0.063 vs 0.078 ms) to 256 (2.2 vs
// 5.3 ms), and equal for the single shared submap of configs[1].
struct TargetTables {
    std::vector<TargetSeg>& tsegs;        // } empty on entry
    std::vector<BlockDesc>& tblocks;      // }
    std::vector<BlockDesc>& tchunks;      // }
    int t_elems, t_buckets, t_strips, t_max_units, t_max_ucells;
    bool strip_now;                       // the verdict ("index_build" = 1 with strip_now false is the caller's to refuse)
};
template <class Targets>
inline void plan_target_tables(const std::vector<int>& slots, const Targets& targets, const BatchOptions& o, TargetTables& out)
{
    int tflat = 0, tbucket = 0, tstrip = 0;
    out.t_max_units = 0; out.t_max_ucells = 0;
    bool strips_fit = true;
    for (int slot : slots)
        for (int k = 0; k < 2; ++k) {
            const TargetView t = targets(slot);
            const GridIndex& g = *t.g[k];
            TargetSeg ts;
            memset(&ts, 0, sizeof ts);
            ts.raw = t.raw[k]; ts.sorted_out = t.sorted[k]; ts.cell_start_out = t.cell_start[k];
            ts.n = t.n[k]; ts.n_cells = t.n[k] > 0 ? t.n_cells[k] : 0;
            ts.flat_base = tflat; ts.bucket_base = tbucket;
            ts.ox = g.ox; ts.oy = g.oy; ts.oz = g.oz; ts.inv_cell = g.inv_cell;
            ts.nx = g.nx; ts.ny = g.ny; ts.nz = g.nz;
            ts.grid_id = slot * 2 + k;
            ts.strip_base = tstrip;
            // cells per strip: a batch of one or two targets (a shared submap: configs[1]) wants more, smaller strips than the 2048 cells that suit
            // a batch of hundreds — its strip build is a handful of workgroups (k_strip_build<true> 22 -> 15.6 us with 1024; configs[3] loses
            // 2.7 % with it): "index_strip_cells" = 0 (default) picks by the number of targets in the batch
            const int strip_cells = o.strip_cells > 0 ? o.strip_cells : (slots.size() <= 2 ? 1024 : 2048);
            ts.ystrip = std::max(1, std::min(ts.ny, (strip_cells + ts.nz / 2) / std::max(ts.nz, 1)));
            // wide grids: fewer, longer strips so that nx * nstrips stays inside the partition histogram (kMaxStrips bins)
            if (ts.nx > 0 && ts.nx <= kMaxStrips) {
                const int max_nstrips = std::max(1, kMaxStrips / ts.nx);
                ts.ystrip = std::max(ts.ystrip, (ts.ny + max_nstrips - 1) / max_nstrips);
            }
            ts.nstrips = (ts.ny + ts.ystrip - 1) / ts.ystrip;
            const int id = (int)out.tsegs.size();
            out.tsegs.push_back(ts);
            for (int s = 0; s < ts.n; s += kBlockQ) out.tblocks.push_back(BlockDesc{ id, s, std::min(kBlockQ, ts.n - s), 0 });
            for (int s = 0; s < ts.n; s += kPartChunkHost) out.tchunks.push_back(BlockDesc{ id, s, std::min(kPartChunkHost, ts.n - s), 0 });
            tflat += ts.n; tbucket += ts.n_cells;
            if (ts.n > 0) {
                const int units = ts.nx * ts.nstrips;
                tstrip += units; out.t_max_units = std::max(out.t_max_units, units); out.t_max_ucells = std::max(out.t_max_ucells, ts.ystrip * ts.nz);
                strips_fit = strips_fit && units <= kMaxStrips;
            }
        }
    out.t_elems = tflat; out.t_buckets = std::max(tbucket, 1); out.t_strips = tstrip;
    strips_fit = strips_fit && ((size_t)out.t_max_ucells + 1) * 4 + (size_t)o.strip_cap * 6 + 8192 <= kStripLdsLarge;
    out.strip_now = strips_fit && o.index_build != 0;
}

// A batch whose registrations bring targets of their own (configs[3]: 256 candidate pairs, 256 x 6 MB of index) takes the dispatch order
// by TARGET whatever the front-end — whole targets per XCD, so that an L2 holds the one or two targets its CUs are working on instead of
// a slice of all eight-plus in flight.  (measured on configs[3], 256 own-target registrations through the cell walk: 13 539 reg/s against
// 13 716 in plain order — no gain, the walk is not bound by L2 misses either; the order by target is taken only with xcd_order = 1,
// profiles/r05_kernel_experiments.md)
inline bool many_targets(const BatchOptions& o, const PreparedBatch& b) { return b.batch_slots.size() >= 8 && o.xcd_order == 1; }

// XCD-aware dispatch order of the prepared batch's correspondence launches (lisreg_assoc.hip, launch_xcd_order)?  Auto: the graph and
// cell-row front-ends with >= 32 registrations and >= 2048 blocks (measured: +2.5 % at 64 scans, +4.9 % at 256; with 8 big scans the
// sectors are unevenly loaded and it costs 2 %; the walk front-end gains nothing)
inline bool xcd_order_wanted(const BatchOptions& o, const PreparedBatch& b)
{
    return b.lanes_q != 8 &&
           (((b.mode_now == 3 || b.mode_now == 5) && (o.xcd_order == 1 || (o.xcd_order == 2 && b.n_blocks >= 2048 && b.n_items >= 32))) ||
            (many_targets(o, b) && o.xcd_order != 0 && b.n_blocks >= 2048));
}

// does this batch want the reach words of option "row_reach" (cell rows, targets rebuilt inside every run)?
inline bool reach_marks_wanted(const BatchOptions& o, const PreparedBatch& b) { return b.mode_now == 5 && o.rebuild_targets_each_run && o.row_reach != 0; }

// The split point of an interleaved run: the batch is cut in two at the first item boundary at or past the middle of the workgroups.
// (a lop-sided cut — a half under a quarter of the blocks — hides nothing: no split, both zero)
struct Split { int item = 0, blk = 0; };
inline Split plan_split(const std::vector<ItemState>& items, int n_items, int n_blocks)
{
    Split s;
    for (int i = 1; i < n_items; ++i)
        if (items[(size_t)i].blk_begin * 2 >= n_blocks) { s.item = i; s.blk = items[(size_t)i].blk_begin; break; }
    if (s.blk * 4 < n_blocks || (n_blocks - s.blk) * 4 < n_blocks) s = Split();
    return s;
}

// The cut of a FREE-RUNNING interleaved run ("interleave" = 2, and the runs the library splits by itself): the item boundary nearest to
// `share_permille` thousandths of the workgroups (the earlier of two equally near ones) among the boundaries that leave neither part
// under a quarter of the blocks; where no boundary qualifies, what plan_split returns — so this form engages on every batch the even
// form engages on.  kFreeRunShare is measured, not derived (profiles/interleave_uneven.md): 64 scans against one submap gain 1.8-1.9 % over
// the unsplit run with the first part at 0.30, 0.33 or 0.40 of the workgroups and 0.85 % with equal halves.  On the timeline the smaller
// part's solves wait behind the larger part's resident workgroups, both parts keep one iteration period, and the larger part runs only
// its last launch alone.
constexpr int kFreeRunShare = 400;
inline Split plan_split_uneven(const std::vector<ItemState>& items, int n_items, int n_blocks, int share_permille = kFreeRunShare)
{
    Split s;
    long long best = -1;
    for (int i = 1; i < n_items; ++i) {
        const int blk = items[(size_t)i].blk_begin;
        if ((long long)blk * 4 < n_blocks || ((long long)n_blocks - blk) * 4 < n_blocks) continue;
        const long long d = std::llabs((long long)blk * 1000 - (long long)n_blocks * share_permille);
        if (best < 0 || d < best) { best = d; s.item = i; s.blk = blk; }
    }
    return best < 0 ? plan_split(items, n_items, n_blocks) : s;
}

// May this run be cut in two parts on two streams, and in which form?  0: no; 1: halves whose launches alternate through events
// ("interleave" = 1, cut by plan_split); 2: free-running parts (cut by plan_split_uneven).  Never: the exact-arithmetic build, a run that
// can stop early from the host, eight lanes per query, a single registration, fewer workgroups than "interleave_min_blocks".
// "interleave" = 0, the default, leaves the choice to the library: the free-running form for the shape it was measured to pay on
// (profiles/interleave_uneven.md) — a fixed iteration count, at least kAutoSplitBlocks workgroups, at most kAutoSplitItems registrations
// (64 x 1800 scans against one submap: 40 gain 3.7 %, 64 gain 1.9 %, 128 lose 0.6 % — their solve launches are no empty chip; 256
// own-target registrations, configs[3], stay unsplit with them) and `alone`: no other context of the process ran a batch since this
// one's last run (batch_runner_alone) — and every other batch unsplit.  Raising "interleave_min_blocks" past the batch switches it off
// under every value of "interleave".
constexpr int kAutoSplitBlocks = 16384, kAutoSplitItems = 64;
inline int split_form(int n_blocks, int n_items, int lanes_q, int fixed_iters, bool can_stop, bool exact, int interleave, int min_blocks, bool alone)
{
    if (exact || can_stop || lanes_q != 1 || n_items < 2 || n_blocks < min_blocks) return 0;
    if (interleave == 0) return alone && fixed_iters > 0 && n_blocks >= kAutoSplitBlocks && n_items <= kAutoSplitItems ? 2 : 0;
    return interleave == 1 ? 1 : 2;
}
// ... and where: both zero for "not cut" (the form says no, or no item boundary qualifies)
inline Split plan_run_split(const BatchOptions& o, const PreparedBatch& b, bool can_stop, bool alone)
{
    const int form = split_form(b.n_blocks, b.n_items, b.lanes_q, b.prm.fixed_iters, can_stop, o.exact, o.interleave, o.interleave_min_blocks, alone);
    if (form == 0) return Split();
    return form == 1 ? plan_split(b.h_items, b.n_items, b.n_blocks) : plan_split_uneven(b.h_items, b.n_items, b.n_blocks);
}

}  // namespace lisreg
