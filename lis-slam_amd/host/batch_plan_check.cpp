// batch_plan_check.cpp — the planning functions of the batch pipeline (csrc/lisreg_batch_plan.hpp: front-end choice, sort tile, item /
// segment / block tables, target-rebuild tables and strip verdict, split point, xcd_order_wanted) against the loops they were cut out
// of, kept here in closed form on a context of loose fields (closed_prepare / closed_split / closed_xcd_order_wanted below: what
// lisreg_batch_prepare and run_impl ran before they went through the plan; the independent restatement, never a wrapper around it).
// Both sides are given the same seeded random batch — items, targets' grids and counts, options, parameters — and every table, count
// and verdict is compared as bytes.  The generator aims at the edges named in kEdgeName and the program counts how often each was met;
// it fails if one was not.  Host code only: no HIP call, no library of the project.
// g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../csrc batch_plan_check.cpp
#include "lisreg_batch_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

using namespace lisreg;

namespace {

enum Edge { kEmptySegment, kSeg256m1, kSeg256, kSeg256p1, kLanes8, kSrc131071, kSrc131072, kSrc131073, kRefused2e9, kSlotUnset, kSlotOutOfRange,
            kTileGrewTwice, kNxAboveMaxStrips, kNxBelowMaxStrips, kNy1, kYstrip1ByNz, kStripCellsSet2, kStripCellsSet3, kStripCellsUnset2,
            kStripCellsUnset3, kSplitLopSided, kSplitAtQuarter, kSplitTaken, kMode1, kMode3, kMode5, kStripNow, kStripRefused, kXcdWanted, kManyTargets, kEdges };
const char* const kEdgeName[kEdges] = { "empty_segment", "seg_256k-1", "seg_256k", "seg_256k+1", "lanes_q_8", "src_131071", "src_131072", "src_131073",
    "refused_2e9", "slot_unset", "slot_out_of_range", "tile_grew_twice", "nx_above_max_strips", "nx_below_max_strips", "ny_1", "ystrip_1_by_nz",
    "strip_cells_set_2_targets", "strip_cells_set_3_targets", "strip_cells_unset_2_targets", "strip_cells_unset_3_targets", "split_lop_sided",
    "split_at_quarter", "split_taken", "mode_1", "mode_3", "mode_5", "strip_now", "strip_refused", "xcd_wanted", "many_targets" };
long long hits[kEdges];

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    int pick(int n) { return (int)(next() % (uint64_t)n); }
    int range(int lo, int hi) { return lo + pick(hi - lo + 1); }
    float uni() { return (float)(next() >> 40) / (float)(1 << 24); }
};

// the context as the closed form knew it: loose fields
struct Ptr { void* p; template <class T> T* as() const { return reinterpret_cast<T*>(p); } };
struct LooseTarget {
    bool valid; int n[2]; int n_cells[2]; GridIndex g[2]; const float4* raw_ptr[2]; Ptr sorted[2], cell_start[2];
};
struct Loose {
    std::vector<LooseTarget> targets;
    int search_mode, graph_min_ratio, cell_min_ratio, cell_rows_max_mb; bool lanes_per_query_auto;
    int strip_cells, strip_cap, index_build, xcd_order;
    DevParams prm;
    int mode_now, lanes_q, n_items, n_blocks, n_segs, n_elems, n_buckets;
    std::vector<BlockDesc> h_blocks, h_blocks_q, h_tblocks, h_tchunks;
    std::vector<Segment> h_segs;
    std::vector<ItemState> h_items;
    std::vector<TargetSeg> h_tsegs;
    std::vector<int> batch_slots;
    int t_elems, t_buckets, t_strips, t_max_units, t_max_ucells; bool strip_now;
    float tile;
};
enum { kOk = 0, kTooMany, kFormat, kNullSource, kNoTarget, kStripRefusedErr };

// lisreg_batch_prepare's host loops as they stood, HIP calls left out
int closed_prepare(Loose* c, int n_items, const lisreg_item* items, const float* T_init)
{
    c->n_items = n_items;
    c->h_blocks.clear(); c->h_segs.clear(); c->h_items.assign((size_t)n_items, ItemState());
    c->batch_slots.clear();
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
        if (total_src > 2000000000LL) return kTooMany;
        c->mode_now = c->search_mode;
        if (c->search_mode == 4) {
            const double qi = (double)total_src * (double)c->prm.bound;
            c->mode_now = (t_pts > 0 && qi >= (double)c->graph_min_ratio * t_pts) ? 3 : 1;
            if (t_pts > 0 && qi >= (double)c->cell_min_ratio * t_pts && t_pts * 5120.0 <= (double)c->cell_rows_max_mb * 1048576.0) c->mode_now = 5;
        }
        c->lanes_q = (c->mode_now == 1 && c->lanes_per_query_auto && total_src > 0 && total_src <= 131072) ? 8 : 1;
        if (total_src >= 131071 && total_src <= 131073) ++hits[kSrc131071 + (int)(total_src - 131071)];
    }
    float tile = 0.25f;
    int grown = 0;
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
        ++grown;
    }
    if (grown >= 2) ++hits[kTileGrewTwice];
    c->tile = tile;
    const int qpb = kBlockQ / c->lanes_q;
    c->h_blocks_q.clear();
    int flat = 0, bucket = 0;
    for (int i = 0; i < n_items; ++i) {
        const lisreg_item& in = items[i];
        if (in.fmt != LISREG_FMT_DEVICE) return kFormat;
        if (in.n_corner < 0 || in.n_surf < 0 || (in.n_corner > 0 && !in.src_corner) || (in.n_surf > 0 && !in.src_surf))
            return kNullSource;
        if (in.target < 0 || (size_t)in.target >= c->targets.size() || !c->targets[(size_t)in.target].valid) {
            ++hits[in.target < 0 || (size_t)in.target >= c->targets.size() ? kSlotOutOfRange : kSlotUnset];
            return kNoTarget;
        }
        if (std::find(c->batch_slots.begin(), c->batch_slots.end(), in.target) == c->batch_slots.end()) c->batch_slots.push_back(in.target);
        const LooseTarget& t = c->targets[(size_t)in.target];
        ItemState& st = c->h_items[(size_t)i];
        memset(&st, 0, sizeof st);
        memcpy(st.T_init, T_init + 6 * (size_t)i, 24);
        memcpy(st.T, st.T_init, 24);
        st.degenerate_in = in.degenerate_in;
        st.imu = in.imu;
        st.n_sc = in.n_corner; st.n_ss = in.n_surf;
        if (!(st.n_sc > c->prm.edge_min && st.n_ss > c->prm.surf_min)) ++c->prm.n_guard_failed;
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
            if (sg.n == 0) ++hits[kEmptySegment];
            else if (sg.n % 256 == 255) ++hits[kSeg256m1];
            else if (sg.n % 256 == 0) ++hits[kSeg256];
            else if (sg.n % 256 == 1 && sg.n > 1) ++hits[kSeg256p1];
        }
        st.blk_count = (int)c->h_blocks.size() - st.blk_begin;
    }
    c->n_blocks = (int)c->h_blocks.size();
    c->n_segs = (int)c->h_segs.size();
    c->n_elems = flat;
    c->n_buckets = std::max(bucket, 1);
    ++hits[c->mode_now == 1 ? kMode1 : c->mode_now == 3 ? kMode3 : kMode5];
    if (c->lanes_q == 8) ++hits[kLanes8];
    c->h_tsegs.clear(); c->h_tblocks.clear(); c->h_tchunks.clear();
    int tflat = 0, tbucket = 0, tstrip = 0;
    c->t_max_units = 0; c->t_max_ucells = 0;
    bool strips_fit = true;
    for (int slot : c->batch_slots)
        for (int k = 0; k < 2; ++k) {
            LooseTarget& t = c->targets[(size_t)slot];
            TargetSeg ts;
            memset(&ts, 0, sizeof ts);
            ts.raw = t.raw_ptr[k]; ts.sorted_out = t.sorted[k].as<float4>(); ts.cell_start_out = t.cell_start[k].as<int>();
            ts.n = t.n[k]; ts.n_cells = t.n[k] > 0 ? t.n_cells[k] : 0;
            ts.flat_base = tflat; ts.bucket_base = tbucket;
            ts.ox = t.g[k].ox; ts.oy = t.g[k].oy; ts.oz = t.g[k].oz; ts.inv_cell = t.g[k].inv_cell;
            ts.nx = t.g[k].nx; ts.ny = t.g[k].ny; ts.nz = t.g[k].nz;
            ts.grid_id = slot * 2 + k;
            ts.strip_base = tstrip;
            const int strip_cells = c->strip_cells > 0 ? c->strip_cells : (c->batch_slots.size() <= 2 ? 1024 : 2048);
            ts.ystrip = std::max(1, std::min(ts.ny, (strip_cells + ts.nz / 2) / std::max(ts.nz, 1)));
            if (ts.ny > 1 && (strip_cells + ts.nz / 2) / std::max(ts.nz, 1) < 1) ++hits[kYstrip1ByNz];
            if (ts.nx > 0 && ts.nx <= kMaxStrips) {
                const int max_nstrips = std::max(1, kMaxStrips / ts.nx);
                ts.ystrip = std::max(ts.ystrip, (ts.ny + max_nstrips - 1) / max_nstrips);
            }
            ++hits[ts.nx > kMaxStrips ? kNxAboveMaxStrips : kNxBelowMaxStrips];
            if (ts.ny == 1) ++hits[kNy1];
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
    if (c->batch_slots.size() == 2) ++hits[c->strip_cells > 0 ? kStripCellsSet2 : kStripCellsUnset2];
    if (c->batch_slots.size() == 3) ++hits[c->strip_cells > 0 ? kStripCellsSet3 : kStripCellsUnset3];
    c->t_elems = tflat; c->t_buckets = std::max(tbucket, 1); c->t_strips = tstrip;
    strips_fit = strips_fit && ((size_t)c->t_max_ucells + 1) * 4 + (size_t)c->strip_cap * 6 + 8192 <= kStripLdsLarge;
    c->strip_now = strips_fit && c->index_build != 0;
    if (c->strip_now) ++hits[kStripNow];
    if (c->index_build == 1 && !c->strip_now) { ++hits[kStripRefused]; return kStripRefusedErr; }
    return kOk;
}

// run_impl's split point as it stood
void closed_split(const Loose* c, int* split_item_out, int* split_blk_out)
{
    int split_item = 0, split_blk = 0;
    for (int i = 1; i < c->n_items; ++i)
        if (c->h_items[(size_t)i].blk_begin * 2 >= c->n_blocks) { split_item = i; split_blk = c->h_items[(size_t)i].blk_begin; break; }
    if (split_blk > 0 && (split_blk * 4 < c->n_blocks || (c->n_blocks - split_blk) * 4 < c->n_blocks)) ++hits[kSplitLopSided];
    if (split_blk * 4 < c->n_blocks || (c->n_blocks - split_blk) * 4 < c->n_blocks) { split_item = 0; split_blk = 0; }     // (a lop-sided cut hides nothing)
    if (split_blk > 0 && (c->n_blocks - split_blk) * 4 == c->n_blocks) ++hits[kSplitAtQuarter];
    if (split_blk > 0) ++hits[kSplitTaken];
    *split_item_out = split_item; *split_blk_out = split_blk;
}

bool closed_xcd_order_wanted(const Loose* c)
{
    const bool many_targets = c->batch_slots.size() >= 8 && c->xcd_order == 1;
    if (many_targets) ++hits[kManyTargets];
    return c->lanes_q != 8 &&
           (((c->mode_now == 3 || c->mode_now == 5) && (c->xcd_order == 1 || (c->xcd_order == 2 && c->n_blocks >= 2048 && c->n_items >= 32))) ||
            (many_targets && c->xcd_order != 0 && c->n_blocks >= 2048));
}

// the plan's view of the same targets
struct LooseTargets {
    const std::vector<LooseTarget>& v;
    size_t size() const { return v.size(); }
    TargetView operator()(int slot) const
    {
        const LooseTarget& t = v[(size_t)slot];
        return TargetView{ t.valid, { t.n[0], t.n[1] }, { t.n_cells[0], t.n_cells[1] }, { &t.g[0], &t.g[1] }, { t.raw_ptr[0], t.raw_ptr[1] },
                           { t.sorted[0].as<float4>(), t.sorted[1].as<float4>() }, { t.cell_start[0].as<int>(), t.cell_start[1].as<int>() } };
    }
};

// lisreg_batch_prepare's order of the plan's phases (lisreg_api_batch.hip), HIP calls left out
int plan_prepare(const std::vector<LooseTarget>& targets, const BatchOptions& o, PreparedBatch& b, int n_items, const lisreg_item* items,
                 const float* T_init, float* tile_out)
{
    const LooseTargets tv{ targets };
    b.n_items = n_items;
    b.h_blocks.clear(); b.h_segs.clear(); b.h_items.assign((size_t)n_items, ItemState());
    b.batch_slots.clear();
    std::vector<int> seen;
    if (plan_front_end(n_items, items, tv, o, b.prm.bound, seen, &b.mode_now, &b.lanes_q) != kPlanOk) return kTooMany;
    const float tile = plan_sort_tile(n_items, items, tv);
    *tile_out = tile;
    b.h_blocks_q.clear();
    ItemTables it{ b.h_items, b.h_segs, b.h_blocks, b.h_blocks_q, b.batch_slots, 0, 0 };
    switch (plan_item_tables(n_items, items, T_init, tv, tile, b.lanes_q, b.prm, it)) {
    case kPlanItemFormat: return kFormat;
    case kPlanNullSource: return kNullSource;
    case kPlanNoTarget: return kNoTarget;
    default: break;
    }
    b.n_blocks = (int)b.h_blocks.size(); b.n_segs = (int)b.h_segs.size(); b.n_elems = it.n_elems; b.n_buckets = it.n_buckets;
    b.h_tsegs.clear(); b.h_tblocks.clear(); b.h_tchunks.clear();
    TargetTables tt{ b.h_tsegs, b.h_tblocks, b.h_tchunks, 0, 0, 0, 0, 0, false };
    plan_target_tables(b.batch_slots, tv, o, tt);
    b.t_elems = tt.t_elems; b.t_buckets = tt.t_buckets; b.t_strips = tt.t_strips; b.t_max_units = tt.t_max_units; b.t_max_ucells = tt.t_max_ucells;
    b.strip_now = tt.strip_now;
    return o.index_build == 1 && !b.strip_now ? kStripRefusedErr : kOk;
}

template <class T>
bool same(const std::vector<T>& a, const std::vector<T>& b) { return a.size() == b.size() && (a.empty() || !memcmp(a.data(), b.data(), sizeof(T) * a.size())); }

GridIndex make_grid_index(Rng& r, int shape)
{
    GridIndex g;
    memset(&g, 0, sizeof g);
    g.ox = 200.f * r.uni() - 100.f; g.oy = 200.f * r.uni() - 100.f; g.oz = 10.f * r.uni() - 5.f;
    g.cell = 0.25f + 0.75f * r.uni(); g.inv_cell = 1.f / g.cell;
    g.nx = r.range(1, 300); g.ny = r.range(1, 300); g.nz = r.range(1, 40);
    switch (shape) {
    case 1: g.nx = r.range(3500, 4500); g.ny = r.range(3500, 4500); g.cell = 1.0f; g.inv_cell = 1.f; g.nz = r.range(1, 4); break;   // the tile grows twice at least
    case 2: g.nx = kMaxStrips + r.range(1, 900); g.ny = r.range(1, 6); g.nz = r.range(1, 8); break;
    case 3: g.ny = 1; break;
    case 4: g.nz = r.range(4200, 9000); g.ny = r.range(2, 40); g.nx = r.range(1, 40); break;                                     // ystrip = 1 by nz alone
    case 5: g.nx = r.range(2000, kMaxStrips); g.ny = r.range(2, 400); g.nz = r.range(1, 6); break;                                 // a few strips per ix only
    default: break;
    }
    return g;
}

}  // namespace

int main(int argc, char** argv)
{
    const int n_batches = argc > 1 ? atoi(argv[1]) : 2400;
    long long blocks_total = 0, items_total = 0;
    static float fake_points[4];               // the sources' and targets' addresses are copied, never read
    for (int bi = 0; bi < n_batches; ++bi) {
        Rng r{ 0x5eedull * 1000003ull + (uint64_t)bi };
        const int kind = bi % 12;              // what this batch aims at
        Loose L;
        BatchOptions o;
        PreparedBatch B;
        // targets
        const int n_targets = kind == 7 ? r.range(8, 12) : r.range(1, 4);
        L.targets.resize((size_t)n_targets + (size_t)r.pick(2));
        for (size_t s = 0; s < L.targets.size(); ++s) {
            LooseTarget& t = L.targets[s];
            memset(&t, 0, sizeof t);
            t.valid = s < (size_t)n_targets;
            for (int k = 0; k < 2 && t.valid; ++k) {
                const int shape = kind == 1 ? 1 : kind == 2 ? r.range(2, 5) : (r.pick(6) == 0 ? r.range(2, 5) : 0);
                t.g[k] = make_grid_index(r, shape);
                t.n[k] = r.pick(8) == 0 ? 0 : r.range(1, kind == 3 ? 400 : 60000);
                t.n_cells[k] = (int)std::min<long long>((long long)t.g[k].nx * t.g[k].ny * t.g[k].nz, 1LL << 30);
                t.g[k].n = t.n[k];
                t.raw_ptr[k] = reinterpret_cast<const float4*>(fake_points) + s * 2 + k;
                t.sorted[k].p = fake_points + 1; t.cell_start[k].p = fake_points + 2 + k;
            }
        }
        // options
        auto of = [&](std::initializer_list<int> l) { return *(l.begin() + r.pick((int)l.size())); };
        L.search_mode = o.search_mode = kind == 4 || kind == 5 ? 1 : of({ 1, 3, 4, 4, 4, 5 });
        L.graph_min_ratio = o.graph_min_ratio = of({ 60, 0, 1 << 30, 5 });
        L.cell_min_ratio = o.cell_min_ratio = of({ 110, 0, 1 << 30, 20 });
        L.cell_rows_max_mb = o.cell_rows_max_mb = of({ 16384, 1, 64 });
        L.lanes_per_query_auto = o.lanes_per_query_auto = kind == 4 || kind == 5 || r.pick(4) != 0;
        L.strip_cells = o.strip_cells = r.pick(2) ? 0 : of({ 1, 512, 1024, 100000 });
        L.strip_cap = o.strip_cap = of({ 2048, 64, 16384 });
        L.index_build = o.index_build = of({ 2, 2, 0, 1 });
        L.xcd_order = o.xcd_order = r.pick(3);
        memset(&L.prm, 0, sizeof L.prm);
        L.prm.bound = r.range(1, 30); L.prm.edge_min = r.pick(3) ? -1 : 10; L.prm.surf_min = of({ 100, 0, 5000 });
        B.prm = L.prm;
        // items
        int n_items = kind == 6 || kind == 7 ? r.range(32, 48) : r.range(0, 9);
        if (kind == 8) n_items = r.range(2, 4);
        if (kind == 11) n_items = 2;
        std::vector<lisreg_item> items((size_t)n_items);
        std::vector<float> T_init(6 * (size_t)n_items + 1);
        for (float& v : T_init) v = r.uni() - 0.5f;
        for (int i = 0; i < n_items; ++i) {
            lisreg_item& in = items[(size_t)i];
            memset(&in, 0, sizeof in);
            in.fmt = LISREG_FMT_DEVICE;
            in.target = kind == 7 ? i % n_targets : r.pick(n_targets);
            auto count = [&]() {
                const int m = r.pick(8);
                if (m == 0) return 0;
                if (m == 1) return 256 * r.range(1, 12) + r.range(-1, 1);
                if (kind == 6 || kind == 7) return r.range(6000, 9000);      // enough workgroups for the auto order
                return r.range(1, 3000);
            };
            in.n_corner = count(); in.n_surf = count();
            if (kind == 8) { in.n_corner = i == 0 ? r.range(30000, 40000) : r.range(1, 2000); in.n_surf = i == 0 ? r.range(30000, 40000) : r.range(1, 600); }
            if (kind == 11) { in.n_corner = 256 * (i == 0 ? 3 : 1) * (bi % 7 + 1); in.n_surf = 0; }      // the second half is a quarter of the blocks exactly
            if (kind == 9 && i == 0) { in.n_corner = 1000000000 + r.pick(1000); in.n_surf = 1000000001 + r.pick(1000); }   // past 2e9 together
            in.degenerate_in = r.pick(2);
            in.imu.imu_available = r.pick(2); in.imu.imu_roll_init = r.uni(); in.imu.imu_pitch_init = r.uni();
        }
        if ((kind == 4 || kind == 5) && n_items > 0) {        // the eight-lane boundary: 131071, 131072 or 131073 source points in all
            long long rest = 131071 + r.pick(3);
            for (int i = 0; i < n_items; ++i) {
                items[(size_t)i].n_corner = i + 1 == n_items ? (int)(rest / 2) : r.range(0, 3000); rest -= items[(size_t)i].n_corner;
                items[(size_t)i].n_surf = i + 1 == n_items ? (int)rest : r.range(0, 3000); rest -= items[(size_t)i].n_surf;
            }
        }
        for (int i = 0; i < n_items; ++i) {
            items[(size_t)i].src_corner = items[(size_t)i].n_corner > 0 ? fake_points : nullptr;
            items[(size_t)i].src_surf = items[(size_t)i].n_surf > 0 ? fake_points + 1 : nullptr;
        }
        if (kind == 10 && n_items > 0) {                      // one bad item: a slot never set, a slot out of range, a wrong format, a NULL cloud
            lisreg_item& in = items[(size_t)r.pick(n_items)];
            switch (r.pick(5)) {
            case 0: in.target = -1 - r.pick(3); break;
            case 1: in.target = (int)L.targets.size() + r.pick(3); break;
            case 2: if (L.targets.size() > (size_t)n_targets) in.target = n_targets; else in.target = -1; break;
            case 3: in.fmt = LISREG_FMT_XYZI; break;
            default: in.n_surf = 7; in.src_surf = nullptr; break;
            }
        }
        // both sides
        float tile_new = 0.f;
        L.tile = 0.f; L.mode_now = B.mode_now = -1; L.lanes_q = B.lanes_q = -1;
        const int rc_closed = closed_prepare(&L, n_items, items.data(), T_init.data());
        const int rc_plan = plan_prepare(L.targets, o, B, n_items, items.data(), T_init.data(), &tile_new);
        bool ok = rc_closed == rc_plan && L.mode_now == B.mode_now && L.lanes_q == B.lanes_q;
        if (rc_closed == kTooMany) ++hits[kRefused2e9];
        else {
            ok = ok && !memcmp(&L.tile, &tile_new, 4) && same(L.h_items, B.h_items) && same(L.h_segs, B.h_segs) && same(L.h_blocks, B.h_blocks) &&
                 same(L.h_blocks_q, B.h_blocks_q) && same(L.batch_slots, B.batch_slots) && !memcmp(&L.prm, &B.prm, sizeof L.prm);
        }
        if (rc_closed == kOk || rc_closed == kStripRefusedErr) {
            ok = ok && L.n_blocks == B.n_blocks && L.n_segs == B.n_segs && L.n_elems == B.n_elems && L.n_buckets == B.n_buckets &&
                 same(L.h_tsegs, B.h_tsegs) && same(L.h_tblocks, B.h_tblocks) && same(L.h_tchunks, B.h_tchunks) && L.t_elems == B.t_elems &&
                 L.t_buckets == B.t_buckets && L.t_strips == B.t_strips && L.t_max_units == B.t_max_units && L.t_max_ucells == B.t_max_ucells &&
                 L.strip_now == B.strip_now;
        }
        if (ok && rc_closed == kOk) {
            int si = -1, sb = -1;
            closed_split(&L, &si, &sb);
            const Split s = plan_split(B.h_items, B.n_items, B.n_blocks);
            const bool xw = closed_xcd_order_wanted(&L);
            if (xw) ++hits[kXcdWanted];
            ok = si == s.item && sb == s.blk && xw == xcd_order_wanted(o, B) &&
                 (L.batch_slots.size() >= 8 && L.xcd_order == 1) == many_targets(o, B);
            blocks_total += L.n_blocks; items_total += n_items;
        }
        if (!ok) {
            printf("batch %d (kind %d) differs: rc %d / %d, mode %d / %d, lanes %d / %d, blocks %zu / %zu, tsegs %zu / %zu\n", bi, kind, rc_closed, rc_plan,
                   L.mode_now, B.mode_now, L.lanes_q, B.lanes_q, L.h_blocks.size(), B.h_blocks.size(), L.h_tsegs.size(), B.h_tsegs.size());
            return 1;
        }
    }
    // the row budget: the expression prepare and ensure_crows each wrote out
    for (int mb : { -5, 0, 1, 16, 16384, 2000000 })
        if (crow_row_budget(mb) != (long long)std::max(mb, 1) * 1048576LL / (long long)(sizeof(float4) * kGraphK + sizeof(float2))) { printf("row budget of %d MB differs\n", mb); return 1; }
    printf("batches %d items %lld blocks %lld hits", n_batches, items_total, blocks_total);
    bool all = true;
    for (int k = 0; k < kEdges; ++k) { printf(" %s=%lld", kEdgeName[k], hits[k]); all = all && hits[k] > 0; }
    if (!all) { printf("\nan edge was never met\n"); return 1; }
    printf("\nbatch_plan_check ok\n");
    return 0;
}
