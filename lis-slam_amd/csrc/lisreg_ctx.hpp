// lisreg_ctx.hpp — the context behind the C ABI (shared by the lisreg_api*.hip translation units; not installed).
#pragma once
#include <algorithm>
#include "lisreg_internal.hpp"

#include <atomic>
#include <map>
#include <memory>
#include <string>
#include <vector>

namespace lisreg {

// Owners of the context's GPU resources.  Each gives back what it holds in its destructor and can be moved but not copied, so a buffer,
// event or stream that is a member (of the context, a Target, a map, a ring frame, ...) or a local goes away with its owner, on error
// paths too.  A moved-from owner is empty; move-assignment first gives back what the target held.
template <hipError_t (*Free)(void*)>
struct OwnedMem {
    void*  p = nullptr;
    size_t cap = 0;
    OwnedMem() = default;
    OwnedMem(const OwnedMem&) = delete;
    OwnedMem& operator=(const OwnedMem&) = delete;
    OwnedMem(OwnedMem&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    OwnedMem& operator=(OwnedMem&& o) noexcept { if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~OwnedMem() { release(); }
    void release() { if (p) (void)Free(p); p = nullptr; cap = 0; }      // for memory that goes back early, on purpose: teardown is the destructor's
    template <class T> T* as() const { return reinterpret_cast<T*>(p); }
};

struct DevBuf : OwnedMem<hipFree> {
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        const size_t old_cap = cap;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        // doubling: a buffer that follows a growing map (the sliding local map, the key-frame ring) is reallocated a handful of times, not
        // every few frames — hipFree waits for the device and hipMalloc costs 0.1-1 ms, which showed as spikes in the frame loops
        // the head-room is capped (a GB-scale buffer growing by a byte must not ask for twice itself), and a refused request falls back
        // to the size that is actually needed
        size_t want = std::max(bytes + bytes / 4 + 256, std::min(2 * old_cap, bytes + ((size_t)256 << 20)));
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess && want > bytes + 256) { (void)hipGetLastError(); want = bytes + 256; e = hipMalloc(&p, want); }
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
};

// pinned host memory; the caller chooses the head-room: `want` bytes are allocated when `bytes` no longer fit
struct PinnedBuf : OwnedMem<hipHostFree> {
    hipError_t ensure(size_t bytes, size_t want)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want; else p = nullptr;
        return e;
    }
};

// an event / a stream of the context's own: made on first use by create(), converts to the raw handle
template <class H, hipError_t (*Destroy)(H)>
struct OwnedHandle {
    H h = nullptr;
    OwnedHandle() = default;
    OwnedHandle(const OwnedHandle&) = delete;
    OwnedHandle& operator=(const OwnedHandle&) = delete;
    OwnedHandle(OwnedHandle&& o) noexcept : h(o.h) { o.h = nullptr; }
    OwnedHandle& operator=(OwnedHandle&& o) noexcept { if (this != &o) { reset(); h = o.h; o.h = nullptr; } return *this; }
    ~OwnedHandle() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
struct Event : OwnedHandle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags) { reset(); const hipError_t e = hipEventCreateWithFlags(&h, flags); if (e != hipSuccess) h = nullptr; return e; }
};
struct Stream : OwnedHandle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { reset(); const hipError_t e = hipStreamCreateWithFlags(&h, flags); if (e != hipSuccess) h = nullptr; return e; }
};

// What a batch verifier keeps between calls (lisreg_batch_driver.hpp): the sources' finite points and covariances, the work table of a
// round, its partial and total records, and the pinned host sides of the table and of the totals; grow-only, like the rest
struct BatchBufs {
    DevBuf    src, cov, work, part, out;
    PinnedBuf host_work, host_out;
};

struct Target {
    bool      valid = false;
    int       n[2] = { 0, 0 };
    int       n_cells[2] = { 1, 1 };
    GridIndex g[2];
    lisreg::DevBuf    raw[2], sorted[2], cell_start[2];
    lisreg::DevBuf    nbr[2], nbr_meta[2];                // k-NN graph of the sorted points (search_mode 3)
    bool      graph_valid[2] = { false, false };
    lisreg::DevBuf    crow[2], crow_meta[2], crow_tab[2], crow_need[2], crow_omask[2], crow_scan[2], crow_scan_tmp[2];   // cell rows (search_mode 5)
    lisreg::DevBuf    crow_qmark[2], crow_reach[2];    // query marks of the running batch and their two-cell dilation (option "row_reach"; GridIndex::qmark)
    float     bbox[2][6] = { { 0 }, { 0 } };           // the cloud's bounding box (the grid is made from it, with or without a margin)
    int       grid_margin[2] = { 0, 0 };               // cells the grid reaches past the cloud on every side (the cell rows want two)
    int       omask_zero[2] = { 0, 0 };                // cells at the head of crow_omask known to be zero (launch_crow_classify / _build)
    int       crow_cap[2] = { 0, 0 };                  // rows allocated (= rows the classified index asked for when it was last sized)
    bool      crow_valid[2] = { false, false };
    bool      crow_chosen[2] = { false, false };       // a batch took the cell rows for this slot before: its next target is indexed with the margin at once
    bool      crow_too_big[2] = { false, false };      // the rows this target asks for exceed "cell_rows_max_mb" (auto: the batch takes the graph instead)
    bool      raw_external[2] = { false, false };     // LISREG_FMT_DEVICE: caller's memory, not ours
    const float4* raw_ptr[2] = { nullptr, nullptr };
    unsigned long long gen = 0;                        // bumped by every set_target of this slot (who built what is in here?)
};

// k = 1 search index over one cloud (lisreg_map_index_set)
struct MapIndex {
    bool      valid = false;
    int       n = 0, n_cells = 1;
    GridIndex g;
    DevBuf    raw, sorted, cell_start, g_dev;
    const float4* raw_ptr = nullptr;
};

// The dense voxel table of one target cloud (voxel_table_build in lisreg_api_cloud.hip): pcl::VoxelGrid's geometry at `resolution`, one
// record of kVoxelRec doubles per occupied voxel in ascending cell order, and the cell -> voxel table.  What a record holds behind the
// mean is its family's business (the statistics kernels of lisreg_ndt.hip / lisreg_vgicp.hip fill stats, cell and table)
constexpr int kVoxelRec = 10;      // doubles per voxel: mean [3], a symmetric 3 x 3 as its upper triangle [6], points
struct VoxelTable {
    int       n_voxels = 0;
    int       dims[3] = { 1, 1, 1 }, min_b[3] = { 0, 0, 0 };
    double    resolution = 0;
    DevBuf    stats;               // [n_voxels][kVoxelRec] doubles
    DevBuf    cell;                // [n_voxels] ints: cell id
    DevBuf    table;               // [dims product] ints: cell -> voxel, -1 none
};
// the kernels' view of a table (voxel_table_view)
struct VoxelView {
    const double* stats;
    const int*    table;
    int    d0, d1, d2, m0, m1, m2;
    double inv_res;
};

// the Gaussians of one NDT target (lisreg_ndt.hip: lisreg_ndt_set_target): stats = mean, upper triangle of the inverse covariance, finite
// points; the table names the voxels that became a Gaussian only; and a search grid over the target's finite points, its own copy (the
// fitness score of lisreg_ndt_align_batch searches it)
struct NdtTarget : VoxelTable {
    bool      valid = false;
    int       n_occupied = 0, n_valid = 0;
    DevBuf    vflag;               // [n_voxels] ints: became a Gaussian
    int       n_points = 0;        // finite points
    GridIndex grid;                // the search grid (pts = sorted, cell_start = cells)
    float     bb[6] = { 0, 0, 0, 0, 0, 0 };   // the finite bounding box
    DevBuf    sorted;              // [n_points] float4 by grid cell, .w = index among the finite points
    DevBuf    cells;               // [nx * ny * nz + 1] ints
};

// the voxel statistics of one VGICP target (lisreg_vgicp.hip: lisreg_vgicp_set_target): stats = mean, upper triangle of the mean
// covariance, points; and its own copy of the search grid the distributions were made with (the fitness score of
// lisreg_vgicp_align_batch searches it)
struct VgicpTarget : VoxelTable {
    bool      valid = false;
    int       n_points = 0;
    GridIndex grid;                // the search grid (pts = sorted, cell_start = cells)
    float     bb[6] = { 0, 0, 0, 0, 0, 0 };   // the finite bounding box
    DevBuf    sorted;              // [n_points] float4 by grid cell, .w = index among the finite points
    DevBuf    cells;               // [nx * ny * nz + 1] ints
};

// one FastGICP target (lisreg_fgicp.hip: lisreg_fgicp_set_target): its own copies of what the distributions leave in the context's scratch
struct FgicpTarget {
    bool      valid = false;
    int       n_points = 0;        // finite points
    GridIndex grid;                // the search grid (pts = sorted, cell_start = cells)
    float     bb[6] = { 0, 0, 0, 0, 0, 0 };   // the finite bounding box
    DevBuf    sorted;              // [n_points] float4 by grid cell, .w = index among the finite points
    DevBuf    cells;               // [nx * ny * nz + 1] ints
    DevBuf    orig;                // [n_points] ints: index among the finite points -> index in the caller's cloud
    DevBuf    cov;                 // [n_points][6] doubles by index among the finite points
};

// device-resident sliding local map (lisreg_api_localmap.hip)
struct LocalMap {
    bool   valid = false;
    DevBuf cls[5];                 // dynamic, pole, ground, building, outlier (map frame)
    int    n[5] = { 0, 0, 0, 0, 0 };
    DevBuf tgt[2];                 // corner / surf registration targets of the last extract
    int    n_tgt[2] = { 0, 0 };
    int    feature_point_num = 0;
    double bound[6] = { 0, 0, 0, 0, 0, 0 };
};

// the <= 19 newest key frames of the odometry node in the map frame (lisreg_api_localmap.hip: lisreg_keyframes_*)
struct KeyframeRing {
    bool valid = false;
    bool payload_is_label = false;  // fourth channel of the kept records: label (vote) or intensity (average) in the voxel grids
    struct Frame { DevBuf cloud[2]; int n[2] = { 0, 0 }; };     // corner, surf
    std::vector<Frame> frames;      // oldest first
    DevBuf cat[2], tgt[2];
    int    n_tgt[2] = { 0, 0 };
    // the target built by the last lisreg_keyframes_target: still current while no frame was pushed, the leaf sizes are the same and the
    // registration slot still holds it (the reference rebuilds the identical clouds and kd-trees for every sweep, :185-207)
    bool   built = false;
    float  built_leaf[2] = { 0.f, 0.f };
    int    built_slot = -1;
    unsigned long long built_gen = 0;
};

struct PackPool;           // host feeder threads (lisreg_api_feed.hip)
struct LoopDet;            // loop-closure candidate databases and their scratch (lisreg_loop.hip)
// (both are incomplete here: their deleters are defined next to the types)
struct PackPoolDelete { void operator()(PackPool* p) const; };
struct LoopDetDelete { void operator()(LoopDet* p) const; };
struct PackChunk { const unsigned char* src; lisreg_dpoint* dst; int n, stride, fmt; int pinned; };      // <= 64 k points of one host cloud; pinned: the DMA engine may read src

struct RcclApi {
    void* handle = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, const void* /* ncclUniqueId by value, 128 B */, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
};

// ---- the batch pipeline's host state (lisreg_batch_prepare / run_impl / lisreg_batch_fetch), grouped by who may write it --------------------
// Options: written only by lisreg_set_option (and, for the length of one call, lisreg_align's trace_cap / fetch_trace_records).  They
// survive every call; prepare, run and fetch read them through a const reference.
struct BatchOptions {
    int       early_stop_chunk = -1;        // iterations between host looks at the finished-counter; -1 auto, 0 never
    int       fetch_trace_records = 0;      // lisreg_align: trace records copied out together with the results
    int       trace_cap = 0;
    int       index_build = 2;                          // 0 bucket sort, 1 strip form (error if a grid does not fit it), 2 strip form whenever it fits
    int       strip_cells = 0, strip_cap = 2048;        // cells per strip aimed at (0: 1024 for a batch of one or two targets, else 2048); points per strip of the small-workgroup variant
    int         row_reach = 2;                          // option "row_reach": rows only for the cells the batch's queries come within a metre of (runs that rebuild their targets);
                                                        // 2: of those, only the cells a query starts in or that lie within half a metre of a target point
    bool      count_searches = false;
    bool      dump_neighbors = false;   // tests: keep the five neighbour ids of every query of the last iteration run
    int       search_mode = 4;           // 1 per-lane cell walk, 3 k-NN graph scan, 5 cell rows,
                                         // 4 auto: 3 when the prepared batch asks enough queries per target point to pay for the graph, else 1
    bool      lanes_per_query_auto = true;
    int       cell_min_ratio = 110;      // auto: query-iterations per target point from which the cell rows pay (they cost more than the graph to build and
                                         // halve the first iterations of a batch).  Round 6, rows filtered by the query marks: 16 scans against 200 k points
                                         // (92) draw, 24 (138) win 1.5 %, 32 (184) win 7 % (170 in rounds 4-5: 24 scans lost 4 %, 32 won 2 %)
    int       cell_rows_max_mb = 16384;  // auto: cell rows only while the targets' rows are expected to fit this (about 5 KB per target point)
    int       graph_min_ratio = 60;      // auto: query-iterations per target point from which the graph build pays (measured break-even ~55)
    int       interleave = 0;            // "interleave": big batches that run a fixed number of iterations are cut in two parts iterating on two
                                         // streams, each part's solves underneath the other part's correspondence launch (run_impl).  0 (default):
                                         // the library's choice — free-running parts for the batches choose_split names (one lane per query, at
                                         // least 16384 workgroups, at most 64 registrations, run by lisreg_batch_run, no other context running batches in between), unsplit otherwise; 1 two halves whose launches
                                         // alternate through events; 2 free-running, cut by plan_split_uneven.  Measured on configs[1] (round 5):
                                         // 24.09 k reg/s off, 21.7 k alternating (a cross-stream hand-off costs more than the solve it hides),
                                         // 24.5 k free-running (two launches then share the chip and their durations stop being a launch's own:
                                         // 122 us per half against 98); today's figures: profiles/interleave_uneven.md — bit-identical results
                                         // either way (tests)
    int       interleave_min_blocks = 8192;   // workgroups from which a run is interleaved (each part should still fill the chip; tests lower it;
                                              // raised past a batch it keeps that batch unsplit under every value of "interleave")
    int       xcd_order = 2;             // XCD-aware dispatch order of the correspondence launches: 0 off, 1 on (graph front-end), 2 auto (graph front-end, >= 32 registrations, >= 2048 blocks)
    int       cell_anchor_until = 1;     // graph front-end: GN iterations 1 .. this also try an anchor out of the query's own grid column
    bool      canonical_ties = false;    // "canonical_ties" (always on with exact_arithmetic)
    bool      exact = false;             // "exact_arithmetic": the correspondence launches and the pose cache run the reference's arithmetic (lisreg_assoc.hip)
    int       sort_sources = 2;          // 0: keep the caller order, 1: 2-D column sort, 2: auto (probe the order at prepare time)
    float     first_pass_r = 0.45f;
    bool      rebuild_targets_each_run = false;
};

// The prepared batch: what lisreg_batch_prepare decided.  Constant until the next prepare, except `live`; prepare fills it field by field
// (the host vectors keep their capacity: a single-frame lisreg_align prepares once per frame).
struct PreparedBatch {
    lisreg_params params;
    DevParams prm;                       // (a run hands the kernels a copy with its own reach_miss and cell_anchor_until)
    int       n_items = 0, n_blocks = 0, n_segs = 0, n_elems = 0, n_buckets = 0;
    int       mode_now = 1;              // front-end of the prepared batch
    int       lanes_q = 1;               // lanes per query of the prepared batch (8 for small walk-mode batches)
    bool      sort_now = false;          // the sort verdict
    bool      strip_now = false;         // the strip-form verdict
    std::vector<int> batch_slots;           // target slots used by the prepared batch
    std::vector<BlockDesc> h_blocks;      // 256-query workgroups: partial rows, sorts, probes
    std::vector<BlockDesc> h_blocks_q;    // lanes_q > 1: kBlockQ / lanes_q queries per workgroup of the search kernel
    std::vector<Segment>   h_segs;
    std::vector<ItemState> h_items;
    std::vector<TargetSeg> h_tsegs;
    std::vector<BlockDesc> h_tblocks;
    std::vector<BlockDesc> h_tchunks;          // the same targets in chunks of kPartChunkHost points (strip form of the build)
    int       t_strips = 0, t_max_units = 0, t_max_ucells = 0;
    int       t_elems = 0, t_buckets = 0;
    // ---- what changes while the batch stays prepared, each with its writers --------------------------------------------------------------
    struct Live {
        bool  prepared = false;          // prepare sets it; dropped by set_target, the options that change what prepare decides, ensure_crows
                                         // (a grid re-made with the rows' margin) and lisreg_align
        bool  reach_ready = false;       // prepare made the reach words of this batch's targets; cleared by a fetch that saw too many misses
        bool  xcd_cached = false;        // the dispatch-order table of this batch is made (by prepare, or by the last run that needed another one:
                                         // runs reuse it); cleared by option "xcd_order"
        int   xcd_split_blk = 0;         // ... for a run cut at this workgroup (one table per part, ids relative to the part); 0: the whole batch's
        bool  items_reset = false;       // the device registrations are in their start-of-run state (prepare, or the run before: launch_finalize); a run clears it while it runs
        bool  one_shot = false;          // prepared by a synchronous entry point (lisreg_align_batch, lisreg_align) for the one run it enqueues right behind
        int   reach_miss_seen = 0;       // the cumulative miss count the last fetch read (prepare: 0)
        int   runs_since_fetch = 0;      // run counts, prepare and fetch clear
    } live;
};

// What the last run did: written by run_impl and lisreg_batch_fetch, read by lisreg_get_option
struct LastRun {
    bool      xcd_now = false;           // the XCD-aware dispatch order was used
    bool      reach_now = false;         // its rows were built for the reached cells only ("row_reach")
    bool      interleaved_now = false;   // it ran as two halves
    int       reach_miss_last = 0;       // query-iterations of the last fetched run that found their cell without rows
    std::vector<float> h_results;        // the last fetch's result records
};

// What the context remembers from one batch to the next
struct BatchMemory {
    int       probe_items = -1, probe_elems = -1, probe_age = 0; bool probe_verdict = false;   // the batch shape the order was last probed on (auto): batches of a stream are alike ("sort_sources" forgets it)
    int       reach_backoff = 0;         // batches still to be prepared without the marks after a run that missed too often ("row_reach" clears it)
    int       strip_zero_ints = 0;       // leading ints of strip_tab known to be zero (a strip build hands its counters back clean)
    int       last_launches = 0;         // Gauss-Newton iterations the last fetched batch ran (its slowest item): where run_impl looks first
    int       degenerate = 0;            // isDegenerate member (odomEstimationNode.cpp:67)
    std::vector<float> last_trace;       // last align trace (host copy)
    int       last_trace_n = 0;
};

}  // namespace lisreg

struct lisreg_ctx {
    int          device = 0;
    lisreg::Stream own_stream;
    hipStream_t  stream = nullptr;           // own_stream, or the caller's (lisreg_set_stream): not owned
    std::string  err;
    std::vector<lisreg::Target> targets;
    unsigned long long   target_gen = 0;
    lisreg::DevBuf       grids_dev;
    bool         grids_dirty = true;
    lisreg::PinnedBuf grids_host;           // pinned staging of the GridIndex table (upload_grids does not wait for the stream)
    lisreg::Event grids_done;               // the last upload has left the staging buffer
    // sort scratch (shared by target build and source sort; stream-ordered so reuse is safe)
    lisreg::DevBuf hist, bucket_start, scan_tmp, elem_bucket, elem_sub, tmp_bucket, tmp_sub, tmp_idx, tmp_pts, bbox_dev, bbox_scratch;
    // batch
    lisreg::DevBuf blocks, segs, items, sorted_all, order_all, partials, results, trace, src_upload, raw_upload, dbg_nn, blocks_q, coef, coef_ok, nn, counters, tseg_dev, tblk_dev, tchunk_dev, strip_tab, done_dev, xcd_tab,
           vox_in, vox_lab, vox_order, vox_sidx, vox_head, vox_slot, vox_start, vox_out, vox_outlab, vox_M,
           ft_owner, ft_flag, ft_pos, ft_scan, ft_col, ft_range, ft_src, ft_curv, ft_picked, ft_label, ft_rlists, ft_rcounts,
           ft_lists, ft_counts, ft_rings, ft_gather, ft_cat, ft_bounds, ft_dsk_tab, ft_dsk_pts, ft_dsk_misc, ft_dsk_time;
    // laser pretreatment (lisreg_pretreat.hip): startOri / endOri per sweep, per-point ring / ori, per-workgroup partials, result headers, the
    // sweep table of a batch; staging of a host sweep and of its results
    lisreg::DevBuf pt_ends, pt_ring, pt_ori, pt_blk, pt_hdr, pt_tab, pt_in, pt_out, pt_time;
    lisreg::PinnedBuf pt_hdr_host;
    // motion compensation (lisreg_api_motion.hip): the job table of a batch; staging of a host sweep, of its times and of its result
    lisreg::DevBuf mo_tab, mo_in, mo_time, mo_out;
    // lisreg_voxel_downsample_batch (lisreg_voxel_batch.hip): [cloud table | chunk table] uploaded per call followed by the per-cloud
    // state and the result table the device writes; the chunks' bounding boxes, the list of big voxels and its counter; the pinned host
    // sides of the upload and of the results.  The sort itself runs in the sort scratch and the vox_* buffers above.
    lisreg::DevBuf vb_tab, vb_part, vb_big;
    lisreg::PinnedBuf vb_host;
    // lisreg_semantic_split_batch (lisreg_semantic_batch.hip): [frame table | tile table] uploaded per call followed by the tiles' counts /
    // bases and the result table the device writes; the pinned host sides of the upload and of the results.  lisreg_concat_device_batch:
    // its job table.
    lisreg::DevBuf sb_tab, cb_tab;
    lisreg::PinnedBuf sb_host;
    // RangeNet++ projection and labelling (lisreg_rangenet.hip): the pixel keys (all empty between calls: rn_keys_clean), per-workgroup
    // valid-pixel counts, per-sweep counts, the sweep table of a batch, staging of a host sweep, the label image when the caller wants none,
    // the per-pixel range image of the kNN clean-up (written in full by every call that reads it: no state between calls)
    lisreg::DevBuf rn_keys, rn_blk, rn_hdr, rn_tab, rn_in, rn_img, rn_rng;
    lisreg::PinnedBuf rn_hdr_host;
    bool         rn_keys_clean = false;
    // host feeder (lisreg_api_feed.hip): clouds packed to 16-byte records by a few threads into pinned staging, uploaded on a copy stream
    std::unique_ptr<lisreg::PackPool, lisreg::PackPoolDelete> pack_pool;
    int          feeder_threads = 8;
    lisreg::PinnedBuf pack_host[2];
    lisreg::DevBuf pack_dev[2];
    int            feeder_engine = 1;                    // 0: the copy engine takes no chunks; 1: when idle (default); 2: whenever a packed chunk is not ready; 3: the same and one chunk up front, ready or not (tests)
    int            pack_stolen = 0, pack_chunks_n = 0;   // last lisreg_stage_host_items: chunks the copy engine took / all chunks
    lisreg::DevBuf pack_raw[2];                // structs that crossed the link as they are (chunks the copy engine took over), packed on the device
    lisreg::PinnedBuf up_host;                 // pinned staging of lisreg_upload_cloud
    lisreg::Event pack_copied[2];                         // the uploads into device buffer b are done (recorded on copy_stream)
    lisreg::Event pack_free[2];                           // the batch reading device buffer b has run (recorded on stream)
    hipEvent_t   pack_pending = nullptr;                  // uploads the next prepared batch has to wait for (one of pack_copied: not owned)
    lisreg::Event pack_raw_done;                          // the copy engine's last read of the CALLER's pinned memory (chunks it took over)
    int          pack_flip = 0, pack_last = -1, pack_in_use = -1;
    lisreg::Stream copy_stream;
    lisreg::Stream pack_stream;                           // chunks the copy engine takes as they are: raw copy + k_pack_cloud (never on copy_stream: see lisreg_stage_host_items)
    lisreg::Event pack_kernels_done;                      // recorded on pack_stream behind the last k_pack_cloud of a staging call
    std::vector<lisreg::PackChunk> pack_chunks;
    std::vector<std::atomic<int>> pack_done;
    std::map<int, lisreg::MapIndex> maps;             // by slot (sparse: the local maps keep theirs at 60000 + id)
    std::vector<lisreg::LocalMap> localmaps;
    std::vector<lisreg::KeyframeRing> keyrings;
    lisreg::DevBuf lm_in, lm_tmp, lm_bbox, exact_trig;
    // submap gather (lisreg_globalmap.hip): the segment table + matrices of a call, staged in one of two pinned slots (a call does not wait
    // for the GPU, so the slot of the call before may still be read by its upload: gm_up[s] = the upload out of slot s is through);
    // host destinations: two chunk buffers, "the kernel into buffer b has run" (on stream), "buffer b has been copied out" (on copy_stream)
    lisreg::DevBuf    gm_tab, gm_chunk[2];
    lisreg::PinnedBuf gm_host[2];
    lisreg::Event     gm_up[2], gm_kernel[2], gm_copied[2];
    int               gm_flip = 0;
    lisreg::DevBuf map_stage;                          // lisreg_map_index_set_batch: host clouds of a batch, packed, in one upload
    lisreg::DevBuf mp_pts, mp_flag, mp_pos, mp_idx, mp_cnt, mp_d2, mp_out, icp_state, icp_partials, icp_cur, icp_items, map_tab, map_tsegs, map_tblocks;
    // lisreg_icp_gn_match_batch (lisreg_api_icpgn.hip), its own (icp_state / icp_partials / icp_cur stay the single calls' and
    // lisreg_icp_align_batch's): [states | block table | packed host sources] in pinned memory and on the device, the partial rows, the
    // neighbour of every (item, source point)
    lisreg::PinnedBuf gnb_host;
    lisreg::DevBuf gnb_tab, gnb_part, gnb_nn;
    // one evaluation of the NDT, VGICP and FastGICP verifiers (eval_totals in lisreg_fp64_sums.hpp): per-workgroup partial sums, their
    // total and its pinned landing area
    lisreg::DevBuf eval_part, eval_out;
    lisreg::PinnedBuf eval_host;
    // NDT registration (lisreg_ndt.hip): targets by slot (apart from the map-index slots), the cleaned target cloud and the staged source,
    // the voxel counters
    std::map<int, lisreg::NdtTarget> ndt;
    lisreg::DevBuf ndt_pts, ndt_src, ndt_cnt;
    // VGICP registration (lisreg_vgicp.hip): targets by slot (apart from the map-index and the NDT slots); of the cloud whose
    // distributions were made last (a target being set, or a source): the staged records, finite flags, their scan, the finite points and
    // their indices, the same points by search-grid cell with the cells' starts, the covariances, neighbour rows and covariance rows of the
    // test hook; the finite-point count
    std::map<int, lisreg::VgicpTarget> vgicp;
    lisreg::DevBuf vg_raw, vg_flag, vg_pos, vg_pts, vg_idx, vg_sorted, vg_cells, vg_cov, vg_nbr, vg_rows, vg_cnt;
    // FastGICP registration (lisreg_fgicp.hip): targets by slot (a numbering of their own); of the source being aligned: the sorted
    // position of every finite point's correspondent (-1: none), the six entries of its M, its squared distance (the test hook); the
    // correspondence rows of the test hook by the caller's index
    std::map<int, lisreg::FgicpTarget> fgicp;
    lisreg::DevBuf fg_pair, fg_M, fg_d2, fg_rows_i, fg_rows_d;
    // lisreg_fgicp_set_target_batch (lisreg_fgicp_target_batch.hip): [job table | tile table] and, behind the read-back, [descriptors |
    // sort segments | blocks] uploaded per call, with the per-target results the device writes; the tiles' finite counts, bases and
    // boxes; the pinned host side of all of it.  The finite points of all targets are compacted into vg_pts; the sort runs in the sort
    // scratch.  ft_enqueues / ft_syncs: what the last call enqueued and how often it waited (lisreg_fgicp_target_batch_counts)
    lisreg::DevBuf ft_tab, ft_part;
    lisreg::PinnedBuf ft_host;
    int          ft_enqueues = 0, ft_syncs = 0;
    // lisreg_vgicp_set_target_batch (lisreg_vgicp_target_batch.hip) runs the same two phases on the same tables; besides: its own table
    // of [voxel descriptors | fill chunks] uploaded per call with [first voxels | voxel counts] the device writes, the counter and the
    // list of the voxels a wavefront sums, the pinned host side.  The covariances of all targets go to vg_cov, their indices to vg_idx,
    // the voxel sort runs in the sort scratch and vox_order / vox_sidx / vox_head / vox_slot / vox_start.  vt_enqueues / vt_syncs: as above
    // (lisreg_vgicp_target_batch_counts)
    lisreg::DevBuf vt_tab, vt_big;
    lisreg::PinnedBuf vt_host;
    int          vt_enqueues = 0, vt_syncs = 0;
    // lisreg_ndt_set_target_batch (lisreg_ndt_target_batch.hip): the same two phases without the distributions, and the voxel half on
    // the tables above (a context is single-threaded and every such call ends in a wait, so the families share them): [voxel descriptors
    // | fill chunks | blocks of the raw records] uploaded per call with [first voxels | voxel counts | occupied and valid counts] the
    // device writes.  nt_enqueues / nt_syncs: as above (lisreg_ndt_target_batch_counts)
    int          nt_enqueues = 0, nt_syncs = 0;
    // lisreg_fgicp_align_batch (lisreg_fgicp_batch.hip), lisreg_vgicp_align_batch (lisreg_vgicp_batch.hip), lisreg_ndt_align_batch
    // (lisreg_ndt_batch.hip) and lisreg_gicp_align_batch (lisreg_gicp_batch.hip): a set of buffers each (a call of one family leaves the
    // others' alone; NDT's has no covariances), and the pairs and M FastGICP's items keep from a search to the sums after it
    lisreg::BatchBufs fgb, vgb, ndb, gcb;
    lisreg::DevBuf fgb_pair, fgb_M;
    lisreg::PinnedBuf done_host;            // one int
    lisreg::PinnedBuf stage_host;           // pinned staging of the per-batch tables
    lisreg::Event stage_done;
    lisreg::PinnedBuf fetch_host;           // pinned landing area of results (+ trace)
    lisreg::Stream side_stream;                         // strip build: the big-strip kernel runs here, forked from / joined to `stream`
    lisreg::Event ev_fork, ev_join;
    lisreg::Event ev_ab, ev_ba;                         // interleaved runs: "half A's / half B's correspondence launch is through"
    int       feeder_numa = 1;           // packing threads bound to the CPUs of the device's NUMA node (those this process owns)
    int       feeder_node = -1, feeder_cpus = 0;       // what that found: the node, the CPUs bound to
    // the batch pipeline's host state (lisreg_api_batch.hip), by who may write it: see the four structs above
    lisreg::BatchOptions  opt;
    lisreg::PreparedBatch batch;
    lisreg::LastRun       last;
    lisreg::BatchMemory   mem;
    // profiling
    bool      profiling = false;
    std::vector<lisreg::Event> ev;
    std::vector<int>        ev_kind;        // kind of the interval STARTING at event i: 0 assoc, 1 solve, 2 index, -1 none
    std::vector<int>        ev_sidx;        // stream the event was recorded on: 0 the context's, 1 the side stream (interleaved runs)
    double    timing[5] = { 0, 0, 0, 0, 0 };
    // RCCL
    lisreg::RcclApi   rccl;
    void*     comm = nullptr;
    int       comm_nranks = 0;
    // FEPSC loop-closure candidate detection (lisreg_loop.hip): created on first use
    std::unique_ptr<lisreg::LoopDet, lisreg::LoopDetDelete> loopdet;
};

namespace lisreg {
void feeder_stop(lisreg_ctx* c);       // drains the copy and pack streams and joins the packing threads (lisreg_destroy, before the staging goes)
// ---- lisreg_api_ctx.hip: what the entry points of every translation unit share ------------------------------------------------------
int  ctx_fail(lisreg_ctx* c, int code, const std::string& msg);     // keeps the text for lisreg_last_error and returns `code`
int  bad(lisreg_ctx* c, const std::string& msg);                    // ctx_fail(c, LISREG_ERR_ARG, msg)
// The (cloud, n, stride, fmt) arguments of an entry point.  accepted_formats: the fmt_bit()s this entry point takes — any other value of
// fmt is refused; allow_empty: n == 0 passes.  Refused besides: n < 0, a NULL cloud with n > 0, and host structs whose stride is too
// short for what pack_cloud reads of them (12 bytes; XYZIL 22, the label; XYZI_PACKED 16).  Device records: the stride is not read.
constexpr unsigned fmt_bit(int fmt) { return 1u << fmt; }
constexpr unsigned kFmtDevice = fmt_bit(LISREG_FMT_DEVICE) | fmt_bit(LISREG_FMT_DEVICE_XYZI);
constexpr unsigned kFmtPackable = fmt_bit(LISREG_FMT_DEVICE) | fmt_bit(LISREG_FMT_XYZI) | fmt_bit(LISREG_FMT_XYZIL) | fmt_bit(LISREG_FMT_XYZIRT);   // what pack_cloud reads, and records
constexpr unsigned kFmtSweep = fmt_bit(LISREG_FMT_XYZI) | fmt_bit(LISREG_FMT_XYZI_PACKED) | fmt_bit(LISREG_FMT_DEVICE_XYZI);      // a raw sweep: x y z intensity
int  check_cloud(lisreg_ctx* c, const char* who, const void* cloud, int n, int stride, int fmt, unsigned accepted_formats, bool allow_empty);
// do the byte ranges [a, a + na) and [b, b + nb) meet?  (a NULL pointer or an empty range meets nothing)
bool spans_overlap(const void* a, size_t na, const void* b, size_t nb);
// the side stream and its fork / join events, created on first use; false if they cannot be made (the caller then runs on one stream)
bool ensure_side_stream(lisreg_ctx* c);
// pack PCL structs (stride/format of common.h:9,25-35) into 16-B device records
void pack_cloud(const void* cloud, int n, int stride, int fmt, lisreg_dpoint* out);
// n packed records from the caller's local `h` into `into` (grown to fit, at least one record) by a pageable copy on the context's stream,
// waited for because `h` is a local; n == 0 copies nothing and waits for nothing
int  upload_packed(lisreg_ctx* c, const lisreg_dpoint* h, size_t n, DevBuf& into);
// one cloud as 16-byte device records: the caller's own memory for LISREG_FMT_DEVICE, else pack_cloud + upload_packed into `into`
int  stage_records(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, DevBuf& into, const float4** out);
// `output` of an align(): the n staged records `raw` under Rt = [R|t] (3 x 4, row-major, float, like lisreg_transform_cloud) into
// aligned_out, waited for.  LISREG_FMT_DEVICE: 16-byte records in device memory; else the caller's structs (`source`, `stride`) with
// their x y z replaced, by way of `scratch`
int  emit_aligned(lisreg_ctx* c, const float4* raw, int n, const float Rt[12], const void* source, int stride, int fmt, DevBuf& scratch,
                  void* aligned_out);
// each coordinate's finite minimum and maximum over n > 0 device records: launch_bbox on the context's stream, read back and waited for.
// A cloud without a finite point gives min > max; Inf coordinates come back as they are: what to refuse is the caller's business
int  cloud_bbox(lisreg_ctx* c, const float4* pts, int n, float bb[6]);
// lisreg_upload_cloud's body: fmt is LISREG_FMT_XYZI (payload 0), _XYZIL (uint16 at byte 20), _XYZI_PACKED (the float at byte 12) or
// kPackIntensity (PCL PointXYZI with the float intensity at byte 16 as the payload)
constexpr int kPackIntensity = 0x100;
int  upload_records(lisreg_ctx* c, const void* cloud, int n, int stride_bytes, int fmt, void* dev_out);
// grid geometry from a bounding box; cell edge grows if the box would need too many cells
void make_grid(const float bb[6], int n, GridIndex* g, int* n_cells, int margin_cells = 0);
SortBuffers sort_buffers(lisreg_ctx* c);
int  ensure_sort_scratch(lisreg_ctx* c, size_t n_elems, size_t n_buckets);
// ---- lisreg_vgicp.hip: what the fast_gicp family's units share -----------------------------------------------------------------------------
// The distributions of one cloud of n device records (the k nearest points of every finite point within the cloud, plane-regularised
// covariances): afterwards c->vg_pts holds its *m_out finite points in input order, c->vg_idx their indices in the cloud, c->vg_flag /
// c->vg_pos the finite flags and their exclusive scan, c->vg_sorted / c->vg_cells the same points by search-grid cell, c->vg_cov the
// m x 6 covariances by index among the finite points and, if nbr_dev is given, nbr_dev the n x k neighbour rows.  bb: the finite bounding
// box.  edge: the search grid's cell edge, <= 0: chosen from the cloud's density.  grid_out (may be null): the search grid.  All of it
// is the context's scratch: the next call overwrites it.
int  vg_distributions(lisreg_ctx* c, const char* who, const float4* raw, int n, int k, double plane_eps, float edge, float bb[6], int* m_out,
                      int* nbr_dev, GridIndex* grid_out);
// Its grid half, which lisreg_ndt_set_target calls too: the *m_out finite points of n device records with the finite bounding box bb into
// c->vg_pts (with c->vg_idx, c->vg_flag, c->vg_pos as above) and by search-grid cell into c->vg_sorted / c->vg_cells; fewer than
// min_points is refused.  mark >= 0: that profiling interval is opened in front of the gather.  *g: the grid, on the context's scratch.
int  vg_search_grid(lisreg_ctx* c, const char* who, const float4* raw, int n, const float bb[6], float edge, int min_points, int mark,
                    int* m_out, GridIndex* g);
// The geometry of the search grid over the finite bounding box bb of m > 0 finite points under `edge` (as vg_distributions'): what
// vg_search_grid chooses, as a function of its own for lisreg_fgicp_set_target_batch.  Host arithmetic only.  A grid has at most
// kVgGridMaxCells cells.
constexpr long long kVgGridMaxCells = 1LL << 22;
struct VgGrid { float ox, oy, oz, cell, inv_cell; int nx, ny, nz; };
void vg_grid_geometry(const float bb[6], int m, float edge, VgGrid* g);
// out[29] = the n_part partial records of 29 doubles added in a fixed order (one wavefront: sum_records of lisreg_fp64_sums.hpp)
void launch_eval_total(const double* part, int n_part, double* out, hipStream_t st);
// ---- lisreg_api_cloud.hip: the voxel sort of one cloud and the voxel table of a target ---------------------------------------------------
// n device records sorted by the voxel index of `d` (d.span is set here, for at most 2^22 buckets over `total` cells): afterwards
// c->vox_order / c->vox_sidx hold the sorted positions' records and cell ids, c->vox_head / c->vox_slot the voxel heads and their scan;
// *n_vox = the occupied voxels, read back and waited for.  mark >= 0: that profiling interval is opened in front of the sort.
int  voxel_sort_cloud(lisreg_ctx* c, const char* who, const float4* pts, int n, VoxelDesc d, long long total, int mark, int* n_vox);
// The table of n device records (no NaN coordinate among them) with the finite bounding box bb at `resolution`, ready for the family's
// statistics kernels: T's geometry, voxel_sort_cloud, c->vox_start = the voxels' starts, T.stats / T.cell sized and T.table all -1.
// Refused: a grid of more than 2^26 cells (the table is dense; `table_word` names it in the text: "cell table", "voxel table").
int  voxel_table_build(lisreg_ctx* c, const char* who, const char* table_word, const float4* pts, int n, const float bb[6], double resolution,
                       int mark, VoxelTable& T);
// Its geometry alone (host arithmetic): min_b / dims, the sort's keys (d->span = 1: the sort chooses it) and the cells in all.  false:
// the grid is refused and *why is voxel_table_build's text behind "<who>: "
bool voxel_table_geometry(const float bb[6], double resolution, const char* table_word, int min_b[3], int dims[3], VoxelDesc* d,
                          long long* total, std::string* why);
VoxelView voxel_table_view(const VoxelTable& T);
// the records of a table on the host, those with flag[v] != 0 only if `flag` is given ([n_voxels] ints on the device), at most `capacity`:
// cell ids, point counts, means [3] and the six doubles behind them
int  voxel_table_read(lisreg_ctx* c, const VoxelTable& T, const DevBuf* flag, int* cell_ids, int* counts, double* means, double* sym6, int capacity);
// ---- lisreg_api.hip -------------------------------------------------------------------------------------------------------------------
// (sidx 1: the mark goes on the side stream — the second half of an interleaved run; an interval runs from a mark to the next on the SAME stream)
void ctx_prof_mark(lisreg_ctx* c, int kind_of_next_interval, int sidx = 0);      // 0 correspondence kernel, 1 solve, 2 index build, -1 nothing
void ctx_prof_collect(lisreg_ctx* c);
// Which context of the process enqueued the last batch run: true if it was `c` itself or nobody (`c` takes the place either way).  A process
// that runs batches on several contexts in turn is overlapping them itself: the library then leaves its own split of a batch (the default
// of option "interleave") alone — two batches in flight on two contexts, each cut in two, ran 5 % slower than uncut
// (profiles/interleave_uneven.md).  lisreg_destroy forgets a context that goes.
bool batch_runner_alone(const lisreg_ctx* c);
DevParams make_dev_params(const lisreg_params& p);                  // the literals of lisreg_params as the kernels want them
// the target indices a batch asks for (lisreg_api_batch.hip); the index itself must already be enqueued on the stream
int  ensure_graph(lisreg_ctx* c, Target& t, int k, bool launch);
int  ensure_crows(lisreg_ctx* c, Target& t, int k, bool may_decline = false, long long* rows_left = nullptr);
int  ensure_reach(lisreg_ctx* c, Target& t, int k, bool on);
CrowBuffers crow_buffers(Target& t, int k, bool with_reach = false, bool near_only = false);
int  upload_grids(lisreg_ctx* c);
}  // namespace lisreg

#define HIPCHK(c, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return lisreg::ctx_fail((c), LISREG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
