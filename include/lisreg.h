/*
 * lisreg.h — C ABI of liblisreg.so: MI355X-native (gfx950, HIP) LOAM-style scan-to-submap registration.
 *
 * This header is the drop-in boundary for ONE hot path of QingzhiWang/LIS-SLAM: the private member
 * functions scan2SubMapOptimization() / subMap2SubMapOptimization() and everything they call
 *   copy #1  src/node/odomEstimationNode.cpp:596-1006      (plain PointXYZI, tau=1.0, 15 iters)
 *   copy #2  src/node/subMapOptmizationNode.cpp:1509-2001  (PointXYZIL, label weights, tau=2.0, 20 iters)
 *   copy #3  src/node/subMapOptmizationNode.cpp:4485-4977  (as #2, 30 iters, no IMU blend)
 * The reference has no FFI / plugin layer for this path; this header creates the seam.
 * Each entry point below cites the reference lines it replaces.  Plain pointers and sizes only; no C++ or
 * torch types; never throws; every function returns an int status (0 = OK) unless stated otherwise.
 *
 * Conventions
 *   pose      T[6] = {roll, pitch, yaw, x, y, z}, float32 — the reference's transformTobeMapped[6]
 *             (odomEstimationNode.cpp:66).  M(T) = pcl::getTransformation(x,y,z,roll,pitch,yaw) =
 *             Rz(yaw)*Ry(pitch)*Rx(roll) + t (src/core/common.cpp:54-57).
 *   clouds    host clouds are arrays of PCL point structs as the reference holds them
 *             (`cloud->points.data()`), i.e. stride 32 B, 16-B aligned: PointXYZI = {x,y,z,pad,intensity,pad*3},
 *             PointXYZIL = {x,y,z,pad,intensity,uint16 label,pad} (src/include/common.h:9,25-35).  Any
 *             stride >= 12 is accepted; `fmt` says where (whether) a label lives.
 *   device    device-resident clouds are arrays of lisreg_dpoint (16 B): x,y,z + 32-bit payload whose low
 *             16 bits are the label (0 when unlabelled).
 */
#ifndef LISREG_H_
#define LISREG_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LISREG_VERSION 1

/* ---- status codes (error conventions: SURVEY.md §8b "Error conventions") -------------------------------- */
#define LISREG_OK                        0
#define LISREG_NOT_ENOUGH_FEATURES       1   /* guard at odomEstimationNode.cpp:598,623-625 failed: T untouched */
#define LISREG_TOO_FEW_CORRESPONDENCES   2   /* every iteration hit the `< 50` early return (:870-872): no step, but transformUpdate (:622) still ran on T */
#define LISREG_LEAF_TOO_SMALL            3   /* VoxelGrid: dx*dy*dz overflows int32 — PCL warns and copies the input  */
#define LISREG_ERR_ARG                  -1
#define LISREG_ERR_HIP                  -2
#define LISREG_ERR_NO_TARGET            -3
#define LISREG_ERR_NOMEM                -4
#define LISREG_ERR_COMM                 -5

/* ---- cloud formats --------------------------------------------------------------------------------------- */
#define LISREG_FMT_XYZI    0   /* pcl::PointXYZI   : floats x@0 y@4 z@8, intensity@16                        */
#define LISREG_FMT_XYZIL   1   /* PointXYZIL       : as XYZI + uint16 label@20   (common.h:25-35)            */
#define LISREG_FMT_DEVICE  2   /* pointer is a DEVICE pointer to lisreg_dpoint[n] (stride ignored)           */
#define LISREG_FMT_DEVICE_XYZI 4 /* the same, but the 32-bit payload is a float intensity, not a label: only where a function says so
                                  * (lisreg_voxel_downsample averages it like PCL's PointXYZI centroid instead of taking a label vote;
                                  * lisreg_keyframes_push remembers it for the ring's voxel grids)                                      */

typedef struct lisreg_dpoint {   /* 16-B device record (SURVEY.md §8d "Device record")                        */
    float    x, y, z;
    uint32_t payload;            /* low 16 bits: semantic label (RangeNet learning class 0..19)                */
} lisreg_dpoint;

/* ---- the three reference call sites ---------------------------------------------------------------------- */
#define LISREG_VARIANT_ODOM      1   /* OdomEstimationNode::scan2SubMapOptimization      odomEstimationNode.cpp:596  */
#define LISREG_VARIANT_KEYFRAME  2   /* SubMapOdometryNode::scan2SubMapOptimization      subMapOptmizationNode.cpp:1509 */
#define LISREG_VARIANT_SUBMAP    3   /* SubMapOptmizationNode::subMap2SubMapOptimization subMapOptmizationNode.cpp:4485 */

/* Every literal / rosparam the path reads (SURVEY.md §5 "Config / flags"), gathered in one struct. */
typedef struct lisreg_params {
    int   max_iters;            /* loop bound 15 | 20 | 30            (:606 | :1520 | :4501)                   */
    int   fixed_iters;          /* >0: benchmark mode — run exactly this many iterations, no early exit        */
    float knn_sq_thresh;        /* pointSearchSqDis[4] < tau: 1.0 | 2.0 | 2.0   (:657,776 | :1610 | :4609)     */
    float conv_deg;             /* deltaR bound 0.005 | 0.003 | 0.002 (:969 | :1963 | :4962)                   */
    float conv_cm;              /* deltaT bound 0.05  | 0.03  | 0.02                                            */
    int   min_corr;             /* laserCloudSelNum < 50 -> no-op iteration (:870)                             */
    float eig_thresh;           /* degeneracy eigenvalue threshold 100 (:932)                                  */
    int   edge_min;             /* edgeFeatureMinValidNum (config/params.yaml:119 = -1)                        */
    int   surf_min;             /* surfFeatureMinValidNum (config/params.yaml:120 = 100)                       */
    float line_ratio;           /* lambda0 > 3*lambda1 (:692)                                                  */
    float plane_tol;            /* |n.p + d| > 0.2 invalidates the plane (:798)                                */
    float accept_s;             /* keep correspondence iff s > 0.1 (:734,814)                                  */
    int   use_label_weight;     /* w = 2 - LabelSorce[label] (subMapOptmizationNode.cpp:1671,1795)             */
    float label_score[32];      /* LabelSorce table, config/label.yaml:214-234, indexed by label; 20..31 default to 0 and labels
                                 * >= 32 read as 0: std::map::operator[] on a label the yaml does not list gives w = 2.0      */
    int   emulate_matp_shadow;  /* 1: reproduce the local-matP quirk; 0: keep P from iter 0 */
    int   skip_empty_target;    /* variant #3 skips a stage whose target cloud is empty (:4505-4509)           */
    int   use_imu_blend;        /* transformUpdate slerps roll/pitch toward IMU (#1,#2) or not (#3)            */
    float imu_rpy_weight;       /* imuRPYWeight (config/params.yaml:88 = 0.1)                                  */
    float rotation_tol;         /* rotation_tollerance (config/params.yaml:124 = 1000)                         */
    float z_tol;                /* z_tollerance (config/params.yaml:123 = 1000)                                */
} lisreg_params;

/* IMU scalars the path reads from cloud_info / semantic_info (msg/cloud_info.msg:4-10). */
typedef struct lisreg_imu {
    int   imu_available;        /* cloudInfo.imuAvailable   */
    float imu_roll_init;        /* cloudInfo.imuRollInit    */
    float imu_pitch_init;       /* cloudInfo.imuPitchInit   */
} lisreg_imu;

typedef struct lisreg_stats {
    int   iters;                /* iterCount as the reference prints it (:620 | :1535 | :4517)                 */
    float deltaR, deltaT;       /* last computed (deg, cm); 100 if no iteration solved (member init :70-71)    */
    int   degenerate;           /* isDegenerate after the call (persists in the context, :67)                  */
    int   n_corr_last;          /* laserCloudSelNum of the last iteration run                                  */
    int   status;               /* LISREG_OK | LISREG_NOT_ENOUGH_FEATURES | LISREG_TOO_FEW_CORRESPONDENCES     */
} lisreg_stats;

/* Optional per-iteration trace (parity tests): LISREG_TRACE_STRIDE floats per iteration:
 *   [0] n_corr  [1..36] AtA row-major  [37..42] AtB  [43..48] X (after projection)  [49..54] T after update
 *   [55] 1 if this iteration solved (n_corr >= min_corr) else 0 */
#define LISREG_TRACE_STRIDE 56

/* One independent registration of a batch (independent frames / loop-closure candidate pairs). */
typedef struct lisreg_item {
    const void* src_corner; int n_corner;     /* source edge features   (laserCloudSharpCornerLast, :641)      */
    const void* src_surf;   int n_surf;       /* source planar features (laserCloudSharpSurfLast,  :757)      */
    int         stride_bytes;                 /* 32 for PCL structs; ignored for LISREG_FMT_DEVICE             */
    int         fmt;                          /* LISREG_FMT_*                                                  */
    int         target;                       /* target slot id from lisreg_set_target_slot (0 = default)      */
    int         degenerate_in;                /* isDegenerate carried in from the previous frame (usually 0)   */
    lisreg_imu  imu;
} lisreg_item;

typedef struct lisreg_ctx lisreg_ctx;

/* ---- lifecycle ------------------------------------------------------------------------------------------- */
int  lisreg_device_count(void);                                   /* number of visible HIP devices (0 if none)  */
int  lisreg_create(int device, lisreg_ctx** out);                 /* one context per caller thread (§8b Callers) */
void lisreg_destroy(lisreg_ctx* ctx);
const char* lisreg_last_error(const lisreg_ctx* ctx);             /* never NULL                                 */
/* Use an existing HIP stream (e.g. the caller's); NULL restores the context's own stream.  The switch drains the stream in use
 * before: a call on the new stream sees what was queued on the old one.  A caller's stream may be destroyed once it is no longer set.
 * Streams (pinned by tests/test_caller_stream.py, on a stream that is still busy producing the input when the call is made):
 *   - Every entry point reads its device inputs and writes its device outputs in the order of the context's stream, side streams of
 *     the library (interleaved halves, the strip build, the feeder's uploads) forking from and joining it: an input another
 *     operation of that stream is still producing needs no host synchronisation in front of the call, an output is ready for the next
 *     operation queued on that stream behind it.  Work the caller puts on ANY other stream is not ordered against the library.
 *   - Without waiting for the GPU return lisreg_batch_run, lisreg_concat_device, lisreg_submap_gather into device memory and
 *     lisreg_set_option("count_searches") (its zeroing goes behind a run still queued: counters belong to whole runs).
 *     lisreg_batch_prepare and lisreg_stage_host_items may wait (for a staging buffer of theirs whose copy is still queued); several
 *     prepare / run pairs, gathers or sweep batches queued behind one another each keep their own tables.  Every other entry point
 *     returns with its outputs complete (it hands counts or poses back to the host).
 *   - The library orders by itself what it owns: its device copy of a HOST target (lisreg_set_target* from host memory lands behind a
 *     run still queued against that slot — that run registers against the old cloud, also when it rebuilds its targets), the submap
 *     store (lisreg_submap_insert lands behind a gather still queued) and the search counters.
 *   - The caller's duty: device records the library only REFERENCES — a LISREG_FMT_DEVICE target or map index, the device sources of
 *     a prepared batch — must not be overwritten (other than in the order of the context's stream) or freed while a run that reads
 *     them is queued; with "rebuild_targets_each_run" every run re-reads the target's records. */
int  lisreg_set_stream(lisreg_ctx* ctx, void* hip_stream);
void* lisreg_get_stream(const lisreg_ctx* ctx);

/* Fill `p` with the literals of one of the three reference copies. */
int  lisreg_default_params(int variant, lisreg_params* p);

/* ---- target (local map / submap) ------------------------------------------------------------------------- */
/* Replaces kdtreeCornerFromMap->setInputCloud / kdtreeSurfFromMap->setInputCloud
 * (odomEstimationNode.cpp:602-603 | subMapOptmizationNode.cpp:1516-1517 | :4496-4497): builds the device search index
 * of the two target clouds.  Host clouds are copied to the device; LISREG_FMT_DEVICE clouds are REFERENCED, not copied —
 * the caller's records must stay valid and unchanged until the slot is set again or the context is destroyed (with the
 * option "rebuild_targets_each_run" every lisreg_batch_run re-reads them).  The index persists until the next call for
 * that slot, so a target shared by many registrations is built once.  Slot 0 is what lisreg_align uses.  A cloud with an
 * infinite coordinate, or with no finite point at all, is refused (LISREG_ERR_ARG); NaN points are simply never neighbours.
 * A cloud is limited to 2^28 - 1 points (the kernels address its 16-byte records by 32-bit byte offsets).
 * Supported coordinate range: every finite coordinate of the target, and of the transformed source points searched against it, below
 * 8192 m in magnitude.  The 5-NN front-ends (walk, graph scan, cell rows) prove their exactness with one millimetre of absolute slack,
 * which has to absorb the rounding of the cell faces they recompute (ox + ix * cell, and + cell): one float step of the coordinate in
 * all, 0.49 mm below 8192 m and 0.98 mm — the whole millimetre, with the 0.02 mm the cell assignment needs — from there on.  Beyond
 * the range the searches still run and still return true neighbours in all but face-grazing cases; they are no longer proven exact.
 * Keep the map frame's origin near the work (tests/test_far_frame.py runs at 8000 m). */
int  lisreg_set_target(lisreg_ctx* ctx, const void* corner, int n_corner,
                       const void* surf, int n_surf, int stride_bytes, int fmt);
int  lisreg_set_target_slot(lisreg_ctx* ctx, int slot, const void* corner, int n_corner,
                            const void* surf, int n_surf, int stride_bytes, int fmt);
/* Adapter for the submap API (subMap.h:435-777): concatenates class clouds in the reference's order —
 * corner = pole; surf = ground, building, dynamic (extractSlidingCloud subMapOptmizationNode.cpp:1408-1419;
 * extractSubMapCloud :3996-4007) — then behaves as lisreg_set_target_slot.  NULL/0 classes are skipped. */
int  lisreg_target_from_classes(lisreg_ctx* ctx, int slot,
                                const void* pole, int n_pole, const void* ground, int n_ground,
                                const void* building, int n_building, const void* dynamic, int n_dynamic,
                                int stride_bytes, int fmt);

/* ---- registration ---------------------------------------------------------------------------------------- */
/* Replaces the whole body of scan2SubMapOptimization() (odomEstimationNode.cpp:596-626 and the two copies):
 * guard, GN loop {cornerOptimization :633, surfOptimization :749, combineOptimizationCoeffs :829,
 * LMOptimization :852}, transformUpdate :976.  T: in = initial guess, out = result.  The context keeps
 * isDegenerate across calls like the reference's member (:67). */
int  lisreg_align(lisreg_ctx* ctx,
                  const void* src_corner, int n_corner, const void* src_surf, int n_surf,
                  int stride_bytes, int fmt,
                  const lisreg_params* params, const lisreg_imu* imu /* may be NULL */,
                  float T[6], lisreg_stats* stats /* may be NULL */);

/* Batch of independent registrations (same semantics per item as lisreg_align with its own isDegenerate).
 * T: n_items x 6 floats in/out; stats: n_items entries (may be NULL).  Returns 0 if the batch ran; per-item
 * outcomes are in stats[i].status. */
int  lisreg_align_batch(lisreg_ctx* ctx, int n_items, const lisreg_item* items,
                        const lisreg_params* params, float* T, lisreg_stats* stats);

/* Asynchronous form for device-resident batches (all items LISREG_FMT_DEVICE): enqueue on the context's
 * stream with poses/stats left on the device; lisreg_batch_fetch synchronises and copies them out.
 * `prepare` does all per-batch allocation and the item-table upload (one pinned staging buffer, asynchronous copies);
 * `run` only launches kernels — optional index rebuild, then `bound` x {correspondence kernel, solve kernel}, finalize:
 * eager launches, no host synchronisation, registrations that have converged make their workgroups exit at once — so
 * it can be timed with events on lisreg_get_stream().  T_init is copied at prepare time and re-applied on the device at
 * the start of every run.  (The synchronous entry points lisreg_align / lisreg_align_batch additionally read a 4-byte
 * finished-counter every few iterations and stop launching once every item is done.)
 * Life time of a target's search structures: the grid index of a target slot is built by lisreg_set_target* and stays valid until that
 * slot is set again; its k-NN graph (front-end 3) is built on first use — at lisreg_set_target when "search_mode" is 3, else at the first
 * lisreg_batch_prepare whose auto choice falls on the graph — and is then REUSED by every later prepare / run against that slot: a node
 * that registers many batches against one submap pays for index and graph once.  Only with "rebuild_targets_each_run" = 1 (bench.py: the
 * reference rebuilds both kd-trees inside every scan2SubMapOptimization, :602-603) does every lisreg_batch_run rebuild the indexes, and
 * the graphs with them, of all targets of the prepared batch. */
int  lisreg_batch_prepare(lisreg_ctx* ctx, int n_items, const lisreg_item* items,
                          const lisreg_params* params, const float* T_init);
int  lisreg_batch_run(lisreg_ctx* ctx);
int  lisreg_batch_fetch(lisreg_ctx* ctx, float* T, lisreg_stats* stats);
/* Host feeder for streams of batches (lisreg_api_feed.hip).  Packs the HOST clouds of `items` (the reference's PCL structs) to 16-byte
 * device records with "feeder_threads" host threads (option, default 8) into pinned staging and uploads them asynchronously, on a copy
 * stream of the context, into one of two device buffers the context owns; items_out[i] is items[i] with device pointers and
 * LISREG_FMT_DEVICE.  The caller's clouds are not referenced after the call returns.  The next lisreg_batch_prepare waits for the
 * uploads ON THE DEVICE.  Buffers alternate between calls, so the loop
 *     stage(k+1); fetch(k); prepare(k+1); run(k+1);          (or: prepare(k); run(k); stage(k+1); fetch(k); ...)
 * uploads batch k+1 underneath the kernels of batch k — the reference has no counterpart (its clouds never leave the host);
 * lisreg_align_batch uses it internally for batches of >= 262144 source points. */
int  lisreg_stage_host_items(lisreg_ctx* ctx, int n_items, const lisreg_item* items, lisreg_item* items_out);

/* Device pointer to the prepared batch's result block: n_items x 12 floats
 * {T[6], iters, deltaR, deltaT, degenerate, n_corr_last, status} — what a multi-GPU host all-gathers. */
void* lisreg_batch_result_device(const lisreg_ctx* ctx);

/* Options outside the reference's parameter surface: "rebuild_targets_each_run" (0/1: re-run the target index
 * build inside every lisreg_batch_run, as the reference rebuilds both kd-trees per registration, :602-603),
 * "trace_cap" (per-item trace records kept on the device for batches; 0 = off), "search_mode" (the exact 5-NN front-end
 * that stands in for pcl::KdTreeFLANN::nearestKSearch: 1 per-lane grid walk,
 * 3 k-NN graph scan with the walk as its fall-back — costs 1 KB of device memory per target point for the
 * neighbour rows —, 5 cell rows: the same certified list scan, but the list belongs to the grid cell (or the octant of it) the query
 * falls into instead of to last iteration's nearest neighbour, so nothing is carried between Gauss-Newton iterations and the first
 * iterations of a batch — queries a pose error away from every surface — cost the same scan as the last ones; ~3-5 KB of device memory
 * per target point, built in ~3 ns per target point —, 4 auto [default]: 5 when the prepared batch asks at least "cell_min_ratio"
 * [default 170] query-iterations per target point and its targets' rows fit "cell_rows_max_mb" [default 16384], else 3 from
 * "graph_min_ratio" [default 60] query-iterations per target point on, else 1 — all return the same neighbours; the one exception is two candidates at exactly equal float distance from a query
 * competing for the fifth place: the first one met wins, and the front-ends meet them in different orders),
 * "sort_sources" (0 caller order, 1 column sort, 2 auto [default]: probe the order when a batch is prepared — one pass over the sources
 * and a 4-byte read-back, skipped for batches of the same shape (items, points) as the one last probed, whose verdict is reused; every 32nd
 * such batch is probed again; the search is exact on any order — the same neighbours —, but a sorted batch sums the rows of its
 * workgroups in another order, so its poses may differ from the unsorted ones in the last bits),
 * "index_build" (how "rebuild_targets_each_run" rebuilds the target grids of a batch: 0 bucket sort with one global atomic per
 * point, 1 strip form — LDS histograms, one workgroup per strip of cells; an error if a grid does not fit its LDS tables —,
 * 2 [default] strip form whenever the grids fit; both produce the same index bit for bit), "index_strip_cells" (cells per strip aimed at; 0 [default]: 1024 for a batch of one or two
 * targets, 2048 beyond — a shared submap is a handful of strips and wants them smaller), "index_strip_cap",
 * "xcd_order" (dispatch order of the correspondence workgroups of a graph-front-end batch: 0 block order, 1 by target sector so that
 * each of the 8 XCDs — each with its own L2 — works on one eighth of the target, 2 auto [default]: 1 for batches of >= 32 registrations;
 * results do not depend on it, bit for bit),
 * "exact_arithmetic" (0 [default] the production arithmetic of the correspondence kernel: FMA contraction, 1-ulp hardware reciprocal /
 * square root in the line and plane fits, fp32 sums inside a wavefront — poses within 1e-3 of the reference, a handful of
 * threshold-straddling correspondences per thousand may differ; 1 the reference's arithmetic operation for operation — IEEE division
 * and sqrt, cv::eigen's pivoted Jacobi, fp64 sums, no contraction, the pose's sines / cosines from the host's libm (one small
 * synchronous round trip per iteration: a run of this build blocks the caller and cannot be stream-captured): accept flags,
 * correspondence counts, iteration counts and — bit for bit on the 100-configuration sweep — poses EQUAL the CPU restatement's
 * (tests/test_exact.py, tests/exact_sweep.py), at roughly 0.5x the throughput),
 * "canonical_ties" (0 [default]: of two target points at EXACTLY equal float distance from a query the first one met is kept, and
 * the search front-ends meet them in different orders — about one query in 10^5-10^6 on scan data, like FLANN's own traversal order;
 * 1: such ties are noted during the search and resolved by (distance, original index), so the five neighbours, their order and every
 * bit computed from them are the same in every front-end and batch shape — a frame registers identically alone and inside any batch —
 * at +7 % per correspondence launch; implied by "exact_arithmetic"),
 * "cell_anchor_until" (graph front-end: during GN iterations 1 .. this [default 1] a query also tries an anchor out of its own grid column
 * and takes the nearer of the two — the pose moves by decimetres in the first step, last iteration's nearest neighbour is a poor start;
 * results do not depend on it),
 * "feeder_threads" (host threads of lisreg_stage_host_items, default 8; 0 = structs uploaded as they are and packed on the device),
 * "feeder_numa" (1 [default]: the packing threads are bound to those CPUs of the device's NUMA node that the process may run on — the
 * pinned staging buffers are on that node already; read-only "feeder_numa_node" / "feeder_numa_cpus" say what was found),
 * "feeder_copy_engine" (1 [default]: while the next packed chunk is not ready and the copy engine is idle, the engine takes the last free
 * chunk of a pinned cloud as it is and a kernel packs it on the device; 0: never; 2: whenever a packed chunk is not ready — for tests;
 * 3: the engine takes the FIRST chunk whatever the packing threads do — for tests),
 * "interleave" (0 [default]: one launch per Gauss-Newton iteration for the whole batch; 1 / 2: a fixed-iteration run of at least
 * "interleave_min_blocks" [8192] workgroups is cut at an item boundary near its middle and the halves iterate on two streams, so that each
 * half's 6x6 solves run underneath the other half's correspondence launch — 1: the halves' launches alternate, 2: free-running; same
 * kernels on the same data in the same order per registration, results identical to the bit; measured +1.7 % (mode 2) on
 * BASELINE configs[1], +5.8 % on configs[4], at the price of per-kernel durations that are no longer a launch's own — off),
 * "row_reach" (1: a batch that takes the cell rows and rebuilds its targets inside every run ("rebuild_targets_each_run") builds
 * rows only for the grid cells its queries come within a metre of under their INITIAL poses — lisreg_batch_prepare makes one pass over
 * the batch's source points for that —; a query that reaches a cell without rows takes the cell walk, so results do not depend on it,
 * bit for bit.  2 [default]: of those cells, only the ones a query starts in and the ones within half a metre of a target point (a
 * target point in the cell's 3 x 3 x 3 block; grids with cells under 0.5 m, where half a metre is two cells, keep the rows of 1): a
 * query moves from where its initial pose puts it towards the target's surface, not a metre in every direction.  A run counts the
 * queries that find their cell without rows; more than one query-iteration in a thousand and the prepared batch's later runs, and the
 * next 32 batches prepared on the context, build all rows.  0: all rows always; other values are refused with LISREG_ERR_ARG),
 * "graph_min_ratio", "cell_min_ratio" (auto takes the cell rows from this many query-iterations per target point: 110), "cell_rows_max_mb",
 * "first_pass_mm" (radius of the cell walk's first pass, >= 0: a negative value is refused with LISREG_ERR_ARG), "count_searches",
 * "early_stop_chunk" (<= -1 auto, 0 never look).  Out-of-range values of the numeric knobs are clamped, not refused: "index_strip_cells"
 * below 0 is 0 (auto), "index_strip_cap" is kept in [64, 16384], "interleave_min_blocks" below 2 is 2, "cell_anchor_until" and
 * "trace_cap" below 0 are 0; "xcd_order", "interleave", "index_build" and "search_mode" (0, 2, 6, ...) refuse values they do not name.
 * Which options may change results, and which must not, is pinned by tests/test_option_state.py. */
int  lisreg_set_option(lisreg_ctx* ctx, const char* name, int value);
/* Read back an option, or "front_end" = the search front-end the prepared batch actually runs (auto resolved), or
 * "index_build_now" = 1 if the prepared batch rebuilds its targets in strip form, "xcd_order_now" = 1 if the last run used the
 * sector dispatch order, "interleaved_now" = 1 if it ran as two halves; size of the prepared batch's search index: "index_kib_grid"
 * (sorted records + cell tables of its targets), "index_kib_front_end" (k-NN graph rows or cell rows + their tables; 0 for the cell
 * walk), "index_target_points" (points in those targets) — bench.py's roofline.index_bytes_per_target_point —, "index_kib_front_end_built" (the
 * cell rows the last run really built, read back from the device: synchronous); "row_reach_now" = 1 if the last
 * run built its cell rows for the cells the query marks reach only, "row_reach_misses" = query-iterations of the last FETCHED run that
 * found their cell without rows. */
int  lisreg_get_option(const lisreg_ctx* ctx, const char* name, int* value);

/* Diagnostics of the motion certificate (enable with option "count_searches" = 1; accumulates until re-enabled):
 * out[2*k] = queries re-searched at GN iteration k, out[2*k+1] = queries processed at iteration k (k < 32).
 * Graph front-end, n > 64: out[64+k] = (wavefronts with a walking lane) << 32 | wavefronts, of iteration k. */
int  lisreg_get_counters(lisreg_ctx* ctx, unsigned long long* out, int n);

/* Test hook (option "dump_neighbors" = 1 before the batch is prepared; search modes 1 and 3): the five neighbours the LAST
 * executed GN iteration used for every source point, as ORIGINAL indices into the target cloud of the point's kind, nearest
 * first, -1 where fewer than five lie inside sqrt(knn_sq_thresh) — i.e. what nearestKSearch(5) + the `sqDist[4] < tau` test
 * of :657 / :776 select; row 5 = 1 where the point passed every accept test and contributed a row to the normal equations
 * (laserCloudOriFlag, :741 / :820).  out: host int[6][n_elems], n_elems = all source points of the batch in item order (corner
 * then surf of each item). */
int  lisreg_get_neighbors(lisreg_ctx* ctx, int* out, int n_elems);

/* Test hook, read-only (host code: no kernel, and no buffer of the production path is sized, cleared or kept for it): what the LAST
 * executed GN iteration of the prepared batch left of the normal equations, one partial row per workgroup.  Call after
 * lisreg_batch_run / lisreg_batch_fetch; available, like lisreg_get_neighbors, only if option "dump_neighbors" was 1 when the batch was
 * prepared.  Synchronises the context's stream.  The rows are still there because only the next correspondence launch writes them: the
 * solve reads them, and the finalize (also the one folded into the last solve of a fixed-iteration run) resets the registrations only.
 *   *n_blocks                 workgroups of the row reduction (call with NULL buffers to learn it)
 *   blocks[n_blocks][4]       item, kind (0 corner / 1 surf), the block's first query as a batch position (positions as for
 *                             lisreg_get_neighbors; a batch that sorts its sources orders the positions inside a segment), count
 *                             (<= 256) — the descriptors the row reduction ran with
 *   rows[n_blocks][28]        21 upper-triangle AtA terms (row-major), 6 AtB, the correspondence count, summed over the block's
 *                             queries.  UNSPECIFIED for the blocks of a registration that was through when the launch started (the
 *                             feature-count guard): the kernels return before they write those rows.
 *   capacity_blocks           blocks the two arrays above hold (>= n_blocks if either is given)
 *   coef[n_elems][4], coef_ok[n_elems]   only for a batch that runs eight lanes per query ("lanes_per_query" reads 8): the coefficients
 *                             (coeff.x, y, z, intensity) and the accept flag the search kernel handed to the row reduction, per batch
 *                             position; LISREG_ERR_ARG if asked of a one-lane batch or with another n_elems than the batch's source
 *                             point count.  UNSPECIFIED for the queries of a segment whose target has fewer than five points: the
 *                             search kernel returns before it writes them (the rows of such a segment's blocks are zero).
 * Any of blocks / rows / coef / coef_ok may be NULL and is skipped.  A refused call leaves every output untouched. */
int  lisreg_get_partial_rows(lisreg_ctx* ctx, int* n_blocks, int* blocks, double* rows, int capacity_blocks, float* coef,
                             int* coef_ok, int n_elems);

/* Test hook: the DEVICE functions of the two residual models, one case per thread, on caller-given neighbourhoods — what the
 * correspondence kernel computes for a query once its five neighbours are known.  kind 1 = surfOptimization's body
 * (odomEstimationNode.cpp:776-821: plane through the five neighbours, |n.p + d| <= plane_tol test, point-to-plane residual, robust
 * weight, accept test; in the production arithmetic the plane comes from the closed form `plane5_closed` with its hand-over to the
 * column-pivoted QR), kind 0 = cornerOptimization's (:664-739).  neighbours: host float[n][5][3] (nearest first), queries: host
 * float[n][3] (the TRANSFORMED query point), label weight 1.  exact != 0 runs the exact-arithmetic build of the same source.
 * out: host float[n][10]: kind 1: pa, pb, pc, pd (NaN = plane rejected), 1 if the closed form produced it / 0 if the QR did,
 * coeff x, y, z, intensity (:808-811), 1 if accepted (s > accept_s, :813); kind 0: centroid x, y, z and two components of the line
 * direction (NaN = lambda-ratio test failed), coeff x, y, z, intensity (:729-732), accepted (:734); kind 2: cornerOptimization's
 * eigen-solver alone: the two largest eigenvalues of the scatter matrix, the line direction x, y, z, 1 if the closed form was
 * certified / 0 if the Jacobi ran (always 0 in the exact build), 1 if the lambda-ratio test passed, 0, 0, accepted. */
int  lisreg_test_fit_models(lisreg_ctx* ctx, int kind, int n, const float* neighbours, const float* queries,
                            const lisreg_params* params, int exact, float* out);

/* Test hook: the production Gauss-Newton step kernels (the fixed-order fp64 row sum, cv::solve, the iteration-0 degeneracy analysis,
 * the projection, the convergence test; then transformUpdate) on caller-given normal equations — n_items independent registrations
 * of one workgroup each, in buffers of the call's own (a prepared batch of the context is untouched): the registrations are reset, the
 * solve kernel runs n_steps (1 .. 64) times, then the finalize kernel, all on the context's stream; returns with the outputs complete.
 *   n_rows[n_items]          partial rows of every item; the items' rows lie back to back in item order (R = their sum)
 *   rows[n_steps][R][28]     per step, the 28 doubles of every row: 21 upper-triangle AtA (row-major), 6 AtB, 1 count
 *   T_init[n_items][6], degenerate_in[n_items] (NULL: 0), n_sc / n_ss[n_items] (source sizes for the feature-count guard; NULL:
 *   the guard passes), imu[n_items] (NULL: none available), params as for lisreg_batch_prepare
 *   trace_out[n_items][n_steps][LISREG_TRACE_STRIDE]   the trace records (zeros where an item was finished already)
 *   state_out[n_items][n_steps][LISREG_SOLVE_STATE_STRIDE]   (indexed like trace_out) the registration in device memory after that step:
 *       [0..35] matP  [36..47] the 3 x 4 pose matrix of the next correspondence launch  [48] isDegenerate  [49] deltaR  [50] deltaT
 *       [51] n_corr  [52] 1 if finished  [53] iterCount to report  [54] 1 if any step solved  [55] steps started
 *   results_out[n_items][12] the result block after finalize: T[6], iters, deltaR, deltaT, degenerate, n_corr_last, status
 * Any output may be NULL. */
#define LISREG_SOLVE_STATE_STRIDE 56
int  lisreg_test_solve_steps(lisreg_ctx* ctx, int n_items, int n_steps, const int* n_rows, const double* rows,
                             const float* T_init, const int* degenerate_in, const int* n_sc, const int* n_ss,
                             const lisreg_imu* imu, const lisreg_params* params,
                             float* trace_out, float* state_out, float* results_out);

/* Diagnostics (tests): the grid of the map index of `slot` (lisreg_map_index_set): dims = {n, nx, ny, nz, n_cells}, geom = {ox, oy, oz,
 * cell edge} — an empty map has nx = ny = nz = 0 and one cell.  Either output may be NULL. */
int  lisreg_get_map_grid(lisreg_ctx* ctx, int slot, int* dims, float* geom);

/* Test hook: ONE chosen form of the exact k = 1 search (lisreg_nn1.hip) per query, on the map index of `slot` (lisreg_map_index_set):
 * form 1, 4, 8 = the column walk nn1_search<Q> with that many lanes per query (what lisreg_nearest, the dynamic filter, ICP-GN and small
 * ICP batches run), form 0 = the flattened one-lane walk nn1_search_flat of large ICP batches — the device functions production calls.
 * All forms must return the same point: the lexicographic minimum of (squared distance, original index) within max_dist.
 *   queries[n][3]   host, x y z
 *   seeds[n]        host, or NULL for none: the "probably near" point the ICP kernels hand the search, which must never change the result.
 *                   >= 0: an ORIGINAL index into the map cloud (translated here to the position in the cell-sorted array the search takes);
 *                   -1: no seed; -2: nn1_cell_seed(query), the seed of ICP's first iteration; a value >= the map's size is passed on as
 *                   it is (the search must ignore it)
 *   idx_out[n]      host: ORIGINAL index of the nearest map point, -1 none;  sqd_out[n]: the search's squared distance (as lisreg_nearest)
 * Runs on the context's stream in buffers of the call's own and returns with the outputs complete.  n = 0: OK, nothing touched. */
int  lisreg_test_nn1(lisreg_ctx* ctx, int slot, const float* queries, int n, float max_dist, int form, const int* seeds,
                     int* idx_out, float* sqd_out);

/* Test hook: the exclusive scan under every bucket sort, compaction and cell-row build (lisreg_index.hip), dispatched exactly as production
 * dispatches it — no forced form, the thresholds as they stand: n <= 16 384 one workgroup (k_scan_small), up to 4 096 tiles of 2 048 the
 * fused two-launch form, beyond that three launches.
 *   in1 == NULL   single form: out0[n0 + 1] = exclusive scan of in0[n0], out0[n0] = the total.  n0 = 0 is valid: out0[0] = 0.
 *   in1 != NULL   pair form: the two scans of a slot's corner and surf row counts in one launch pair (the tiled kernels at any size, one
 *                 tile included; either half beyond 4 096 tiles sends both through the single form).  A half with n = 0 is off, as in
 *                 production: its output is neither written nor returned (its pointers may be anything).
 *   in_offset, out_offset   0 to 3, in ints, added to 16-byte aligned device allocations: the tiled kernels move full tiles as int4 only
 *                 when both pointers are aligned, so (0, 0) takes the vector path and anything else the scalar path (the feature
 *                 extractor scans into such an address on purpose).  k_scan_small has one path.
 *   in_place      != 0: out = in (the offsets must be equal).  Every form reads a thread's items before it writes them, so all three
 *                 support it.
 * Inputs and outputs are host arrays; the device buffers are the call's own, the scratch of each half is n / 2048 + 4 ints (the smallest
 * a production call site allocates).  16 guard words behind out[n], the words in front of a shifted out and 16 behind the scratch are
 * checked after the run: LISREG_ERR_HIP with a text that names the word if one changed.  Runs on the context's stream and returns with
 * the outputs complete.  LISREG_ERR_ARG: a NULL pointer of a half that runs, a negative size, n1 > 0 without in1, an offset outside
 * 0 to 3, in_place with differing offsets. */
int  lisreg_test_scan(lisreg_ctx* ctx, const int* in0, int n0, const int* in1, int n1, int in_offset, int out_offset, int in_place,
                      int* out0, int* out1);

/* Diagnostics (tests): the search index of target `slot`, kind 0 = corner / 1 = surf, as it stands in HBM after the work queued on
 * the context's stream: dims = {n, nx, ny, nz, n_cells}, geom = {ox, oy, oz, cell edge}, the cell-sorted records
 * (x, y, z, bit-cast original index; ordered by cell (ix * ny + iy) * nz + iz, then original index) and cell_start[n_cells + 1].
 * Any output pointer may be NULL. */
int  lisreg_get_target_index(lisreg_ctx* ctx, int slot, int kind, int* dims, float* geom,
                             float* sorted_out, int sorted_capacity, int* cell_start_out, int cell_capacity);

/* Diagnostics: the k-NN graph of a target's search index (search front-end 3; built now if it was not yet).  *k = entries per
 * row; rows_out[p * k + j] = (x, y, z, sorted position as int bits) of the j-th nearest other point of sorted point p, ascending
 * by distance (to 2^-16 relative: the build sorts quantised keys, the scan's stop test carries a millimetre of slack for it), padded with (p's own coordinates, -1); meta_out[p] = (rho^2, count as int bits): every point closer to p than rho
 * is in its row.  Either output may be NULL.  capacity_points >= the target's point count. */
int  lisreg_get_target_graph(lisreg_ctx* ctx, int slot, int kind, int* k, float* rows_out, float* meta_out, int capacity_points);

/* Diagnostics: the cell rows of a target's search index (search front-end 5; built now if they were not yet).  *n_rows = rows in all,
 * *k = entries per row.  table_out[cell] (the index's n_cells entries, cell = (ix * ny + iy) * nz + iz): -2 = no target point within two
 * cells of this one, -1 = no row, else (first row << 8) | octant mask — the cell's rows are [the row at its centre, then one row per
 * octant of the mask in ascending octant order, octant = (x upper half) + 2 (y upper half) + 4 (z upper half)]; rows_out[r * k + j] =
 * (x, y, z, sorted position as int bits) of the j-th nearest target point of the row's centre, ascending (to 2^-16 relative), padded with
 * (the centre's coordinates, -1); meta_out[r] = (rho^2, count as int bits): every point closer to the centre than rho is in the row.
 * Outputs may be NULL; capacity_rows >= *n_rows when rows_out / meta_out are given (call once with NULLs to learn it).  Building the rows
 * re-makes the target's grid two cells wider than the cloud on every side (once per target): read lisreg_get_target_index after this.
 * When that happens a batch prepared on this context (lisreg_batch_prepare) is no longer valid — its copy of the grid geometry is stale —
 * and lisreg_batch_run refuses it (LISREG_ERR_ARG, "no prepared batch") until it is prepared again. */
int  lisreg_get_target_cell_rows(lisreg_ctx* ctx, int slot, int kind, int* n_rows, int* k, int* table_out, int capacity_cells,
                                 float* rows_out, float* meta_out, int capacity_rows);

/* Trace of the LAST lisreg_align call: copies min(n_iters_run, max_iters) records; returns the count. */
int  lisreg_get_trace(lisreg_ctx* ctx, float* buf, int max_iters);

/* Per-kernel timing of the last align/batch_run when enabled (HIP events on the context's stream):
 * out[0] = total ms in the correspondence+normal-equation kernel, out[1] = its launch count,
 * out[2] = total ms in the solve/update kernel, out[3] = its launch count, out[4] = index build ms.
 * After a lisreg_vgicp_* call: out[0] / out[1] = the linearisations and their number, out[2] = the voxel sort and statistics,
 * out[4] = the distributions (search grid, k-nearest search, covariances); after lisreg_vgicp_align_batch out[0] / out[1] = the
 * rounds' linearisation and total launches (one interval per round) and their number, out[2] / out[3] = the fitness search, out[4] =
 * the distributions of every staged source.  After a lisreg_fgicp_* call: out[0] / out[1] = the sum
 * launches and their number, out[2] / out[3] = the search launches and their number, out[4] = the distributions.  After
 * lisreg_ndt_align_batch: out[0] / out[1] = the rounds' evaluation and total launches (one interval per round) and their number,
 * out[2] / out[3] = the fitness search.  After a lisreg_gicp_* call: out[2] / out[3] = the search-and-moments launches and their
 * number, out[0] / out[1] = their fixed-order totals, out[4] = the distributions; after lisreg_gicp_align_batch the same per round
 * (one moments interval and one totals interval per round), plus the fitness search in out[2] / out[3] and its totals in out[0] /
 * out[1], and out[4] = the distributions of every staged source. */
int  lisreg_set_profiling(lisreg_ctx* ctx, int enable);
int  lisreg_get_timing(lisreg_ctx* ctx, double out[5]);

/* ---- the step before the registration --------------------------------------------------- */
/* Replaces pcl::VoxelGrid<PointT>::filter with the reference's default settings — downSizeFilterCorner/Surf on the
 * incoming feature clouds (odomEstimationNode.cpp:272-277) and on the assembled local map (:196-201), and
 * voxel_downsample_pcl on submap class clouds (src/include/subMap.h:1207-1249): one centroid per occupied voxel of
 * edge `leaf` (xyz and intensity averaged, label = most frequent), output in ascending PCL voxel index.
 * in/out: LISREG_FMT_XYZI / _XYZIL host clouds (out has the input's stride), or LISREG_FMT_DEVICE (in and out are device
 * lisreg_dpoint arrays; payload label majority-voted) so the result can feed lisreg_align / lisreg_set_target directly.
 * *n_out receives the voxel count; if it exceeds out_capacity nothing is written and LISREG_ERR_ARG is returned.
 * Returns LISREG_LEAF_TOO_SMALL (and copies the input, as PCL does) when the voxel index would overflow int32. */
int  lisreg_voxel_downsample(lisreg_ctx* ctx, const void* in, int n, int stride_bytes, int fmt, float leaf,
                             void* out, int out_capacity, int* n_out);
/* The same for K clouds of device records (LISREG_FMT_DEVICE: label vote, or LISREG_FMT_DEVICE_XYZI: intensity average) in ONE launch
 * sequence with three host round trips in all (the K bounding boxes, the K counts, completion) — the five class grids of a key frame or of the local
 * map are bound by their ~12 launches and 3 round trips apiece, not by bandwidth.  Results equal K single calls bit for bit; clouds
 * that do not fit the joint sort (a leaf too small for its cloud, > 8 clouds) are done one by one. */
int  lisreg_voxel_downsample_multi(lisreg_ctx* ctx, int k, const void* const* in, const int* n, const float* leaf, int fmt,
                                   void* const* out, const int* out_capacity, int* n_out);
/* The same for up to LISREG_VOXEL_BATCH_MAX clouds of device records — the corner and surface clouds of a whole sweep batch
 * (currentCloudInit, odomEstimationNode.cpp:260-281) or the class clouds of many key frames — in one launch sequence whose length does
 * not depend on n_clouds, with ONE host synchronisation (the n_out / status table).  fmt: LISREG_FMT_DEVICE (label vote) or
 * LISREG_FMT_DEVICE_XYZI (.w averaged), one per call.  Per job, out[0 .. n_out), n_out and status are byte for byte those of
 * lisreg_voxel_downsample(ctx, in, n, 16, fmt, leaf, out, out_capacity, &n_out) on that cloud alone (clouds without NaN coordinates):
 * LISREG_OK; LISREG_LEAF_TOO_SMALL with a copy of the input (needs out_capacity >= n); LISREG_ERR_ARG with n_out = the count needed
 * and nothing written when the voxels exceed out_capacity; LISREG_ERR_ARG with n_out = 0 and nothing written for a cloud with an
 * infinite coordinate.  A job's failure leaves the other jobs alone, and the call returns LISREG_OK when the batch ran.
 * Refused with LISREG_ERR_ARG before anything is launched (lisreg_last_error names the job): a NULL pointer, n < 0, a leaf that is not
 * > 0, n_clouds outside 0 .. LISREG_VOXEL_BATCH_MAX, a bad fmt, more than 2e9 points in all, an `out` range (out_capacity records) that
 * overlaps any job's `in` range or another job's `out` range — the batch form does no in-place grids.  Outputs are complete on return. */
#define LISREG_VOXEL_BATCH_MAX 1024
typedef struct lisreg_voxel_job {
    const void* in;  int n;          /* device lisreg_dpoint records */
    float       leaf;
    void*       out; int out_capacity;
    int         n_out;               /* written back: voxels of this cloud (the count needed, when the capacity is too small) */
    int         status;              /* written back: LISREG_OK, LISREG_LEAF_TOO_SMALL or LISREG_ERR_ARG */
} lisreg_voxel_job;
int  lisreg_voxel_downsample_batch(lisreg_ctx* ctx, int n_clouds, lisreg_voxel_job* jobs, int fmt);
/* Replaces transformPointCloud(cloud, &pose6D) (src/core/common.cpp:112-173 and the PointXYZIL overload; callers
 * odomEstimationNode.cpp:457-458, 574-575): p' = R(T) p + t with T = {roll,pitch,yaw,x,y,z}; other fields copied.
 * Same formats as above; in == out is allowed. */
int  lisreg_transform_cloud(lisreg_ctx* ctx, const void* in, int n, int stride_bytes, int fmt, const float T[6], void* out);

/* ---- producer of cloud_info: range-image projection + LOAM feature extraction ----------------- */
/* Host point layout of the raw scan: PointXYZIRT (src/include/common.h:12-23): x@0 y@4 z@8 intensity@16 uint16 ring@20
 * float time@24, 32-byte stride.  Device layout: lisreg_dpoint with the ring in the low 16 bits of the payload. */
#define LISREG_FMT_XYZIRT  3
typedef struct lisreg_feature_params {
    int   n_scan;             /* N_SCAN        (config/params.yaml:68 = 64)   */
    int   horizon_scan;       /* Horizon_SCAN  (config/params.yaml:69 = 1800) */
    int   downsample_rate;    /* downsampleRate(config/params.yaml:72 = 2): rows with ring % rate != 0 are dropped */
    float min_range;          /* lidarMinRange (config/params.yaml:73 = 0.0)  */
    float max_range;          /* lidarMaxRange (config/params.yaml:74 = 70.0) */
    float edge_threshold;     /* edgeThreshold (config/params.yaml:117 = 1.0) */
    float surf_threshold;     /* surfThreshold (config/params.yaml:118 = 0.1) */
} lisreg_feature_params;
/* The five clouds of cloud_info (msg/cloud_info.msg:20-25).  Buffers are caller-allocated in the INPUT's layout with the
 * stated capacities (points); counts are written back.  n_scan*horizon_scan is always enough for each. */
typedef struct lisreg_feature_out {
    void* deskewed;      int cap_deskewed,      n_deskewed;       /* extractedCloud    -> cloud_deskewed        */
    void* corner;        int cap_corner,        n_corner;         /* cornerCloud       -> cloud_corner          */
    void* surface;       int cap_surface,       n_surface;        /* surfaceCloud      -> cloud_surface         */
    void* corner_sharp;  int cap_corner_sharp,  n_corner_sharp;   /* sharpCornerCloud  -> cloud_corner_sharp    */
    void* surface_sharp; int cap_surface_sharp, n_surface_sharp;  /* SharpSurfaceCloud -> cloud_surface_sharp   */
} lisreg_feature_out;
/* Replaces LaserProcessing::projectPointCloud, cloudExtraction, calculateSmoothness, markOccludedPoints and
 * extractFeatures (src/core/laserProcessing.cpp:467-510, 515-539, 544-563, 568-605, 610-713) for one scan, without the
 * IMU de-skew (deskewPoint returns the point unchanged when no IMU data is available, :429; lisreg_extract_features_deskew
 * below applies it).  Output order is the
 * reference's: rings ascending, six sectors per ring, corners in pick order (largest curvature first). */
int  lisreg_extract_features(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt,
                             const lisreg_feature_params* params, lisreg_feature_out* out);
int  lisreg_default_feature_params(lisreg_feature_params* p);
/* The IMU de-skew inside projectPointCloud (deskewPoint / findRotation, laserProcessing.cpp:368-399, 427-462, called at :501):
 * every point that wins a range-image pixel is rotated into the frame of the first such point, with the rotation integrated from
 * the IMU (imuDeskewInfo, :222-266 — a ~50-term prefix sum that stays on the host) interpolated at the point's time stamp.
 * findPosition returns zeros in the reference (:405-421), so there is no positional part.  Ranges, columns and the feature
 * selection use the raw points, hence only the coordinates of the five output clouds change. */
typedef struct lisreg_deskew {
    int    enabled;               /* deskewFlag == 1 && cloudInfo.imuAvailable (:429) */
    int    imu_pointer_cur;       /* last valid index of the tables (imuPointerCur after :261) */
    const double* imu_time;       /* host arrays [imu_pointer_cur + 1] */
    const double* imu_rot_x;
    const double* imu_rot_y;
    const double* imu_rot_z;
    double time_scan_cur;         /* timeScanCur; a point's time = time_scan_cur + its `time` field */
    const float* time_device;     /* LISREG_FMT_DEVICE only: per-point `time` (device array [n]); host structs carry it at offset 24 */
} lisreg_deskew;
/* lisreg_extract_features with the de-skew applied to the output coordinates; deskew == NULL or enabled == 0 is the plain call */
int  lisreg_extract_features_deskew(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt,
                                    const lisreg_feature_params* params, const lisreg_deskew* deskew, lisreg_feature_out* out);

/* lisreg_extract_features for n_sweeps sweeps at once — the throughput form: the sweeps are stacked into one range image (the
 * selection kernel's grid is sweeps x rings) and every pass of the pipeline runs once.  sweeps[s] / n[s]: DEVICE lisreg_dpoint
 * records (ring in the low 16 bits of the payload); outs[s]: device buffers as in lisreg_extract_features.  No IMU de-skew.
 * The five clouds of every sweep are identical to what a single call on that sweep returns.  At most 256 sweeps and
 * n_sweeps x n_scan <= 32768 per call. */
int  lisreg_extract_features_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                                   const lisreg_feature_params* params, lisreg_feature_out* outs);
/* lisreg_extract_features_batch with the IMU de-skew of lisreg_extract_features_deskew (deskewPoint / findRotation,
 * laserProcessing.cpp:368-399, 427-462, called at :501) applied per sweep: deskews[s] is that sweep's own lisreg_deskew — its own host
 * tables of any length the single call accepts, its own time_scan_cur and its own time_device (required when enabled;
 * lisreg_pretreat_batch's time_device output goes in directly).  The five clouds of every sweep are byte for byte what
 * lisreg_extract_features_deskew gives for that sweep alone; a sweep with enabled == 0, and every sweep when deskews == NULL, gets
 * lisreg_extract_features_batch's bytes, and a call without an enabled sweep issues exactly that call's launches.  The de-skew adds
 * one table upload and three launches, whatever n_sweeps is.  Every argument is checked before the first launch (the single call's
 * rules per sweep): on LISREG_ERR_ARG for an argument no output buffer has been written. */
int  lisreg_extract_features_deskew_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                                          const lisreg_feature_params* params, const lisreg_deskew* deskews /* [n_sweeps] or NULL */,
                                          lisreg_feature_out* outs);

/* ---- laser pretreatment: ring and per-point time of a raw sweep ------------------------------------------------- */
/* Replaces LaserPretreatment::Pretreatment (src/core/laserPretreatment.cpp:4-81, :84-161; inline in src/node/laserPretreatmentNode.cpp:
 * 60-219; removeClosedPointCloud, src/include/laserPretreatment.h:25-54): non-finite and out-of-range points are dropped, the ring comes
 * from the elevation angle through the beam table of N_SCAN 16 / 32 / 64 (points outside the table are dropped), the time from the
 * azimuth with the halfPassed seam logic; input order is kept and x, y, z, intensity are copied bit for bit.  The arithmetic is the
 * reference's, operation for operation (float / double steps listed at the top of lis-slam_amd/csrc/lisreg_pretreat.hip; a float libm
 * function is the correctly rounded value, as for lisreg_extract_features).  Its outputs are what lisreg_extract_features* (ring) and
 * lisreg_deskew.time_device (time) take. */
#define LISREG_FMT_XYZI_PACKED 5   /* host: floats x@0 y@4 z@8 intensity@12, 16-byte stride (KITTI velodyne .bin files, PointCloud2 point_step 16) */
typedef struct lisreg_pretreat_params {
    int    n_scan;        /* N_SCAN: 16, 32 or 64 — anything else LISREG_ERR_ARG (the reference: ROS_BREAK)      */
    float  min_range;     /* lidarMinRange (config/params.yaml:73)                                               */
    float  max_range;     /* lidarMaxRange (:74)                                                                 */
    double scan_period;   /* scanPeriod = 0.1, a double constant (laserPretreatment.h:12)                        */
} lisreg_pretreat_params;
typedef struct lisreg_pretreat_out {
    void*  cloud;         /* host input: PointXYZIRT structs (32 B: x y z, intensity@16, uint16 ring@20, float time@24);
                             device input: lisreg_dpoint, ring in the low 16 bits of the payload                   */
    int    capacity;      /* points; n (input count) is always enough                                             */
    int    n;             /* written back: points kept                                                            */
    float* time_device;   /* device input only: per-point time [capacity] — what lisreg_deskew.time_device takes  */
    float* intensity_device; /* device input only, may be NULL: per-point intensity [capacity]                    */
    float  start_ori, end_ori;   /* written back: the sweep's startOri / endOri after the 2 pi adjustment (0 when no point is finite and in range) */
    int    half_index;    /* written back: output index of the point at which halfPassed became true, -1 if never */
} lisreg_pretreat_out;
int  lisreg_default_pretreat_params(lisreg_pretreat_params* p);          /* 64, 0.0, 70.0, 0.1 */
/* One sweep.  fmt: LISREG_FMT_XYZI (PCL PointXYZI / the reference's PointIn: intensity at byte 16) or LISREG_FMT_XYZI_PACKED — host in,
 * host PointXYZIRT out; LISREG_FMT_DEVICE_XYZI (device records, payload = float intensity) — device in, device out, only the 16-byte
 * result header crosses the link.  More points kept than `capacity`: nothing is written, out->n receives the count, LISREG_ERR_ARG.
 * n_scan not 16 / 32 / 64, n < 0, or an output that overlaps the input: LISREG_ERR_ARG.  n == 0 or nothing kept: LISREG_OK, out->n = 0,
 * half_index = -1 (the reference reads points[0] of an empty cloud there). */
int  lisreg_pretreat(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt,
                     const lisreg_pretreat_params* params, lisreg_pretreat_out* out);
/* n_sweeps (<= 256) sweeps of device records (LISREG_FMT_DEVICE_XYZI) in ONE launch sequence — the same launches as a single call; every
 * outs[s] is identical to what a single call on sweeps[s] gives and feeds lisreg_extract_features_batch directly. */
int  lisreg_pretreat_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                           const lisreg_pretreat_params* params, lisreg_pretreat_out* outs);

/* ---- constant-velocity motion compensation of a sweep --------------------------------------------------------------- */
/* Replaces DistortionAdjust::SetMotionInfo, AdjustCloud and UpdateMatrix (src/core/distortionAdjust.cpp:412-417, 419-469, 471-480), the
 * middle stage of dataPretreatNode's LaserPretreatment -> DistortionAdjust -> FeatureExtraction: point 0 is dropped (the loop starts at
 * point_index = 1, :437), and every other point, in input order, becomes R(angular_velocity * real_time) * p + linear_velocity * real_time
 * with real_time = time - scan_period / 2 (:447) and R the float matrix of AngleAxisf t_V = t_Vz * t_Vy * t_Vx (:474-479); intensity,
 * ring and time are copied bit for bit.  The float / double steps, and the reading of Eigen they rest on, are listed in
 * tests/adjust_ref.py and at the top of lis-slam_amd/csrc/lisreg_motion.hip.  Which velocity to pass is the caller's choice (the
 * reference's deskewInfo takes vel_data_.front() of a deque it never pops, :245). */
typedef struct lisreg_motion {
    float  scan_period;           /* SetMotionInfo's first argument; the reference passes 0.1 (distortionAdjust.cpp:246) */
    double linear_velocity[3];    /* VelocityData, cast to float as SetMotionInfo's << does (:415-416) */
    double angular_velocity[3];
} lisreg_motion;
typedef struct lisreg_adjust_out {
    void*  cloud;         /* host input: structs of the input's stride; device input: lisreg_dpoint records  */
    int    capacity;      /* points; n - 1 is always enough                                                   */
    int    n;             /* written back: max(n - 1, 0)                                                      */
    float* time_device;   /* device input only: per-point time [capacity], shifted by one like the cloud      */
} lisreg_adjust_out;
int  lisreg_default_motion(lisreg_motion* m);                            /* 0.1f, zeros */
/* One sweep.  fmt: LISREG_FMT_XYZIRT — host PointXYZIRT structs in and out (stride >= 28; a record is copied whole, then its x y z are
 * replaced), time_device is not read; LISREG_FMT_DEVICE — device records with the ring in the payload plus the device time array
 * `time_device` [n], device records and times out (what lisreg_pretreat* writes goes in as it is, and what comes out goes into
 * lisreg_extract_features* as it is).  One launch.  capacity < n - 1: nothing is written, out->n receives the count, LISREG_ERR_ARG.
 * An output that overlaps the input: LISREG_ERR_ARG (the shift by one makes in-place a race).  n == 0 or 1: LISREG_OK, out->n = 0. */
int  lisreg_adjust_cloud(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt, const float* time_device,
                         const lisreg_motion* motion, lisreg_adjust_out* out);
/* n_sweeps (<= 256) sweeps of device records (LISREG_FMT_DEVICE), each with its own motion, in ONE launch behind one upload of the job
 * table; every outs[s] is identical to what a single call on sweeps[s] gives.  A refused argument (LISREG_ERR_ARG) writes no buffer. */
int  lisreg_adjust_cloud_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                               const float* const* time_device, const lisreg_motion* motions, lisreg_adjust_out* outs);

/* ---- RangeNet++ around the network: range-image projection and point labelling --------------------------------- */
/* The host code the reference wraps around its segmentation network, without the network (the model is the
 * caller's).  lisreg_rangenet_project replaces NetTensorRT::doProjection and the input half of NetTensorRT::infer (src/segnet/
 * netTensorRT.cpp:143-300, :333-354): spherical projection of the sweep into an img_h x img_w image in which the nearest point wins a
 * pixel, the invalid-pixel test, normalisation into the 5 x H x W input tensor (range, x, y, z, intensity; channel-major).
 * lisreg_rangenet_label replaces the output half (:403-428) and RangenetAPI::infer's argmax (src/core/rangenetAPI.cpp:50-73, :103-110):
 * invalid pixels masked, one logit vector per point through its pixel, argmax, labelled records — what lisreg_semantic_split takes.
 * The arithmetic is the reference's, operation for operation (float / double steps listed at the top of lis-slam_amd/csrc/
 * lisreg_rangenet.hip; a float libm function is the correctly rounded value).  Defined where the reference is not: among points of
 * exactly equal range in one pixel the one of highest input index wins; a point with a non-finite x, y, z or intensity takes no part
 * (pixel index -1, label 0); img_h * img_w <= 2^24; n_classes <= 32. */
typedef struct lisreg_rangenet_params {
    int    img_h, img_w;          /* the network's input height and width                                          */
    double fov_up, fov_down;      /* degrees, doubles as in the reference (net.hpp:103)                           */
    float  means[5], stds[5];     /* per channel (range, x, y, z, intensity).  The real ones belong to the caller's model — its
                                     arch_cfg.yaml, which is not part of the reference tree: the defaults are 0 and 1 */
    int    n_classes;             /* planes of the logits, 1 .. 32                                                 */
} lisreg_rangenet_params;
typedef struct lisreg_rangenet_out {   /* caller-owned DEVICE buffers                                              */
    float*         tensor;        /* [5][img_h][img_w]; may be a torch tensor's data_ptr()                         */
    unsigned char* invalid_mask;  /* [img_h * img_w]: 1 where the pixel is invalid (empty, or all five values truncate to 0) */
    int*           pixel_index;   /* [n]: y * img_w + x of every point, -1 for a non-finite one                    */
    int            n_valid;       /* written back: valid pixels (the one read-back of the call)                    */
} lisreg_rangenet_out;
int  lisreg_default_rangenet_params(lisreg_rangenet_params* p);   /* 64, 2048, 3.0, -25.0 (netTensorRT.cpp:144-145), means 0, stds 1, 20 */
/* One sweep.  fmt: LISREG_FMT_XYZI or LISREG_FMT_XYZI_PACKED (host sweep, uploaded first) or LISREG_FMT_DEVICE_XYZI (device records,
 * payload = float intensity; stride ignored).  The outputs are complete when the call returns.  img_h / img_w / n_classes out of range,
 * n < 0, a NULL buffer, or an output that overlaps the input or another output: LISREG_ERR_ARG.  n == 0: an all-invalid image, an
 * all-zero tensor, LISREG_OK. */
int  lisreg_rangenet_project(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt,
                             const lisreg_rangenet_params* params, lisreg_rangenet_out* out);
/* n_sweeps (<= 256) sweeps of device records (LISREG_FMT_DEVICE_XYZI) in ONE launch sequence; outs[s].tensor = base + s * 5 * H * W
 * gives the n_sweeps x 5 x H x W tensor of a batched network.  Every outs[s] is bit for bit what a single call on sweeps[s] gives. */
int  lisreg_rangenet_project_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                                   const lisreg_rangenet_params* params, lisreg_rangenet_out* outs);
/* Labels from the network's logits (DEVICE float [n_classes][img_h][img_w]).  cloud: the sweep that was projected (device records,
 * LISREG_FMT_DEVICE_XYZI or LISREG_FMT_DEVICE; the payload is not read); pixel_index / invalid_mask: what lisreg_rangenet_project wrote.
 * labelled_out: n LISREG_FMT_DEVICE records, x y z bit for bit, the label in the payload.  label_image_out: the img_h x img_w label
 * image (one byte per pixel), or NULL.  The outputs are complete when the call returns. */
int  lisreg_rangenet_label(lisreg_ctx* ctx, const void* cloud, int n, int fmt, const int* pixel_index,
                           const unsigned char* invalid_mask, const float* logits, const lisreg_rangenet_params* params,
                           void* labelled_out, unsigned char* label_image_out);
/* The same for n_sweeps (<= 256) sweeps in one launch sequence; label_image_out may be NULL, and so may any of its entries. */
int  lisreg_rangenet_label_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                                 const int* const* pixel_index, const unsigned char* const* invalid_mask,
                                 const float* const* logits, const lisreg_rangenet_params* params,
                                 void* const* labelled_out, unsigned char* const* label_image_out);
/* The kNN label clean-up of RangeNet++ (the "++"): lisreg_rangenet_label gives a point the argmax of its pixel, whoever won that pixel, so
 * a point that lost its pixel to a nearer surface inherits that surface's class.  lisreg_rangenet_label_knn votes instead, per point,
 * among the knn cells of a search x search window of the range image that are nearest to the point IN RANGE (Gaussian-weighted by their
 * distance in the window).  The reference tree has no text for this step; it is DEFINED, after the authors' published post-processing,
 * at the kNN section of lis-slam_amd/csrc/lisreg_rangenet.hip and in tests/rangenet_knn_ref.py: the range image holds the smallest
 * sqrtf((x*x + y*y) + z*z) of each pixel's points (+inf: empty); cells outside the image are zero padding (range 0, label 0; no wrap at
 * the azimuth seam); the centre cell takes the point's own range; d_j = fabsf(range_j - r) * w_j; the knn smallest in (d_j, then j) are
 * selected; a selected cell with cutoff > 0 && d_j > cutoff votes for nobody; the class 1 .. n_classes - 1 with the most votes wins, the
 * lowest id on a tie, and class 0 never; a point without any such vote gets no_vote_label; a point with pixel index -1 gets 0; a point
 * whose own range overflows keeps its pixel's label. */
typedef struct lisreg_rangenet_knn_params {
    int   knn;                    /* voters per point, 1 .. min(search * search, 16)                                 */
    int   search;                 /* window side: 1, 3, 5 or 7                                                      */
    float sigma;                  /* of the Gaussian over window offsets, finite and > 0                             */
    float cutoff;                 /* weighted range distance beyond which a selected cell does not vote; <= 0: none   */
    int   no_vote_label;          /* 0 .. n_classes - 1.  1 is the authors' behaviour (argmax + 1 of all-zero counts); 0, the default,
                                     sends such points to the outlier class of lisreg_semantic_split                 */
} lisreg_rangenet_knn_params;
int  lisreg_default_rangenet_knn_params(lisreg_rangenet_knn_params* p);   /* 5, 5, 1.0, 1.0, 0 — the model's own are the `post: KNN: params:` block of its arch_cfg.yaml */
/* Host only: the search * search window weights w_j = (float)(1.0 - g_j / sum g), g_j = exp(-(dx*dx + dy*dy) / (2 sigma^2)) in double.
 * Writes nothing when search or sigma is out of range. */
void lisreg_rangenet_knn_weights(const lisreg_rangenet_knn_params* knn_params, float* out /* [search * search] */);
/* lisreg_rangenet_label with the clean-up: the same arguments, argument rules and stream behaviour; label_image_out (or NULL) receives
 * the per-pixel argmax image, as in the plain call.  n_classes must be 2 .. 32; kNN parameters outside their limits: LISREG_ERR_ARG. */
int  lisreg_rangenet_label_knn(lisreg_ctx* ctx, const void* cloud, int n, int fmt, const int* pixel_index,
                               const unsigned char* invalid_mask, const float* logits, const lisreg_rangenet_params* params,
                               const lisreg_rangenet_knn_params* knn_params, void* labelled_out, unsigned char* label_image_out);
/* The same for n_sweeps (<= 256) sweeps in one launch sequence; every sweep gets bit for bit what a single call gives. */
int  lisreg_rangenet_label_knn_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n,
                                     const int* const* pixel_index, const unsigned char* const* invalid_mask,
                                     const float* const* logits, const lisreg_rangenet_params* params,
                                     const lisreg_rangenet_knn_params* knn_params, void* const* labelled_out,
                                     unsigned char* const* label_image_out);

/* The "semantic mask": SemanticFusionNode::categoryMapping (src/node/semanticFusionNode.cpp:173-189) splits the labelled
 * cloud, preserving order, by UsingLableMap[label] (config/label.yaml:177-196): 10 -> dynamic, 40 -> ground, 50 -> building,
 * 81 -> pole, anything else (label 0 has no entry) -> outlier.  These five clouds are what semantic_info carries and what
 * selects the edge (pole) and planar (ground + building + dynamic) feature sets of copies #2/#3.
 * using_label[32]: the map indexed by label & 31, or NULL for the reference's label.yaml.  Clouds: LISREG_FMT_XYZIL host
 * structs or LISREG_FMT_DEVICE records (label in the payload); outputs in the input's layout. */
typedef struct lisreg_semantic_out {
    void* cloud[5];          /* dynamic, ground, building, pole, outlier — the order of the reference's if-chain */
    int   cap[5];
    int   n[5];
} lisreg_semantic_out;
int  lisreg_semantic_split(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt,
                           const uint32_t* using_label /* [32] or NULL */, lisreg_semantic_out* out);

/* `*a += *b` for device records: the K (<= 8) clouds end to end into `out` (capacity >= the sum), one launch on the context's stream;
 * the call does not wait, every later call of this context is ordered behind it.  *n_out = the total (may be NULL). */
int  lisreg_concat_device(lisreg_ctx* ctx, int k, const void* const* in, const int* n, void* out, int* n_out);

/* lisreg_semantic_split for the labelled device clouds of up to LISREG_SEMANTIC_BATCH_MAX key frames (what lisreg_rangenet_label*_batch
 * writes) in one launch sequence whose length does not depend on n_frames — three launches — behind ONE upload of the job and tile
 * tables, with ONE read-back (n[5] + status per frame) and ONE host synchronisation, all on the context's stream.  using_label: one map
 * per call, [32] indexed by payload & 31, or NULL for label.yaml.  Per job, out.cloud[0..4][0 .. n[k]), out.n[0..4] and status are byte
 * for byte what lisreg_semantic_split(ctx, in, n, 16, LISREG_FMT_DEVICE, using_label, &out) gives for that frame alone: the stable
 * five-way partition in input order, records copied whole (all 16 bytes, whatever they hold), nothing written beyond n[k] records; a
 * NULL cloud[k] is counted and not written.  A frame some non-NULL cloud[k] of which has cap[k] below the class count gets status
 * LISREG_ERR_ARG, n[] = the five counts needed and nothing written in any of its buffers; every other frame is unaffected, and the
 * call returns LISREG_OK when the batch ran.  n_frames == 0: LISREG_OK, no launch; a frame with n == 0: five zero counts, LISREG_OK.
 * Refused with LISREG_ERR_ARG before anything is launched or written (lisreg_last_error names the job), in this order: n_frames outside
 * 0 .. LISREG_SEMANTIC_BATCH_MAX; jobs == NULL with n_frames > 0; per job n < 0, in == NULL with n > 0, cap[k] < 0 on a non-NULL cloud;
 * more than 2e9 points in all; an output range (cap[k] records) that meets any job's input range (its own included) or any other output
 * range, another class of the same job included.  Inputs may meet each other: two jobs may split the same cloud.  Outputs are complete
 * on return. */
#define LISREG_SEMANTIC_BATCH_MAX 256
typedef struct lisreg_semantic_job {
    const void*         in;  int n;   /* device lisreg_dpoint records, label in the payload */
    lisreg_semantic_out out;          /* cloud[5]: device buffers, NULL = that class is counted but not written; cap[5]; n[5] written back */
    int                 status;       /* written back: LISREG_OK or LISREG_ERR_ARG */
} lisreg_semantic_job;               /* LP64: in@0 n@8 out@16 (80 bytes) status@96, sizeof 104 */
int  lisreg_semantic_split_batch(lisreg_ctx* ctx, int n_frames, lisreg_semantic_job* jobs,
                                 const uint32_t* using_label /* [32] or NULL, one map per call */);

/* lisreg_concat_device for up to LISREG_CONCAT_BATCH_MAX jobs — currentCloudInit's surf source (dynamic_down + building_down +
 * ground_down) of every key frame of a batch — in ONE launch behind one upload of the job table, whatever n_jobs is, on the context's
 * stream; the call returns when the table has been read (the outputs are complete by then).  Per job, out[0 .. n_out) is byte for byte
 * what lisreg_concat_device(ctx, k, in, n, out, &n_out) writes, and n_out = the sum of n[0 .. k) (known on the host).  Refused with
 * LISREG_ERR_ARG before the launch, nothing written (lisreg_last_error names the job), in this order: n_jobs outside
 * 0 .. LISREG_CONCAT_BATCH_MAX; jobs == NULL with n_jobs > 0; per job k outside 0 .. 8, n < 0, a NULL input with n > 0, out_capacity
 * below the sum, a NULL out with a sum > 0; an `out` range (out_capacity records) that meets any job's input range or another job's
 * `out` range. */
#define LISREG_CONCAT_BATCH_MAX 1024
typedef struct lisreg_concat_job {
    const void* in[8]; int n[8]; int k;      /* k <= 8 device clouds, end to end in this order; an empty one may be NULL */
    void* out; int out_capacity;             /* device records */
    int   n_out;                             /* written back: the sum */
} lisreg_concat_job;
int  lisreg_concat_device_batch(lisreg_ctx* ctx, int n_jobs, lisreg_concat_job* jobs);

/* One host cloud (the reference's PCL structs: LISREG_FMT_XYZI, or LISREG_FMT_XYZIL whose uint16 at byte 20 — label, or the ring of a
 * raw sweep — becomes the payload) into a caller-owned device buffer of n 16-byte lisreg_dpoint records, through a pinned staging buffer
 * packed by the feeder threads; returns when the records are in HBM.  What a node's callback does first with a sensor_msgs cloud
 * (pcl::fromROSMsg in laserCloudInfoHandler, odomEstimationNode.cpp:164-175), for the *_DEVICE forms of the entry points. */
int  lisreg_upload_cloud(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt, void* dev_out);

/* ---- §8 f-3: local-map maintenance (src/include/subMap.h) -------------------------------------------------- */
/* Supported coordinate range of this section: |coordinate| < 8192 m for the map cloud of a k = 1 index and for its queries
 * (lisreg_map_index_set*, lisreg_nearest, lisreg_dynamic_filter, the ICP rows that search it).  The k = 1 walk carries the same
 * millimetre of absolute slack as the 5-NN front-ends (see lisreg_set_target): it absorbs one rounding each of ox + ix * cell and of
 * xl + cell — together one float step of the coordinate, 0.49 mm in [4096, 8192) m — plus about 0.02 mm from the float cell
 * assignment at any offset; at 0.98 mm per step, from 8192 m on, it is spent.  lisreg_bbx_filter, lisreg_cloud_bounds,
 * lisreg_voxel_downsample* and lisreg_transform_cloud carry no slack at all: they restate the reference's arithmetic operation for
 * operation and equal it bit for bit at any offset at which floorf(x / leaf) fits an int (tests/test_far_frame.py: 8000 m, leaf
 * 0.05 m).  The fp64 verifiers (lisreg_ndt_*, lisreg_vgicp_*, lisreg_fgicp_*) form their cell faces in double with a slack of
 * 1e-3 of the cell edge and are not limited by this range. */
/* A k = 1 search index over one cloud, kept in HBM under `slot` (its own slot space, separate from the registration
 * targets).  Replaces pcl::search::KdTree<PointT>::setInputCloud (subMap.h:889 `local_map->tree_dynamic`,
 * subMapOptmizationNode.cpp:2779 icp.setInputTarget).  LISREG_FMT_DEVICE clouds are referenced, not copied. */
int  lisreg_map_index_set(lisreg_ctx* ctx, int slot, const void* cloud, int n, int stride_bytes, int fmt);
/* The same for n clouds at once — setInputTarget of every candidate of a loop-closure batch (subMapOptmizationNode.cpp:2793 inside the
 * candidate loop of :2776-2840): one bounding-box launch, one read-back and ONE sort launch sequence for all of them.  slots[k] receives
 * clouds[k] (counts[k] points; one stride / format for the batch; a slot may not be named twice).  Each index equals what
 * lisreg_map_index_set builds for that cloud, bit for bit.  Two or more clouds whose grids fit it take the strip form of the build
 * (option "index_build": 0 keeps the batched bucket sort; 256 clouds of 200 k points: 1.2 instead of 4.9 ms). */
int  lisreg_map_index_set_batch(lisreg_ctx* ctx, int n_maps, const int* slots, const void* const* clouds, const int* counts,
                                int stride_bytes, int fmt);
/* nearestKSearch(query, k = 1) for a whole cloud: idx_out[i] = index into the map cloud of the nearest point, or -1 when it
 * is farther than max_dist (pass a huge value for the reference's unbounded search); sqd_out[i] = squared distance in float,
 * accumulated x, y, z like FLANN's L2_Simple.  Equidistant candidates resolve to the smallest index.  A point at exactly max_dist
 * is found (d2 <= max_dist * max_dist, the product formed in float after max_dist is clipped to 1.8e19).  Where idx_out[i] is -1 — nothing
 * within max_dist, a NaN query, an empty map — sqd_out[i] is the first float above that product (the bound the search started from; a
 * denormal for max_dist = 0), never a distance.  NaN map points are never returned.  idx_out / sqd_out are host arrays, or device
 * arrays when fmt is LISREG_FMT_DEVICE. */
int  lisreg_nearest(lisreg_ctx* ctx, int slot, const void* query, int n, int stride_bytes, int fmt, float max_dist,
                    int* idx_out, float* sqd_out);
/* SubMapManager::map_scan_feature_pts_distance_removal (subMap.h:1064-1100): drop the points of `cloud` within
 * center_radius (x, y) of the sensor whose nearest point of the indexed map lies at distance d with d <= near_dist_thre or
 * dist_thre_min <= d <= dist_thre_max; order preserved.  `out` has room for n points of the input layout.  Returns
 * LISREG_NOT_ENOUGH_FEATURES (and out = in) where the reference returns false (n <= 10). */
int  lisreg_dynamic_filter(lisreg_ctx* ctx, int slot, const void* cloud, int n, int stride_bytes, int fmt, float center_radius,
                           float dist_thre_min, float dist_thre_max, float near_dist_thre, void* out, int* n_out);
/* SubMapManager::bbx_filter (subMap.h:1124-1152): bounds = {min_x, min_y, min_z, max_x, max_y, max_z} (bounds_t); keeps the
 * points strictly inside, or the others when delete_box is set; order preserved. */
int  lisreg_bbx_filter(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt, const double bounds[6],
                       int delete_box, void* out, int* n_out);
/* SubMapManager::get_cloud_bbx (subMap.h:131-163); an empty cloud yields {DBL_MAX x3, -DBL_MAX x3}. */
int  lisreg_cloud_bounds(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt, double bounds[6]);

/* The sliding local map as ONE device-resident object (localMap_t, subMap.h:679-777): five class clouds in the map frame kept in
 * HBM as 16-byte records, class order of append_feature / merge_feature_points: 0 dynamic, 1 pole, 2 ground, 3 building,
 * 4 outlier.  lisreg_localmap_insert = SubMapManager::insert_local_map (subMap.h:979-1059) as makeSubMapThread calls it
 * (subMapOptmizationNode.cpp:640-646, 708-714); lisreg_localmap_extract = extractSlidingCloud (:1369-1432) followed by the two
 * kdtree setInputCloud calls of scan2SubMapOptimization (:1517-1518): it leaves the registration target in `target_slot`
 * (pass -1 to skip that), so a frame loop is  extract -> lisreg_align / batch -> insert  with no cloud crossing PCIe
 * except the incoming frame. */
typedef struct lisreg_localmap_params {
    int   max_num_pts;                    /* 80000: dynamic removal starts once feature_point_num > max_num_pts / 5 (:605, subMap.h:1007) */
    int   dynamic_removal_on;             /* map_based_dynamic_removal_on = true (:608)                                         */
    float dynamic_removal_center_radius;  /* 30.0 (:609) — compared with x^2 + y^2 of the MAP-frame point, as the reference does */
    float dynamic_dist_thre_min;          /* 0.3  (:610)                                                                        */
    float dynamic_dist_thre_max;          /* 3.0  (:611); widened to at least min + 0.1 like subMap.h:1006                      */
    float near_dist_thre;                 /* 0.03 (:612)                                                                        */
    float leaf[5];                        /* in-place voxel grids of extractSlidingCloud: 0.1, 0.05, 0.4, 0.2, 0.6 (:1385-1389)  */
    float crop_box[6];                    /* cur_bbx = {-70,-70,-10, 70,70,20} (:1377-1379), moved by the current pose           */
    float crop_pad;                       /* 2.0: bbx_boundary_pad of get_intersection_bbx (:1384)                               */
} lisreg_localmap_params;
typedef struct lisreg_localmap_info {
    int    n[5];                          /* points per class now                                   */
    int    feature_point_num;             /* as of the last insert (subMap.h:1039-1043)             */
    double bound[6];                      /* localMap->bound as of the last insert (:1047-1049)     */
    double crop[6];                       /* bbx_intersection of the last extract                   */
    int    n_target_corner, n_target_surf;/* laserCloud{Corner,Surf}FromSubMap sizes of the last extract */
} lisreg_localmap_info;
int  lisreg_localmap_default_params(lisreg_localmap_params* p);
int  lisreg_localmap_reset(lisreg_ctx* ctx, int map_id);
/* clouds[5] / n[5]: the key frame's UN-downsampled class clouds in the sensor frame (semantic_dynamic, _pole, _ground, _building,
 * _outlier); host PointXYZIL structs or LISREG_FMT_DEVICE records.  pose = the frame's optimized_pose {roll,pitch,yaw,x,y,z}.
 * The outlier cloud is accepted and ignored, exactly as the reference leaves its transform commented out (subMap.h:1003).
 * While the map's dynamic class is empty the dynamic removal does not run, whatever feature_point_num is: every dynamic point of
 * the frame is appended (the reference reads distances_square[0] of an empty vector there, which is undefined; the same holds for
 * lisreg_submap_insert). */
int  lisreg_localmap_insert(lisreg_ctx* ctx, int map_id, const void* const clouds[5], const int n[5], int stride_bytes, int fmt,
                            const float pose[6], const lisreg_localmap_params* params, lisreg_localmap_info* info);
int  lisreg_localmap_extract(lisreg_ctx* ctx, int map_id, const float cur_pose[6], const lisreg_localmap_params* params,
                             int target_slot, lisreg_localmap_info* info);
/* Copy one cloud out as 16-byte records (host or device destination): cls 0-4 = the class clouds, 5 / 6 = the corner / surf
 * target of the last extract.  *n_out is always set; LISREG_ERR_ARG if capacity is too small. */
int  lisreg_localmap_get(lisreg_ctx* ctx, int map_id, int cls, void* out, int capacity, int* n_out);
/* Copy #3's side of the same row: submap_t + SubMapManager::insert_submap (src/include/subMap.h:835-978) and
 * SubMapOptmizationNode::extractSubMapCloud (src/node/subMapOptmizationNode.cpp:3976-4081), device-resident.  Submaps share the id space and
 * the storage of the local maps (lisreg_localmap_reset / _get work on them: classes 0-4, 5 / 6 = the clouds of the last extract).
 *   _insert  = insert_submap: the key frame's DOWN-sampled class clouds (semantic_*_down, all FIVE — the outlier class is appended here,
 *              :882) are transformPointCloud'ed by the frame's relative_pose into the submap's own frame, the dynamic class goes through
 *              the map-based removal once feature_point_num > max_num_pts / 5 (:887-892), append_feature, feature_point_num, local_bound
 *              over all classes (:961-963) and bound = transform_bbx(local_bound, local_cp, submap_pose_6D_optimized) (:968-969);
 *              relative_pose = NULL is fisrt_submap (:785-830): the first key frame of a submap, appended as it is;
 *   _extract = extractSubMapCloud for (previous submap, current submap): bound boxes under the two poses, their intersection padded by
 *              `pad` (10 m, :3995); TARGET = previous submap's pole | ground + building + dynamic transformed into the map frame by pre_pose
 *              and cropped (:3997-4020), installed as registration target `target_slot` (-1: assembled only); SOURCES = current submap's
 *              pole | dynamic + ground + building in the submap's own frame, cropped by the intersection box moved into that frame
 *              (tran_map.inverse(), :4056-4061) and voxel-downsampled (0.2 / 0.5, :4066-4067): device records owned by the context, valid
 *              until the next call on that submap — hand them to lisreg_align (LISREG_FMT_DEVICE, LISREG_VARIANT_SUBMAP) with cur_pose as
 *              the guess = subMap2SubMapOptimization (:4485-4540);
 *   _crop_boxes = the host arithmetic of the two boxes alone (double boxes, float matrices, Eigen's cofactor Affine3f::inverse). */
typedef struct lisreg_submap_info {
    int    n[5];                          /* points per class now (dynamic, pole, ground, building, outlier)       */
    int    feature_point_num;
    double local_bound[6];                /* local_bound: {min x, y, z, max x, y, z} in the submap's own frame       */
    double bound[6];                      /* bound: local_bound moved by submap_pose (transform_bbx)                 */
} lisreg_submap_info;
typedef struct lisreg_submap_extract_out {
    double isect[6];                      /* bbx_intersection in the map frame                                       */
    double isect_local[6];                /* the same box moved into the current submap's frame                      */
    int    n_target_corner, n_target_surf;/* laserCloud{Corner,Surf}FromSubMap                                       */
    const void* src_corner; int n_src_corner;     /* laserCloudCornerLastDS (device records)                         */
    const void* src_surf;   int n_src_surf;       /* laserCloudSurfLastDS                                            */
} lisreg_submap_extract_out;
int  lisreg_submap_insert(lisreg_ctx* ctx, int map_id, const void* const clouds[5], const int n[5], int stride_bytes, int fmt,
                          const float relative_pose[6], const float submap_pose[6], const lisreg_localmap_params* params,
                          lisreg_submap_info* info);
int  lisreg_submap_extract(lisreg_ctx* ctx, int pre_id, int cur_id, const float pre_pose[6], const float cur_pose[6], float pad,
                           float corner_leaf, float surf_leaf, int target_slot, lisreg_submap_extract_out* out);
void lisreg_submap_crop_boxes(const double pre_local_bound[6], const float pre_pose[6], const double cur_local_bound[6],
                              const float cur_pose[6], float pad, double isect[6], double isect_local[6]);

/* The global map (visualizeGlobalMapThread: publishGlobalMap, src/node/subMapOptmizationNode.cpp:3553-3574, and the PCD export,
 * :3502-3514) and every other "these classes of these submaps under these poses" cloud of the reference (the loop-verification target
 * :2787-2790, the corrected current submap :2906-2912, laserCloudFromPre :1151-1154) as ONE gather over the resident store:
 *   segment 5 * i + k of the output = class k of map_ids[i] (0 dynamic, 1 pole, 2 ground, 3 building, 4 outlier) moved by poses[i]
 *   ({roll,pitch,yaw,x,y,z} -> lisreg_pose_to_matrix, the arithmetic of lisreg_transform_cloud bit for bit); segments lie end to end in
 *   that order (:3560-3571); a class that is masked out or empty is an empty segment.  map_ids may name a map twice; local maps and
 *   submaps share the id space; which submaps go in (the reference leaves the newest out unless FINISHMAP, :3561-3562) is the caller's list.
 *   poses == NULL: no arithmetic at all, the records are copied bit for bit (an identity matrix would turn -0.0f into +0.0f).
 *   The payload word (the label) is copied as bits.  The store is read, never changed.
 * out_fmt LISREG_FMT_DEVICE: 16-byte lisreg_dpoint records.  LISREG_FMT_XYZIL: 32-byte PointXYZIL structs — x, y, z, the label's low 16
 *   bits as uint16 at byte 20, zeros everywhere else: the store keeps 16-byte records, so the intensity is not available and reads 0.0f.
 * out may be DEVICE memory (capacity_points records / structs): the table upload and one kernel launch go on the context's stream
 *   whatever n_maps is, the call does not wait for the GPU, and later calls of the context are ordered behind it (like
 *   lisreg_concat_device).  Or HOST memory (anything the runtime does not know as device memory): the cloud is produced chunk_points
 *   points at a time into two buffers of the context, the copy of one chunk under the kernel of the next, and the call returns when the
 *   data is in out.  All offsets are 64-bit: a map of a few hundred submaps passes 2^32 bytes.
 * _gather_count: *n_total = points the gather would write; seg_offsets[n_maps * 5 + 1] (or NULL) = where every segment starts, the last
 *   entry = *n_total.  _gather: *n_out and seg_offsets the same.
 * Errors: an id that names no map (never reset, never inserted into) LISREG_ERR_NO_TARGET — a map that was only reset is an empty map; capacity_points too small LISREG_ERR_ARG with *n_out = the need — in both
 *   cases nothing is written to out; n_maps < 0, NULL params, class_mask bits above 31, an out_fmt other than the two: LISREG_ERR_ARG.
 *   n_maps == 0 or class_mask == 0: LISREG_OK, 0 points. */
#define LISREG_CLS_DYNAMIC 1u   /* bit k = class k of the store: 0 dynamic, 1 pole, 2 ground, 3 building, 4 outlier */
#define LISREG_CLS_POLE 2u
#define LISREG_CLS_GROUND 4u
#define LISREG_CLS_BUILDING 8u
#define LISREG_CLS_OUTLIER 16u
#define LISREG_CLS_ALL 31u
typedef struct lisreg_gather_params {
    unsigned class_mask;    /* LISREG_CLS_ALL = publishGlobalMap; 15 = the verification target of :2787-2790 */
    int      out_fmt;       /* LISREG_FMT_DEVICE: 16-byte records; LISREG_FMT_XYZIL: 32-byte PointXYZIL structs */
    int      chunk_points;  /* host destinations only: points per staged chunk, 0 = the library's default */
} lisreg_gather_params;
int  lisreg_default_gather_params(lisreg_gather_params* p);      /* 31, LISREG_FMT_DEVICE, 0 */
int  lisreg_submap_gather_count(lisreg_ctx* ctx, int n_maps, const int* map_ids, unsigned class_mask,
                                long long* n_total, long long* seg_offsets /* n_maps*5 + 1, or NULL */);
int  lisreg_submap_gather(lisreg_ctx* ctx, int n_maps, const int* map_ids, const float* poses /* n_maps x 6, or NULL */,
                          const lisreg_gather_params* params, void* out, long long capacity_points,
                          long long* n_out, long long* seg_offsets /* or NULL */);

/* The odometry node's target (odomEstimationNode.cpp, USING_MULTI_FRAME_TARGET), device-resident:
 *   _push   = saveKeyFrames (:421-468): the frame's FULL corner / surf feature clouds (host PCL structs or LISREG_FMT_DEVICE records,
 *             sensor frame) are transformPointCloud'ed by `pose` into the map frame and kept; the oldest frames are dropped until at
 *             most max_keep remain (the reference keeps fewer than 20: max_keep = 19);
 *   _target = laserCloudInfoHandler (:185-207) + the two kd-tree builds (:602-603): the kept frames concatenated NEWEST FIRST, voxel
 *             grids with the two leaf sizes (mappingCornerLeafSize 0.2, mappingSurfLeafSize 0.4), installed as target `target_slot`
 *             (-1: assembled only).  The target clouds live in the ring until the next _target / _reset of that ring.  The reference
 *             rebuilds clouds and trees for every sweep although they only change with a key frame; here a call finds its work done —
 *             and returns at once — while no frame was pushed since the last call, the leaf sizes are the same and `target_slot` still
 *             holds what that call installed (any lisreg_set_target* on the slot in between makes the next call rebuild). */
typedef struct lisreg_keyframes_info {
    int n_keyframes;                      /* frames kept now                                                 */
    int n_target_corner, n_target_surf;   /* laserCloud{Corner,Surf}FromMapDS sizes of the last _target call */
} lisreg_keyframes_info;
int  lisreg_keyframes_reset(lisreg_ctx* ctx, int ring_id);
int  lisreg_keyframes_push(lisreg_ctx* ctx, int ring_id, const void* corner, int n_corner, const void* surf, int n_surf, int stride_bytes,
                           int fmt, const float pose[6], int max_keep, lisreg_keyframes_info* info);
int  lisreg_keyframes_target(lisreg_ctx* ctx, int ring_id, float corner_leaf, float surf_leaf, int target_slot, lisreg_keyframes_info* info);
/* updateInitialGuess with neither IMU nor odometry (odomEstimationNode.cpp:351-392; subMapOptmizationNode.cpp:984-1020): the
 * constant-velocity guess T_cur * (T_last^-1 * T_cur). */
void lisreg_predict_pose(const float T_last[6], const float T_cur[6], float T_guess[6]);
/* updateInitialGuess as a whole (odomEstimationNode.cpp:297-419 = variant 0; subMapOptmizationNode.cpp:896-1032 = variant 1): the first
 * call takes the IMU attitude (yaw 0 unless useImuHeadingInitialization); with odometry (cloudInfo.odomAvailable, the IMU pre-integration
 * guess initialGuess*) the increment between consecutive guesses is applied to the pose; with the IMU alone the increment of its attitude;
 * with neither the constant-velocity guess above.  The copies differ where the reference's do: #1 tests `odomAvailable == false` alone for
 * the constant-velocity branch and lets the FIRST odometry message fall through to the IMU increment; #2 saves the IMU attitude in the
 * odometry branch only when there is an IMU and takes the constant-velocity branch only with neither input.  The function-local statics
 * of the reference live in lisreg_guess_state (zero-initialise; one per node).  T = transformTobeMapped / transformTobeSubMapped
 * {roll,pitch,yaw,x,y,z}, updated in place; T_prediction (may be NULL) receives transPredictionMapped where the reference sets it.
 * Host arithmetic, Eigen's Affine3f operations step by step in float. */
typedef struct lisreg_guess_input {
    int   odom_available, imu_available;                                  /* cloudInfo.odomAvailable, .imuAvailable           */
    float imu_roll_init, imu_pitch_init, imu_yaw_init;                    /* cloudInfo.imuRollInit, ...                       */
    float initial_guess_x, initial_guess_y, initial_guess_z;              /* cloudInfo.initialGuessX, ...                     */
    float initial_guess_roll, initial_guess_pitch, initial_guess_yaw;
} lisreg_guess_input;
typedef struct lisreg_guess_state {
    int   first_trans_available;                 /* firstTransAvailable                                  */
    int   last_imu_pre_trans_available;          /* lastImuPreTransAvailable                             */
    int   first;                                 /* `first` of the constant-velocity branch              */
    int   reserved;
    float last_imu_transformation[12];           /* lastImuTransformation, row-major 3x4                 */
    float last_imu_pre_transformation[12];       /* lastImuPreTransformation                             */
    float last_transform_tobe_mapped[6];         /* lastTransformTobeMapped / lastTransformTobeSubMapped */
} lisreg_guess_state;
void lisreg_guess_state_init(lisreg_guess_state* st);
void lisreg_update_initial_guess(int variant, int use_imu_heading_initialization, const lisreg_guess_input* in, lisreg_guess_state* st,
                                 float T[6], float T_prediction[6]);

/* ---- §8 f-4: pcl::IterativeClosestPoint as the loop-closure / relocalisation code drives it ------------------- */
/* Call sites: src/node/subMapOptmizationNode.cpp:2763-2833 (loop closure: 10 m, 30 iterations, 1e-4, 1e-4),
 * :1444-1465 and :4400-4420 (0.2 m, 50 iterations, 1e-5, 1e-5); RANSAC iterations 0 everywhere, no rejectors.
 * Point-to-point ICP: per iteration k = 1 correspondences within max_corr_dist -> closed-form rigid transform
 * (TransformationEstimationSVD = Umeyama without scale) -> DefaultConvergenceCriteria. */
enum {                       /* pcl::registration::DefaultConvergenceCriteria::ConvergenceState */
    LISREG_ICP_NOT_CONVERGED      = 0,
    LISREG_ICP_ITERATIONS         = 1,
    LISREG_ICP_TRANSFORM          = 2,
    LISREG_ICP_ABS_MSE            = 3,
    LISREG_ICP_REL_MSE            = 4,
    LISREG_ICP_NO_CORRESPONDENCES = 5
};
typedef struct lisreg_icp_params {
    double max_corr_dist;               /* setMaxCorrespondenceDistance (compared squared, in double, like PCL) */
    int    max_iters;                   /* setMaximumIterations */
    int    reserved;
    double transformation_epsilon;      /* setTransformationEpsilon: squared-translation bound, and 1 - eps bounds cos(angle) */
    double euclidean_fitness_epsilon;   /* setEuclideanFitnessEpsilon -> relative MSE threshold */
    double prev_mse;                    /* correspondences_prev_mse_: DBL_MAX on a fresh object; the reference's `static`
                                           ICP objects carry it from one align() to the next (feed lisreg_icp_result.prev_mse back) */
} lisreg_icp_params;
typedef struct lisreg_icp_result {
    float  final_transform[16];         /* getFinalTransformation(), row-major 4x4 */
    int    converged;                   /* hasConverged() */
    int    iters;                       /* nr_iterations_ */
    int    state;                       /* LISREG_ICP_* */
    int    n_corr_last;                 /* correspondences of the last iteration */
    double fitness;                     /* getFitnessScore(): mean squared k = 1 distance of the aligned source, unbounded */
    double prev_mse;
} lisreg_icp_result;
/* {10, 30, 1e-4, 1e-4} for kind 0 (loop closure), {0.2, 50, 1e-5, 1e-5} for kind 1; prev_mse = DBL_MAX */
int  lisreg_icp_default_params(int kind, lisreg_icp_params* p);
/* align(): target = the map index in `slot` (setInputTarget), source = `source` (setInputSource), guess = row-major 4x4 or
 * NULL for identity.  aligned_out: NULL, or room for n points of the input layout (the `output` cloud of align()). */
int  lisreg_icp_align(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                      const lisreg_icp_params* params, const float* guess, lisreg_icp_result* result, void* aligned_out);

/* The candidate loop of loop-closure verification as one call (detectLoopClosureForSubMap, subMapOptmizationNode.cpp:2776-2840; BASELINE
 * configs[3]: per candidate setInputTarget(:2793) / setInputSource(:2823) / align(:2831) / getFitnessScore(:2835) / hasConverged(:2836) /
 * getFinalTransformation(:2841)).  Item k aligns ITS source against the map index of ITS slot from ITS guess; every ICP iteration is one
 * launch sequence over all items, an item that has converged drops out of the launches that follow, results[k] is what
 * lisreg_icp_align returns for item k alone — to the bit (the sums are formed by one tree whatever the batch size).
 * chain_prev_mse: 0 = every item starts from params->prev_mse (fresh ICP objects); 1 = the reference's `static` object (:2763), whose
 * DefaultConvergenceCriteria carries correspondences_prev_mse_ from one align() to the next: item 0 starts from params->prev_mse, item
 * k from results[k - 1].prev_mse, in array order (results as if the items had been aligned one after the other).
 * Sources: host PCL structs or LISREG_FMT_DEVICE records (one stride / format for the batch); n = 0 items are allowed. */
typedef struct lisreg_icp_item {
    const void*  source;                /* setInputSource */
    int          n;
    int          slot;                  /* setInputTarget: lisreg_map_index_set(slot) */
    const float* guess;                 /* row-major 4x4, NULL = identity */
} lisreg_icp_item;
int  lisreg_icp_align_batch(lisreg_ctx* ctx, const lisreg_icp_item* items, int n_items, int stride_bytes, int fmt,
                            const lisreg_icp_params* params, int chain_prev_mse, lisreg_icp_result* results);

/* OptimizedICPGN (src/core/registration.cpp:19-115, src/include/registration.h:44-70): Gauss-Newton point-to-point ICP — per
 * iteration k = 1 correspondences, J = [I, -R hat(p)], H += J^T J, B -= J^T e, delta = H^-1 B, t += delta[0:3],
 * R = R exp(delta[3:6]) (Sophus SO3).  The class is never instantiated in the reference (commented-out call sites only); it is
 * built because SURVEY.md §8 f-4 lists it.  Quirk kept: the squared k = 1 distance is compared with the un-squared
 * max_correspond_distance (:50).  No convergence test (HasConverged() returns true). */
typedef struct lisreg_icpgn_result {
    float final_transform[16];          /* result_pose, row-major 4x4 */
    int   steps_applied;                /* iterations whose Hessian had a non-zero determinant */
    int   n_corr_last;
    float fitness;                      /* GetFitnessScore() */
    int   reserved;
} lisreg_icpgn_result;
/* SetTargetCloud = lisreg_map_index_set(slot); Match(source, predict_pose, transformed_out, result) + GetFitnessScore() */
int  lisreg_icp_gn_match(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                         unsigned max_iterations, float max_correspond_distance, const float predict_pose[16],
                         lisreg_icpgn_result* result, void* transformed_out);

/* The candidate loop of detectLoopClosureForSubMapICP (src/node/subMapOptmizationNode.cpp:2496-2621: a static OptimizedICPGN
 * myICP(30, 10) and, per candidate, SetTargetCloud / Match / GetFitnessScore / HasConverged, then the `best` rule) as ONE call (DESIGN.md
 * section 7s).  Item k matches sources[items[k].source] against the map index of items[k].slot from items[k].predict_pose.
 * Batch equals single: results[k] is what lisreg_icp_gn_match(ctx, items[k].slot, sources[items[k].source], ..., max_iterations,
 *   max_correspond_distance, predict_pose or identity, &r, NULL) writes, in all bytes of lisreg_icpgn_result, whatever else is in the
 *   batch: the quirk of :49-50 (squared distance against the un-squared threshold), a negative max_correspond_distance does no
 *   iteration work, max_iterations == 0 gives the pose untouched plus a fitness, the pcl::isFinite filter, a singular Hessian skips the
 *   step.  (An item keeps the lanes per query, the partial rows and the order of sums of its single call.)
 * Sources: host PCL structs or LISREG_FMT_DEVICE records, one stride and one format for the call; a source is staged once however
 *   many items name it; a source no item names is neither checked nor staged (its pointer may be NULL, its n anything).
 * info->best: bestScore starts at DBL_MAX and the items are walked in order; an item with (double)fitness > bestScore is skipped, any
 *   other is taken — equal scores go to the later item and a NaN score is taken, as the comparison of :2551-2558 is written
 *   (HasConverged() is always true and drops out).  -1 only for n_items == 0.
 * Refused for the whole batch, results untouched (LISREG_ERR_ARG / LISREG_ERR_NO_TARGET as the single call chooses): NULL items /
 *   results / sources / n with n_items > 0, n_items < 0, a source index out of range, a slot without a map index, max_iterations >
 *   100000, a named source the single call refuses, a batch whose workgroups or partial rows do not fit 32-bit counts (nor may the
 *   source points summed over the items: the neighbours are kept per item).
 *   n_items == 0 is LISREG_OK with best = -1.  There is no per-item transformed_out and there are no per-item parameters.
 * Synchronisation: every iteration is one correspondence launch per lanes-per-query class present (at most three, one in practice)
 *   and one solve launch over all items; the host waits only every 64 iterations (as the single call does, to bound the queue) and for
 *   the read-back: n_syncs = max_iterations / 64 + 1 (1 when a negative max_correspond_distance leaves nothing to iterate).  Ordered
 *   on the context's stream (lisreg_set_stream).
 * Memory (grow-only, the batch's own: lisreg_icp_align_batch's and lisreg_icp_gn_match's scratch is left alone): per item a state of
 *   192 bytes and a table entry of 48, per workgroup of 256 lanes a partial row of 176 bytes, per (item, source point) 4 bytes for the
 *   neighbour kept as the next iteration's seed, and the host sources staged as 16-byte records. */
typedef struct lisreg_icpgn_item {
    int          source;                /* index into sources[] */
    int          slot;                  /* SetTargetCloud: lisreg_map_index_set(slot) */
    const float* predict_pose;          /* row-major 4x4, NULL = identity */
} lisreg_icpgn_item;                    /* 16 bytes */
typedef struct lisreg_icpgn_batch_info {
    int best;                           /* see above; -1 only for n_items == 0 */
    int n_sources_staged;               /* named sources actually staged */
    int n_syncs;                        /* host synchronisations of the call, read-back included */
    int reserved;
} lisreg_icpgn_batch_info;              /* 16 bytes */
int  lisreg_icp_gn_match_batch(lisreg_ctx* ctx, const void* const* sources, const int* n, int n_sources, int stride_bytes, int fmt,
                               const lisreg_icpgn_item* items, int n_items, unsigned max_iterations, float max_correspond_distance,
                               lisreg_icpgn_result* results, lisreg_icpgn_batch_info* info /* may be NULL */);

/* ---- §7j: Normal Distributions Transform registration (loop-closure verification) ------------------------------------
 * select_registration_method("NDT") (src/core/registration.cpp:147-155) returns a pcl::NormalDistributionsTransform with
 * epsilon 0.01, step size 0.1, resolution 1.0 and 35 iterations; detectLoopClosureForSubMap carries the same four settings as its
 * first choice of verifier (src/node/subMapOptmizationNode.cpp:2756-2760).  The method: the target is cut into voxels of edge
 * `resolution`, every voxel with enough points becomes a Gaussian (mean, inflated covariance), and Newton steps with a
 * More-Thuente line search maximise the sum of the Gaussians' responses to the transformed source points (Magnusson 2009, eq.
 * 6.8-6.21, algorithm 2).  The DEFINITION is tests/ndt_ref.py (PCL's source is not available to this project); it departs from
 * what PCL is believed to do in four places:
 *   - the transform: source points are transformed in double from their float coordinates (PCL transforms the cloud in float);
 *   - the covariance normalisation: sum d d^T / (n - 1) around the double mean, two passes (PCL's is believed to differ by a
 *     factor of the order (n - 1) / n);
 *   - the angle chart: p = (tx, ty, tz, a, b, c), x' = Rx(a) Ry(b) Rz(c) x + t, a = atan2(-R12, R22), b = asin(R02),
 *     c = atan2(-R01, R00) for a guess matrix; Eigen's [0, pi] eulerAngles convention is not reproduced (the output is the transform);
 *   - the line-search flag: line_search = 1 runs More-Thuente with the interval starting NOT converged (strong Wolfe conditions,
 *     at most 10 trials, the next trial selected before the interval is updated, a trial that coincides with an end point ends the
 *     search); line_search = 0 is the behaviour of PCL releases remembered to start with the flag set, so that the loop never
 *     runs: one evaluation at clamp(|delta|, transformation_epsilon / 2, step_size).
 * The GPU evaluates score, gradient and Hessian (one lane per source point, fp64, fixed-order sums: two evaluations of the same
 * input give the same bits); the 6 x 6 solve and the line search run on the host in double. */
typedef struct lisreg_ndt_params {
    double resolution;                  /* setResolution: voxel edge */
    double step_size;                   /* setStepSize: the longest Newton step */
    double transformation_epsilon;      /* setTransformationEpsilon */
    double outlier_ratio;               /* 0.55 */
    double min_covar_eigvalue_mult;     /* 0.01: the two smaller eigenvalues are raised to this fraction of the largest */
    int    max_iters;                   /* setMaximumIterations */
    int    min_points_per_voxel;        /* 6 */
    int    line_search;                 /* 1 More-Thuente, 0 a single clamped step (see above) */
    int    reserved;
} lisreg_ndt_params;
typedef struct lisreg_ndt_info {
    int dims[3];                        /* voxel grid of the target */
    int n_voxels;                       /* voxels holding at least one finite point */
    int n_valid;                        /* voxels that became a Gaussian */
    int reserved;
} lisreg_ndt_info;
typedef struct lisreg_ndt_result {
    float  final_transform[16];         /* getFinalTransformation(), row-major 4x4 */
    double p[6];                        /* tx, ty, tz, a, b, c of it */
    int    converged;                   /* hasConverged() */
    int    iters;
    int    n_evals;                     /* evaluations of the score (with or without the Hessian) */
    int    reserved;
    long long n_pairs_last;             /* (source point, voxel) pairs of the last evaluation */
    double score;                       /* of the last evaluation */
    double trans_probability;           /* getTransformationProbability(): score / n */
} lisreg_ndt_result;
/* kind 0: {1.0, 0.1, 0.01, 0.55, 0.01, 35, 6, 1} */
int  lisreg_ndt_default_params(int kind, lisreg_ndt_params* p);
/* setInputTarget + setResolution: the Gaussians of `cloud` into NDT slot `slot` (0 .. 65535; NDT slots are apart from the map-index
 * slots).  Uses resolution, min_points_per_voxel and min_covar_eigvalue_mult of `params`.  NaN points belong to no voxel.  Refused
 * (LISREG_ERR_ARG): n <= 0, resolution <= 0, an infinite coordinate, a grid of more than 2^26 cells (the cell table is dense),
 * a target without a valid voxel.  info may be NULL.  Besides the Gaussians the slot keeps a search grid over the target's finite
 * points, for the fitness score of lisreg_ndt_align_batch (§7o): 16 bytes per finite point and 4 per grid cell (3.2 MB for a target
 * of 200 000 points); the voxels and every alignment do not depend on it. */
int  lisreg_ndt_set_target(lisreg_ctx* ctx, int slot, const void* cloud, int n, int stride_bytes, int fmt,
                           const lisreg_ndt_params* params, lisreg_ndt_info* info);
/* align(): guess = row-major 4x4 or NULL for identity; aligned_out: NULL, or room for n points of the input layout.  Host PCL
 * structs or LISREG_FMT_DEVICE records.  params->resolution must be the slot's.  A source without a pair at the guess returns
 * converged = 1, iters = 0 and the guess. */
int  lisreg_ndt_align(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                      const lisreg_ndt_params* params, const float* guess, lisreg_ndt_result* result, void* aligned_out);
/* test hooks: the valid voxels of a slot in ascending cell order (cell id = i + j * dims[0] + k * dims[0] * dims[1]; means [3],
 * icov6 = xx, xy, xz, yy, yz, zz of the inverse covariance; *n_out = their number, copied only if it fits `capacity`), and one
 * evaluation at p: out[28] = score, gradient [6], upper triangle of the Hessian row by row [21] (zeros without with_hessian) */
int  lisreg_ndt_get_voxels(lisreg_ctx* ctx, int slot, int* cell_ids, int* counts, double* means, double* icov6, int capacity,
                           int* n_out);
int  lisreg_ndt_derivatives(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                            const lisreg_ndt_params* params, const double p[6], int with_hessian, double out[28],
                            long long* n_pairs);

/* ---- §7o: NDT verification of a candidate list as one call ----------------------------------------------------------------------
 * The candidate loop of detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) with the verifier the reference
 * names first (select_registration_method("NDT"), src/core/registration.cpp:147-155): lisreg_ndt_align_batch is
 * lisreg_vgicp_align_batch (§7n, below) read for NDT.  Item k aligns sources[items[k].source] against the target of NDT slot
 * items[k].slot from items[k].guess, and results[k] is what lisreg_ndt_align returns for the same arguments alone, to the bit, in
 * every field; trans_probability keeps dividing by the source's record count, NaN records included.  A source is staged (uploaded)
 * once per call however many items name it; a source no item names is neither checked nor read, and its pointer may be NULL.  The
 * Newton loops of all items, each with its More-Thuente line search, advance in lockstep rounds: every unfinished item has exactly
 * one evaluation outstanding, and one round answers them all with two evaluation launches (the items that want the Hessian, those
 * that do not), one launch of fixed-order totals, one copy and one synchronisation; info->n_rounds is the largest n_evals of the items.
 * fitness (may be NULL: no fitness pass, best = -1): fitness[k] = the mean, over the FINITE points of the source, of the squared
 * distance to the nearest finite target point at the pose of results[k] — x' = ((R0 a0 + R1 a1) + R2 a2) + t and
 * ((dx dx + dy dy) + dz dz) in double from the float coordinates as §7l's search defines it, ties to the lower index, without a
 * cut-off (PCL's getFitnessScore() default), for every item, converged or not; two calls give the same bits.  The transform is the one
 * the evaluations use, R and t of the pose results[k].p in double (x' = Rx(a) Ry(b) Rz(c) x + t, true trigonometry), NOT the float
 * final_transform.  A source without a finite point has the score 0 / 0.  The search runs over the grid lisreg_ndt_set_target keeps
 * with the slot.
 * info->best: the best score starts at DBL_MAX; the items are walked in order, an item with converged == 0 or fitness > the best so
 * far is skipped, any other one is taken (:2834-2840; equal scores go to the later item); -1 if none converged.  The DEFINITION is
 * tests/ndt_batch_ref.py.
 * Refused (LISREG_ERR_ARG) for the whole batch, with `results` and `fitness` untouched: NULL items / results / sources / n with
 * n_items > 0, a source index outside 0 .. n_sources - 1, a slot without an NDT target, params lisreg_ndt_align refuses (among them
 * a params->resolution that differs from ANY named slot's), a NAMED source it refuses (n <= 0, a NULL cloud, a short stride), and a
 * batch of more than INT_MAX / 29 wavefronts (items x source records / 64).  Nothing a single call accepts is refused: a source may
 * hold NaN records and needs no minimum point count.  n_items == 0 is LISREG_OK with best = -1.  All sources of a call share
 * stride_bytes and fmt (host PCL structs or LISREG_FMT_DEVICE records).  Device memory the batch keeps (grow-only): 16 bytes per
 * source record, 232 per (item, 64 source records), about 0.8 KB per item.  No per-item aligned_out and no per-item params. */
typedef struct lisreg_ndt_item {
    int          source;   /* index into sources[] */
    int          slot;     /* lisreg_ndt_set_target(slot) */
    const float* guess;    /* row-major 4x4, NULL = identity */
} lisreg_ndt_item;
typedef struct lisreg_ndt_batch_info {
    int best;              /* -1 if no item converged (or fitness == NULL) */
    int n_rounds;          /* host round trips of the alignment phase = the largest n_evals of the items */
    int n_sources_staged;  /* sources actually uploaded */
    int reserved;
} lisreg_ndt_batch_info;
int  lisreg_ndt_align_batch(lisreg_ctx* ctx, const void* const* sources, const int* n, int n_sources, int stride_bytes, int fmt,
                            const lisreg_ndt_item* items, int n_items, const lisreg_ndt_params* params,
                            lisreg_ndt_result* results, double* fitness, lisreg_ndt_batch_info* info);

/* ---- §7v: the NDT targets of a whole candidate list as one call ------------------------------------------------------------------
 * detectLoopClosureForSubMap sets a different target submap for every candidate (src/node/subMapOptmizationNode.cpp:2793).  The slot
 * of every job that comes back with status == LISREG_OK is, in every byte a later call can observe (dims, min_b, resolution, the voxel
 * records of ALL voxels in ascending cell id with their cell ids and flags — those that did not become a Gaussian included —, their
 * number as the table counts them, the occupied and the valid voxels, the dense table with the voxel numbers it holds, the bounding
 * box, the search grid's geometry, points by cell and cells' starts), what
 * lisreg_ndt_set_target(ctx, slot, cloud, n, 16, LISREG_FMT_DEVICE, params, &info) leaves for that cloud alone.  resolution,
 * min_points_per_voxel and min_covar_eigvalue_mult of `params` apply to all jobs.  The clouds are device records, read where they lie.
 * The number of launches and of host synchronisations (two: one read-back of every target's finite count and bounding box, one at the
 * end, with every target's three counts: voxel records, occupied, valid) does not depend on n_targets; the call runs on the context's
 * stream and has returned when the slots are complete.
 * A target with an infinite coordinate, without a finite coordinate box, with a finite box but no record finite in all three
 * coordinates, with a voxel grid of more than 2^26 cells or without a valid voxel fails alone: status = LISREG_ERR_ARG (the last kind
 * with `info` filled as the single call fills it before it refuses, n_valid == 0), its slot holds no target afterwards (whatever it
 * held before), every other target is unaffected, the call returns LISREG_OK and lisreg_last_error names the first such job with the
 * single call's text ("ndt_set_target_batch: job <t>: ndt_set_target: <text>").
 * Refused for the whole call (LISREG_ERR_ARG) before anything is launched, with no slot and no job field touched: NULL jobs with
 * n_targets > 0, params lisreg_ndt_set_target refuses, a slot outside 0 .. 65535, a slot named twice, n <= 0 or a NULL cloud in any
 * job, n_targets outside 0 .. LISREG_NDT_TARGET_BATCH_MAX, more than LISREG_NDT_TARGET_BATCH_MAX_POINTS records in all.
 * n_targets == 0 is LISREG_OK. */
#define LISREG_NDT_TARGET_BATCH_MAX 1024
#define LISREG_NDT_TARGET_BATCH_MAX_POINTS 134217728          /* 2^27 */
typedef struct lisreg_ndt_target_job {
    int         slot;        /* NDT slot 0 .. 65535 */
    int         n;           /* records in cloud */
    const void* cloud;       /* DEVICE lisreg_dpoint records (LISREG_FMT_DEVICE) */
    int         status;      /* out: LISREG_OK, or LISREG_ERR_ARG for this target alone */
    lisreg_ndt_info info;    /* out: what the single call writes to *info */
} lisreg_ndt_target_job;
int  lisreg_ndt_set_target_batch(lisreg_ctx* ctx, int n_targets, lisreg_ndt_target_job* jobs, const lisreg_ndt_params* params);
/* test hook: reads a slot back, whoever set it: info; voxel_dims [3], voxel_min_b [3] and *resolution = the voxel grid; geom = the
 * search grid's origin x y z, cell edge, its inverse, the bounding box [6]; grid_dims [3] = the search grid's cells per axis;
 * *n_points = the finite points; *n_records = the voxel records (every voxel that holds a record of the cloud: a NaN record sits in
 * cell 0, so this may be one more than info->n_voxels); sorted_xyzw [n_points][4] = the finite points by search-grid cell, ascending
 * index inside a cell, the fourth word the point's index among the finite points as int bits; cell_start [grid cells + 1]; table
 * [voxel cells] = cell -> voxel record, -1 none (valid voxels only); record_cells / record_flags [n_records] = every record's cell
 * id and whether it became a Gaussian; records [n_records][10] = mean [3], inverse covariance xx xy xz yy yz zz, finite points.  Any
 * output pointer may be NULL.  A slot without a target, capacity_points < n_points with sorted_xyzw wanted, capacity_cells < grid
 * cells + 1 with cell_start wanted, capacity_table < voxel cells with table wanted or capacity_records < n_records with any of the
 * three record outputs wanted: LISREG_ERR_ARG (info, the voxel grid, geom and the two numbers are filled all the same when the slot
 * holds a target). */
int  lisreg_ndt_get_target(lisreg_ctx* ctx, int slot, lisreg_ndt_info* info, int voxel_dims[3], int voxel_min_b[3],
                           double* resolution, float geom[11], int grid_dims[3], int* n_points, int* n_records, float* sorted_xyzw,
                           int* cell_start, int* table, int* record_cells, int* record_flags, double* records, int capacity_points,
                           int capacity_cells, int capacity_table, int capacity_records);
/* what the last lisreg_ndt_set_target_batch of this context enqueued (its kernel launches, table copies and the two clears, one more
 * for every further sort sequence of the search grids, and the launches of the scans) and how often it waited for the stream */
int  lisreg_ndt_target_batch_counts(const lisreg_ctx* ctx, int* enqueues, int* synchronisations);

/* ---- §7k: voxelised GICP registration (loop-closure verification) ----------------------------------------------------
 * select_registration_method("FAST_VGICP") is the verifier detectLoopClosureForSubMap's authors chose last
 * (src/node/subMapOptmizationNode.cpp:2771, commented out); src/core/registration.cpp:156-187 carries the whole fast_gicp family
 * as a comment because it would not link.  The method (Koide et al. 2021): every point of either cloud gets a distribution from
 * its k nearest points within its own cloud, regularised to a plane (eigenvalues 1, 1, plane_epsilon); the target is cut into
 * voxels of edge `resolution` holding the mean of their points and of their points' covariances; a source point x' = R a + t with
 * the cell f = floor(x' / resolution) - grid origin is paired with every voxel among the cells f + o of its neighbourhood
 * (neighbor_search, the last int of params, §7w: DIRECT1 o = (0, 0, 0), the voxel it falls into; DIRECT7 the offsets in {-1, 0, 1}^3 with
 * |dx| + |dy| + |dz| <= 1; DIRECT27 all of them; every offset is tested against the grid on its own, so a point one cell outside
 * the grid still pairs with the voxels inside; the offsets are walked in ascending cell id) and a Levenberg-Marquardt loop minimises
 * the sum of sqrt(N) d^T (C_voxel + R C_a R^T)^-1 d over the pairs; n_pairs counts pairs, not points.  The neighbourhood belongs to
 * the alignment: a slot serves all three, and the calls that only build or read a target check the field and otherwise ignore it.
 * The DEFINITION is tests/vgicp_ref.py with the pairing of tests/vgicp_nb_ref.py (fast_gicp's source is not available to this
 * project); DESIGN.md §7k and §7w list where it picks a reading of fast_gicp it cannot verify.  NaN points are no points: never a
 * neighbour, in no voxel, in no pair.
 * The GPU makes the distributions (an exact k-nearest search, one query per lane), the voxel statistics and every linearisation
 * (fp64, fixed-order sums: two evaluations of the same input give the same bits); the 6 x 6 solve and the LM loop run on the host in
 * double.  A single alignment has no fitness score (a caller who wants one has aligned_out and lisreg_nearest); the batch form below
 * (§7n) computes one per item. */
/* neighbor_search, fast_gicp's setNeighborSearchMethod: the last int of lisreg_vgicp_params.  The struct member keeps the name it had
 * while it was unused, `reserved` (tests/test_vgicp_ref.py compares the member names of the struct with the Python mirror's, whose
 * list of fields is pinned by the same file); the C++ mirror's setNeighborSearchMethod and the Python mirror's neighbor_search property
 * write it.  0 means DIRECT1 (what lisreg_vgicp_default_params writes, and a zero-initialised struct); any other value than these is
 * refused (LISREG_ERR_ARG) by every lisreg_vgicp_* call that takes params */
#define LISREG_VGICP_DIRECT1  1
#define LISREG_VGICP_DIRECT7  7
#define LISREG_VGICP_DIRECT27 27
typedef struct lisreg_vgicp_params {
    double resolution;                  /* voxel edge */
    double transformation_epsilon;      /* a step is converged when max|exp(delta).t| is below this ... */
    double rotation_epsilon;            /* ... and max|exp(delta).R - I| below this */
    double lm_init_lambda_factor;       /* lambda starts at this times max|diag H| of the first linearisation */
    double plane_epsilon;               /* the smallest eigenvalue of a regularised covariance */
    int    k_correspondences;           /* points per distribution, 4 .. 32 */
    int    max_iters;                   /* outer iterations (linearisations) */
    int    lm_max_iterations;           /* trials per outer iteration */
    int    reserved;                    /* neighbor_search: 0 or LISREG_VGICP_DIRECT1, LISREG_VGICP_DIRECT7, LISREG_VGICP_DIRECT27 (§7w) */
} lisreg_vgicp_params;
typedef struct lisreg_vgicp_info {
    int dims[3];                        /* voxel grid of the target */
    int n_voxels;                       /* voxels holding at least one point */
    int n_points;                       /* finite points of the target */
} lisreg_vgicp_info;
typedef struct lisreg_vgicp_result {
    double final_transform[16];         /* row-major 4x4, in double: the steps are far below a float's resolution of a map coordinate */
    int    converged;
    int    iters;                       /* outer iterations */
    int    n_evals;                     /* evaluations of the error (with or without H) */
    int    n_rejected;                  /* trials whose step was rejected */
    long long n_pairs_last;             /* (source point, voxel) pairs of the last evaluation */
    double error;                       /* at final_transform */
    double lambda;                      /* the damping the loop ended with */
} lisreg_vgicp_result;
/* kind 0 (the reference's commented FAST_VGICP block + fast_gicp's defaults as remembered): {1.0, 0.01, 2e-3, 1e-9, 1e-3, 20, 50, 10} */
int  lisreg_vgicp_default_params(int kind, lisreg_vgicp_params* p);
/* The distributions and voxel statistics of `cloud` into VGICP slot `slot` (0 .. 65535; VGICP slots are apart from the map-index
 * and the NDT slots).  Uses resolution, k_correspondences and plane_epsilon of `params`.  Refused (LISREG_ERR_ARG): n <= 0, fewer
 * finite points than k_correspondences, an infinite coordinate, resolution <= 0, k_correspondences outside 4 .. 32, a grid of more
 * than 2^26 cells (the voxel table is dense).  info may be NULL.  Besides the voxels the slot keeps the search grid its distributions
 * were made with, for the fitness score of lisreg_vgicp_align_batch: 16 bytes per finite point and 4 per grid cell (3.2 MB for a
 * target of 200 000 points). */
int  lisreg_vgicp_set_target(lisreg_ctx* ctx, int slot, const void* cloud, int n, int stride_bytes, int fmt,
                             const lisreg_vgicp_params* params, lisreg_vgicp_info* info);
/* guess = row-major 4x4 or NULL for identity; aligned_out: NULL, or room for n points of the input layout (the source under
 * final_transform rounded to float).  Host PCL structs or LISREG_FMT_DEVICE records.  params->resolution must be the slot's, and the
 * slot must hold a target (LISREG_ERR_ARG otherwise).  The source's distributions are made by every call; a source with fewer finite
 * points than k_correspondences is refused.  A source without a pair at the guess returns converged = 0, iters = 0 and the guess. */
int  lisreg_vgicp_align(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                        const lisreg_vgicp_params* params, const float* guess, lisreg_vgicp_result* result, void* aligned_out);
/* test hooks.  _covariances: the distribution of every point of a cloud — cov6_out [n][6] = xx, xy, xz, yy, yz, zz (NaN rows for
 * NaN points), neighbours_out [n][k] (may be NULL) = the k nearest points' indices by ascending (distance, index), -1 rows for NaN
 * points; plane_epsilon is 1e-3; cell_edge > 0 forces the cell edge of the search grid (0: chosen from the cloud's density) — the
 * results do not depend on it.  _get_voxels: the voxels of a slot in ascending cell order (cell id = i + j * dims[0] + k * dims[0] *
 * dims[1]; means [3], cov6 of the mean covariance; *n_out = their number, copied only if it fits `capacity`).  _linearize: one
 * linearisation at T (row-major 4x4): out[28] = error, b [6], upper triangle of H row by row [21] (zeros without with_hessian). */
int  lisreg_vgicp_covariances(lisreg_ctx* ctx, const void* cloud, int n, int stride_bytes, int fmt, int k, double* cov6_out,
                              int* neighbours_out, float cell_edge);
int  lisreg_vgicp_get_voxels(lisreg_ctx* ctx, int slot, int* cell_ids, int* counts, double* means, double* cov6, int capacity,
                             int* n_out);
int  lisreg_vgicp_linearize(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                            const lisreg_vgicp_params* params, const double T[16], int with_hessian, double out[28],
                            long long* n_pairs);
/* §7u: the targets of a whole candidate list as one call (detectLoopClosureForSubMap sets a different target submap for every
 * candidate, src/node/subMapOptmizationNode.cpp:2793).  The slot of every job that comes back with status == LISREG_OK is, in every
 * byte a later call can observe (dims, min_b, resolution, n_voxels, n_points, the voxel records in ascending cell id with their cell
 * ids, the dense table, the bounding box, the search grid's geometry, points by cell and cells' starts), what
 * lisreg_vgicp_set_target(ctx, slot, cloud, n, 16, LISREG_FMT_DEVICE, params, &info) leaves for that cloud alone.  resolution,
 * k_correspondences and plane_epsilon of `params` apply to all jobs.  The clouds are device records, read where they lie.  The number
 * of launches and of host synchronisations (two: one read-back of every target's finite count and bounding box, one at the end, with
 * the voxel counts) does not depend on n_targets; the call runs on the context's stream and has returned when the slots are complete.
 * A target with an infinite coordinate, with fewer finite points than k_correspondences or an empty finite box, or with a voxel grid
 * of more than 2^26 cells fails alone: status = LISREG_ERR_ARG, its slot holds no target afterwards (whatever it held before), every
 * other target is unaffected, the call returns LISREG_OK and lisreg_last_error names the first such job with the single call's text.
 * Refused for the whole call (LISREG_ERR_ARG) before anything is launched, with no slot and no job field touched: NULL jobs with
 * n_targets > 0, params lisreg_vgicp_set_target refuses, a slot outside 0 .. 65535, a slot named twice, n <= 0 or a NULL cloud in any
 * job, n_targets outside 0 .. LISREG_VGICP_TARGET_BATCH_MAX, more than LISREG_VGICP_TARGET_BATCH_MAX_POINTS records in all.
 * n_targets == 0 is LISREG_OK. */
#define LISREG_VGICP_TARGET_BATCH_MAX 1024
#define LISREG_VGICP_TARGET_BATCH_MAX_POINTS 134217728          /* 2^27 */
typedef struct lisreg_vgicp_target_job {
    int         slot;        /* VGICP slot 0 .. 65535 */
    int         n;           /* records in cloud */
    const void* cloud;       /* DEVICE lisreg_dpoint records (LISREG_FMT_DEVICE) */
    int         status;      /* out: LISREG_OK, or LISREG_ERR_ARG for this target alone */
    lisreg_vgicp_info info;  /* out: what the single call writes to *info */
} lisreg_vgicp_target_job;
int  lisreg_vgicp_set_target_batch(lisreg_ctx* ctx, int n_targets, lisreg_vgicp_target_job* jobs,
                                   const lisreg_vgicp_params* params);
/* test hook: reads a slot back, whoever set it: info; voxel_dims [3], voxel_min_b [3] and *resolution = the voxel grid; geom = the
 * search grid's origin x y z, cell edge, its inverse, the bounding box [6]; grid_dims [3] = the search grid's cells per axis;
 * sorted_xyzw [n_points][4] = the finite points by search-grid cell, ascending index inside a cell, the fourth word the point's index
 * among the finite points as int bits; cell_start [grid cells + 1]; table [voxel cells] = cell -> voxel, -1 none.  (The voxel
 * records: lisreg_vgicp_get_voxels.)  Any output pointer may be NULL.  A slot without a target, capacity_points < n_points with sorted_xyzw wanted, capacity_cells < grid cells + 1 with
 * cell_start wanted or capacity_table < voxel cells with table wanted: LISREG_ERR_ARG (info, the voxel grid and geom are filled all the
 * same when the slot holds a target). */
int  lisreg_vgicp_get_target(lisreg_ctx* ctx, int slot, lisreg_vgicp_info* info, int voxel_dims[3], int voxel_min_b[3],
                             double* resolution, float geom[11], int grid_dims[3], float* sorted_xyzw, int* cell_start, int* table,
                             int capacity_points, int capacity_cells, int capacity_table);
/* what the last lisreg_vgicp_set_target_batch of this context enqueued (its kernel launches, table copies and the one histogram
 * clear, one more for every further sort sequence of the search grids, and the launches of the scans) and how often it waited for
 * the stream */
int  lisreg_vgicp_target_batch_counts(const lisreg_ctx* ctx, int* enqueues, int* synchronisations);

/* ---- §7n: VGICP verification of a candidate list as one call -------------------------------------------------------------------
 * The candidate loop of detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) with the verifier its authors
 * wrote down last (select_registration_method("FAST_VGICP"), :2771): lisreg_vgicp_align_batch is lisreg_fgicp_align_batch (§7m, below)
 * read for VGICP.  Item k aligns sources[items[k].source] against the target of VGICP slot items[k].slot from items[k].guess, and
 * results[k] is what lisreg_vgicp_align returns for the same arguments alone, to the bit, in every field.  The distributions of a
 * source are made once per call however many items name it; a source no item names is neither checked nor staged.  The
 * Levenberg-Marquardt loops of all items advance in lockstep rounds: one round answers the outstanding evaluation of every unfinished
 * item with two linearisation launches (the items that want the Hessian, the error evaluations), one launch of fixed-order totals,
 * one copy and one synchronisation; info->n_rounds is the largest n_evals of the items.
 * fitness (may be NULL: no fitness pass, best = -1): fitness[k] = the mean, over the finite source points, of the squared distance to
 * the nearest finite target point at results[k].final_transform — x' = ((R0 a0 + R1 a1) + R2 a2) + t and ((dx dx + dy dy) + dz dz) in
 * double from the float coordinates as §7l's search defines it, ties to the lower index, without a cut-off (PCL's getFitnessScore()
 * default), for every item, converged or not; two calls give the same bits.  The search runs over the grid lisreg_vgicp_set_target
 * keeps with the slot.
 * info->best: the best score starts at DBL_MAX; the items are walked in order, an item with converged == 0 or fitness > the best so
 * far is skipped, any other one is taken (:2834-2840; equal scores go to the later item); -1 if none converged.  The DEFINITION is
 * tests/vgicp_batch_ref.py.
 * Refused (LISREG_ERR_ARG) for the whole batch, with `results` and `fitness` untouched: NULL items / results / sources / n with
 * n_items > 0, a source index outside 0 .. n_sources - 1, a slot without a target, params lisreg_vgicp_align refuses (among them a
 * params->resolution that differs from ANY named slot's), a NAMED source it refuses (n <= 0, a NULL cloud, a short stride, an infinite
 * coordinate, fewer finite points than k_correspondences; the last two are found while the distributions are made, before any
 * alignment work), and a batch of more than INT_MAX / 29 wavefronts (items x source points / 64).  n_items == 0 is LISREG_OK with
 * best = -1.  All sources of a call share stride_bytes and fmt (host PCL structs or LISREG_FMT_DEVICE records).  Device memory the
 * batch keeps (grow-only): 64 bytes per finite source point, 232 per (item, 64 source points).  No per-item aligned_out and no
 * per-item params. */
typedef struct lisreg_vgicp_item {
    int          source;   /* index into sources[] */
    int          slot;     /* lisreg_vgicp_set_target(slot) */
    const float* guess;    /* row-major 4x4, NULL = identity */
} lisreg_vgicp_item;
typedef struct lisreg_vgicp_batch_info {
    int best;              /* -1 if no item converged (or fitness == NULL) */
    int n_rounds;          /* host round trips of the LM phase = the largest n_evals of the items */
    int n_sources_staged;  /* distributions actually computed */
    int reserved;
} lisreg_vgicp_batch_info;
int  lisreg_vgicp_align_batch(lisreg_ctx* ctx, const void* const* sources, const int* n, int n_sources, int stride_bytes, int fmt,
                              const lisreg_vgicp_item* items, int n_items, const lisreg_vgicp_params* params,
                              lisreg_vgicp_result* results, double* fitness, lisreg_vgicp_batch_info* info);

/* ---- §7l: FastGICP registration (loop-closure verification) --------------------------------------------------------------
 * select_registration_method("FAST_GICP") (src/core/registration.cpp:157-166: FastGICP, transformation epsilon 0.01, 50 iterations,
 * max correspondence distance 5, correspondence randomness 20) is the other verifier of the fast_gicp family that
 * detectLoopClosureForSubMap's call (src/node/subMapOptmizationNode.cpp:2771) can name.  The method: every point of either cloud
 * gets the distribution of §7k; at every linearisation each transformed source point is paired with its NEAREST target point — an
 * exact search, squared distances in double from the float coordinates, ties to the lower index — if that point is nearer than
 * max_correspondence_distance (strictly), and a Levenberg-Marquardt loop (§7k's) minimises the sum of d^T (C_b + R C_a R^T)^-1 d over
 * the pairs.  An error evaluation inside the loop reuses the pairs and the matrices of the last linearisation.  The DEFINITION is
 * tests/fgicp_ref.py (fast_gicp's source is not available to this project); DESIGN.md §7l lists where it picks a reading of fast_gicp
 * it cannot verify.  NaN points are no points: never a neighbour, never a correspondent, in no pair.  The GPU makes the distributions,
 * every search (one query per lane over the target's search grid, fp64) and every sum (fixed order: two evaluations of the same input
 * give the same bits); the 6 x 6 solve and the LM loop run on the host in double.  A single alignment has no fitness score (a caller
 * who wants one has aligned_out and lisreg_nearest); the batch form below (§7m) computes one per item. */
typedef struct lisreg_fgicp_params {
    double max_correspondence_distance; /* a nearest point this far away or further is no pair */
    double transformation_epsilon;      /* a step is converged when max|exp(delta).t| is below this ... */
    double rotation_epsilon;            /* ... and max|exp(delta).R - I| below this */
    double lm_init_lambda_factor;       /* lambda starts at this times max|diag H| of the first linearisation */
    double plane_epsilon;               /* the smallest eigenvalue of a regularised covariance */
    int    k_correspondences;           /* points per distribution ("correspondence randomness"), 4 .. 32 */
    int    max_iters;                   /* outer iterations (linearisations) */
    int    lm_max_iterations;           /* trials per outer iteration */
    int    reserved;
} lisreg_fgicp_params;
typedef struct lisreg_fgicp_info {
    int grid_dims[3];                   /* cells of the target's search grid */
    int n_points;                       /* finite points of the target */
} lisreg_fgicp_info;
typedef struct lisreg_fgicp_result {
    double final_transform[16];         /* row-major 4x4, in double */
    int    converged;
    int    iters;                       /* outer iterations */
    int    n_evals;                     /* evaluations of the error (with or without H) */
    int    n_rejected;                  /* trials whose step was rejected */
    long long n_pairs_last;             /* pairs of the last linearisation */
    double error;                       /* at final_transform, over the pairs of the last linearisation */
    double lambda;                      /* the damping the loop ended with */
} lisreg_fgicp_result;
/* kind 0 (the reference's commented FAST_GICP block + fast_gicp's defaults as remembered): {5.0, 0.01, 2e-3, 1e-9, 1e-3, 20, 50, 10};
 * kind 1: the same with max_correspondence_distance = FLT_MAX, fast_gicp's own default (no cut-off) */
int  lisreg_fgicp_default_params(int kind, lisreg_fgicp_params* p);
/* The distributions and the search grid of `cloud` into FastGICP slot `slot` (0 .. 65535; FastGICP slots are a numbering of their
 * own, apart from the map-index, the NDT and the VGICP slots).  Uses k_correspondences and plane_epsilon of `params`.  Refused
 * (LISREG_ERR_ARG): n <= 0, fewer finite points than k_correspondences, an infinite coordinate, k_correspondences outside 4 .. 32,
 * max_correspondence_distance <= 0 or NaN.  info may be NULL.  cell_edge 0: the search grid's cell edge is chosen from the cloud's
 * density; > 0 forces it: results do not depend on it. */
int  lisreg_fgicp_set_target(lisreg_ctx* ctx, int slot, const void* cloud, int n, int stride_bytes, int fmt,
                             const lisreg_fgicp_params* params, lisreg_fgicp_info* info, float cell_edge);
/* §7t: the targets of a whole candidate list as one call (detectLoopClosureForSubMap sets a different target submap for every
 * candidate, src/node/subMapOptmizationNode.cpp:2793).  The slot of every job that comes back with status == LISREG_OK is, in every
 * byte a later call can observe (the grid's geometry and dims, the bounding box, the points by cell, the cells' starts, the indices in
 * the caller's cloud, the m x 6 covariances), what lisreg_fgicp_set_target(ctx, slot, cloud, n, 16, LISREG_FMT_DEVICE, params, &info,
 * cell_edge) leaves for that cloud alone.  The clouds are device records, read where they lie.  The number of launches and of host
 * synchronisations (two: one read-back of every target's finite count and bounding box, one at the end) does not depend on
 * n_targets; the call runs on the context's stream and has returned when the slots are complete.
 * A target with fewer finite points than k_correspondences, with an infinite coordinate or with an empty finite box fails alone:
 * status = LISREG_ERR_ARG, its slot holds no target afterwards (whatever it held before), every other target is unaffected, the call
 * returns LISREG_OK and lisreg_last_error names the first such job with the single call's text.
 * Refused for the whole call (LISREG_ERR_ARG) before anything is launched, with no slot and no job field touched: NULL jobs with
 * n_targets > 0, params lisreg_fgicp_set_target refuses, a slot outside 0 .. 65535, a slot named twice, n <= 0, a NULL cloud or a
 * cell_edge that is negative or not finite in any job, n_targets outside 0 .. LISREG_FGICP_TARGET_BATCH_MAX, more than
 * LISREG_FGICP_TARGET_BATCH_MAX_POINTS records in all.  n_targets == 0 is LISREG_OK. */
#define LISREG_FGICP_TARGET_BATCH_MAX 1024
#define LISREG_FGICP_TARGET_BATCH_MAX_POINTS 134217728          /* 2^27 */
typedef struct lisreg_fgicp_target_job {
    int         slot;        /* FastGICP slot 0 .. 65535 */
    int         n;           /* records in cloud */
    const void* cloud;       /* DEVICE lisreg_dpoint records (LISREG_FMT_DEVICE) */
    float       cell_edge;   /* as the single call's: 0 = from the density, > 0 forced */
    int         status;      /* out: LISREG_OK, or LISREG_ERR_ARG for this target alone */
    lisreg_fgicp_info info;  /* out: what the single call writes to *info */
} lisreg_fgicp_target_job;
int  lisreg_fgicp_set_target_batch(lisreg_ctx* ctx, int n_targets, lisreg_fgicp_target_job* jobs,
                                   const lisreg_fgicp_params* params);
/* test hooks.  _get_target reads a slot back, whoever set it: info; geom = the grid's origin x y z, cell edge, its inverse, the
 * bounding box [6]; sorted_xyzw [n_points][4] = the finite points by grid cell, ascending index inside a cell, the fourth word the
 * point's index among the finite points as int bits; cell_start [cells + 1]; orig [n_points] = index among the finite points -> index
 * in the caller's cloud; cov6 [n_points][6] by index among the finite points.  Any output pointer may be NULL.  A slot without a target,
 * capacity_points < n_points with a per-point output wanted or capacity_cells < cells + 1 with cell_start wanted: LISREG_ERR_ARG (info
 * and geom are filled all the same when the slot holds a target).  _grid_geometry: the search grid lisreg_fgicp_set_target[_batch]
 * chooses for n_points finite points in the finite box bb (min x y z, max x y z) under cell_edge — dims [3], cell = {edge, 1 / edge};
 * host arithmetic only, no device. */
int  lisreg_fgicp_get_target(lisreg_ctx* ctx, int slot, lisreg_fgicp_info* info, float geom[11], float* sorted_xyzw, int* cell_start,
                             int* orig, double* cov6, int capacity_points, int capacity_cells);
int  lisreg_fgicp_grid_geometry(const float bb[6], int n_points, float cell_edge, int dims[3], float cell[2]);
/* what the last lisreg_fgicp_set_target_batch of this context enqueued (its kernel launches and table copies, and one for every sort
 * sequence) and how often it waited for the stream */
int  lisreg_fgicp_target_batch_counts(const lisreg_ctx* ctx, int* enqueues, int* synchronisations);
/* guess = row-major 4x4 or NULL for identity; aligned_out: NULL, or room for n points of the input layout (the source under
 * final_transform rounded to float).  Host PCL structs or LISREG_FMT_DEVICE records.  The slot must hold a target (LISREG_ERR_ARG
 * otherwise).  The source's distributions are made by every call; a source with fewer finite points than k_correspondences is
 * refused.  A source without a pair at the guess returns converged = 0, iters = 0, n_evals = 1 and the guess. */
int  lisreg_fgicp_align(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                        const lisreg_fgicp_params* params, const float* guess, lisreg_fgicp_result* result, void* aligned_out);
/* test hooks.  _correspondences: the search at T (row-major 4x4) — index_out [n] = the correspondent's index in the caller's target
 * cloud, -1 for a source point without one or a NaN point; sqdist_out [n] (may be NULL) = its squared distance, NaN where -1.
 * _linearize: pairs and their matrices from a search at T_pairs, then out[28] = error, b [6], upper triangle of H row by row [21]
 * (zeros without with_hessian) at T_eval (NULL: T_pairs) — the reuse of the pairs by an error evaluation, as one call. */
int  lisreg_fgicp_correspondences(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                                  const lisreg_fgicp_params* params, const double T[16], int* index_out, double* sqdist_out);
int  lisreg_fgicp_linearize(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                            const lisreg_fgicp_params* params, const double T_pairs[16], const double* T_eval, int with_hessian,
                            double out[28], long long* n_pairs);

/* ---- §7m: FastGICP verification of a candidate list as one call ---------------------------------------------------------------
 * The candidate loop of detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) aligns one key-frame cloud against
 * every candidate submap from that candidate's initial pose and keeps the candidate with the lowest getFitnessScore() among those
 * that hasConverged().  lisreg_fgicp_align_batch runs that loop as one call: item k aligns sources[items[k].source] against the
 * target of FastGICP slot items[k].slot from items[k].guess, and results[k] is what lisreg_fgicp_align returns for the same
 * arguments alone, to the bit, in every field.  The distributions of a source are made once per call however many items name it; a
 * source no item names is neither checked nor staged.  The Levenberg-Marquardt loops of all items advance in lockstep rounds: one
 * round answers the outstanding evaluation of every unfinished item with one search launch (the items that linearise), two sum
 * launches, one launch of fixed-order totals, one copy and one synchronisation; info->n_rounds is the largest n_evals of the items.
 * fitness (may be NULL: no fitness pass, best = -1): fitness[k] = the mean, over the finite source points, of the squared distance to
 * the nearest finite target point at results[k].final_transform — in double from the float coordinates as §7l's search defines it,
 * without a cut-off (PCL's getFitnessScore() default), for every item, converged or not; two calls give the same bits.
 * info->best: the items are walked in order, an item with converged == 0 or fitness > the best so far is skipped, any other one is
 * taken (:2834-2840; equal scores go to the later item); -1 if none converged.  The DEFINITION is tests/fgicp_batch_ref.py.
 * Refused (LISREG_ERR_ARG) for the whole batch, with `results` untouched: NULL items / results / sources / n with n_items > 0, a
 * source index outside 0 .. n_sources - 1, a slot without a target, params lisreg_fgicp_align refuses, and a NAMED source it
 * refuses (n <= 0, a NULL cloud, a short stride, an infinite coordinate, fewer finite points than k_correspondences; the last two
 * are found while the distributions are made, before any alignment work).  n_items == 0 is LISREG_OK with best = -1.  All sources of
 * a call share stride_bytes and fmt (host PCL structs or LISREG_FMT_DEVICE records).  Device memory the batch keeps (grow-only):
 * 52 bytes per (item, finite source point) for the pairs and their matrices, 64 per finite source point.  No per-item aligned_out
 * and no per-item params. */
typedef struct lisreg_fgicp_item {
    int          source;   /* index into sources[] */
    int          slot;     /* lisreg_fgicp_set_target(slot) */
    const float* guess;    /* row-major 4x4, NULL = identity */
} lisreg_fgicp_item;
typedef struct lisreg_fgicp_batch_info {
    int best;              /* see above; -1 if no item converged */
    int n_rounds;          /* host round trips of the LM phase */
    int n_sources_staged;  /* distributions actually computed */
    int reserved;
} lisreg_fgicp_batch_info;
int  lisreg_fgicp_align_batch(lisreg_ctx* ctx, const void* const* sources, const int* n, int n_sources, int stride_bytes, int fmt,
                              const lisreg_fgicp_item* items, int n_items, const lisreg_fgicp_params* params,
                              lisreg_fgicp_result* results, double* fitness, lisreg_fgicp_batch_info* info);

/* ---- §7q: PCL's GICP registration (loop-closure verification) ---------------------------------------------------------------
 * select_registration_method("GICP") (src/core/registration.cpp:137-146: pcl::GeneralizedIterativeClosestPoint, max correspondence
 * distance 10, 30 iterations, transformation epsilon 1e-6, Euclidean fitness epsilon 1e-3, RANSAC 0) is the fifth verifier the
 * reference names.  The method: the distributions and the nearest-neighbour pairs of §7l (a GICP target IS a FastGICP slot:
 * lisreg_fgicp_set_target with plane_epsilon = gicp_epsilon); per OUTER iteration the pairs and their M = (C_b + R C_a R^T)^-1 are
 * fixed at T_k = X(x_k) guess and a BFGS with Fletcher's line search (PCL's BFGS<> = GSL's vector_bfgs2) minimises
 * f(x) = (1/m) sum (X(x) p - q)^T M (X(x) p - q) over x = (tx, ty, tz, roll, pitch, yaw), X(x) = [Rz(yaw) Ry(pitch) Rx(roll) | t].
 * With the pairs fixed f is an exact quadratic in the 12 entries of X(x): the GPU makes ONE search-and-moments launch and one launch
 * of fixed-order totals per outer iteration (74 doubles: c0, g [12], S [60], the pair count; two evaluations of the same input give
 * the same bits), and the whole inner BFGS runs on the host over those 74 doubles.  The DEFINITION is tests/gicp_ref.py (PCL's source
 * is not available to this project); DESIGN.md §7q lists the readings it picks.  Fewer than 4 pairs is PCL's "need at least 4 points":
 * converged = 0 and the pose at which that round searched.  Both ends of the outer loop (max_iters reached, delta < 1) set
 * converged = 1, as PCL 1.8 does.  No fitness score of its own (aligned_out and lisreg_nearest give one); the batch form below (§7r)
 * computes one per item. */
typedef struct lisreg_gicp_params {
    double max_correspondence_distance; /* a nearest point this far away or further is no pair */
    double transformation_epsilon;      /* delta scales the translation entries of X(x_k) - X(x_k+1) by 1 / this ... */
    double rotation_epsilon;            /* ... and the rotation entries by 1 / this; the outer loop ends when delta < 1 */
    double gicp_epsilon;                /* the smallest eigenvalue of a regularised covariance (the slot's plane_epsilon) */
    double rho, sigma;                  /* Fletcher's two tests */
    double tau1, tau2, tau3;            /* the bracket's growth and the section's two margins */
    double step_size;                   /* the first trial step of an inner minimisation */
    double gradient_tol;                /* an inner minimisation ends when |grad f| is below this */
    int    k_correspondences;           /* points per distribution, 4 .. 32 */
    int    max_iters;                   /* outer iterations, >= 1 */
    int    max_inner_iters;             /* BFGS steps per outer iteration, >= 1 */
    int    order;                       /* of the line search's interpolation: 3 (cubic) or 2 */
} lisreg_gicp_params;
typedef struct lisreg_gicp_result {
    double final_transform[16];         /* row-major 4x4, in double: X(x) guess */
    int    converged;
    int    iters;                       /* outer iterations (inner minimisations run) */
    int    inner_iters;                 /* BFGS steps, all outer iterations together */
    int    n_evals;                     /* host evaluations of f or its gradient from the moments */
    int    n_rounds;                    /* GPU round trips: == iters, or iters + 1 when the loop ended on fewer than 4 pairs */
    int    inner_exit;                  /* how the last inner loop ended: 0 gradient_tol, 1 max_inner_iters, 2 no progress; -1: none ran */
    long long n_pairs_last;             /* pairs of the last round */
    double error;                       /* f at final_transform over the pairs of the last round */
    double last_delta;                  /* delta of the last outer iteration */
} lisreg_gicp_result;
/* kind 0 (the reference's GICP block + PCL's defaults): {10, 1e-6, 2e-3, 1e-3, 0.01, 0.01, 9, 0.05, 0.5, 0.01, 1e-2, 20, 30, 20, 3};
 * kind 1: the settings of src/node/subMapOptmizationNode.cpp:2765-2769 read for GICP: transformation_epsilon 1e-4 */
int  lisreg_gicp_default_params(int kind, lisreg_gicp_params* p);
/* `slot` is a FastGICP slot (lisreg_fgicp_set_target): there is no GICP slot family.  guess, aligned_out, the source formats and the
 * refusals are lisreg_fgicp_align's; also refused: max_iters < 1, max_inner_iters < 1, rho / sigma / tau2 / tau3 outside (0, 1),
 * tau1 <= 1, step_size or gradient_tol <= 0, order outside 2 .. 3.  A refused call leaves `result` untouched. */
int  lisreg_gicp_align(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                       const lisreg_gicp_params* params, const float* guess, lisreg_gicp_result* result, void* aligned_out);
/* test hooks.  _moments: one round at T (row-major 4x4): the search, the moments about the centre of the slot's bounding box and
 * their total, out[74] in the order tests/gicp_ref.py lists.  _inner: the inner minimisation alone, from moments[74], that centre
 * and the outer iterate x0 — no device, no context, callable without a GPU; counts (may be NULL) = BFGS steps, evaluations of f,
 * evaluations of the gradient alone, inner_exit; f_out (may be NULL) = f at x_out.  Refused: a NULL pointer, fewer than 1 pair. */
int  lisreg_gicp_moments(lisreg_ctx* ctx, int slot, const void* source, int n, int stride_bytes, int fmt,
                         const lisreg_gicp_params* params, const double T[16], double out[74]);
int  lisreg_gicp_inner(const double moments[74], const double centre[3], const double x0[6], const lisreg_gicp_params* params,
                       double x_out[6], int counts[4], double* f_out);

/* ---- §7r: PCL's GICP verification of a candidate list as one call ------------------------------------------------------------
 * The candidate loop of detectLoopClosureForSubMap (src/node/subMapOptmizationNode.cpp:2779-2846) with the one verifier whose block
 * is live in select_registration_method ("GICP", src/core/registration.cpp:137-146): lisreg_gicp_align_batch is
 * lisreg_fgicp_align_batch (§7m, above) read for GICP.  Item k aligns sources[items[k].source] against the target of FastGICP slot
 * items[k].slot (a GICP target IS a FastGICP slot, §7q) from items[k].guess, and results[k] is what lisreg_gicp_align returns for the
 * same arguments alone, to the bit, in all 176 bytes.  The distributions of a source are made once per call however many items name
 * it; a source no item names is neither checked nor staged.  The outer loops of all items advance in lockstep rounds: one round
 * answers the outstanding outer iteration of every unfinished item with one search-and-moments launch, one launch of fixed-order
 * totals, one copy of 592 bytes per item and one synchronisation, and then runs the items' inner BFGS minimisations on the host one
 * after the other; info->n_rounds is the largest n_rounds of the items.
 * fitness (may be NULL: no fitness pass, best = -1): fitness[k] = the mean, over the finite source points, of the squared distance to
 * the nearest finite target point at results[k].final_transform (the double T = X(x) guess) — in double from the float coordinates as
 * §7l's search defines it, without a cut-off (PCL's getFitnessScore() default), for every item, converged or not; two calls give the
 * same bits.  info->best: the items are walked in order, an item with converged == 0 or fitness > the best so far is skipped, any
 * other one is taken (:2834-2840; equal scores go to the later item); -1 if none converged.  An item that ends on fewer than 4 pairs
 * (a guess far off) has converged = 0: `best` skips it, and it still gets a score.  The DEFINITION is tests/gicp_batch_ref.py.
 * Refused (LISREG_ERR_ARG) for the whole batch, with `results`, `fitness` and best untouched: NULL items / results / sources / n with
 * n_items > 0, n_items < 0, a source index outside 0 .. n_sources - 1, a slot without a FastGICP target, params lisreg_gicp_align
 * refuses, a NAMED source it refuses (n <= 0, a NULL cloud, a short stride, an infinite coordinate, fewer finite points than
 * k_correspondences; the last two are found while the distributions are made, before any alignment work), and a batch of more than
 * INT_MAX / 74 wavefronts (items x ceil(finite source points / 64)).  n_items == 0 is LISREG_OK with best = -1.  All sources of a
 * call share stride_bytes and fmt (host PCL structs or LISREG_FMT_DEVICE records).  Device memory the batch keeps (grow-only): 592
 * bytes per (item, wavefront of its source) for the partial records, 64 per finite source point; an item owns nothing per point.  No
 * per-item aligned_out and no per-item params. */
typedef struct lisreg_gicp_item {
    int          source;   /* index into sources[] */
    int          slot;     /* lisreg_fgicp_set_target(slot) */
    const float* guess;    /* row-major 4x4, NULL = identity */
} lisreg_gicp_item;
typedef struct lisreg_gicp_batch_info {
    int best;              /* see above; -1 if no item converged */
    int n_rounds;          /* host round trips of the alignment phase */
    int n_sources_staged;  /* distributions actually computed */
    int reserved;
} lisreg_gicp_batch_info;
int  lisreg_gicp_align_batch(lisreg_ctx* ctx, const void* const* sources, const int* n, int n_sources, int stride_bytes, int fmt,
                             const lisreg_gicp_item* items, int n_items, const lisreg_gicp_params* params,
                             lisreg_gicp_result* results, double* fitness, lisreg_gicp_batch_info* info);

/* ---- loop-closure candidate detection: FEPSC (src/core/epscGeneration.cpp) -------------------------------------------
 * EPSCGeneration::loopDetection (:663-992) with UsingFEPSCFlag (config/params.yaml:22-28), as loopClosureThread calls it for every
 * key frame (subMapOptmizationNode.cpp:2328-2362): its matched_frame_id / matched_frame_transform become loopKeyPre and the EPSC
 * init pose that seeds the verification ICP (:2796-2805, lisreg_icp_align_batch).  Per key frame: pose and travel gate (:686-745,
 * in double on the host), then on the device for every gated history frame the 1 x 360 projection yaw search + 2-D ICP (globalICP,
 * :258-401), the three current clouds moved by its result and binned into the 20 x 80 FEPSC (:478-607), the 20-shift score
 * (calculateDistance, :633-660), and the first strict maximum above the threshold.  One deliberate deviation: the yaw search wraps
 * the shifted column modulo 360 (the reference wraps once and reads past its 360-entry row for yaw shifts above 331 sectors).
 * Clouds: corner / surf LISREG_FMT_XYZI host structs, semantic LISREG_FMT_XYZIL host structs (label = the uint16 at byte 20), or
 * all three LISREG_FMT_DEVICE records (label in the payload); one format and stride per call. */
#define LISREG_LOOPDET_MAX_DB   16
#define LISREG_LOOPDET_NO_SHIFT (-2147483647 - 1)   /* yaw_shift when no shift beat the initial 100000 */
typedef struct lisreg_loopdet_params {
    double skip_neighbour_distance;     /* SKIP_NEIBOUR_DISTANCE 20: delta_travel > this */
    double inflation_covariance;        /* INFLATION_COVARIANCE 0.01: pos_distance < delta_travel * this */
    double distance_threshold;          /* DISTANCE_THRESHOLD 0.75: score > this */
} lisreg_loopdet_params;
typedef struct lisreg_loopdet_frame {
    const void* corner;  int n_corner;  /* cloud_corner (XYZI) */
    const void* surf;    int n_surf;    /* cloud_surface (XYZI) */
    const void* semantic; int n_semantic; /* semantic_raw (XYZIL) */
    float odom[12];                     /* pclPointToAffine3f(optimized_pose) as a row-major 3 x 4 (lisreg_pose_to_matrix) */
} lisreg_loopdet_frame;
typedef struct lisreg_loopdet_result {
    int    current_frame_id;            /* frames stored before this one */
    int    n_candidates;                /* gated history frames */
    int    matched_frame_id;            /* -1: none */
    int    reserved;
    float  matched_transform[16];       /* row-major 4 x 4: translation (diff_x, diff_y, 0), rotation about z by the ICP's yaw */
    double score;                       /* best FEPSC score (0 when none) */
} lisreg_loopdet_result;
typedef struct lisreg_loopdet_candidate {
    int    history_id;
    int    yaw_shift;                   /* winning column shift of the 1 x 360 search, or LISREG_LOOPDET_NO_SHIFT */
    float  yaw_angle;                   /* the angle the ICP source is rotated by (shift * step, or the wrapped yaw * step) */
    int    icp_state, icp_iters, icp_n_corr; /* LISREG_ICP_*, iterations, correspondences of the last one */
    float  transform[16];               /* trans * trans1, row-major 4 x 4 */
    int    score_shift;                 /* -10 .. 9, the first strict minimum (0 when none) */
    int    reserved;
    double score;                       /* 1 - min difference */
} lisreg_loopdet_candidate;
int  lisreg_loopdet_default_params(lisreg_loopdet_params* p);
/* forget every frame of database db_id (0 .. LISREG_LOOPDET_MAX_DB - 1); databases are independent */
int  lisreg_loopdet_reset(lisreg_ctx* ctx, int db_id);
/* loopDetection for frames[0 .. n_frames) in order (frame k sees frames 0 .. k - 1 as history); params NULL = defaults.  results[k]
 * equals, to the bit, what a call with frame k alone returns after frames 0 .. k - 1.  stride: of the host structs (ignored for
 * LISREG_FMT_DEVICE); corner / surf may be XYZIL structs too (the label is not read). */
int  lisreg_loopdet_detect(lisreg_ctx* ctx, int db_id, const lisreg_loopdet_frame* frames, int n_frames, int stride_bytes, int fmt,
                           const lisreg_loopdet_params* params, lisreg_loopdet_result* results);
/* every gated candidate of frame k of the last lisreg_loopdet_detect on db_id, in history order: *n_out = their count, at most
 * cap are written */
int  lisreg_loopdet_candidates(lisreg_ctx* ctx, int db_id, int k, lisreg_loopdet_candidate* out, int cap, int* n_out);
/* the stored descriptors of frame frame_id: FEPSC [20 x 80] (row = ring) and the projection [360 x 4] (count, x, y, label) */
int  lisreg_loopdet_get(lisreg_ctx* ctx, int db_id, int frame_id, uint8_t* fepsc, float* projection);
/* one frame's descriptors under M (row-major 4 x 4, NULL = the clouds as they are): FEPSC, EPSC, SEPSC [20 x 80] and the
 * projection [360 x 4] of the moved semantic cloud; any output may be NULL */
int  lisreg_loop_descriptor(lisreg_ctx* ctx, const void* corner, int n_corner, const void* surf, int n_surf, const void* semantic,
                            int n_semantic, int stride_bytes, int fmt, const float* M, uint8_t* fepsc, uint8_t* epsc,
                            uint8_t* sepsc, float* projection);

/* ---- loop-closure candidate selectors: the seven Using*Flag of loopDetection (src/include/utility.h:446-452) ---------------
 * A database detects with the kinds it was configured with; each enabled kind contributes its own best match, and the matched list
 * is pushed in this bit order (:894-990).  ISC, SC, SSC are computed from the semantic cloud moved by the pair's globalICP
 * transform (calculateISC / calculateSC / calculateSSC, :403-476, 564-589); EPSC, SEPSC, FEPSC as above.  ISC, SC, EPSC, SEPSC,
 * FEPSC score with calculateDistance (threshold distance_threshold), SSC with calculateLabelSim (threshold label_threshold; an empty
 * pair of descriptors scores NaN and is never selected), POSE takes the smallest gate distance.  Deviation: SSC treats labels >= 20
 * (past order_vec) as order 0.  ISC reads the float intensity at byte 16 of the semantic host structs: ISC with LISREG_FMT_DEVICE
 * clouds is LISREG_ERR_ARG. */
#define LISREG_LOOP_ISC   1u
#define LISREG_LOOP_SC    2u
#define LISREG_LOOP_EPSC  4u
#define LISREG_LOOP_SEPSC 8u
#define LISREG_LOOP_FEPSC 16u
#define LISREG_LOOP_SSC   32u
#define LISREG_LOOP_POSE  64u
#define LISREG_LOOP_KINDS 7                 /* kind index = bit position: ISC 0 .. POSE 6 */
#define LISREG_LOOP_LABEL_THRESHOLD 0.79    /* LABEL_THRESHOLD (epscGeneration.h:17) */
typedef struct lisreg_loopdet_match {
    int    kind;                            /* one LISREG_LOOP_* bit */
    int    history_id;
    float  transform[16];                   /* row-major 4 x 4: (diff_x, diff_y, 0) rotated by the kind's angle; SSC / POSE: trans * trans1 */
    double score;                           /* the kind's score; POSE: the gate's pos_distance */
} lisreg_loopdet_match;
typedef struct lisreg_loopdet_kind_scores {
    int    history_id;
    int    shift[LISREG_LOOP_KINDS];        /* calculateDistance's first strict minimum, -10 .. 9 (0 for SSC, POSE and disabled kinds) */
    double score[LISREG_LOOP_KINDS];        /* per kind index; POSE: pos_distance; 0 for disabled kinds */
} lisreg_loopdet_kind_scores;
/* select the kinds (a nonzero mask of LISREG_LOOP_* below 128) of database db_id and SSC's threshold; only while the database is
 * empty (lisreg_loopdet_reset keeps the configuration).  A database never configured is LISREG_LOOP_FEPSC. */
int  lisreg_loopdet_configure(lisreg_ctx* ctx, int db_id, unsigned kinds, double label_threshold);
/* the matched list of frame k of the last lisreg_loopdet_detect on db_id (matched_frame_id / matched_frame_transform), push order */
int  lisreg_loopdet_matches(lisreg_ctx* ctx, int db_id, int k, lisreg_loopdet_match* out, int cap, int* n_out);
/* every gated candidate of frame k of the last detect, in history order, with the score of every enabled kind */
int  lisreg_loopdet_candidate_scores(lisreg_ctx* ctx, int db_id, int k, lisreg_loopdet_kind_scores* out, int cap, int* n_out);
/* the stored (untransformed) descriptor of one enabled kind (ISC .. SSC) of frame frame_id: uint8 [20 x 80], row = ring */
int  lisreg_loopdet_get_descriptor(lisreg_ctx* ctx, int db_id, int frame_id, unsigned kind, uint8_t* out);
/* one frame's descriptor of one kind (ISC .. SSC) under M (NULL = the clouds as they are) */
int  lisreg_loop_descriptor_kind(lisreg_ctx* ctx, unsigned kind, const void* corner, int n_corner, const void* surf, int n_surf,
                                 const void* semantic, int n_semantic, int stride_bytes, int fmt, const float* M, uint8_t* out);

/* ---- helpers that mirror src/core/common.cpp ------------------------------------------------------------- */
/* trans2Affine3f (common.cpp:54-57): row-major 3x4 [R|t]. */
void lisreg_pose_to_matrix(const float T[6], float M[12]);
/* transformUpdate (odomEstimationNode.cpp:976-1006): IMU roll/pitch blend + constraintTransformation clamps. */
void lisreg_transform_update(const lisreg_params* p, const lisreg_imu* imu, float T[6]);

/* ---- multi-GPU pose gather (one process per GPU) ------------------------------------------ */
/* RCCL bootstrap without MPI: rank 0 calls lisreg_comm_unique_id, ships the 128 bytes to the other ranks by
 * any means (file, env, torch.distributed store), then every rank calls lisreg_comm_init.  lisreg_gather_results
 * all-gathers each rank's n_local x 12-float result block (device memory) into `out_device`
 * (nranks x n_local x 12 floats) on the context's stream. */
int  lisreg_comm_unique_id(unsigned char id[128]);
int  lisreg_comm_init(lisreg_ctx* ctx, int rank, int nranks, const unsigned char id[128]);
int  lisreg_gather_results(lisreg_ctx* ctx, const void* local_device, int n_local, void* out_device);
void lisreg_comm_destroy(lisreg_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* LISREG_H_ */
