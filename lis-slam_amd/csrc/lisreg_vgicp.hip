// lisreg_vgicp.hip — voxelised GICP registration: the loop-closure verifier the reference's authors chose last and could
// not link (select_registration_method("FAST_VGICP"), src/core/registration.cpp:156-187, src/node/subMapOptmizationNode.cpp:2771).
// The definition is tests/vgicp_ref.py.  GPU: the distribution of every point of a cloud (its k nearest points within the cloud by an
// exact shell walk over a uniform grid, one query per lane, then mean, covariance and the plane regularisation, fp64), the target's
// per-voxel statistics (the voxel table of voxel_table_build, lisreg_api_cloud.hip, as the NDT target's; one lane or one wavefront per
// voxel) and one linearisation per call (one lane per source point, fp64, sums in a fixed order: the same input gives the same bits).
// Host: the 6 x 6 solve and the Levenberg-Marquardt loop in double, one 29-double read-back per evaluation (eval_totals).  This unit also
// holds the one total kernel of the three verifiers (launch_eval_total).  No CPU fallback.
#include "lisreg_vgicp_lane.hpp"
#include "lisreg_vg_knn_lane.hpp"
#include "lisreg_vg_voxel_lane.hpp"
#include "lisreg_lm_stepper.hpp"
#include "lisreg_jacobi3.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

using namespace lisreg;
using namespace lisreg::vgicp_host;

namespace {

constexpr long long kVgKnnMaxCells = 1LL << 22;     // the search grid of a cloud is dense
constexpr int kVgKnnMaxDim = 2048;                  // cells per axis of the search grid (the walk's rounding slack is sized for this)
static_assert(kVgKnnMaxCells == kVgGridMaxCells, "lisreg_ctx.hpp states the bound for the units that size by it");

// ---- NaN points are no points: the finite records, in input order ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_vg_flag(const float4* __restrict__ in, int n, int* __restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    flag[i] = (p.x == p.x && p.y == p.y && p.z == p.z) ? 1 : 0;
}

// ---- the k nearest points of every point within its own cloud, and its distribution ------------------------------------------------
// One query per lane (vg_knn_lane of lisreg_vg_knn_lane.hpp: the shell walk, the k best in registers, mean, covariance, regularisation)
template <int KT>
__global__ __launch_bounds__(64) void k_vg_knn(VgKnn A)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= A.m) return;
    vg_knn_lane<KT>(A, s);
}

// cov6 rows by the caller's index: NaN rows for the points that are none
__global__ __launch_bounds__(256) void k_vg_cov_rows(const double* __restrict__ cov, const int* __restrict__ flag, const int* __restrict__ pos,
                                                     int n, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (flag[i]) {
        const double* r = cov + (size_t)pos[i] * 6;
#pragma unroll
        for (int e = 0; e < 6; ++e) out[(size_t)i * 6 + e] = r[e];
    } else {
#pragma unroll
        for (int e = 0; e < 6; ++e) out[(size_t)i * 6 + e] = (double)NAN;
    }
}

// ---- target voxels ----------------------------------------------------------------------------------------------------------------
struct VgBuild {
    const float4*   pts;        // the finite points
    const double*   cov;        // [m][6]
    const int*      order;      // sorted position -> point
    const uint32_t* sidx;       // sorted position -> cell id
    const int*      vstart;     // [n_vox + 1]
    int             n_vox;
    long long       n_cells;
    double*         stats;      // [n_vox][kVoxelRec]
    int*            cell;       // [n_vox]
    int*            table;      // [n_cells], -1 on entry
    template <bool WAVE> static __device__ void voxel(const VgBuild& B, int v, int lane);
};

// the body is vg_voxel_lane (lisreg_vg_voxel_lane.hpp), which the batched target build inlines too
template <bool WAVE>
__device__ __forceinline__ void VgBuild::voxel(const VgBuild& B, int v, int lane)
{
    vg_voxel_lane<WAVE>(B.pts, B.cov, B.order, B.sidx, B.vstart[v], B.vstart[v + 1], lane, v, B.n_cells,
                        B.stats + (size_t)v * kVoxelRec, B.cell + v, B.table);
}

// ---- one linearisation ------------------------------------------------------------------------------------------------------------
// one lane per source point (vg_linearize_lane of lisreg_vgicp_lane.hpp), one wavefront per workgroup, one partial record per workgroup;
// NB: the neighbourhood (1, 7 or 27 cells, §7w)
template <bool HESS, int NB>
__global__ __launch_bounds__(64) void k_vgicp_linearize(const float4* __restrict__ src, const double* __restrict__ cov, int n, VoxelView G,
                                                        VgPose P, double* __restrict__ part)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    double acc[28], pairs;
    if constexpr (NB == 1) vg_linearize_lane<HESS>(i < n, src + i, cov + (size_t)i * 6, G, P, acc, pairs);
    else                   vg_linearize_lane_nb<HESS, NB>(i < n, src + i, cov + (size_t)i * 6, G, P, acc, pairs);
    if (threadIdx.x == 0) {
        double* o = part + (size_t)blockIdx.x * kOut;
#pragma unroll
        for (int k = 0; k < 28; ++k) o[k] = acc[k];
        o[28] = pairs;
    }
}

// the partial records of one evaluation added in a fixed order (sum_records), for the three verifiers
__global__ __launch_bounds__(64) void k_eval_total(const double* __restrict__ part, int n_part, double* __restrict__ out)
{
    double acc[kEvalOut];
    sum_records<kEvalOut>(part, n_part, acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kEvalOut; ++k) out[k] = acc[k];
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int check_params(lisreg_ctx* c, const lisreg_vgicp_params* P, const char* who)
{
    if (!P) return bad(c, std::string(who) + ": NULL params");
    if (!(P->resolution > 0) || !std::isfinite(P->resolution)) return bad(c, std::string(who) + ": resolution <= 0");
    if (P->k_correspondences < 4 || P->k_correspondences > 32) return bad(c, std::string(who) + ": k_correspondences outside 4 .. 32");
    if (!(P->transformation_epsilon > 0) || !(P->rotation_epsilon > 0) || !(P->lm_init_lambda_factor > 0) || P->max_iters < 0 ||
        P->lm_max_iterations < 1 || !(P->plane_epsilon > 0 && P->plane_epsilon <= 1))
        return bad(c, std::string(who) + ": bad transformation_epsilon / rotation_epsilon / lm_init_lambda_factor / max_iters / lm_max_iterations / plane_epsilon");
    const int nbs = vg_neighbor_search(*P);
    if (nbs != 0 && nbs != LISREG_VGICP_DIRECT1 && nbs != LISREG_VGICP_DIRECT7 && nbs != LISREG_VGICP_DIRECT27)
        return bad(c, std::string(who) + ": neighbor_search (the last int of params) is none of 0, 1, 7, 27");
    return LISREG_OK;
}

int find_target(lisreg_ctx* c, int slot, const lisreg_vgicp_params* P, const char* who, VgicpTarget** out)
{
    auto it = c->vgicp.find(slot);
    if (slot < 0 || it == c->vgicp.end() || !it->second.valid)
        return bad(c, std::string(who) + ": no VGICP target in this slot (lisreg_vgicp_set_target)");
    if (P && P->resolution != it->second.resolution) return bad(c, std::string(who) + ": params->resolution differs from the slot's");
    *out = &it->second;
    return LISREG_OK;
}

}  // namespace

// the one copy of the checks, for lisreg_vgicp_batch.hip
int lisreg::vg_check_params(lisreg_ctx* c, const lisreg_vgicp_params* P, const char* who) { return check_params(c, P, who); }
int lisreg::vg_find_target(lisreg_ctx* c, int slot, const lisreg_vgicp_params* P, const char* who, VgicpTarget** out)
{
    return find_target(c, slot, P, who, out);
}

// The distributions of one cloud of n device records: afterwards c->vg_pts holds its *m_out finite points in input order, c->vg_idx
// their indices in the cloud, c->vg_flag / c->vg_pos the finite flags and their exclusive scan, c->vg_cov the m x 6 covariances and, if
// nbr_dev is given, nbr_dev the n x k neighbour rows.  bb: the finite bounding box.  edge: the search grid's cell edge, <= 0: chosen
// from the cloud's density so that the 27 cells around a query hold a few tens of points.  grid_out, if given, receives the search grid
// (pts / cell_start = c->vg_sorted / c->vg_cells).  Declared in lisreg_ctx.hpp: lisreg_fgicp.hip makes its distributions with it too.
int lisreg::vg_distributions(lisreg_ctx* c, const char* who, const float4* raw, int n, int k, double plane_eps, float edge, float bb[6],
                             int* m_out, int* nbr_dev, GridIndex* grid_out)
{
    hipStream_t st = c->stream;
    int rc = cloud_bbox(c, raw, n, bb);
    if (rc) return rc;
    for (int e = 0; e < 6; ++e)
        if (std::isinf(bb[e])) return bad(c, std::string(who) + ": the cloud has infinite coordinates");
    GridIndex g;
    rc = vg_search_grid(c, who, raw, n, bb, edge, k, 2, m_out, &g);           // (2: the "index" interval opens in front of the gather)
    if (rc) return rc;
    const int m = *m_out;
    HIPCHK(c, c->vg_cov.ensure(sizeof(double) * 6 * (size_t)m));
    VgKnn A;
    A.sorted = c->vg_sorted.as<float4>(); A.cell_start = c->vg_cells.as<int>(); A.pts = c->vg_pts.as<float4>(); A.orig = c->vg_idx.as<int>();
    A.m = m; A.k = k; A.ox = g.ox; A.oy = g.oy; A.oz = g.oz; A.cell = g.cell; A.inv_cell = g.inv_cell; A.nx = g.nx; A.ny = g.ny; A.nz = g.nz;
    A.plane_eps = plane_eps; A.cov = c->vg_cov.as<double>(); A.nbr = nbr_dev;
    if (k <= 20) k_vg_knn<20><<<(m + 63) / 64, 64, 0, st>>>(A);
    else         k_vg_knn<32><<<(m + 63) / 64, 64, 0, st>>>(A);
    ctx_prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    if (grid_out) *grid_out = g;
    return LISREG_OK;
}

// The grid half of the distributions, which the NDT target shares (lisreg_ndt_set_target keeps the grid for the batch's fitness score):
// the finite points of n device records with the finite bounding box bb, compacted in input order into c->vg_pts (c->vg_idx their
// indices in the cloud, c->vg_flag / c->vg_pos the finite flags and their exclusive scan), and the same points by search-grid cell in
// c->vg_sorted / c->vg_cells.  *m_out = their number, read back and waited for; fewer than min_points (or an empty box) is refused.
// edge as vg_distributions'.  mark >= 0: that profiling interval is opened in front of the gather.  *g = the grid, on the scratch.
int lisreg::vg_search_grid(lisreg_ctx* c, const char* who, const float4* raw, int n, const float bb[6], float edge, int min_points, int mark,
                           int* m_out, GridIndex* g_out)
{
    hipStream_t st = c->stream;
    int rc;
    HIPCHK(c, c->vg_flag.ensure(sizeof(int) * ((size_t)n + 1)));
    HIPCHK(c, c->vg_pos.ensure(sizeof(int) * ((size_t)n + 2)));
    HIPCHK(c, c->vg_idx.ensure(sizeof(int) * ((size_t)n + 1)));
    HIPCHK(c, c->vg_cnt.ensure(sizeof(int) * 4));
    HIPCHK(c, c->scan_tmp.ensure(sizeof(int) * ((size_t)n / 2048 + 4)));
    k_vg_flag<<<(n + 255) / 256, 256, 0, st>>>(raw, n, c->vg_flag.as<int>());
    launch_compact(n, c->vg_flag.as<int>(), c->vg_pos.as<int>(), c->scan_tmp.as<int>(), c->vg_idx.as<int>(), c->vg_cnt.as<int>(), st);
    HIPCHK(c, hipGetLastError());
    int m = 0;
    HIPCHK(c, hipMemcpyAsync(&m, c->vg_cnt.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (m < 0 || m > n) return ctx_fail(c, LISREG_ERR_HIP, std::string(who) + ": the compaction returned an impossible count");
    if (m < min_points || !(bb[0] <= bb[3] && bb[1] <= bb[4] && bb[2] <= bb[5]))
        return bad(c, std::string(who) + ": the cloud has fewer finite points than k_correspondences");
    *m_out = m;
    HIPCHK(c, c->vg_pts.ensure(sizeof(float4) * (size_t)m));
    if (mark >= 0) ctx_prof_mark(c, mark);                         // lisreg_get_timing: "index" = the search grid, the search, the covariances
    launch_gather_points(raw, c->vg_idx.as<int>(), m, c->vg_pts.as<float4>(), st);
    // ---- the search grid ---------------------------------------------------------------------------------------------------------
    GridIndex g;
    memset(&g, 0, sizeof g);
    VgGrid vg;
    vg_grid_geometry(bb, m, edge, &vg);                            // (below: the batched target build chooses with it too)
    g.n = m; g.ox = vg.ox; g.oy = vg.oy; g.oz = vg.oz; g.cell = vg.cell; g.inv_cell = vg.inv_cell; g.nx = vg.nx; g.ny = vg.ny; g.nz = vg.nz;
    const int n_cells = g.nx * g.ny * g.nz;
    rc = ensure_sort_scratch(c, (size_t)m, (size_t)n_cells + 1);
    if (rc) return rc;
    HIPCHK(c, c->vg_sorted.ensure(sizeof(float4) * (size_t)m));
    HIPCHK(c, c->vg_cells.ensure(sizeof(int) * ((size_t)n_cells + 2)));
    launch_build_target(c->vg_pts.as<float4>(), m, g, c->vg_sorted.as<float4>(), c->vg_cells.as<int>(), n_cells, sort_buffers(c), st);
    HIPCHK(c, hipGetLastError());
    *g_out = g; g_out->pts = c->vg_sorted.as<float4>(); g_out->cell_start = c->vg_cells.as<int>();
    return LISREG_OK;
}

// The geometry of the search grid over the finite bounding box bb (min <= max on every axis) of m > 0 finite points: the one copy, for
// vg_search_grid above and for lisreg_fgicp_set_target_batch (lisreg_fgicp_target_batch.hip), which chooses the grids of all its targets
// on the host between its two phases.  edge > 0: the cell edge is forced; else it is chosen from the cloud's density.  The edge grows by
// 1.26 (a doubling of the cell volume) until the grid has at most kVgKnnMaxDim cells per axis and kVgKnnMaxCells in all.  Host arithmetic
// only.
void lisreg::vg_grid_geometry(const float bb[6], int m, float edge, VgGrid* g)
{
    const double ex[3] = { (double)bb[3] - bb[0], (double)bb[4] - bb[1], (double)bb[5] - bb[2] };
    double cell = edge;
    if (!(cell > 0)) {
        // lidar clouds are surfaces over a ground plane: with 4 points per cell footprint the 3 x 3 columns around a query hold about 36
        const double area = std::max(ex[0], 1.0e-3) * std::max(ex[1], 1.0e-3);
        cell = std::sqrt(4.0 * area / (double)m);
    }
    cell = std::max(cell, 1.0e-4);
    for (;;) {
        const double nx = floor(ex[0] / cell) + 1, ny = floor(ex[1] / cell) + 1, nz = floor(ex[2] / cell) + 1;
        if (nx <= kVgKnnMaxDim && ny <= kVgKnnMaxDim && nz <= kVgKnnMaxDim && nx * ny * nz <= (double)kVgKnnMaxCells) {
            g->nx = (int)nx; g->ny = (int)ny; g->nz = (int)nz;
            break;
        }
        cell *= 1.26;
    }
    g->ox = bb[0]; g->oy = bb[1]; g->oz = bb[2]; g->cell = (float)cell; g->inv_cell = 1.f / g->cell;
}

void lisreg::launch_eval_total(const double* part, int n_part, double* out, hipStream_t st)
{
    k_eval_total<<<1, 64, 0, st>>>(part, n_part, out);
}

namespace {

int distributions(lisreg_ctx* c, const char* who, const float4* raw, int n, int k, double plane_eps, float edge, float bb[6], int* m_out,
                  int* nbr_dev)
{
    return vg_distributions(c, who, raw, n, k, plane_eps, edge, bb, m_out, nbr_dev, nullptr);
}

struct VgRun {
    lisreg_ctx*        c;
    const VgicpTarget* T;
    const float4*      src;      // the source's finite points
    const double*      cov;
    int                n;
    int                neighbors = 0;       // vg_neighbor_search of the call's params
    int                n_evals = 0;
};

template <bool HESS>
void launch_linearize(const VgRun& r, int nb, const VoxelView& G, const VgPose& P, double* part)
{
    hipStream_t st = r.c->stream;
    switch (r.neighbors) {
    case LISREG_VGICP_DIRECT7:  k_vgicp_linearize<HESS, 7><<<nb, 64, 0, st>>>(r.src, r.cov, r.n, G, P, part); break;
    case LISREG_VGICP_DIRECT27: k_vgicp_linearize<HESS, 27><<<nb, 64, 0, st>>>(r.src, r.cov, r.n, G, P, part); break;
    default:                    k_vgicp_linearize<HESS, 1><<<nb, 64, 0, st>>>(r.src, r.cov, r.n, G, P, part); break;     // 0 and 1 (check_params)
    }
}

int evaluate(VgRun& r, const double T[16], bool hess, double out[kOut])
{
    lisreg_ctx* c = r.c;
    const VgPose P = pose_of<VgPose>(T);
    const VoxelView G = voxel_table_view(*r.T);
    const int nb = (r.n + 63) / 64;
    const int rc = eval_totals(c, nb, [&](double* part) {
        ctx_prof_mark(c, 0);                                       // "assoc" = the linearisations (both launches), one interval each
        if (hess) launch_linearize<true>(r, nb, G, P, part);
        else      launch_linearize<false>(r, nb, G, P, part);
    }, true, out);
    if (!rc) ++r.n_evals;
    return rc;
}

// the checks and the staging every entry point with a source shares: its distributions end up in c->vg_pts / c->vg_cov
int stage_source(lisreg_ctx* c, const char* who, int slot, const void* source, int n, int stride, int fmt, const lisreg_vgicp_params* P,
                 VgRun* r, const float4** raw)
{
    int rc = check_params(c, P, who);
    if (rc) return rc;
    VgicpTarget* T = nullptr;
    rc = find_target(c, slot, P, who, &T);
    if (rc) return rc;
    rc = check_cloud(c, who, source, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = stage_records(c, source, n, stride, fmt, c->vg_raw, raw);
    if (rc) return rc;
    float bb[6];
    int m = 0;
    rc = distributions(c, who, *raw, n, P->k_correspondences, P->plane_epsilon, 0.f, bb, &m, nullptr);
    if (rc) return rc;
    r->c = c; r->T = T; r->src = c->vg_pts.as<float4>(); r->cov = c->vg_cov.as<double>(); r->n = m;
    r->neighbors = vg_neighbor_search(*P);
    return LISREG_OK;
}

}  // namespace

extern "C" {

int lisreg_vgicp_default_params(int kind, lisreg_vgicp_params* p)
{
    if (!p || kind != 0) return LISREG_ERR_ARG;
    *p = lisreg_vgicp_params{ 1.0, 0.01, 2.0e-3, 1.0e-9, 1.0e-3, 20, 50, 10, 0 };
    return LISREG_OK;
}

int lisreg_vgicp_set_target(lisreg_ctx* c, int slot, const void* cloud, int n, int stride, int fmt, const lisreg_vgicp_params* P,
                            lisreg_vgicp_info* info)
{
    if (!c) return LISREG_ERR_ARG;
    if (slot < 0 || slot > 65535) return bad(c, "vgicp_set_target: bad slot");
    int rc = check_params(c, P, "vgicp_set_target");
    if (rc) return rc;
    rc = check_cloud(c, "vgicp_set_target", cloud, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    VgicpTarget& T = c->vgicp[slot];
    T.valid = false;
    const float4* raw = nullptr;
    rc = stage_records(c, cloud, n, stride, fmt, c->vg_raw, &raw);
    if (rc) return rc;
    float bb[6];
    int m = 0;
    GridIndex g;
    rc = vg_distributions(c, "vgicp_set_target", raw, n, P->k_correspondences, P->plane_epsilon, 0.f, bb, &m, nullptr, &g);
    if (rc) return rc;
    // the search grid of the distributions stays with the slot (the batch's fitness score searches it): its own copies, made before the
    // voxel sort reuses any scratch
    const size_t n_grid_cells = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    HIPCHK(c, T.sorted.ensure(sizeof(float4) * (size_t)m));
    HIPCHK(c, T.cells.ensure(sizeof(int) * (n_grid_cells + 1)));
    HIPCHK(c, hipMemcpyAsync(T.sorted.p, c->vg_sorted.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(T.cells.p, c->vg_cells.p, sizeof(int) * (n_grid_cells + 1), hipMemcpyDeviceToDevice, st));
    T.grid = g; T.grid.pts = T.sorted.as<float4>(); T.grid.cell_start = T.cells.as<int>();
    for (int k = 0; k < 6; ++k) T.bb[k] = bb[k];
    // ---- the voxel table (pcl::VoxelGrid's geometry and sort, as the NDT target's) and its statistics --------------------------------------
    // "solve" = the voxel sort and statistics (with the wait for the voxel count)
    rc = voxel_table_build(c, "vgicp_set_target", "voxel table", c->vg_pts.as<float4>(), m, bb, P->resolution, 1, T);
    if (rc) return rc;
    VgBuild B;
    B.pts = c->vg_pts.as<float4>(); B.cov = c->vg_cov.as<double>(); B.order = c->vox_order.as<int>(); B.sidx = c->vox_sidx.as<uint32_t>();
    B.vstart = c->vox_start.as<int>(); B.n_vox = T.n_voxels; B.n_cells = (long long)T.dims[0] * T.dims[1] * T.dims[2];
    B.stats = T.stats.as<double>(); B.cell = T.cell.as<int>(); B.table = T.table.as<int>();
    launch_voxel_stats(B, st);
    ctx_prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));
    ctx_prof_collect(c);
    T.n_points = m;
    if (info) { for (int k = 0; k < 3; ++k) info->dims[k] = T.dims[k]; info->n_voxels = T.n_voxels; info->n_points = m; }
    T.valid = true;
    return LISREG_OK;
}

int lisreg_vgicp_covariances(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, int k, double* cov6_out, int* neighbours_out,
                             float cell_edge)
{
    if (!c) return LISREG_ERR_ARG;
    if (k < 4 || k > 32) return bad(c, "vgicp_covariances: k outside 4 .. 32");
    if (!cov6_out) return bad(c, "vgicp_covariances: NULL cov6_out");
    if (!(cell_edge >= 0.f) || !std::isfinite(cell_edge)) return bad(c, "vgicp_covariances: cell_edge < 0");
    int rc = check_cloud(c, "vgicp_covariances", cloud, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const float4* raw = nullptr;
    rc = stage_records(c, cloud, n, stride, fmt, c->vg_raw, &raw);
    if (rc) return rc;
    if (neighbours_out) {
        HIPCHK(c, c->vg_nbr.ensure(sizeof(int) * (size_t)n * (size_t)k));
        HIPCHK(c, hipMemsetAsync(c->vg_nbr.p, 0xFF, sizeof(int) * (size_t)n * (size_t)k, st));      // -1 rows for the points that are none
    }
    float bb[6];
    int m = 0;
    rc = distributions(c, "vgicp_covariances", raw, n, k, 1.0e-3, cell_edge, bb, &m, neighbours_out ? c->vg_nbr.as<int>() : nullptr);
    if (rc) return rc;
    HIPCHK(c, c->vg_rows.ensure(sizeof(double) * 6 * (size_t)n));
    k_vg_cov_rows<<<(n + 255) / 256, 256, 0, st>>>(c->vg_cov.as<double>(), c->vg_flag.as<int>(), c->vg_pos.as<int>(), n, c->vg_rows.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(cov6_out, c->vg_rows.p, sizeof(double) * 6 * (size_t)n, hipMemcpyDeviceToHost, st));
    if (neighbours_out) HIPCHK(c, hipMemcpyAsync(neighbours_out, c->vg_nbr.p, sizeof(int) * (size_t)n * (size_t)k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ctx_prof_collect(c);
    return LISREG_OK;
}

int lisreg_vgicp_get_voxels(lisreg_ctx* c, int slot, int* cell_ids, int* counts, double* means, double* cov6, int capacity, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    VgicpTarget* T = nullptr;
    int rc = find_target(c, slot, nullptr, "vgicp_get_voxels", &T);
    if (rc) return rc;
    if (!n_out || capacity < 0) return bad(c, "vgicp_get_voxels: bad arguments");
    *n_out = T->n_voxels;
    if (T->n_voxels > capacity) return LISREG_OK;
    if (!cell_ids || !counts || !means || !cov6) return bad(c, "vgicp_get_voxels: NULL output");
    return voxel_table_read(c, *T, nullptr, cell_ids, counts, means, cov6, capacity);
}

int lisreg_vgicp_linearize(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_vgicp_params* P,
                           const double T[16], int with_hessian, double out[28], long long* n_pairs)
{
    if (!c) return LISREG_ERR_ARG;
    if (!T || !out) return bad(c, "vgicp_linearize: NULL T / out");
    VgRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "vgicp_linearize", slot, source, n, stride, fmt, P, &r, &raw);
    if (rc) return rc;
    double o[kOut];
    rc = evaluate(r, T, with_hessian != 0, o);
    if (rc) return rc;
    memcpy(out, o, sizeof(double) * 28);
    if (n_pairs) *n_pairs = (long long)o[28];
    ctx_prof_collect(c);
    return LISREG_OK;
}

int lisreg_vgicp_align(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_vgicp_params* P,
                       const float* guess, lisreg_vgicp_result* res, void* aligned_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!res) return bad(c, "vgicp_align: NULL result");
    VgRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "vgicp_align", slot, source, n, stride, fmt, P, &r, &raw);
    if (rc) return rc;
    double T0[16];
    guess_to_T0(guess, T0);
    LmResult lr;
    rc = lm_optimise([&](const double T[16], bool hess, double out[kOut]) { return evaluate(r, T, hess, out); }, T0, lm_params_of(*P), &lr);
    if (rc) return rc;
    ctx_prof_collect(c);
    lm_result_to(lr, res);
    if (aligned_out) {                                    // the source under the final transformation (in float, like lisreg_transform_cloud)
        float F[12];
        for (int k = 0; k < 12; ++k) F[k] = (float)lr.T[k];
        return emit_aligned(c, raw, n, F, source, stride, fmt, c->vg_sorted, aligned_out);
    }
    return LISREG_OK;
}

}  // extern "C"
