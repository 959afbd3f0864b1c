// lisreg_ndt.hip — Normal Distributions Transform registration: the loop-closure verifier the reference names first
// (pcl::NormalDistributionsTransform, src/core/registration.cpp:147-155, src/node/subMapOptmizationNode.cpp:2756-2760).
// The definition is tests/ndt_ref.py.  GPU: the target's per-voxel Gaussians (the voxel table of voxel_table_build, lisreg_api_cloud.hip,
// then one lane or one wavefront per voxel, fp64) and one evaluation of score / gradient / Hessian per call (one lane per source point,
// fp64, sums in a fixed order: no floating-point atomics, the same input gives the same bits).  Host: the 6 x 6 solve and the
// More-Thuente line search in double (the resumable loop of lisreg_ndt_stepper.hpp, answered one request at a time), one 29-double
// read-back per evaluation (eval_totals).  The butterfly, the total, the round trip and the statistics' launch shell are the ones VGICP
// and FastGICP use (lisreg_fp64_sums.hpp); the lane's body of an evaluation is shared with the batch form (lisreg_ndt_lane.hpp,
// lisreg_ndt_batch.hip).  No CPU fallback.
#include "lisreg_fp64_sums.hpp"
#include "lisreg_ndt_lane.hpp"
#include "lisreg_ndt_voxel_lane.hpp"
#include "lisreg_ndt_stepper.hpp"
#include "lisreg_jacobi3.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

using namespace lisreg;
using namespace lisreg::ndt_host;

namespace {

// ---- target: NaN points out of the way ------------------------------------------------------------------------------------------
// A point with a NaN coordinate belongs to no voxel.  It is moved onto the box's minimum corner and marked in .w, so that the voxel keys
// of every record are inside the grid whatever a float -> int conversion makes of a NaN; the statistics skip the marked records.
__global__ __launch_bounds__(256) void k_ndt_clean(const float4* __restrict__ in, int n, float lx, float ly, float lz, float4* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float4 p = in[i];
    const bool bad = p.x != p.x || p.y != p.y || p.z != p.z;
    out[i] = bad ? make_float4(lx, ly, lz, 1.0f) : make_float4(p.x, p.y, p.z, 0.0f);
}

struct NdtBuild {
    const float4*   pts;        // cleaned records
    const int*      order;      // sorted position -> record
    const uint32_t* sidx;       // sorted position -> cell id
    const int*      vstart;     // [n_vox + 1]
    int             n_vox, min_pts;
    long long       n_cells;
    double          mult;
    double*         stats;      // [n_vox][kVoxelRec]
    int*            vflag;      // [n_vox]
    int*            cell;       // [n_vox]
    int*            table;      // [n_cells], -1 on entry
    int*            counters;   // [0] voxels with a finite point, [1] valid voxels
    template <bool WAVE> static __device__ void voxel(const NdtBuild& B, int v, int lane);
};

// the body is ndt_voxel_lane (lisreg_ndt_voxel_lane.hpp), which the batched target build inlines too
template <bool WAVE>
__device__ __forceinline__ void NdtBuild::voxel(const NdtBuild& B, int v, int lane)
{
    ndt_voxel_lane<WAVE, NdtSkipMarked>(B.pts, B.order, B.sidx, B.vstart[v], B.vstart[v + 1], lane, v, B.n_cells, B.min_pts, B.mult,
                                        B.stats + (size_t)v * kVoxelRec, B.vflag + v, B.cell + v, B.table, B.counters);
}

// ---- one evaluation --------------------------------------------------------------------------------------------------------------
// one lane per source record, one wavefront per workgroup, one partial record per workgroup (the lane's body: lisreg_ndt_lane.hpp)
template <bool HESS>
__global__ __launch_bounds__(64) void k_ndt_eval(const float4* __restrict__ src, int n, VoxelView G, NdtGauss K, NdtPose P, double* __restrict__ part)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    double acc[28], pairs;
    ndt_eval_lane<HESS>(i < n, src + i, G, K, P, acc, pairs);
    ndt_store_partial(acc, pairs, part + (size_t)blockIdx.x * kEvalOut);
}

struct NdtRun {
    lisreg_ctx*      c;
    const NdtTarget* T;
    const float4*    src;
    int              n;
    double           g1, g2;
    double           out[kEvalOut];
};

int evaluate(NdtRun& r, const double p[6], bool hess)
{
    lisreg_ctx* c = r.c;
    NdtPose P;
    pose_matrices(p, &P);
    const VoxelView G = voxel_table_view(*r.T);
    const NdtGauss K = { r.T->resolution * r.T->resolution, r.g1, r.g2 };
    const int nb = (r.n + 63) / 64;
    return eval_totals(c, nb, [&](double* part) {
        if (hess) k_ndt_eval<true><<<nb, 64, 0, c->stream>>>(r.src, r.n, G, K, P, part);
        else      k_ndt_eval<false><<<nb, 64, 0, c->stream>>>(r.src, r.n, G, K, P, part);
    }, false, r.out);
}

int find_target(lisreg_ctx* c, int slot, const lisreg_ndt_params* P, const char* who, NdtTarget** out)
{
    auto it = c->ndt.find(slot);
    if (slot < 0 || it == c->ndt.end() || !it->second.valid)
        return ctx_fail(c, LISREG_ERR_NO_TARGET, std::string(who) + ": no NDT target in this slot (lisreg_ndt_set_target)");
    if (P && P->resolution != it->second.resolution) return bad(c, std::string(who) + ": params->resolution differs from the slot's");
    *out = &it->second;
    return LISREG_OK;
}

int check_params(lisreg_ctx* c, const lisreg_ndt_params* P, const char* who)
{
    if (!P) return bad(c, std::string(who) + ": NULL params");
    if (!(P->resolution > 0) || !std::isfinite(P->resolution)) return bad(c, std::string(who) + ": resolution <= 0");
    if (!(P->outlier_ratio > 0 && P->outlier_ratio < 1)) return bad(c, std::string(who) + ": outlier_ratio outside (0, 1)");
    if (!(P->step_size > 0) || !(P->transformation_epsilon > 0) || P->max_iters < 0 || !(P->min_covar_eigvalue_mult >= 0))
        return bad(c, std::string(who) + ": bad step_size / transformation_epsilon / max_iters / min_covar_eigvalue_mult");
    return LISREG_OK;
}

}  // namespace

// the one copy of the checks and of the result's conversion, for lisreg_ndt_batch.hip
int lisreg::ndt_check_params(lisreg_ctx* c, const lisreg_ndt_params* P, const char* who) { return check_params(c, P, who); }
int lisreg::ndt_find_target(lisreg_ctx* c, int slot, const lisreg_ndt_params* P, const char* who, NdtTarget** out)
{
    return find_target(c, slot, P, who, out);
}
void lisreg::ndt_result_to(const NdtLoopResult& lr, lisreg_ndt_result* res)
{
    NdtPose Pm;
    pose_matrices(lr.p, &Pm);
    float* F = res->final_transform;
    for (int i = 0; i < 3; ++i) { for (int j = 0; j < 3; ++j) F[4 * i + j] = (float)Pm.R[3 * i + j]; F[4 * i + 3] = (float)lr.p[i]; }
    F[12] = F[13] = F[14] = 0.f; F[15] = 1.f;
    memcpy(res->p, lr.p, sizeof lr.p);
    res->converged = lr.converged; res->iters = lr.iters; res->n_evals = lr.n_evals; res->reserved = 0;
    res->n_pairs_last = lr.n_pairs_last;
    res->score = lr.score; res->trans_probability = lr.trans_probability;
}

extern "C" {

int lisreg_ndt_default_params(int kind, lisreg_ndt_params* p)
{
    if (!p || kind != 0) return LISREG_ERR_ARG;
    *p = lisreg_ndt_params{ 1.0, 0.1, 0.01, 0.55, 0.01, 35, 6, 1, 0 };
    return LISREG_OK;
}

int lisreg_ndt_set_target(lisreg_ctx* c, int slot, const void* cloud, int n, int stride, int fmt, const lisreg_ndt_params* P,
                          lisreg_ndt_info* info)
{
    if (!c) return LISREG_ERR_ARG;
    if (slot < 0 || slot > 65535) return bad(c, "ndt_set_target: bad slot");
    int rc = check_params(c, P, "ndt_set_target");
    if (rc) return rc;
    rc = check_cloud(c, "ndt_set_target", cloud, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    NdtTarget& T = c->ndt[slot];
    T.valid = false;
    const float4* raw = nullptr;
    rc = stage_records(c, cloud, n, stride, fmt, c->ndt_src, &raw);
    if (rc) return rc;
    // ---- bounding box (each coordinate's finite minimum / maximum) and the pcl::VoxelGrid geometry ----------------------------------
    float bb[6];
    rc = cloud_bbox(c, raw, n, bb);
    if (rc) return rc;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(bb[k])) return bad(c, "ndt_set_target: the cloud has infinite coordinates");
    if (!(bb[0] <= bb[3] && bb[1] <= bb[4] && bb[2] <= bb[5])) return bad(c, "ndt_set_target: the cloud has no finite point: no valid voxel");
    // ---- the search grid over the finite points (the fitness score of lisreg_ndt_align_batch searches it): the grid half of the fast_gicp
    // family's distributions, and the slot's own copies of it, made before the voxel sort reuses any scratch ---------------------------
    GridIndex g;
    int m = 0;
    rc = vg_search_grid(c, "ndt_set_target", raw, n, bb, 0.f, 1, -1, &m, &g);
    if (rc) return rc;
    const size_t n_grid_cells = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    HIPCHK(c, T.sorted.ensure(sizeof(float4) * (size_t)m));
    HIPCHK(c, T.cells.ensure(sizeof(int) * (n_grid_cells + 1)));
    HIPCHK(c, hipMemcpyAsync(T.sorted.p, c->vg_sorted.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(T.cells.p, c->vg_cells.p, sizeof(int) * (n_grid_cells + 1), hipMemcpyDeviceToDevice, st));
    T.grid = g; T.grid.pts = T.sorted.as<float4>(); T.grid.cell_start = T.cells.as<int>();
    T.n_points = m;
    for (int k = 0; k < 6; ++k) T.bb[k] = bb[k];
    // ---- NaN points aside, then the voxel table (the sort of lisreg_voxel_downsample) ------------------------------------------------
    HIPCHK(c, c->ndt_pts.ensure(sizeof(float4) * (size_t)n));
    k_ndt_clean<<<(n + 255) / 256, 256, 0, st>>>(raw, n, bb[0], bb[1], bb[2], c->ndt_pts.as<float4>());
    rc = voxel_table_build(c, "ndt_set_target", "cell table", c->ndt_pts.as<float4>(), n, bb, P->resolution, -1, T);
    if (rc) return rc;
    // ---- the Gaussians ------------------------------------------------------------------------------------------------------------------
    const int n_vox = T.n_voxels;
    HIPCHK(c, T.vflag.ensure(sizeof(int) * (size_t)n_vox));
    HIPCHK(c, c->ndt_cnt.ensure(sizeof(int) * 4));
    HIPCHK(c, hipMemsetAsync(c->ndt_cnt.p, 0, sizeof(int) * 4, st));
    NdtBuild B;
    B.pts = c->ndt_pts.as<float4>(); B.order = c->vox_order.as<int>(); B.sidx = c->vox_sidx.as<uint32_t>(); B.vstart = c->vox_start.as<int>();
    B.n_vox = n_vox; B.min_pts = P->min_points_per_voxel; B.n_cells = (long long)T.dims[0] * T.dims[1] * T.dims[2]; B.mult = P->min_covar_eigvalue_mult;
    B.stats = T.stats.as<double>(); B.vflag = T.vflag.as<int>(); B.cell = T.cell.as<int>(); B.table = T.table.as<int>();
    B.counters = c->ndt_cnt.as<int>();
    launch_voxel_stats(B, st);
    HIPCHK(c, hipGetLastError());
    int cnt[2] = { 0, 0 };
    HIPCHK(c, hipMemcpyAsync(cnt, c->ndt_cnt.p, sizeof cnt, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    T.n_occupied = cnt[0]; T.n_valid = cnt[1];
    if (info) { for (int k = 0; k < 3; ++k) info->dims[k] = T.dims[k]; info->n_voxels = cnt[0]; info->n_valid = cnt[1]; info->reserved = 0; }
    if (cnt[1] < 1) return bad(c, "ndt_set_target: the target has no valid voxel (min_points_per_voxel points with a positive-definite covariance)");
    T.valid = true;
    return LISREG_OK;
}

int lisreg_ndt_get_voxels(lisreg_ctx* c, int slot, int* cell_ids, int* counts, double* means, double* icov6, int capacity, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    NdtTarget* T = nullptr;
    int rc = find_target(c, slot, nullptr, "ndt_get_voxels", &T);
    if (rc) return rc;
    if (!n_out || capacity < 0) return bad(c, "ndt_get_voxels: bad arguments");
    *n_out = T->n_valid;
    if (T->n_valid > capacity) return LISREG_OK;
    if (!cell_ids || !counts || !means || !icov6) return bad(c, "ndt_get_voxels: NULL output");
    return voxel_table_read(c, *T, &T->vflag, cell_ids, counts, means, icov6, capacity);
}

int lisreg_ndt_derivatives(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_ndt_params* P,
                           const double p[6], int with_hessian, double out[28], long long* n_pairs)
{
    if (!c) return LISREG_ERR_ARG;
    int rc = check_params(c, P, "ndt_derivatives");
    if (rc) return rc;
    NdtTarget* T = nullptr;
    rc = find_target(c, slot, P, "ndt_derivatives", &T);
    if (rc) return rc;
    rc = check_cloud(c, "ndt_derivatives", source, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    if (!p || !out) return bad(c, "ndt_derivatives: NULL p / out");
    HIPCHK(c, hipSetDevice(c->device));
    NdtRun r; r.c = c; r.T = T; r.n = n;
    rc = stage_records(c, source, n, stride, fmt, c->ndt_src, &r.src);
    if (rc) return rc;
    gauss_constants(P->outlier_ratio, P->resolution, &r.g1, &r.g2);
    rc = evaluate(r, p, with_hessian != 0);
    if (rc) return rc;
    memcpy(out, r.out, sizeof(double) * 28);
    if (n_pairs) *n_pairs = (long long)r.out[28];
    return LISREG_OK;
}

int lisreg_ndt_align(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_ndt_params* P,
                     const float* guess, lisreg_ndt_result* res, void* aligned_out)
{
    if (!c) return LISREG_ERR_ARG;
    int rc = check_params(c, P, "ndt_align");
    if (rc) return rc;
    NdtTarget* T = nullptr;
    rc = find_target(c, slot, P, "ndt_align", &T);
    if (rc) return rc;
    rc = check_cloud(c, "ndt_align", source, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    if (!res) return bad(c, "ndt_align: NULL result");
    HIPCHK(c, hipSetDevice(c->device));
    NdtRun r; r.c = c; r.T = T; r.n = n;
    rc = stage_records(c, source, n, stride, fmt, c->ndt_src, &r.src);
    if (rc) return rc;
    gauss_constants(P->outlier_ratio, P->resolution, &r.g1, &r.g2);
    // the Newton loop with its line search, one evaluation at a time
    double p0[6];
    p_from_matrix(guess, p0);
    NdtLoopResult lr;
    rc = ndt_optimise([&](const double p[6], bool hess, double out[kNdtOut]) {
        const int e = evaluate(r, p, hess);
        memcpy(out, r.out, sizeof r.out);
        return e;
    }, p0, ndt_loop_params_of(*P), n, &lr);
    if (rc) return rc;
    ndt_result_to(lr, res);
    // `output` of align(): the source under the final transformation
    if (aligned_out) return emit_aligned(c, r.src, n, res->final_transform, source, stride, fmt, c->ndt_pts, aligned_out);
    return LISREG_OK;
}

}  // extern "C"
