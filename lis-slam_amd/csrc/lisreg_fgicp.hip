// lisreg_fgicp.hip — FastGICP registration: the last verifier of the fast_gicp family that
// select_registration_method names (src/core/registration.cpp:157-166: "FAST_GICP", max correspondence distance 5, correspondence
// randomness 20).  The definition is tests/fgicp_ref.py.  The distributions, the SE(3) exponential, the damped solve and the
// Levenberg-Marquardt loop are VGICP's (lisreg_vgicp.hip, lisreg_vgicp_host.hpp).  What is new on the GPU: per linearisation an exact
// nearest-neighbour search of every transformed source point in the target cloud (one query per lane, a shell walk over the target's
// search grid, fp64, ties to the lower index) that leaves the pair and its M = (C_b + R C_a R^T)^-1 behind, and the 28 sums over the stored
// pairs at any pose (an error evaluation reuses the pairs and the M of the last linearisation).  Sums in a fixed order: the same input
// gives the same bits.  No CPU fallback.
#include "lisreg_fgicp_lane.hpp"
#include "lisreg_lm_stepper.hpp"
#include "lisreg_jacobi3.hpp"

#include <cfloat>
#include <cmath>
#include <cstring>

using namespace lisreg;
using namespace lisreg::vgicp_host;

namespace {

// One source point per lane (fg_pairs_lane of lisreg_fgicp_lane.hpp: the search, the cut-off and the pair's M).  pair[i] = sorted position
// of the correspondent or -1; M6[i] = xx, xy, xz, yy, yz, zz of M (written for pairs only).
__global__ __launch_bounds__(64) void k_fgicp_pairs(const float4* __restrict__ src, const double* __restrict__ scov, int n, FgTarget A, FgPose P,
                                                    double max_d, double max2, int* __restrict__ pair, double* __restrict__ M6,
                                                    double* __restrict__ d2_out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    fg_pairs_lane(src[i], scov + (size_t)i * 6, A, P, max_d, max2, pair + i, M6 + (size_t)i * 6, d2_out ? d2_out + i : nullptr);
}

// The 28 sums and the pair count over the stored pairs at P (fg_sums_lane).  One lane per source point, one wavefront per workgroup, one
// partial record per workgroup (the shape of k_vgicp_linearize); eval_totals adds them.
template <bool HESS>
__global__ __launch_bounds__(64) void k_fgicp_sums(const float4* __restrict__ src, const int* __restrict__ pair, const double* __restrict__ M6,
                                                   int n, const float4* __restrict__ tgt_sorted, FgPose P, double* __restrict__ part)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    double acc[28], pairs;
    const int j = i < n ? pair[i] : -1;
    fg_sums_lane<HESS>(j, src + i, M6 + (size_t)i * 6, tgt_sorted, P, acc, pairs);
    if (threadIdx.x == 0) {
        double* o = part + (size_t)blockIdx.x * kOut;
#pragma unroll
        for (int k = 0; k < 28; ++k) o[k] = acc[k];
        o[28] = pairs;
    }
}

// the test hook's rows by the CALLER's source index: the correspondent's index in the caller's target cloud and its squared distance
__global__ __launch_bounds__(256) void k_fgicp_rows(const int* __restrict__ pair, const double* __restrict__ d2, const int* __restrict__ flag,
                                                    const int* __restrict__ pos, int n, const float4* __restrict__ tgt_sorted,
                                                    const int* __restrict__ tgt_orig, int* __restrict__ idx_out, double* __restrict__ d_out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int idx = -1;
    double d = (double)NAN;
    if (flag[i]) {
        const int s = pos[i], j = pair[s];
        if (j >= 0) { idx = tgt_orig[__float_as_int(tgt_sorted[j].w)]; d = d2[s]; }
    }
    idx_out[i] = idx;
    d_out[i] = d;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int check_params(lisreg_ctx* c, const lisreg_fgicp_params* P, const char* who)
{
    if (!P) return bad(c, std::string(who) + ": NULL params");
    if (!(P->max_correspondence_distance > 0)) return bad(c, std::string(who) + ": max_correspondence_distance <= 0");
    if (P->k_correspondences < 4 || P->k_correspondences > 32) return bad(c, std::string(who) + ": k_correspondences outside 4 .. 32");
    if (!(P->transformation_epsilon > 0) || !(P->rotation_epsilon > 0) || !(P->lm_init_lambda_factor > 0) || P->max_iters < 0 ||
        P->lm_max_iterations < 1 || !(P->plane_epsilon > 0 && P->plane_epsilon <= 1))
        return bad(c, std::string(who) + ": bad transformation_epsilon / rotation_epsilon / lm_init_lambda_factor / max_iters / lm_max_iterations / plane_epsilon");
    return LISREG_OK;
}

int find_target(lisreg_ctx* c, int slot, const char* who, FgicpTarget** out)
{
    auto it = c->fgicp.find(slot);
    if (slot < 0 || it == c->fgicp.end() || !it->second.valid)
        return bad(c, std::string(who) + ": no FastGICP target in this slot (lisreg_fgicp_set_target)");
    *out = &it->second;
    return LISREG_OK;
}

struct FgRun {
    lisreg_ctx*        c;
    const FgicpTarget* T;
    const float4*      src;      // the source's finite points, in input order: the lanes' order
    const double*      cov;
    int                n;
    double             max_d;
};

// the search at T: pairs and M into c->fg_pair / c->fg_M (and the squared distances into c->fg_d2 if wanted)
int search(FgRun& r, const double T[16], bool want_d2)
{
    lisreg_ctx* c = r.c;
    const FgicpTarget& G = *r.T;
    const FgTarget A = fg_target_view(G);
    ctx_prof_mark(c, 1);                                           // lisreg_get_timing: "solve" = the search launches, one interval each
    k_fgicp_pairs<<<(r.n + 63) / 64, 64, 0, c->stream>>>(r.src, r.cov, r.n, A, pose_of<FgPose>(T), r.max_d, r.max_d * r.max_d, c->fg_pair.as<int>(),
                                                          c->fg_M.as<double>(), want_d2 ? c->fg_d2.as<double>() : nullptr);
    ctx_prof_mark(c, -1);
    HIPCHK(c, hipGetLastError());
    return LISREG_OK;
}

// the sums over the stored pairs at T
int sums(FgRun& r, const double T[16], bool hess, double out[kOut])
{
    lisreg_ctx* c = r.c;
    const int nb = (r.n + 63) / 64;
    const FgPose P = pose_of<FgPose>(T);
    return eval_totals(c, nb, [&](double* part) {
        ctx_prof_mark(c, 0);                                       // "assoc" = the sum launches (with the fixed-order total), one interval each
        if (hess) k_fgicp_sums<true><<<nb, 64, 0, c->stream>>>(r.src, c->fg_pair.as<int>(), c->fg_M.as<double>(), r.n, r.T->sorted.as<float4>(), P, part);
        else      k_fgicp_sums<false><<<nb, 64, 0, c->stream>>>(r.src, c->fg_pair.as<int>(), c->fg_M.as<double>(), r.n, r.T->sorted.as<float4>(), P, part);
    }, true, out);
}

// one evaluation as the LM loop asks for it: a linearisation searches, an error evaluation reuses the pairs and the M of the last one
int evaluate(FgRun& r, const double T[16], bool hess, double out[kOut])
{
    if (hess) {
        const int rc = search(r, T, false);
        if (rc) return rc;
    }
    return sums(r, T, hess, out);
}

// the checks and the staging every entry point with a source shares: its distributions end up in c->vg_pts / c->vg_cov
int stage_source(lisreg_ctx* c, const char* who, int slot, const void* source, int n, int stride, int fmt, const lisreg_fgicp_params* P,
                 FgRun* r, const float4** raw)
{
    int rc = check_params(c, P, who);
    if (rc) return rc;
    FgicpTarget* T = nullptr;
    rc = find_target(c, slot, who, &T);
    if (rc) return rc;
    rc = check_cloud(c, who, source, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = stage_records(c, source, n, stride, fmt, c->vg_raw, raw);
    if (rc) return rc;
    float bb[6];
    int m = 0;
    rc = vg_distributions(c, who, *raw, n, P->k_correspondences, P->plane_epsilon, 0.f, bb, &m, nullptr, nullptr);
    if (rc) return rc;
    HIPCHK(c, c->fg_pair.ensure(sizeof(int) * (size_t)m));
    HIPCHK(c, c->fg_M.ensure(sizeof(double) * 6 * (size_t)m));
    HIPCHK(c, c->fg_d2.ensure(sizeof(double) * (size_t)m));
    r->c = c; r->T = T; r->src = c->vg_pts.as<float4>(); r->cov = c->vg_cov.as<double>(); r->n = m;
    r->max_d = P->max_correspondence_distance;
    return LISREG_OK;
}

}  // namespace

// the one copy of the checks, for lisreg_fgicp_batch.hip
int lisreg::fg_check_params(lisreg_ctx* c, const lisreg_fgicp_params* P, const char* who) { return check_params(c, P, who); }
int lisreg::fg_find_target(lisreg_ctx* c, int slot, const char* who, FgicpTarget** out) { return find_target(c, slot, who, out); }

FgTarget lisreg::fg_target_view(const FgicpTarget& G)
{
    FgTarget A;
    A.sorted = G.sorted.as<float4>(); A.cell_start = G.cells.as<int>(); A.cov = G.cov.as<double>();
    A.ox = G.grid.ox; A.oy = G.grid.oy; A.oz = G.grid.oz; A.cell = G.grid.cell; A.nx = G.grid.nx; A.ny = G.grid.ny; A.nz = G.grid.nz;
    for (int k = 0; k < 3; ++k) { A.b0[k] = (double)G.bb[k]; A.b1[k] = (double)G.bb[3 + k]; }
    return A;
}

extern "C" {

int lisreg_fgicp_default_params(int kind, lisreg_fgicp_params* p)
{
    if (!p || (kind != 0 && kind != 1)) return LISREG_ERR_ARG;
    *p = lisreg_fgicp_params{ kind == 1 ? (double)FLT_MAX : 5.0, 0.01, 2.0e-3, 1.0e-9, 1.0e-3, 20, 50, 10, 0 };
    return LISREG_OK;
}

int lisreg_fgicp_set_target(lisreg_ctx* c, int slot, const void* cloud, int n, int stride, int fmt, const lisreg_fgicp_params* P,
                            lisreg_fgicp_info* info, float cell_edge)
{
    if (!c) return LISREG_ERR_ARG;
    if (slot < 0 || slot > 65535) return bad(c, "fgicp_set_target: bad slot");
    int rc = check_params(c, P, "fgicp_set_target");
    if (rc) return rc;
    if (!(cell_edge >= 0.f) || !std::isfinite(cell_edge)) return bad(c, "fgicp_set_target: cell_edge < 0");
    rc = check_cloud(c, "fgicp_set_target", cloud, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    FgicpTarget& T = c->fgicp[slot];
    T.valid = false;
    const float4* raw = nullptr;
    rc = stage_records(c, cloud, n, stride, fmt, c->vg_raw, &raw);
    if (rc) return rc;
    int m = 0;
    GridIndex g;
    rc = vg_distributions(c, "fgicp_set_target", raw, n, P->k_correspondences, P->plane_epsilon, cell_edge, T.bb, &m, nullptr, &g);
    if (rc) return rc;
    // the context's scratch is overwritten by the next source: the slot keeps its own copies
    const size_t n_cells = (size_t)g.nx * (size_t)g.ny * (size_t)g.nz;
    HIPCHK(c, T.sorted.ensure(sizeof(float4) * (size_t)m));
    HIPCHK(c, T.cells.ensure(sizeof(int) * (n_cells + 1)));
    HIPCHK(c, T.orig.ensure(sizeof(int) * (size_t)m));
    HIPCHK(c, T.cov.ensure(sizeof(double) * 6 * (size_t)m));
    HIPCHK(c, hipMemcpyAsync(T.sorted.p, c->vg_sorted.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(T.cells.p, c->vg_cells.p, sizeof(int) * (n_cells + 1), hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(T.orig.p, c->vg_idx.p, sizeof(int) * (size_t)m, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipMemcpyAsync(T.cov.p, c->vg_cov.p, sizeof(double) * 6 * (size_t)m, hipMemcpyDeviceToDevice, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ctx_prof_collect(c);
    T.grid = g; T.grid.pts = T.sorted.as<float4>(); T.grid.cell_start = T.cells.as<int>();
    T.n_points = m;
    if (info) { info->grid_dims[0] = g.nx; info->grid_dims[1] = g.ny; info->grid_dims[2] = g.nz; info->n_points = m; }
    T.valid = true;
    return LISREG_OK;
}

int lisreg_fgicp_correspondences(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_fgicp_params* P,
                                 const double T[16], int* index_out, double* sqdist_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!T || !index_out) return bad(c, "fgicp_correspondences: NULL T / index_out");
    FgRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "fgicp_correspondences", slot, source, n, stride, fmt, P, &r, &raw);
    if (rc) return rc;
    hipStream_t st = c->stream;
    rc = search(r, T, true);
    if (rc) return rc;
    HIPCHK(c, c->fg_rows_i.ensure(sizeof(int) * (size_t)n));
    HIPCHK(c, c->fg_rows_d.ensure(sizeof(double) * (size_t)n));
    k_fgicp_rows<<<(n + 255) / 256, 256, 0, st>>>(c->fg_pair.as<int>(), c->fg_d2.as<double>(), c->vg_flag.as<int>(), c->vg_pos.as<int>(), n,
                                                  r.T->sorted.as<float4>(), r.T->orig.as<int>(), c->fg_rows_i.as<int>(), c->fg_rows_d.as<double>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(index_out, c->fg_rows_i.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost, st));
    if (sqdist_out) HIPCHK(c, hipMemcpyAsync(sqdist_out, c->fg_rows_d.p, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    ctx_prof_collect(c);
    return LISREG_OK;
}

int lisreg_fgicp_linearize(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_fgicp_params* P,
                           const double T_pairs[16], const double* T_eval, int with_hessian, double out[28], long long* n_pairs)
{
    if (!c) return LISREG_ERR_ARG;
    if (!T_pairs || !out) return bad(c, "fgicp_linearize: NULL T_pairs / out");
    FgRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "fgicp_linearize", slot, source, n, stride, fmt, P, &r, &raw);
    if (rc) return rc;
    rc = search(r, T_pairs, false);
    if (rc) return rc;
    double o[kOut];
    rc = sums(r, T_eval ? T_eval : T_pairs, with_hessian != 0, o);
    if (rc) return rc;
    memcpy(out, o, sizeof(double) * 28);
    if (n_pairs) *n_pairs = (long long)o[28];
    ctx_prof_collect(c);
    return LISREG_OK;
}

int lisreg_fgicp_align(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_fgicp_params* P,
                       const float* guess, lisreg_fgicp_result* res, void* aligned_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!res) return bad(c, "fgicp_align: NULL result");
    FgRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "fgicp_align", slot, source, n, stride, fmt, P, &r, &raw);
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
