// lisreg_gicp.hip — PCL's GeneralizedIterativeClosestPoint: the fifth verifier select_registration_method names
// (src/core/registration.cpp:137-146: "GICP", max correspondence distance 10, 30 iterations, transformation epsilon 1e-6).  The
// definition is tests/gicp_ref.py.  The distributions, the search and the pair matrices are FastGICP's (a GICP target IS a FastGICP
// slot).  What is new: within one outer iteration PCL fixes the pairs and their M and lets BFGS minimise a function that is an exact
// quadratic in the 12 entries of (R, t) — so the GPU makes ONE launch per outer iteration that searches, forms every pair's 73 moment
// terms in registers and leaves one partial record per wavefront, one launch adds the records in a fixed order, and the whole BFGS with
// its line search runs on the host over 74 doubles (lisreg_gicp_host.hpp).  One round trip per outer iteration; the same input gives
// the same bits.  No CPU fallback.
#include "lisreg_gicp_lane.hpp"
#include "lisreg_gicp_stepper.hpp"

#include <cmath>
#include <cstring>

using namespace lisreg;
using namespace lisreg::gicp_host;
using lisreg::vgicp_host::guess_to_T0;
using lisreg::vgicp_host::pose_of;

namespace {

// One finite source point per lane, one wavefront per workgroup, one partial record of 74 doubles per workgroup (gicp_moments_lane).
__global__ __launch_bounds__(64) void k_gicp_moments(const float4* __restrict__ src, const double* __restrict__ scov, int n, FgTarget A, FgPose P,
                                                     double max_d, double max2, GicpCentre C, double* __restrict__ part)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const int at = live ? i : 0;                                    // (n >= 1: a lane past the end reads point 0 and drops it)
    gicp_moments_lane(live, src[at], scov + (size_t)at * 6, A, P, max_d, max2, C, part + (size_t)blockIdx.x * kGicpRec);
}

// the partial records of one outer iteration added in a fixed order (sum_records)
__global__ __launch_bounds__(64) void k_gicp_total(const double* __restrict__ part, int n_part, double* __restrict__ out)
{
    double acc[kGicpRec];
    sum_records<kGicpRec>(part, n_part, acc);
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < kGicpRec; ++k) out[k] = acc[k];
}

void launch_gicp_total(const double* part, int n_part, double* out, hipStream_t st) { k_gicp_total<<<1, 64, 0, st>>>(part, n_part, out); }

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct GicpRun {
    lisreg_ctx*        c;
    const FgicpTarget* T;
    const float4*      src;      // the source's finite points, in input order: the lanes' order
    const double*      cov;
    int                n;
    double             max_d;
    GicpCentre         C;
};

// the checks and the staging every entry point with a source shares (as lisreg_fgicp_align's): the distributions end up in c->vg_pts /
// c->vg_cov
int stage_source(lisreg_ctx* c, const char* who, int slot, const void* source, int n, int stride, int fmt, const lisreg_gicp_params* P,
                 GicpRun* r, const float4** raw)
{
    int rc = gc_check_params(c, P, who);
    if (rc) return rc;
    FgicpTarget* T = nullptr;
    rc = fg_find_target(c, slot, who, &T);
    if (rc) return rc;
    rc = check_cloud(c, who, source, n, stride, fmt, kFmtPackable, false);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    rc = stage_records(c, source, n, stride, fmt, c->vg_raw, raw);
    if (rc) return rc;
    float bb[6];
    int m = 0;
    rc = vg_distributions(c, who, *raw, n, P->k_correspondences, P->gicp_epsilon, 0.f, bb, &m, nullptr, nullptr);
    if (rc) return rc;
    r->c = c; r->T = T; r->src = c->vg_pts.as<float4>(); r->cov = c->vg_cov.as<double>(); r->n = m;
    r->max_d = P->max_correspondence_distance;
    r->C = gicp_centre_of(*T);
    return LISREG_OK;
}

// one round: the search, the moments and their total at T, waited for
int moments_at(GicpRun& r, const double T[16], double rec[kGicpRec])
{
    lisreg_ctx* c = r.c;
    const int nb = (r.n + 63) / 64;
    const FgTarget A = fg_target_view(*r.T);
    const FgPose P = pose_of<FgPose>(T);
    return record_totals<kGicpRec>(c, nb, [&](double* part) {
        ctx_prof_mark(c, 1);                                       // lisreg_get_timing: "solve" = the search-and-moments launches, one interval each
        k_gicp_moments<<<nb, 64, 0, c->stream>>>(r.src, r.cov, r.n, A, P, r.max_d, r.max_d * r.max_d, r.C, part);
        ctx_prof_mark(c, 0);                                       // "assoc" = the fixed-order totals
    }, launch_gicp_total, true, rec);
}

}  // namespace

// the parameter checks of every GICP entry point, the batch's among them (declared in lisreg_gicp_lane.hpp)
int lisreg::gc_check_params(lisreg_ctx* c, const lisreg_gicp_params* P, const char* who)
{
    if (!P) return bad(c, std::string(who) + ": NULL params");
    if (!(P->max_correspondence_distance > 0)) return bad(c, std::string(who) + ": max_correspondence_distance <= 0");
    if (P->k_correspondences < 4 || P->k_correspondences > 32) return bad(c, std::string(who) + ": k_correspondences outside 4 .. 32");
    if (!(P->transformation_epsilon > 0) || !(P->rotation_epsilon > 0) || P->max_iters < 1 || P->max_inner_iters < 1 ||
        !(P->gicp_epsilon > 0 && P->gicp_epsilon <= 1))
        return bad(c, std::string(who) + ": bad transformation_epsilon / rotation_epsilon / max_iters / max_inner_iters / gicp_epsilon");
    if (!(P->rho > 0 && P->rho < 1) || !(P->sigma > 0 && P->sigma < 1) || !(P->tau1 > 1) || !(P->tau2 > 0 && P->tau2 < 1) ||
        !(P->tau3 > 0 && P->tau3 < 1) || !(P->step_size > 0) || !std::isfinite(P->step_size) || !(P->gradient_tol > 0) || P->order < 2 || P->order > 3)
        return bad(c, std::string(who) + ": bad rho / sigma / tau1 / tau2 / tau3 / step_size / gradient_tol / order");
    return LISREG_OK;
}

extern "C" {

int lisreg_gicp_default_params(int kind, lisreg_gicp_params* p)
{
    if (!p || (kind != 0 && kind != 1)) return LISREG_ERR_ARG;
    *p = lisreg_gicp_params{ 10.0, kind == 1 ? 1.0e-4 : 1.0e-6, 2.0e-3, 1.0e-3, 0.01, 0.01, 9.0, 0.05, 0.5, 0.01, 1.0e-2, 20, 30, 20, 3 };
    return LISREG_OK;
}

int lisreg_gicp_moments(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_gicp_params* P,
                        const double T[16], double out[74])
{
    if (!c) return LISREG_ERR_ARG;
    if (!T || !out) return bad(c, "gicp_moments: NULL T / out");
    GicpRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "gicp_moments", slot, source, n, stride, fmt, P, &r, &raw);
    if (rc) return rc;
    double rec[kGicpRec];
    rc = moments_at(r, T, rec);
    if (rc) return rc;
    memcpy(out, rec, sizeof rec);
    ctx_prof_collect(c);
    return LISREG_OK;
}

int lisreg_gicp_inner(const double moments[74], const double centre[3], const double x0[6], const lisreg_gicp_params* P, double x_out[6],
                      int counts[4], double* f_out)
{
    if (!moments || !centre || !x0 || !P || !x_out || !(moments[73] >= 1.0) || P->max_inner_iters < 1) return LISREG_ERR_ARG;
    double x[6];
    memcpy(x, x0, sizeof x);
    InnerCounts cnt;
    const double f = inner(moments, centre, x, bfgs_params_of(*P), &cnt);
    memcpy(x_out, x, sizeof x);
    if (counts) { counts[0] = cnt.iters; counts[1] = cnt.n_f; counts[2] = cnt.n_df; counts[3] = cnt.exit; }
    if (f_out) *f_out = f;
    return LISREG_OK;
}

int lisreg_gicp_align(lisreg_ctx* c, int slot, const void* source, int n, int stride, int fmt, const lisreg_gicp_params* P,
                      const float* guess, lisreg_gicp_result* res, void* aligned_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!res) return bad(c, "gicp_align: NULL result");
    GicpRun r;
    const float4* raw = nullptr;
    int rc = stage_source(c, "gicp_align", slot, source, n, stride, fmt, P, &r, &raw);
    if (rc) return rc;
    double G[16];
    guess_to_T0(guess, G);
    GicpLoopResult lr;                                              // computeTransformation: one round per outer iteration (GicpStepper)
    rc = gicp_closed_loop([&](const double T[16], double rec[kGicpRec]) { return moments_at(r, T, rec); }, G, gicp_loop_params_of(*P), r.C.c, &lr);
    if (rc) return rc;
    ctx_prof_collect(c);
    lisreg_gicp_result out;
    gicp_result_to(lr, &out);
    *res = out;
    if (aligned_out) {                                    // the source under the final transformation (in float, like lisreg_transform_cloud)
        float F[12];
        for (int k = 0; k < 12; ++k) F[k] = (float)out.final_transform[k];
        return emit_aligned(c, raw, n, F, source, stride, fmt, c->vg_sorted, aligned_out);
    }
    return LISREG_OK;
}

}  // extern "C"
