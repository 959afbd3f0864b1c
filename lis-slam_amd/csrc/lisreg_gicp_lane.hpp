// lisreg_gicp_lane.hpp — what one lane of PCL's GICP computes per outer iteration: FastGICP's search and pair matrix
// (lisreg_fgicp_lane.hpp, unchanged) and, with the pair and its M still in registers, the lane's 73 moment terms and its 1.0 for the
// pair count; the wavefront adds them (wave_sum) and lane 0 writes one partial record of 74 doubles.  Nothing per pair goes to memory.
// Kept apart from lisreg_gicp.hip and inlined, so that a batch unit built with -ffp-contract=off computes the same bits.  The order of
// the record is tests/gicp_ref.py's.  Not installed.
#pragma once
#include "lisreg_fgicp_lane.hpp"
#include "lisreg_gicp_host.hpp"

namespace lisreg {

constexpr int kGicpRec = gicp_host::kRec;
struct GicpCentre { double c[3]; };     // the centre of the target's finite bounding box: the moments are taken about it

// live: the lane has a source point (s, ca[6]); P = T_k.  out: the workgroup's partial record (lane 0 writes it).  Every lane of the
// wavefront must call.
__device__ __forceinline__ void gicp_moments_lane(bool live, const float4 s, const double* __restrict__ ca, const FgTarget& A, const FgPose& P,
                                                  double max_d, double max2, const GicpCentre& C, double* __restrict__ out)
{
    int    pair = -1;
    double m6[6] = { 0.0, 0.0, 0.0, 0.0, 0.0, 0.0 };
    if (live) fg_pairs_lane(s, ca, A, P, max_d, max2, &pair, m6, nullptr);
    double r[3] = { 0.0, 0.0, 0.0 }, yt[4] = { 0.0, 0.0, 0.0, 0.0 }, one = 0.0;
    if (pair >= 0) {
        double x0, x1, x2;
        fg_transform(P, s, x0, x1, x2);
        const float4 b = A.sorted[pair];
        r[0] = x0 - (double)b.x; r[1] = x1 - (double)b.y; r[2] = x2 - (double)b.z;
        yt[0] = x0 - C.c[0]; yt[1] = x1 - C.c[1]; yt[2] = x2 - C.c[2]; yt[3] = 1.0;
        one = 1.0;
    }
    // without a pair m6, r and yt are zero: every term below is 0.0
    const double M[3][3] = { { m6[0], m6[1], m6[2] }, { m6[1], m6[3], m6[4] }, { m6[2], m6[4], m6[5] } };
    double Mr[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) Mr[a] = (M[a][0] * r[0] + M[a][1] * r[1]) + M[a][2] * r[2];
    const bool writer = threadIdx.x == 0;
    double v = wave_sum((r[0] * Mr[0] + r[1] * Mr[1]) + r[2] * Mr[2]);
    if (writer) out[0] = v;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            v = wave_sum(Mr[a] * yt[b]);
            if (writer) out[1 + 4 * a + b] = v;
        }
    int q = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int b2 = b; b2 < 4; ++b2, ++q) {
            const double yy = yt[b] * yt[b2];
#pragma unroll
            for (int p = 0; p < 6; ++p) {
                v = wave_sum(m6[p] * yy);
                if (writer) out[13 + 10 * p + q] = v;
            }
        }
    v = wave_sum(one);
    if (writer) out[73] = v;
}

// ---- what the single call (lisreg_gicp.hip) and the batch (lisreg_gicp_batch.hip) share on the host, one copy each ----------------------
// the parameter checks of every GICP entry point (defined in lisreg_gicp.hip)
int gc_check_params(lisreg_ctx* c, const lisreg_gicp_params* P, const char* who);
// the centre of a slot's finite bounding box
inline GicpCentre gicp_centre_of(const FgicpTarget& T)
{
    GicpCentre C;
    for (int k = 0; k < 3; ++k) C.c[k] = ((double)T.bb[k] + (double)T.bb[3 + k]) / 2.0;
    return C;
}

}  // namespace lisreg
