// lisreg_jacobi3.hpp — eigen-decomposition of a symmetric 3 x 3 in double by cyclic Jacobi sweeps, for device code: every index is a
// compile-time constant, so matrix and vectors stay in registers.  Shared by the voxel Gaussians of lisreg_ndt.hip and the point
// distributions of lisreg_vgicp.hip.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

namespace lisreg {

#define LISREG_JACOBI3_ROT(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)                       \
    if (apq != 0.0) {                                                                                     \
        const double th = (aqq - app) / (2.0 * apq);                                                      \
        const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));                    \
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;                                           \
        app -= t * apq; aqq += t * apq; apq = 0.0;                                                        \
        const double rp = cs * arp - sn * arq, rq = sn * arp + cs * arq; arp = rp; arq = rq;              \
        double x;                                                                                         \
        x = cs * v0p - sn * v0q; v0q = sn * v0p + cs * v0q; v0p = x;                                      \
        x = cs * v1p - sn * v1q; v1q = sn * v1p + cs * v1q; v1p = x;                                      \
        x = cs * v2p - sn * v2q; v2q = sn * v2p + cs * v2q; v2p = x;                                      \
    }

// On return a00, a11, a22 are the eigenvalues (the off-diagonal entries are zero or negligible) and the columns of v the eigenvectors:
// eigenvalue a00 belongs to (v00, v10, v20).  At most 40 sweeps; a NaN entry ends the sweeps at once.
__device__ __forceinline__ void jacobi3(double& a00, double& a01, double& a02, double& a11, double& a12, double& a22,
                                        double& v00, double& v01, double& v02, double& v10, double& v11, double& v12,
                                        double& v20, double& v21, double& v22)
{
    v00 = 1; v01 = 0; v02 = 0; v10 = 0; v11 = 1; v12 = 0; v20 = 0; v21 = 0; v22 = 1;
    for (int sweep = 0; sweep < 40; ++sweep) {
        const double off = fabs(a01) + fabs(a02) + fabs(a12);
        if (!(off > 1.0e-22 * (fabs(a00) + fabs(a11) + fabs(a22)))) break;         // also ends on NaN
        LISREG_JACOBI3_ROT(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
        LISREG_JACOBI3_ROT(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
        LISREG_JACOBI3_ROT(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
    }
}

}  // namespace lisreg
