// lisreg_motion.hip — constant-velocity motion compensation of a sweep: the kernel of lisreg_adjust_cloud / lisreg_adjust_cloud_batch
// (entry points: lisreg_api_motion.hip).
//
// Replaces DistortionAdjust::SetMotionInfo, AdjustCloud and UpdateMatrix (src/core/distortionAdjust.cpp:412-417, 419-469, 471-480).
// Restated from knowledge of the C++ expressions and of Eigen's, operation for operation (tests/adjust_ref.py is the yardstick and says
// which reading of Eigen this is, and that it could not be checked against Eigen itself); per point i >= 1, in input order:
//   1. real_time = (float)((double)time - (double)scan_period / 2.0)                                              (:447)
//   2. angle = angular_rate * real_time, three float products                                                      (:473)
//   3. three AngleAxisf -> Quaternionf: ha = 0.5f * angle, w = cosf(ha), vec = sinf(ha) * axis (products with the axis' 0 / 1 entries:
//      the zeros keep their sign); (qz * qy) * qx, two Hamilton products in Eigen's scalar order, left to right              (:474-478)
//   4. quaternion -> AngleAxisf (Eigen 3.3): n = sqrtf(x*x + (y*y + z*z)); n < FLT_EPSILON: stableNorm; n != 0: angle = 2 atan2f(n, |w|),
//      n = -n if w < 0, axis = vec / n; else angle 0, axis (1, 0, 0)
//   5. toRotationMatrix: sin_axis = sinf(angle) * axis, cos1_axis = (1 - cosf(angle)) * axis, the three tmp -+ sin_axis pairs, diagonal
//      cos1_axis * axis + cosf(angle)                                                                              (:479)
//   6. out = ((R[r][0] * x + R[r][1] * y) + R[r][2] * z) + velocity[r] * real_time                                  (:454-455)
//   7. payload (ring) and time copied bit for bit                                                                  (:460-462)
// A float libm function is DEFINED as the correctly rounded value — the double function rounded once to float — as in
// lisreg_pretreat.hip; sqrtf and the float division are exact by IEEE; no contraction (csrc/Makefile).
//
// gfx950 mapping: one lane per output point, 256-thread workgroups, ONE launch for one sweep or for 256: a workgroup finds its sweep in
// the job table by its first-workgroup number.  20 bytes read and 20 written per point (a 16-byte record and a time, both by whole
// vector loads / stores, coalesced: lane i reads record i + 1 and writes record i); eight fp64 sin / cos and one atan2 per point on
// top of it, so the kernel is bound by the fp64 pipe, not by HBM.
#include "lisreg_internal.hpp"

#include <cfloat>

namespace lisreg {

namespace {

struct Quat { float w, x, y, z; };

__device__ __forceinline__ float sin_cr(float a) { return (float)sin((double)a); }
__device__ __forceinline__ float cos_cr(float a) { return (float)cos((double)a); }

__device__ __forceinline__ Quat axis_quat(float angle, float ax, float ay, float az)
{
    const float ha = 0.5f * angle, s = sin_cr(ha);
    return Quat{ cos_cr(ha), s * ax, s * ay, s * az };
}

__device__ __forceinline__ Quat quat_mul(const Quat& a, const Quat& b)
{
    return Quat{ a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z,
                 a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                 a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                 a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x };
}

__device__ __forceinline__ const AdjustJob& job_of(const AdjustJob& one, const AdjustJob* __restrict__ tab, int n_jobs, int blk)
{
    if (!tab) return one;
    int a = 0, b = n_jobs - 1;                                          // last job whose first workgroup is <= blk: jobs without a
    while (a < b) { const int mid = (a + b + 1) >> 1; if (tab[mid].blk0 <= blk) a = mid; else b = mid - 1; }      // workgroup share the next one's number
    return tab[a];
}

__global__ __launch_bounds__(256) void k_adjust_cloud(AdjustJob one, const AdjustJob* __restrict__ tab, int n_jobs)
{
    const AdjustJob& j = job_of(one, tab, n_jobs, blockIdx.x);
    const int i = (blockIdx.x - j.blk0) * 256 + threadIdx.x;            // output index; input index i + 1
    if (i < 0 || i >= j.n_out) return;
    const float4 p = j.src[i + 1];
    const float t = j.time[i + 1];
    const float rt = (float)((double)t - (double)j.scan_period / 2.0);
    const Quat qz = axis_quat(j.rate[2] * rt, 0.0f, 0.0f, 1.0f), qy = axis_quat(j.rate[1] * rt, 0.0f, 1.0f, 0.0f),
               qx = axis_quat(j.rate[0] * rt, 1.0f, 0.0f, 0.0f);
    const Quat q = quat_mul(quat_mul(qz, qy), qx);
    float n = sqrtf(q.x * q.x + (q.y * q.y + q.z * q.z));
    if (n < FLT_EPSILON) {                                              // stableNorm
        float m = fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fabsf(q.z));
        if (m > 0.0f) {
            float inv = 1.0f / m;
            if (inv > FLT_MAX) { inv = FLT_MAX; m = 1.0f / FLT_MAX; }
            const float sx = q.x * inv, sy = q.y * inv, sz = q.z * inv;
            n = m * sqrtf(sx * sx + (sy * sy + sz * sz));
        } else n = 0.0f;
    }
    float angle = 0.0f, ax = 1.0f, ay = 0.0f, az = 0.0f;
    if (n != 0.0f) {
        angle = 2.0f * (float)atan2((double)n, (double)fabsf(q.w));
        if (q.w < 0.0f) n = -n;
        ax = q.x / n; ay = q.y / n; az = q.z / n;
    }
    const float s = sin_cr(angle), c = cos_cr(angle);
    const float sx = s * ax, sy = s * ay, sz = s * az;
    const float k1 = 1.0f - c;
    const float cx = k1 * ax, cy = k1 * ay, cz = k1 * az;
    const float t01 = cx * ay, t02 = cx * az, t12 = cy * az;
    const float R00 = cx * ax + c, R01 = t01 - sz, R02 = t02 + sy;
    const float R10 = t01 + sz, R11 = cy * ay + c, R12 = t12 - sx;
    const float R20 = t02 - sy, R21 = t12 + sx, R22 = cz * az + c;
    float4 o;
    o.x = ((R00 * p.x + R01 * p.y) + R02 * p.z) + j.vel[0] * rt;
    o.y = ((R10 * p.x + R11 * p.y) + R12 * p.z) + j.vel[1] * rt;
    o.z = ((R20 * p.x + R21 * p.y) + R22 * p.z) + j.vel[2] * rt;
    o.w = p.w;
    j.dst[i] = o;
    if (j.dst_time) j.dst_time[i] = t;
}

}  // namespace

int adjust_blocks(AdjustJob* jobs, int n_jobs)
{
    int blocks = 0;
    for (int s = 0; s < n_jobs; ++s) { jobs[s].blk0 = blocks; blocks += (jobs[s].n_out + 255) / 256; }
    return blocks;
}

void launch_adjust_cloud(const AdjustJob& one, const AdjustJob* tab_dev, int n_jobs, int blocks, hipStream_t st)
{
    if (blocks > 0) k_adjust_cloud<<<blocks, 256, 0, st>>>(one, tab_dev, n_jobs);
}

}  // namespace lisreg
