// lisreg_loop.hip — loop-closure candidate detection: EPSCGeneration::loopDetection (src/core/epscGeneration.cpp:663-992) with
// any of its seven selectors (ISC, SC, EPSC, SEPSC, FEPSC, SSC, Pose; FEPSC alone is config/params.yaml:22-28's default).  The host
// applies the pose / travel gate (:686-745) in double; everything after it is one launch sequence over every (frame, candidate) pair
// of a call:
//   k_loop_project  one workgroup per frame: project() (:84-120), the 1 x 360 table of (count, x, y, label) of labels
//                   {13, 14, 16, 18, 19}; "the last point wins" is the largest point index per sector, gathered afterwards;
//   k_loop_icp      one workgroup per gated pair: globalICP (:258-401) — the 60-shift yaw search on the counts, the two sector
//                   clouds in LDS, pcl::IterativeClosestPoint with PCL's defaults (10 iterations, no distance cap, transformation
//                   epsilon 0, relative MSE -DBL_MAX) by brute-force k = 1 (FLANN L2_Simple order, ties to the smaller index) and
//                   the shared Umeyama step (lisreg_icp_step.hpp); result trans * trans1;
//   k_loop_bin      the hot path: the whole current frame (corner, surf, semantic) moved by the pair's matrix and binned into four
//                   20 x 80 integer histograms in LDS (EPSC corner / surf, SEPSC 40|50 / 81), merged with integer atomics; with SC,
//                   ISC or SSC enabled (the template instance k_loop_bin<true>) also, per cell, the last point whose SC / ISC value
//                   resets the cell (an index-keyed atomicMax) and the largest SSC order;
//   k_loop_fold     (SC or ISC only) the semantic cloud again: per cell the largest in-range value after the last reset;
//   k_loop_finish   the uchar counters (mod 256), 100 * psc / (1 + esc) in int (mod 256), FEPSC = (uchar)(0.4 s + 0.6 e) in double;
//                   SC / ISC = max(the reset value or 0, the later in-range maximum), SSC = the label of the largest order;
//   k_loop_score    per (pair, enabled kind): calculateDistance (:633-660), shifts -10 .. 9, first strict minimum, or
//                   calculateLabelSim (:611-631) for SSC;
//   k_loop_select   per frame and kind, the first strict maximum above the threshold (Pose: the first strict minimum of the gate
//                   distance), the transforms of :771-890 and the matched list in push order (:894-990).
// The frame's own (untransformed) descriptor is the identity pair of the same launch and goes straight into the database, so a
// batch of K frames can match frames earlier in the same batch.  Compiled -ffp-contract=off: every float / double operation rounds
// on its own like the reference's x86 build.
// Deviation from the reference: globalICP wraps j + i once (`if (new_col >= sectors) new_col -= sectors`), which for a
// wrapped yaw above 331 sectors (a slightly negative yaw difference) reads past the 360-entry row — undefined behaviour.  Here the
// column is wrapped modulo 360.  SSC labels >= 20 (past order_vec, undefined behaviour) count as order 0; ISC needs host structs
// (device records carry the label, not the intensity).
#include "lisreg_ctx.hpp"
#include "lisreg_icp_step.hpp"

#include <cfloat>
#include <climits>
#include <cmath>
#include <cstring>

namespace lisreg {

namespace {

constexpr int    kRings = 20, kSectors = 80, kCells = kRings * kSectors, kProj = 360;
constexpr int    kHist = 4 * kCells;                 // EPSC esc (corner), EPSC psc (surf), SEPSC psc (40 | 50), SEPSC esc (81)
constexpr int    kLoopAcc = 17;                      // icp_solve_step's sums: count, sum p (3), sum q (3), sum q_r p_c (9), sum d2
constexpr int    kBinChunk = 4096;                   // points of one pair per binning workgroup
constexpr double kMaxDis = 60.0, kMinDis = 3.0;
constexpr double kRingStep = (kMaxDis - kMinDis) / kRings;       // epscGeneration.h:42
constexpr double kSectorStep = 2 * M_PI / kSectors;              // epscGeneration.h:43
constexpr float  kStep360 = (float)(2. * M_PI / 360.f);          // project() / globalICP: float step = 2. * M_PI / sectors_range
// config/label.yaml using_label (a std::map: labels without an entry map to 0): 40 or 50 -> psc, 81 -> esc
constexpr unsigned kPscLabels = (1u << 9) | (1u << 10) | (1u << 11) | (1u << 13) | (1u << 14);
constexpr unsigned kEscLabels = (1u << 16) | (1u << 18) | (1u << 19);
constexpr unsigned kProjLabels = (1u << 13) | (1u << 14) | (1u << 16) | (1u << 18) | (1u << 19);

// the seven selectors by kind index (bit position of LISREG_LOOP_*), and the descriptor slots of a pair: FEPSC, EPSC, SEPSC are
// always computed (slots 0 - 2); SC, ISC, SSC (slots 3 - 5) only when one of them is enabled
enum { kIsc = 0, kSc, kEpsc, kSepsc, kFepsc, kSsc, kPose, kKinds };
constexpr int      kDescKinds = 6;
constexpr int      kSlotOf[kDescKinds] = { 4, 3, 1, 2, 0, 5 };                     // kind index -> descriptor slot
constexpr unsigned kFoldKinds = LISREG_LOOP_ISC | LISREG_LOOP_SC | LISREG_LOOP_SSC;  // the kinds k_loop_bin<true> is for
// order_vec (epscGeneration.h:24-25) for labels 0 .. 19; labels >= 20 (past the vector: undefined behaviour) count as order 0
__constant__ int kOrder[20] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 11, 12, 13, 15, 16, 14, 17, 9, 18, 19 };
__constant__ int kLabelOfOrder[20] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 17, 9, 10, 11, 12, 15, 13, 14, 16, 18, 19 };
// per pair, the fold state of k_loop_bin<true> / k_loop_fold (zeroed each call; 0 = nothing yet)
struct LoopFold {
    unsigned           reset[2][kCells];     // SC, ISC: ((index + 1) << 8) | the byte the last resetting point stores
    int                maxv[2][kCells];      // SC: value + 129, ISC: value + 1 — the largest in-range value after that reset
    int                order[kCells];        // SSC: the largest order_vec value of a point in the cell
};

struct LoopFrame {
    const float4* pts[3];    // corner, surf, semantic (16-B records, label in the payload of the semantic ones)
    const float*  inten;     // ISC: the semantic cloud's intensities (host structs only), or null
    float4*       proj;      // where k_loop_project writes the frame's 360 sectors
    uint8_t*      db[kDescKinds];     // per descriptor slot, where the identity pair's descriptor goes (the database), or null
    int           n[3];
    int           has_M;     // lisreg_loop_descriptor with a matrix: the identity pair moves the clouds by M
    int           frame_id, cand0, n_cand, pad_;
    float         M[16];
};
struct LoopPair {
    int    frame, hist, kind, tmp_id;                    // kind 0: the frame's own descriptor, 1: a gated candidate
    float  yaw;                                          // yaw difference wrapped into [0, 2 pi) (float, as globalICP)
    float  yaw_diff;                                     // the same, unwrapped (EPSC's initial angle, :817)
    double pos_distance;                                 // the gate's distance (Pose)
};
struct LoopPairOut {
    float  T[16];
    float  yaw_angle;
    int    yaw_shift, state, iters, n_corr, score_shift;
    double score;
    double kscore[kDescKinds];                           // per kind index ISC .. SSC (enabled kinds only)
    int    kshift[kDescKinds];
};
// what k_loop_score scores: the enabled descriptor kinds and their databases
struct LoopScoreKinds {
    const uint8_t* db[kDescKinds];                       // per kind index
    int            kind[kDescKinds];                     // blockIdx.y -> kind index
};

__device__ __forceinline__ void apply_m(const float* M, float x, float y, float z, float& ox, float& oy, float& oz)
{
    ox = ((M[0] * x + M[1] * y) + M[2] * z) + M[3];      // mat4_apply / icp.hpp transformCloud order
    oy = ((M[4] * x + M[5] * y) + M[6] * z) + M[7];
    oz = ((M[8] * x + M[9] * y) + M[10] * z) + M[11];
}

__device__ __forceinline__ int label_of(float4 p) { return (int)(__float_as_uint(p.w) & 0xffffu); }

// project(): counts per sector, last point (largest index) per sector
__global__ __launch_bounds__(1024) void k_loop_project(const LoopFrame* __restrict__ frames)
{
    __shared__ int cnt[kProj], last[kProj];
    const LoopFrame& F = frames[blockIdx.x];
    for (int s = threadIdx.x; s < kProj; s += blockDim.x) { cnt[s] = 0; last[s] = -1; }
    __syncthreads();
    const float4* pts = F.pts[2];
    const int n = F.n[2];
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float4 p = pts[i];
        const int lab = label_of(p);
        if (lab >= 32 || !((kProjLabels >> lab) & 1u)) continue;
        float x = p.x, y = p.y, z = p.z;
        if (F.has_M) apply_m(F.M, p.x, p.y, p.z, x, y, z);
        const float dist = sqrtf(x * x + y * y);
        if (!(dist == dist) || (double)dist < 1e-2) continue;           // NaN: the reference's cast gives INT_MIN, skipped
        const float angle = (float)(M_PI + (double)atan2f(y, x));
        const int s = (int)floorf(angle / kStep360);
        if (s >= kProj || s < 0) continue;
        atomicAdd(&cnt[s], 1);
        atomicMax(&last[s], i);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < kProj; s += blockDim.x) {
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cnt[s] > 0) {
            const float4 p = pts[last[s]];
            float x = p.x, y = p.y, z = p.z;
            if (F.has_M) apply_m(F.M, p.x, p.y, p.z, x, y, z);
            o = make_float4((float)cnt[s], x, y, (float)label_of(p));
        }
        F.proj[s] = o;
    }
}

__device__ __forceinline__ double wave_sum_d(double v)
{
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// globalICP for one gated pair: yaw search, sector clouds, PCL-default ICP, trans * trans1
__global__ __launch_bounds__(256) void k_loop_icp(const LoopPair* __restrict__ pairs, int cand0, const LoopFrame* __restrict__ frames,
                                                  const float4* __restrict__ db_proj, LoopPairOut* __restrict__ pout)
{
    __shared__ float4 sh[kProj], sc[kProj], tgt[kProj], cur[kProj];
    __shared__ float dis[60];
    __shared__ double red[4][kLoopAcc], tot[kLoopAcc];
    __shared__ IcpState st;
    __shared__ float s_angle;
    __shared__ int s_shift, s_nt, s_ns;
    const int p = cand0 + (int)blockIdx.x;
    const LoopPair P = pairs[p];
    const float4* hp = db_proj + (size_t)P.hist * kProj;
    const float4* cp = frames[P.frame].proj;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < kProj; j += 256) { sh[j] = hp[j]; sc[j] = cp[j]; }
    __syncthreads();
    if (tid < 60) {
        const int i = P.tmp_id - 30 + tid;
        float dc = 0.f;                                   // the reference's float sum, in its order (exact: small integers)
        for (int j = 0; j < kProj; ++j) {
            int nc = (j + i) % kProj;                      // modulo 360 (the reference wraps once: see the header)
            if (nc < 0) nc += kProj;
            dc += fabsf(sh[j].x - sc[nc].x);
        }
        dis[tid] = dc;
    }
    __syncthreads();
    if (tid == 0) {
        double sim = 100000;
        float angle = P.yaw;
        int shift = LISREG_LOOPDET_NO_SHIFT;
        for (int t = 0; t < 60; ++t)
            if ((double)dis[t] < sim) { sim = dis[t]; shift = P.tmp_id - 30 + t; angle = (float)shift; }
        s_angle = angle * kStep360;
        s_shift = shift;
    }
    __syncthreads();
    const float angle = s_angle;
    if (wave == 0) {
        // cloud 1 (target): history sectors with a label; cloud 2 (source): current ones rotated by the search's angle; sector order
        const float cs = cosf(angle), sn = sinf(angle);
        int nt = 0, ns = 0;
        for (int b = 0; b < kProj; b += 64) {
            const int j = b + lane;
            const bool f1 = j < kProj && sh[j].w > 0.f, f2 = j < kProj && sc[j].w > 0.f;
            const unsigned long long m1 = __ballot(f1), m2 = __ballot(f2), lt = (1ull << lane) - 1ull;
            if (f1) tgt[nt + __popcll(m1 & lt)] = make_float4(sh[j].y, sh[j].z, 0.f, 0.f);
            if (f2) {
                const float x = sc[j].y, y = sc[j].z;
                cur[ns + __popcll(m2 & lt)] = make_float4(x * cs - y * sn, x * sn + y * cs, 0.f, 0.f);
            }
            nt += __popcll(m1); ns += __popcll(m2);
        }
        if (lane == 0) {
            s_nt = nt; s_ns = ns;
            for (int k = 0; k < 16; ++k) { st.F[k] = (k % 5 == 0) ? 1.f : 0.f; st.Tm[k] = st.F[k]; }
            st.iters = 0; st.done = 0; st.state = LISREG_ICP_NOT_CONVERGED; st.converged = 0; st.n_corr = 0; st.fit_n = 0;
            st.prev_mse = DBL_MAX; st.cur_mse = DBL_MAX; st.fit_sum = 0; st.first_mse = -1.0; st.defer_first = 0; st.pad_ = 0;
        }
    }
    __syncthreads();
    const int nt = s_nt, ns = s_ns;
    for (;;) {
        double v[kLoopAcc];
#pragma unroll
        for (int k = 0; k < kLoopAcc; ++k) v[k] = 0.0;
        for (int i = tid; i < ns; i += 256) {
            const float4 q = cur[i];
            float best = __builtin_inff();
            int bj = -1;
            for (int j = 0; j < nt; ++j) {
                const float4 c = tgt[j];
                const float ex = q.x - c.x, ey = q.y - c.y, ez = q.z - c.z;
                const float d2 = ex * ex + ey * ey + ez * ez;      // flann::L2_Simple order; ascending j: ties keep the smaller index
                if (d2 < best) { best = d2; bj = j; }
            }
            if (bj >= 0) {
                const float4 t = tgt[bj];
                const float fa[4] = { 1.f, t.x, t.y, t.z }, fb[4] = { 1.f, q.x, q.y, q.z };
                // 0 count, 1-3 sum p (source), 4-6 sum q (target), 7-15 sum q_r p_c, 16 sum d2 (icp_solve_step's layout)
                v[0] += 1.0;
                for (int c = 1; c < 4; ++c) v[c] += (double)fb[c];
                for (int r = 1; r < 4; ++r) v[3 + r] += (double)fa[r];
                for (int r = 1; r < 4; ++r) for (int c = 1; c < 4; ++c) v[7 + 3 * (r - 1) + (c - 1)] += (double)fa[r] * (double)fb[c];
                v[16] += (double)best;
            }
        }
#pragma unroll
        for (int k = 0; k < kLoopAcc; ++k) {
            const double w = wave_sum_d(v[k]);
            if (lane == 0) red[wave][k] = w;
        }
        __syncthreads();
        if (tid < kLoopAcc) tot[tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
        __syncthreads();
        if (tid == 0) icp_solve_step(tot, &st, 10, 0.0, -DBL_MAX);
        __syncthreads();
        if (st.done) break;
        for (int i = tid; i < ns; i += 256) {
            const float4 q = cur[i];
            float x, y, z;
            apply_m(st.Tm, q.x, q.y, q.z, x, y, z);
            cur[i] = make_float4(x, y, z, 0.f);
        }
        __syncthreads();
    }
    if (tid == 0) {
        // trans1 = Identity().rotate(AngleAxisf(angle, UnitZ())) (Eigen's toRotationMatrix for the z axis), then trans * trans1
        const float c = cosf(angle), s = sinf(angle);
        const float R[9] = { c, -s, 0.f, s, c, 0.f, 0.f, 0.f, (1.f - c) + c };
        LoopPairOut& o = pout[p];
        for (int r = 0; r < 3; ++r) {
            for (int k = 0; k < 3; ++k)
                o.T[4 * r + k] = (st.F[4 * r] * R[k] + st.F[4 * r + 1] * R[3 + k]) + st.F[4 * r + 2] * R[6 + k];
            o.T[4 * r + 3] = st.F[4 * r + 3];
        }
        o.T[12] = 0.f; o.T[13] = 0.f; o.T[14] = 0.f; o.T[15] = 1.f;
        o.yaw_angle = angle; o.yaw_shift = s_shift;
        o.state = st.state; o.iters = st.iters; o.n_corr = st.n_corr;
    }
}

// calculateEPSC's bin of a moved point (ring * 80 + sector), or -1 when it is skipped
__device__ __forceinline__ int bin_of(float x, float y)
{
    const double d = (double)sqrtf(x * x + y * y);
    if (!(d == d) || d >= kMaxDis || d < kMinDis) return -1;
    const int ring = (int)floor((d - kMinDis) / kRingStep);
    const double angle = M_PI + (double)atan2f(y, x);
    const int sector = (int)floor(angle / kSectorStep);
    if (ring >= kRings || ring < 0 || sector >= kSectors || sector < 0) return -1;
    return ring * kSectors + sector;
}

// (int) of a double / float as the reference's x86 build converts it (cvttsd2si / cvttss2si): NaN and out-of-range give INT_MIN.
// gfx950's v_cvt_i32_f* saturate and map NaN to 0, so the range is tested first.
__device__ __forceinline__ int x86_int(double t) { return (t > -2147483649.0 && t < 2147483648.0) ? (int)t : INT_MIN; }
__device__ __forceinline__ int x86_int(float t) { return (t >= -2147483648.f && t < 2147483648.f) ? (int)t : INT_MIN; }
// calculateSC's z_temp (LIDAR_HEIGHT 5.0, in double) and calculateISC's intensity_temp (255 * intensity, a float product)
__device__ __forceinline__ int sc_value(float z) { return x86_int(100.0 * ((double)z + 5.0) / 8.0); }
__device__ __forceinline__ int isc_value(float intensity) { return x86_int(255.f * intensity); }

// the three clouds of a pair's frame, moved by the pair's matrix, into 4 x 1600 integer counters (LDS, then global atomics).
// kFold (SC, ISC or SSC enabled): every semantic point is binned, and per cell the last resetting SC / ISC point (`(signed char)
// s < v` with v >= 128, `(uchar) s < v` with v >= 256 always store v's low byte) and the largest SSC order are kept as well.
template <bool kFold>
__global__ __launch_bounds__(256) void k_loop_bin(const LoopPair* __restrict__ pairs, const LoopFrame* __restrict__ frames,
                                                  const LoopPairOut* __restrict__ pout, int* __restrict__ hist, LoopFold* __restrict__ fold,
                                                  unsigned kinds)
{
    __shared__ int h[kHist];
    __shared__ float sM[16];
    const int p = blockIdx.x;
    const LoopPair P = pairs[p];
    const LoopFrame& F = frames[P.frame];
    const int n0 = F.n[0], n1 = F.n[1], n2 = F.n[2];
    const long long total = (long long)n0 + n1 + n2;
    const long long base = (long long)blockIdx.y * kBinChunk;
    if (base >= total) return;
    const bool moved = P.kind == 1 || F.has_M;
    for (int k = threadIdx.x; k < kHist; k += 256) h[k] = 0;
    if (threadIdx.x < 16) sM[threadIdx.x] = P.kind == 1 ? pout[p].T[threadIdx.x] : F.M[threadIdx.x];
    if constexpr (!kFold) {
        __syncthreads();
        const int end = (int)(total - base < kBinChunk ? total - base : kBinChunk);
        for (int l = threadIdx.x; l < end; l += 256) {
            const long long g = base + l;
            int cl, i;
            if (g < n0) { cl = 0; i = (int)g; } else if (g < (long long)n0 + n1) { cl = 1; i = (int)(g - n0); } else { cl = 2; i = (int)(g - n0 - n1); }
            const float4 q = F.pts[cl][i];
            int slot;
            if (cl == 2) {
                const int lab = label_of(q);
                if (lab >= 32) continue;
                slot = ((kPscLabels >> lab) & 1u) ? 2 : (((kEscLabels >> lab) & 1u) ? 3 : -1);
                if (slot < 0) continue;
            } else {
                slot = cl;
            }
            float x = q.x, y = q.y, z = q.z;
            if (moved) apply_m(sM, q.x, q.y, q.z, x, y, z);
            const int cell = bin_of(x, y);
            if (cell < 0) continue;
            atomicAdd(&h[slot * kCells + cell], 1);
        }
        __syncthreads();
    } else {
        __shared__ unsigned rk[2][kCells];
        __shared__ int ord[kCells];
        for (int k = threadIdx.x; k < kCells; k += 256) { rk[0][k] = 0; rk[1][k] = 0; ord[k] = 0; }
        __syncthreads();
        const bool want_sc = kinds & LISREG_LOOP_SC, want_isc = kinds & LISREG_LOOP_ISC, want_ssc = kinds & LISREG_LOOP_SSC;
        const int end = (int)(total - base < kBinChunk ? total - base : kBinChunk);
        for (int l = threadIdx.x; l < end; l += 256) {
            const long long g = base + l;
            int cl, i;
            if (g < n0) { cl = 0; i = (int)g; } else if (g < (long long)n0 + n1) { cl = 1; i = (int)(g - n0); } else { cl = 2; i = (int)(g - n0 - n1); }
            const float4 q = F.pts[cl][i];
            int slot = cl, lab = 0;
            if (cl == 2) {
                lab = label_of(q);
                slot = lab >= 32 ? -1 : ((kPscLabels >> lab) & 1u) ? 2 : (((kEscLabels >> lab) & 1u) ? 3 : -1);
            }
            float x = q.x, y = q.y, z = q.z;
            if (moved) apply_m(sM, q.x, q.y, q.z, x, y, z);
            const int cell = bin_of(x, y);
            if (cell < 0) continue;
            if (slot >= 0) atomicAdd(&h[slot * kCells + cell], 1);
            if (cl != 2) continue;
            const unsigned key = (unsigned)(i + 1) << 8;                  // i + 1 < 2^24 (run_launch)
            if (want_sc) {
                const int v = sc_value(z);
                if (v >= 128) atomicMax(&rk[0][cell], key | (unsigned)(v & 255));
            }
            if (want_isc) {
                const int v = isc_value(F.inten[i]);
                if (v >= 256) atomicMax(&rk[1][cell], key | (unsigned)(v & 255));
            }
            if (want_ssc && lab < 20 && kOrder[lab] > 0) atomicMax(&ord[cell], kOrder[lab]);
        }
        __syncthreads();
        LoopFold& fo = fold[p];
        for (int k = threadIdx.x; k < kCells; k += 256) {
            if (rk[0][k]) atomicMax(&fo.reset[0][k], rk[0][k]);
            if (rk[1][k]) atomicMax(&fo.reset[1][k], rk[1][k]);
            if (ord[k]) atomicMax(&fo.order[k], ord[k]);
        }
    }
    int* out = hist + (size_t)p * kHist;
    for (int k = threadIdx.x; k < kHist; k += 256) {
        const int v = h[k];
        if (v) atomicAdd(&out[k], v);
    }
}

// SC / ISC after k_loop_bin<true>: per cell the largest in-range value (SC -128 .. 127, ISC 0 .. 255) of the points after the cell's
// last reset (every point when none).  Values below the range (v <= -129, v < 0, INT_MIN) never change a cell.
__global__ __launch_bounds__(256) void k_loop_fold(const LoopPair* __restrict__ pairs, const LoopFrame* __restrict__ frames,
                                                   const LoopPairOut* __restrict__ pout, LoopFold* __restrict__ fold, unsigned kinds)
{
    __shared__ int after[2][kCells], mx[2][kCells];
    __shared__ float sM[16];
    const int p = blockIdx.x;
    const LoopPair P = pairs[p];
    const LoopFrame& F = frames[P.frame];
    const int n = F.n[2];
    const int base = (int)blockIdx.y * kBinChunk;
    if (base >= n) return;
    const bool moved = P.kind == 1 || F.has_M;
    LoopFold& fo = fold[p];
    for (int k = threadIdx.x; k < kCells; k += 256) {
        after[0][k] = (int)(fo.reset[0][k] >> 8); after[1][k] = (int)(fo.reset[1][k] >> 8);     // index + 1 of the last reset, or 0
        mx[0][k] = 0; mx[1][k] = 0;
    }
    if (threadIdx.x < 16) sM[threadIdx.x] = P.kind == 1 ? pout[p].T[threadIdx.x] : F.M[threadIdx.x];
    __syncthreads();
    const bool want_sc = kinds & LISREG_LOOP_SC, want_isc = kinds & LISREG_LOOP_ISC;
    const int end = n - base < kBinChunk ? n - base : kBinChunk;
    for (int l = threadIdx.x; l < end; l += 256) {
        const int i = base + l;
        const float4 q = F.pts[2][i];
        float x = q.x, y = q.y, z = q.z;
        if (moved) apply_m(sM, q.x, q.y, q.z, x, y, z);
        const int cell = bin_of(x, y);
        if (cell < 0) continue;
        if (want_sc && i >= after[0][cell]) {
            const int v = sc_value(z);
            if (v >= -128 && v <= 127) atomicMax(&mx[0][cell], v + 129);
        }
        if (want_isc && i >= after[1][cell]) {
            const int v = isc_value(F.inten[i]);
            if (v >= 0 && v <= 255) atomicMax(&mx[1][cell], v + 1);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < kCells; k += 256) {
        if (mx[0][k]) atomicMax(&fo.maxv[0][k], mx[0][k]);
        if (mx[1][k]) atomicMax(&fo.maxv[1][k], mx[1][k]);
    }
}

// calculateEPSC / calculateSEPSC / calculateFEPSC from the counters, and with fold state calculateSC / calculateISC / calculateSSC:
// desc[p] = nd descriptor slots of 1600 bytes (FEPSC, EPSC, SEPSC [, SC, ISC, SSC])
__global__ __launch_bounds__(256) void k_loop_finish(const LoopPair* __restrict__ pairs, const LoopFrame* __restrict__ frames,
                                                     const int* __restrict__ hist, const LoopFold* __restrict__ fold, int nd,
                                                     uint8_t* __restrict__ desc)
{
    const int p = blockIdx.x;
    const LoopPair P = pairs[p];
    const LoopFrame& F = frames[P.frame];
    const bool own = P.kind == 0;
    const int* h = hist + (size_t)p * kHist;
    uint8_t* d = desc + (size_t)p * nd * kCells;
    for (int c = threadIdx.x; c < kCells; c += 256) {
        const int e1 = h[c] & 255, p1 = h[kCells + c] & 255, p2 = h[2 * kCells + c] & 255, e2 = h[3 * kCells + c] & 255;   // uchar ++
        const uint8_t epsc = (uint8_t)(100 * p1 / (1 + e1)), sepsc = (uint8_t)(100 * p2 / (1 + e2));
        const uint8_t fepsc = (uint8_t)(sepsc * 0.4 + epsc * 0.6);
        uint8_t v[kDescKinds] = { fepsc, epsc, sepsc, 0, 0, 0 };
        if (nd > 3) {
            const LoopFold& fo = fold[p];
            const unsigned r0 = fo.reset[0][c], r1 = fo.reset[1][c];
            int sc = r0 ? (int)(signed char)(uint8_t)(r0 & 255) : 0;          // the resetting point's byte, read as a signed char
            if (fo.maxv[0][c]) sc = max(sc, fo.maxv[0][c] - 129);
            int isc = r1 ? (int)(r1 & 255) : 0;
            if (fo.maxv[1][c]) isc = max(isc, fo.maxv[1][c] - 1);
            v[3] = (uint8_t)sc; v[4] = (uint8_t)isc; v[5] = (uint8_t)kLabelOfOrder[fo.order[c]];
        }
        for (int s = 0; s < nd; ++s) {
            d[s * kCells + c] = v[s];
            if (own && F.db[s]) F.db[s][c] = v[s];
        }
    }
}

// per (gated pair, enabled kind): calculateDistance(desc_db[hist], desc_cur) — shifts -10 .. 9 of the current descriptor's columns —
// or, for SSC, calculateLabelSim (no shift; 0 / 0 = NaN when both descriptors are empty)
__global__ __launch_bounds__(256) void k_loop_score(int cand0, const LoopPair* __restrict__ pairs, LoopScoreKinds ks, int nd,
                                                    const uint8_t* __restrict__ desc, LoopPairOut* __restrict__ pout)
{
    __shared__ uint8_t d1[kCells], d2[kCells];
    __shared__ int cnt[20];
    const int p = cand0 + (int)blockIdx.x;
    const int kind = ks.kind[blockIdx.y];
    const LoopPair P = pairs[p];
    const uint8_t* a = ks.db[kind] + (size_t)P.hist * kCells;
    const uint8_t* b = desc + ((size_t)p * nd + kSlotOf[kind]) * kCells;
    for (int c = threadIdx.x; c < kCells; c += 256) { d1[c] = a[c]; d2[c] = b[c]; }
    if (threadIdx.x < 20) cnt[threadIdx.x] = 0;
    __syncthreads();
    if (kind == kSsc) {
        int valid = 0, same = 0;
        for (int c = threadIdx.x; c < kCells; c += 256) {
            const int v1 = d1[c], v2 = d2[c];
            if (v1 == 0 && v2 == 0) continue;
            ++valid;
            same += v1 == v2;
        }
        for (int m = 32; m >= 1; m >>= 1) { valid += __shfl_xor(valid, m, 64); same += __shfl_xor(same, m, 64); }
        if ((threadIdx.x & 63) == 0) { atomicAdd(&cnt[0], valid); atomicAdd(&cnt[1], same); }
        __syncthreads();
        if (threadIdx.x == 0) {
            pout[p].kscore[kSsc] = (double)cnt[1] / (double)cnt[0];
            pout[p].kshift[kSsc] = 0;
        }
        return;
    }
    int part[20];
#pragma unroll
    for (int s = 0; s < 20; ++s) part[s] = 0;
    for (int c = threadIdx.x; c < kCells; c += 256) {
        const int q = c / kSectors, col = c - q * kSectors, v1 = d1[c];
#pragma unroll
        for (int s = 0; s < 20; ++s) {
            int nc = col + s - 10;
            if (nc >= kSectors) nc -= kSectors;
            if (nc < 0) nc += kSectors;
            part[s] += abs(v1 - (int)d2[q * kSectors + nc]);
        }
    }
#pragma unroll
    for (int s = 0; s < 20; ++s) {
        int v = part[s];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&cnt[s], v);          // integers: any order
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double difference = 1.0;
        int shift = 0;
        for (int s = 0; s < 20; ++s) {
            const double t = ((double)cnt[s]) / (kSectors * kRings * 255);
            if (t < difference) { difference = t; shift = s - 10; }
        }
        pout[p].kscore[kind] = 1 - difference;
        pout[p].kshift[kind] = shift;
        if (kind == kFepsc) {
            pout[p].score = 1 - difference;
            pout[p].score_shift = shift;
        }
    }
}

// Identity().translation() << x, y, 0; rotate(AngleAxisf(angle, UnitZ())): row-major 4 x 4
__device__ void planar_transform(float x, float y, float angle, float* M)
{
    const float c = cosf(angle), s = sinf(angle);
    for (int i = 0; i < 16; ++i) M[i] = (i % 5 == 0) ? 1.f : 0.f;
    M[0] = c; M[1] = -s; M[3] = x;
    M[4] = s; M[5] = c;  M[7] = y;
    M[10] = (1.f - c) + c;
}

// per frame: every enabled kind's first strict maximum above its threshold (Pose: the first strict minimum of the gate distance
// below 1000000), the transforms of :771-890, the matched list in push order (ISC, SC, EPSC, SEPSC, FEPSC, SSC, Pose) and the FEPSC
// result of lisreg_loopdet_detect (-1 / identity / 0 when FEPSC is not enabled)
__global__ __launch_bounds__(64) void k_loop_select(const LoopFrame* __restrict__ frames, int n_frames, const LoopPair* __restrict__ pairs,
                                                    const LoopPairOut* __restrict__ pout, unsigned kinds, double threshold, double label_threshold,
                                                    lisreg_loopdet_result* __restrict__ res, lisreg_loopdet_match* __restrict__ match,
                                                    int* __restrict__ n_match)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_frames) return;
    const LoopFrame& F = frames[k];
    lisreg_loopdet_result r;
    r.current_frame_id = F.frame_id; r.n_candidates = F.n_cand; r.matched_frame_id = -1; r.reserved = 0; r.score = 0.0;
    for (int i = 0; i < 16; ++i) r.matched_transform[i] = (i % 5 == 0) ? 1.f : 0.f;
    int nm = 0;
    for (int kind = 0; kind < kKinds; ++kind) {
        if (!((kinds >> kind) & 1u)) continue;
        double best = kind == kPose ? 1000000.0 : 0.0;
        int at = -1;
        for (int c = F.cand0; c < F.cand0 + F.n_cand; ++c) {
            if (kind == kPose) {
                const double s = pairs[c].pos_distance;
                if (s < best) { best = s; at = c; }
            } else {
                const double s = pout[c].kscore[kind];
                if (s > (kind == kSsc ? label_threshold : threshold) && s > best) { best = s; at = c; }
            }
        }
        if (at < 0) continue;
        lisreg_loopdet_match& m = match[(size_t)k * kKinds + nm++];
        m.kind = 1 << kind; m.history_id = pairs[at].hist; m.score = best;
        const float* T = pout[at].T;
        if (kind == kSsc || kind == kPose) {
            for (int i = 0; i < 16; ++i) m.transform[i] = T[i];
            continue;
        }
        // getTranslationAndEulerAngles(transform): x, y, angle = atan2(m10, m00).  ISC, SC, SEPSC: calculateDistance refines the
        // double angle by shift * sector_step (every selected score improved on 1.0); EPSC starts from the unwrapped yaw_diff
        // instead; FEPSC keeps the ICP's angle
        const float angle = atan2f(T[4], T[0]);
        float a = angle;
        if (kind == kEpsc) a = (float)((double)pairs[at].yaw_diff + pout[at].kshift[kind] * kSectorStep);
        else if (kind != kFepsc) a = (float)((double)angle + pout[at].kshift[kind] * kSectorStep);
        planar_transform(T[3], T[7], a, m.transform);
        if (kind == kFepsc) {
            r.matched_frame_id = m.history_id; r.score = best;
            for (int i = 0; i < 16; ++i) r.matched_transform[i] = m.transform[i];
        }
    }
    n_match[k] = nm;
    res[k] = r;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------


}  // namespace

struct LoopDb {
    std::vector<double> px, py, travel;       // posArr (x, y; z is 0), travelDistanceArr
    std::vector<float>  yaw;                  // yawArr
    DevBuf proj, desc[kDescKinds];            // ProjectArr (float4 [360] per frame); per descriptor slot of an enabled kind, its
                                              // *Arr (uchar [1600] per frame)
    int cap = 0;
    unsigned kinds = LISREG_LOOP_FEPSC;       // lisreg_loopdet_configure
    double label_threshold = LISREG_LOOP_LABEL_THRESHOLD;
    std::vector<std::vector<lisreg_loopdet_candidate>> last;       // candidates of every frame of the last detect call
    std::vector<std::vector<lisreg_loopdet_kind_scores>> last_scores;
    std::vector<std::vector<lisreg_loopdet_match>> last_match;     // matched lists of every frame of the last detect call
    int n() const { return (int)px.size(); }
    bool stores(int slot) const
    {
        for (int k = 0; k < kDescKinds; ++k) if (kSlotOf[k] == slot) return (kinds >> k) & 1u;
        return false;
    }
};

struct LoopDet {
    LoopDb db[LISREG_LOOPDET_MAX_DB];
    DevBuf in, hist, desc, out, proj_tmp, fold;   // the call's upload (tables + host clouds), counters, descriptors, results, fold state
    std::vector<unsigned char> h_in, h_out;
};

void LoopDetDelete::operator()(LoopDet* p) const { delete p; }

namespace {

LoopDet* loopdet_of(lisreg_ctx* c)
{
    if (!c->loopdet) c->loopdet.reset(new (std::nothrow) LoopDet());
    return c->loopdet.get();
}

// grow a database's device arrays to hold `need` frames, keeping the frames stored so far
int db_reserve(lisreg_ctx* c, LoopDb& d, int need)
{
    if (need <= d.cap) return LISREG_OK;
    const int cap = std::max(need, std::max(64, 2 * d.cap));
    DevBuf np, nd[kDescKinds];
    bool ok = np.ensure(sizeof(float4) * kProj * (size_t)cap) == hipSuccess;
    for (int s = 0; s < kDescKinds && ok; ++s)
        if (d.stores(s)) ok = nd[s].ensure((size_t)kCells * cap) == hipSuccess;
    if (!ok) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: device allocation failed");
    const int n = d.n();
    hipError_t e = hipSuccess;
    if (n > 0) {
        e = hipMemcpyAsync(np.p, d.proj.p, sizeof(float4) * kProj * (size_t)n, hipMemcpyDeviceToDevice, c->stream);
        for (int s = 0; s < kDescKinds && e == hipSuccess; ++s)
            if (d.stores(s)) e = hipMemcpyAsync(nd[s].p, d.desc[s].p, (size_t)kCells * n, hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return ctx_fail(c, LISREG_ERR_HIP, std::string("loopdet: ") + hipGetErrorString(e));
    d.proj = std::move(np);
    for (int s = 0; s < kDescKinds; ++s) d.desc[s] = std::move(nd[s]);
    d.cap = cap;
    return LISREG_OK;
}

int check_clouds(lisreg_ctx* c, const void* const* ptr, const int* n, int stride, int fmt, const char* who)
{
    for (int k = 0; k < 3; ++k)
        if (n[k] < 0 || (n[k] > 0 && !ptr[k])) return bad(c, (std::string(who) + ": NULL cloud with n > 0").c_str());
    if (fmt != LISREG_FMT_DEVICE && fmt != LISREG_FMT_XYZI && fmt != LISREG_FMT_XYZIL) return bad(c, (std::string(who) + ": fmt must be XYZI, XYZIL or DEVICE").c_str());
    if (fmt != LISREG_FMT_DEVICE && stride < 22) return bad(c, (std::string(who) + ": host structs need stride >= 22").c_str());
    return LISREG_OK;
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

struct FrameIn { const void* ptr[3]; int n[3]; };

// the launch sequence of one call: K frames (their own descriptors = pairs 0 .. K - 1), then the gated pairs.  frames / pairs are
// filled except for the cloud and output pointers, which are set here.  kinds: the enabled selectors (the descriptors computed and,
// with a database, stored and scored).  Results are read back into h_out: LoopPairOut [P], lisreg_loopdet_result [K],
// lisreg_loopdet_match [K][7], int [K] (detect) — the caller has synchronised when this returns OK.
int run_launch(lisreg_ctx* c, LoopDet* L, std::vector<LoopFrame>& frames, std::vector<LoopPair>& pairs, const std::vector<FrameIn>& fin,
               int stride, int fmt, LoopDb* db, unsigned kinds, double threshold, double label_threshold)
{
    const int K = (int)frames.size(), P = (int)pairs.size(), C = P - K;
    const bool fold = kinds & kFoldKinds, want_int = kinds & LISREG_LOOP_ISC;
    const int nd = fold ? kDescKinds : 3;
    hipStream_t st = c->stream;
    // one upload: frame table, pair table, host clouds packed as 16-B records (then, for ISC, the semantic intensities)
    size_t pts_total = 0, sem_total = 0;
    long long max_total = 0, max_sem = 0;
    for (int k = 0; k < K; ++k) {
        long long t = 0;
        for (int j = 0; j < 3; ++j) { t += fin[(size_t)k].n[j]; if (fmt != LISREG_FMT_DEVICE) pts_total += (size_t)fin[(size_t)k].n[j]; }
        max_total = std::max(max_total, t);
        max_sem = std::max<long long>(max_sem, fin[(size_t)k].n[2]);
        sem_total += (size_t)fin[(size_t)k].n[2];
    }
    const long long chunks = std::max<long long>(1, (max_total + kBinChunk - 1) / kBinChunk);
    const long long sem_chunks = std::max<long long>(1, (max_sem + kBinChunk - 1) / kBinChunk);
    if (chunks > 65535) return bad(c, "loopdet: a frame holds more than 268 M points");
    if (fold && max_sem >= (1 << 24) - 1) return bad(c, "loopdet: SC / ISC / SSC take semantic clouds below 16 M points");
    const size_t off_pairs = align16(sizeof(LoopFrame) * K), off_pts = off_pairs + align16(sizeof(LoopPair) * P);
    const size_t off_int = off_pts + sizeof(float4) * pts_total;
    const size_t in_bytes = off_int + (want_int ? sizeof(float) * sem_total : 0);
    const size_t off_res = align16(sizeof(LoopPairOut) * P), off_match = off_res + align16(sizeof(lisreg_loopdet_result) * K);
    const size_t off_nmatch = off_match + sizeof(lisreg_loopdet_match) * kKinds * K;
    const size_t out_bytes = off_nmatch + sizeof(int) * K;
    HIPCHK(c, L->in.ensure(in_bytes));
    HIPCHK(c, L->hist.ensure(sizeof(int) * kHist * (size_t)P));
    HIPCHK(c, L->desc.ensure((size_t)nd * kCells * P));
    HIPCHK(c, L->out.ensure(out_bytes));
    if (fold) HIPCHK(c, L->fold.ensure(sizeof(LoopFold) * (size_t)P));
    if (!db) HIPCHK(c, L->proj_tmp.ensure(sizeof(float4) * kProj * (size_t)K));
    L->h_in.resize(in_bytes);
    unsigned char* base = L->in.as<unsigned char>();
    size_t at = 0, at_int = 0;
    for (int k = 0; k < K; ++k) {
        LoopFrame& F = frames[(size_t)k];
        for (int j = 0; j < 3; ++j) {
            F.n[j] = fin[(size_t)k].n[j];
            if (fmt == LISREG_FMT_DEVICE) { F.pts[j] = static_cast<const float4*>(fin[(size_t)k].ptr[j]); continue; }
            pack_cloud(fin[(size_t)k].ptr[j], F.n[j], stride, j == 2 ? LISREG_FMT_XYZIL : LISREG_FMT_XYZI,
                       reinterpret_cast<lisreg_dpoint*>(L->h_in.data() + off_pts) + at);
            F.pts[j] = reinterpret_cast<const float4*>(base + off_pts) + at;
            at += (size_t)F.n[j];
        }
        if (want_int) {
            // the float intensity of PointXYZIL (byte 16)
            float* dst = reinterpret_cast<float*>(L->h_in.data() + off_int) + at_int;
            const unsigned char* src = static_cast<const unsigned char*>(fin[(size_t)k].ptr[2]);
            for (int i = 0; i < F.n[2]; ++i) memcpy(dst + i, src + (size_t)i * stride + 16, sizeof(float));
            F.inten = reinterpret_cast<const float*>(base + off_int) + at_int;
            at_int += (size_t)F.n[2];
        }
        for (int s = 0; s < kDescKinds; ++s) F.db[s] = nullptr;
        if (db) {
            F.proj = db->proj.as<float4>() + (size_t)F.frame_id * kProj;
            for (int s = 0; s < kDescKinds; ++s)
                if (db->stores(s)) F.db[s] = db->desc[s].as<uint8_t>() + (size_t)F.frame_id * kCells;
        } else {
            F.proj = L->proj_tmp.as<float4>() + (size_t)k * kProj;
        }
    }
    memcpy(L->h_in.data(), frames.data(), sizeof(LoopFrame) * K);
    if (P) memcpy(L->h_in.data() + off_pairs, pairs.data(), sizeof(LoopPair) * P);
    const LoopFrame* d_frames = reinterpret_cast<const LoopFrame*>(base);
    const LoopPair* d_pairs = reinterpret_cast<const LoopPair*>(base + off_pairs);
    unsigned char* d_out = L->out.as<unsigned char>();
    LoopPairOut* d_pout = reinterpret_cast<LoopPairOut*>(d_out);
    LoopFold* d_fold = fold ? L->fold.as<LoopFold>() : nullptr;
    HIPCHK(c, hipMemcpyAsync(base, L->h_in.data(), in_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(L->hist.p, 0, sizeof(int) * kHist * (size_t)P, st));
    if (fold) HIPCHK(c, hipMemsetAsync(L->fold.p, 0, sizeof(LoopFold) * (size_t)P, st));
    const float4* db_proj = db ? db->proj.as<float4>() : nullptr;
    // the kinds scored per gated pair (blockIdx.y of k_loop_score): the enabled descriptor kinds
    LoopScoreKinds sk;
    memset(&sk, 0, sizeof sk);
    int n_score = 0;
    for (int k = 0; k < kDescKinds && db; ++k)
        if ((kinds >> k) & 1u) { sk.db[k] = db->desc[kSlotOf[k]].as<uint8_t>(); sk.kind[n_score++] = k; }
    // without FEPSC nothing else writes a candidate's score / score_shift (lisreg_loopdet_candidate)
    if (C > 0 && !(kinds & LISREG_LOOP_FEPSC)) HIPCHK(c, hipMemsetAsync(d_pout, 0, sizeof(LoopPairOut) * (size_t)P, st));
    k_loop_project<<<K, 1024, 0, st>>>(d_frames);
    if (C > 0) k_loop_icp<<<C, 256, 0, st>>>(d_pairs, K, d_frames, db_proj, d_pout);
    if (fold) k_loop_bin<true><<<dim3((unsigned)P, (unsigned)chunks), 256, 0, st>>>(d_pairs, d_frames, d_pout, L->hist.as<int>(), d_fold, kinds);
    else k_loop_bin<false><<<dim3((unsigned)P, (unsigned)chunks), 256, 0, st>>>(d_pairs, d_frames, d_pout, L->hist.as<int>(), nullptr, kinds);
    if (kinds & (LISREG_LOOP_SC | LISREG_LOOP_ISC))
        k_loop_fold<<<dim3((unsigned)P, (unsigned)sem_chunks), 256, 0, st>>>(d_pairs, d_frames, d_pout, d_fold, kinds);
    k_loop_finish<<<P, 256, 0, st>>>(d_pairs, d_frames, L->hist.as<int>(), d_fold, nd, L->desc.as<uint8_t>());
    if (C > 0 && n_score > 0) k_loop_score<<<dim3((unsigned)C, (unsigned)n_score), 256, 0, st>>>(K, d_pairs, sk, nd, L->desc.as<uint8_t>(), d_pout);
    if (db)
        k_loop_select<<<(K + 63) / 64, 64, 0, st>>>(d_frames, K, d_pairs, d_pout, kinds, threshold, label_threshold,
                                                    reinterpret_cast<lisreg_loopdet_result*>(d_out + off_res),
                                                    reinterpret_cast<lisreg_loopdet_match*>(d_out + off_match), reinterpret_cast<int*>(d_out + off_nmatch));
    HIPCHK(c, hipGetLastError());
    L->h_out.resize(out_bytes);
    if (db) HIPCHK(c, hipMemcpyAsync(L->h_out.data(), L->out.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

// one LISREG_LOOP_* bit of a descriptor kind (ISC .. SSC) -> its kind index, or -1
int desc_kind_index(unsigned kind)
{
    for (int k = 0; k < kDescKinds; ++k) if (kind == (1u << k)) return k;
    return -1;
}

}  // namespace
}  // namespace lisreg

using namespace lisreg;

extern "C" {

int lisreg_loopdet_default_params(lisreg_loopdet_params* p)
{
    if (!p) return LISREG_ERR_ARG;
    p->skip_neighbour_distance = 20.0;      // SKIP_NEIBOUR_DISTANCE (epscGeneration.h:9)
    p->inflation_covariance = 0.01;         // INFLATION_COVARIANCE (:11)
    p->distance_threshold = 0.75;           // DISTANCE_THRESHOLD (:16)
    return LISREG_OK;
}

int lisreg_loopdet_reset(lisreg_ctx* c, int db_id)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_reset: bad db_id");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    LoopDb& d = L->db[db_id];
    d.px.clear(); d.py.clear(); d.travel.clear(); d.yaw.clear(); d.last.clear();     // device arrays and the kinds are kept
    d.last_scores.clear(); d.last_match.clear();
    return LISREG_OK;
}

int lisreg_loopdet_configure(lisreg_ctx* c, int db_id, unsigned kinds, double label_threshold)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_configure: bad db_id");
    if (kinds == 0 || kinds >= (1u << kKinds)) return bad(c, "loopdet_configure: kinds must be a nonzero mask of LISREG_LOOP_* bits");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    LoopDb& d = L->db[db_id];
    if (d.n() > 0) return bad(c, "loopdet_configure: the database holds frames (lisreg_loopdet_reset first)");
    if (kinds != d.kinds) {       // other descriptors: the arrays of the old ones go back now, the next add sizes new ones
        d.proj.release();
        for (auto& b : d.desc) b.release();
        d.cap = 0;
    }
    d.kinds = kinds;
    d.label_threshold = label_threshold;
    return LISREG_OK;
}

int lisreg_loopdet_detect(lisreg_ctx* c, int db_id, const lisreg_loopdet_frame* frames, int n_frames, int stride, int fmt,
                          const lisreg_loopdet_params* params, lisreg_loopdet_result* results)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_detect: bad db_id");
    if (n_frames < 0 || (n_frames > 0 && (!frames || !results))) return bad(c, "loopdet_detect: NULL frames / results");
    for (int k = 0; k < n_frames; ++k) {
        const void* ptr[3] = { frames[k].corner, frames[k].surf, frames[k].semantic };
        const int n[3] = { frames[k].n_corner, frames[k].n_surf, frames[k].n_semantic };
        const int rc = check_clouds(c, ptr, n, stride, fmt, "loopdet_detect");
        if (rc) return rc;
    }
    lisreg_loopdet_params prm;
    lisreg_loopdet_default_params(&prm);
    if (params) prm = *params;
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    LoopDb& d = L->db[db_id];
    if ((d.kinds & LISREG_LOOP_ISC) && fmt == LISREG_FMT_DEVICE)
        return bad(c, "loopdet_detect: ISC reads the intensity of host structs; device records carry only the label");
    if (n_frames == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const int n0 = d.n();
    int rc = db_reserve(c, d, n0 + n_frames);
    if (rc) return rc;
    // the gate, frame by frame, in double (:686-745); the current position is stored after the search (:900), so pos_distance is
    // measured against the PREVIOUS key frame
    std::vector<LoopFrame> lf((size_t)n_frames);
    std::vector<LoopPair> pairs((size_t)n_frames), cands;
    std::vector<FrameIn> fin((size_t)n_frames);
    for (int k = 0; k < n_frames; ++k) {
        const lisreg_loopdet_frame& f = frames[k];
        const float x_t = f.odom[3], y_t = f.odom[7], yaw_t = atan2f(f.odom[4], f.odom[0]);     // pcl::getTranslationAndEulerAngles
        if (d.travel.empty()) d.travel.push_back(0);
        else {
            const double dx = d.px.back() - (double)x_t, dy = d.py.back() - (double)y_t, dz = 0.0 - 0.0;
            d.travel.push_back(d.travel.back() + std::sqrt(dx * dx + dy * dy + dz * dz));
        }
        LoopFrame& F = lf[(size_t)k];
        memset(&F, 0, sizeof F);
        F.frame_id = d.n();
        F.cand0 = n_frames + (int)cands.size();
        const double cur_travel = d.travel.back();
        for (int i = 0; i < d.n(); ++i) {
            const double delta = cur_travel - d.travel[(size_t)i];
            const double ex = d.px[(size_t)i] - d.px.back(), ey = d.py[(size_t)i] - d.py.back(), ez = 0.0 - 0.0;
            const double pos_distance = std::sqrt(ex * ex + ey * ey + ez * ez);
            if (!(delta > prm.skip_neighbour_distance && pos_distance < delta * prm.inflation_covariance)) continue;
            LoopPair q;
            memset(&q, 0, sizeof q);
            q.frame = k; q.hist = i; q.kind = 1;
            float angle = yaw_t - d.yaw[(size_t)i];                   // globalICP's wrap (:262-265), float through double
            q.yaw_diff = angle;
            if (angle >= 2. * M_PI) angle = angle - 2. * M_PI;
            if (angle < 0) angle = angle + 2. * M_PI;
            q.yaw = angle;
            q.tmp_id = (int)std::floor(angle / kStep360);
            q.pos_distance = pos_distance;
            cands.push_back(q);
        }
        F.n_cand = (int)cands.size() - (F.cand0 - n_frames);
        d.px.push_back(x_t); d.py.push_back(y_t); d.yaw.push_back(yaw_t);
        LoopPair& own = pairs[(size_t)k];
        memset(&own, 0, sizeof own);
        own.frame = k; own.hist = F.frame_id; own.kind = 0;
        fin[(size_t)k] = FrameIn{ { f.corner, f.surf, f.semantic }, { f.n_corner, f.n_surf, f.n_semantic } };
    }
    pairs.insert(pairs.end(), cands.begin(), cands.end());
    rc = run_launch(c, L, lf, pairs, fin, stride, fmt, &d, d.kinds, prm.distance_threshold, d.label_threshold);
    if (rc) {
        // roll the database back to what it held before the call
        d.px.resize((size_t)n0); d.py.resize((size_t)n0); d.yaw.resize((size_t)n0); d.travel.resize((size_t)n0);
        return rc;
    }
    const unsigned char* ho = L->h_out.data();
    const LoopPairOut* po = reinterpret_cast<const LoopPairOut*>(ho);
    const size_t off_res = align16(sizeof(LoopPairOut) * pairs.size()), off_match = off_res + align16(sizeof(lisreg_loopdet_result) * n_frames);
    const lisreg_loopdet_result* res = reinterpret_cast<const lisreg_loopdet_result*>(ho + off_res);
    const lisreg_loopdet_match* mt = reinterpret_cast<const lisreg_loopdet_match*>(ho + off_match);
    const int* nm = reinterpret_cast<const int*>(ho + off_match + sizeof(lisreg_loopdet_match) * kKinds * n_frames);
    d.last.assign((size_t)n_frames, {});
    d.last_scores.assign((size_t)n_frames, {});
    d.last_match.assign((size_t)n_frames, {});
    for (int k = 0; k < n_frames; ++k) {
        results[k] = res[k];
        d.last_match[(size_t)k].assign(mt + (size_t)k * kKinds, mt + (size_t)k * kKinds + nm[k]);
        const LoopFrame& F = lf[(size_t)k];
        auto& v = d.last[(size_t)k];
        auto& vs = d.last_scores[(size_t)k];
        v.resize((size_t)F.n_cand);
        vs.resize((size_t)F.n_cand);
        for (int j = 0; j < F.n_cand; ++j) {
            const LoopPairOut& o = po[F.cand0 + j];
            const LoopPair& q = pairs[(size_t)(F.cand0 + j)];
            lisreg_loopdet_candidate& r = v[(size_t)j];
            memset(&r, 0, sizeof r);
            r.history_id = q.hist;
            r.yaw_shift = o.yaw_shift; r.yaw_angle = o.yaw_angle;
            r.icp_state = o.state; r.icp_iters = o.iters; r.icp_n_corr = o.n_corr;
            memcpy(r.transform, o.T, sizeof r.transform);
            r.score_shift = o.score_shift; r.score = o.score;
            lisreg_loopdet_kind_scores& s = vs[(size_t)j];
            memset(&s, 0, sizeof s);
            s.history_id = q.hist;
            for (int kk = 0; kk < kDescKinds; ++kk)
                if ((d.kinds >> kk) & 1u) { s.score[kk] = o.kscore[kk]; s.shift[kk] = o.kshift[kk]; }
            if (d.kinds & LISREG_LOOP_POSE) s.score[kPose] = q.pos_distance;
        }
    }
    return LISREG_OK;
}

int lisreg_loopdet_candidates(lisreg_ctx* c, int db_id, int k, lisreg_loopdet_candidate* out, int cap, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_candidates: bad db_id");
    if (!n_out || cap < 0 || (cap > 0 && !out)) return bad(c, "loopdet_candidates: NULL output");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    const LoopDb& d = L->db[db_id];
    if (k < 0 || k >= (int)d.last.size()) return bad(c, "loopdet_candidates: k is not a frame of the last detect call");
    const auto& v = d.last[(size_t)k];
    *n_out = (int)v.size();
    for (int j = 0; j < std::min(cap, (int)v.size()); ++j) out[j] = v[(size_t)j];
    return LISREG_OK;
}

int lisreg_loopdet_candidate_scores(lisreg_ctx* c, int db_id, int k, lisreg_loopdet_kind_scores* out, int cap, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_candidate_scores: bad db_id");
    if (!n_out || cap < 0 || (cap > 0 && !out)) return bad(c, "loopdet_candidate_scores: NULL output");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    const LoopDb& d = L->db[db_id];
    if (k < 0 || k >= (int)d.last_scores.size()) return bad(c, "loopdet_candidate_scores: k is not a frame of the last detect call");
    const auto& v = d.last_scores[(size_t)k];
    *n_out = (int)v.size();
    for (int j = 0; j < std::min(cap, (int)v.size()); ++j) out[j] = v[(size_t)j];
    return LISREG_OK;
}

int lisreg_loopdet_matches(lisreg_ctx* c, int db_id, int k, lisreg_loopdet_match* out, int cap, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_matches: bad db_id");
    if (!n_out || cap < 0 || (cap > 0 && !out)) return bad(c, "loopdet_matches: NULL output");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    const LoopDb& d = L->db[db_id];
    if (k < 0 || k >= (int)d.last_match.size()) return bad(c, "loopdet_matches: k is not a frame of the last detect call");
    const auto& v = d.last_match[(size_t)k];
    *n_out = (int)v.size();
    for (int j = 0; j < std::min(cap, (int)v.size()); ++j) out[j] = v[(size_t)j];
    return LISREG_OK;
}

int lisreg_loopdet_get(lisreg_ctx* c, int db_id, int frame_id, uint8_t* fepsc, float* projection)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_get: bad db_id");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    const LoopDb& d = L->db[db_id];
    if (frame_id < 0 || frame_id >= d.n()) return bad(c, "loopdet_get: frame_id out of range");
    if (fepsc && !(d.kinds & LISREG_LOOP_FEPSC)) return bad(c, "loopdet_get: FEPSC is not enabled on this database");
    HIPCHK(c, hipSetDevice(c->device));
    if (fepsc) HIPCHK(c, hipMemcpyAsync(fepsc, d.desc[0].as<uint8_t>() + (size_t)frame_id * kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    if (projection)
        HIPCHK(c, hipMemcpyAsync(projection, d.proj.as<float4>() + (size_t)frame_id * kProj, sizeof(float4) * kProj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

int lisreg_loopdet_get_descriptor(lisreg_ctx* c, int db_id, int frame_id, unsigned kind, uint8_t* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_get_descriptor: bad db_id");
    if (!out) return bad(c, "loopdet_get_descriptor: NULL output");
    const int ki = desc_kind_index(kind);
    if (ki < 0) return bad(c, "loopdet_get_descriptor: kind must be one of LISREG_LOOP_ISC .. LISREG_LOOP_SSC");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    const LoopDb& d = L->db[db_id];
    if (!(d.kinds & kind)) return bad(c, "loopdet_get_descriptor: the kind is not enabled on this database");
    if (frame_id < 0 || frame_id >= d.n()) return bad(c, "loopdet_get_descriptor: frame_id out of range");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, d.desc[kSlotOf[ki]].as<uint8_t>() + (size_t)frame_id * kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

namespace {

// one frame's descriptors under M (no database): pair 0 of a launch with the given kinds; on success L->desc holds nd slots
int descriptor_launch(lisreg_ctx* c, LoopDet* L, const void* const* ptr, const int* n, int stride, int fmt, const float* M, unsigned kinds)
{
    std::vector<LoopFrame> lf(1);
    memset(&lf[0], 0, sizeof lf[0]);
    if (M) { lf[0].has_M = 1; memcpy(lf[0].M, M, sizeof lf[0].M); }
    std::vector<LoopPair> pairs(1);
    memset(&pairs[0], 0, sizeof pairs[0]);
    std::vector<FrameIn> fin(1, FrameIn{ { ptr[0], ptr[1], ptr[2] }, { n[0], n[1], n[2] } });
    return run_launch(c, L, lf, pairs, fin, stride, fmt, nullptr, kinds, 0.0, 0.0);
}

}  // namespace

int lisreg_loop_descriptor(lisreg_ctx* c, const void* corner, int n_corner, const void* surf, int n_surf, const void* semantic,
                           int n_semantic, int stride, int fmt, const float* M, uint8_t* fepsc, uint8_t* epsc, uint8_t* sepsc,
                           float* projection)
{
    if (!c) return LISREG_ERR_ARG;
    const void* ptr[3] = { corner, surf, semantic };
    const int n[3] = { n_corner, n_surf, n_semantic };
    int rc = check_clouds(c, ptr, n, stride, fmt, "loop_descriptor");
    if (rc) return rc;
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    HIPCHK(c, hipSetDevice(c->device));
    rc = descriptor_launch(c, L, ptr, n, stride, fmt, M, LISREG_LOOP_FEPSC);
    if (rc) return rc;
    const uint8_t* dd = L->desc.as<uint8_t>();
    if (fepsc) HIPCHK(c, hipMemcpyAsync(fepsc, dd, kCells, hipMemcpyDeviceToHost, c->stream));
    if (epsc) HIPCHK(c, hipMemcpyAsync(epsc, dd + kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    if (sepsc) HIPCHK(c, hipMemcpyAsync(sepsc, dd + 2 * kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    if (projection) HIPCHK(c, hipMemcpyAsync(projection, L->proj_tmp.p, sizeof(float4) * kProj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

int lisreg_loop_descriptor_kind(lisreg_ctx* c, unsigned kind, const void* corner, int n_corner, const void* surf, int n_surf,
                                const void* semantic, int n_semantic, int stride, int fmt, const float* M, uint8_t* out)
{
    if (!c) return LISREG_ERR_ARG;
    const int ki = desc_kind_index(kind);
    if (ki < 0) return bad(c, "loop_descriptor_kind: kind must be one of LISREG_LOOP_ISC .. LISREG_LOOP_SSC");
    if (!out) return bad(c, "loop_descriptor_kind: NULL output");
    const void* ptr[3] = { corner, surf, semantic };
    const int n[3] = { n_corner, n_surf, n_semantic };
    int rc = check_clouds(c, ptr, n, stride, fmt, "loop_descriptor_kind");
    if (rc) return rc;
    if (kind == LISREG_LOOP_ISC && fmt == LISREG_FMT_DEVICE)
        return bad(c, "loop_descriptor_kind: ISC reads the intensity of host structs; device records carry only the label");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    HIPCHK(c, hipSetDevice(c->device));
    rc = descriptor_launch(c, L, ptr, n, stride, fmt, M, kind);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, L->desc.as<uint8_t>() + (size_t)kSlotOf[ki] * kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

}  // extern "C"
