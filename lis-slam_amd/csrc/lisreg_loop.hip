// lisreg_loop.hip — FEPSC loop-closure candidate detection: EPSCGeneration::loopDetection (src/core/epscGeneration.cpp:663-992)
// with UsingFEPSCFlag, the only descriptor config/params.yaml:22-28 enables.  The host applies the pose / travel gate (:686-745)
// in double; everything after it is one launch sequence over every (frame, candidate) pair of a call:
//   k_loop_project  one workgroup per frame: project() (:84-120), the 1 x 360 table of (count, x, y, label) of labels
//                   {13, 14, 16, 18, 19}; "the last point wins" is the largest point index per sector, gathered afterwards;
//   k_loop_icp      one workgroup per gated pair: globalICP (:258-401) — the 60-shift yaw search on the counts, the two sector
//                   clouds in LDS, pcl::IterativeClosestPoint with PCL's defaults (10 iterations, no distance cap, transformation
//                   epsilon 0, relative MSE -DBL_MAX) by brute-force k = 1 (FLANN L2_Simple order, ties to the smaller index) and
//                   the shared Umeyama step (lisreg_icp_step.hpp); result trans * trans1;
//   k_loop_bin      the hot path: the whole current frame (corner, surf, semantic) moved by the pair's matrix and binned into four
//                   20 x 80 integer histograms in LDS (EPSC corner / surf, SEPSC 40|50 / 81), merged with integer atomics;
//   k_loop_finish   the uchar counters (mod 256), 100 * psc / (1 + esc) in int (mod 256), FEPSC = (uchar)(0.4 s + 0.6 e) in double;
//   k_loop_score    calculateDistance (:633-660): shifts -10 .. 9, first strict minimum;
//   k_loop_select   per frame, the first strict maximum above the threshold, and the transform of :860-870.
// The frame's own (untransformed) descriptor is the identity pair of the same launch and goes straight into the database, so a
// batch of K frames can match frames earlier in the same batch.  Compiled -ffp-contract=off: every float / double operation rounds
// on its own like the reference's x86 build.
// Deviation from the reference: globalICP wraps j + i once (`if (new_col >= sectors) new_col -= sectors`), which for a
// wrapped yaw above 331 sectors (a slightly negative yaw difference) reads past the 360-entry row — undefined behaviour.  Here the
// column is wrapped modulo 360.
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

struct LoopFrame {
    const float4* pts[3];    // corner, surf, semantic (16-B records, label in the payload of the semantic ones)
    float4*       proj;      // where k_loop_project writes the frame's 360 sectors
    uint8_t*      fepsc;     // where the identity pair's FEPSC goes (the database), or null
    int           n[3];
    int           has_M;     // lisreg_loop_descriptor with a matrix: the identity pair moves the clouds by M
    int           frame_id, cand0, n_cand, pad_;
    float         M[16];
};
struct LoopPair {
    int   frame, hist, kind, tmp_id;                     // kind 0: the frame's own descriptor, 1: a gated candidate
    float yaw;                                           // yaw difference wrapped into [0, 2 pi) (float, as globalICP)
    int   pad_[3];
};
struct LoopPairOut {
    float  T[16];
    float  yaw_angle;
    int    yaw_shift, state, iters, n_corr, score_shift;
    double score;
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

// the three clouds of a pair's frame, moved by the pair's matrix, into 4 x 1600 integer counters (LDS, then global atomics)
__global__ __launch_bounds__(256) void k_loop_bin(const LoopPair* __restrict__ pairs, const LoopFrame* __restrict__ frames,
                                                  const LoopPairOut* __restrict__ pout, int* __restrict__ hist)
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
        const double d = (double)sqrtf(x * x + y * y);
        if (!(d == d) || d >= kMaxDis || d < kMinDis) continue;
        const int ring = (int)floor((d - kMinDis) / kRingStep);
        const double angle = M_PI + (double)atan2f(y, x);
        const int sector = (int)floor(angle / kSectorStep);
        if (ring >= kRings || ring < 0 || sector >= kSectors || sector < 0) continue;
        atomicAdd(&h[slot * kCells + ring * kSectors + sector], 1);
    }
    __syncthreads();
    int* out = hist + (size_t)p * kHist;
    for (int k = threadIdx.x; k < kHist; k += 256) {
        const int v = h[k];
        if (v) atomicAdd(&out[k], v);
    }
}

// calculateEPSC / calculateSEPSC / calculateFEPSC from the counters: desc[p] = FEPSC, EPSC, SEPSC (1600 bytes each)
__global__ __launch_bounds__(256) void k_loop_finish(const LoopPair* __restrict__ pairs, const LoopFrame* __restrict__ frames,
                                                     const int* __restrict__ hist, uint8_t* __restrict__ desc)
{
    const int p = blockIdx.x;
    const LoopPair P = pairs[p];
    uint8_t* fepsc_db = P.kind == 0 ? frames[P.frame].fepsc : nullptr;
    const int* h = hist + (size_t)p * kHist;
    uint8_t* d = desc + (size_t)p * 3 * kCells;
    for (int c = threadIdx.x; c < kCells; c += 256) {
        const int e1 = h[c] & 255, p1 = h[kCells + c] & 255, p2 = h[2 * kCells + c] & 255, e2 = h[3 * kCells + c] & 255;   // uchar ++
        const uint8_t epsc = (uint8_t)(100 * p1 / (1 + e1)), sepsc = (uint8_t)(100 * p2 / (1 + e2));
        const uint8_t fepsc = (uint8_t)(sepsc * 0.4 + epsc * 0.6);
        d[c] = fepsc; d[kCells + c] = epsc; d[2 * kCells + c] = sepsc;
        if (fepsc_db) fepsc_db[c] = fepsc;
    }
}

// calculateDistance(FEPSCArr[hist], FEPSC_cur): shifts -10 .. 9 of the current descriptor's columns
__global__ __launch_bounds__(256) void k_loop_score(int cand0, const LoopPair* __restrict__ pairs, const uint8_t* __restrict__ db_fepsc,
                                                    const uint8_t* __restrict__ desc, LoopPairOut* __restrict__ pout)
{
    __shared__ uint8_t d1[kCells], d2[kCells];
    __shared__ int cnt[20];
    const int p = cand0 + (int)blockIdx.x;
    const LoopPair P = pairs[p];
    const uint8_t* a = db_fepsc + (size_t)P.hist * kCells;
    const uint8_t* b = desc + (size_t)p * 3 * kCells;
    for (int c = threadIdx.x; c < kCells; c += 256) { d1[c] = a[c]; d2[c] = b[c]; }
    if (threadIdx.x < 20) cnt[threadIdx.x] = 0;
    __syncthreads();
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
        pout[p].score = 1 - difference;
        pout[p].score_shift = shift;
    }
}

// best FEPSC candidate per frame (score > threshold && score > best: the first strict maximum) and its transform (:860-870)
__global__ __launch_bounds__(64) void k_loop_select(const LoopFrame* __restrict__ frames, int n_frames, const LoopPair* __restrict__ pairs,
                                                    const LoopPairOut* __restrict__ pout, double threshold, lisreg_loopdet_result* __restrict__ res)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= n_frames) return;
    const LoopFrame& F = frames[k];
    double best = 0.0;
    int id = -1, at = -1;
    for (int c = F.cand0; c < F.cand0 + F.n_cand; ++c) {
        const double s = pout[c].score;
        if (s > threshold && s > best) { best = s; id = pairs[c].hist; at = c; }
    }
    lisreg_loopdet_result r;
    r.current_frame_id = F.frame_id; r.n_candidates = F.n_cand; r.matched_frame_id = id; r.reserved = 0; r.score = best;
    for (int i = 0; i < 16; ++i) r.matched_transform[i] = (i % 5 == 0) ? 1.f : 0.f;
    if (at >= 0) {
        // getTranslationAndEulerAngles(transform): x, y, yaw = atan2(m10, m00); Identity().translation() << x, y, 0; rotate(yaw about z)
        const float* T = pout[at].T;
        const float yaw = atan2f(T[4], T[0]), c = cosf(yaw), s = sinf(yaw);
        r.matched_transform[0] = c; r.matched_transform[1] = -s; r.matched_transform[3] = T[3];
        r.matched_transform[4] = s; r.matched_transform[5] = c;  r.matched_transform[7] = T[7];
        r.matched_transform[10] = (1.f - c) + c;
    }
    res[k] = r;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

int bad(lisreg_ctx* c, const char* msg) { return ctx_fail(c, LISREG_ERR_ARG, msg); }

}  // namespace

struct LoopDb {
    std::vector<double> px, py, travel;       // posArr (x, y; z is 0), travelDistanceArr
    std::vector<float>  yaw;                  // yawArr
    DevBuf proj, fepsc;                       // ProjectArr (float4 [360] per frame), FEPSCArr (uchar [1600] per frame)
    int cap = 0;
    std::vector<std::vector<lisreg_loopdet_candidate>> last;     // candidates of every frame of the last detect call
    int n() const { return (int)px.size(); }
};

struct LoopDet {
    LoopDb db[LISREG_LOOPDET_MAX_DB];
    DevBuf in, hist, desc, out, proj_tmp;     // the call's upload (tables + host clouds), counters, descriptors, results
    std::vector<unsigned char> h_in, h_out;
};

void loopdet_destroy(lisreg_ctx* c)
{
    if (!c->loopdet) return;
    for (auto& d : c->loopdet->db) { d.proj.release(); d.fepsc.release(); }
    c->loopdet->in.release(); c->loopdet->hist.release(); c->loopdet->desc.release(); c->loopdet->out.release(); c->loopdet->proj_tmp.release();
    delete c->loopdet;
    c->loopdet = nullptr;
}

namespace {

LoopDet* loopdet_of(lisreg_ctx* c)
{
    if (!c->loopdet) c->loopdet = new (std::nothrow) LoopDet();
    return c->loopdet;
}

// grow a database's device arrays to hold `need` frames, keeping the frames stored so far
int db_reserve(lisreg_ctx* c, LoopDb& d, int need)
{
    if (need <= d.cap) return LISREG_OK;
    const int cap = std::max(need, std::max(64, 2 * d.cap));
    DevBuf np, nf;
    if (np.ensure(sizeof(float4) * kProj * (size_t)cap) != hipSuccess || nf.ensure((size_t)kCells * cap) != hipSuccess) {
        np.release(); nf.release();
        return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: device allocation failed");
    }
    const int n = d.n();
    hipError_t e = hipSuccess;
    if (n > 0) {
        e = hipMemcpyAsync(np.p, d.proj.p, sizeof(float4) * kProj * (size_t)n, hipMemcpyDeviceToDevice, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(nf.p, d.fepsc.p, (size_t)kCells * n, hipMemcpyDeviceToDevice, c->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) { np.release(); nf.release(); return ctx_fail(c, LISREG_ERR_HIP, std::string("loopdet: ") + hipGetErrorString(e)); }
    d.proj.release(); d.fepsc.release();
    d.proj = np; d.fepsc = nf; d.cap = cap;
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
// filled except for the cloud and output pointers, which are set here.  Results are read back into h_out: LoopPairOut [P] then
// lisreg_loopdet_result [K] (detect) — the caller has synchronised when this returns OK.
int run_launch(lisreg_ctx* c, LoopDet* L, std::vector<LoopFrame>& frames, std::vector<LoopPair>& pairs, const std::vector<FrameIn>& fin,
               int stride, int fmt, LoopDb* db, double threshold)
{
    const int K = (int)frames.size(), P = (int)pairs.size(), C = P - K;
    hipStream_t st = c->stream;
    // one upload: frame table, pair table, host clouds packed as 16-B records
    size_t pts_total = 0;
    long long max_total = 0;
    for (int k = 0; k < K; ++k) {
        long long t = 0;
        for (int j = 0; j < 3; ++j) { t += fin[(size_t)k].n[j]; if (fmt != LISREG_FMT_DEVICE) pts_total += (size_t)fin[(size_t)k].n[j]; }
        max_total = std::max(max_total, t);
    }
    const long long chunks = std::max<long long>(1, (max_total + kBinChunk - 1) / kBinChunk);
    if (chunks > 65535) return bad(c, "loopdet: a frame holds more than 268 M points");
    const size_t off_pairs = align16(sizeof(LoopFrame) * K), off_pts = off_pairs + align16(sizeof(LoopPair) * P);
    const size_t in_bytes = off_pts + sizeof(float4) * pts_total;
    const size_t out_bytes = align16(sizeof(LoopPairOut) * P) + sizeof(lisreg_loopdet_result) * K;
    HIPCHK(c, L->in.ensure(in_bytes));
    HIPCHK(c, L->hist.ensure(sizeof(int) * kHist * (size_t)P));
    HIPCHK(c, L->desc.ensure((size_t)3 * kCells * P));
    HIPCHK(c, L->out.ensure(out_bytes));
    if (!db) HIPCHK(c, L->proj_tmp.ensure(sizeof(float4) * kProj * (size_t)K));
    L->h_in.resize(in_bytes);
    unsigned char* base = L->in.as<unsigned char>();
    size_t at = 0;
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
        if (db) {
            F.proj = db->proj.as<float4>() + (size_t)F.frame_id * kProj;
            F.fepsc = db->fepsc.as<uint8_t>() + (size_t)F.frame_id * kCells;
        } else {
            F.proj = L->proj_tmp.as<float4>() + (size_t)k * kProj;
            F.fepsc = nullptr;
        }
    }
    memcpy(L->h_in.data(), frames.data(), sizeof(LoopFrame) * K);
    if (P) memcpy(L->h_in.data() + off_pairs, pairs.data(), sizeof(LoopPair) * P);
    const LoopFrame* d_frames = reinterpret_cast<const LoopFrame*>(base);
    const LoopPair* d_pairs = reinterpret_cast<const LoopPair*>(base + off_pairs);
    LoopPairOut* d_pout = L->out.as<LoopPairOut>();
    lisreg_loopdet_result* d_res = reinterpret_cast<lisreg_loopdet_result*>(L->out.as<unsigned char>() + align16(sizeof(LoopPairOut) * P));
    HIPCHK(c, hipMemcpyAsync(base, L->h_in.data(), in_bytes, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemsetAsync(L->hist.p, 0, sizeof(int) * kHist * (size_t)P, st));
    const float4* db_proj = db ? db->proj.as<float4>() : nullptr;
    const uint8_t* db_fepsc = db ? db->fepsc.as<uint8_t>() : nullptr;
    k_loop_project<<<K, 1024, 0, st>>>(d_frames);
    if (C > 0) k_loop_icp<<<C, 256, 0, st>>>(d_pairs, K, d_frames, db_proj, d_pout);
    k_loop_bin<<<dim3((unsigned)P, (unsigned)chunks), 256, 0, st>>>(d_pairs, d_frames, d_pout, L->hist.as<int>());
    k_loop_finish<<<P, 256, 0, st>>>(d_pairs, d_frames, L->hist.as<int>(), L->desc.as<uint8_t>());
    if (C > 0) k_loop_score<<<C, 256, 0, st>>>(K, d_pairs, db_fepsc, L->desc.as<uint8_t>(), d_pout);
    if (db) k_loop_select<<<(K + 63) / 64, 64, 0, st>>>(d_frames, K, d_pairs, d_pout, threshold, d_res);
    HIPCHK(c, hipGetLastError());
    L->h_out.resize(out_bytes);
    if (db) HIPCHK(c, hipMemcpyAsync(L->h_out.data(), L->out.p, out_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
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
    d.px.clear(); d.py.clear(); d.travel.clear(); d.yaw.clear(); d.last.clear();     // device arrays are kept for reuse
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
    if (n_frames == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    LoopDb& d = L->db[db_id];
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
            if (angle >= 2. * M_PI) angle = angle - 2. * M_PI;
            if (angle < 0) angle = angle + 2. * M_PI;
            q.yaw = angle;
            q.tmp_id = (int)std::floor(angle / kStep360);
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
    rc = run_launch(c, L, lf, pairs, fin, stride, fmt, &d, prm.distance_threshold);
    if (rc) {
        // roll the database back to what it held before the call
        d.px.resize((size_t)n0); d.py.resize((size_t)n0); d.yaw.resize((size_t)n0); d.travel.resize((size_t)n0);
        return rc;
    }
    const LoopPairOut* po = reinterpret_cast<const LoopPairOut*>(L->h_out.data());
    const lisreg_loopdet_result* res = reinterpret_cast<const lisreg_loopdet_result*>(L->h_out.data() + align16(sizeof(LoopPairOut) * pairs.size()));
    d.last.assign((size_t)n_frames, {});
    for (int k = 0; k < n_frames; ++k) {
        results[k] = res[k];
        const LoopFrame& F = lf[(size_t)k];
        auto& v = d.last[(size_t)k];
        v.resize((size_t)F.n_cand);
        for (int j = 0; j < F.n_cand; ++j) {
            const LoopPairOut& o = po[F.cand0 + j];
            lisreg_loopdet_candidate& r = v[(size_t)j];
            memset(&r, 0, sizeof r);
            r.history_id = pairs[(size_t)(F.cand0 + j)].hist;
            r.yaw_shift = o.yaw_shift; r.yaw_angle = o.yaw_angle;
            r.icp_state = o.state; r.icp_iters = o.iters; r.icp_n_corr = o.n_corr;
            memcpy(r.transform, o.T, sizeof r.transform);
            r.score_shift = o.score_shift; r.score = o.score;
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

int lisreg_loopdet_get(lisreg_ctx* c, int db_id, int frame_id, uint8_t* fepsc, float* projection)
{
    if (!c) return LISREG_ERR_ARG;
    if (db_id < 0 || db_id >= LISREG_LOOPDET_MAX_DB) return bad(c, "loopdet_get: bad db_id");
    LoopDet* L = loopdet_of(c);
    if (!L) return ctx_fail(c, LISREG_ERR_NOMEM, "loopdet: out of host memory");
    const LoopDb& d = L->db[db_id];
    if (frame_id < 0 || frame_id >= d.n()) return bad(c, "loopdet_get: frame_id out of range");
    HIPCHK(c, hipSetDevice(c->device));
    if (fepsc) HIPCHK(c, hipMemcpyAsync(fepsc, d.fepsc.as<uint8_t>() + (size_t)frame_id * kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    if (projection)
        HIPCHK(c, hipMemcpyAsync(projection, d.proj.as<float4>() + (size_t)frame_id * kProj, sizeof(float4) * kProj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

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
    std::vector<LoopFrame> lf(1);
    memset(&lf[0], 0, sizeof lf[0]);
    if (M) { lf[0].has_M = 1; memcpy(lf[0].M, M, sizeof lf[0].M); }
    std::vector<LoopPair> pairs(1);
    memset(&pairs[0], 0, sizeof pairs[0]);
    std::vector<FrameIn> fin(1, FrameIn{ { corner, surf, semantic }, { n_corner, n_surf, n_semantic } });
    rc = run_launch(c, L, lf, pairs, fin, stride, fmt, nullptr, 0.0);
    if (rc) return rc;
    const uint8_t* dd = L->desc.as<uint8_t>();
    if (fepsc) HIPCHK(c, hipMemcpyAsync(fepsc, dd, kCells, hipMemcpyDeviceToHost, c->stream));
    if (epsc) HIPCHK(c, hipMemcpyAsync(epsc, dd + kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    if (sepsc) HIPCHK(c, hipMemcpyAsync(sepsc, dd + 2 * kCells, kCells, hipMemcpyDeviceToHost, c->stream));
    if (projection) HIPCHK(c, hipMemcpyAsync(projection, L->proj_tmp.p, sizeof(float4) * kProj, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

}  // extern "C"
