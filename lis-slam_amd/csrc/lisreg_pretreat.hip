// lisreg_pretreat.hip — laser pretreatment: ring and per-point time from a raw sweep (x y z intensity).
//
// Replaces LaserPretreatment::Pretreatment (src/core/laserPretreatment.cpp:4-81, the same loop at :84-161 and twice inline in
// src/node/laserPretreatmentNode.cpp:60-219; removeClosedPointCloud, src/include/laserPretreatment.h:25-54).  Restated from knowledge of
// the C++ expressions, operation for operation; in input order:
//   1. removeNaNFromPointCloud: a point is dropped unless x, y and z are all finite.
//   2. removeClosedPointCloud: r2 = (x*x + y*y) + z*z in float, no contraction; dropped if r2 < min*min or r2 > max*max (float products).
//   3. startOri / endOri from the FIRST and LAST point that survived 1-2 (also when the ring table drops that point afterwards):
//      startOri = -atan2f(y0, x0); endOri = (float)(-atan2f(yl, xl) + 2 pi); then, with the difference a float subtraction compared
//      against a double and the update a double sum rounded to float: if (endOri - startOri > 3 pi) endOri -= 2 pi; else if
//      (endOri - startOri < pi) endOri += 2 pi.
//   4. angle = atanf(z / sqrtf(x*x + y*y)) * 180 / M_PI: `float * int` is a float product, the division by M_PI is a double one, the
//      result is stored in a float.  Ring by N_SCAN:
//        16: int((angle + 15) / 2 + 0.5) — float sum and quotient, + 0.5 in double; dropped if > 15 or < 0;
//        32: int((angle + 92.0 / 3.0) * 3.0 / 4.0) — double; dropped if > 31 or < 0;
//        64: angle >= -8.83 ? int((2 - angle) * 3.0 + 0.5) : 32 + int((-8.83 - angle) * 2.0 + 0.5) — `2 - angle` is a float difference,
//            the rest double; dropped if angle > 2 || angle < -24.33 || ring > 50 || ring < 0 (comparisons in double).
//      int() truncates toward zero (-0.25 -> ring 0, kept).  A NaN angle (x = y = z = 0 with min_range 0) is dropped EXPLICITLY: the x86
//      conversion yields INT_MIN there, which fails `ring < 0`; the GPU's conversion yields 0.
//   5. time of a kept point: ori = -atan2f(y, x); before halfPassed: if (ori < startOri - pi/2) ori += 2 pi; else if (ori > startOri +
//      3 pi/2) ori -= 2 pi; if (ori - startOri > pi) halfPassed = true; after it: ori += 2 pi; if (ori < endOri - 3 pi/2) ori += 2 pi;
//      else if (ori > endOri + pi/2) ori -= 2 pi; relTime = (ori - startOri) / (endOri - startOri) in float; time = (float)(scanPeriod *
//      relTime), a double product.  Points dropped in step 4 neither get a time nor move halfPassed.
//   6. kept points in input order; x, y, z and intensity copied bit for bit.
// A float libm function (atanf, atan2f) is DEFINED as the correctly rounded value — the double function rounded once to float — as in
// lisreg_features.hip; sqrtf and the float division are exact by IEEE.
//
// The parallel form.  The only loop-carried state, halfPassed, is monotone.  Let a_i be the before-halfPassed value of ori for kept point i
// (it depends on startOri only) and k = min { i kept : a_i - startOri > pi }.  Points i <= k take the first branch, points i > k the
// second (the point that flips the flag was itself computed by the first).  startOri / endOri are a min / max over the indices that
// pass steps 1-2.  So: two index reductions, a third for k, an order-preserving compaction, per-point arithmetic.
//
// gfx950 mapping: one thread per point, 16-byte reads, 256-thread workgroups; a sweep of 10^5 points is launch-latency-bound, so the
// launch sequence is short and the same for one sweep and for 256 (a workgroup finds its sweep in a table of first-workgroup numbers):
//   k_pt_classify   filters, ring, ori (atan2 once per point, kept in scratch); per workgroup: kept points, first / last index that
//                   passes steps 1-2
//   k_pt_flag       first / last of the sweep = min / max over its workgroups' entries; startOri / endOri; per workgroup: the first kept
//                   index that flips halfPassed
//   k_pt_write      kept points of the workgroups before this one and k, again over the sweep's entries (<= n / 256 reads), ballot +
//                   popcount inside the workgroup; time; records, times, intensities and the 16-byte result header by vector stores
// Per-workgroup partials, integer min / max only, no atomics and nothing to clear between calls; same bits on every run.
#include "lisreg_ctx.hpp"

#include <cstring>
#include <vector>

namespace lisreg {

namespace {

constexpr int kNone = 0x7f7f7f7f;                   // "no such index": larger than any point index
constexpr double kPi = 3.14159265358979323846;      // M_PI

struct PtSweep {                                    // one sweep of a call (48 bytes)
    const float4* in; float4* out; float* time; float* inten;
    int n, cap, blk0, pad;                          // blk0: the sweep's first workgroup
};
struct PtHeader { int n; float start_ori, end_ori; int half_index; };      // what crosses the link back

__device__ __forceinline__ const PtSweep& sweep_of(const PtSweep& one, const PtSweep* __restrict__ tab, int n_sweeps, int blk, int& s)
{
    if (!tab) { s = 0; return one; }
    int a = 0, b = n_sweeps - 1;                                       // last sweep whose first workgroup is <= blk
    while (a < b) { const int mid = (a + b + 1) >> 1; if (tab[mid].blk0 <= blk) a = mid; else b = mid - 1; }
    s = a;
    return tab[a];
}

__device__ __forceinline__ float neg_atan2f(float y, float x) { return -(float)atan2((double)y, (double)x); }

// step 4; -1: dropped
__device__ __forceinline__ int ring_of(float x, float y, float z, int n_scan)
{
    const float ratio = z / sqrtf(x * x + y * y);
    const float at = (float)atan((double)ratio);
    const float angle = (float)((double)(at * 180.0f) / kPi);
    if (angle != angle) return -1;
    int id;
    if (n_scan == 16) {
        id = (int)((double)((angle + 15.0f) / 2.0f) + 0.5);
        if (id > 15 || id < 0) return -1;
    } else if (n_scan == 32) {
        id = (int)(((double)angle + 92.0 / 3.0) * 3.0 / 4.0);
        if (id > 31 || id < 0) return -1;
    } else {
        const double a = (double)angle;
        if (a >= -8.83) id = (int)((double)(2.0f - angle) * 3.0 + 0.5);
        else id = 32 + (int)((-8.83 - a) * 2.0 + 0.5);
        if (a > 2.0 || a < -24.33 || id > 50 || id < 0) return -1;
    }
    return id;
}

// step 5, before halfPassed
__device__ __forceinline__ float ori_first_half(float ori, float startOri)
{
    if ((double)ori < (double)startOri - kPi / 2) ori = (float)((double)ori + 2 * kPi);
    else if ((double)ori > (double)startOri + kPi * 3 / 2) ori = (float)((double)ori - 2 * kPi);
    return ori;
}

// step 3
__device__ __forceinline__ void sweep_ends(const float4* __restrict__ in, int first, int last, float& startOri, float& endOri)
{
    startOri = 0.f; endOri = 0.f;
    if (first == kNone) return;
    const float4 p0 = in[first], pl = in[last];
    startOri = neg_atan2f(p0.y, p0.x);
    endOri = (float)((double)neg_atan2f(pl.y, pl.x) + 2 * kPi);
    if ((double)(endOri - startOri) > 3 * kPi) endOri = (float)((double)endOri - 2 * kPi);
    else if ((double)(endOri - startOri) < kPi) endOri = (float)((double)endOri + 2 * kPi);
}

__device__ __forceinline__ int wave_min(int v) { for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64)); return v; }

// what a workgroup found among its 256 points: kept points, first / last index that passes steps 1-2 (kNone / -1: none), and — from
// k_pt_flag — the first kept index that flips halfPassed (kNone: none).  The sweep's values are reductions over its workgroups' entries,
// made again by every workgroup that needs them (<= n / 256 entries): no atomics, nothing to clear between calls.
struct PtBlock { int count, first, last, k; };

__device__ __forceinline__ int wave_max(int v) { for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64)); return v; }

__global__ __launch_bounds__(256) void k_pt_classify(PtSweep one, const PtSweep* __restrict__ tab, int n_sweeps, int n_scan, float min2, float max2,
                                                     int* __restrict__ ring, float* __restrict__ ori, PtBlock* __restrict__ blk)
{
    __shared__ int s_cnt[4], s_first[4], s_last[4];
    int s;
    const PtSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x, s);
    const int i = (blockIdx.x - sw.blk0) * 256 + threadIdx.x;
    const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    int id = -1, mine = kNone, mine_last = -1;
    if (i < sw.n) {
        const float4 p = sw.in[i];
        const float r2 = (p.x * p.x + p.y * p.y) + p.z * p.z;
        // isfinite of all three; then the two range tests as the reference writes them (a NaN r2 cannot occur past the first test)
        const bool ok = (fabsf(p.x) <= 3.402823466e38f) && (fabsf(p.y) <= 3.402823466e38f) && (fabsf(p.z) <= 3.402823466e38f) &&
                        !(r2 < min2) && !(r2 > max2);
        if (ok) {
            mine = i; mine_last = i;
            id = ring_of(p.x, p.y, p.z, n_scan);
            if (id >= 0) ori[slot] = neg_atan2f(p.y, p.x);
        }
        ring[slot] = id;
    }
    const int wf = wave_min(mine), wl = wave_max(mine_last);
    const unsigned long long kept = __ballot(id >= 0);
    if ((threadIdx.x & 63) == 0) { s_cnt[threadIdx.x >> 6] = __popcll(kept); s_first[threadIdx.x >> 6] = wf; s_last[threadIdx.x >> 6] = wl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        PtBlock b;
        b.count = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        b.first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
        b.last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
        b.k = kNone;
        blk[blockIdx.x] = b;
    }
}

// ends[s] = { startOri, endOri } of every sweep, written by the sweep's first workgroup
__global__ __launch_bounds__(256) void k_pt_flag(PtSweep one, const PtSweep* __restrict__ tab, int n_sweeps, const int* __restrict__ ring,
                                                 const float* __restrict__ ori, PtBlock* __restrict__ blk, float2* __restrict__ ends)
{
    __shared__ int s_first[4], s_last[4], s_k[4];
    __shared__ float s_start;
    int s;
    const PtSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x, s);
    const int nb = max(1, (sw.n + 255) / 256), me = blockIdx.x - sw.blk0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int first = kNone, last = -1;
    for (int b = threadIdx.x; b < nb; b += 256) { const PtBlock e = blk[sw.blk0 + b]; first = min(first, e.first); last = max(last, e.last); }
    first = wave_min(first); last = wave_max(last);
    if (lane == 0) { s_first[wave] = first; s_last[wave] = last; }
    __syncthreads();
    if (threadIdx.x == 0) {
        first = min(min(s_first[0], s_first[1]), min(s_first[2], s_first[3]));
        last = max(max(s_last[0], s_last[1]), max(s_last[2], s_last[3]));
        float a, b;
        sweep_ends(sw.in, first, last, a, b);
        s_start = a;
        if (me == 0) ends[s] = make_float2(a, b);
    }
    __syncthreads();
    const int i = me * 256 + threadIdx.x;
    const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    int mine = kNone;
    if (i < sw.n && ring[slot] >= 0) {
        const float startOri = s_start;
        const float a = ori_first_half(ori[slot], startOri);
        if ((double)(a - startOri) > kPi) mine = i;
    }
    const int wk = wave_min(mine);
    if (lane == 0) s_k[wave] = wk;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x].k = min(min(s_k[0], s_k[1]), min(s_k[2], s_k[3]));
}

__global__ __launch_bounds__(256) void k_pt_write(PtSweep one, const PtSweep* __restrict__ tab, int n_sweeps, double scan_period,
                                                  const int* __restrict__ ring, const float* __restrict__ ori, const PtBlock* __restrict__ blk,
                                                  const float2* __restrict__ ends, PtHeader* __restrict__ hdr)
{
    __shared__ int s_before[4], s_total[4], s_k[4], s_wave[4];
    int s;
    const PtSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x, s);
    const int nb = max(1, (sw.n + 255) / 256), me = blockIdx.x - sw.blk0;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // kept points of the sweep's workgroups before this one and of all of them; the sweep's k
    int before = 0, total = 0, k = kNone;
    for (int b = threadIdx.x; b < nb; b += 256) { const PtBlock e = blk[sw.blk0 + b]; total += e.count; if (b < me) before += e.count; k = min(k, e.k); }
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o, 64); total += __shfl_xor(total, o, 64); }
    k = wave_min(k);
    const int i = me * 256 + threadIdx.x;
    const size_t slot = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int id = i < sw.n ? ring[slot] : -1;
    const unsigned long long kept = __ballot(id >= 0);
    if (lane == 0) { s_before[wave] = before; s_total[wave] = total; s_k[wave] = k; s_wave[wave] = __popcll(kept); }
    __syncthreads();
    before = (s_before[0] + s_before[1]) + (s_before[2] + s_before[3]);
    total = (s_total[0] + s_total[1]) + (s_total[2] + s_total[3]);
    k = min(min(s_k[0], s_k[1]), min(s_k[2], s_k[3]));
    const float2 e = ends[s];
    const float startOri = e.x, endOri = e.y;
    const bool fits = total <= sw.cap;                                  // too small: the count goes back, nothing is written
    if (me == 0 && threadIdx.x == 0) {
        PtHeader h;
        h.n = total; h.start_ori = startOri; h.end_ori = endOri; h.half_index = -1;
        if (k == kNone || !fits) hdr[s] = h;
        else { hdr[s].n = h.n; hdr[s].start_ori = h.start_ori; hdr[s].end_ori = h.end_ori; }     // half_index: the thread that owns point k
    }
    if (id < 0 || !fits) return;
    int pos = before + __popcll(kept & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) pos += s_wave[w];
    float o = ori[slot];
    if (i <= k) o = ori_first_half(o, startOri);
    else {
        o = (float)((double)o + 2 * kPi);
        if ((double)o < (double)endOri - kPi * 3 / 2) o = (float)((double)o + 2 * kPi);
        else if ((double)o > (double)endOri + kPi / 2) o = (float)((double)o - 2 * kPi);
    }
    const float relTime = (o - startOri) / (endOri - startOri);
    const float4 p = sw.in[i];
    sw.out[pos] = make_float4(p.x, p.y, p.z, __uint_as_float((uint32_t)id));
    sw.time[pos] = (float)(scan_period * (double)relTime);
    if (sw.inten) sw.inten[pos] = p.w;
    if (i == k) hdr[s].half_index = pos;
}

// the launch sequence over device sweeps; headers land in c->pt_hdr_host (pinned) when the call returns
int pretreat_device(lisreg_ctx* c, int n_sweeps, std::vector<PtSweep>& sw, const lisreg_pretreat_params& P)
{
    hipStream_t st = c->stream;
    int blocks = 0;
    for (auto& s : sw) { s.blk0 = blocks; s.pad = 0; blocks += std::max(1, (s.n + 255) / 256); }
    const size_t slots = (size_t)blocks * 256;
    HIPCHK(c, c->pt_ends.ensure(sizeof(float2) * (size_t)n_sweeps));
    HIPCHK(c, c->pt_ring.ensure(sizeof(int) * slots));
    HIPCHK(c, c->pt_ori.ensure(sizeof(float) * slots));
    HIPCHK(c, c->pt_blk.ensure(sizeof(PtBlock) * (size_t)blocks));
    HIPCHK(c, c->pt_hdr.ensure(sizeof(PtHeader) * (size_t)n_sweeps));
    if (sizeof(PtHeader) * (size_t)n_sweeps > c->pt_hdr_host.cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, c->pt_hdr_host.ensure(sizeof(PtHeader) * (size_t)n_sweeps, sizeof(PtHeader) * 256));
    }
    const PtSweep* tab = nullptr;
    if (n_sweeps > 1) {                                                 // one sweep travels as a kernel argument
        HIPCHK(c, c->pt_tab.ensure(sizeof(PtSweep) * (size_t)n_sweeps));
        HIPCHK(c, hipMemcpyAsync(c->pt_tab.p, sw.data(), sizeof(PtSweep) * (size_t)n_sweeps, hipMemcpyHostToDevice, st));
        tab = c->pt_tab.as<PtSweep>();
    }
    int* ring = c->pt_ring.as<int>();
    float* ori = c->pt_ori.as<float>();
    PtBlock* blk = c->pt_blk.as<PtBlock>();
    float2* ends = c->pt_ends.as<float2>();
    k_pt_classify<<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, P.n_scan, P.min_range * P.min_range, P.max_range * P.max_range, ring, ori, blk);
    k_pt_flag<<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, ring, ori, blk, ends);
    k_pt_write<<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, P.scan_period, ring, ori, blk, ends, c->pt_hdr.as<PtHeader>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->pt_hdr_host.p, c->pt_hdr.p, sizeof(PtHeader) * (size_t)n_sweeps, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));                               // `sw` is the caller's local
    return LISREG_OK;
}

int check_params(lisreg_ctx* c, const lisreg_pretreat_params* P, const char* who)
{
    if (!P) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": no parameters");
    if (P->n_scan != 16 && P->n_scan != 32 && P->n_scan != 64) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": n_scan must be 16, 32 or 64");
    return LISREG_OK;
}

void header_out(const PtHeader& h, lisreg_pretreat_out* o)
{
    o->n = h.n; o->start_ori = h.start_ori; o->end_ori = h.end_ori; o->half_index = h.half_index;
}

}  // namespace
}  // namespace lisreg

using namespace lisreg;

int lisreg_default_pretreat_params(lisreg_pretreat_params* p)
{
    if (!p) return LISREG_ERR_ARG;
    p->n_scan = 64; p->min_range = 0.0f; p->max_range = 70.0f;          // config/params.yaml:68, 73-74
    p->scan_period = 0.1;                                               // laserPretreatment.h:12
    return LISREG_OK;
}

int lisreg_pretreat(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, const lisreg_pretreat_params* P, lisreg_pretreat_out* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!out) return bad(c, "pretreat: bad arguments");
    if (const int rc = check_params(c, P, "pretreat")) return rc;
    const bool dev = fmt == LISREG_FMT_DEVICE_XYZI;
    if (const int rc = check_cloud(c, "pretreat", cloud, n, stride, fmt, kFmtSweep, true)) return rc;
    if (fmt == LISREG_FMT_XYZI && stride < 20) return bad(c, "pretreat: XYZI needs stride >= 20 (the intensity is read)");
    if (out->capacity < 0 || (out->capacity > 0 && (!out->cloud || (dev && !out->time_device))))
        return ctx_fail(c, LISREG_ERR_ARG, "pretreat: output buffers missing");
    const size_t in_bytes = (size_t)n * (dev ? sizeof(lisreg_dpoint) : (size_t)stride), cap = (size_t)out->capacity;
    if (spans_overlap(cloud, in_bytes, out->cloud, cap * (dev ? 16 : 32)) ||
        (dev && (spans_overlap(cloud, in_bytes, out->time_device, cap * 4) || spans_overlap(cloud, in_bytes, out->intensity_device, cap * 4))))
        return ctx_fail(c, LISREG_ERR_ARG, "pretreat: the output overlaps the input");
    out->n = 0; out->start_ori = out->end_ori = 0.f; out->half_index = -1;
    if (n == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<PtSweep> sw(1);
    if (dev) {
        sw[0] = PtSweep{ static_cast<const float4*>(cloud), static_cast<float4*>(out->cloud), out->time_device, out->intensity_device, n,
                         out->capacity, 0, 0 };
        if (const int rc = pretreat_device(c, 1, sw, *P)) return rc;
        const PtHeader h = c->pt_hdr_host.as<PtHeader>()[0];
        header_out(h, out);
        if (h.n > out->capacity) { out->half_index = -1; return ctx_fail(c, LISREG_ERR_ARG, "pretreat: the output buffer is too small (count written back)"); }
        return LISREG_OK;
    }
    // host structs: up as 16-byte records (intensity in the payload) through the pinned staging, results copied back
    HIPCHK(c, c->pt_in.ensure(sizeof(float4) * (size_t)n));
    HIPCHK(c, c->pt_out.ensure(sizeof(float4) * (size_t)n));
    HIPCHK(c, c->pt_time.ensure(sizeof(float) * 2 * (size_t)n));
    if (const int rc = upload_records(c, cloud, n, stride, fmt == LISREG_FMT_XYZI ? kPackIntensity : LISREG_FMT_XYZI_PACKED, c->pt_in.p)) return rc;
    sw[0] = PtSweep{ c->pt_in.as<float4>(), c->pt_out.as<float4>(), c->pt_time.as<float>(), c->pt_time.as<float>() + n, n, n, 0, 0 };
    if (const int rc = pretreat_device(c, 1, sw, *P)) return rc;
    const PtHeader h = c->pt_hdr_host.as<PtHeader>()[0];
    header_out(h, out);
    if (h.n > out->capacity) { out->half_index = -1; return ctx_fail(c, LISREG_ERR_ARG, "pretreat: the output buffer is too small (count written back)"); }
    if (h.n == 0) return LISREG_OK;
    std::vector<float4> rec((size_t)h.n);
    std::vector<float> ti(2 * (size_t)h.n);
    hipStream_t st = c->stream;
    HIPCHK(c, hipMemcpyAsync(rec.data(), c->pt_out.p, sizeof(float4) * (size_t)h.n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(ti.data(), c->pt_time.p, sizeof(float) * (size_t)h.n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipMemcpyAsync(ti.data() + h.n, c->pt_time.as<float>() + n, sizeof(float) * (size_t)h.n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    unsigned char* o = static_cast<unsigned char*>(out->cloud);
    for (int j = 0; j < h.n; ++j, o += 32) {                            // PointXYZIRT (common.h:12-23)
        memset(o, 0, 32);
        memcpy(o, &rec[(size_t)j], 12);
        memcpy(o + 16, &ti[(size_t)h.n + j], 4);
        uint32_t payload; memcpy(&payload, &rec[(size_t)j].w, 4);
        const uint16_t ring = (uint16_t)payload;
        memcpy(o + 20, &ring, 2);
        memcpy(o + 24, &ti[(size_t)j], 4);
    }
    return LISREG_OK;
}

int lisreg_pretreat_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const lisreg_pretreat_params* P,
                          lisreg_pretreat_out* outs)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_sweeps < 0 || n_sweeps > 256 || (n_sweeps > 0 && (!sweeps || !n || !outs))) return ctx_fail(c, LISREG_ERR_ARG, "pretreat_batch: bad arguments (at most 256 sweeps)");
    if (const int rc = check_params(c, P, "pretreat_batch")) return rc;
    if (n_sweeps == 0) return LISREG_OK;
    std::vector<PtSweep> sw((size_t)n_sweeps);
    long long total = 0;
    for (int s = 0; s < n_sweeps; ++s) {
        const lisreg_pretreat_out& o = outs[s];
        if (n[s] < 0 || (n[s] > 0 && !sweeps[s])) return ctx_fail(c, LISREG_ERR_ARG, "pretreat_batch: NULL sweep with n > 0");
        if (o.capacity < 0 || (o.capacity > 0 && (!o.cloud || !o.time_device))) return ctx_fail(c, LISREG_ERR_ARG, "pretreat_batch: output buffers missing");
        if ((total += n[s]) > 1000000000LL) return ctx_fail(c, LISREG_ERR_ARG, "pretreat_batch: too many points");
        sw[(size_t)s] = PtSweep{ static_cast<const float4*>(sweeps[s]), static_cast<float4*>(o.cloud), o.time_device, o.intensity_device, n[s],
                                 o.capacity, 0, 0 };
    }
    for (int s = 0; s < n_sweeps; ++s)                                  // no output of the call may lie over an input of the call
        for (int t = 0; t < n_sweeps; ++t) {
            const size_t in_bytes = (size_t)n[t] * 16, cap = (size_t)outs[s].capacity;
            if (spans_overlap(sweeps[t], in_bytes, outs[s].cloud, cap * 16) || spans_overlap(sweeps[t], in_bytes, outs[s].time_device, cap * 4) ||
                spans_overlap(sweeps[t], in_bytes, outs[s].intensity_device, cap * 4))
                return ctx_fail(c, LISREG_ERR_ARG, "pretreat_batch: an output overlaps an input");
        }
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = pretreat_device(c, n_sweeps, sw, *P)) return rc;
    const PtHeader* h = c->pt_hdr_host.as<PtHeader>();
    bool small = false;
    for (int s = 0; s < n_sweeps; ++s) {
        header_out(h[s], &outs[s]);
        if (h[s].n > outs[s].capacity) { outs[s].half_index = -1; small = true; }
    }
    if (small) return ctx_fail(c, LISREG_ERR_ARG, "pretreat_batch: an output buffer is too small (counts written back; that sweep was not written)");
    return LISREG_OK;
}
