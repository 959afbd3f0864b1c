// lisreg_rangenet.hip — the host code the reference wraps around its RangeNet++ network: spherical range-image projection into the
// network's input tensor, and labelling of the points from the network's logits.  The network itself is the caller's.
//
// Replaces NetTensorRT::doProjection and the two host halves of NetTensorRT::infer (src/segnet/netTensorRT.cpp:143-300, :333-354,
// :403-428) and the argmax / PointXYZIL loop of RangenetAPI::infer (src/core/rangenetAPI.cpp:50-73, :103-110).  Restated from knowledge of
// the C++ expressions, operation for operation:
//   1. (:146-148) fov_up = (float)(_fov_up / 180.0 * M_PI), fov_down likewise: double quotient and product rounded to float;
//      fov = fabsf(fov_down) + fabsf(fov_up), a float sum.
//   2. (:167) range = sqrtf((x*x + y*y) + z*z) in float, no contraction.
//   3. (:177-178) yaw = -atan2f(y, x); pitch = asinf(z / range), the quotient a float one (0 / 0 = NaN for a point at the origin).
//   4. (:192-193) proj_x = (float)(0.5 * ((double)yaw / M_PI + 1.0)); proj_y = (float)(1.0 - (double)((pitch + fabsf(fov_down)) / fov)),
//      the inner sum and quotient float.
//   5. (:196-207) proj_x *= _img_w, proj_y *= _img_h: `float * int` is a float product; floorf; std::min(size - 1.0f, v) is
//      `v < size - 1 ? v : size - 1` and std::max(0.0f, v) is `0 < v ? v : 0`, so a NaN proj_y becomes row H - 1.
//   6. (:272-294) the points are assigned to pixel y * W + x in order of decreasing range, later assignments overwrite: a pixel keeps its
//      point of smallest range.  sort_indexes is an unstable std::sort, so the reference does not say which of several points of exactly
//      equal range in one pixel is kept; DEFINED here as the one of highest input index (a stable sort assigned in order).
//   7. (:341) a pixel is invalid when its five values (range, x, y, z, intensity) all convert to the int 0 — the lambda takes `int i` —
//      i.e. all are of magnitude below 1: every empty pixel, and a pixel whose winner has range < 1 and |intensity| < 1.  Invalid pixels
//      carry five zeros; the others (v - mean[c]) / std[c] in float; the tensor is channel-major, 5 x H x W (:348-352).
//   8. (:420-428) the logits of an invalid pixel are replaced by {1, 0, ..., 0}; a point takes the vector of its own pixel (also when
//      another point won that pixel).
//   9. (rangenetAPI.cpp:62-72) prob = 0, label = 0; for j in order: if (prob <= logit[j]) { label = j; prob = logit[j]; } — the last of
//      equal maxima wins, all-negative logits give 0, a NaN logit is never taken; an invalid pixel gives 0.
//  10. (:103-110) x, y, z copied bit for bit, the label next to them.
// A float libm function (atan2f, asinf) is DEFINED as the correctly rounded value — the double function rounded once to float — as in
// lisreg_features.hip and lisreg_pretreat.hip; sqrtf and the float division are exact by IEEE.
// Defined where the reference is undefined: a point with a non-finite x, y, z or intensity takes no part in the projection (pixel
// index -1, label 0); H * W <= 2^24 (the reference forms the pixel index in float); n_classes <= 32.
//
// The parallel form.  "Sort by decreasing range, assign in order" leaves in each pixel the point that is smallest in (range, then
// -index): a per-pixel minimum over the 64-bit key (range bits << 32 | ~index).  Ranges are non-negative floats (or +inf), whose bit
// patterns order like their values; no key equals the empty mark ~0 (its high word would be a NaN).
//
// gfx950 mapping (a sweep of 10^5 points and an image of 10^5 pixels are launch-latency-bound, so the sequences are short and the same
// for one sweep and for 256):
//   k_rn_project   one thread per point, 16-byte reads: steps 2-5, the per-point pixel index, one 64-bit atomicMin on the pixel's key —
//                  the addresses spread over the whole image, unlike the same-address atomics DESIGN.md §7g-3 measured and removed
//   k_rn_pixel     one thread per pixel: the winner's record, step 7, five coalesced plane writes, the mask byte, the key put back to
//                  empty (so nothing is cleared between calls and there is no memset launch), valid pixels counted per workgroup
//   k_rn_count     one workgroup per sweep: the sum of its workgroups' counts (no atomics, nothing to clear)
//   k_rn_argmax    one thread per pixel: step 8-9 over coalesced plane reads, one label byte
//   k_rn_gather    one thread per point: one byte gathered through the pixel index, one 16-byte record written
// The kNN label clean-up of RangeNet++ (lisreg_rangenet_label_knn: k_rn_argmax_range, k_rn_range_min, k_rn_knn) is defined and mapped
// in its own section below.
// Plain C++ and vector stores only.
#include "lisreg_ctx.hpp"

#include <cmath>
#include <cstring>
#include <vector>

namespace lisreg {

namespace {

constexpr double kPi = 3.14159265358979323846;      // M_PI
constexpr unsigned long long kEmpty = ~0ull;
constexpr float kFltMax = 3.402823466e38f;

struct RnSweep {                                    // one sweep of a projection call (48 bytes)
    const float4* in; float* tensor; unsigned char* mask; int* pix;
    int n, blk0, pad0, pad1;                        // blk0: the sweep's first workgroup in k_rn_project
};
struct RnLabelSweep {                               // one sweep of a labelling call (64 bytes)
    const float4* in; const int* pix; const unsigned char* mask; const float* logits;
    float4* out; unsigned char* image;              // image: the caller's, or the context's scratch
    int n, blk0, pad0, pad1;
};
struct RnGeom { int h, w; float fov_down_abs, fov; float mean[5], std[5]; };

template <class S>
__device__ __forceinline__ const S& sweep_of(const S& one, const S* __restrict__ tab, int n_sweeps, int blk)
{
    if (!tab) return one;
    int a = 0, b = n_sweeps - 1;                                       // last sweep whose first workgroup is <= blk
    while (a < b) { const int mid = (a + b + 1) >> 1; if (tab[mid].blk0 <= blk) a = mid; else b = mid - 1; }
    return tab[a];
}

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= kFltMax; }
// (int)v == 0 for the values that have an int at all; NaN / inf (undefined in the reference) count as non-zero
__device__ __forceinline__ bool int_zero(float v) { return fabsf(v) < 1.0f; }

// steps 2-5: range and the pixel y * W + x of a finite point
__device__ __forceinline__ int pixel_of(float x, float y, float z, const RnGeom& g, float& range)
{
    range = sqrtf((x * x + y * y) + z * z);
    const float yaw = -(float)atan2((double)y, (double)x);
    const float pitch = (float)asin((double)(z / range));
    float px = (float)(0.5 * ((double)yaw / kPi + 1.0));
    float py = (float)(1.0 - (double)((pitch + g.fov_down_abs) / g.fov));
    px = px * (float)g.w;
    py = py * (float)g.h;
    const float wm1 = (float)g.w - 1.0f, hm1 = (float)g.h - 1.0f;
    px = floorf(px); px = (px < wm1) ? px : wm1; px = (0.0f < px) ? px : 0.0f;
    py = floorf(py); py = (py < hm1) ? py : hm1; py = (0.0f < py) ? py : 0.0f;
    return (int)py * g.w + (int)px;
}

__global__ __launch_bounds__(256) void k_rn_project(RnSweep one, const RnSweep* __restrict__ tab, int n_sweeps, RnGeom g,
                                                    unsigned long long* __restrict__ keys)
{
    const RnSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x);
    const int s = tab ? (int)(&sw - tab) : 0;
    const int i = (blockIdx.x - sw.blk0) * 256 + threadIdx.x;
    if (i >= sw.n) return;
    const float4 p = sw.in[i];
    int pix = -1;
    if (finite_f(p.x) && finite_f(p.y) && finite_f(p.z) && finite_f(p.w)) {
        float range;
        pix = pixel_of(p.x, p.y, p.z, g, range);
        const unsigned long long key = ((unsigned long long)__float_as_uint(range) << 32) | (unsigned long long)(~(unsigned)i);
        atomicMin(&keys[(size_t)s * (size_t)(g.h * g.w) + (size_t)pix], key);
    }
    sw.pix[i] = pix;
}

// grid: n_sweeps x bpi workgroups, bpi = ceil(H * W / 256)
__global__ __launch_bounds__(256) void k_rn_pixel(RnSweep one, const RnSweep* __restrict__ tab, int bpi, RnGeom g,
                                                  unsigned long long* __restrict__ keys, int* __restrict__ blk_valid)
{
    __shared__ int s_cnt[4];
    const int s = blockIdx.x / bpi, hw = g.h * g.w;
    const RnSweep& sw = tab ? tab[s] : one;
    const int pix = (blockIdx.x - s * bpi) * 256 + threadIdx.x;
    bool valid = false;
    if (pix < hw) {
        unsigned long long* kp = &keys[(size_t)s * (size_t)hw + (size_t)pix];
        const unsigned long long key = *kp;
        float v[5] = { 0.f, 0.f, 0.f, 0.f, 0.f };
        if (key != kEmpty) {
            *kp = kEmpty;
            const unsigned i = ~(unsigned)(key & 0xffffffffull);
            const float4 p = sw.in[i];
            const float range = __uint_as_float((unsigned)(key >> 32));
            valid = !(int_zero(range) && int_zero(p.x) && int_zero(p.y) && int_zero(p.z) && int_zero(p.w));
            if (valid) {
                v[0] = (range - g.mean[0]) / g.std[0];
                v[1] = (p.x - g.mean[1]) / g.std[1];
                v[2] = (p.y - g.mean[2]) / g.std[2];
                v[3] = (p.z - g.mean[3]) / g.std[3];
                v[4] = (p.w - g.mean[4]) / g.std[4];
            }
        }
#pragma unroll
        for (int c = 0; c < 5; ++c) sw.tensor[(size_t)c * (size_t)hw + (size_t)pix] = v[c];
        sw.mask[pix] = valid ? 0 : 1;
    }
    const unsigned long long b = __ballot(valid);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blk_valid[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

__global__ __launch_bounds__(256) void k_rn_count(int bpi, const int* __restrict__ blk_valid, int* __restrict__ n_valid)
{
    __shared__ int s_cnt[4];
    int v = 0;
    for (int b = threadIdx.x; b < bpi; b += 256) v += blk_valid[blockIdx.x * bpi + b];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) n_valid[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// grid: n_sweeps x bpi workgroups
__global__ __launch_bounds__(256) void k_rn_argmax(RnLabelSweep one, const RnLabelSweep* __restrict__ tab, int bpi, int hw, int n_classes)
{
    const int s = blockIdx.x / bpi;
    const RnLabelSweep& sw = tab ? tab[s] : one;
    const int pix = (blockIdx.x - s * bpi) * 256 + threadIdx.x;
    if (pix >= hw) return;
    int label = 0;
    if (!sw.mask[pix]) {                                                // an invalid pixel: {1, 0, ..., 0} gives 0
        float prob = 0.f;
        for (int j = 0; j < n_classes; ++j) {
            const float v = sw.logits[(size_t)j * (size_t)hw + (size_t)pix];
            if (prob <= v) { label = j; prob = v; }
        }
    }
    sw.image[pix] = (unsigned char)label;
}

__global__ __launch_bounds__(256) void k_rn_gather(RnLabelSweep one, const RnLabelSweep* __restrict__ tab, int n_sweeps, int hw)
{
    const RnLabelSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x);
    const int i = (blockIdx.x - sw.blk0) * 256 + threadIdx.x;
    if (i >= sw.n) return;
    const float4 p = sw.in[i];
    const int pix = sw.pix[i];
    const unsigned label = ((unsigned)pix < (unsigned)hw) ? (unsigned)sw.image[pix] : 0u;     // -1 (or anything outside the image): 0
    sw.out[i] = make_float4(p.x, p.y, p.z, __uint_as_float(label));
}

// ---- the kNN label clean-up (lisreg_rangenet_label_knn) ------------------------------------------------------------------------
// The post-processing step of RangeNet++ (the "++"): a k-nearest-neighbour vote in range over a small window of the range image, per
// point, after the network.  The reference tree has no text for it (its vendored wrapper never reads the `post: KNN: params:` block of
// the model's arch_cfg.yaml), so it is DEFINED here, after the authors' published post-processing, restated from knowledge.  With
// S = search, C = n_classes, window cell j = 0 .. S*S - 1 at row offset j / S - (S - 1) / 2 and column offset j % S - (S - 1) / 2:
//   1. Label image: steps 8-9 above (k_rn_argmax); invalid pixels are 0.
//   2. Range image: per pixel the smallest range = sqrtf((x*x + y*y) + z*z) (the float expression of step 2, no contraction: the
//      projection winner's range bit for bit) over the points with that pixel_index; points with pixel_index -1 take no part; a pixel no
//      point fell into has range +inf.  The invalid mask plays no part in the range image.
//   3. Weights: g_j = exp(-(dx*dx + dy*dy) / (2 sigma^2)) in double through the C library's exp, summed in the order of j;
//      w_j = (float)(1.0 - g_j / sum g), rounded once.  Computed on the host (lisreg_rangenet_knn_weights), handed to the kernel.
//   4. Per point with pixel_index >= 0 and a finite own range r: every window cell takes range and label of its pixel; a cell outside
//      the image takes range 0 and label 0 (the authors' zero padding, rows and columns, no wrap at the azimuth seam); the centre cell's
//      range is replaced by r, its label stays the pixel's.  d_j = fabsf(range_j - r) * w_j in float: +inf for an empty pixel, never NaN.
//   5. Selection: the knn cells smallest in (d_j, then j) — a tie in d goes to the lower window position.
//   6. Vote: a selected cell with cutoff > 0 && d_j > cutoff votes for nobody; every other selected cell votes for its label.
//   7. Result: the class in 1 .. C - 1 with the most votes, lowest class id on a tie; class 0 never wins; a point with no vote for any
//      class 1 .. C - 1 gets no_vote_label (1: the authors' argmax + 1 of all-zero counts; 0, the default: the outlier class).
//   8. A point with pixel_index -1 gets 0; a point whose own range is not finite keeps its pixel's label of step 1.
//   9. x, y, z bit for bit, the label in the payload.
// Limits: search in {1, 3, 5, 7}; 1 <= knn <= min(search^2, 16); sigma finite and > 0; 0 <= no_vote_label < C; C >= 2.
//
// gfx950 mapping (the same sequence for one sweep and for 256):
//   k_rn_argmax_range  one thread per pixel: k_rn_argmax, and the pixel's range set to +inf (nothing is cleared by a memset launch)
//   k_rn_range_min     one thread per point: step 2 as a 32-bit atomicMin on the range bits (non-negative floats order like their bits)
//   k_rn_knn<S>        one thread per point: the S*S distances in registers (every index a compile-time constant after unrolling), knn
//                      rounds of "smallest (d, j) above the last one taken" over them, the selected labels packed a byte each into two
//                      64-bit words, the vote as knn^2 byte compares — no per-thread array is indexed at run time, no LDS, no scratch
struct RnKnnSweep {                                 // one sweep of a kNN labelling call (64 bytes)
    const float4* in; const int* pix; const unsigned char* mask; const float* logits;
    float4* out; unsigned char* image; unsigned* range;   // image: the caller's, or the context's scratch; range: the context's scratch
    int n, blk0;
};
struct RnKnn { int h, w, knn, no_vote; float cutoff; float wgt[49]; };
constexpr unsigned kInfBits = 0x7f800000u;

// grid: n_sweeps x bpi workgroups
__global__ __launch_bounds__(256) void k_rn_argmax_range(RnKnnSweep one, const RnKnnSweep* __restrict__ tab, int bpi, int hw, int n_classes)
{
    const int s = blockIdx.x / bpi;
    const RnKnnSweep& sw = tab ? tab[s] : one;
    const int pix = (blockIdx.x - s * bpi) * 256 + threadIdx.x;
    if (pix >= hw) return;
    int label = 0;
    if (!sw.mask[pix]) {
        float prob = 0.f;
        for (int j = 0; j < n_classes; ++j) {
            const float v = sw.logits[(size_t)j * (size_t)hw + (size_t)pix];
            if (prob <= v) { label = j; prob = v; }
        }
    }
    sw.image[pix] = (unsigned char)label;
    sw.range[pix] = kInfBits;
}

__global__ __launch_bounds__(256) void k_rn_range_min(RnKnnSweep one, const RnKnnSweep* __restrict__ tab, int n_sweeps, int hw)
{
    const RnKnnSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x);
    const int i = (blockIdx.x - sw.blk0) * 256 + threadIdx.x;
    if (i >= sw.n) return;
    const int pix = sw.pix[i];
    if ((unsigned)pix >= (unsigned)hw) return;                          // -1 (or anything outside the image)
    const float4 p = sw.in[i];
    const float range = sqrtf((p.x * p.x + p.y * p.y) + p.z * p.z);     // >= 0 or +inf for the finite coordinates of such a point
    atomicMin(&sw.range[pix], __float_as_uint(range));
}

template <int S>
__global__ __launch_bounds__(256) void k_rn_knn(RnKnnSweep one, const RnKnnSweep* __restrict__ tab, int n_sweeps, RnKnn K)
{
    const RnKnnSweep& sw = sweep_of(one, tab, n_sweeps, blockIdx.x);
    const int i = (blockIdx.x - sw.blk0) * 256 + threadIdx.x;
    if (i >= sw.n) return;
    const float4 p = sw.in[i];
    const int pix = sw.pix[i];
    unsigned label = 0;
    if ((unsigned)pix < (unsigned)(K.h * K.w)) {
        label = sw.image[pix];
        const float r = sqrtf((p.x * p.x + p.y * p.y) + p.z * p.z);
        if (finite_f(r)) {
            const int row = pix / K.w, y0 = row - (S - 1) / 2, x0 = pix - row * K.w - (S - 1) / 2;
            float d[S * S];
#pragma unroll
            for (int j = 0; j < S * S; ++j) {
                const int y = y0 + j / S, x = x0 + j % S;
                float rj = 0.f;                                         // outside the image: zero padding
                if ((unsigned)y < (unsigned)K.h && (unsigned)x < (unsigned)K.w) rj = __uint_as_float(sw.range[y * K.w + x]);
                if (j == (S * S) / 2) rj = r;
                d[j] = fabsf(rj - r) * K.wgt[j];
            }
            // d >= 0 and never NaN: (bits of d, j + 1) orders like (d, j), and 0 is below every key
            unsigned long long last = 0, lo = 0, hi = 0;
            for (int a = 0; a < K.knn; ++a) {
                unsigned long long best = ~0ull;
#pragma unroll
                for (int j = 0; j < S * S; ++j) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(d[j]) << 32) | (unsigned long long)(j + 1);
                    if (key > last && key < best) best = key;
                }
                last = best;
                const int j = (int)(best & 0xffull) - 1;
                const float dj = __uint_as_float((unsigned)(best >> 32));
                const int y = y0 + j / S, x = x0 + j % S;
                unsigned long long vote = 0;                            // 0: nobody (class 0 never wins, so its votes need no count)
                if (!(K.cutoff > 0.f && dj > K.cutoff) && (unsigned)y < (unsigned)K.h && (unsigned)x < (unsigned)K.w)
                    vote = sw.image[y * K.w + x];
                if (a < 8) lo |= vote << (8 * a); else hi |= vote << (8 * (a - 8));
            }
            int best_n = 0;
            label = (unsigned)K.no_vote;
            for (int a = 0; a < K.knn; ++a) {
                const unsigned la = (unsigned)(((a < 8 ? lo : hi) >> (8 * (a & 7))) & 0xffull);
                if (la == 0) continue;
                int cnt = 0;
                for (int b = 0; b < K.knn; ++b) cnt += (unsigned)(((b < 8 ? lo : hi) >> (8 * (b & 7))) & 0xffull) == la;
                if (cnt > best_n || (cnt == best_n && la < label)) { best_n = cnt; label = la; }
            }
        }
    }
    sw.out[i] = make_float4(p.x, p.y, p.z, __uint_as_float(label));
}

struct Span { const void* p; size_t bytes; };
// no output may lie over an input or over another output
bool any_overlap(const std::vector<Span>& in, const std::vector<Span>& out)
{
    for (size_t a = 0; a < out.size(); ++a) {
        for (const Span& i : in) if (spans_overlap(out[a].p, out[a].bytes, i.p, i.bytes)) return true;
        for (size_t b = a + 1; b < out.size(); ++b) if (spans_overlap(out[a].p, out[a].bytes, out[b].p, out[b].bytes)) return true;
    }
    return false;
}

int check_params(lisreg_ctx* c, const lisreg_rangenet_params* P, const char* who)
{
    if (!P) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": no parameters");
    if (P->img_h < 1 || P->img_w < 1 || (long long)P->img_h * (long long)P->img_w > (1LL << 24))
        return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": img_h and img_w must be >= 1 and img_h * img_w <= 2^24");
    if (P->n_classes < 1 || P->n_classes > 32) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": n_classes must be 1 .. 32");
    return LISREG_OK;
}

RnGeom geometry(const lisreg_rangenet_params& P)
{
    RnGeom g;
    g.h = P.img_h; g.w = P.img_w;
    const float fov_up = (float)(P.fov_up / 180.0 * kPi), fov_down = (float)(P.fov_down / 180.0 * kPi);
    g.fov_down_abs = fabsf(fov_down);
    g.fov = fabsf(fov_down) + fabsf(fov_up);
    for (int k = 0; k < 5; ++k) { g.mean[k] = P.means[k]; g.std[k] = P.stds[k]; }
    return g;
}

// the pixel keys: all empty between calls.  They are filled when the buffer is made (or grown), and again only after a call that failed
// between its two launches.
int ensure_keys(lisreg_ctx* c, size_t n_keys)
{
    const size_t bytes = sizeof(unsigned long long) * n_keys;
    if (bytes > c->rn_keys.cap || !c->rn_keys_clean) {
        HIPCHK(c, c->rn_keys.ensure(bytes));
        HIPCHK(c, hipMemsetAsync(c->rn_keys.p, 0xff, c->rn_keys.cap, c->stream));
        c->rn_keys_clean = true;
    }
    return LISREG_OK;
}

// the launch sequence over device sweeps; the valid-pixel counts land in c->rn_hdr_host (pinned) when the call returns
int project_device(lisreg_ctx* c, int n_sweeps, std::vector<RnSweep>& sw, const lisreg_rangenet_params& P)
{
    hipStream_t st = c->stream;
    const RnGeom g = geometry(P);
    const int hw = g.h * g.w, bpi = (hw + 255) / 256;
    int blocks = 0;
    for (auto& s : sw) { s.blk0 = blocks; s.pad0 = s.pad1 = 0; blocks += (s.n + 255) / 256; }
    if (const int rc = ensure_keys(c, (size_t)n_sweeps * (size_t)hw)) return rc;
    HIPCHK(c, c->rn_blk.ensure(sizeof(int) * (size_t)n_sweeps * (size_t)bpi));
    HIPCHK(c, c->rn_hdr.ensure(sizeof(int) * (size_t)n_sweeps));
    if (sizeof(int) * (size_t)n_sweeps > c->rn_hdr_host.cap) {
        HIPCHK(c, hipStreamSynchronize(st));
        HIPCHK(c, c->rn_hdr_host.ensure(sizeof(int) * (size_t)n_sweeps, sizeof(int) * 256));
    }
    const RnSweep* tab = nullptr;
    if (n_sweeps > 1) {                                                 // one sweep travels as a kernel argument
        HIPCHK(c, c->rn_tab.ensure(sizeof(RnSweep) * (size_t)n_sweeps));
        HIPCHK(c, hipMemcpyAsync(c->rn_tab.p, sw.data(), sizeof(RnSweep) * (size_t)n_sweeps, hipMemcpyHostToDevice, st));
        tab = c->rn_tab.as<RnSweep>();
    }
    unsigned long long* keys = c->rn_keys.as<unsigned long long>();
    c->rn_keys_clean = false;
    if (blocks > 0) k_rn_project<<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, g, keys);
    k_rn_pixel<<<n_sweeps * bpi, 256, 0, st>>>(sw[0], tab, bpi, g, keys, c->rn_blk.as<int>());
    k_rn_count<<<n_sweeps, 256, 0, st>>>(bpi, c->rn_blk.as<int>(), c->rn_hdr.as<int>());
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->rn_hdr_host.p, c->rn_hdr.p, sizeof(int) * (size_t)n_sweeps, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));                               // `sw` is the caller's local; the tensor is complete
    c->rn_keys_clean = true;
    return LISREG_OK;
}

int label_device(lisreg_ctx* c, int n_sweeps, std::vector<RnLabelSweep>& sw, const lisreg_rangenet_params& P)
{
    hipStream_t st = c->stream;
    const int hw = P.img_h * P.img_w, bpi = (hw + 255) / 256;
    int blocks = 0, scratch = 0;
    for (auto& s : sw) { s.blk0 = blocks; s.pad0 = s.pad1 = 0; blocks += (s.n + 255) / 256; if (!s.image) ++scratch; }
    if (scratch) {
        HIPCHK(c, c->rn_img.ensure((size_t)scratch * (size_t)hw));
        unsigned char* p = c->rn_img.as<unsigned char>();
        for (auto& s : sw) if (!s.image) { s.image = p; p += hw; }
    }
    const RnLabelSweep* tab = nullptr;
    if (n_sweeps > 1) {
        HIPCHK(c, c->rn_tab.ensure(sizeof(RnLabelSweep) * (size_t)n_sweeps));
        HIPCHK(c, hipMemcpyAsync(c->rn_tab.p, sw.data(), sizeof(RnLabelSweep) * (size_t)n_sweeps, hipMemcpyHostToDevice, st));
        tab = c->rn_tab.as<RnLabelSweep>();
    }
    k_rn_argmax<<<n_sweeps * bpi, 256, 0, st>>>(sw[0], tab, bpi, hw, P.n_classes);
    if (blocks > 0) k_rn_gather<<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, hw);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));                               // `sw` is the caller's local; the records are complete
    return LISREG_OK;
}

int check_knn_params(lisreg_ctx* c, const lisreg_rangenet_params* P, const lisreg_rangenet_knn_params* K, const char* who)
{
    if (!K) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": no kNN parameters");
    if (P->n_classes < 2) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": n_classes must be 2 .. 32");
    if (K->search != 1 && K->search != 3 && K->search != 5 && K->search != 7)
        return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": search must be 1, 3, 5 or 7");
    if (K->knn < 1 || K->knn > K->search * K->search || K->knn > 16)
        return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": knn must be 1 .. min(search^2, 16)");
    if (!(K->sigma > 0.f) || !(K->sigma <= kFltMax)) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": sigma must be finite and > 0");
    if (K->no_vote_label < 0 || K->no_vote_label >= P->n_classes)
        return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": no_vote_label must be 0 .. n_classes - 1");
    return LISREG_OK;
}

// step 3; the parameters have been checked
void knn_weights(const lisreg_rangenet_knn_params& K, float* out)
{
    const int S = K.search, half = (S - 1) / 2;
    const double s = (double)K.sigma;
    double g[49], sum = 0.0;
    for (int j = 0; j < S * S; ++j) {
        const int dy = j / S - half, dx = j % S - half;
        g[j] = exp(-(double)(dx * dx + dy * dy) / (2.0 * s * s));
        sum += g[j];
    }
    for (int j = 0; j < S * S; ++j) out[j] = (float)(1.0 - g[j] / sum);
}

int label_knn_device(lisreg_ctx* c, int n_sweeps, std::vector<RnKnnSweep>& sw, const lisreg_rangenet_params& P, const lisreg_rangenet_knn_params& Kp)
{
    hipStream_t st = c->stream;
    const int hw = P.img_h * P.img_w, bpi = (hw + 255) / 256;
    int blocks = 0, scratch = 0;
    for (auto& s : sw) { s.blk0 = blocks; blocks += (s.n + 255) / 256; if (!s.image) ++scratch; }
    HIPCHK(c, c->rn_rng.ensure(sizeof(unsigned) * (size_t)n_sweeps * (size_t)hw));
    if (scratch) HIPCHK(c, c->rn_img.ensure((size_t)scratch * (size_t)hw));
    unsigned* rp = c->rn_rng.as<unsigned>();
    unsigned char* ip = c->rn_img.as<unsigned char>();
    for (auto& s : sw) {
        s.range = rp; rp += hw;
        if (!s.image) { s.image = ip; ip += hw; }
    }
    const RnKnnSweep* tab = nullptr;
    if (n_sweeps > 1) {
        HIPCHK(c, c->rn_tab.ensure(sizeof(RnKnnSweep) * (size_t)n_sweeps));
        HIPCHK(c, hipMemcpyAsync(c->rn_tab.p, sw.data(), sizeof(RnKnnSweep) * (size_t)n_sweeps, hipMemcpyHostToDevice, st));
        tab = c->rn_tab.as<RnKnnSweep>();
    }
    RnKnn K;
    K.h = P.img_h; K.w = P.img_w; K.knn = Kp.knn; K.no_vote = Kp.no_vote_label; K.cutoff = Kp.cutoff;
    for (float& w : K.wgt) w = 0.f;
    knn_weights(Kp, K.wgt);
    k_rn_argmax_range<<<n_sweeps * bpi, 256, 0, st>>>(sw[0], tab, bpi, hw, P.n_classes);
    if (blocks > 0) {
        k_rn_range_min<<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, hw);
        switch (Kp.search) {
        case 1:  k_rn_knn<1><<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, K); break;
        case 3:  k_rn_knn<3><<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, K); break;
        case 5:  k_rn_knn<5><<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, K); break;
        default: k_rn_knn<7><<<blocks, 256, 0, st>>>(sw[0], tab, n_sweeps, K); break;
        }
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));                               // `sw` is the caller's local; the records are complete
    return LISREG_OK;
}

}  // namespace
}  // namespace lisreg

using namespace lisreg;

int lisreg_default_rangenet_params(lisreg_rangenet_params* p)
{
    if (!p) return LISREG_ERR_ARG;
    p->img_h = 64; p->img_w = 2048; p->fov_up = 3.0; p->fov_down = -25.0;      // the comment at netTensorRT.cpp:144-145
    for (int k = 0; k < 5; ++k) { p->means[k] = 0.0f; p->stds[k] = 1.0f; }   // the model's own, from its arch_cfg.yaml: the caller's
    p->n_classes = 20;
    return LISREG_OK;
}

int lisreg_rangenet_project(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, const lisreg_rangenet_params* P,
                            lisreg_rangenet_out* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!out) return bad(c, "rangenet_project: bad arguments");
    if (const int rc = check_params(c, P, "rangenet_project")) return rc;
    const bool dev = fmt == LISREG_FMT_DEVICE_XYZI;
    if (const int rc = check_cloud(c, "rangenet_project", cloud, n, stride, fmt, kFmtSweep, true)) return rc;
    if (fmt == LISREG_FMT_XYZI && stride < 20) return bad(c, "rangenet_project: XYZI needs stride >= 20 (the intensity is read)");
    if (!out->tensor || !out->invalid_mask || (n > 0 && !out->pixel_index))
        return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project: output buffers missing");
    const size_t hw = (size_t)P->img_h * (size_t)P->img_w;
    std::vector<Span> in, outs = { { out->tensor, hw * 20 }, { out->invalid_mask, hw }, { out->pixel_index, (size_t)n * 4 } };
    if (dev) in.push_back({ cloud, (size_t)n * 16 });
    if (any_overlap(in, outs)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project: an output overlaps the input or another output");
    out->n_valid = 0;
    HIPCHK(c, hipSetDevice(c->device));
    const float4* din = static_cast<const float4*>(cloud);
    if (!dev && n > 0) {                                                // host structs: up as 16-byte records, intensity in the payload
        HIPCHK(c, c->rn_in.ensure(sizeof(float4) * (size_t)n));
        if (const int rc = upload_records(c, cloud, n, stride, fmt == LISREG_FMT_XYZI ? kPackIntensity : LISREG_FMT_XYZI_PACKED, c->rn_in.p)) return rc;
        din = c->rn_in.as<float4>();
    }
    std::vector<RnSweep> sw(1);
    sw[0] = RnSweep{ din, out->tensor, out->invalid_mask, out->pixel_index, n, 0, 0, 0 };
    if (const int rc = project_device(c, 1, sw, *P)) return rc;
    out->n_valid = c->rn_hdr_host.as<int>()[0];
    return LISREG_OK;
}

int lisreg_rangenet_project_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const lisreg_rangenet_params* P,
                                  lisreg_rangenet_out* outs)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_sweeps < 0 || n_sweeps > 256 || (n_sweeps > 0 && (!sweeps || !n || !outs)))
        return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project_batch: bad arguments (at most 256 sweeps)");
    if (const int rc = check_params(c, P, "rangenet_project_batch")) return rc;
    if (n_sweeps == 0) return LISREG_OK;
    const size_t hw = (size_t)P->img_h * (size_t)P->img_w;
    std::vector<RnSweep> sw((size_t)n_sweeps);
    std::vector<Span> in, out;
    long long total = 0;
    for (int s = 0; s < n_sweeps; ++s) {
        const lisreg_rangenet_out& o = outs[s];
        if (n[s] < 0 || (n[s] > 0 && !sweeps[s])) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project_batch: NULL sweep with n > 0");
        if (!o.tensor || !o.invalid_mask || (n[s] > 0 && !o.pixel_index)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project_batch: output buffers missing");
        if ((total += n[s]) > 1000000000LL) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project_batch: too many points");
        sw[(size_t)s] = RnSweep{ static_cast<const float4*>(sweeps[s]), o.tensor, o.invalid_mask, o.pixel_index, n[s], 0, 0, 0 };
        in.push_back({ sweeps[s], (size_t)n[s] * 16 });
        out.push_back({ o.tensor, hw * 20 }); out.push_back({ o.invalid_mask, hw }); out.push_back({ o.pixel_index, (size_t)n[s] * 4 });
    }
    if (any_overlap(in, out)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_project_batch: an output overlaps an input or another output");
    for (int s = 0; s < n_sweeps; ++s) outs[s].n_valid = 0;
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = project_device(c, n_sweeps, sw, *P)) return rc;
    for (int s = 0; s < n_sweeps; ++s) outs[s].n_valid = c->rn_hdr_host.as<int>()[s];
    return LISREG_OK;
}

int lisreg_rangenet_label(lisreg_ctx* c, const void* cloud, int n, int fmt, const int* pixel_index, const unsigned char* invalid_mask,
                          const float* logits, const lisreg_rangenet_params* P, void* labelled_out, unsigned char* label_image_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (n < 0 || (n > 0 && (!cloud || !pixel_index || !labelled_out)) || !invalid_mask || !logits)
        return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label: bad arguments");
    if (const int rc = check_params(c, P, "rangenet_label")) return rc;
    if (fmt != LISREG_FMT_DEVICE_XYZI && fmt != LISREG_FMT_DEVICE) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label: fmt must be DEVICE_XYZI or DEVICE");
    const size_t hw = (size_t)P->img_h * (size_t)P->img_w;
    const std::vector<Span> in = { { cloud, (size_t)n * 16 }, { pixel_index, (size_t)n * 4 }, { invalid_mask, hw }, { logits, hw * 4 * (size_t)P->n_classes } };
    const std::vector<Span> out = { { labelled_out, (size_t)n * 16 }, { label_image_out, label_image_out ? hw : 0 } };
    if (any_overlap(in, out)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label: an output overlaps an input or the other output");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<RnLabelSweep> sw(1);
    sw[0] = RnLabelSweep{ static_cast<const float4*>(cloud), pixel_index, invalid_mask, logits, static_cast<float4*>(labelled_out), label_image_out, n, 0, 0, 0 };
    return label_device(c, 1, sw, *P);
}

int lisreg_rangenet_label_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const int* const* pixel_index,
                                const unsigned char* const* invalid_mask, const float* const* logits, const lisreg_rangenet_params* P,
                                void* const* labelled_out, unsigned char* const* label_image_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_sweeps < 0 || n_sweeps > 256 || (n_sweeps > 0 && (!sweeps || !n || !pixel_index || !invalid_mask || !logits || !labelled_out)))
        return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_batch: bad arguments (at most 256 sweeps)");
    if (const int rc = check_params(c, P, "rangenet_label_batch")) return rc;
    if (n_sweeps == 0) return LISREG_OK;
    const size_t hw = (size_t)P->img_h * (size_t)P->img_w;
    std::vector<RnLabelSweep> sw((size_t)n_sweeps);
    std::vector<Span> in, out;
    long long total = 0;
    for (int s = 0; s < n_sweeps; ++s) {
        if (n[s] < 0 || (n[s] > 0 && (!sweeps[s] || !pixel_index[s] || !labelled_out[s])) || !invalid_mask[s] || !logits[s])
            return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_batch: NULL buffer");
        if ((total += n[s]) > 1000000000LL) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_batch: too many points");
        unsigned char* img = label_image_out ? label_image_out[s] : nullptr;
        sw[(size_t)s] = RnLabelSweep{ static_cast<const float4*>(sweeps[s]), pixel_index[s], invalid_mask[s], logits[s],
                                      static_cast<float4*>(labelled_out[s]), img, n[s], 0, 0, 0 };
        in.push_back({ sweeps[s], (size_t)n[s] * 16 }); in.push_back({ pixel_index[s], (size_t)n[s] * 4 });
        in.push_back({ invalid_mask[s], hw }); in.push_back({ logits[s], hw * 4 * (size_t)P->n_classes });
        out.push_back({ labelled_out[s], (size_t)n[s] * 16 }); out.push_back({ img, img ? hw : 0 });
    }
    if (any_overlap(in, out)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_batch: an output overlaps an input or another output");
    HIPCHK(c, hipSetDevice(c->device));
    return label_device(c, n_sweeps, sw, *P);
}

int lisreg_default_rangenet_knn_params(lisreg_rangenet_knn_params* p)
{
    if (!p) return LISREG_ERR_ARG;
    p->knn = 5; p->search = 5; p->sigma = 1.0f; p->cutoff = 1.0f;      // the `post: KNN: params:` block of the authors' arch_cfg.yaml
    p->no_vote_label = 0;
    return LISREG_OK;
}

void lisreg_rangenet_knn_weights(const lisreg_rangenet_knn_params* K, float* out)
{
    if (!K || !out || (K->search != 1 && K->search != 3 && K->search != 5 && K->search != 7) || !(K->sigma > 0.f) || !(K->sigma <= kFltMax)) return;
    knn_weights(*K, out);
}

int lisreg_rangenet_label_knn(lisreg_ctx* c, const void* cloud, int n, int fmt, const int* pixel_index, const unsigned char* invalid_mask,
                              const float* logits, const lisreg_rangenet_params* P, const lisreg_rangenet_knn_params* K, void* labelled_out,
                              unsigned char* label_image_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (n < 0 || (n > 0 && (!cloud || !pixel_index || !labelled_out)) || !invalid_mask || !logits)
        return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn: bad arguments");
    if (const int rc = check_params(c, P, "rangenet_label_knn")) return rc;
    if (const int rc = check_knn_params(c, P, K, "rangenet_label_knn")) return rc;
    if (fmt != LISREG_FMT_DEVICE_XYZI && fmt != LISREG_FMT_DEVICE) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn: fmt must be DEVICE_XYZI or DEVICE");
    const size_t hw = (size_t)P->img_h * (size_t)P->img_w;
    const std::vector<Span> in = { { cloud, (size_t)n * 16 }, { pixel_index, (size_t)n * 4 }, { invalid_mask, hw }, { logits, hw * 4 * (size_t)P->n_classes } };
    const std::vector<Span> out = { { labelled_out, (size_t)n * 16 }, { label_image_out, label_image_out ? hw : 0 } };
    if (any_overlap(in, out)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn: an output overlaps an input or the other output");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<RnKnnSweep> sw(1);
    sw[0] = RnKnnSweep{ static_cast<const float4*>(cloud), pixel_index, invalid_mask, logits, static_cast<float4*>(labelled_out), label_image_out, nullptr, n, 0 };
    return label_knn_device(c, 1, sw, *P, *K);
}

int lisreg_rangenet_label_knn_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const int* const* pixel_index,
                                    const unsigned char* const* invalid_mask, const float* const* logits, const lisreg_rangenet_params* P,
                                    const lisreg_rangenet_knn_params* K, void* const* labelled_out, unsigned char* const* label_image_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_sweeps < 0 || n_sweeps > 256 || (n_sweeps > 0 && (!sweeps || !n || !pixel_index || !invalid_mask || !logits || !labelled_out)))
        return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn_batch: bad arguments (at most 256 sweeps)");
    if (const int rc = check_params(c, P, "rangenet_label_knn_batch")) return rc;
    if (const int rc = check_knn_params(c, P, K, "rangenet_label_knn_batch")) return rc;
    if (n_sweeps == 0) return LISREG_OK;
    const size_t hw = (size_t)P->img_h * (size_t)P->img_w;
    std::vector<RnKnnSweep> sw((size_t)n_sweeps);
    std::vector<Span> in, out;
    long long total = 0;
    for (int s = 0; s < n_sweeps; ++s) {
        if (n[s] < 0 || (n[s] > 0 && (!sweeps[s] || !pixel_index[s] || !labelled_out[s])) || !invalid_mask[s] || !logits[s])
            return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn_batch: NULL buffer");
        if ((total += n[s]) > 1000000000LL) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn_batch: too many points");
        unsigned char* img = label_image_out ? label_image_out[s] : nullptr;
        sw[(size_t)s] = RnKnnSweep{ static_cast<const float4*>(sweeps[s]), pixel_index[s], invalid_mask[s], logits[s],
                                    static_cast<float4*>(labelled_out[s]), img, nullptr, n[s], 0 };
        in.push_back({ sweeps[s], (size_t)n[s] * 16 }); in.push_back({ pixel_index[s], (size_t)n[s] * 4 });
        in.push_back({ invalid_mask[s], hw }); in.push_back({ logits[s], hw * 4 * (size_t)P->n_classes });
        out.push_back({ labelled_out[s], (size_t)n[s] * 16 }); out.push_back({ img, img ? hw : 0 });
    }
    if (any_overlap(in, out)) return ctx_fail(c, LISREG_ERR_ARG, "rangenet_label_knn_batch: an output overlaps an input or another output");
    HIPCHK(c, hipSetDevice(c->device));
    return label_knn_device(c, n_sweeps, sw, *P, *K);
}
