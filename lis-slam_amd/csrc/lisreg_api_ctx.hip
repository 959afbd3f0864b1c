// lisreg_api_ctx.hip — what every translation unit behind the C ABI shares (declared in lisreg_ctx.hpp): the error text, the argument
// checks of a cloud, the packing and staging of host clouds, the aligned cloud an align() hands out, the bounding-box read-back, the sort scratch and the grid geometry.
// Host code only: no kernel lives here.
#include "lisreg_ctx.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace lisreg {

static thread_local std::string g_static_err;      // the text of a failure without a context (lisreg_create, lisreg_comm_unique_id)
int ctx_fail(lisreg_ctx* c, int code, const std::string& msg)
{
    if (c) c->err = msg; else g_static_err = msg;
    return code;
}

int bad(lisreg_ctx* c, const std::string& msg) { return ctx_fail(c, LISREG_ERR_ARG, msg); }

int check_cloud(lisreg_ctx* c, const char* who, const void* cloud, int n, int stride, int fmt, unsigned accepted_formats, bool allow_empty)
{
    if (n < 0 || (n == 0 && !allow_empty)) return bad(c, std::string(who) + (allow_empty ? ": n < 0" : ": n <= 0"));
    if (n > 0 && !cloud) return bad(c, std::string(who) + ": NULL cloud with n > 0");
    if (fmt < 0 || fmt >= 32 || !(accepted_formats & fmt_bit(fmt))) return bad(c, std::string(who) + ": this fmt is not accepted here");
    if (fmt_bit(fmt) & kFmtDevice) return LISREG_OK;                        // 16-byte records: the stride is not read
    const int need = fmt == LISREG_FMT_XYZIL ? 22 : (fmt == LISREG_FMT_XYZI_PACKED ? 16 : 12);
    if (stride < need) return bad(c, std::string(who) + ": stride < " + std::to_string(need) + " for this fmt");
    return LISREG_OK;
}

bool spans_overlap(const void* a, size_t na, const void* b, size_t nb)
{
    if (!a || !b || na == 0 || nb == 0) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}


bool ensure_side_stream(lisreg_ctx* c)
{
    if (!c->side_stream && (c->side_stream.create(hipStreamNonBlocking) != hipSuccess || c->ev_fork.create(hipEventDisableTiming) != hipSuccess ||
                            c->ev_join.create(hipEventDisableTiming) != hipSuccess)) {
        c->side_stream.reset(); c->ev_fork.reset(); c->ev_join.reset();
    }
    return c->side_stream != nullptr;
}

// pack PCL structs (stride/format of common.h:9,25-35) into 16-B device records
void pack_cloud(const void* cloud, int n, int stride, int fmt, lisreg_dpoint* out)
{
    const unsigned char* b = static_cast<const unsigned char*>(cloud);
    for (int i = 0; i < n; ++i) {
        const unsigned char* r = b + (size_t)i * (size_t)stride;
        memcpy(&out[i], r, 12);
        uint16_t lab = 0;
        if (fmt == LISREG_FMT_XYZIL) memcpy(&lab, r + 20, 2);
        out[i].payload = lab;
    }
}

int upload_packed(lisreg_ctx* c, const lisreg_dpoint* h, size_t n, DevBuf& into)
{
    HIPCHK(c, into.ensure(sizeof(float4) * std::max<size_t>(n, 1)));
    if (n > 0) {                      // on the context's stream: behind whatever still reads `into` there
        HIPCHK(c, hipMemcpyAsync(into.p, h, sizeof(float4) * n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));      // h is the caller's local
    }
    return LISREG_OK;
}

int stage_records(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, DevBuf& into, const float4** out)
{
    if (fmt == LISREG_FMT_DEVICE) { *out = static_cast<const float4*>(cloud); return LISREG_OK; }
    std::vector<lisreg_dpoint> h((size_t)std::max(n, 1));
    pack_cloud(cloud, n, stride, fmt, h.data());
    if (const int rc = upload_packed(c, h.data(), (size_t)std::max(n, 0), into)) return rc;
    *out = into.as<float4>();
    return LISREG_OK;
}

int emit_aligned(lisreg_ctx* c, const float4* raw, int n, const float Rt[12], const void* source, int stride, int fmt, DevBuf& scratch,
                 void* aligned_out)
{
    hipStream_t st = c->stream;
    HIPCHK(c, c->vox_M.ensure(sizeof(float) * 12));
    HIPCHK(c, hipMemcpyAsync(c->vox_M.p, Rt, sizeof(float) * 12, hipMemcpyHostToDevice, st));
    if (fmt == LISREG_FMT_DEVICE) {
        launch_transform_cloud(raw, n, c->vox_M.as<float>(), static_cast<float4*>(aligned_out), st);
        HIPCHK(c, hipStreamSynchronize(st));
        return LISREG_OK;
    }
    HIPCHK(c, scratch.ensure(sizeof(float4) * (size_t)n));
    launch_transform_cloud(raw, n, c->vox_M.as<float>(), scratch.as<float4>(), st);
    std::vector<float4> hp((size_t)n);
    HIPCHK(c, hipMemcpyAsync(hp.data(), scratch.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const unsigned char* b = static_cast<const unsigned char*>(source);
    unsigned char* o = static_cast<unsigned char*>(aligned_out);
    for (int i = 0; i < n; ++i) {
        if (o != b) memcpy(o + (size_t)i * (size_t)stride, b + (size_t)i * (size_t)stride, (size_t)stride);
        memcpy(o + (size_t)i * (size_t)stride, &hp[(size_t)i], 12);
    }
    return LISREG_OK;
}

int cloud_bbox(lisreg_ctx* c, const float4* pts, int n, float bb[6])
{
    HIPCHK(c, c->bbox_dev.ensure(sizeof(float) * 8));
    HIPCHK(c, c->bbox_scratch.ensure(sizeof(float) * 6 * 256));
    launch_bbox(pts, n, c->bbox_dev.as<float>(), c->bbox_scratch.as<float>(), c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(bb, c->bbox_dev.p, sizeof(float) * 6, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return LISREG_OK;
}

SortBuffers sort_buffers(lisreg_ctx* c)
{
    SortBuffers sb;
    sb.hist = c->hist.as<int>(); sb.bucket_start = c->bucket_start.as<int>(); sb.scan_tmp = c->scan_tmp.as<int>();
    sb.elem_bucket = c->elem_bucket.as<uint32_t>(); sb.elem_sub = c->elem_sub.as<uint32_t>();
    sb.tmp_bucket = c->tmp_bucket.as<uint32_t>(); sb.tmp_sub = c->tmp_sub.as<uint32_t>();
    sb.tmp_idx = c->tmp_idx.as<int>();
    sb.tmp_pts = c->tmp_pts.as<float4>();
    return sb;
}

int ensure_sort_scratch(lisreg_ctx* c, size_t n_elems, size_t n_buckets)
{
    HIPCHK(c, c->hist.ensure(sizeof(int) * (n_buckets + 1)));
    HIPCHK(c, c->bucket_start.ensure(sizeof(int) * (n_buckets + 2)));
    HIPCHK(c, c->scan_tmp.ensure(sizeof(int) * (n_buckets / 2048 + 4)));
    HIPCHK(c, c->elem_bucket.ensure(sizeof(uint32_t) * (n_elems + 1)));
    HIPCHK(c, c->elem_sub.ensure(sizeof(uint32_t) * (n_elems + 1)));
    HIPCHK(c, c->tmp_bucket.ensure(sizeof(uint32_t) * (n_elems + 1)));
    HIPCHK(c, c->tmp_sub.ensure(sizeof(uint32_t) * (n_elems + 1)));
    HIPCHK(c, c->tmp_idx.ensure(sizeof(int) * (n_elems + 1)));
    HIPCHK(c, c->tmp_pts.ensure(sizeof(float4) * (n_elems + 1)));
    return LISREG_OK;
}

// grid geometry from a bounding box; cell edge grows if the box would need too many cells
void make_grid(const float bb_in[6], int n, GridIndex* g, int* n_cells, int margin_cells)
{
    float bb[6] = { bb_in[0], bb_in[1], bb_in[2], bb_in[3], bb_in[4], bb_in[5] };
    memset(g, 0, sizeof *g);
    g->n = n;
    // Cell edge: 0.5 m is the measured optimum for the 200 k-point submap of BASELINE configs[1]; the optimum
    // scales with the point spacing, so denser maps get smaller cells (footprint density as the proxy: lidar maps are
    // surfaces over a ground plane).  1 M points over the same 80 x 80 m: 0.25 m, +14 % registrations/s.
    float cell = 0.5f;
    if (n > 0) {
        const double area = std::max(1.0, (double)(bb[3] - bb[0]) * (double)(bb[4] - bb[1]));
        cell = (float)std::min(0.5, std::max(0.25, 2.8 / std::sqrt((double)n / area)));
    }
    if (n <= 0) { g->cell = cell; g->inv_cell = 1.f / cell; g->nx = g->ny = g->nz = 0; *n_cells = 1; return; }
    const double max_cells = 1 << 24;
    // registration targets: the grid reaches `margin_cells` cells past the cloud on every side, so that a query a pose error away from
    // a wall that bounds the cloud still has a cell of its own (cell rows, search_mode 5); empty cells cost four bytes of table each
    const float bb0[6] = { bb[0], bb[1], bb[2], bb[3], bb[4], bb[5] };
    for (;;) {
        for (int d = 0; d < 3; ++d) { bb[d] = bb0[d] - (float)margin_cells * cell; bb[3 + d] = bb0[3 + d] + (float)margin_cells * cell; }
        double nx = floor((bb[3] - bb[0]) / cell) + 1, ny = floor((bb[4] - bb[1]) / cell) + 1,
               nz = floor((bb[5] - bb[2]) / cell) + 1;
        if (nx * ny * nz <= max_cells) { g->nx = (int)nx; g->ny = (int)ny; g->nz = (int)nz; break; }
        cell *= 1.26f;
    }
    g->ox = bb[0]; g->oy = bb[1]; g->oz = bb[2];
    g->cell = cell; g->inv_cell = 1.f / cell;
    *n_cells = g->nx * g->ny * g->nz;
}

}  // namespace lisreg

extern "C" {

const char* lisreg_last_error(const lisreg_ctx* c) { return c ? c->err.c_str() : lisreg::g_static_err.c_str(); }

// pcl::getTransformation via trans2Affine3f (src/core/common.cpp:54-57)
void lisreg_pose_to_matrix(const float T[6], float M[12])
{
    float A = cosf(T[2]), B = sinf(T[2]), C = cosf(T[1]), D = sinf(T[1]), E = cosf(T[0]), F = sinf(T[0]);
    float DE = D * E, DF = D * F;
    M[0] = A * C;  M[1] = A * DF - B * E;  M[2]  = B * F + A * DE;  M[3]  = T[3];
    M[4] = B * C;  M[5] = A * E + B * DF;  M[6]  = B * DE - A * F;  M[7]  = T[4];
    M[8] = -D;     M[9] = C * F;           M[10] = C * E;           M[11] = T[5];
}

}  // extern "C"
