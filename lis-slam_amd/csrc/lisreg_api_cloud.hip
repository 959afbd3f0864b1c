// lisreg_api_cloud.hip — C-ABI entry points of SURVEY.md §8 f-1: the voxel grid of one cloud and of K clouds at once, the concatenation of
// device clouds and the rigid transform of a cloud; and, from the same pcl::VoxelGrid keys, the voxel sort and the dense voxel table the
// NDT and VGICP targets are built on (voxel_sort_cloud, voxel_table_build; declared in lisreg_ctx.hpp).  Kernels: lisreg_index.hip,
// lisreg_features.hip.  Host code only.
#include "lisreg_ctx.hpp"
#include "lisreg_voxel_shared.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

using namespace lisreg;

int lisreg::voxel_sort_cloud(lisreg_ctx* c, const char* who, const float4* pts, int n, VoxelDesc d, long long total, int mark, int* n_vox)
{
    hipStream_t st = c->stream;
    const long long max_buckets = 1LL << 22;
    d.span = (uint32_t)std::max(1LL, (total + max_buckets - 1) / max_buckets);
    const int n_buckets = (int)((total + d.span - 1) / d.span);
    const int rc = ensure_sort_scratch(c, (size_t)n, (size_t)std::max(n_buckets, n) + 1);
    if (rc) return rc;
    HIPCHK(c, c->vox_order.ensure(sizeof(int) * (size_t)n));
    HIPCHK(c, c->vox_sidx.ensure(sizeof(uint32_t) * (size_t)n));
    HIPCHK(c, c->vox_head.ensure(sizeof(int) * ((size_t)n + 1)));
    HIPCHK(c, c->vox_slot.ensure(sizeof(int) * ((size_t)n + 2)));
    if (mark >= 0) ctx_prof_mark(c, mark);
    launch_voxel_sort(pts, n, d, n_buckets, sort_buffers(c), c->vox_order.as<int>(), c->vox_sidx.as<uint32_t>(), c->vox_head.as<int>(),
                      c->vox_slot.as<int>(), st);
    *n_vox = 0;
    HIPCHK(c, hipMemcpyAsync(n_vox, c->vox_slot.as<int>() + n, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    if (*n_vox < 1 || *n_vox > n) return ctx_fail(c, LISREG_ERR_HIP, std::string(who) + ": the voxel sort returned an impossible voxel count");
    return LISREG_OK;
}

// The geometry of the dense voxel table over the finite box bb at `resolution`: pcl::VoxelGrid's min_b / div_b and the sort's keys
// (d->span is left to the sort).  The one copy, for voxel_table_build below and for lisreg_vgicp_set_target_batch, which decides every
// target's table on the host between its phases.  false: *why is the refusal's text behind "<who>: ".  Host arithmetic only.
bool lisreg::voxel_table_geometry(const float bb[6], double resolution, const char* table_word, int min_b[3], int dims[3], VoxelDesc* d,
                                  long long* total, std::string* why)
{
    const float inv = 1.0f / (float)resolution;
    const long long max_cells = 1LL << 26;
    for (int k = 0; k < 3; ++k) {
        const double lo = floor((double)(bb[k] * inv)), hi = floor((double)(bb[3 + k] * inv));
        if (!(fabs(lo) < 2.0e9 && fabs(hi) < 2.0e9)) { *why = "the grid has more than 2^26 cells (resolution too small for this cloud)"; return false; }
    }
    long long div_b[3];
    voxel_bounds(bb, inv, min_b, div_b);
    if (div_b[0] > max_cells || div_b[1] > max_cells || div_b[2] > max_cells || div_b[0] * div_b[1] > max_cells ||
        div_b[0] * div_b[1] * div_b[2] > max_cells) {
        *why = std::string("the grid has more than 2^26 cells (the ") + table_word + " is dense; resolution too small for this cloud)";
        return false;
    }
    *total = div_b[0] * div_b[1] * div_b[2];
    for (int k = 0; k < 3; ++k) dims[k] = (int)div_b[k];
    memset(d, 0, sizeof *d);
    d->inv_leaf = inv; d->min_b0 = min_b[0]; d->min_b1 = min_b[1]; d->min_b2 = min_b[2];
    d->mul1 = dims[0]; d->mul2 = dims[0] * dims[1];
    d->span = 1u;
    return true;
}

// The shared build of the NDT and the VGICP target: pcl::VoxelGrid's keys, so both families see the voxels
// lisreg_voxel_downsample sees, in the same order
int lisreg::voxel_table_build(lisreg_ctx* c, const char* who, const char* table_word, const float4* pts, int n, const float bb[6],
                              double resolution, int mark, VoxelTable& T)
{
    hipStream_t st = c->stream;
    VoxelDesc d;
    long long total = 0;
    std::string why;
    if (!voxel_table_geometry(bb, resolution, table_word, T.min_b, T.dims, &d, &total, &why)) return bad(c, std::string(who) + ": " + why);
    int n_vox = 0;
    const int rc = voxel_sort_cloud(c, who, pts, n, d, total, mark, &n_vox);
    if (rc) return rc;
    HIPCHK(c, c->vox_start.ensure(sizeof(int) * ((size_t)n_vox + 2)));
    launch_voxel_starts(n, c->vox_head.as<int>(), c->vox_slot.as<int>(), c->vox_start.as<int>(), st);
    HIPCHK(c, T.stats.ensure(sizeof(double) * kVoxelRec * (size_t)n_vox));
    HIPCHK(c, T.cell.ensure(sizeof(int) * (size_t)n_vox));
    HIPCHK(c, T.table.ensure(sizeof(int) * (size_t)total));
    HIPCHK(c, hipMemsetAsync(T.table.p, 0xFF, sizeof(int) * (size_t)total, st));
    T.n_voxels = n_vox; T.resolution = resolution;
    return LISREG_OK;
}

VoxelView lisreg::voxel_table_view(const VoxelTable& T)
{
    VoxelView G;
    G.stats = T.stats.as<double>(); G.table = T.table.as<int>();
    G.d0 = T.dims[0]; G.d1 = T.dims[1]; G.d2 = T.dims[2];
    G.m0 = T.min_b[0]; G.m1 = T.min_b[1]; G.m2 = T.min_b[2];
    G.inv_res = 1.0 / T.resolution;
    return G;
}

int lisreg::voxel_table_read(lisreg_ctx* c, const VoxelTable& T, const DevBuf* flag, int* cell_ids, int* counts, double* means, double* sym6,
                             int capacity)
{
    const size_t nv = (size_t)T.n_voxels;
    std::vector<double> st(nv * kVoxelRec);
    std::vector<int> ce(nv), fl(flag ? nv : 0);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(st.data(), T.stats.p, sizeof(double) * st.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ce.data(), T.cell.p, sizeof(int) * nv, hipMemcpyDeviceToHost, c->stream));
    if (flag) HIPCHK(c, hipMemcpyAsync(fl.data(), flag->p, sizeof(int) * nv, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int m = 0;
    for (size_t v = 0; v < nv && m < capacity; ++v) {
        if (flag && !fl[v]) continue;
        const double* r = &st[v * kVoxelRec];
        cell_ids[m] = ce[v]; counts[m] = (int)r[9];
        memcpy(means + 3 * (size_t)m, r, sizeof(double) * 3);
        memcpy(sym6 + 6 * (size_t)m, r + 3, sizeof(double) * 6);
        ++m;
    }
    return LISREG_OK;
}

extern "C" {

// ---- §8 f-1: voxel-grid down-sampling and cloud transform --------------------------------------------------------------
int lisreg_voxel_downsample(lisreg_ctx* c, const void* in, int n, int stride, int fmt, float leaf, void* out,
                            int out_capacity, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!n_out || !(leaf > 0.f) || (n > 0 && !out)) return bad(c, "voxel_downsample: bad arguments");
    const bool dev = fmt == LISREG_FMT_DEVICE || fmt == LISREG_FMT_DEVICE_XYZI;
    // (any other value of fmt is read as XYZI structs)
    if (const int rc = check_cloud(c, "voxel_downsample", in, n, stride, dev || fmt == LISREG_FMT_XYZIL ? fmt : LISREG_FMT_XYZI,
                                   kFmtDevice | fmt_bit(LISREG_FMT_XYZI) | fmt_bit(LISREG_FMT_XYZIL), true)) return rc;
    *n_out = 0;
    if (n == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool has_intensity = !dev && stride >= 20;
    // ---- stage the input as float4 (x,y,z, intensity | payload) [+ labels] ---------------------------------------
    const float4* pts = nullptr;
    const uint32_t* labels = nullptr;
    std::vector<float4> h_pts;
    std::vector<uint32_t> h_lab;
    if (dev) pts = static_cast<const float4*>(in);
    else {
        h_pts.resize((size_t)n);
        if (fmt == LISREG_FMT_XYZIL) h_lab.resize((size_t)n);
        const unsigned char* b = static_cast<const unsigned char*>(in);
        for (int i = 0; i < n; ++i) {
            const unsigned char* r = b + (size_t)i * (size_t)stride;
            float v[3], it = 0.f;
            memcpy(v, r, 12);
            if (has_intensity) memcpy(&it, r + 16, 4);
            h_pts[(size_t)i] = make_float4(v[0], v[1], v[2], it);
            if (fmt == LISREG_FMT_XYZIL) { uint16_t l; memcpy(&l, r + 20, 2); h_lab[(size_t)i] = l; }
        }
        HIPCHK(c, c->vox_in.ensure(sizeof(float4) * (size_t)n));
        HIPCHK(c, hipMemcpyAsync(c->vox_in.p, h_pts.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, st));
        pts = c->vox_in.as<float4>();
        if (fmt == LISREG_FMT_XYZIL) {
            HIPCHK(c, c->vox_lab.ensure(sizeof(uint32_t) * (size_t)n));
            HIPCHK(c, hipMemcpyAsync(c->vox_lab.p, h_lab.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
            labels = c->vox_lab.as<uint32_t>();
        }
    }
    // ---- getMinMax3D + grid geometry (voxel_grid.hpp) -------------------------------------------------------------
    float bb[6];
    if (const int rc = cloud_bbox(c, pts, n, bb)) return rc;
    for (int k = 0; k < 6; ++k)       // the reference strips non-finite returns before any filter (pcl::removeNaNFromPointCloud)
        if (!std::isfinite(bb[k])) return bad(c, "voxel_downsample: the cloud has infinite coordinates");
    VoxelDesc d;
    long long total = 0;
    if (!voxel_geometry(bb, leaf, &d, &total)) {           // "Leaf size is too small for the input dataset": output = input
        if (n > out_capacity) { *n_out = n; return bad(c, "voxel_downsample: out_capacity too small"); }
        if (dev) { if (out != in) HIPCHK(c, hipMemcpyAsync(out, in, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, st)); }
        else if (out != in) memmove(out, in, (size_t)n * (size_t)stride);
        HIPCHK(c, hipStreamSynchronize(st));
        *n_out = n;
        return LISREG_LEAF_TOO_SMALL;
    }
    // ---- sort by voxel index, count voxels ------------------------------------------------------------------------
    int n_vox = 0;
    if (const int rc = voxel_sort_cloud(c, "voxel_downsample", pts, n, d, total, -1, &n_vox)) return rc;
    *n_out = n_vox;
    if (n_vox > out_capacity) return bad(c, "voxel_downsample: out_capacity too small (see *n_out)");
    // ---- centroids ---------------------------------------------------------------------------------------------------
    HIPCHK(c, c->vox_start.ensure(sizeof(int) * ((size_t)n_vox + 2)));
    // in place (out inside the input records — lisreg_localmap_extract grids a class cloud onto itself): the centroid kernels read
    // pts[order[..]] while other threads write out[v], so the result is formed in scratch and copied over the input afterwards
    const bool aliased = dev && (const char*)out < (const char*)in + sizeof(float4) * (size_t)n &&
                         (const char*)in < (const char*)out + sizeof(float4) * (size_t)std::max(out_capacity, 1);
    float4* out_pts = dev && !aliased ? static_cast<float4*>(out) : nullptr;
    if (!out_pts) { HIPCHK(c, c->vox_out.ensure(sizeof(float4) * (size_t)std::max(n_vox, 1))); out_pts = c->vox_out.as<float4>(); }
    uint32_t* out_lab = nullptr;
    if (fmt == LISREG_FMT_XYZIL) { HIPCHK(c, c->vox_outlab.ensure(sizeof(uint32_t) * (size_t)n_vox)); out_lab = c->vox_outlab.as<uint32_t>(); }
    launch_voxel_centroids(n, n_vox, pts, labels, fmt == LISREG_FMT_DEVICE ? 1 : 0 /* label vote on the payload, else .w averaged */, c->vox_order.as<int>(), c->vox_head.as<int>(),
                           c->vox_slot.as<int>(), c->vox_start.as<int>(), out_pts, out_lab, st);
    HIPCHK(c, hipGetLastError());
    if (!dev) {
        std::vector<float4> r((size_t)n_vox);
        std::vector<uint32_t> rl(fmt == LISREG_FMT_XYZIL ? (size_t)n_vox : 0);
        HIPCHK(c, hipMemcpyAsync(r.data(), out_pts, sizeof(float4) * (size_t)n_vox, hipMemcpyDeviceToHost, st));
        if (out_lab) HIPCHK(c, hipMemcpyAsync(rl.data(), out_lab, sizeof(uint32_t) * (size_t)n_vox, hipMemcpyDeviceToHost, st));
        HIPCHK(c, hipStreamSynchronize(st));
        unsigned char* o = static_cast<unsigned char*>(out);
        for (int i = 0; i < n_vox; ++i) {
            unsigned char* q = o + (size_t)i * (size_t)stride;
            memset(q, 0, (size_t)stride);
            memcpy(q, &r[(size_t)i], 12);
            if (has_intensity) memcpy(q + 16, &r[(size_t)i].w, 4);
            if (out_lab) { const uint16_t l = (uint16_t)rl[(size_t)i]; memcpy(q + 20, &l, 2); }
        }
    } else {
        if (aliased && n_vox > 0) HIPCHK(c, hipMemcpyAsync(out, out_pts, sizeof(float4) * (size_t)n_vox, hipMemcpyDeviceToDevice, st));
        HIPCHK(c, hipStreamSynchronize(st));
    }
    return LISREG_OK;
}

// K device clouds through ONE launch sequence (one sort keyed by (cloud, voxel index), one centroid launch) with three host round trips
// in all — the K bounding boxes, the K voxel counts — instead of ~12 launches and three round trips per cloud: the five class grids of a
// key frame (subMapOptmizationNode.cpp:806-811) or of extractSlidingCloud (:1385-1389) are launch-bound, not bandwidth-bound.
// Results are those of K lisreg_voxel_downsample calls, bit for bit (same sort order inside every cloud, same sequential sums).
int lisreg_voxel_downsample_multi(lisreg_ctx* c, int k, const void* const* in, const int* n, const float* leaf, int fmt,
                                  void* const* out, const int* out_capacity, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (k < 0 || (k > 0 && (!in || !n || !leaf || !out || !out_capacity || !n_out))) return bad(c, "voxel_downsample_multi: bad arguments");
    if (fmt != LISREG_FMT_DEVICE && fmt != LISREG_FMT_DEVICE_XYZI) return bad(c, "voxel_downsample_multi: device records only (LISREG_FMT_DEVICE / _DEVICE_XYZI)");
    for (int s = 0; s < k; ++s) {
        if (n[s] < 0 || !(leaf[s] > 0.f) || (n[s] > 0 && (!in[s] || !out[s]))) return bad(c, "voxel_downsample_multi: bad cloud");
        n_out[s] = 0;
    }
    auto one_by_one = [&]() -> int {
        for (int s = 0; s < k; ++s) {
            int rc = lisreg_voxel_downsample(c, in[s], n[s], 16, fmt, leaf[s], out[s], out_capacity[s], &n_out[s]);
            if (rc != LISREG_OK && rc != LISREG_LEAF_TOO_SMALL) return rc;
        }
        return LISREG_OK;
    };
    long long total_n = 0;
    int live = 0;
    for (int s = 0; s < k; ++s) { total_n += n[s]; live += n[s] > 0; }
    if (live <= 1 || k > kVoxelMultiMax || total_n > 2000000000LL) return one_by_one();
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int N = (int)total_n;
    // ---- concatenate, K bounding boxes, one round trip ---------------------------------------------------------------------------
    HIPCHK(c, c->vox_in.ensure(sizeof(float4) * (size_t)N));
    HIPCHK(c, c->bbox_dev.ensure(sizeof(float) * 6 * kVoxelMultiMax));
    HIPCHK(c, c->bbox_scratch.ensure(sizeof(float) * 6 * 256 * kVoxelMultiMax));
    VoxelMulti m;
    memset(&m, 0, sizeof m);
    m.k = k;
    float4* cat = c->vox_in.as<float4>();
    for (int s = 0, o = 0; s < k; ++s) {
        m.off[s] = o;
        o += n[s];
        m.off[s + 1] = o;
    }
    {
        BboxJobs jobs;
        memset(&jobs, 0, sizeof jobs);
        jobs.k = k;
        for (int s = 0; s < k; ++s) { jobs.pts[s] = static_cast<const float4*>(in[s]); jobs.n[s] = n[s]; }
        launch_concat_jobs(jobs, m, cat, st);                  // one launch instead of K copies
    }
    launch_bbox_multi(cat, m, c->bbox_dev.as<float>(), c->bbox_scratch.as<float>(), st);
    float bb[6 * kVoxelMultiMax];
    HIPCHK(c, hipMemcpyAsync(bb, c->bbox_dev.p, sizeof(float) * 6 * (size_t)k, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // ---- per-cloud geometry (voxel_grid.hpp), one common bucket span ----------------------------------------------------------
    long long totals[kVoxelMultiMax] = { 0 }, sum_total = 0;
    for (int s = 0; s < k; ++s) {
        if (n[s] == 0) continue;
        const float* b = bb + 6 * s;
        for (int q = 0; q < 6; ++q) if (!std::isfinite(b[q])) return bad(c, "voxel_downsample_multi: a cloud has infinite coordinates");
        if (!voxel_geometry(b, leaf[s], &m.d[s], &totals[s])) return one_by_one();      // "leaf size too small" for one of them: the single-cloud path knows what to do
        sum_total += totals[s];
    }
    if (sum_total >= (1LL << 32)) return one_by_one();                 // the joint voxel index has to fit 32 bits
    // every cloud its own bucket span (a cloud with a tiny leaf must not coarsen the others' buckets: the rank pass is quadratic inside
    // a bucket), at most 2^22 buckets in all
    const long long max_buckets = (1LL << 22) / k;
    long long nb = 0, ib = 0;
    for (int s = 0; s < k; ++s) {
        const uint32_t span = (uint32_t)std::max(1LL, (totals[s] + max_buckets - 1) / max_buckets);
        m.d[s].span = span;
        m.bucket_base[s] = (int)nb;
        m.idx_base[s] = (uint32_t)ib;
        nb += (totals[s] + span - 1) / span;
        ib += totals[s];
    }
    m.bucket_base[k] = (int)nb;
    m.idx_base[k] = (uint32_t)ib;
    const int n_buckets = (int)std::max(nb, 1LL);
    // ---- one sort, the K voxel counts in one round trip -------------------------------------------------------------------------
    int rc = ensure_sort_scratch(c, (size_t)N, (size_t)std::max(n_buckets, N) + 1);
    if (rc) return rc;
    HIPCHK(c, c->vox_order.ensure(sizeof(int) * (size_t)N));
    HIPCHK(c, c->vox_sidx.ensure(sizeof(uint32_t) * (size_t)N));
    HIPCHK(c, c->vox_head.ensure(sizeof(int) * ((size_t)N + 1)));
    HIPCHK(c, c->vox_slot.ensure(sizeof(int) * ((size_t)N + 2)));
    launch_voxel_sort_multi(cat, N, m, n_buckets, sort_buffers(c), c->vox_order.as<int>(), c->vox_sidx.as<uint32_t>(),
                            c->vox_head.as<int>(), c->vox_slot.as<int>(), st);
    int vo[kVoxelMultiMax + 1];
    // the sorted sequence is cloud by cloud: cloud s starts at sorted position off[s]; its voxels start at slot[off[s]]
    HIPCHK(c, c->mp_cnt.ensure(sizeof(int) * (kVoxelMultiMax + 1)));
    launch_multi_bounds(c->vox_slot.as<int>(), m, c->mp_cnt.as<int>(), st);
    HIPCHK(c, hipMemcpyAsync(vo, c->mp_cnt.p, sizeof(int) * (size_t)(k + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const int n_vox = vo[k];
    for (int s = 0; s < k; ++s) {
        n_out[s] = vo[s + 1] - vo[s];
        if (n_out[s] > out_capacity[s]) return bad(c, "voxel_downsample_multi: out_capacity too small (see n_out)");
    }
    // ---- one centroid launch, the slices handed out ------------------------------------------------------------------------------
    HIPCHK(c, c->vox_start.ensure(sizeof(int) * ((size_t)n_vox + 2)));
    HIPCHK(c, c->vox_out.ensure(sizeof(float4) * (size_t)std::max(n_vox, 1)));
    launch_voxel_centroids(N, n_vox, cat, nullptr, fmt == LISREG_FMT_DEVICE ? 1 : 0, c->vox_order.as<int>(), c->vox_head.as<int>(),
                           c->vox_slot.as<int>(), c->vox_start.as<int>(), c->vox_out.as<float4>(), nullptr, st);
    HIPCHK(c, hipGetLastError());
    VoxelHandOut ho;
    memset(&ho, 0, sizeof ho);
    ho.k = k;
    for (int s = 0; s <= k; ++s) ho.vo[s] = vo[s];
    for (int s = 0; s < k; ++s) ho.out[s] = static_cast<float4*>(out[s]);
    launch_hand_out(c->vox_out.as<float4>(), ho, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));           // like the single-cloud call: the outputs are complete on return
    return LISREG_OK;
}

// pcl's `*cloud += *other` for device records: K clouds end to end into `out` (one launch on the context's stream, nothing waited for —
// every later call of this context is ordered behind it).  currentCloudInit's surf source = dynamic + building + ground (:866-889).
int lisreg_concat_device(lisreg_ctx* c, int k, const void* const* in, const int* n, void* out, int* n_out)
{
    if (!c) return LISREG_ERR_ARG;
    if (k < 0 || k > kVoxelMultiMax || (k > 0 && (!in || !n))) return bad(c, "concat_device: bad arguments (at most 8 clouds)");
    VoxelMulti m;
    BboxJobs jobs;
    memset(&m, 0, sizeof m); memset(&jobs, 0, sizeof jobs);
    m.k = jobs.k = k;
    long long total = 0;
    for (int s = 0; s < k; ++s) {
        if (n[s] < 0 || (n[s] > 0 && !in[s])) return bad(c, "concat_device: NULL cloud with n > 0");
        m.off[s] = (int)total; jobs.pts[s] = static_cast<const float4*>(in[s]); jobs.n[s] = n[s];
        total += n[s];
    }
    if (total > 2000000000LL || (total > 0 && !out)) return bad(c, "concat_device: bad output");
    m.off[k] = (int)total;
    if (n_out) *n_out = (int)total;
    HIPCHK(c, hipSetDevice(c->device));
    launch_concat_jobs(jobs, m, static_cast<float4*>(out), c->stream);
    HIPCHK(c, hipGetLastError());
    return LISREG_OK;
}

int lisreg_transform_cloud(lisreg_ctx* c, const void* in, int n, int stride, int fmt, const float T[6], void* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!T || (n > 0 && !out)) return bad(c, "transform_cloud: bad arguments");
    // (only x, y, z are read: every fmt but LISREG_FMT_DEVICE is taken as host structs with the three floats in front)
    if (const int rc = check_cloud(c, "transform_cloud", in, n, stride, fmt == LISREG_FMT_DEVICE ? fmt : LISREG_FMT_XYZI,
                                   fmt_bit(LISREG_FMT_DEVICE) | fmt_bit(LISREG_FMT_XYZI), true)) return rc;
    if (n == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    float M[12];
    lisreg_pose_to_matrix(T, M);                      // pcl::getTransformation (common.cpp:140-142)
    if (fmt == LISREG_FMT_DEVICE) {                  // the matrix travels as a kernel argument
        launch_transform_cloud_m(static_cast<const float4*>(in), n, M, static_cast<float4*>(out), st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));
        return LISREG_OK;
    }
    HIPCHK(c, c->vox_M.ensure(sizeof M));
    HIPCHK(c, hipMemcpyAsync(c->vox_M.p, M, sizeof M, hipMemcpyHostToDevice, st));
    std::vector<float4> h((size_t)n);
    const unsigned char* b = static_cast<const unsigned char*>(in);
    for (int i = 0; i < n; ++i) { float v[3]; memcpy(v, b + (size_t)i * (size_t)stride, 12); h[(size_t)i] = make_float4(v[0], v[1], v[2], 0.f); }
    HIPCHK(c, c->vox_in.ensure(sizeof(float4) * (size_t)n));
    HIPCHK(c, hipMemcpyAsync(c->vox_in.p, h.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, st));
    launch_transform_cloud(c->vox_in.as<float4>(), n, c->vox_M.as<float>(), c->vox_in.as<float4>(), st);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->vox_in.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    unsigned char* o = static_cast<unsigned char*>(out);
    for (int i = 0; i < n; ++i) {
        if (o != b) memcpy(o + (size_t)i * (size_t)stride, b + (size_t)i * (size_t)stride, (size_t)stride);   // other fields copied
        memcpy(o + (size_t)i * (size_t)stride, &h[(size_t)i], 12);
    }
    return LISREG_OK;
}

}  // extern "C"
