// lisreg_api_features.hip — host side of the C-ABI entry points of SURVEY.md §8 f-2: range-image projection + feature extraction (one sweep,
// with IMU de-skew, or a batch of sweeps with a de-skew per sweep) and the semantic split.  Kernels: lisreg_features.hip.  Host code only.
#include "lisreg_ctx.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace lisreg;

extern "C" {

// ---- §8 f-2: range-image projection + feature extraction ----------------------------------------------------------------
int lisreg_default_feature_params(lisreg_feature_params* p)
{
    if (!p) return LISREG_ERR_ARG;
    p->n_scan = 64; p->horizon_scan = 1800; p->downsample_rate = 2;        // config/params.yaml:68-72
    p->min_range = 0.0f; p->max_range = 70.0f;                            // :73-74
    p->edge_threshold = 1.0f; p->surf_threshold = 0.1f;                   // :117-118
    return LISREG_OK;
}

int lisreg_extract_features(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, const lisreg_feature_params* P,
                            lisreg_feature_out* out)
{
    return lisreg_extract_features_deskew(c, cloud, n, stride, fmt, P, nullptr, out);
}

int lisreg_extract_features_deskew(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, const lisreg_feature_params* P,
                                   const lisreg_deskew* dk, lisreg_feature_out* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!P || !out) return bad(c, "extract_features: bad arguments");
    if (const int rc = check_cloud(c, "extract_features", cloud, n, stride, fmt, fmt_bit(LISREG_FMT_XYZIRT) | fmt_bit(LISREG_FMT_DEVICE), true)) return rc;
    if (fmt == LISREG_FMT_XYZIRT && stride < 22) return bad(c, "extract_features: XYZIRT needs stride >= 22 (the ring)");
    const bool deskew = dk && dk->enabled && n > 0;
    if (deskew) {
        // imu_pointer_cur == 0 is a table of one entry: findRotation (:376-387) hands every point that entry's rotation, as the CPU
        // restatement does (the reference itself leaves imuAvailable false then, :263, which is the caller's `enabled`)
        if (dk->imu_pointer_cur < 0 || dk->imu_pointer_cur > (1 << 20) || !dk->imu_time || !dk->imu_rot_x || !dk->imu_rot_y || !dk->imu_rot_z)
            return bad(c, "extract_features: de-skew needs IMU tables with imu_pointer_cur >= 0");
        if (fmt == LISREG_FMT_DEVICE && !dk->time_device) return bad(c, "extract_features: de-skew of device records needs time_device");
        if (fmt == LISREG_FMT_XYZIRT && stride < 28) return bad(c, "extract_features: de-skew needs the time field (stride >= 28)");
    }
    if (P->n_scan < 1 || P->n_scan > 1024 || P->horizon_scan < 16 || P->horizon_scan > 4096 || P->downsample_rate < 1)
        return bad(c, "extract_features: n_scan in [1,1024], horizon_scan in [16,4096], downsample_rate >= 1");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool dev = fmt == LISREG_FMT_DEVICE;
    const int H = P->n_scan, W = P->horizon_scan, hw = H * W;
    const size_t L = (size_t)hw + 16;
    HIPCHK(c, c->ft_owner.ensure(sizeof(int) * (size_t)hw));      HIPCHK(c, c->ft_flag.ensure(sizeof(int) * L));
    HIPCHK(c, c->ft_pos.ensure(sizeof(int) * 2 * (L + 1)));       HIPCHK(c, c->ft_scan.ensure(sizeof(int) * (L / 2048 + 8)));
    HIPCHK(c, c->ft_col.ensure(sizeof(int) * L));                 HIPCHK(c, c->ft_range.ensure(sizeof(float) * L));
    HIPCHK(c, c->ft_src.ensure(sizeof(int) * L));                 HIPCHK(c, c->ft_curv.ensure(sizeof(float) * L));
    HIPCHK(c, c->ft_picked.ensure(sizeof(int) * L));              HIPCHK(c, c->ft_label.ensure(sizeof(int) * L));
    HIPCHK(c, c->ft_rlists.ensure(sizeof(int) * (size_t)H * 3 * 128));
    HIPCHK(c, c->ft_rcounts.ensure(sizeof(int) * (size_t)H * 4)); HIPCHK(c, c->ft_lists.ensure(sizeof(int) * 4 * L));
    HIPCHK(c, c->ft_counts.ensure(sizeof(int) * 8));
    FeatureBuffers fb;
    fb.owner = c->ft_owner.as<int>(); fb.flag = c->ft_flag.as<int>(); fb.pos = c->ft_pos.as<int>(); fb.scan_tmp = c->ft_scan.as<int>();
    fb.col = c->ft_col.as<int>(); fb.range = c->ft_range.as<float>(); fb.src = c->ft_src.as<int>(); fb.curv = c->ft_curv.as<float>();
    fb.picked = c->ft_picked.as<int>(); fb.label = c->ft_label.as<int>(); fb.ring_lists = c->ft_rlists.as<int>();
    fb.ring_counts = c->ft_rcounts.as<int>(); fb.lists = c->ft_lists.as<int>(); fb.counts = c->ft_counts.as<int>();
    // ---- stage the sweep -----------------------------------------------------------------------------------------
    const float4* pts = nullptr;
    const uint32_t* rings = nullptr;
    std::vector<float4> h_pts;
    std::vector<uint32_t> h_rings;
    if (dev) pts = static_cast<const float4*>(cloud);
    else if (n > 0) {
        h_pts.resize((size_t)n); h_rings.resize((size_t)n);
        const unsigned char* b = static_cast<const unsigned char*>(cloud);
        for (int i = 0; i < n; ++i) {
            const unsigned char* r = b + (size_t)i * (size_t)stride;
            float v[3], it = 0.f; uint16_t ring;
            memcpy(v, r, 12); memcpy(&it, r + 16, 4); memcpy(&ring, r + 20, 2);
            h_pts[(size_t)i] = make_float4(v[0], v[1], v[2], it); h_rings[(size_t)i] = ring;
        }
        HIPCHK(c, c->vox_in.ensure(sizeof(float4) * (size_t)n));
        HIPCHK(c, c->ft_rings.ensure(sizeof(uint32_t) * (size_t)n));
        HIPCHK(c, hipMemcpyAsync(c->vox_in.p, h_pts.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->ft_rings.p, h_rings.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
        pts = c->vox_in.as<float4>(); rings = c->ft_rings.as<uint32_t>();
    }
    launch_extract_features(pts, rings, n, *P, fb, st);
    HIPCHK(c, hipGetLastError());
    // ---- IMU de-skew: only the coordinates handed back change (ranges, columns and the selection use the raw points) ----
    const float4* out_pts = pts;
    std::vector<float4> h_dsk;
    if (deskew) {
        const size_t m = (size_t)dk->imu_pointer_cur + 1;
        HIPCHK(c, c->ft_dsk_tab.ensure(sizeof(double) * 4 * m + 64));
        HIPCHK(c, c->ft_dsk_pts.ensure(sizeof(float4) * (size_t)n));
        HIPCHK(c, c->ft_dsk_misc.ensure(64));
        double* tab = c->ft_dsk_tab.as<double>();
        const double* srcs[4] = { dk->imu_time, dk->imu_rot_x, dk->imu_rot_y, dk->imu_rot_z };
        for (int k = 0; k < 4; ++k) HIPCHK(c, hipMemcpyAsync(tab + (size_t)k * m, srcs[k], sizeof(double) * m, hipMemcpyHostToDevice, st));
        const float* times_dev = dk->time_device;
        std::vector<float> h_time;
        if (!dev) {
            h_time.resize((size_t)n);
            const unsigned char* b = static_cast<const unsigned char*>(cloud);
            for (int i = 0; i < n; ++i) memcpy(&h_time[(size_t)i], b + (size_t)i * (size_t)stride + 24, 4);
            HIPCHK(c, c->ft_dsk_time.ensure(sizeof(float) * (size_t)n));
            HIPCHK(c, hipMemcpyAsync(c->ft_dsk_time.p, h_time.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st));
            times_dev = c->ft_dsk_time.as<float>();
        }
        HIPCHK(c, hipMemcpyAsync(c->ft_dsk_pts.p, pts, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, st));
        DeskewTables T{ tab, tab + m, tab + 2 * m, tab + 3 * m, dk->imu_pointer_cur, dk->time_scan_cur };
        launch_deskew(fb.owner, hw, times_dev, T, c->ft_dsk_misc.as<int>(), c->ft_dsk_misc.as<float>() + 4, c->ft_dsk_pts.as<float4>(), st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));               // h_time and the caller's tables are done with
        out_pts = c->ft_dsk_pts.as<float4>();
        if (!dev) {
            h_dsk.resize((size_t)n);
            HIPCHK(c, hipMemcpyAsync(h_dsk.data(), c->ft_dsk_pts.p, sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost, st));
        }
    }
    int counts[8];
    HIPCHK(c, hipMemcpyAsync(counts, fb.counts, sizeof counts, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // ---- hand the five clouds back in the caller's layout ------------------------------------------------------------
    struct Slot { void* buf; int cap; int* n; const int* idx; int cnt; };
    Slot slots[5] = { { out->deskewed, out->cap_deskewed, &out->n_deskewed, fb.src, counts[0] },
                      { out->corner, out->cap_corner, &out->n_corner, fb.lists + 0 * L, counts[1] },
                      { out->surface, out->cap_surface, &out->n_surface, fb.lists + 1 * L, counts[2] },
                      { out->corner_sharp, out->cap_corner_sharp, &out->n_corner_sharp, fb.lists + 2 * L, counts[3] },
                      { out->surface_sharp, out->cap_surface_sharp, &out->n_surface_sharp, fb.lists + 3 * L, counts[4] } };
    for (auto& sl : slots) *sl.n = sl.cnt;
    for (auto& sl : slots)
        if (sl.buf && sl.cnt > sl.cap) return bad(c, "extract_features: an output buffer is too small (counts written back)");
    std::vector<int> h_idx;
    for (auto& sl : slots) {
        if (!sl.buf || sl.cnt == 0) continue;
        if (dev) launch_gather_points(out_pts, sl.idx, sl.cnt, static_cast<float4*>(sl.buf), st);
        else {
            h_idx.resize((size_t)sl.cnt);
            HIPCHK(c, hipMemcpyAsync(h_idx.data(), sl.idx, sizeof(int) * (size_t)sl.cnt, hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            const unsigned char* b = static_cast<const unsigned char*>(cloud);
            unsigned char* o = static_cast<unsigned char*>(sl.buf);
            for (int i = 0; i < sl.cnt; ++i) {
                memcpy(o + (size_t)i * (size_t)stride, b + (size_t)h_idx[(size_t)i] * (size_t)stride, (size_t)stride);
                if (deskew) memcpy(o + (size_t)i * (size_t)stride, &h_dsk[(size_t)h_idx[(size_t)i]], 12);     // newPoint.x/y/z (:451-456)
            }
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

// S sweeps in one pass: the sweeps are stacked into ONE range image of S x H rows (grid of the selection kernel = sweeps x
// rings), every flat pass of the single-sweep pipeline runs once over the stack with per-sweep end guards, and one gather per
// output list hands every sweep its slice.  Device records in, device records out; the only host round trip is the (S + 1) x 5
// list boundaries the caller needs anyway.  Results are identical to S single calls (tests/test_features.py).
//
// deskews (NULL: none): the IMU de-skew of the enabled sweeps, between the extraction passes and the gathers — by then every pass has
// read the raw coordinates (ranges, columns and the selection use the raw points), so the library's concatenated copy is de-skewed in
// place.  Every sweep's tables and the per-sweep descriptors are packed on the host and cross the link in ONE copy; three launches
// (launch_deskew_batch) whatever n_sweeps is.  Without an enabled sweep nothing is added to the plain call.
static int extract_features_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const lisreg_feature_params* P,
                                  const lisreg_deskew* deskews, lisreg_feature_out* outs)
{
    if (n_sweeps < 0 || (n_sweeps > 0 && (!sweeps || !n || !outs)) || !P) return bad(c, "extract_features_batch: bad arguments");
    if (n_sweeps == 0) return LISREG_OK;
    if (P->n_scan < 1 || P->n_scan > 1024 || P->horizon_scan < 16 || P->horizon_scan > 4096 || P->downsample_rate < 1)
        return bad(c, "extract_features_batch: n_scan in [1,1024], horizon_scan in [16,4096], downsample_rate >= 1");
    if (n_sweeps > 256 || (long long)n_sweeps * P->n_scan > 32768) return bad(c, "extract_features_batch: at most 256 sweeps and 32768 rows per call");
    std::vector<int> off((size_t)n_sweeps + 1, 0);
    for (int s = 0; s < n_sweeps; ++s) {
        if (n[s] < 0 || (n[s] > 0 && !sweeps[s])) return bad(c, "extract_features_batch: NULL sweep with n > 0");
        if ((long long)off[(size_t)s] + n[s] > 2000000000LL) return bad(c, "extract_features_batch: too many points");
        off[(size_t)s + 1] = off[(size_t)s] + n[s];
    }
    const int N = off[(size_t)n_sweeps];
    // ---- the de-skew arguments, by the single call's rules per sweep; packed: [n_sweeps] descriptors, then every enabled sweep's tables ----
    std::vector<DeskewSweep> dsk;
    std::vector<double> dsk_tab;
    bool any_deskew = false;
    if (deskews) {
        dsk.assign((size_t)n_sweeps, DeskewSweep{ nullptr, 0.0, 0, 0, 0, 0 });
        for (int s = 0; s < n_sweeps; ++s) {
            const lisreg_deskew& dk = deskews[s];
            if (!dk.enabled || n[s] == 0) continue;
            if (dk.imu_pointer_cur < 0 || dk.imu_pointer_cur > (1 << 20) || !dk.imu_time || !dk.imu_rot_x || !dk.imu_rot_y || !dk.imu_rot_z)
                return bad(c, "extract_features_batch: de-skew needs IMU tables with imu_pointer_cur >= 0");
            if (!dk.time_device) return bad(c, "extract_features_batch: de-skew of device records needs time_device");
        }
        for (int s = 0; s < n_sweeps; ++s) {
            const lisreg_deskew& dk = deskews[s];
            if (!dk.enabled || n[s] == 0) continue;
            const size_t m = (size_t)dk.imu_pointer_cur + 1;
            if (dsk_tab.size() + 4 * m > 0x7fffffffu) return bad(c, "extract_features_batch: the IMU tables of the call are too long");
            dsk[(size_t)s] = DeskewSweep{ dk.time_device, dk.time_scan_cur, (int)dsk_tab.size(), dk.imu_pointer_cur, off[(size_t)s], 1 };
            for (const double* src : { dk.imu_time, dk.imu_rot_x, dk.imu_rot_y, dk.imu_rot_z }) dsk_tab.insert(dsk_tab.end(), src, src + m);
            any_deskew = true;
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int Hs = P->n_scan, W = P->horizon_scan, H = Hs * n_sweeps, hw = H * W, hw_sweep = Hs * W;
    const size_t L = (size_t)hw + 16;
    HIPCHK(c, c->ft_owner.ensure(sizeof(int) * (size_t)hw));      HIPCHK(c, c->ft_flag.ensure(sizeof(int) * L));
    HIPCHK(c, c->ft_pos.ensure(sizeof(int) * 2 * (L + 1)));       HIPCHK(c, c->ft_scan.ensure(sizeof(int) * (L / 2048 + 8)));
    HIPCHK(c, c->ft_col.ensure(sizeof(int) * L));                 HIPCHK(c, c->ft_range.ensure(sizeof(float) * L));
    HIPCHK(c, c->ft_src.ensure(sizeof(int) * L));                 HIPCHK(c, c->ft_curv.ensure(sizeof(float) * L));
    HIPCHK(c, c->ft_picked.ensure(sizeof(int) * L));              HIPCHK(c, c->ft_label.ensure(sizeof(int) * L));
    HIPCHK(c, c->ft_rlists.ensure(sizeof(int) * (size_t)H * 3 * 128));
    HIPCHK(c, c->ft_rcounts.ensure(sizeof(int) * (size_t)H * 4)); HIPCHK(c, c->ft_lists.ensure(sizeof(int) * 4 * L));
    HIPCHK(c, c->ft_counts.ensure(sizeof(int) * 8));
    HIPCHK(c, c->ft_cat.ensure(sizeof(float4) * (size_t)std::max(N, 1)));
    HIPCHK(c, c->ft_rings.ensure(sizeof(uint32_t) * (size_t)std::max(N, 1)));
    // layout: (S + 1) x 5 list boundaries, then — at the next 16-byte boundary — the 5 x S gather jobs (16 bytes each)
    const size_t jobs_off = (sizeof(int) * 5 * ((size_t)n_sweeps + 1) + 15) & ~(size_t)15;
    HIPCHK(c, c->ft_bounds.ensure(jobs_off + 16 * 5 * (size_t)n_sweeps));
    FeatureBuffers fb;
    fb.owner = c->ft_owner.as<int>(); fb.flag = c->ft_flag.as<int>(); fb.pos = c->ft_pos.as<int>(); fb.scan_tmp = c->ft_scan.as<int>();
    fb.col = c->ft_col.as<int>(); fb.range = c->ft_range.as<float>(); fb.src = c->ft_src.as<int>(); fb.curv = c->ft_curv.as<float>();
    fb.picked = c->ft_picked.as<int>(); fb.label = c->ft_label.as<int>(); fb.ring_lists = c->ft_rlists.as<int>();
    fb.ring_counts = c->ft_rcounts.as<int>(); fb.lists = c->ft_lists.as<int>(); fb.counts = c->ft_counts.as<int>();
    float4* cat = c->ft_cat.as<float4>();
    for (int s = 0; s < n_sweeps; ++s)
        if (n[s] > 0) HIPCHK(c, hipMemcpyAsync(cat + off[(size_t)s], sweeps[s], sizeof(float4) * (size_t)n[s], hipMemcpyDeviceToDevice, st));
    launch_feature_batch_rows(cat, N, off.data(), n_sweeps, Hs, P->downsample_rate, c->ft_rings.as<uint32_t>(), st);
    lisreg_feature_params Pst = *P;
    Pst.n_scan = H; Pst.downsample_rate = 1;                    // rows are stack rows; the ring filter was applied by k_feat_batch_rows
    launch_extract_features(cat, c->ft_rings.as<uint32_t>(), N, Pst, fb, st, n_sweeps);
    int* Bdev = c->ft_bounds.as<int>();
    launch_feature_batch_bounds(n_sweeps, Hs, hw_sweep, fb, hw, Bdev, st);
    HIPCHK(c, hipGetLastError());
    std::vector<unsigned char> dsk_pack;                               // lives until the wait below
    if (any_deskew) {
        static_assert(sizeof(DeskewSweep) == 32, "descriptors of 32 bytes: the tables behind them stay 8-byte aligned");
        const size_t desc_bytes = sizeof(DeskewSweep) * (size_t)n_sweeps, tab_bytes = sizeof(double) * dsk_tab.size();
        dsk_pack.resize(desc_bytes + tab_bytes);
        memcpy(dsk_pack.data(), dsk.data(), desc_bytes);
        memcpy(dsk_pack.data() + desc_bytes, dsk_tab.data(), tab_bytes);
        HIPCHK(c, c->ft_dsk_tab.ensure(dsk_pack.size()));
        HIPCHK(c, c->ft_dsk_misc.ensure((sizeof(int) + 9 * sizeof(float)) * (size_t)n_sweeps + 64));
        HIPCHK(c, hipMemcpyAsync(c->ft_dsk_tab.p, dsk_pack.data(), dsk_pack.size(), hipMemcpyHostToDevice, st));
        const unsigned char* base = c->ft_dsk_tab.as<unsigned char>();
        launch_deskew_batch(fb.owner, hw_sweep, n_sweeps, reinterpret_cast<const DeskewSweep*>(base), reinterpret_cast<const double*>(base + desc_bytes),
                            c->ft_dsk_misc.as<int>(), c->ft_dsk_misc.as<float>() + n_sweeps, cat, st);
        HIPCHK(c, hipGetLastError());
    }
    std::vector<int> B(5 * ((size_t)n_sweeps + 1));
    HIPCHK(c, hipMemcpyAsync(B.data(), Bdev, sizeof(int) * B.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    // ---- per sweep: counts, capacity check, one gather job per list ---------------------------------------------------------
    struct Job { void* dst; int begin, count; };
    std::vector<Job> jobs(5 * (size_t)n_sweeps);
    int max_count[5] = { 0, 0, 0, 0, 0 };
    for (int s = 0; s < n_sweeps; ++s) {
        lisreg_feature_out& o = outs[s];
        // B columns: extracted, corner, corner_sharp, surface_sharp, surface
        const int cnt[5] = { B[(s + 1) * 5 + 0] - B[s * 5 + 0], B[(s + 1) * 5 + 1] - B[s * 5 + 1], B[(s + 1) * 5 + 4] - B[s * 5 + 4],
                             B[(s + 1) * 5 + 2] - B[s * 5 + 2], B[(s + 1) * 5 + 3] - B[s * 5 + 3] };      // deskewed, corner, surface, corner_sharp, surface_sharp
        const int beg[5] = { B[s * 5 + 0], B[s * 5 + 1], B[s * 5 + 4], B[s * 5 + 2], B[s * 5 + 3] };
        void* bufs[5] = { o.deskewed, o.corner, o.surface, o.corner_sharp, o.surface_sharp };
        const int caps[5] = { o.cap_deskewed, o.cap_corner, o.cap_surface, o.cap_corner_sharp, o.cap_surface_sharp };
        o.n_deskewed = cnt[0]; o.n_corner = cnt[1]; o.n_surface = cnt[2]; o.n_corner_sharp = cnt[3]; o.n_surface_sharp = cnt[4];
        for (int k = 0; k < 5; ++k) {
            if (bufs[k] && cnt[k] > caps[k]) return bad(c, "extract_features_batch: an output buffer is too small (counts written back)");
            jobs[(size_t)k * n_sweeps + s] = Job{ bufs[k], beg[k], bufs[k] ? cnt[k] : 0 };
            if (bufs[k]) max_count[k] = std::max(max_count[k], cnt[k]);
        }
    }
    static_assert(sizeof(Job) == 16, "gather job = one 16-byte slot");
    Job* jobs_dev = reinterpret_cast<Job*>(reinterpret_cast<unsigned char*>(Bdev) + jobs_off);     // hipMalloc'ed base is 256-byte aligned
    HIPCHK(c, hipMemcpyAsync(jobs_dev, jobs.data(), sizeof(Job) * jobs.size(), hipMemcpyHostToDevice, st));
    const int* idx[5] = { fb.src, fb.lists + 0 * L, fb.lists + 1 * L, fb.lists + 2 * L, fb.lists + 3 * L };
    for (int k = 0; k < 5; ++k)
        launch_feature_batch_gather(cat, idx[k], jobs_dev + (size_t)k * n_sweeps, n_sweeps, max_count[k], st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));           // `jobs` is a local
    return LISREG_OK;
}

int lisreg_extract_features_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const lisreg_feature_params* P,
                                  lisreg_feature_out* outs)
{
    if (!c) return LISREG_ERR_ARG;
    return extract_features_batch(c, n_sweeps, sweeps, n, P, nullptr, outs);
}

int lisreg_extract_features_deskew_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const lisreg_feature_params* P,
                                         const lisreg_deskew* deskews, lisreg_feature_out* outs)
{
    if (!c) return LISREG_ERR_ARG;
    return extract_features_batch(c, n_sweeps, sweeps, n, P, deskews, outs);
}

int lisreg_semantic_split(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, const uint32_t* using_label,
                          lisreg_semantic_out* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!out) return bad(c, "semantic_split: bad arguments");
    if (const int rc = check_cloud(c, "semantic_split", cloud, n, stride, fmt, fmt_bit(LISREG_FMT_XYZIL) | fmt_bit(LISREG_FMT_DEVICE), true)) return rc;
    static const uint32_t kUsingLabel[32] = { 0, 10, 10, 10, 10, 10, 10, 10, 10, 40, 40, 40, 70, 50, 50, 70, 81, 70, 81, 81 };   // label.yaml:177-196
    const uint32_t* map = using_label ? using_label : kUsingLabel;
    for (int k = 0; k < 5; ++k) out->n[k] = 0;
    if (n == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool dev = fmt == LISREG_FMT_DEVICE;
    const float4* pts = nullptr;
    const uint32_t* labels = nullptr;
    std::vector<float4> h_pts;
    std::vector<uint32_t> h_lab;
    if (dev) pts = static_cast<const float4*>(cloud);
    else {
        h_pts.resize((size_t)n); h_lab.resize((size_t)n);
        const unsigned char* b = static_cast<const unsigned char*>(cloud);
        for (int i = 0; i < n; ++i) {
            const unsigned char* r = b + (size_t)i * (size_t)stride;
            float v[3]; uint16_t l; memcpy(v, r, 12); memcpy(&l, r + 20, 2);
            h_pts[(size_t)i] = make_float4(v[0], v[1], v[2], 0.f); h_lab[(size_t)i] = l;
        }
        HIPCHK(c, c->vox_in.ensure(sizeof(float4) * (size_t)n));
        HIPCHK(c, c->vox_lab.ensure(sizeof(uint32_t) * (size_t)n));
        HIPCHK(c, hipMemcpyAsync(c->vox_in.p, h_pts.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(c, hipMemcpyAsync(c->vox_lab.p, h_lab.data(), sizeof(uint32_t) * (size_t)n, hipMemcpyHostToDevice, st));
        pts = c->vox_in.as<float4>(); labels = c->vox_lab.as<uint32_t>();
    }
    HIPCHK(c, c->vox_head.ensure(sizeof(int) * (5 * (size_t)n + 1)));
    HIPCHK(c, c->vox_slot.ensure(sizeof(int) * (5 * (size_t)n + 2)));
    HIPCHK(c, c->scan_tmp.ensure(sizeof(int) * (5 * (size_t)n / 2048 + 8)));
    HIPCHK(c, c->ft_lists.ensure(sizeof(int) * 5 * (size_t)n));
    HIPCHK(c, c->ft_counts.ensure(sizeof(int) * 8));
    launch_semantic_split(pts, labels, n, map, c->vox_head.as<int>(), c->vox_slot.as<int>(), c->scan_tmp.as<int>(),
                          c->ft_lists.as<int>(), c->ft_counts.as<int>(), st);
    HIPCHK(c, hipGetLastError());
    int counts[5];
    HIPCHK(c, hipMemcpyAsync(counts, c->ft_counts.p, sizeof counts, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int k = 0; k < 5; ++k) out->n[k] = counts[k];
    for (int k = 0; k < 5; ++k)
        if (out->cloud[k] && counts[k] > out->cap[k]) return bad(c, "semantic_split: an output buffer is too small (counts written back)");
    std::vector<int> h_idx;
    if (dev) {
        SemanticGather sg;
        for (int k = 0; k < 5; ++k) { sg.out[k] = static_cast<float4*>(out->cloud[k]); sg.count[k] = out->cloud[k] ? counts[k] : 0; }
        launch_semantic_gather(pts, c->ft_lists.as<int>(), n, sg, st);
    }
    for (int k = 0; k < 5; ++k) {
        if (dev || !out->cloud[k] || counts[k] == 0) continue;
        const int* idx = c->ft_lists.as<int>() + (size_t)k * n;
        {
            h_idx.resize((size_t)counts[k]);
            HIPCHK(c, hipMemcpyAsync(h_idx.data(), idx, sizeof(int) * (size_t)counts[k], hipMemcpyDeviceToHost, st));
            HIPCHK(c, hipStreamSynchronize(st));
            const unsigned char* b = static_cast<const unsigned char*>(cloud);
            unsigned char* o = static_cast<unsigned char*>(out->cloud[k]);
            for (int i = 0; i < counts[k]; ++i) memcpy(o + (size_t)i * (size_t)stride, b + (size_t)h_idx[(size_t)i] * (size_t)stride, (size_t)stride);
        }
    }
    HIPCHK(c, hipStreamSynchronize(st));
    return LISREG_OK;
}

}  // extern "C"
