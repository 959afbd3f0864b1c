// lisreg_api_motion.hip — host side of lisreg_adjust_cloud / lisreg_adjust_cloud_batch: the constant-velocity motion compensation of
// DistortionAdjust (src/core/distortionAdjust.cpp:412-480).  Kernel: lisreg_motion.hip.  Host code only.
#include "lisreg_ctx.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace lisreg;

namespace {

// SetMotionInfo (:412-417): the rates are rounded to float once
void set_motion(AdjustJob& j, const lisreg_motion& m)
{
    j.scan_period = m.scan_period;
    for (int k = 0; k < 3; ++k) { j.vel[k] = (float)m.linear_velocity[k]; j.rate[k] = (float)m.angular_velocity[k]; }
    j.pad = 0;
}

// the output arguments of one device sweep of n points; on success *n_out = max(n - 1, 0)
int check_device_out(lisreg_ctx* c, const char* who, int n, const float* time_device, const lisreg_adjust_out& o)
{
    if (n > 0 && !time_device) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": device records need time_device");
    if (o.capacity < 0 || (o.capacity > 0 && (!o.cloud || !o.time_device))) return ctx_fail(c, LISREG_ERR_ARG, std::string(who) + ": output buffers missing");
    return LISREG_OK;
}

}  // namespace

extern "C" {

int lisreg_default_motion(lisreg_motion* m)
{
    if (!m) return LISREG_ERR_ARG;
    m->scan_period = 0.1f;                                              // distortionAdjust.cpp:246
    for (int k = 0; k < 3; ++k) m->linear_velocity[k] = m->angular_velocity[k] = 0.0;
    return LISREG_OK;
}

int lisreg_adjust_cloud(lisreg_ctx* c, const void* cloud, int n, int stride, int fmt, const float* time_device, const lisreg_motion* M,
                        lisreg_adjust_out* out)
{
    if (!c) return LISREG_ERR_ARG;
    if (!M || !out) return bad(c, "adjust_cloud: bad arguments");
    if (const int rc = check_cloud(c, "adjust_cloud", cloud, n, stride, fmt, fmt_bit(LISREG_FMT_XYZIRT) | fmt_bit(LISREG_FMT_DEVICE), true)) return rc;
    const bool dev = fmt == LISREG_FMT_DEVICE;
    if (!dev && stride < 28) return bad(c, "adjust_cloud: XYZIRT needs stride >= 28 (the time is read)");
    if (dev) { if (const int rc = check_device_out(c, "adjust_cloud", n, time_device, *out)) return rc; }
    else if (out->capacity < 0 || (out->capacity > 0 && !out->cloud)) return bad(c, "adjust_cloud: output buffers missing");
    const size_t rec = dev ? sizeof(lisreg_dpoint) : (size_t)stride, cap = (size_t)out->capacity;
    if (spans_overlap(cloud, (size_t)n * rec, out->cloud, cap * rec) ||
        (dev && (spans_overlap(cloud, (size_t)n * rec, out->time_device, cap * 4) || spans_overlap(time_device, (size_t)n * 4, out->cloud, cap * rec) ||
                 spans_overlap(time_device, (size_t)n * 4, out->time_device, cap * 4))))
        return bad(c, "adjust_cloud: the output overlaps the input");
    const int n_out = std::max(n - 1, 0);
    out->n = n_out;
    if (n_out > out->capacity) return bad(c, "adjust_cloud: the output buffer is too small (count written back)");
    if (n_out == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    AdjustJob j;
    set_motion(j, *M);
    j.n_out = n_out;
    if (dev) {
        j.src = static_cast<const float4*>(cloud); j.time = time_device;
        j.dst = static_cast<float4*>(out->cloud); j.dst_time = out->time_device;
        launch_adjust_cloud(j, nullptr, 1, adjust_blocks(&j, 1), st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(st));
        return LISREG_OK;
    }
    // host structs: x y z and the time go up, x y z come back; every record is copied whole on the host and its coordinates replaced
    std::vector<float4> h_pts((size_t)n);
    std::vector<float> h_time((size_t)n);
    const unsigned char* b = static_cast<const unsigned char*>(cloud);
    for (int i = 0; i < n; ++i) {
        const unsigned char* r = b + (size_t)i * (size_t)stride;
        float v[3];
        memcpy(v, r, 12); memcpy(&h_time[(size_t)i], r + 24, 4);
        h_pts[(size_t)i] = make_float4(v[0], v[1], v[2], 0.f);
    }
    HIPCHK(c, c->mo_in.ensure(sizeof(float4) * (size_t)n));
    HIPCHK(c, c->mo_time.ensure(sizeof(float) * (size_t)n));
    HIPCHK(c, c->mo_out.ensure(sizeof(float4) * (size_t)n_out));
    HIPCHK(c, hipMemcpyAsync(c->mo_in.p, h_pts.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice, st));
    HIPCHK(c, hipMemcpyAsync(c->mo_time.p, h_time.data(), sizeof(float) * (size_t)n, hipMemcpyHostToDevice, st));
    j.src = c->mo_in.as<float4>(); j.time = c->mo_time.as<float>(); j.dst = c->mo_out.as<float4>(); j.dst_time = nullptr;
    launch_adjust_cloud(j, nullptr, 1, adjust_blocks(&j, 1), st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(h_pts.data(), c->mo_out.p, sizeof(float4) * (size_t)n_out, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    unsigned char* o = static_cast<unsigned char*>(out->cloud);
    for (int i = 0; i < n_out; ++i) {
        memcpy(o + (size_t)i * (size_t)stride, b + (size_t)(i + 1) * (size_t)stride, (size_t)stride);
        memcpy(o + (size_t)i * (size_t)stride, &h_pts[(size_t)i], 12);
    }
    return LISREG_OK;
}

int lisreg_adjust_cloud_batch(lisreg_ctx* c, int n_sweeps, const void* const* sweeps, const int* n, const float* const* time_device,
                              const lisreg_motion* motions, lisreg_adjust_out* outs)
{
    if (!c) return LISREG_ERR_ARG;
    if (n_sweeps < 0 || n_sweeps > 256 || (n_sweeps > 0 && (!sweeps || !n || !time_device || !motions || !outs)))
        return bad(c, "adjust_cloud_batch: bad arguments (at most 256 sweeps)");
    if (n_sweeps == 0) return LISREG_OK;
    std::vector<AdjustJob> jobs((size_t)n_sweeps);
    long long total = 0;
    for (int s = 0; s < n_sweeps; ++s) {
        if (const int rc = check_cloud(c, "adjust_cloud_batch", sweeps[s], n[s], 16, LISREG_FMT_DEVICE, fmt_bit(LISREG_FMT_DEVICE), true)) return rc;
        if (const int rc = check_device_out(c, "adjust_cloud_batch", n[s], time_device[s], outs[s])) return rc;
        if ((total += n[s]) > 1000000000LL) return bad(c, "adjust_cloud_batch: too many points");
    }
    for (int s = 0; s < n_sweeps; ++s)                                  // no output of the call may lie over an input of the call
        for (int t = 0; t < n_sweeps; ++t) {
            const size_t in_bytes = (size_t)n[t] * 16, t_bytes = (size_t)n[t] * 4, cap = (size_t)outs[s].capacity;
            if (spans_overlap(sweeps[t], in_bytes, outs[s].cloud, cap * 16) || spans_overlap(sweeps[t], in_bytes, outs[s].time_device, cap * 4) ||
                spans_overlap(time_device[t], t_bytes, outs[s].cloud, cap * 16) || spans_overlap(time_device[t], t_bytes, outs[s].time_device, cap * 4))
                return bad(c, "adjust_cloud_batch: an output overlaps an input");
        }
    bool small = false;
    for (int s = 0; s < n_sweeps; ++s) {
        AdjustJob& j = jobs[(size_t)s];
        set_motion(j, motions[s]);
        j.src = static_cast<const float4*>(sweeps[s]); j.time = time_device[s];
        j.dst = static_cast<float4*>(outs[s].cloud); j.dst_time = outs[s].time_device;
        j.n_out = std::max(n[s] - 1, 0);
        outs[s].n = j.n_out;
        if (j.n_out > outs[s].capacity) small = true;
    }
    if (small) return bad(c, "adjust_cloud_batch: an output buffer is too small (counts written back; nothing was written)");
    const int blocks = adjust_blocks(jobs.data(), n_sweeps);
    if (blocks == 0) return LISREG_OK;
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    HIPCHK(c, c->mo_tab.ensure(sizeof(AdjustJob) * (size_t)n_sweeps));
    HIPCHK(c, hipMemcpyAsync(c->mo_tab.p, jobs.data(), sizeof(AdjustJob) * (size_t)n_sweeps, hipMemcpyHostToDevice, st));
    launch_adjust_cloud(jobs[0], c->mo_tab.as<AdjustJob>(), n_sweeps, blocks, st);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(st));                               // `jobs` is a local
    return LISREG_OK;
}

}  // extern "C"
