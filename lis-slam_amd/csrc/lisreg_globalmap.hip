// lisreg_globalmap.hip — the global map of visualizeGlobalMapThread (src/node/subMapOptmizationNode.cpp:3553-3574
// publishGlobalMap, :3502-3514 the PCD export) assembled on the device from the resident submaps: walk the submaps in the caller's
// order, transformPointCloud each of the five class clouds by the submap's pose, concatenate.  The same gather with other class masks
// and poses is the loop-verification target (:2787-2790), the corrected current submap (:2906-2912) and laserCloudFromPre (:1151-1154).
//
// One launch whatever the number of submaps: a grid over 256-point tiles of the concatenated output.  A host-built table holds, per
// non-empty segment, the source pointer, the destination start, the count, the matrix index and the segment's first tile; tiles never
// straddle segments (the tile count is padded per segment, the output is not).  A workgroup finds its segment by a binary search over
// the first-tile column with blockIdx alone, so the search, the table entry and the 12 matrix floats live in scalar registers; per
// point there is one 16-byte load and one 16-byte store (two for PointXYZIL structs) and nothing else.  HBM-bound at 32 B per point.
// The search starts from a host-built hint — the entry of every 16th tile — because its dependent scalar loads are what a 256-point
// workgroup waits for before it can issue its one load: a dozen steps over a table of thousands of entries cost more than the copy.
// Built without FMA contraction (csrc/Makefile): the arithmetic is transform_record of lisreg_internal.hpp, the one k_transform_cloud runs.
// No CPU fallback: without a HIP device these fail with LISREG_ERR_HIP.
#include "lisreg_ctx.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

using namespace lisreg;

namespace {

constexpr int       kTile = 256;
constexpr int       kHintShift = 4;               // one search hint per 16 tiles
constexpr long long kDefaultChunk = 1 << 20;      // points per staged chunk of a host destination: 16 MB of records, 32 MB of structs

struct GatherSeg {                  // 32 bytes: two scalar 16-byte loads
    const float4* src;              // first record of this piece of a class cloud
    long long     dst;              // its place in the destination, in points
    unsigned      tile0;            // first tile of the piece (ascending over the table)
    int           count;
    int           mat;              // matrix index (12 floats each), -1: copy the bits
    int           pad_;
};
static_assert(sizeof(GatherSeg) == 32, "table entry layout");

template <bool kXyzil>
__global__ __launch_bounds__(kTile) void k_submap_gather(const GatherSeg* __restrict__ segs, const unsigned* __restrict__ hints,
                                                         const float* __restrict__ mats, void* __restrict__ out)
{
    const unsigned tile = blockIdx.x;
    // the last entry whose first tile is <= this tile lies between the entries of the two hinted tiles around it (block-uniform: scalar loads)
    int lo = (int)hints[tile >> kHintShift], hi = (int)hints[(tile >> kHintShift) + 1];
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[mid].tile0 <= tile) lo = mid; else hi = mid - 1;
    }
    const GatherSeg s = segs[__builtin_amdgcn_readfirstlane(lo)];
    const unsigned i = (tile - s.tile0) * (unsigned)kTile + threadIdx.x;
    if (i >= (unsigned)s.count) return;
    // the source pointer comes out of the table, so the compiler knows no address space for it: say "global" (a global_load, not a flat one)
    typedef float __attribute__((ext_vector_type(4))) vec4;
    const vec4 v = ((const __attribute__((address_space(1))) vec4*)s.src)[i];
    float4 p = make_float4(v.x, v.y, v.z, v.w);
    if (s.mat >= 0) p = transform_record(p, mats + 12 * s.mat);       // poses == NULL: no arithmetic, -0.0f stays -0.0f
    const long long o = s.dst + (long long)i;
    if (!kXyzil) {
        static_cast<float4*>(out)[o] = p;
    } else {                                      // PointXYZIL: x y z 0 | intensity 0, uint16 label at byte 20, 0, 0
        uint4* q = static_cast<uint4*>(out) + 2 * o;
        q[0] = make_uint4(__float_as_uint(p.x), __float_as_uint(p.y), __float_as_uint(p.z), 0u);
        q[1] = make_uint4(0u, __float_as_uint(p.w) & 0xffffu, 0u, 0u);
    }
}


// segment starts of the gather (n_maps * 5 + 1 entries); LISREG_ERR_NO_TARGET for an id that names no map
int plan_offsets(lisreg_ctx* c, const char* who, int n_maps, const int* map_ids, unsigned class_mask, std::vector<long long>& off)
{
    off.assign((size_t)n_maps * 5 + 1, 0);
    long long total = 0;
    for (int i = 0; i < n_maps; ++i) {
        const int id = map_ids[i];
        if (id < 0 || (size_t)id >= c->localmaps.size() || !c->localmaps[(size_t)id].valid)
            return ctx_fail(c, LISREG_ERR_NO_TARGET, std::string(who) + ": no such submap");
        const LocalMap& m = c->localmaps[(size_t)id];
        for (int k = 0; k < 5; ++k) {
            off[(size_t)i * 5 + k] = total;
            if (class_mask & (1u << k)) total += m.n[k];
        }
    }
    off[(size_t)n_maps * 5] = total;
    return LISREG_OK;
}

int check_list(lisreg_ctx* c, const char* who, int n_maps, const int* map_ids, unsigned class_mask)
{
    if (n_maps < 0 || (n_maps > 0 && !map_ids)) return bad(c, (std::string(who) + ": bad map list").c_str());
    if (class_mask & ~LISREG_CLS_ALL) return bad(c, (std::string(who) + ": class_mask has bits above 31").c_str());
    return LISREG_OK;
}

// The table of the points [c0, c1) of the concatenation, destinations counted from c0: one entry per non-empty piece of a segment.
// Returns the number of tiles (0: nothing to do).
long long append_pieces(lisreg_ctx* c, int n_maps, const int* map_ids, bool with_poses, const std::vector<long long>& off, long long c0,
                        long long c1, std::vector<GatherSeg>& tab)
{
    long long tiles = 0;
    // the first segment that ends behind c0
    size_t s = (size_t)(std::upper_bound(off.begin(), off.end(), c0) - off.begin()) - 1;
    for (; s < (size_t)n_maps * 5 && off[s] < c1; ++s) {
        const long long b = std::max(off[s], c0), e = std::min(off[s + 1], c1);
        if (e <= b) continue;
        const int i = (int)(s / 5), k = (int)(s % 5);
        GatherSeg g;
        g.src = c->localmaps[(size_t)map_ids[i]].cls[k].as<float4>() + (b - off[s]);
        g.dst = b - c0;
        g.tile0 = (unsigned)tiles;
        g.count = (int)(e - b);
        g.mat = with_poses ? i : -1;
        g.pad_ = 0;
        tab.push_back(g);
        tiles += (e - b + kTile - 1) / kTile;
    }
    return tiles;
}

// The search hints of the entries tab[first ..) (a table of their own, entry numbers counted from `first`) whose tiles are [0, tiles):
// hint[j] = the entry tile 16 j lies in, one more hint than the last tile needs, tiles past the end = the last entry.
void append_hints(const std::vector<GatherSeg>& tab, size_t first, long long tiles, std::vector<unsigned>& hints)
{
    const long long n_hints = tiles > 0 ? ((tiles - 1) >> kHintShift) + 2 : 0;
    size_t e = first;
    for (long long j = 0; j < n_hints; ++j) {
        while (e + 1 < tab.size() && (long long)tab[e + 1].tile0 <= (j << kHintShift)) ++e;
        hints.push_back((unsigned)(e - first));
    }
}

// table, hints and matrices into one of the two pinned slots, one upload on the context's stream; the device addresses come back
int upload_table(lisreg_ctx* c, const std::vector<GatherSeg>& tab, const std::vector<unsigned>& hints, int n_maps, const float* poses,
                 const GatherSeg** segs_dev, const unsigned** hints_dev, const float** mats_dev)
{
    const size_t tab_bytes = sizeof(GatherSeg) * tab.size(), hint_bytes = (sizeof(unsigned) * hints.size() + 15) & ~(size_t)15;
    const size_t mat_bytes = poses ? sizeof(float) * 12 * (size_t)n_maps : 0;
    const size_t bytes = tab_bytes + hint_bytes + mat_bytes;
    const int slot = c->gm_flip;
    c->gm_flip ^= 1;
    // the upload that last read this slot (two calls back) is through; only then may the slot be rewritten or reallocated
    if (c->gm_up[slot]) HIPCHK(c, hipEventSynchronize(c->gm_up[slot]));
    else HIPCHK(c, c->gm_up[slot].create(hipEventDisableTiming));
    HIPCHK(c, c->gm_host[slot].ensure(bytes, bytes + bytes / 2 + 4096));
    HIPCHK(c, c->gm_tab.ensure(bytes));          // (growing it frees the old table: hipFree waits for the kernels that read it)
    unsigned char* h = c->gm_host[slot].as<unsigned char>();
    memcpy(h, tab.data(), tab_bytes);
    memcpy(h + tab_bytes, hints.data(), sizeof(unsigned) * hints.size());
    float* M = reinterpret_cast<float*>(h + tab_bytes + hint_bytes);
    for (int i = 0; poses && i < n_maps; ++i) lisreg_pose_to_matrix(poses + 6 * (size_t)i, M + 12 * (size_t)i);
    HIPCHK(c, hipMemcpyAsync(c->gm_tab.p, h, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(c->gm_up[slot], c->stream));
    *segs_dev = c->gm_tab.as<GatherSeg>();
    *hints_dev = reinterpret_cast<const unsigned*>(c->gm_tab.as<unsigned char>() + tab_bytes);
    *mats_dev = reinterpret_cast<const float*>(c->gm_tab.as<unsigned char>() + tab_bytes + hint_bytes);
    return LISREG_OK;
}

void launch_gather(bool xyzil, const GatherSeg* segs, const unsigned* hints, const float* mats, void* out, long long tiles, hipStream_t st)
{
    if (xyzil) k_submap_gather<true><<<(unsigned)tiles, kTile, 0, st>>>(segs, hints, mats, out);
    else k_submap_gather<false><<<(unsigned)tiles, kTile, 0, st>>>(segs, hints, mats, out);
}

// device memory as the runtime knows it; anything it does not know is host memory
bool is_device_pointer(const void* p)
{
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

}  // namespace

extern "C" {

int lisreg_default_gather_params(lisreg_gather_params* p)
{
    if (!p) return LISREG_ERR_ARG;
    p->class_mask = LISREG_CLS_ALL;
    p->out_fmt = LISREG_FMT_DEVICE;
    p->chunk_points = 0;
    return LISREG_OK;
}

int lisreg_submap_gather_count(lisreg_ctx* c, int n_maps, const int* map_ids, unsigned class_mask, long long* n_total, long long* seg_offsets)
{
    if (!c) return LISREG_ERR_ARG;
    int rc = check_list(c, "submap_gather_count", n_maps, map_ids, class_mask);
    if (rc) return rc;
    if (!n_total) return bad(c, "submap_gather_count: NULL n_total");
    std::vector<long long> off;
    rc = plan_offsets(c, "submap_gather_count", n_maps, map_ids, class_mask, off);
    if (rc) return rc;
    *n_total = off.back();
    if (seg_offsets) memcpy(seg_offsets, off.data(), sizeof(long long) * off.size());
    return LISREG_OK;
}

int lisreg_submap_gather(lisreg_ctx* c, int n_maps, const int* map_ids, const float* poses, const lisreg_gather_params* P, void* out,
                         long long capacity_points, long long* n_out, long long* seg_offsets)
{
    if (!c) return LISREG_ERR_ARG;
    if (!P) return bad(c, "submap_gather: NULL params");
    int rc = check_list(c, "submap_gather", n_maps, map_ids, P->class_mask);
    if (rc) return rc;
    if (P->out_fmt != LISREG_FMT_DEVICE && P->out_fmt != LISREG_FMT_XYZIL) return bad(c, "submap_gather: out_fmt must be LISREG_FMT_DEVICE or LISREG_FMT_XYZIL");
    if (P->chunk_points < 0 || !n_out) return bad(c, "submap_gather: negative chunk_points / NULL n_out");
    std::vector<long long> off;
    rc = plan_offsets(c, "submap_gather", n_maps, map_ids, P->class_mask, off);
    if (rc) return rc;
    const long long total = off.back();
    *n_out = total;
    if (seg_offsets) memcpy(seg_offsets, off.data(), sizeof(long long) * off.size());
    if (total > capacity_points) return bad(c, "submap_gather: capacity too small (see *n_out)");
    if (total == 0) return LISREG_OK;
    if (!out) return bad(c, "submap_gather: NULL out");
    HIPCHK(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const bool xyzil = P->out_fmt == LISREG_FMT_XYZIL;
    const size_t rec = xyzil ? 32 : 16;
    std::vector<GatherSeg> tab;
    std::vector<unsigned> hints;
    const GatherSeg* segs_dev = nullptr;
    const unsigned* hints_dev = nullptr;
    const float* mats_dev = nullptr;

    if (is_device_pointer(out)) {                     // one upload, one launch, nothing waited for
        tab.reserve((size_t)n_maps * 5);
        const long long tiles = append_pieces(c, n_maps, map_ids, poses != nullptr, off, 0, total, tab);
        if (tiles > 0x7fffffffLL) return bad(c, "submap_gather: more than 2^31 tiles");
        append_hints(tab, 0, tiles, hints);
        rc = upload_table(c, tab, hints, n_maps, poses, &segs_dev, &hints_dev, &mats_dev);
        if (rc) return rc;
        launch_gather(xyzil, segs_dev, hints_dev, mats_dev, out, tiles, st);
        HIPCHK(c, hipGetLastError());
        return LISREG_OK;
    }

    // host destination: chunk j is gathered into buffer j & 1 on the context's stream and copied out on the copy stream while the kernel
    // of chunk j + 1 runs.  The copy stream carries copies and event records only (lisreg_stage_host_items says why), so the two
    // hand-overs — "the kernel has filled the buffer", "the copy has emptied it" — are waited for by the host.
    const long long chunk = P->chunk_points > 0 ? P->chunk_points : kDefaultChunk;
    const long long n_chunks = (total + chunk - 1) / chunk;
    std::vector<size_t> first((size_t)n_chunks, 0), first_hint((size_t)n_chunks, 0);      // every chunk has a table and hints of its own
    std::vector<long long> tiles((size_t)n_chunks, 0);
    for (long long j = 0; j < n_chunks; ++j) {
        first[(size_t)j] = tab.size(); first_hint[(size_t)j] = hints.size();
        tiles[(size_t)j] = append_pieces(c, n_maps, map_ids, poses != nullptr, off, j * chunk, std::min(total, (j + 1) * chunk), tab);
        append_hints(tab, first[(size_t)j], tiles[(size_t)j], hints);
    }
    if (!c->copy_stream) HIPCHK(c, c->copy_stream.create(hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b) {
        if (!c->gm_kernel[b]) HIPCHK(c, c->gm_kernel[b].create(hipEventDisableTiming));
        if (!c->gm_copied[b]) HIPCHK(c, c->gm_copied[b].create(hipEventDisableTiming));
        if (b < n_chunks) HIPCHK(c, c->gm_chunk[b].ensure((size_t)std::min(chunk, total) * rec));
    }
    rc = upload_table(c, tab, hints, n_maps, poses, &segs_dev, &hints_dev, &mats_dev);
    if (rc) return rc;
    unsigned char* dst = static_cast<unsigned char*>(out);
    auto copy_out = [&](long long j) -> int {         // chunk j: wait for its kernel, then the copy engine takes it
        const int b = (int)(j & 1);
        const long long n = std::min(total, (j + 1) * chunk) - j * chunk;
        HIPCHK(c, hipEventSynchronize(c->gm_kernel[b]));
        HIPCHK(c, hipMemcpyAsync(dst + (size_t)(j * chunk) * rec, c->gm_chunk[b].p, (size_t)n * rec, hipMemcpyDeviceToHost, c->copy_stream));
        HIPCHK(c, hipEventRecord(c->gm_copied[b], c->copy_stream));
        return LISREG_OK;
    };
    for (long long j = 0; j < n_chunks; ++j) {
        const int b = (int)(j & 1);
        if (j >= 2) HIPCHK(c, hipEventSynchronize(c->gm_copied[b]));            // chunk j - 2 has left this buffer
        launch_gather(xyzil, segs_dev + first[(size_t)j], hints_dev + first_hint[(size_t)j], mats_dev, c->gm_chunk[b].p, tiles[(size_t)j], st);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->gm_kernel[b], st));
        if (j >= 1) { rc = copy_out(j - 1); if (rc) return rc; }
    }
    rc = copy_out(n_chunks - 1);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    return LISREG_OK;
}

}  // extern "C"
