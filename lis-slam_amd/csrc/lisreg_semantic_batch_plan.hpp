// lisreg_semantic_batch_plan.hpp — the decisions of lisreg_semantic_split_batch and lisreg_concat_device_batch that need no device
// (lisreg_semantic_batch.hip): argument validation in the order include/lisreg.h names it, the overlap sweep, the label map folded into
// a class table, the frame and tile tables, the launch sizes and the scratch sizes.  Plain C++: no HIP header, no HIP call.  Everything
// here is a function of the jobs' n / pointers / capacities and the constants below — never of a count the device makes — so a call
// sizes its allocations and launches before the first kernel runs.  host/semantic_batch_plan_check.cpp compares these functions with
// brute-force restatements on random batches.
#pragma once
#include "../../include/lisreg.h"

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

namespace lisreg {

constexpr int       kSbThreads     = 256;                      // a workgroup of the count and scatter passes: four wavefronts
constexpr int       kSbRounds      = 4;                        // records a lane takes from its tile
constexpr int       kSbTile        = kSbThreads * kSbRounds;   // points of one tile: every tile belongs to one frame (the VbChunk pattern)
constexpr int       kSbRecordBytes = 16;                       // sizeof(lisreg_dpoint)
constexpr long long kSbMaxPoints   = 2000000000LL;
constexpr int       kSbPartInts    = 8;                        // ints a tile owns in the part table: its five counts, which become its five bases in place, + pad
constexpr int       kSbResultInts  = 8;                        // ints a frame owns in the result table: n[5], status, + pad
constexpr int       kCbMaxBlocksX  = 64;                       // workgroups that stride over one concat job (the k_feat_batch_gather shape)

// categoryMapping's classes (semanticFusionNode.cpp:173-189) in the order of lisreg_semantic_out.cloud
inline int sb_class_of(uint32_t using_label_value)
{
    return using_label_value == 10u ? 0 : (using_label_value == 40u ? 1 : (using_label_value == 50u ? 2 : (using_label_value == 81u ? 3 : 4)));
}
// config/label.yaml:177-196 (entries 20 .. 31 have none: outlier) — what lisreg_semantic_split takes for using_label == NULL
constexpr uint32_t kSbDefaultUsingLabel[32] = { 0, 10, 10, 10, 10, 10, 10, 10, 10, 40, 40, 40, 70, 50, 50, 70, 81, 70, 81, 81 };
// The map as the kernels take it, by value: the class of label l (= payload & 31) is nibble l, 16 nibbles a word — no table in memory
struct SbClassMap { uint64_t nib[2]; };
inline SbClassMap sb_class_map(const uint32_t* using_label /* [32] or NULL */)
{
    const uint32_t* m = using_label ? using_label : kSbDefaultUsingLabel;
    SbClassMap c{ { 0, 0 } };
    for (int l = 0; l < 32; ++l) c.nib[l >> 4] |= (uint64_t)sb_class_of(m[l]) << (4 * (l & 15));
    return c;
}
inline int sb_class_lookup(const SbClassMap& c, uint32_t payload)
{
    const uint32_t l = payload & 31u;
    return (int)((c.nib[l >> 4] >> (4 * (l & 15))) & 7u);
}

// One frame of the batch as the kernels read it (uploaded; 80 bytes)
struct SbFrame {
    const void* in;            // n records
    void*       cloud[5];      // cap[k] records each, or NULL: counted, not written
    int         cap[5];
    int         n;
    int         tile0;         // first tile
    int         n_tiles;
};
// One workgroup of the count and scatter passes
struct SbTile {
    int frame;
    int start;                 // first point of the tile, relative to the frame
    int count;                 // 1 .. kSbTile
    int pad_;
};
struct SbPlan {
    std::vector<SbFrame> frames;
    std::vector<SbTile>  tiles;
    long long n_points = 0;
};

// One concat job as the kernel reads it (uploaded; 112 bytes): source s lands at out[off[s] .. off[s + 1])
struct CbJob {
    const void* in[8];
    void*       out;
    int         off[9];
    int         k;
};

// do the byte ranges [a, a + na) and [b, b + nb) meet?  (an empty range meets nothing)
inline bool sb_ranges_meet(uintptr_t a, size_t na, uintptr_t b, size_t nb) { return na != 0 && nb != 0 && a < b + nb && b < a + na; }

// The overlap rule of both calls: no output range may meet any input range of the call or any other output range of the call (another
// class of the same job included).  Inputs may meet each other.  One sort and one sweep instead of all pairs.  false: *job names a
// job one of whose outputs is in conflict.
struct SbRange { uintptr_t lo, hi; int job; int is_out; };
inline bool sb_sweep(std::vector<SbRange>& r, int* job)
{
    std::sort(r.begin(), r.end(), [](const SbRange& a, const SbRange& b) {
        return a.lo != b.lo ? a.lo < b.lo : (a.job != b.job ? a.job < b.job : a.is_out < b.is_out); });
    // the furthest end among the ranges in front (all start at or before this one's start), of any kind and of the outputs alone
    uintptr_t end_any = 0, end_out = 0;
    int job_out = -1;
    for (const SbRange& x : r) {
        if (x.is_out && end_any > x.lo) { *job = x.job; return false; }
        if (!x.is_out && end_out > x.lo) { *job = job_out; return false; }
        end_any = std::max(end_any, x.hi);
        if (x.is_out && x.hi > end_out) { end_out = x.hi; job_out = x.job; }
    }
    return true;
}
inline void sb_push(std::vector<SbRange>& r, const void* p, long long records, int job, int is_out)
{
    if (p && records > 0) r.push_back({ (uintptr_t)p, (uintptr_t)p + (size_t)records * kSbRecordBytes, job, is_out });
}

inline bool sb_check_overlap(int n_frames, const lisreg_semantic_job* jobs, int* job)
{
    std::vector<SbRange> r;
    r.reserve(6 * (size_t)n_frames);
    for (int s = 0; s < n_frames; ++s) {
        sb_push(r, jobs[s].in, jobs[s].n, s, 0);
        for (int k = 0; k < 5; ++k) sb_push(r, jobs[s].out.cloud[k], jobs[s].out.cap[k], s, 1);
    }
    return sb_sweep(r, job);
}

// The argument checks of lisreg_semantic_split_batch, in the order the header names them.  true: the batch may run.  false: *why is
// the text for lisreg_last_error (it names the job where there is one).
inline bool sb_validate(int n_frames, const lisreg_semantic_job* jobs, std::string* why)
{
    const std::string who = "semantic_split_batch: ";
    if (n_frames < 0 || n_frames > LISREG_SEMANTIC_BATCH_MAX) { *why = who + "n_frames outside 0 .. " + std::to_string(LISREG_SEMANTIC_BATCH_MAX); return false; }
    if (n_frames > 0 && !jobs) { *why = who + "jobs is NULL"; return false; }
    long long total = 0;
    for (int s = 0; s < n_frames; ++s) {
        const lisreg_semantic_job& j = jobs[s];
        const auto at = [&] { return who + "job " + std::to_string(s) + ": "; };      // (made only for a job that fails)
        if (j.n < 0) { *why = at() + "n < 0"; return false; }
        if (j.n > 0 && !j.in) { *why = at() + "NULL in with n > 0"; return false; }
        for (int k = 0; k < 5; ++k)
            if (j.out.cloud[k] && j.out.cap[k] < 0) { *why = at() + "cap[" + std::to_string(k) + "] < 0"; return false; }
        total += j.n;
    }
    if (total > kSbMaxPoints) { *why = who + "more than 2e9 points in all"; return false; }
    int job = -1;
    if (!sb_check_overlap(n_frames, jobs, &job)) {
        *why = who + "job " + std::to_string(job) + ": an output range overlaps an input range or another output range of the call";
        return false;
    }
    return true;
}

// frame and tile tables of a validated batch
inline void sb_plan(int n_frames, const lisreg_semantic_job* jobs, SbPlan* P)
{
    P->frames.assign((size_t)n_frames, SbFrame{});
    P->tiles.clear();
    P->n_points = 0;
    for (int s = 0; s < n_frames; ++s) {
        const lisreg_semantic_job& j = jobs[s];
        SbFrame& f = P->frames[(size_t)s];
        f.in = j.in; f.n = j.n;
        for (int k = 0; k < 5; ++k) { f.cloud[k] = j.out.cloud[k]; f.cap[k] = j.out.cloud[k] ? j.out.cap[k] : 0; }
        f.tile0 = (int)P->tiles.size();
        f.n_tiles = (int)(((long long)j.n + kSbTile - 1) / kSbTile);
        for (int b = 0; b < f.n_tiles; ++b) P->tiles.push_back({ s, b * kSbTile, std::min(kSbTile, j.n - b * kSbTile), 0 });
        P->n_points += j.n;
    }
}

// bytes of the context's scratch a call uses: [frames | tiles] uploaded, then the tiles' part table and the result table the device writes
struct SbSizes { size_t tab_upload, tab_part, tab_result; };
inline SbSizes sb_sizes(const SbPlan& P)
{
    SbSizes z;
    z.tab_upload = sizeof(SbFrame) * P.frames.size() + sizeof(SbTile) * P.tiles.size();
    z.tab_part = sizeof(int) * kSbPartInts * std::max<size_t>(P.tiles.size(), 1);
    z.tab_result = sizeof(int) * kSbResultInts * P.frames.size();
    return z;
}

// ---- lisreg_concat_device_batch ------------------------------------------------------------------------------------------------
inline bool cb_validate(int n_jobs, const lisreg_concat_job* jobs, std::string* why)
{
    const std::string who = "concat_device_batch: ";
    if (n_jobs < 0 || n_jobs > LISREG_CONCAT_BATCH_MAX) { *why = who + "n_jobs outside 0 .. " + std::to_string(LISREG_CONCAT_BATCH_MAX); return false; }
    if (n_jobs > 0 && !jobs) { *why = who + "jobs is NULL"; return false; }
    std::vector<SbRange> r;
    for (int s = 0; s < n_jobs; ++s) {
        const lisreg_concat_job& j = jobs[s];
        const auto at = [&] { return who + "job " + std::to_string(s) + ": "; };
        if (j.k < 0 || j.k > 8) { *why = at() + "k outside 0 .. 8"; return false; }
        long long total = 0;
        for (int i = 0; i < j.k; ++i) {
            if (j.n[i] < 0) { *why = at() + "n < 0"; return false; }
            if (j.n[i] > 0 && !j.in[i]) { *why = at() + "NULL cloud with n > 0"; return false; }
            total += j.n[i];
            sb_push(r, j.in[i], j.n[i], s, 0);
        }
        if (j.out_capacity < 0 || total > j.out_capacity) { *why = at() + "out_capacity below the sum of the clouds"; return false; }
        if (total > 0 && !j.out) { *why = at() + "NULL out"; return false; }
        sb_push(r, j.out, j.out_capacity, s, 1);
    }
    int job = -1;
    if (!sb_sweep(r, &job)) {
        *why = who + "job " + std::to_string(job) + ": its out range overlaps an input range or another job's out range";
        return false;
    }
    return true;
}

// the job table of a validated batch; *max_total: the longest job (the launch's grid.x follows it)
inline void cb_plan(int n_jobs, const lisreg_concat_job* jobs, std::vector<CbJob>* tab, int* max_total)
{
    tab->assign((size_t)n_jobs, CbJob{});
    *max_total = 0;
    for (int s = 0; s < n_jobs; ++s) {
        const lisreg_concat_job& j = jobs[s];
        CbJob& t = (*tab)[(size_t)s];
        int off = 0;
        for (int i = 0; i < 8; ++i) {
            t.off[i] = off;
            if (i < j.k) { t.in[i] = j.in[i]; off += j.n[i]; }
        }
        t.off[8] = off; t.k = j.k; t.out = j.out;
        *max_total = std::max(*max_total, off);
    }
}
inline int cb_blocks_x(int max_total) { return std::max(1, std::min(kCbMaxBlocksX, (max_total + 255) / 256)); }

}  // namespace lisreg
