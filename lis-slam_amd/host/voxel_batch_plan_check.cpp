// voxel_batch_plan_check.cpp — the device-free decisions of lisreg_voxel_downsample_batch (csrc/lisreg_voxel_batch_plan.hpp: argument
// validation, the overlap sweep, offsets, chunk table, bucket budget, launch and scratch sizes) against brute-force restatements on
// seeded random batches: the overlap verdict against all pairs, the tables against their defining properties.  The pointers are
// made-up addresses that nothing dereferences.  The generator aims at the edges named in kEdgeName and the program fails if one was
// never met.  Host code only: no HIP header, no HIP call, no library of the project.
// g++ -std=c++17 -Wall -Wextra -Werror -I../csrc voxel_batch_plan_check.cpp      (also with -fsanitize=address,undefined)
#include "lisreg_voxel_batch_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>

using namespace lisreg;

namespace {

enum Edge { kEmptyCloud, kChunkM1, kChunk, kChunkP1, kOneCloud, kMaxClouds, kTooManyClouds, kNegativeN, kLeafZero, kLeafNan, kBadFmt, kNullIn,
            kNullOut, kNullJobs, kNegativeCap, kTotal2e9, kOutMeetsOwnIn, kOutMeetsOtherIn, kOutMeetsOut, kInMeetsIn, kTouching, kCapBinds,
            kMinBuckets, kEdges };
const char* const kEdgeName[kEdges] = { "empty_cloud", "n_256k-1", "n_256k", "n_256k+1", "one_cloud", "1024_clouds", "1025_clouds", "negative_n",
    "leaf_zero", "leaf_nan", "bad_fmt", "null_in", "null_out", "null_jobs", "negative_capacity", "total_above_2e9", "out_meets_own_in",
    "out_meets_other_in", "out_meets_out", "in_meets_in_allowed", "touching_ranges_allowed", "bucket_cap_binds", "min_buckets" };
long long hits[kEdges];

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    int pick(int n) { return (int)(next() % (uint64_t)n); }
    int range(int lo, int hi) { return lo + pick(hi - lo + 1); }
};

void* addr(uintptr_t a) { return reinterpret_cast<void*>(a); }

// all pairs: is there an `out` that meets an `in` (its own included) or another job's `out`?  bad[s]: job s's out is in such a conflict
bool brute_overlap(const std::vector<lisreg_voxel_job>& j, std::vector<char>& bad)
{
    bool any = false;
    bad.assign(j.size(), 0);
    for (size_t a = 0; a < j.size(); ++a) {
        const uintptr_t oa = (uintptr_t)j[a].out;
        const size_t na = (size_t)j[a].out_capacity * 16;
        for (size_t b = 0; b < j.size(); ++b) {
            if (vb_ranges_meet(oa, na, (uintptr_t)j[b].in, (size_t)j[b].n * 16)) { bad[a] = 1; any = true; }
            if (a != b && vb_ranges_meet(oa, na, (uintptr_t)j[b].out, (size_t)j[b].out_capacity * 16)) { bad[a] = bad[b] = 1; any = true; }
        }
    }
    return any;
}

// a batch of disjoint clouds laid out one after the other from `base`
std::vector<lisreg_voxel_job> disjoint_batch(Rng& r, int k, int max_n, uintptr_t base = 0x10000000)
{
    std::vector<lisreg_voxel_job> j((size_t)k);
    uintptr_t at = base;
    for (int s = 0; s < k; ++s) {
        int n = r.pick(8) == 0 ? 0 : r.range(1, max_n);
        const int q = r.pick(12);
        if (q < 3 && max_n >= 1024) { n = 256 * r.range(1, 3) + (q - 1); ++hits[q == 0 ? kChunkM1 : q == 1 ? kChunk : kChunkP1]; }
        if (n == 0) ++hits[kEmptyCloud];
        const int cap = n + r.pick(3);
        j[(size_t)s] = lisreg_voxel_job{ addr(at), n, 0.05f + 0.1f * (float)r.pick(20), addr(at + (size_t)n * 16), cap, -7, -7 };
        at += ((size_t)n + (size_t)cap) * 16 + (r.pick(2) ? 0 : 16 * (size_t)r.pick(5));
    }
    return j;
}

bool expect_refused(const std::vector<lisreg_voxel_job>& j, int n_clouds, int fmt, const char* word, const char* what)
{
    std::string why;
    if (vb_validate(n_clouds, j.empty() ? nullptr : j.data(), fmt, &why)) { printf("%s was not refused\n", what); return false; }
    if (why.find(word) == std::string::npos) { printf("%s: the text \"%s\" lacks \"%s\"\n", what, why.c_str(), word); return false; }
    return true;
}

bool check_plan(const std::vector<lisreg_voxel_job>& j)
{
    const int k = (int)j.size();
    VbPlan P;
    vb_plan(k, j.data(), &P);
    long long off = 0, nb = 0, want_all = 0;
    size_t ch = 0;
    for (int s = 0; s < k; ++s) if (j[(size_t)s].n > 0) want_all += std::max<long long>(64, 8LL * j[(size_t)s].n);
    if (want_all > (1LL << 24)) ++hits[kCapBinds];
    for (int s = 0; s < k; ++s) {
        const VbCloud& c = P.clouds[(size_t)s];
        const lisreg_voxel_job& q = j[(size_t)s];
        if (c.in != q.in || c.out != q.out || c.n != q.n || c.cap != q.out_capacity || memcmp(&c.leaf, &q.leaf, 4) || c.off != off) return false;
        if (c.bucket_base != nb || (q.n > 0) != (c.n_buckets > 0)) return false;
        long long share = q.n > 0 ? std::max<long long>(64, 8LL * q.n) : 0;
        if (q.n > 0 && q.n <= 8) ++hits[kMinBuckets];
        if (want_all > (1LL << 24) && q.n > 0) share = std::max(1LL, share * (1LL << 24) / want_all);
        if (c.n_buckets != share) return false;
        if (c.chunk0 != (int)ch || c.n_chunks != (q.n + 255) / 256) return false;
        int covered = 0;
        for (int b = 0; b < c.n_chunks; ++b, ++ch) {
            if (ch >= P.chunks.size()) return false;
            const VbChunk& x = P.chunks[ch];
            if (x.cloud != s || x.start != covered || x.count < 1 || x.count > kVbChunk || (b + 1 < c.n_chunks && x.count != kVbChunk)) return false;
            covered += x.count;
        }
        if (covered != q.n) return false;
        off += q.n; nb += c.n_buckets;
    }
    if (ch != P.chunks.size() || P.n_points != off || P.n_buckets != nb || nb > (1LL << 24) + k) return false;
    const VbSizes z = vb_sizes(P);
    const size_t N = (size_t)off, B = (size_t)nb;
    // what the kernels index: hist [B], bucket_start [B + 1], the scans' tile sums, per-point arrays [N], head [N], slot [N + 1],
    // vstart [voxels + 1 <= N + 1], a box per chunk, a list entry per voxel of more than kVbVoteBig points (int2) behind 16 bytes
    if (z.hist < 4 * B || z.bucket_start < 4 * (B + 1) || z.scan_tmp < 4 * (std::max(B, N) / 2048 + 4) || z.per_point < 4 * N || z.head < 4 * N ||
        z.slot < 4 * (N + 1) || z.vstart < 4 * (N + 1) || z.part < 24 * P.chunks.size() || z.big < 16 + 8 * (N / 25 + 1) ||
        z.tab_upload != 48 * (size_t)k + 16 * P.chunks.size() || z.tab_state != 48 * (size_t)k || z.tab_result != 8 * (size_t)k) return false;
    if (vb_voxel_blocks((int)N) < 1 || vb_voxel_blocks((int)N) > kVbMaxVoxelBlocks || vb_big_blocks((int)N) < 1 || vb_big_blocks((int)N) > kVbMaxBigBlocks ||
        (long long)vb_big_capacity((int)N) * (kVbVoteBig + 1) < (long long)N) return false;
    return true;
}

}  // namespace

int main()
{
    Rng r{ 20240607 };
    std::string why;
    // ---- refusals ----------------------------------------------------------------------------------------------------------------------
    {
        std::vector<lisreg_voxel_job> j = disjoint_batch(r, 4, 1000);
        for (size_t s = 0; s < j.size(); ++s) if (j[s].n == 0) { j[s].n = j[s].out_capacity = 5; j[s].in = addr(0x7000000 + 0x1000 * s); j[s].out = addr(0x7800000 + 0x1000 * s); }
        if (!vb_validate(4, j.data(), LISREG_FMT_DEVICE, &why) || !vb_validate(4, j.data(), LISREG_FMT_DEVICE_XYZI, &why)) { printf("a good batch was refused: %s\n", why.c_str()); return 1; }
        if (!vb_validate(0, nullptr, LISREG_FMT_DEVICE, &why)) { printf("an empty batch was refused\n"); return 1; }
        auto g = j;
        bool ok = true;
        g[2].n = -1; ok = ok && expect_refused(g, 4, LISREG_FMT_DEVICE, "job 2", "n < 0"); ++hits[kNegativeN]; g = j;
        g[1].leaf = 0.f; ok = ok && expect_refused(g, 4, LISREG_FMT_DEVICE, "job 1", "leaf 0"); ++hits[kLeafZero]; g = j;
        g[3].leaf = __builtin_nanf(""); ok = ok && expect_refused(g, 4, LISREG_FMT_DEVICE, "job 3", "leaf NaN"); ++hits[kLeafNan]; g = j;
        g[0].in = nullptr; ok = ok && expect_refused(g, 4, LISREG_FMT_DEVICE, "job 0", "NULL in"); ++hits[kNullIn]; g = j;
        g[1].out = nullptr; ok = ok && expect_refused(g, 4, LISREG_FMT_DEVICE, "job 1", "NULL out"); ++hits[kNullOut]; g = j;
        g[2].out_capacity = -3; ok = ok && expect_refused(g, 4, LISREG_FMT_DEVICE, "job 2", "capacity < 0"); ++hits[kNegativeCap]; g = j;
        ok = ok && expect_refused(j, 4, LISREG_FMT_XYZI, "device records", "fmt XYZI") && expect_refused(j, 4, 77, "device records", "fmt 77"); ++hits[kBadFmt];
        ok = ok && expect_refused({}, 3, LISREG_FMT_DEVICE, "NULL", "NULL jobs"); ++hits[kNullJobs];
        ok = ok && expect_refused(j, -1, LISREG_FMT_DEVICE, "n_clouds", "n_clouds -1");
        std::vector<lisreg_voxel_job> many = disjoint_batch(r, 1025, 40);
        ok = ok && expect_refused(many, 1025, LISREG_FMT_DEVICE, "n_clouds", "1025 clouds"); ++hits[kTooManyClouds];
        if (!vb_validate(1024, many.data(), LISREG_FMT_DEVICE, &why)) { printf("1024 clouds were refused: %s\n", why.c_str()); return 1; }
        ++hits[kMaxClouds];
        if (!check_plan(std::vector<lisreg_voxel_job>(many.begin(), many.begin() + 1024))) { printf("the plan of 1024 clouds is wrong\n"); return 1; }
        // three clouds of 7e8 points each: every one passes, the total does not
        std::vector<lisreg_voxel_job> big(3);
        for (int s = 0; s < 3; ++s) big[(size_t)s] = lisreg_voxel_job{ addr(0x100000000ull + (uintptr_t)s * 0x1000000000ull), 700000000, 0.2f, addr(0x800000000ull + (uintptr_t)s * 0x1000000000ull), 10, 0, 0 };
        ok = ok && expect_refused(big, 3, LISREG_FMT_DEVICE, "2e9", "2.1e9 points"); ++hits[kTotal2e9];
        if (!vb_validate(2, big.data(), LISREG_FMT_DEVICE, &why) || !check_plan(std::vector<lisreg_voxel_job>(big.begin(), big.begin() + 2))) { printf("1.4e9 points: refused or planned wrongly\n"); return 1; }
        if (!ok) return 1;
    }
    // ---- the overlap sweep against all pairs ---------------------------------------------------------------------------------------------
    long long conflicts = 0, clean = 0;
    for (int t = 0; t < 4000; ++t) {
        const int k = t % 7 == 0 ? r.range(200, 1024) : r.range(1, 12);
        if (k == 1) ++hits[kOneCloud];
        std::vector<lisreg_voxel_job> j = disjoint_batch(r, k, 300);
        const int kind = r.pick(7);
        const int a = r.pick(k), b = r.pick(k);
        lisreg_voxel_job &A = j[(size_t)a], &B = j[(size_t)b];
        if (kind == 1 && A.n > 0) { A.out = addr((uintptr_t)A.in + 16 * (size_t)r.pick(A.n)); ++hits[kOutMeetsOwnIn]; }        // in place
        if (kind == 2 && a != b && B.n > 0 && A.out_capacity > 0) { A.out = addr((uintptr_t)B.in + 16 * (size_t)(B.n - 1)); ++hits[kOutMeetsOtherIn]; }
        if (kind == 3 && a != b && B.out_capacity > 0 && A.out_capacity > 0) { A.out = addr((uintptr_t)B.out + 16 * (size_t)r.pick(B.out_capacity)); ++hits[kOutMeetsOut]; }
        if (kind == 4 && a != b && B.n > 0) { A.in = B.in; A.n = std::min(A.n, B.n); ++hits[kInMeetsIn]; }                        // two jobs read one cloud: fine
        if (kind == 5 && B.n > 0) { A.out = addr((uintptr_t)0x90000000); B.in = addr((uintptr_t)0x90000000 + 16 * (size_t)A.out_capacity); B.out = addr((uintptr_t)0xA0000000); ++hits[kTouching]; }
        if (kind == 6 && a != b && A.out_capacity > 0 && B.out_capacity > 0) { B.out = A.out; ++hits[kOutMeetsOut]; }             // equal starts
        std::vector<char> bad;
        const bool any = brute_overlap(j, bad);
        int job = -1;
        const bool ok = vb_check_overlap(k, j.data(), &job);
        if (ok == any) { printf("batch %d (kind %d, %d clouds): sweep %d, all pairs %d\n", t, kind, k, (int)!ok, (int)any); return 1; }
        if (!ok && (job < 0 || job >= k || !bad[(size_t)job])) { printf("batch %d (kind %d): the sweep names job %d, whose out meets nothing\n", t, kind, job); return 1; }
        if (any) {
            ++conflicts;
            if (vb_validate(k, j.data(), LISREG_FMT_DEVICE, &why) || why.find("job " + std::to_string(job) + ":") == std::string::npos) { printf("batch %d: overlap not refused by name\n", t); return 1; }
        } else {
            ++clean;
            if (!vb_validate(k, j.data(), LISREG_FMT_DEVICE_XYZI, &why)) { printf("batch %d refused: %s\n", t, why.c_str()); return 1; }
            if (!check_plan(j)) { printf("batch %d: the plan is wrong\n", t); return 1; }
        }
    }
    // ---- plans of big batches: the bucket cap binds ---------------------------------------------------------------------------------------
    for (int t = 0; t < 40; ++t) {
        std::vector<lisreg_voxel_job> j = disjoint_batch(r, r.range(1, 300), t % 2 ? 200000 : 3000000, 0x100000000ull);
        if (!vb_validate((int)j.size(), j.data(), LISREG_FMT_DEVICE, &why)) {
            if (why.find("2e9") == std::string::npos) { printf("big batch %d refused: %s\n", t, why.c_str()); return 1; }
            continue;
        }
        if (!check_plan(j)) { printf("big batch %d: the plan is wrong\n", t); return 1; }
    }
    printf("overlap batches: %lld in conflict, %lld clean; hits", conflicts, clean);
    bool all = true;
    for (int k = 0; k < kEdges; ++k) { printf(" %s=%lld", kEdgeName[k], hits[k]); all = all && hits[k] > 0; }
    if (!all) { printf("\nan edge was never met\n"); return 1; }
    printf("\nvoxel_batch_plan_check ok\n");
    return 0;
}
