// semantic_batch_plan_check.cpp — the device-free decisions of lisreg_semantic_split_batch and lisreg_concat_device_batch
// (csrc/lisreg_semantic_batch_plan.hpp: argument validation, the overlap sweep, the class table, the frame and tile tables, the job
// table of the concat, launch and scratch sizes) against brute-force restatements on seeded random batches: the overlap verdict against
// all pairs, the tables against their defining properties.  The pointers are made-up addresses that nothing dereferences.  The
// generator aims at the edges named in kEdgeName and the program fails if one was never met.  Host code only: no HIP header, no HIP
// call, no library of the project.
// g++ -std=c++17 -Wall -Wextra -Werror -I../csrc semantic_batch_plan_check.cpp      (also with -fsanitize=address,undefined)
#include "lisreg_semantic_batch_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstring>

using namespace lisreg;

namespace {

enum Edge { kEmptyFrame, kTileM1, kTileExact, kTileP1, kOneFrame, kMaxFrames, kTooManyFrames, kNegativeN, kNullIn, kNullJobs, kNegativeCap,
            kTotal2e9, kOutMeetsOwnIn, kOutMeetsOtherIn, kOutMeetsOutSameJob, kOutMeetsOutOtherJob, kInMeetsIn, kTouching, kNullClass,
            kAllNullClasses, kCustomMap, kConcatK9, kConcatShortCap, kConcatOverlap, kConcatMaxJobs, kConcatTooManyJobs, kConcatEmptyMiddle, kEdges };
const char* const kEdgeName[kEdges] = { "empty_frame", "n_tile-1", "n_tile", "n_tile+1", "one_frame", "256_frames", "257_frames", "negative_n",
    "null_in", "null_jobs", "negative_cap", "total_above_2e9", "out_meets_own_in", "out_meets_other_in", "out_meets_out_same_job",
    "out_meets_out_other_job", "in_meets_in_allowed", "touching_ranges_allowed", "null_class", "all_classes_null", "custom_map",
    "concat_k_9", "concat_short_capacity", "concat_overlap", "concat_1024_jobs", "concat_1025_jobs", "concat_empty_middle" };
long long hits[kEdges];

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    int pick(int n) { return (int)(next() % (uint64_t)n); }
    int range(int lo, int hi) { return lo + pick(hi - lo + 1); }
};

void* addr(uintptr_t a) { return reinterpret_cast<void*>(a); }

// all pairs: is there an output that meets an input (its own job's included) or another output (of any job)?  bad[s]: job s has such an output
bool brute_overlap(const std::vector<lisreg_semantic_job>& j, std::vector<char>& bad)
{
    bool any = false;
    bad.assign(j.size(), 0);
    for (size_t a = 0; a < j.size(); ++a)
        for (int ka = 0; ka < 5; ++ka) {
            if (!j[a].out.cloud[ka]) continue;
            const uintptr_t oa = (uintptr_t)j[a].out.cloud[ka];
            const size_t na = (size_t)j[a].out.cap[ka] * 16;
            for (size_t b = 0; b < j.size(); ++b) {
                if (j[b].in && sb_ranges_meet(oa, na, (uintptr_t)j[b].in, (size_t)j[b].n * 16)) { bad[a] = 1; any = true; }
                for (int kb = 0; kb < 5; ++kb) {
                    if ((a == b && ka == kb) || !j[b].out.cloud[kb]) continue;
                    if (sb_ranges_meet(oa, na, (uintptr_t)j[b].out.cloud[kb], (size_t)j[b].out.cap[kb] * 16)) { bad[a] = bad[b] = 1; any = true; }
                }
            }
        }
    return any;
}

// a batch of disjoint frames laid out one after the other from `base`: the input, then the five class buffers
std::vector<lisreg_semantic_job> disjoint_batch(Rng& r, int k, int max_n, uintptr_t base = 0x10000000)
{
    std::vector<lisreg_semantic_job> j((size_t)k);
    uintptr_t at = base;
    for (int s = 0; s < k; ++s) {
        int n = r.pick(8) == 0 ? 0 : r.range(1, max_n);
        const int q = r.pick(12);
        if (q < 3 && max_n >= 4 * kSbTile) { n = kSbTile * r.range(1, 3) + (q - 1); ++hits[q == 0 ? kTileM1 : q == 1 ? kTileExact : kTileP1]; }
        if (n == 0) ++hits[kEmptyFrame];
        lisreg_semantic_job& f = j[(size_t)s];
        memset(&f, 0, sizeof f);
        f.in = n ? addr(at) : (r.pick(2) ? addr(at) : nullptr); f.n = n; f.status = -7;
        at += (size_t)n * 16 + (r.pick(2) ? 0 : 16 * (size_t)r.pick(5));
        const int nulls = r.pick(6) == 0 ? 5 : (r.pick(3) == 0 ? r.range(1, 4) : 0);
        int made_null = 0;
        for (int c = 0; c < 5; ++c) {
            f.out.n[c] = -7;
            if (made_null < nulls && (nulls == 5 || r.pick(2))) { f.out.cloud[c] = nullptr; f.out.cap[c] = r.pick(3) - 1; ++made_null; continue; }   // cap ignored, even < 0
            f.out.cap[c] = r.pick(4) == 0 ? 0 : n / (1 + r.pick(5)) + r.pick(3);
            f.out.cloud[c] = addr(at);
            at += (size_t)f.out.cap[c] * 16 + (r.pick(2) ? 0 : 16 * (size_t)r.pick(5));
            if (f.out.cap[c] == 0) at += 16;                                 // distinct addresses
        }
        if (made_null == 5) ++hits[kAllNullClasses]; else if (made_null) ++hits[kNullClass];
    }
    return j;
}

bool expect_refused(const std::vector<lisreg_semantic_job>& j, int n_frames, const char* word, const char* what)
{
    std::string why;
    if (sb_validate(n_frames, j.empty() ? nullptr : j.data(), &why)) { printf("%s was not refused\n", what); return false; }
    if (why.find(word) == std::string::npos) { printf("%s: the text \"%s\" lacks \"%s\"\n", what, why.c_str(), word); return false; }
    return true;
}

bool check_plan(const std::vector<lisreg_semantic_job>& j)
{
    const int k = (int)j.size();
    SbPlan P;
    sb_plan(k, j.data(), &P);
    long long total = 0;
    size_t at = 0;
    if ((int)P.frames.size() != k) return false;
    for (int s = 0; s < k; ++s) {
        const SbFrame& f = P.frames[(size_t)s];
        const lisreg_semantic_job& q = j[(size_t)s];
        if (f.in != q.in || f.n != q.n || f.tile0 != (int)at || f.n_tiles != (q.n + kSbTile - 1) / kSbTile) return false;
        for (int c = 0; c < 5; ++c)
            if (f.cloud[c] != q.out.cloud[c] || (q.out.cloud[c] && f.cap[c] != q.out.cap[c])) return false;
        int covered = 0;
        for (int b = 0; b < f.n_tiles; ++b, ++at) {
            if (at >= P.tiles.size()) return false;
            const SbTile& x = P.tiles[at];
            if (x.frame != s || x.start != covered || x.count < 1 || x.count > kSbTile || (b + 1 < f.n_tiles && x.count != kSbTile)) return false;
            covered += x.count;
        }
        if (covered != q.n) return false;
        total += q.n;
    }
    if (at != P.tiles.size() || P.n_points != total) return false;
    const SbSizes z = sb_sizes(P);
    // what the kernels index: a part row of kSbPartInts (>= 5) ints per tile, a result row of kSbResultInts (>= 6) ints per frame
    if (z.tab_upload != 80 * (size_t)k + 16 * P.tiles.size() || z.tab_part < 4 * 5 * P.tiles.size() || z.tab_part < 4 * (size_t)kSbPartInts * P.tiles.size() ||
        z.tab_result < 4 * 6 * (size_t)k || z.tab_result != 4 * (size_t)kSbResultInts * (size_t)k || z.tab_upload % 4 || z.tab_part % 4) return false;
    return true;
}

bool check_class_map(Rng& r)
{
    const uint32_t values[7] = { 10, 40, 50, 81, 0, 70, 11 };
    for (int t = 0; t < 200; ++t) {
        uint32_t m[32];
        for (int l = 0; l < 32; ++l) m[l] = t == 0 ? kSbDefaultUsingLabel[l] : (r.pick(10) == 0 ? (uint32_t)r.next() : values[r.pick(7)]);
        const SbClassMap c = sb_class_map(t == 0 ? nullptr : m);
        if (t) ++hits[kCustomMap];
        for (int q = 0; q < 400; ++q) {
            const uint32_t payload = q < 64 ? (uint32_t)q : (uint32_t)r.next();
            const uint32_t u = m[payload & 31u];
            const int want = u == 10 ? 0 : u == 40 ? 1 : u == 50 ? 2 : u == 81 ? 3 : 4;
            if (sb_class_lookup(c, payload) != want) return false;
        }
    }
    // label.yaml: 1 .. 8 dynamic, 9 .. 11 ground, 13 14 building, 16 18 19 pole, the rest (0, 12, 15, 17, 20 .. 31) outlier
    const SbClassMap d = sb_class_map(nullptr);
    const int want[32] = { 4, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 4, 2, 2, 4, 3, 4, 3, 3, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4 };
    for (uint32_t l = 0; l < 32; ++l) if (sb_class_lookup(d, l) != want[l] || sb_class_lookup(d, l + 0xFFFFFFE0u) != want[l]) return false;
    return true;
}

// ---- the concat ------------------------------------------------------------------------------------------------------------------
std::vector<lisreg_concat_job> concat_batch(Rng& r, int k, uintptr_t base = 0x40000000)
{
    std::vector<lisreg_concat_job> j((size_t)k);
    uintptr_t at = base;
    for (int s = 0; s < k; ++s) {
        lisreg_concat_job& q = j[(size_t)s];
        memset(&q, 0, sizeof q);
        q.k = r.range(0, 8); q.n_out = -7;
        int sum = 0;
        for (int i = 0; i < q.k; ++i) {
            q.n[i] = r.pick(3) == 0 ? 0 : r.range(1, 60);
            if (q.n[i] == 0 && i > 0 && i + 1 < q.k) ++hits[kConcatEmptyMiddle];
            q.in[i] = q.n[i] || r.pick(2) ? addr(at) : nullptr;
            at += 16 * (size_t)q.n[i]; sum += q.n[i];
        }
        q.out_capacity = sum + r.pick(3); q.out = addr(at);
        at += 16 * (size_t)q.out_capacity + 16;
    }
    return j;
}

bool concat_brute_overlap(const std::vector<lisreg_concat_job>& j)
{
    for (size_t a = 0; a < j.size(); ++a)
        for (size_t b = 0; b < j.size(); ++b) {
            for (int i = 0; i < j[b].k; ++i)
                if (j[b].in[i] && sb_ranges_meet((uintptr_t)j[a].out, 16 * (size_t)j[a].out_capacity, (uintptr_t)j[b].in[i], 16 * (size_t)j[b].n[i])) return true;
            if (a != b && sb_ranges_meet((uintptr_t)j[a].out, 16 * (size_t)j[a].out_capacity, (uintptr_t)j[b].out, 16 * (size_t)j[b].out_capacity)) return true;
        }
    return false;
}

bool check_concat_plan(const std::vector<lisreg_concat_job>& j)
{
    std::vector<CbJob> tab;
    int max_total = -1, want_max = 0;
    cb_plan((int)j.size(), j.data(), &tab, &max_total);
    if (tab.size() != j.size()) return false;
    for (size_t s = 0; s < j.size(); ++s) {
        int off = 0;
        for (int i = 0; i < 8; ++i) {
            if (tab[s].off[i] != off) return false;
            if (i < j[s].k) { if (tab[s].in[i] != j[s].in[i]) return false; off += j[s].n[i]; }
        }
        if (tab[s].off[8] != off || tab[s].k != j[s].k || tab[s].out != j[s].out || off > j[s].out_capacity) return false;
        want_max = std::max(want_max, off);
    }
    return max_total == want_max && cb_blocks_x(max_total) >= 1 && cb_blocks_x(max_total) <= kCbMaxBlocksX;
}

bool concat_refused(const std::vector<lisreg_concat_job>& j, int n_jobs, const char* word, const char* what)
{
    std::string why;
    if (cb_validate(n_jobs, j.empty() ? nullptr : j.data(), &why)) { printf("concat: %s was not refused\n", what); return false; }
    if (why.find(word) == std::string::npos) { printf("concat: %s: the text \"%s\" lacks \"%s\"\n", what, why.c_str(), word); return false; }
    return true;
}

}  // namespace

int main()
{
    Rng r{ 20261021 };
    std::string why;
    static_assert(sizeof(lisreg_semantic_job) == 104 && sizeof(SbFrame) == 80 && sizeof(SbTile) == 16 && sizeof(CbJob) == 112, "layouts");
    // ---- refusals ----------------------------------------------------------------------------------------------------------------------
    {
        std::vector<lisreg_semantic_job> j = disjoint_batch(r, 4, 3000);
        uintptr_t at = 0x7000000;
        for (auto& f : j) {                                                   // every frame live, every class present
            f.n = 100 + r.pick(50); f.in = addr(at); at += 16 * (size_t)f.n;
            for (int c = 0; c < 5; ++c) { f.out.cloud[c] = addr(at); f.out.cap[c] = f.n; at += 16 * (size_t)f.n; }
        }
        if (!sb_validate(4, j.data(), &why)) { printf("a good batch was refused: %s\n", why.c_str()); return 1; }
        if (!sb_validate(0, nullptr, &why) || !sb_validate(0, j.data(), &why)) { printf("an empty batch was refused\n"); return 1; }
        auto g = j;
        bool ok = true;
        g[2].n = -1; ok = ok && expect_refused(g, 4, "job 2", "n < 0"); ++hits[kNegativeN]; g = j;
        g[0].in = nullptr; ok = ok && expect_refused(g, 4, "job 0", "NULL in"); ++hits[kNullIn]; g = j;
        g[3].out.cap[4] = -3; ok = ok && expect_refused(g, 4, "job 3", "cap < 0"); ++hits[kNegativeCap]; g = j;
        g[3].out.cap[4] = -3; g[3].out.cloud[4] = nullptr;
        if (!sb_validate(4, g.data(), &why)) { printf("a negative cap of a NULL class was refused: %s\n", why.c_str()); return 1; }
        g = j;
        ok = ok && expect_refused({}, 3, "NULL", "NULL jobs"); ++hits[kNullJobs];
        ok = ok && expect_refused(j, -1, "n_frames", "n_frames -1");
        std::vector<lisreg_semantic_job> many = disjoint_batch(r, 257, 40);
        ok = ok && expect_refused(many, 257, "n_frames", "257 frames"); ++hits[kTooManyFrames];
        if (!sb_validate(256, many.data(), &why)) { printf("256 frames were refused: %s\n", why.c_str()); return 1; }
        ++hits[kMaxFrames];
        if (!check_plan(std::vector<lisreg_semantic_job>(many.begin(), many.begin() + 256))) { printf("the plan of 256 frames is wrong\n"); return 1; }
        // three frames of 7e8 points each: every one passes, the total does not
        std::vector<lisreg_semantic_job> big(3);
        for (int s = 0; s < 3; ++s) {
            memset(&big[(size_t)s], 0, sizeof big[0]);
            big[(size_t)s].in = addr(0x100000000ull + (uintptr_t)s * 0x1000000000ull); big[(size_t)s].n = 700000000;
            big[(size_t)s].out.cloud[1] = addr(0x800000000ull + (uintptr_t)s * 0x1000000000ull); big[(size_t)s].out.cap[1] = 10;
        }
        ok = ok && expect_refused(big, 3, "2e9", "2.1e9 points"); ++hits[kTotal2e9];
        if (!sb_validate(2, big.data(), &why) || !check_plan(std::vector<lisreg_semantic_job>(big.begin(), big.begin() + 2))) { printf("1.4e9 points: refused or planned wrongly\n"); return 1; }
        if (!ok) return 1;
    }
    if (!check_class_map(r)) { printf("the class table disagrees with the if-chain\n"); return 1; }
    // ---- the overlap sweep against all pairs ---------------------------------------------------------------------------------------------
    long long conflicts = 0, clean = 0;
    for (int t = 0; t < 4000; ++t) {
        const int k = t % 9 == 0 ? r.range(100, 256) : r.range(1, 10);
        if (k == 1) ++hits[kOneFrame];
        std::vector<lisreg_semantic_job> j = disjoint_batch(r, k, t % 5 == 0 ? 5 * kSbTile : 300);
        const int kind = r.pick(8);
        const int a = r.pick(k), b = r.pick(k), ca = r.pick(5), cb = r.pick(5);
        lisreg_semantic_job &A = j[(size_t)a], &B = j[(size_t)b];
        const bool a_out = A.out.cloud[ca] && A.out.cap[ca] > 0, b_out = B.out.cloud[cb] && B.out.cap[cb] > 0;
        if (kind == 1 && A.n > 0 && a_out) { A.out.cloud[ca] = addr((uintptr_t)A.in + 16 * (size_t)r.pick(A.n)); ++hits[kOutMeetsOwnIn]; }
        if (kind == 2 && a != b && B.n > 0 && a_out) { A.out.cloud[ca] = addr((uintptr_t)B.in + 16 * (size_t)(B.n - 1)); ++hits[kOutMeetsOtherIn]; }
        if (kind == 3 && a != b && a_out && b_out) { A.out.cloud[ca] = addr((uintptr_t)B.out.cloud[cb] + 16 * (size_t)r.pick(B.out.cap[cb])); ++hits[kOutMeetsOutOtherJob]; }
        if (kind == 4 && a != b && B.n > 0 && A.n > 0) { A.in = B.in; A.n = std::min(A.n, B.n); ++hits[kInMeetsIn]; }                 // two jobs split one cloud: fine
        if (kind == 5 && B.n > 0 && a_out && a != b) {                                                                              // out ends where an in begins
            A.out.cloud[ca] = addr((uintptr_t)0x90000000); B.in = addr((uintptr_t)0x90000000 + 16 * (size_t)A.out.cap[ca]); ++hits[kTouching];
        }
        if (kind == 6 && a_out) {                                                                                                   // two classes of one job
            const int other = (ca + 1 + r.pick(4)) % 5;
            if (A.out.cloud[other] && A.out.cap[other] > 0) { A.out.cloud[other] = addr((uintptr_t)A.out.cloud[ca] + 16 * (size_t)r.pick(A.out.cap[ca])); ++hits[kOutMeetsOutSameJob]; }
        }
        if (kind == 7 && a != b && a_out && b_out) { B.out.cloud[cb] = A.out.cloud[ca]; ++hits[kOutMeetsOutOtherJob]; }             // equal starts
        std::vector<char> bad;
        const bool any = brute_overlap(j, bad);
        int job = -1;
        const bool ok = sb_check_overlap(k, j.data(), &job);
        if (ok == any) { printf("batch %d (kind %d, %d frames): sweep %d, all pairs %d\n", t, kind, k, (int)!ok, (int)any); return 1; }
        if (!ok && (job < 0 || job >= k || !bad[(size_t)job])) { printf("batch %d (kind %d): the sweep names job %d, none of whose outputs meets anything\n", t, kind, job); return 1; }
        if (any) {
            ++conflicts;
            if (sb_validate(k, j.data(), &why) || why.find("job " + std::to_string(job) + ":") == std::string::npos) { printf("batch %d: overlap not refused by name\n", t); return 1; }
        } else {
            ++clean;
            if (!sb_validate(k, j.data(), &why)) { printf("batch %d refused: %s\n", t, why.c_str()); return 1; }
            if (!check_plan(j)) { printf("batch %d: the plan is wrong\n", t); return 1; }
        }
    }
    // ---- the concat: refusals, sweep, table ----------------------------------------------------------------------------------------------
    long long c_conflicts = 0, c_clean = 0;
    {
        std::vector<lisreg_concat_job> j = concat_batch(r, 5);
        for (auto& q : j) if (q.k < 2) { q.k = 2; q.n[0] = q.n[1] = 3; q.in[0] = q.in[1] = addr(0x3000000); q.out_capacity = 6; }
        if (!cb_validate(5, j.data(), &why) || !cb_validate(0, nullptr, &why)) { printf("a good concat batch was refused: %s\n", why.c_str()); return 1; }
        auto g = j;
        bool ok = true;
        g[1].k = 9; ok = ok && concat_refused(g, 5, "job 1", "k = 9"); ++hits[kConcatK9]; g = j;
        g[1].k = -1; ok = ok && concat_refused(g, 5, "job 1", "k = -1"); g = j;
        g[2].n[1] = -4; ok = ok && concat_refused(g, 5, "job 2", "n < 0"); g = j;
        g[3].in[0] = nullptr; g[3].n[0] = 3; ok = ok && concat_refused(g, 5, "job 3", "NULL input"); g = j;
        g[4].out_capacity = g[4].n[0] + g[4].n[1] - 1; g[4].k = 2; ok = ok && concat_refused(g, 5, "job 4", "short capacity"); ++hits[kConcatShortCap]; g = j;
        g[0].out = nullptr; ok = ok && concat_refused(g, 5, "job 0", "NULL out"); g = j;
        ok = ok && concat_refused({}, 2, "NULL", "NULL jobs") && concat_refused(j, -1, "n_jobs", "n_jobs -1");
        std::vector<lisreg_concat_job> many = concat_batch(r, 1025);
        ok = ok && concat_refused(many, 1025, "n_jobs", "1025 jobs"); ++hits[kConcatTooManyJobs];
        if (!cb_validate(1024, many.data(), &why) || !check_concat_plan(std::vector<lisreg_concat_job>(many.begin(), many.begin() + 1024))) { printf("1024 concat jobs: refused or planned wrongly\n"); return 1; }
        ++hits[kConcatMaxJobs];
        if (!ok) return 1;
    }
    for (int t = 0; t < 2000; ++t) {
        const int k = t % 11 == 0 ? r.range(100, 1024) : r.range(1, 8);
        std::vector<lisreg_concat_job> j = concat_batch(r, k);
        const int kind = r.pick(5), a = r.pick(k), b = r.pick(k);
        lisreg_concat_job &A = j[(size_t)a], &B = j[(size_t)b];
        if (kind == 1 && A.k > 0 && A.n[0] > 0) { A.out = addr((uintptr_t)A.in[0] + 16 * (size_t)(A.n[0] - 1)); ++hits[kConcatOverlap]; }      // onto its own input
        if (kind == 2 && a != b && A.out_capacity > 0 && B.out_capacity > 0) { A.out = addr((uintptr_t)B.out + 16 * (size_t)r.pick(B.out_capacity)); ++hits[kConcatOverlap]; }
        if (kind == 3 && a != b && B.k > 1 && B.n[1] > 0 && A.out_capacity > 0) { A.out = const_cast<void*>(B.in[1]); ++hits[kConcatOverlap]; }
        if (kind == 4 && a != b && A.k > 0 && B.k > 0) { A.in[0] = B.in[0]; A.n[0] = std::min(A.n[0], B.n[0]);                                   // shared input: fine
            int sum = 0; for (int i = 0; i < A.k; ++i) sum += A.n[i];
            A.out_capacity = std::max(A.out_capacity, sum); }
        const bool any = concat_brute_overlap(j);
        const bool ok = cb_validate(k, j.data(), &why);
        if (ok == any) { printf("concat batch %d (kind %d, %d jobs): validate %d, all pairs %d: %s\n", t, kind, k, (int)ok, (int)any, why.c_str()); return 1; }
        if (any) { ++c_conflicts; if (why.find("overlaps") == std::string::npos) { printf("concat batch %d: refused for another reason: %s\n", t, why.c_str()); return 1; } }
        else { ++c_clean; if (!check_concat_plan(j)) { printf("concat batch %d: the table is wrong\n", t); return 1; } }
    }
    printf("overlap batches: %lld in conflict, %lld clean; concat: %lld in conflict, %lld clean; hits", conflicts, clean, c_conflicts, c_clean);
    bool all = true;
    for (int k = 0; k < kEdges; ++k) { printf(" %s=%lld", kEdgeName[k], hits[k]); all = all && hits[k] > 0; }
    if (!all) { printf("\nan edge was never met\n"); return 1; }
    printf("\nsemantic_batch_plan_check ok\n");
    return 0;
}
