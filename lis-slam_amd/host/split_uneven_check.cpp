// split_uneven_check.cpp — plan_split_uneven (csrc/lisreg_batch_plan.hpp), the cut of a free-running interleaved run, on random item tables
// against brute force.  For every table and target share:
//   * the cut is an item boundary (or "no cut": both fields zero),
//   * neither part is under a quarter of the workgroups,
//   * it is what plan_split returns exactly when no boundary satisfies the quarter rule (which is then "no cut"),
//   * otherwise it is the qualifying boundary nearest to the share, the earlier of two equally near ones — found here by a plain search
//     over all boundaries in exact rational arithmetic.
// And split_form / plan_run_split, the decision whether a run is cut at all and in which form, against a table of its edges written out
// by hand (the floor of 16384 workgroups and the bound of 64 registrations of the library's own choice under "interleave" = 0 among them)
// and against a restatement over random arguments.
// The generator aims at the edges named in kEdgeName and the program fails if one was never met.  Host code only: no HIP call, no library
// of the project.
// g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I../csrc split_uneven_check.cpp
#include "lisreg_batch_plan.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>

using namespace lisreg;

namespace {

enum Edge { kNoBoundaryQualifies, kEvenCutAlsoNone, kUnevenWhereEvenIsNone, kSameAsEven, kDiffersFromEven, kTieTakesEarlier, kExactlyAQuarter,
            kEmptyItems, kTwoItems, kOneItem, kNoItems, kBigBatch, kAutoSplit, kAutoRefusedByItems, kAutoRefusedByFloor, kAutoRefusedByFreeIters, kAutoRefusedByOtherContext, kEdges };
const char* const kEdgeName[kEdges] = { "no_boundary_qualifies", "even_cut_also_none", "uneven_where_even_is_none", "same_as_even", "differs_from_even",
    "tie_takes_earlier", "exactly_a_quarter", "empty_items", "two_items", "one_item", "no_items", "big_batch", "auto_split", "auto_refused_by_items", "auto_refused_by_floor",
    "auto_refused_by_free_iters", "auto_refused_by_other_context" };
long long hits[kEdges];

struct Rng {
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
    int pick(int n) { return (int)(next() % (uint64_t)n); }
    int range(int lo, int hi) { return lo + pick(hi - lo + 1); }
};

bool quarter_ok(long long blk, long long n_blocks) { return blk * 4 >= n_blocks && (n_blocks - blk) * 4 >= n_blocks; }

// split_form's edges, written out: { n_blocks, n_items, lanes_q, fixed_iters, can_stop, exact, interleave, min_blocks, expected form }
struct FormCase { int n_blocks, n_items, lanes_q, fixed_iters; bool can_stop, exact; int interleave, min_blocks; bool alone; int form; };
const FormCase kFormCases[] = {
    // the library's own choice ("interleave" = 0): the floor, the registration bound, the fixed iteration count, no other context running batches
    { 16384, 64, 1, 10, false, false, 0, 8192, true, 2 }, { 16383, 64, 1, 10, false, false, 0, 8192, true, 0 }, { 1 << 30, 64, 1, 1, false, false, 0, 8192, true, 2 },
    { 16640, 65, 1, 10, false, false, 0, 8192, true, 0 }, { 57472, 128, 1, 10, false, false, 0, 8192, true, 0 }, { 115200, 256, 1, 10, false, false, 0, 8192, true, 0 },
    { 16384, 2, 1, 10, false, false, 0, 8192, true, 2 }, { 16384, 1, 1, 10, false, false, 0, 8192, true, 0 }, { 16384, 0, 1, 10, false, false, 0, 8192, true, 0 },
    { 28736, 64, 1, 0, false, false, 0, 8192, true, 0 }, { 28736, 64, 1, -1, false, false, 0, 8192, true, 0 }, { 28736, 64, 8, 10, false, false, 0, 8192, true, 0 },
    { 28736, 64, 1, 10, true, false, 0, 8192, true, 0 }, { 28736, 64, 1, 10, false, true, 0, 8192, true, 0 }, { 28736, 64, 1, 10, false, false, 0, 8192, false, 0 },
    { 28736, 64, 1, 10, false, false, 0, 8192, true, 2 },
    // "interleave_min_blocks": above the floor it takes the floor's place, below it the floor holds; past the batch it switches everything off
    { 28736, 64, 1, 10, false, false, 0, 28736, true, 2 }, { 28736, 64, 1, 10, false, false, 0, 28737, true, 0 }, { 28736, 64, 1, 10, false, false, 0, 1 << 30, true, 0 },
    { 16383, 64, 1, 10, false, false, 0, 4, true, 0 }, { 40, 3, 1, 5, false, false, 0, 4, true, 0 },
    { 28736, 64, 1, 10, false, false, 1, 28737, true, 0 }, { 28736, 64, 1, 10, false, false, 2, 28737, true, 0 },
    // the option set: any size from "interleave_min_blocks" up, any registration count from two, fixed iteration count or not, other contexts or not
    { 40, 3, 1, 5, false, false, 1, 4, true, 1 }, { 40, 3, 1, 5, false, false, 2, 4, true, 2 }, { 4, 2, 1, 0, false, false, 2, 4, true, 2 }, { 3, 2, 1, 5, false, false, 2, 4, true, 0 },
    { 115200, 256, 1, 10, false, false, 2, 8192, false, 2 }, { 115200, 256, 1, 10, false, false, 1, 8192, false, 1 }, { 40, 1, 1, 5, false, false, 2, 4, true, 0 },
    { 40, 3, 8, 5, false, false, 2, 4, true, 0 }, { 40, 3, 1, 5, true, false, 2, 4, true, 0 }, { 40, 3, 1, 5, false, true, 1, 4, true, 0 },
};

}  // namespace

int main(int argc, char** argv)
{
    const int n_tables = argc > 1 ? atoi(argv[1]) : 4000;
    for (int ti = 0; ti < n_tables; ++ti) {
        Rng r{ 0xc0ffeeull * 1000003ull + (uint64_t)ti };
        const int kind = ti % 10;
        int n_items = r.range(2, 12);
        if (kind == 1) n_items = 2;
        if (kind == 2) n_items = r.range(0, 1);
        if (kind == 3) n_items = r.range(40, 80);
        std::vector<ItemState> items((size_t)n_items);
        int blk = 0;
        bool any_empty = false;
        for (int i = 0; i < n_items; ++i) {
            ItemState& st = items[(size_t)i];
            memset(&st, 0, sizeof st);
            int cnt = r.range(1, 40);
            if (kind == 3) cnt = r.range(300, 500);                       // a benchmark-sized batch: tens of thousands of workgroups
            if (kind == 4) cnt = i == 0 ? r.range(200, 400) : r.range(1, 20);             // one big registration in front: lop-sided boundaries only
            if (kind == 5) cnt = i + 1 == n_items ? r.range(200, 400) : r.range(1, 20);   // ... or at the end
            if (kind == 6) cnt = 8;                                       // equal registrations: ties between boundaries
            if (kind == 7 && r.pick(3) == 0) cnt = 0;                     // registrations without a workgroup (both clouds empty)
            if (kind == 8) cnt = i == 0 ? 3 * (ti % 5 + 1) : (i == 1 ? 9 * (ti % 5 + 1) : 0);   // the first boundary at a quarter exactly
            if (kind == 9) cnt = i == n_items / 2 ? r.range(100, 200) : r.range(1, 30);   // a big one in the middle: the even cut fails, an earlier boundary holds
            any_empty = any_empty || cnt == 0;
            st.blk_begin = blk; st.blk_count = cnt; blk += cnt;
        }
        const int n_blocks = blk;
        if (any_empty) ++hits[kEmptyItems];
        if (n_items == 2) ++hits[kTwoItems];
        if (n_items == 1) ++hits[kOneItem];
        if (n_items == 0) ++hits[kNoItems];
        if (n_blocks >= 16384) ++hits[kBigBatch];
        const Split even = plan_split(items, n_items, n_blocks);
        for (int share : { 300, 333, 400, 500, 250, 750, 1, 999, kFreeRunShare }) {
            const Split s = plan_split_uneven(items, n_items, n_blocks, share);
            // brute force: all boundaries, distances compared as integers (blk / n_blocks against share / 1000, cross-multiplied)
            int best_item = 0, best_blk = 0;
            bool found = false, tie = false;
            long long best_d = 0;
            for (int i = 1; i < n_items; ++i) {
                const long long b = items[(size_t)i].blk_begin;
                if (!quarter_ok(b, n_blocks)) continue;
                long long d = b * 1000 - (long long)n_blocks * share;
                if (d < 0) d = -d;
                if (found && d == best_d && b != best_blk) tie = true;
                if (!found || d < best_d) { found = true; tie = false; best_d = d; best_item = i; best_blk = (int)b; }
            }
            bool ok;
            if (!found) {
                ++hits[kNoBoundaryQualifies];
                ok = s.item == even.item && s.blk == even.blk;                     // falls back to plan_split's answer ...
                if (even.blk == 0 && even.item == 0) ++hits[kEvenCutAlsoNone];
                ok = ok && (even.blk == 0 || n_blocks == 0);                       // ... which cannot be a cut then
            } else {
                // the nearest boundary; registrations without workgroups share a boundary position: the first of them is taken
                ok = s.blk == best_blk && s.item == best_item;
                ok = ok && s.item >= 1 && s.item < n_items && items[(size_t)s.item].blk_begin == s.blk;          // an item boundary
                ok = ok && quarter_ok(s.blk, n_blocks);
                if (tie) ++hits[kTieTakesEarlier];
                if (s.blk * 4LL == n_blocks || (n_blocks - s.blk) * 4LL == n_blocks) ++hits[kExactlyAQuarter];
                if (even.blk == 0) ++hits[kUnevenWhereEvenIsNone];
                else ++hits[s.blk == even.blk ? kSameAsEven : kDiffersFromEven];
            }
            // "exactly when": a cut was returned if and only if a boundary qualifies (an empty batch cuts at workgroup 0: no cut either way)
            ok = ok && ((s.blk > 0) == (found && best_blk > 0));
            // the even cut, where it is one, qualifies: the uneven form engages on every batch the even form engages on
            ok = ok && (even.blk == 0 || s.blk > 0);
            if (!ok) {
                printf("table %d (kind %d) share %d: items %d blocks %d: plan_split_uneven (%d, %d), brute force %s (%d, %d), plan_split (%d, %d)\n", ti, kind, share,
                       n_items, n_blocks, s.item, s.blk, found ? "finds" : "finds none", best_item, best_blk, even.item, even.blk);
                return 1;
            }
        }
    }
    // ---- whether a run is cut at all, and in which form ----
    for (const FormCase& f : kFormCases)
        if (split_form(f.n_blocks, f.n_items, f.lanes_q, f.fixed_iters, f.can_stop, f.exact, f.interleave, f.min_blocks, f.alone) != f.form) {
            printf("split_form(%d blocks, %d items, %d lanes, fixed_iters %d, can_stop %d, exact %d, interleave %d, min_blocks %d, alone %d) is not %d\n", f.n_blocks,
                   f.n_items, f.lanes_q, f.fixed_iters, (int)f.can_stop, (int)f.exact, f.interleave, f.min_blocks, (int)f.alone, f.form);
            return 1;
        }
    if (kAutoSplitBlocks != 16384 || kAutoSplitItems != 64) { printf("the floor or the registration bound of the default moved\n"); return 1; }
    long long forms[3] = { 0, 0, 0 };
    for (int ti = 0; ti < n_tables; ++ti) {
        Rng r{ 0xf0f0ull * 1000003ull + (uint64_t)ti };
        auto of = [&](std::initializer_list<int> l) { return *(l.begin() + r.pick((int)l.size())); };
        const int n_items = of({ 0, 1, 2, 3, 63, 64, 65, 128, 256 });
        const int per_item = of({ 1, 8, 255, 256, 257, 449 });
        const int lanes = r.pick(8) ? 1 : 8, fixed = of({ 0, 1, 5, 10, -1 }), il = r.pick(3);
        const bool can_stop = r.pick(6) == 0, exact = r.pick(8) == 0, alone = r.pick(4) != 0;
        std::vector<ItemState> items((size_t)n_items);
        int blk = 0;
        for (int i = 0; i < n_items; ++i) { memset(&items[(size_t)i], 0, sizeof(ItemState)); items[(size_t)i].blk_begin = blk; items[(size_t)i].blk_count = per_item + (i == 0 ? r.range(-1, 1) : 0); blk += items[(size_t)i].blk_count; }
        const int min_blocks = of({ 2, 4, 8192, blk, blk + 1, 1 << 30 });
        // the rule restated from its description, condition by condition
        int want = 0;
        const bool may = !exact && !can_stop && lanes == 1 && n_items >= 2 && blk >= min_blocks;
        if (may && il == 1) want = 1;
        if (may && il == 2) want = 2;
        if (may && il == 0 && alone && fixed > 0 && blk >= 16384 && n_items <= 64) want = 2;
        BatchOptions o;
        PreparedBatch B;
        o.exact = exact; o.interleave = il; o.interleave_min_blocks = min_blocks;
        B.h_items = items; B.n_items = n_items; B.n_blocks = blk; B.lanes_q = lanes;
        memset(&B.prm, 0, sizeof B.prm); B.prm.fixed_iters = fixed;
        const int form = split_form(blk, n_items, lanes, fixed, can_stop, exact, il, min_blocks, alone);
        const Split s = plan_run_split(o, B, can_stop, alone);
        const Split w = want == 0 ? Split() : want == 1 ? plan_split(items, n_items, blk) : plan_split_uneven(items, n_items, blk);
        if (form != want || s.item != w.item || s.blk != w.blk) {
            printf("run %d: %d items, %d blocks, lanes %d, fixed_iters %d, can_stop %d, exact %d, alone %d, interleave %d, min_blocks %d: form %d (want %d), cut (%d, %d) (want (%d, %d))\n",
                   ti, n_items, blk, lanes, fixed, (int)can_stop, (int)exact, (int)alone, il, min_blocks, form, want, s.item, s.blk, w.item, w.blk);
            return 1;
        }
        ++forms[form];
        if (il == 0 && form == 2) ++hits[kAutoSplit];
        if (il == 0 && form == 0 && may && alone && fixed > 0 && blk >= 16384) ++hits[kAutoRefusedByItems];
        if (il == 0 && form == 0 && may && alone && fixed > 0 && n_items <= 64 && blk < 16384) ++hits[kAutoRefusedByFloor];
        if (il == 0 && form == 0 && may && alone && fixed <= 0 && n_items <= 64 && blk >= 16384) ++hits[kAutoRefusedByFreeIters];
        if (il == 0 && form == 0 && may && !alone && fixed > 0 && n_items <= 64 && blk >= 16384) ++hits[kAutoRefusedByOtherContext];
    }
    printf("forms none=%lld alternating=%lld free_running=%lld; ", forms[0], forms[1], forms[2]);
    printf("tables %d hits", n_tables);
    bool all = true;
    for (int k = 0; k < kEdges; ++k) { printf(" %s=%lld", kEdgeName[k], hits[k]); all = all && hits[k] > 0; }
    if (!all) { printf("\nan edge was never met\n"); return 1; }
    printf("\nsplit_uneven_check ok\n");
    return 0;
}
