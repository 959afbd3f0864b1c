"""Run-time options and the state a context keeps between calls.

Every name lisreg_set_option accepts is classified below, from the code and the tests that pin it:
  (a) NEUTRAL  - results equal the default's to the bit;
  (b) TIES     - bit-neutral under "canonical_ties" = 1 (it picks the search front-end, and the front-ends meet exactly equidistant
                 candidates in different orders); without canonical ties within the oracle bar;
  (c) DESIGN   - changes results by design;
  (d) DIAG     - diagnostics: must be results-neutral as well.
The CPU tests hold the table to the strcmp chains of lisreg_set_option / lisreg_get_option, so an option cannot arrive unclassified.
The GPU tests run every (a), (b) and (d) option in fresh contexts, walk scripted option changes over ONE prepared batch against fresh
contexts, drive the "row_reach" back-off, and tie the exact build to the CPU oracle.  Where the library has a readout, a leg asserts
that its option engaged: the seven ENGAGE values, the search counters ("count_searches"; and "cell_anchor_until" through them on the
graph front-end), the neighbour dump ("dump_neighbors"), the number of correspondence launches ("early_stop_chunk"); "first_pass_mm"
is shown to reach the second pass by test_first_pass_radius_leaves_one_to_four_neighbours.  "index_strip_cells" / "index_strip_cap"
can only be seen to keep the strip form (index_build_now), and a batch's "trace_cap" records have no reader."""
import os
import re

import numpy as np
import pytest

from helpers import copy_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
API = os.path.join(ROOT, "lis-slam_amd", "csrc", "lisreg_api.hip")

NEUTRAL, TIES, DESIGN, DIAG = "a", "b", "c", "d"

# name -> (class, reported by lisreg_get_option, why)
OPTIONS = {
    "cell_anchor_until": (NEUTRAL, True, "a second anchor candidate for the graph scan; the scan is certified either way"),
    "early_stop_chunk": (NEUTRAL, False, "how often the host looks at the finished counter"),
    "first_pass_mm": (NEUTRAL, False, "radius of the walk's first pass; the second pass completes the exact five"),
    "index_build": (NEUTRAL, True, "bucket sort and strip form build the same index bit for bit"),
    "index_strip_cells": (NEUTRAL, False, "strip geometry of the strip-form index build"),
    "index_strip_cap": (NEUTRAL, False, "points per strip of the small-workgroup strip build"),
    "xcd_order": (NEUTRAL, True, "dispatch order of the correspondence workgroups; partials are addressed by block id"),
    "interleave": (NEUTRAL, True, "two halves of a batch on two streams, same kernels per registration"),
    "interleave_min_blocks": (NEUTRAL, False, "size from which a batch is interleaved"),
    "row_reach": (NEUTRAL, True, "cell rows only near the queries; a query in a cell without rows walks"),
    "lanes_per_query": (NEUTRAL, True, "one or eight lanes per query (test_gpu_parity.test_lanes_per_query_variants_are_bit_identical)"),
    "feeder_threads": (NEUTRAL, True, "host packing of staged clouds (test_gpu_batch.test_staged_host_items_equal_align_batch)"),
    "feeder_numa": (NEUTRAL, False, "CPU binding of the packing threads"),
    "feeder_copy_engine": (NEUTRAL, False, "who packs a staged chunk (test_gpu_batch.test_staged_items_through_the_copy_engine_*)"),
    "graph_min_ratio": (TIES, True, "auto front-end choice: graph scan or cell walk"),
    "cell_min_ratio": (TIES, True, "auto front-end choice: cell rows"),
    "cell_rows_max_mb": (TIES, True, "caps the cell rows (cells past the cap walk) or makes auto decline them for the graph scan"),
    "search_mode": (TIES, True, "the front-end itself: 1, 3 and 5 give the same bits under canonical ties "
                                "(test_neighbors.test_equal_distances_resolve_by_original_index_in_every_front_end, test_round4_edges)"),
    # (class (b) without canonical ties — within the oracle bar — is what test_gpu_batch.test_search_front_ends_agree and
    #  test_round4_edges check for the front-ends these four lead to)
    "sort_sources": (DESIGN, True, "same neighbours, but a sorted batch sums its workgroups' rows in another order (last bits); "
                                   "auto equals the choice it makes (test_sort_sources_*)"),
    "exact_arithmetic": (DESIGN, True, "the reference's arithmetic"),
    "canonical_ties": (DESIGN, True, "resolves exactly equal distances by original index"),
    "rebuild_targets_each_run": (DESIGN, True, "every run re-reads the target's points from the caller's buffer"),
    "count_searches": (DIAG, False, "search counters"),
    "dump_neighbors": (DIAG, False, "keeps every query's five neighbours for lisreg_get_neighbors"),
    "trace_cap": (DIAG, False, "per-item trace records of a batch"),
}
# what lisreg_get_option reports besides the options themselves
READ_ONLY = {"front_end", "index_build_now", "sorted_now", "xcd_order_now", "interleaved_now", "row_reach_now", "row_reach_misses",
             "feeder_chunks", "feeder_chunks_by_copy_engine", "feeder_numa_node", "feeder_numa_cpus", "comm_nranks",
             "index_kib_grid", "index_kib_front_end", "index_kib_front_end_built", "index_target_points"}


def option_names(fn, path=API):
    """The names a function of lisreg_api.hip compares `name` with (its strcmp chain)."""
    src = open(path).read()
    start = src.index(f"\nint {fn}(")
    body = src[start:src.index("\n}\n", start)]
    return set(re.findall(r'strcmp\(name,\s*"([^"]+)"\)', body))


def test_option_table_covers_every_settable_name():
    names = option_names("lisreg_set_option")
    assert set(OPTIONS) == names, (sorted(names - set(OPTIONS)), sorted(set(OPTIONS) - names))
    assert all(cls in (NEUTRAL, TIES, DESIGN, DIAG) for cls, _, _ in OPTIONS.values())


def test_option_table_covers_every_readable_name():
    names = option_names("lisreg_get_option")
    want = {n for n, (_, readable, _) in OPTIONS.items() if readable} | READ_ONLY
    assert want == names, (sorted(names - want), sorted(want - names))


def test_option_scan_sees_a_new_option(tmp_path):
    """the chain scan itself: one more strcmp in a copy of the source is one more name (and the table check would fail on it)"""
    src = open(API).read()
    anchor = '    if (!strcmp(name, "interleave_min_blocks"))'
    assert anchor in src
    copy = tmp_path / "lisreg_api.hip"
    copy.write_text(src.replace(anchor, '    if (!strcmp(name, "new_knob")) { return LISREG_OK; }\n' + anchor, 1))
    assert option_names("lisreg_set_option", str(copy)) == option_names("lisreg_set_option") | {"new_knob"}


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU

ENGAGE = ("front_end", "lanes_per_query", "interleaved_now", "xcd_order_now", "row_reach_now", "index_build_now", "sorted_now")
BIG = 1 << 30


def _cases(n, h=16, w=300):
    """The batch of test_gpu_batch._cases: a 30 k-point submap and n scans."""
    from lisreg import synth
    tc, ts = synth.make_submap(30000, 42)
    out = []
    for i in range(n):
        sc = synth.make_scan(h, w, 4000 + i)
        out.append(dict(src_corner=sc["corner"], src_surf=sc["surf"],
                        T_init=synth.perturb_pose(sc["T_true"], np.random.default_rng(i)), T_true=sc["T_true"]))
    return tc, ts, out


class Batch:
    """One batch as host clouds (align_batch / align) and as device records (batch_prepare_device / batch_run)."""

    def __init__(self, n=9, h=16, w=300, fixed_iters=5):
        import lisreg
        self.tc, self.ts, self.cases = _cases(n, h, w)
        self.T0 = np.array([c["T_init"] for c in self.cases], np.float32)
        D = lisreg.DeviceArray
        self.recs = [(D(lisreg.pack_device_records(c["src_corner"])), D(lisreg.pack_device_records(c["src_surf"]))) for c in self.cases]
        self.items = [dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0]) for a, b in self.recs]
        self.p_fixed = lisreg.default_params(1); self.p_fixed.fixed_iters = fixed_iters
        self.p_free = lisreg.default_params(1)
        self.n_src = sum(len(c["src_corner"]) + len(c["src_surf"]) for c in self.cases)


def _context(front, opts=()):
    """A private context with the matrix's base settings (one lane per query and interleave_min_blocks = 4, so that interleaving and the
    XCD tables engage on a small batch; targets rebuilt inside every run, so that the index-build options and "row_reach" engage)."""
    import lisreg
    c = lisreg.Context(0)
    c.set_option("search_mode", front); c.set_option("lanes_per_query", 1); c.set_option("interleave_min_blocks", 4)
    c.set_option("rebuild_targets_each_run", 1)
    for k, v in opts:
        c.set_option(k, v)
    return c


def _run_all(c, b, opts=()):
    """The legs of one option set: prepare / run / fetch with fixed iterations (engagement read behind it), an early-stopping
    align_batch (its correspondence launches counted by the HIP-event profiling), and a single align with its per-iteration trace.
    Returns (results, ENGAGE readouts, other observations)."""
    o = dict(opts)
    c.set_target(b.tc, b.ts)
    c.batch_prepare_device(b.items, b.T0, b.p_fixed)
    c.batch_run()
    fixed = c.batch_fetch()
    state = {k: c.get_option(k) for k in ENGAGE}
    seen = {}
    if o.get("count_searches"):
        cnt = c.counters()
        seen["processed"], seen["walked"] = int(cnt[:, 1].sum()), cnt[:, 0].tolist()
    if o.get("dump_neighbors"):
        seen["dumped"] = int((c.neighbors(b.n_src)[:5] >= 0).any(0).sum())
    c.set_profiling(True)
    free = c.align_batch(b.cases, b.T0, b.p_free)
    c.set_profiling(False)
    seen["launches"] = c.timing()["assoc_launches"]
    single = c.align(b.cases[0]["src_corner"], b.cases[0]["src_surf"], b.T0[0], b.p_free)
    return dict(fixed=fixed, free=free, single=single), state, seen


def _same(a, b):
    """equal to the bit: poses, stats, traces"""
    (Tf, sf), (Tf2, sf2) = a["fixed"], b["fixed"]
    (Te, se), (Te2, se2) = a["free"], b["free"]
    (T1, s1, tr1), (T12, s12, tr12) = a["single"], b["single"]
    bad = []
    if not (np.array_equal(Tf, Tf2) and sf == sf2):
        bad.append(f"fixed-iteration batch: items {np.flatnonzero((Tf != Tf2).any(1)).tolist()} differ")
    if not (np.array_equal(Te, Te2) and se == se2):
        bad.append(f"early-stopping batch: items {np.flatnonzero((Te != Te2).any(1)).tolist()} differ")
    if not (np.array_equal(T1, T12) and s1 == s12 and np.array_equal(tr1, tr12)):
        bad.append("single registration (pose / stats / trace) differs")
    return bad


def _expected_state(front, opts, b):
    """what ENGAGE must read after the fixed-iteration run of an option set (the code's decisions, restated)"""
    o = dict(opts)
    mode = o.get("search_mode", front)
    lanes = 8 if (mode == 1 and o.get("lanes_per_query", 1) != 1 and b.n_src <= 131072) else 1
    xo = o.get("xcd_order", 2)
    n_blocks = sum((len(c["src_corner"]) + 255) // 256 + (len(c["src_surf"]) + 255) // 256 for c in b.cases)
    xcd = lanes != 8 and mode in (3, 5) and (xo == 1 or (xo == 2 and n_blocks >= 2048 and len(b.cases) >= 32))
    inter = o.get("interleave", 0) != 0 and lanes == 1 and n_blocks >= max(o.get("interleave_min_blocks", 4), 2)
    reach = mode == 5 and lanes == 1 and o.get("row_reach", 1) != 0
    return dict(front_end=mode, lanes_per_query=lanes, interleaved_now=int(inter), xcd_order_now=int(xcd), row_reach_now=int(reach),
                sorted_now=0)


# (option, value) legs of the fresh-context matrix: classes (a) and (d); the default's own value is the reference
MATRIX = [("first_pass_mm", v) for v in (0, 1, 150, 100000)] + \
         [("early_stop_chunk", v) for v in (0, 1, 2, 5, -1)] + \
         [("cell_anchor_until", v) for v in (0, 1000)] + \
         [("index_strip_cap", v) for v in (64, 16384)] + \
         [("index_strip_cells", v) for v in (1, 0, 100000, -7)] + \
         [("index_build", v) for v in (0, 1, 2)] + \
         [("xcd_order", v) for v in (0, 1, 2)] + \
         [("interleave", v) for v in (0, 1, 2)] + \
         [("sort_sources", v) for v in (0, 2)] + \
         [("row_reach", 0), ("lanes_per_query", 0)] + \
         [("count_searches", 1), ("dump_neighbors", 1), ("trace_cap", 0), ("trace_cap", 16)]
# the walk's radius-limited first pass runs where a query has no seeds and the iteration is not a wide one: GN iteration 0 of a batch
# searched with eight lanes per query (wide_from_small = 1) — lanes_per_query auto on front 1 (one lane: iteration 0 is wide)
MATRIX_COMBOS = [(("lanes_per_query", 0), ("first_pass_mm", v)) for v in (0, 1, 150, 100000)] + \
                [(("interleave", 1), ("interleave_min_blocks", BIG)), (("interleave", 2), ("interleave_min_blocks", -3)),
                 (("interleave", 2), ("xcd_order", 1)), (("interleave", 1), ("xcd_order", 1), ("first_pass_mm", 150)),
                 (("count_searches", 1), ("cell_anchor_until", 0)), (("count_searches", 1), ("cell_anchor_until", 1000))]


@pytest.mark.gpu
@pytest.mark.parametrize("front", [1, 3, 5])
def test_fresh_context_matrix_of_neutral_options(front):
    """Every class-(a) and class-(d) option, each value, in a fresh context: poses, stats and the per-iteration trace equal the
    default's to the bit, and the option engaged where the library can show it (module docstring)."""
    b = Batch()
    c = _context(front)
    try:
        ref, ref_state, _ = _run_all(c, b)
    finally:
        c.close()
    assert ref_state["index_build_now"] == 1 and ref_state == dict(_expected_state(front, (), b), index_build_now=1), ref_state
    failures, seen = [], {}
    for opts in [(leg,) for leg in MATRIX] + MATRIX_COMBOS:
        c = _context(front, opts)
        try:
            got, state, seen[opts] = _run_all(c, b, opts)
        finally:
            c.close()
        want = _expected_state(front, opts, b)
        idx = dict(opts).get("index_build", 2)
        want["index_build_now"] = 0 if idx == 0 else 1
        if state != want:
            failures.append(f"front {front} {opts}: did not engage as asked: {state} != {want}")
        o = dict(opts)
        if o.get("count_searches") and front != 1 and not seen[opts]["processed"] > 0:
            failures.append(f"front {front} {opts}: no search counted")          # (the cell walk of front 1 counts nothing of its own)
        if o.get("dump_neighbors") and not seen[opts]["dumped"] > b.n_src // 2:
            failures.append(f"front {front} {opts}: {seen[opts]['dumped']} of {b.n_src} queries dumped")
        failures += [f"front {front} {opts}: {m}" for m in _same(ref, got)]
    # "early_stop_chunk": 0 never looks (every one of max_iters launches), 1 looks after every iteration (the fewest), auto in between
    launches = {v: seen[(("early_stop_chunk", v),)]["launches"] for v in (0, 1, 2, 5, -1)}
    needed = max(s["iters"] for s in ref["free"][1]) + 1
    if not (launches[0] == b.p_free.max_iters and all(launches[1] <= n for n in launches.values()) and
            (launches[1] < launches[0] or needed >= b.p_free.max_iters)):
        failures.append(f"front {front}: early_stop_chunk -> correspondence launches {launches} (max_iters {b.p_free.max_iters})")
    if front == 3:      # "cell_anchor_until": the anchor out of the query's grid column changes how many queries fall back to the walk
        w0, w1 = (seen[(("count_searches", 1), ("cell_anchor_until", v))]["walked"] for v in (0, 1000))
        print(f"[cell_anchor_until] walked per iteration: 0 -> {w0[:6]}, 1000 -> {w1[:6]}")
        if w0 == w1:
            failures.append(f"front 3: cell_anchor_until 0 and 1000 walked the same queries {w0[:6]}")
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
@pytest.mark.parametrize("front", [1, 3, 5])
def test_front_end_choice_options_are_neutral_under_canonical_ties(front):
    """Class (b): "graph_min_ratio" / "cell_min_ratio" forced either way under search_mode 4, and "cell_rows_max_mb" capping the rows
    (forced cell rows) or declining them (auto): with canonical ties the bits of the front-end they lead to."""
    b = Batch()
    c = _context(front, (("canonical_ties", 1),))
    try:
        ref, _, _ = _run_all(c, b)
    finally:
        c.close()
    legs = {1: [(("graph_min_ratio", BIG), ("cell_min_ratio", BIG)), (("graph_min_ratio", BIG),)],
            3: [(("graph_min_ratio", 0),), (("graph_min_ratio", 0), ("cell_min_ratio", 0), ("cell_rows_max_mb", 1))],
            5: [(("cell_min_ratio", 0),), (("graph_min_ratio", BIG), ("cell_min_ratio", 0)), (("search_mode", 5), ("cell_rows_max_mb", 1))]}[front]
    failures = []
    for opts in legs:
        opts = (("search_mode", 4), ("canonical_ties", 1)) + tuple(opts)
        c = _context(front, opts)
        try:
            got, state, _ = _run_all(c, b)
            capped = dict(opts).get("cell_rows_max_mb") == 1 and state["front_end"] == 5 and (c.target_cell_rows(0, 1)["table"] == -1).any()
        finally:
            c.close()
        if state["front_end"] != front:
            failures.append(f"{opts}: front-end {state['front_end']}, wanted {front}")
        if dict(opts).get("cell_rows_max_mb") == 1 and front == 5 and not capped:
            failures.append(f"{opts}: the rows were not capped")
        failures += [f"front {front} {opts}: {m}" for m in _same(ref, got)]
    assert not failures, "\n".join(failures)


@pytest.mark.gpu
def test_sort_sources_probe_equals_the_choice_it_makes():
    """"sort_sources" = 2 probes a batch of >= 65 536 source points and sorts it or not: the bits are those of the explicit choice."""
    b = Batch(n=3, h=32, w=900)
    assert b.n_src >= 65536
    out, sorted_now = {}, {}
    for sort in (2, 0, 1):
        c = _context(5, (("sort_sources", sort),))
        try:
            c.set_target(b.tc, b.ts)
            c.batch_prepare_device(b.items, b.T0, b.p_fixed)
            c.batch_run()
            out[sort] = c.batch_fetch()
            sorted_now[sort] = c.get_option("sorted_now")
        finally:
            c.close()
    assert sorted_now[0] == 0 and sorted_now[1] == 1
    pick = sorted_now[2]
    assert np.array_equal(out[2][0], out[pick][0]) and out[2][1] == out[pick][1], pick


@pytest.mark.gpu
@pytest.mark.parametrize("front", [1, 3, 5])
def test_sort_sources_changes_the_summation_order_only(front):
    """Class (c) "sort_sources" = 1: the search is exact on any order — at GN iteration 0 (same initial poses) every query has the same
    five neighbours and accept flag as unsorted (the dump follows the sorted order within each cloud: compared as sets of queries'
    records), so the correspondence counts are equal — but the rows are summed per workgroup of the SORTED order: the poses agree to
    the fp32 summation order, not necessarily to the bit."""
    import lisreg
    b = Batch()
    p1 = lisreg.default_params(1); p1.fixed_iters = 1
    out = {}
    for sort in (0, 1):
        c = _context(front, (("sort_sources", sort), ("dump_neighbors", 1)))
        try:
            c.set_target(b.tc, b.ts)
            c.batch_prepare_device(b.items, b.T0, p1)
            c.batch_run()
            T, st = c.batch_fetch()
            assert c.get_option("sorted_now") == sort
            out[sort] = (T, st, c.neighbors(b.n_src))
        finally:
            c.close()
    (T0_, s0, nb0), (T1, s1, nb1) = out[0], out[1]
    off = 0
    for case in b.cases:
        for key in ("src_corner", "src_surf"):
            n = len(case[key])
            a, z = nb0[:, off:off + n], nb1[:, off:off + n]
            assert np.array_equal(a[:, np.lexsort(a)], z[:, np.lexsort(z)]), (front, off)
            off += n
    assert [s["n_corr_last"] for s in s0] == [s["n_corr_last"] for s in s1]
    assert np.abs(T0_.astype(np.float64) - T1.astype(np.float64)).max() <= 1e-5
    differ = np.flatnonzero((T0_ != T1).any(1)).tolist()
    print(f"[sort_sources] front {front}: items whose pose bits differ sorted / unsorted after one iteration: {differ}")
    assert differ                       # (why the option is class (c): 7 or 8 of the 9 items differ in their last bits)


@pytest.mark.gpu
def test_first_pass_radius_leaves_one_to_four_neighbours():
    """The 150 mm legs reach the walk's second pass over cells the first pass already took points from (lisreg_assoc.hip, the unseeded
    non-wide walk): at GN iteration 0 of an eight-lane batch every query is unseeded, and for many of them 1 to 4 of their five
    neighbours (the dump of that iteration, distances from the query under its initial pose) lie inside 150 mm."""
    import lisreg
    from lisreg import synth
    b = Batch()
    p1 = lisreg.default_params(1); p1.fixed_iters = 1
    c = _context(1, (("lanes_per_query", 0), ("first_pass_mm", 150), ("dump_neighbors", 1)))
    try:
        c.set_target(b.tc, b.ts)
        c.batch_prepare_device(b.items, b.T0, p1)
        c.batch_run()
        c.batch_fetch()
        assert c.get_option("lanes_per_query") == 8 and c.front_end() == 1
        nb = c.neighbors(b.n_src)
    finally:
        c.close()
    tgt = [synth.pcl_xyz(b.tc).astype(np.float64), synth.pcl_xyz(b.ts).astype(np.float64)]
    inside, off = [], 0
    for case, T in zip(b.cases, b.T0):
        M = synth.pose_matrix(T)
        for k, key in enumerate(("src_corner", "src_surf")):
            q = synth.pcl_xyz(case[key]).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
            ids = nb[:5, off:off + len(q)].T
            d = np.where(ids >= 0, np.linalg.norm(tgt[k][np.maximum(ids, 0)] - q[:, None, :], axis=2), np.inf)
            inside.append((d < 0.15).sum(1))
            off += len(q)
    inside = np.concatenate(inside)
    partial = int(((inside >= 1) & (inside <= 4)).sum())
    print(f"[first_pass_mm 150] queries with 1-4 of their five neighbours inside 150 mm at iteration 0: {partial} of {len(inside)}")
    assert off == b.n_src and partial >= len(inside) // 40          # (2225 of 43144 on this batch)


@pytest.mark.gpu
def test_out_of_range_values():
    """refused: a negative first-pass radius, xcd_order / interleave / index_build / search_mode values they do not name; clamped: the
    numeric knobs (the clamped values run as their bounds — the matrix runs index_strip_cells -7 and interleave_min_blocks -3)"""
    import lisreg
    c = lisreg.Context(0)
    try:
        for name, value in (("first_pass_mm", -450), ("xcd_order", 3), ("xcd_order", -1), ("interleave", 3), ("interleave", -1),
                            ("index_build", 3), ("search_mode", 0), ("search_mode", 2), ("search_mode", 6)):
            with pytest.raises(lisreg.LisregError) as e:
                c.set_option(name, value)
            assert e.value.code == lisreg.ERR_ARG, (name, value)
        c.set_option("cell_anchor_until", -4)
        assert c.get_option("cell_anchor_until") == 0
        c.set_option("first_pass_mm", 0)
    finally:
        c.close()


def _fresh(b, front, opts, prep="fixed"):
    """fresh context, same options, the batch run once"""
    c = _context(front, opts)
    try:
        c.set_target(b.tc, b.ts)
        if prep == "free":
            return c.align_batch(b.cases, b.T0, b.p_free)
        c.batch_prepare_device(b.items, b.T0, b.p_fixed)
        c.batch_run()
        return c.batch_fetch()
    finally:
        c.close()


def _prepared(b, front, opts):
    import lisreg
    c = _context(front, opts)
    D = lisreg.DeviceArray
    tcd, tsd = D(lisreg.pack_device_records(b.tc)), D(lisreg.pack_device_records(b.ts))
    c.set_target_device(tcd.ptr, len(b.tc), tsd.ptr, len(b.ts))
    c.batch_prepare_device(b.items, b.T0, b.p_fixed)
    return c, (tcd, tsd)


def _step(c):
    c.batch_run()
    return c.batch_fetch()


def _diff(a, b):
    return np.flatnonzero((a[0] != b[0]).any(1)).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("switch", ["interleave_off", "min_blocks_up", "unsplit_first"])
def test_interleave_then_not_on_one_prepared_batch(switch):
    """lisreg_batch_prepare caches the batch's XCD dispatch table; an interleaved run writes one table per half over it (ids relative
    to the half).  A later unsplit run of the same prepared batch — interleave switched off, or interleave_min_blocks raised past the
    batch — must not read those as the whole batch's table (it ran blocks [0, n - split) twice and the second half never: stale poses
    for the second half's registrations)."""
    b = Batch()
    base = (("xcd_order", 1),)
    ref = _fresh(b, 3, base)
    c, keep = _prepared(b, 3, base + (("interleave", 0 if switch == "unsplit_first" else 2),))
    try:
        runs = []
        if switch == "unsplit_first":
            runs.append((_step(c), c.get_option("interleaved_now")))
            c.set_option("interleave", 2)
            runs.append((_step(c), c.get_option("interleaved_now")))
            c.set_option("interleave", 0)
            runs.append((_step(c), c.get_option("interleaved_now")))
            want = [0, 1, 0]
        else:
            runs.append((_step(c), c.get_option("interleaved_now")))
            if switch == "interleave_off":
                c.set_option("interleave", 0)
            else:
                c.set_option("interleave_min_blocks", BIG)
            runs.append((_step(c), c.get_option("interleaved_now")))
            c.set_option("interleave", 2); c.set_option("interleave_min_blocks", 4)
            runs.append((_step(c), c.get_option("interleaved_now")))
            want = [1, 0, 1]
        assert c.get_option("xcd_order_now") == 1
    finally:
        c.close()
    assert [r[1] for r in runs] == want
    for k, (res, _) in enumerate(runs):
        assert np.array_equal(res[0], ref[0]) and res[1] == ref[1], f"run {k} ({switch}): items {_diff(res, ref)} differ from a fresh context"


@pytest.mark.gpu
def test_option_changes_between_runs_of_one_prepared_batch():
    """xcd_order 1 -> 0 -> 1, rebuild_targets_each_run 1 -> 0 -> 1, and the calls that drop the prepared batch (set_target*, and
    options that change what prepare decides): batch_run then fails with ERR_ARG; a re-prepare gives a fresh context's bits."""
    import lisreg
    b = Batch()
    base = (("xcd_order", 1), ("interleave", 2))
    ref = _fresh(b, 3, base)
    c, keep = _prepared(b, 3, base)
    try:
        got = []
        for name, value, now in (("xcd_order", 1, 1), ("xcd_order", 0, 0), ("xcd_order", 1, 1), ("rebuild_targets_each_run", 0, 1),
                                 ("rebuild_targets_each_run", 1, 1), ("xcd_order", 2, 0), ("xcd_order", 1, 1)):
            c.set_option(name, value)
            got.append((f"{name}={value}", _step(c)))
            assert c.get_option("xcd_order_now") == now, (name, value)
        for name in ("set_target_device", "set_target", "search_mode", "row_reach", "exact_arithmetic", "index_build", "canonical_ties"):
            if name == "set_target_device":
                c.set_target_device(keep[0].ptr, len(b.tc), keep[1].ptr, len(b.ts))
            elif name == "set_target":
                c.set_target(b.tc, b.ts)                         # (the host path: the same points)
            else:
                c.set_option(name, c.get_option(name))          # the same value: still a batch to prepare again
            with pytest.raises(lisreg.LisregError) as e:
                c.batch_run()
            assert e.value.code == lisreg.ERR_ARG, name
            c.batch_prepare_device(b.items, b.T0, b.p_fixed)
            got.append((f"re-prepared after {name}", _step(c)))
    finally:
        c.close()
    for what, res in got:
        assert np.array_equal(res[0], ref[0]) and res[1] == ref[1], f"{what}: items {_diff(res, ref)} differ from a fresh context"


@pytest.mark.gpu
@pytest.mark.parametrize("front", [3, 5])
def test_target_points_changed_in_place_between_runs(front):
    """rebuild_targets_each_run = 1 reads the target from the caller's buffer in every run: overwrite it in place (same counts, points
    inside the original bounding box) and the next run of the SAME prepared batch equals a fresh context set to the new points (canonical
    ties: the fresh grid's geometry differs).  The query marks of "row_reach" depend on the sources only, so they stay right."""
    import lisreg
    from lisreg import synth
    b = Batch()
    opts = (("canonical_ties", 1),)
    rng = np.random.default_rng(77)
    new = []
    for cloud in (b.tc, b.ts):
        xyz = synth.pcl_xyz(cloud).astype(np.float64)
        lo, hi = xyz.min(0), xyz.max(0)
        moved = np.clip(xyz + rng.normal(0, 0.03, xyz.shape), lo, hi).astype(np.float32)
        new.append(synth.to_pcl(moved))
    c, (tcd, tsd) = _prepared(b, front, opts)
    try:
        first = _step(c)
        tcd.upload(lisreg.pack_device_records(new[0])); tsd.upload(lisreg.pack_device_records(new[1]))
        second = _step(c)
        assert c.get_option("row_reach_now") == (1 if front == 5 else 0)
    finally:
        c.close()
    b_old = (b.tc, b.ts)
    ref_old = _fresh(b, front, opts)
    b.tc, b.ts = new
    ref_new = _fresh(b, front, opts)
    b.tc, b.ts = b_old
    assert np.array_equal(first[0], ref_old[0]) and first[1] == ref_old[1]
    assert not np.array_equal(ref_old[0], ref_new[0])
    assert np.array_equal(second[0], ref_new[0]) and second[1] == ref_new[1], _diff(second, ref_new)


@pytest.mark.gpu
def test_early_stop_after_a_batch_that_converged_fast():
    """last_launches (where the host first looks at the finished counter) comes from the last fetched batch: after a batch that
    converged in a few iterations, a batch that needs the full bound gives a fresh context's bits."""
    b = Batch()
    ref = _fresh(b, 1, (), prep="free")
    c = _context(1)
    try:
        c.set_target(b.tc, b.ts)
        easy = np.array([c_["T_true"] for c_ in b.cases], np.float32)
        _, st = c.align_batch(b.cases, easy, b.p_free)
        easy_iters = max(s["iters"] for s in st)
        got = c.align_batch(b.cases, b.T0, b.p_free)
    finally:
        c.close()
    assert max(s["iters"] for s in ref[1]) > easy_iters, (easy_iters, ref[1])
    assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], _diff(got, ref)


@pytest.mark.gpu
def test_row_reach_walk_and_back_off():
    """Initial poses 1.7 m off: the registrations move their queries out of the cells the marks reach (a metre around the initial
    poses).  Those queries walk: the bits of row_reach = 0.  The fetch counts them; more than one query-iteration in a thousand and the
    prepared batch's next run builds all rows, as do the next 32 prepares; the 33rd marks again.  K runs, one fetch: K times the misses."""
    import lisreg
    from lisreg import synth
    D = lisreg.DeviceArray
    tc, ts = synth.make_submap(60000)
    scans = [synth.make_scan(32, 900, 2000 + i) for i in range(8)]
    T0 = np.array([synth.perturb_pose(s["T_true"], np.random.default_rng(9000 + i)) for i, s in enumerate(scans)], np.float32)
    T0[:, 3] += 1.2; T0[:, 4] -= 1.2                     # (12 iterations bring most of them the 1.7 m back: ~2 misses per thousand)
    p = lisreg.default_params(1); p.fixed_iters = 12
    tcd, tsd = D(lisreg.pack_device_records(tc)), D(lisreg.pack_device_records(ts))
    recs = [(D(lisreg.pack_device_records(s["corner"])), D(lisreg.pack_device_records(s["surf"]))) for s in scans]
    items = [dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0]) for a, b in recs]

    def ctx(reach):
        c = lisreg.Context(0)
        c.set_option("search_mode", 5); c.set_option("rebuild_targets_each_run", 1); c.set_option("sort_sources", 0)
        c.set_option("row_reach", reach)
        c.set_target_device(tcd.ptr, len(tc), tsd.ptr, len(ts))
        return c

    ref_c = ctx(0)
    ref_c.batch_prepare_device(items, T0, p)
    ref = _step(ref_c)
    ref_tr = ref_c.align(scans[0]["corner"], scans[0]["surf"], T0[0], p)
    ref_c.close()
    c = ctx(1)
    tr = c.align(scans[0]["corner"], scans[0]["surf"], T0[0], p)
    assert c.get_option("row_reach_now") == 1
    c.close()
    c = ctx(1)
    try:
        c.batch_prepare_device(items, T0, p)
        first = _step(c)
        assert c.get_option("row_reach_now") == 1
        miss1 = c.get_option("row_reach_misses")
        n_elems = sum(a.shape[0] + b.shape[0] for a, b in recs)
        print(f"[row_reach] initial poses 1.7 m off: {miss1} query-iterations of {n_elems * p.fixed_iters} found their cell without rows")
        assert miss1 * 1000 > n_elems * p.fixed_iters
        again = _step(c)                                  # the same prepared batch: all rows now
        assert c.get_option("row_reach_now") == 0
        for k in range(32):
            c.batch_prepare_device(items, T0, p)
            c.batch_run()
            assert c.get_option("row_reach_now") == 0, k
        c.batch_prepare_device(items, T0, p)              # the 33rd marks again
        for _ in range(3):
            c.batch_run()
        assert c.get_option("row_reach_now") == 1
        third = c.batch_fetch()
        assert c.get_option("row_reach_misses") == 3 * miss1
    finally:
        c.close()
    for res in (first, again, third):
        assert np.array_equal(res[0], ref[0]) and res[1] == ref[1], _diff(res, ref)
    assert np.array_equal(tr[0], ref_tr[0]) and tr[1] == ref_tr[1] and np.array_equal(tr[2], ref_tr[2])


@pytest.mark.gpu
def test_other_batches_between_leave_a_batch_its_bits():
    """One context, three batches prepared, run and fetched in turn under the auto front-end: A (the nine scans against the shared
    submap), B (two registrations with small scattered targets of their own in slots 1 and 2 and "cell_rows_max_mb" = 1: auto takes the
    cell rows, finds that they do not fit together, releases them and takes the graph scan), A again with the bound put back.  What one
    batch leaves in the context — decisions, tables, probe and back-off memory, released rows — must not reach the next: all three
    results equal fresh contexts' byte for byte, and the second A engages as the fresh one does."""
    import lisreg
    from lisreg import synth
    b = Batch()
    rng = np.random.default_rng(31)
    own = [[synth.to_pcl(rng.uniform(-10, 10, (50, 3)).astype(np.float32)) for _ in range(2)] for _ in range(2)]     # 200 target points in all
    items_b = [dict(b.items[i], target=1 + i) for i in range(2)]
    readouts = ("front_end", "lanes_per_query", "index_build_now", "row_reach_now")

    def context(max_mb=None):
        c = lisreg.Context(0)
        c.set_option("canonical_ties", 1); c.set_option("sort_sources", 0); c.set_option("rebuild_targets_each_run", 1)
        c.set_option("search_mode", 4)
        if max_mb is not None:
            c.set_option("cell_rows_max_mb", max_mb)
        return c

    def run_a(c):
        c.batch_prepare_device(b.items, b.T0, b.p_fixed)
        return _step(c), {k: c.get_option(k) for k in readouts}

    def run_b(c):
        c.batch_prepare_device(items_b, b.T0[:2], b.p_fixed)
        return _step(c), {k: c.get_option(k) for k in readouts}

    def set_own(c):
        for i, (tc, ts) in enumerate(own):
            c.set_target(tc, ts, slot=1 + i)

    c = context()
    try:
        c.set_target(b.tc, b.ts)
        fresh_a, fresh_a_state = run_a(c)
    finally:
        c.close()
    c = context(1)
    try:
        set_own(c)
        fresh_b, fresh_b_state = run_b(c)
    finally:
        c.close()
    assert fresh_b_state["front_end"] == 3, fresh_b_state          # (5: the rows fitted, nothing was declined)
    c = context()
    try:
        c.set_target(b.tc, b.ts)
        set_own(c)
        max_mb = c.get_option("cell_rows_max_mb")
        first_a, first_a_state = run_a(c)
        c.set_option("cell_rows_max_mb", 1)
        got_b, got_b_state = run_b(c)
        c.set_option("cell_rows_max_mb", max_mb)
        second_a, second_a_state = run_a(c)
    finally:
        c.close()
    print(f"[batches between] A {fresh_a_state}, B {fresh_b_state}")
    for what, got, want in (("first A", first_a, fresh_a), ("B", got_b, fresh_b), ("second A", second_a, fresh_a)):
        assert got[0].tobytes() == want[0].tobytes() and got[1] == want[1], f"{what}: items {_diff(got, want)} differ from a fresh context"
    assert first_a_state == fresh_a_state and got_b_state == fresh_b_state
    assert second_a_state == fresh_a_state, (second_a_state, fresh_a_state)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [2234, 2240])
def test_exact_build_through_neutral_options_equals_oracle(oracle, seed):
    """The exact build through the class-(a) options it does not switch off: per-iteration correspondence counts equal the CPU
    restatement's, poses within test_exact's two float steps, and every option's pose the bits of the exact build's default."""
    import lisreg
    from lisreg import synth
    from test_exact import pose_ulps
    case = synth.make_case(h=16, w=450, m_points=20000, scan_seed=seed, trans=0.4, rot_deg=2.5)
    p_o = oracle.default_params(1)
    p = copy_params(p_o, lisreg.Params)
    To, so, tro = oracle.align(case["tgt_corner"], case["tgt_surf"], case["src_corner"], case["src_surf"], case["T_init"], p_o)

    def run(front, opts):
        c = lisreg.Context(0)
        try:
            c.set_option("exact_arithmetic", 1); c.set_option("search_mode", front); c.set_option("lanes_per_query", 1)
            for k, v in opts:
                c.set_option(k, v)
            c.set_target(case["tgt_corner"], case["tgt_surf"])
            return c.align(case["src_corner"], case["src_surf"], case["T_init"], p)
        finally:
            c.close()

    legs = {1: [(("first_pass_mm", v),) for v in (0, 150, 100000)] + [(("early_stop_chunk", 1),), (("early_stop_chunk", 0),),
                                                                     (("lanes_per_query", 0),)] +
               [(("lanes_per_query", 0), ("first_pass_mm", v)) for v in (0, 150, 100000)],      # (eight lanes: iteration 0 takes the first pass)
            3: [(("cell_anchor_until", v),) for v in (0, 1000)] + [(("rebuild_targets_each_run", 1), ("index_build", v)) for v in (0, 1)],
            5: [(("rebuild_targets_each_run", 1),), (("rebuild_targets_each_run", 1), ("index_strip_cells", 1), ("index_strip_cap", 64))]}
    for front, opt_list in legs.items():
        T0_, s0, tr0 = run(front, ())
        for opts in opt_list:
            T, s, tr = run(front, opts)
            assert s["iters"] == so["iters"] and s["status"] == so["status"], (front, opts, s, so)
            assert np.array_equal(tr[:, 0], tro[:, 0]), (front, opts, tr[:, 0], tro[:, 0])
            assert pose_ulps(T, To) <= 2.0, (front, opts)
            assert np.array_equal(T, T0_) and s == s0 and np.array_equal(tr, tr0), (front, opts)
