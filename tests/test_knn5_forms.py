"""Every search front-end of k_assoc_walk (csrc/lisreg_assoc.hip) per query against the integer definition of tests/knn5_ref.py.

The promise under test: each front-end — the cell walk with one and with eight lanes per query, the k-NN graph scan, the cell rows, the
rows thinned by "row_reach" and the rows capped by "cell_rows_max_mb" — returns the true five nearest target points inside
sqrt(knn_sq_thresh), as nearestKSearch(5) plus the `sqDist[4] < tau` test would.  All coordinates are multiples of 1/64 m and every pose
has zero angles, so the device's distances are exact (knn5_ref's module docstring) and the comparison tolerates NOTHING: every query of
every case, in the production build and with "exact_arithmetic".

"canonical_ties" = 1: rows 0-4 of the neighbour dump equal the reference's five in (distance, original index) order and the found flag
(row 4 >= 0) is equal.  "canonical_ties" = 0 (first met wins among equals): the found flag is equal, the ids are distinct and valid, and
the sorted exact d2 of the returned points equals the reference's — any of the equals may stand in the tied places.
A query with FEWER than five points inside tau: row 4 is -1 and rows 0-3 hold exactly the points inside tau, ascending (a certified scan
has seen every point closer than sqrt(tau), the walk inserts every candidate below the bound), equals ordered by original index under
canonical ties (the dump orders them so: lisreg_assoc.hip, "dump_neighbors").  One difference to that reading is asserted as it stands: for a
target of fewer than five points the kernel leaves before it searches (`g.n < 5`) and the dump holds -1 in every row, which is what
include/lisreg.h promises ("-1 where fewer than five lie inside").

Every registration here runs with min_corr = 2^30, so that no Gauss-Newton step is solved (k_solve: solving = n_sel >= min_corr): the
pose stays T_init, later iterations search at it again (seeded walk, graph scan from last iteration's anchor, rows), and degenerate
planted clouds never reach the 6 x 6 solve."""
import numpy as np
import pytest

import knn5_ref as R

f32 = np.float32
BIG = 1 << 30


# ---------------------------------------------------------------- planted properties, from knn5_ref alone (CPU)
def _float32_distances(tgt, q, ref):
    """the squared distances of the reference's five, formed in float32 as the kernels form them"""
    t32, q32 = R.to_f32(tgt), R.to_f32(q)
    ok = ref["idx"] >= 0
    if len(t32) == 0:
        return np.zeros(ok.shape, f32), ok
    e = q32[:, None, :] - t32[np.where(ok, ref["idx"], 0)]
    d = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    assert d.dtype == f32
    return d, ok


def check_planted(name, tau=1.0):
    """the property case `name` was planted for still holds — asserted from knn5_ref's outputs alone, so that a GPU test whose input
    lost its point fails instead of passing empty"""
    c = R.case(name)
    refs = R.brute5(name, tau)
    q, g = c["queries"], c["groups"]
    tu = R.tau_units(tau)
    assert len(q) <= 4096 and all(len(t) <= 20000 for t in c["tgt"])
    assert all(len(v) > 0 for v in g.values()), [k for k, v in g.items() if len(v) == 0]
    assert np.abs(c["t"]).max() > 0 and tau in c["taus"]
    geoms = [R.grid_geometry(R.to_f32(t)) for t in c["tgt"]]
    for tgt, ref in zip(c["tgt"], refs):
        # every d2 below 4 m^2 survives the float32 round trip, and float32 arithmetic on the float32 coordinates gives exactly it
        d, ok = _float32_distances(tgt, q, ref)
        small = ok & (ref["d2"] < 4 * 4096)
        assert np.array_equal(d[small].astype(np.float64) * 4096.0, ref["d2"][small].astype(np.float64))
        assert np.all(d[ok & ~small] >= f32(4.0))
        if len(tgt) >= 50 and np.ptp(tgt[:, 0]) > 0:                    # original index is unrelated to position
            assert abs(np.corrcoef(np.arange(len(tgt)), tgt[:, 0])[0, 1]) < 0.2
    corner, surf = refs
    gs = geoms[1]
    if name == "lattice":
        assert gs["cell"] == f32(0.25) and geoms[0]["cell"] == f32(0.25) and gs["dims"] == (13, 13, 9)
        p = g["planted"]
        assert np.all(surf["ties5"][p] >= 2) and surf["found"][p].all()                    # a tie at the fifth / sixth place ...
        assert np.all((surf["d2"][p, 1:] == surf["d2"][p, :-1]).any(1))                    # ... and one inside the five
        assert np.all(surf["d2"][g["on"], 0] == 0) and np.all(surf["ties5"][g["on"]] == 6)
        assert np.all(surf["ties5"][g["body"]] == 8) and np.all(surf["ties5"][g["edge_x"]] == 8)
        qq = q[p] + 32                                                                   # (the grid's origin is 32 steps below the block)
        assert ((qq % 16 == 0).all(1)).sum() > 5 and ((qq % 16 == 0).any(1)).sum() > 50  # cell corners and cell faces
        assert ((qq % 16 == 8).any(1)).sum() > 50                                        # octant faces
        assert surf["found"][g["above"]].sum() >= 3 and not corner["found"][g["above"]].any()
        assert 0 < surf["found"][g["random"]].sum() < len(g["random"])
    elif name == "half":
        assert gs["cell"] == f32(0.5) and geoms[0]["cell"] == f32(0.5) and gs["dims"][2] == 5
        assert np.all(c["tgt"][1] % 32 == 0)                                             # every point on a cell corner
        other = {1.0: "2", 2.0: "1"}[tau]
        mine = {1.0: "1", 2.0: "2"}[tau]
        at, below, beside = g["at_tau_" + mine], g["below_tau_" + mine], g["beside_" + mine]
        assert np.all(surf["d2"][at, 4] == tu) and not surf["found"][at].any() and np.all(surf["n_in"][at] == 4)
        assert np.all(surf["ties5"][at] == 4)
        assert np.all(surf["d2"][below, 4] == tu - 2) and surf["found"][below].all()
        assert surf["found"][beside].all()
        # tu - 1 is no sum of three squares: tu - 2 IS the smallest step below tau
        s = np.arange(0, 92) ** 2
        sums = (s[:, None, None] + s[None, :, None] + s[None, None, :]).ravel()
        assert (tu - 1) not in sums and (tu - 2) in sums and (sums == tu).sum() in (3, 3 * 2)    # (64,0,0) x 3 orders / (64,64,0) x 3
        assert len(g["at_tau_" + other]) > 0
    elif name == "shell":
        assert gs["cell"] == f32(0.5) and np.array_equal(gs["o"], f32([-1, -1, -1])) and gs["dims"] == (21, 21, 9)
        want = dict(cell72=72, octant72=72, point72=72, cell48=48, cell64=64)
        for k, n_eq in want.items():
            centre = g[k][0]
            assert surf["ties5"][centre] == n_eq and surf["d2"][centre, 4] == 26, k
            assert corner["ties5"][centre] == n_eq // 2, k
        assert surf["d2"][g["point72"][0], 0] == 0
        cc, _ = R.shell_centres()["cell72"]
        oc, _ = R.shell_centres()["octant72"]
        assert np.all((cc + 64) % 32 == 16) and np.all((oc + 64) % 32 == 8)               # a cell centre, an octant centre
        assert surf["found"].all()
    elif name == "clusters":
        assert gs["cell"] == f32(0.5)
        assert not surf["found"][g["iso4"]].any() and np.all(surf["n_in"][g["iso4"]] == 4) and np.all(surf["d2"][g["iso4"], :4] == 0)
        assert surf["found"][g["iso5"]].all() and np.all(surf["d2"][g["iso5"]] == 0)
        assert not corner["found"][g["iso5"]].any() and np.all(corner["n_in"][g["iso5"]] == 4)
        assert np.all(surf["d2"][g["iso_at_tau"][3:], 4] == tu) and not surf["found"][g["iso_at_tau"]].any()
        assert surf["found"][g["iso_below_tau"][3:]].all() and not surf["found"][g["iso_below_tau"][:3]].any()
        assert set(R.CLUSTER_SIZES) >= {1, 4, 5, 64, 65, 200}
        _, counts = np.unique(c["tgt"][1], axis=0, return_counts=True)
        assert sorted(counts) == sorted(list(R.CLUSTER_SIZES) + [4, 4, 4, 5, 5, 5]) and (counts > R.GRAPH_K).sum() == 3
        assert R.in_minus2_cell(c["tgt"][1], q[g["empty"]], gs).all() and not R.minus2_shortcut_applies(gs, tau)
        assert np.all(surf["ties5"][g["on"]] >= 1) and surf["ties5"].max() >= 200
    elif name in R.FEW_SIZES:
        assert (len(c["tgt"][0]), len(c["tgt"][1])) == R.FEW_SIZES[name]
        for tgt, ref in zip(c["tgt"], refs):
            assert ref["found"].any() == (len(tgt) >= 5)
            assert np.array_equal((ref["idx"] >= 0).sum(1), np.full(len(q), min(5, len(tgt))))
    elif name == "one_cell":
        assert R.grid_geometry(R.to_f32(c["tgt"][1]), 0)["dims"] == (1, 1, 1) and gs["dims"] == (5, 5, 5)
    elif name == "plane":
        d0 = R.grid_geometry(R.to_f32(c["tgt"][1]), 0)["dims"]
        assert d0[2] == 1 and min(d0[:2]) > 1 and gs["dims"][2] == 5
    elif name == "line":
        d0 = R.grid_geometry(R.to_f32(c["tgt"][1]), 0)["dims"]
        assert d0[1:] == (1, 1) and d0[0] > 1 and gs["dims"][1:] == (5, 5) and gs["cell"] == f32(0.25)
    elif name == "outside":
        assert gs["cell"] == f32(0.5) and geoms[0]["cell"] == f32(0.5)
        lo = np.round(gs["o"].astype(np.float64) * 64).astype(np.int64); hi = lo + np.array(gs["dims"]) * 32
        assert lo.tolist() == [-64, -64, -64] and hi.tolist() == [608, 608, 224]
        gap = np.maximum(np.maximum(lo - q[g["far"]], q[g["far"]] - hi), 0).max(1)
        assert gap.min() == 64 and gap.max() == 500 * 64 and not surf["found"][g["far"]].any()
        qm = q[g["margin"]]
        assert np.all((qm >= lo) & (qm < hi)) and np.all((qm[:, 0] < 0) | (qm[:, 0] > 512))
        qf = q[g["faces"]][:9]
        assert np.all(((qf == lo) | (qf == hi)).any(1))
        assert surf["d2"][g["at_tau"][0], 4] == tu and surf["ties5"][g["at_tau"][0]] == 5 and surf["n_in"][g["at_tau"][0]] == 0
        assert q[g["at_tau"][0], 0] == lo[0]                                              # ... and it stands ON the grid's outer face
        assert surf["found"][g["below_tau"]].all() and surf["d2"][g["below_tau"][0], 4] == 63 * 63
    elif name == "grown":
        assert gs["cell"] > f32(0.5) and np.prod(gs["dims"]) <= (1 << 24)
        assert np.prod([np.floor((e + 2.0) / 0.5) + 1 for e in (200.0, 200.0, 250.0)]) > (1 << 24)
        assert float(gs["cell"]) * 64 != round(float(gs["cell"]) * 64)                    # cell faces are no lattice planes
        assert R.minus2_shortcut_applies(gs, tau) and R.in_minus2_cell(c["tgt"][1], q[g["empty"]], gs).all()
        assert not surf["found"][g["empty"]].any() and surf["found"][g["on"]].all()
        assert 0 < surf["found"][g["far"]].sum() + surf["found"][g["near"]].sum()
    elif name == "scene":
        assert f32(0.25) < gs["cell"] < f32(0.5), gs
        assert 0.3 * len(q) < surf["found"].sum() < len(q) and len(q) >= 2000
        assert (surf["ties5"] >= 2).sum() >= 1 and (surf["d2"][:, 1:] == surf["d2"][:, :-1]).any(1).sum() >= 10     # ties on their own
    return c, refs


RUNS = R.runs()
RUN_IDS = [f"{n}-tau{int(t)}" for n, t in RUNS]


@pytest.mark.parametrize("name,tau", RUNS, ids=RUN_IDS)
def test_planted_properties_hold(name, tau):
    check_planted(name, tau)


def test_ref_distances_match_ckdtree():
    """the five distances of brute5 against scipy's k-d tree (float64 on the same coordinates: exact for lattice points this close)"""
    from scipy.spatial import cKDTree
    for name in ("lattice", "clusters", "scene", "outside"):
        c = R.case(name)
        for tgt, ref in zip(c["tgt"], R.brute5(name)):
            d, _ = cKDTree(tgt.astype(np.float64)).query(c["queries"].astype(np.float64), k=5)
            want = np.where(ref["d2"] < R.INF, ref["d2"], -1).astype(np.float64)
            got = np.where(np.isfinite(d), np.round(d * d), -1)
            assert np.array_equal(got, want), name


def test_ref_indices_match_the_oracles_knn(oracle):
    """the oracle's k-d tree k-NN (oracle/lisreg_oracle.c) resolves equal distances by index: ids and float32 distances equal brute5's,
    place for place, on the clouds that are all ties"""
    import ctypes as C
    L = oracle.lib()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    for name in ("lattice", "shell", "clusters", "half"):
        c = R.case(name)
        q32 = R.to_f32(c["queries"])
        for tgt, ref in zip(c["tgt"], R.brute5(name)):
            t32 = np.ascontiguousarray(R.to_f32(tgt))
            tree = L.orc_kdtree_build(t32.ctypes.data_as(fp), len(t32), 15)
            try:
                idx = np.zeros(5, np.int32); sq = np.zeros(5, f32)
                for i in range(0, len(q32), 3):
                    qi = np.ascontiguousarray(q32[i])
                    k = L.orc_kdtree_knn(tree, qi.ctypes.data_as(fp), 5, idx.ctypes.data_as(ip), sq.ctypes.data_as(fp))
                    assert k == 5 and np.array_equal(idx, ref["idx"][i]), (name, i, idx, ref["idx"][i])
                    assert np.array_equal(sq.astype(np.float64) * 4096.0, ref["d2"][i].astype(np.float64)) or ref["d2"][i, 4] >= 1 << 24
            finally:
                L.orc_kdtree_free(tree)


# ---------------------------------------------------------------- GPU
def _pcl(lattice_xyz):
    from lisreg import synth
    return synth.to_pcl(R.to_f32(lattice_xyz))


def _pose(t):
    return np.concatenate([np.zeros(3), np.asarray(t, np.float64) / R.UNIT]).astype(f32)


def _params(tau, fixed_iters):
    import lisreg
    p = lisreg.default_params(1)
    p.knn_sq_thresh = tau; p.fixed_iters = fixed_iters
    p.edge_min = -1; p.surf_min = -1                                   # the feature-count guard passes whatever the query count
    p.min_corr = BIG                                                   # no step is ever solved: the pose stays T_init
    return p


def _columns_sorted(a):
    return a[:, np.lexsort(a)]


def compare(ids, tgt, q, ref, canonical, what, unordered=False):
    """one kind's dump ids [5, k] against its reference: nothing tolerated, nothing left out (module docstring).  unordered: the
    queries came back in another order — the columns are compared as a multiset."""
    k, n = len(q), len(tgt)
    assert ids.shape == (5, k), (what, ids.shape)
    found = ids[4] >= 0
    want = R.expected_dump(ref)
    if unordered:
        assert found.sum() == ref["found"].sum(), (what, "found flags", int(found.sum()), int(ref["found"].sum()))
        if canonical:
            assert np.array_equal(_columns_sorted(ids), _columns_sorted(want)), (what, "ids as a multiset")
            return
    else:
        bad = np.flatnonzero(found != ref["found"])
        assert bad.size == 0, (what, "found flag", bad[:8], ids[:, bad[:4]].T, ref["idx"][bad[:4]], ref["d2"][bad[:4]])
    if canonical:
        bad = np.flatnonzero((ids != want).any(0))
        assert bad.size == 0, (what, "ids", len(bad), bad[:8], ids[:, bad[:4]].T, want[:, bad[:4]].T, ref["d2"][bad[:4]])
        return
    assert ((ids >= -1) & (ids < n)).all(), (what, "invalid id")
    listed = ids >= 0
    assert (listed[:-1] | ~listed[1:]).all(), (what, "-1 in front of an id")
    srt = np.sort(np.where(listed, ids, -np.arange(1, 6)[:, None]), axis=0)
    assert (srt[1:] != srt[:-1]).all(), (what, "an id twice")
    if unordered:
        return                      # (first met wins AND an unknown order: no query to measure the ids from; the canonical run is the exact one)
    e = q[None, :, :] - (tgt[np.where(listed, ids, 0)] if n else np.zeros((5, k, 3), np.int64))
    d2 = np.sort(np.where(listed, (e ** 2).sum(-1), R.INF), axis=0)
    want_d2 = np.where(want >= 0, ref["d2"].T, R.INF)
    bad = np.flatnonzero((d2 != want_d2).any(0))
    assert bad.size == 0, (what, "distances", len(bad), bad[:8], d2[:, bad[:4]].T, want_d2[:, bad[:4]].T)


def compare_both(ids, c, refs, canonical, what):
    k = len(c["queries"])
    assert ids.shape == (5, 2 * k)
    for kind in (0, 1):
        compare(ids[:, kind * k:(kind + 1) * k], c["tgt"][kind], c["queries"], refs[kind], canonical, what + (R.KINDS[kind],))


def test_compare_rejects_what_it_must():
    """the comparison itself, on the lattice: the reference's own table passes under both tie settings; two tied places swapped pass
    only without canonical ties; a farther point in the fifth place, a missing fifth, an id twice and a dropped query fail under both"""
    c, refs = check_planted("lattice")
    tgt, q, ref = c["tgt"][1], c["queries"], refs[1]
    good = R.expected_dump(ref)
    for canonical in (1, 0):
        compare(good, tgt, q, ref, canonical, ("self", canonical))
    col = int(c["groups"]["on"][0])
    assert ref["d2"][col, 1] == ref["d2"][col, 2]

    def rejected(bad, canonical):
        try:
            compare(bad, tgt, q, ref, canonical, ("mutant", canonical))
        except AssertionError:
            return True
        return False
    swapped = good.copy(); swapped[[1, 2], col] = swapped[[2, 1], col]
    assert rejected(swapped, 1) and not rejected(swapped, 0)
    D = ((tgt - q[col]) ** 2).sum(1)
    sixth = int(np.flatnonzero((D == ref["d2"][col, 4]) & ~np.isin(np.arange(len(tgt)), good[:, col]))[0])
    tied = good.copy(); tied[4, col] = sixth                              # another of the equals in the fifth place
    assert rejected(tied, 1) and not rejected(tied, 0)
    farther = good.copy(); farther[4, col] = int(np.flatnonzero(D > ref["d2"][col, 4])[0])
    missing = good.copy(); missing[4, col] = -1
    twice = good.copy(); twice[4, col] = twice[3, col]
    nothing = good.copy(); nothing[:, col] = -1
    for bad in (farther, missing, twice, nothing):
        assert rejected(bad, 1) and rejected(bad, 0)
    short = np.flatnonzero(~ref["found"] & (ref["n_in"] > 0))               # a query with fewer than five: its short list counts too
    assert short.size > 0
    cut = good.copy(); cut[ref["n_in"][short[0]] - 1, short[0]] = -1
    assert rejected(cut, 1) and rejected(cut, 0)


def _expected_front_end(ctx, mode, n_src, n_tgt, bound):
    """plan_front_end (csrc/lisreg_batch_plan.hpp) restated for search_mode 4"""
    if mode != 4:
        return mode
    qi = float(n_src) * bound
    out = 3 if (n_tgt > 0 and qi >= float(ctx.get_option("graph_min_ratio")) * n_tgt) else 1
    if n_tgt > 0 and qi >= float(ctx.get_option("cell_min_ratio")) * n_tgt and n_tgt * 5120.0 <= float(ctx.get_option("cell_rows_max_mb")) * 1048576.0:
        out = 5
    return out


class Single:
    """one context with one planted case as its target; align() runs the queries as corner AND surf sources at a lattice translation"""

    def __init__(self, name, mode, lanes, opts=()):
        import lisreg
        self.c = R.case(name)
        self.mode, self.lanes = mode, lanes
        self.ctx = lisreg.Context(0)
        self.ctx.set_option("search_mode", mode); self.ctx.set_option("lanes_per_query", lanes); self.ctx.set_option("dump_neighbors", 1)
        for k, v in opts:
            self.ctx.set_option(k, v)
        self.ctx.set_target(_pcl(self.c["tgt"][0]), _pcl(self.c["tgt"][1]))

    def align(self, t, tau, fixed_iters, opts=()):
        c, ctx = self.c, self.ctx
        for k, v in opts:
            ctx.set_option(k, v)
        src = _pcl(c["queries"] - np.asarray(t, np.int64))
        T0 = _pose(t)
        T, st, tr = ctx.align(src, src, T0, _params(tau, fixed_iters))
        n_src, n_tgt = 2 * len(src), len(c["tgt"][0]) + len(c["tgt"][1])
        front = _expected_front_end(ctx, self.mode, n_src, n_tgt, fixed_iters)
        assert ctx.front_end() == front, (self.mode, ctx.front_end(), front)
        # "lanes_per_query" other than 1 means auto: the eight-lane walk has to be what the batch plan really took for this run
        assert ctx.get_option("lanes_per_query") == (8 if (front == 1 and self.lanes != 1) else 1), (self.mode, self.lanes)
        if front == 5:                                                 # the grid under the rows IS the one knn5_ref restates (the planted cell properties rest on it)
            for kind in (0, 1):
                if len(c["tgt"][kind]):
                    got, want = ctx.target_index(0, kind), R.grid_geometry(R.to_f32(c["tgt"][kind]))
                    assert (got["nx"], got["ny"], got["nz"]) == want["dims"] and f32(got["cell"]) == want["cell"], (got["cell"], want)
                    assert np.array_equal(got["origin"].astype(f32), want["o"]), (got["origin"], want["o"])
        # frozen pose: nothing solved, nothing moved, every iteration ran
        assert st["iters"] == fixed_iters and len(tr) == fixed_iters, (st, len(tr))
        assert np.array_equal(T, T0) and all(np.array_equal(row[49:55], T0) for row in tr), (T, T0, tr[:, 49:55])
        return ctx.neighbors(n_src)[:5].copy()

    def close(self):
        self.ctx.close()


# label -> (search_mode, lanes_per_query (0: auto), option sets to run one after the other in the same context)
FRONT_ENDS = {
    "walk1": (1, 1, [(), (("first_pass_mm", 0),), (("first_pass_mm", 2000),)]),
    "walk8": (1, 0, [(), (("first_pass_mm", 0),), (("first_pass_mm", 2000),)]),
    "graph": (3, 1, [()]),
    "rows": (5, 1, [()]),
    "auto": (4, 0, [(), (("cell_min_ratio", 0),), (("cell_min_ratio", BIG), ("graph_min_ratio", 0))]),
}


@pytest.mark.gpu
@pytest.mark.parametrize("front", list(FRONT_ENDS))
@pytest.mark.parametrize("name,tau", RUNS, ids=RUN_IDS)
def test_hip_single_align_returns_the_definitions_five(name, tau, front):
    """leg a: one lisreg_align with fixed_iters = 1 (GN iteration 0: no seeds, no anchors), at the zero pose and at a lattice
    translation, under both tie settings; the walk also at "first_pass_mm" 0 and 2000 (the eight-lane walk takes the radius-limited first
    pass at iteration 0) and the one-lane walk with "exact_arithmetic"; auto as it resolves by itself and pushed to the rows and the graph"""
    c, refs = check_planted(name, tau)
    mode, lanes, option_sets = FRONT_ENDS[front]
    s = Single(name, mode, lanes)
    try:
        for opts in option_sets:
            for canonical in (1, 0):
                for t in (np.zeros(3, np.int64), c["t"]):
                    ids = s.align(t, tau, 1, opts + (("canonical_ties", canonical),))
                    compare_both(ids, c, refs, canonical, (name, tau, front, opts, canonical, t.tolist()))
        if front == "walk1":
            for t in (np.zeros(3, np.int64), c["t"]):
                ids = s.align(t, tau, 1, (("first_pass_mm", 150), ("canonical_ties", 0), ("exact_arithmetic", 1)))
                assert s.ctx.get_option("exact_arithmetic") == 1
                compare_both(ids, c, refs, 1, (name, tau, "exact", t.tolist()))     # (the exact build resolves ties canonically)
    finally:
        s.close()


LATER = {"walk1": (1, 1, ()), "walk8": (1, 0, ()), "graph_anchor0": (3, 1, (("cell_anchor_until", 0),)),
         "graph_anchor1": (3, 1, (("cell_anchor_until", 1),)), "rows": (5, 1, ())}


@pytest.mark.gpu
@pytest.mark.parametrize("front", list(LATER))
@pytest.mark.parametrize("name,tau", RUNS, ids=RUN_IDS)
def test_hip_later_iterations_at_a_frozen_pose(name, tau, front):
    """leg b: fixed_iters = 3 with min_corr = 2^30 — iterations 1 and 2 search at T_init again, through the seeded walk, the graph scan
    from iteration 0's nearest neighbour (with and without the cell anchor) and the rows; the dump holds the last iteration.  Single.align
    asserts from the trace that the pose never moved and that three iterations ran."""
    c, refs = check_planted(name, tau)
    mode, lanes, opts = LATER[front]
    s = Single(name, mode, lanes, opts + (("count_searches", 1),))
    try:
        for canonical in (1, 0):
            for t in (np.zeros(3, np.int64), c["t"]):
                ids = s.align(t, tau, 3, (("canonical_ties", canonical),))
                compare_both(ids, c, refs, canonical, (name, tau, front, canonical, t.tolist()))
                if mode != 1 and max(len(x) for x in c["tgt"]) >= 5:
                    cnt = s.ctx.counters()
                    assert cnt[1:3, 1].sum() > 0, (name, front, cnt[:4])               # iterations 1 and 2 went through the scan
    finally:
        s.close()


# ---------------------------------------------------------------- leg c: batches
SHARED = ("lattice", "clusters", "shell", "outside")
OWN = ("lattice", "half", "shell", "clusters", "few45", "one_cell", "plane", "line", "outside", "grown")
SHIFTS = np.array([[0, 0, 0], [64, 0, 0], [0, -32, 0], [0, 0, 16], [1, 2, 3], [-7, 5, -3], [128, 128, 0], [-64, 64, -8], [3, 0, -1]], np.int64)
# label -> (search_mode, options, read-out that proves the leg engaged, its value)
BATCH_LEGS = {
    "rows_reach0": (5, (("row_reach", 0),), "row_reach_now", 0),
    "rows_reach1": (5, (("row_reach", 1),), "row_reach_now", 1),
    "rows_reach2": (5, (("row_reach", 2),), "row_reach_now", 1),
    "rows_capped": (5, (("cell_rows_max_mb", 1),), "front_end", 5),
    "graph_xcd": (3, (("xcd_order", 1),), "xcd_order_now", 1),
    "rows_interleaved": (5, (("interleave", 2), ("interleave_min_blocks", 4)), "interleaved_now", 1),
    "walk_interleaved": (1, (("interleave", 2), ("interleave_min_blocks", 4)), "interleaved_now", 1),
    "rows_sorted": (5, (("sort_sources", 1),), "sorted_now", 1),
}


# (only the lattice has more rows than one megabyte holds, and the capped leg asserts that rows were cut)
SHARED_LEGS = [(n, l) for n in SHARED for l in BATCH_LEGS if l != "rows_capped" or n == "lattice"]


def _context(front, opts=()):
    """the base settings of tests/test_option_state.py::_context, with the neighbour dump"""
    import lisreg
    c = lisreg.Context(0)
    c.set_option("search_mode", front); c.set_option("lanes_per_query", 1); c.set_option("interleave_min_blocks", 4)
    c.set_option("rebuild_targets_each_run", 1); c.set_option("dump_neighbors", 1)
    for k, v in opts:
        c.set_option(k, v)
    return c


def _run_batch(leg, plan):
    """plan: list of (case name, slot, shift).  Each item's queries go in as corner and as surf records, moved back by the item's own
    lattice translation, which its T_init undoes.  Both tie settings on one context; every (item, kind) segment against its reference."""
    import lisreg
    front, opts, readout, value = BATCH_LEGS[leg]
    for canonical in (1, 0):                                              # (a fresh context each: "row_reach" backs off after a run with misses)
        _run_batch_once(leg, plan, front, opts + (("canonical_ties", canonical),), readout, value, canonical)


def _run_batch_once(leg, plan, front, opts, readout, value, canonical):
    import lisreg
    ctx = _context(front, opts)
    keep = []
    try:
        slots = {}
        for name, slot, _ in plan:
            if slot not in slots:
                c = R.case(name)
                ctx.set_target(_pcl(c["tgt"][0]), _pcl(c["tgt"][1]), slot=slot)
                slots[slot] = name
        items, T0 = [], []
        for name, slot, shift in plan:
            rec = lisreg.pack_device_records(_pcl(R.case(name)["queries"] - shift))
            a, b = lisreg.DeviceArray(rec), lisreg.DeviceArray(rec)
            keep += [a, b]
            items.append(dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0], target=slot))
            T0.append(_pose(shift))
        T0 = np.array(T0, f32)
        n_src = sum(it["n_corner"] + it["n_surf"] for it in items)
        ctx.batch_prepare_device(items, T0, _params(1.0, 2))
        ctx.batch_run()
        T, st = ctx.batch_fetch()
        assert np.array_equal(T, T0) and all(s["iters"] == 2 for s in st), (leg, st)
        assert ctx.front_end() == front and ctx.get_option(readout) == value, (leg, readout, ctx.get_option(readout))
        if leg == "rows_capped":                                          # walkers and scanners share wavefronts
            assert any((ctx.target_cell_rows(s, k)["table"] == -1).any() for s in slots for k in (0, 1)), leg
        nb = ctx.neighbors(n_src)[:5]
        at = 0
        for i, (name, slot, shift) in enumerate(plan):
            c, refs = R.case(name), R.brute5(name)
            k = len(c["queries"])
            for kind in (0, 1):
                # a sorted batch keeps its segments in item order and orders the queries INSIDE each by tile: there the segment's
                # columns are compared with the reference's as a multiset (every query, nothing forgiven)
                compare(nb[:, at:at + k], c["tgt"][kind], c["queries"], refs[kind], canonical, (leg, canonical, i, name, R.KINDS[kind]),
                        unordered=leg == "rows_sorted")
                at += k
        assert at == n_src
    finally:
        ctx.close()
        for a in keep:
            a.free()


@pytest.mark.gpu
@pytest.mark.parametrize("name,leg", SHARED_LEGS, ids=[f"{n}-{l}" for n, l in SHARED_LEGS])
def test_hip_batch_of_nine_on_a_shared_target(name, leg):
    """leg c, shared target: nine items against one planted target in slot 0, each under its own lattice translation"""
    check_planted(name)
    _run_batch(leg, [(name, 0, SHIFTS[i]) for i in range(len(SHIFTS))])


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(BATCH_LEGS))
def test_hip_batch_of_own_targets(leg):
    """leg c, own targets: every item registers against its own planted case in its own slot"""
    for name in OWN:
        check_planted(name)
    _run_batch(leg, [(name, i, SHIFTS[i % len(SHIFTS)]) for i, name in enumerate(OWN)])
