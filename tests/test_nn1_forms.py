"""Every form of the exact k = 1 search (csrc/lisreg_nn1.hip) per query against brute force.

The search exists as the column walk nn1_search<Q> (Q = 1, 4, 8 lanes per query) and the flattened one-lane walk nn1_search_flat; the
ICP kernels hand either a seed that must never change the result.  `lisreg_test_nn1` runs ONE chosen form per query with a chosen seed;
tests/nn1_ref.py is the definition (brute force, float32, the lexicographic minimum of (d2, original index)) and holds the planted
clouds.  Every comparison is exact: indices equal, squared distances bit for bit wherever a point is found.

CPU: the definition against the oracle's k-d tree and scipy's, and every planted property the GPU tests rely on (ties are ties, the
runs end on every residue mod 4, the refill path of the flattened walk is reached, the grown cell, the distances that EQUAL a threshold).
GPU: all forms on all clouds at the caps 1e18, 3, 0.5 and 0; the cap itself; every seed choice; the production launchers at every
LISREG_NN1_Q; the dynamic filter at its three strict thresholds."""
import numpy as np
import pytest

import nn1_ref as R

f32 = np.float32
FORMS = (1, 4, 8, 0)                       # lanes of the column walk; 0 = the flattened walk
SEED_CASES = ("lattice", "duplicates", "scene")
SLOT = 90


def _pcl(xyz, intensity=None):
    from lisreg import synth
    return synth.to_pcl(np.ascontiguousarray(xyz, f32), intensity=intensity)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_found(got, want, what):
    """idx equal everywhere, d2 bit-equal wherever the point is found"""
    (gi, gd), (wi, wd) = got, want
    bad = np.flatnonzero(gi != wi)
    assert bad.size == 0, (what, "idx", bad[:8], gi[bad[:8]], wi[bad[:8]], gd[bad[:8]], wd[bad[:8]])
    f = wi >= 0
    badd = np.flatnonzero(_bits(gd)[f] != _bits(wd)[f])
    assert badd.size == 0, (what, "d2", badd[:8], gd[f][badd[:8]], wd[f][badd[:8]])


# ---------------------------------------------------------------- planted properties, from nn1_ref alone (CPU)
def check_planted(name, frame=None):
    """the property case `name` was planted for still holds — asserted from nn1_ref's outputs, so that a GPU test whose inputs lost
    it fails instead of passing empty (frame: the case moved into a map frame of tests/far_frame.py)"""
    c = R.case(name, frame)
    idx, d2, cnt, last = R.brute(name, frame)
    m, q, g = c["map"], c["queries"], c["groups"]
    assert len(m) <= 20000 and len(q) <= 4096
    geom = R.grid_geometry(m)
    if name == "scene":
        assert 0.25 <= geom["cell"] <= 0.5
        far = g["far"][np.argsort(d2[g["far"]])[-3:]]
        cols = [R.columns_in_last_pass(m, geom, q[i], d2[i]) for i in far]
        assert max(cols) > R.K_NN1_CAP, cols                          # the flattened walk has to refill its run list
        assert np.all(d2[g["on_map"]] == 0)
        for cap in R.CAPS:                                            # every cap splits the queries
            found = R.apply_cap(idx, d2, cap)[0] >= 0
            assert 0 < found.sum() and (cap == 1e18 or found.sum() < len(q)), cap
    elif name in ("lattice", "lattice2"):
        assert np.all(cnt >= 2) and np.all(last > idx)                # every minimum is attained by different points
        assert set(np.unique(cnt)) == set(g["tie_sizes"])
    elif name == "duplicates":
        sizes = g["sizes"]
        assert set(sizes) == set(range(1, 10))
        runs = R.cell_counts(m, geom)
        assert sorted(runs) == sorted(list(sizes) + [1])               # every cluster is a cell run of its own (+ the outlier)
        assert {int(r) % 4 for r in runs} == {0, 1, 2, 3}
        xy = np.array([m[mem[0], :2] for mem in g["members"]], np.float64)
        dist = np.sqrt(((xy[:, None] - xy[None]) ** 2).sum(-1)) + 1e9 * np.eye(len(xy))
        assert dist.min() >= 1.0
        lowest = np.array([mem.min() for mem in g["members"]])
        assert np.array_equal(idx, lowest[g["cluster_of_query"]])       # the winner is each cluster's lowest index
        assert np.array_equal(cnt, sizes[g["cluster_of_query"]])
        assert np.all(d2[: len(sizes)] == 0) and np.all(d2[len(sizes):] > 0)
        for mem in g["members"]:                                       # scattered original indices
            assert len(mem) < 3 or np.ptp(mem) > len(mem)
    elif name in ("one", "ident25"):
        assert geom["dims"] == (1, 1, 1)
    elif name == "plane":
        assert geom["dims"][2] == 1 and min(geom["dims"][:2]) > 1
    elif name == "line":
        assert geom["dims"][1:] == (1, 1) and geom["dims"][0] > 1
    elif name == "corners":
        assert geom["cell"] > 0.5 and np.prod(geom["dims"]) <= (1 << 24)
        assert np.prod([np.floor(e / 0.5) + 1 for e in (200.0, 200.0, 250.0)]) > (1 << 24)
    elif name == "nan_map":
        assert np.isnan(m[g["nan"]]).any(1).all() and not np.isin(idx, g["nan"]).any()
        # without its NaN each planted point WOULD be the answer of the query beside it
        spots = q[:3]
        for k, p in enumerate(g["nan"]):
            healed = m.copy(); healed[p] = spots[k]
            assert R.nearest(healed, q[[k, k + 3]])[0].tolist() == [p, p]
    elif name == "edges":
        lo = geom["o"].astype(np.float64); hi = lo + np.array(geom["dims"]) * float(geom["cell"])
        out = q[g["outside"]].astype(np.float64)
        gap = np.maximum(np.maximum(lo - out, out - hi), 0).max(1)
        assert np.all((gap > 0.99) & (gap < 501)) and gap.max() > 499
        assert np.all(idx[g["nan"]] == -1) and np.all(idx[g["outside"]] >= 0)
        assert np.array_equal(q[g["origin"][0]], geom["o"])
        assert np.array_equal(q[g["face"][0]], geom["o"] + np.array([3, 2, 1], f32) * geom["cell"])      # a corner of cell (3, 2, 1)
    elif name.startswith("count"):
        assert len(q) == int(name[5:])


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_planted_properties_hold(name):
    check_planted(name)


def test_ref_matches_oracle_on_the_scene(oracle):
    """d2 bit-equal everywhere; idx equal wherever the minimum is unique (the k-d tree's tie rule is another)"""
    c = R.case("scene")
    idx, d2, cnt, _ = R.brute("scene")
    o_idx, o_d2 = oracle.nearest(_pcl(c["map"]), _pcl(c["queries"]))
    assert np.array_equal(_bits(o_d2), _bits(d2))
    uniq = cnt == 1
    assert uniq.mean() > 0.9 and np.array_equal(o_idx[uniq], idx[uniq])
    for cap in R.CAPS[1:]:
        oi, od = oracle.nearest(_pcl(c["map"]), _pcl(c["queries"]), cap)
        ri, rd = R.apply_cap(idx, d2, cap)
        assert np.array_equal(oi >= 0, ri >= 0)
        assert np.array_equal(_bits(od)[ri >= 0], _bits(rd)[ri >= 0])


def test_ref_matches_ckdtree_within_one_ulp():
    from scipy.spatial import cKDTree
    c = R.case("scene")
    _, d2, _, _ = R.brute("scene")
    m, q = c["map"], c["queries"]
    _, t_idx = cKDTree(m.astype(np.float64)).query(q.astype(np.float64), k=1)
    e = q - m[t_idx]
    t_d2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]     # the tree's point, measured in float32
    assert t_d2.dtype == f32
    assert np.all(d2 <= t_d2)                                           # brute force found nothing farther
    assert np.abs(_bits(d2).astype(np.int64) - _bits(t_d2).astype(np.int64)).max() <= 1


def test_ref_tie_rule_on_the_lattice():
    """Integer arithmetic (the lattice in units of 1/8 m) names every tied set; the definition must return its smallest index."""
    for name in ("lattice", "lattice2"):
        c = R.case(name)
        idx, d2, cnt, last = R.brute(name)
        mi = np.round(c["map"].astype(np.float64) * 8).astype(np.int64)
        qi = np.round(c["queries"].astype(np.float64) * 8).astype(np.int64)
        assert np.array_equal(mi / 8.0, c["map"]) and np.array_equal(qi / 8.0, c["queries"])
        D = ((qi[:, None, :] - mi[None, :, :]) ** 2).sum(-1)
        tied = D == D.min(1, keepdims=True)
        assert np.array_equal(idx, tied.argmax(1)) and np.array_equal(cnt, tied.sum(1))
        assert np.array_equal(last, len(mi) - 1 - tied[:, ::-1].argmax(1))
        assert np.array_equal(d2.astype(np.float64), D.min(1) / 64.0)


def _threshold_clouds():
    c = R.case("thresholds")
    return c, _pcl(c["map"]), _pcl(c["queries"], intensity=np.arange(len(c["queries"]), dtype=f32))


THRESHOLD_SETS = [(0.5, 1.0), (0.5, R.FLT_MAX), (R.FLT_MAX, 1.0), (R.FLT_MAX, R.FLT_MAX)]


def check_threshold_cloud():
    c = R.case("thresholds")
    T, g = R.THRESHOLDS, c["groups"]
    m, q = c["map"], c["queries"]
    idx, d2, _, _ = R.brute("thresholds")
    sq = dict(near=f32(T["near"]) * f32(T["near"]), dmin=f32(T["dmin"]) * f32(T["dmin"]), dmax=f32(T["dmax"]) * f32(T["dmax"]))
    for name, v in sq.items():
        assert np.all(d2[g["exact"][name]] == v), name                   # d2 EQUALS the threshold
        assert np.all(d2[g["below"][name]] < v) and np.all(d2[g["above"][name]] > v), name
        assert len(g["exact"][name]) == 9
    r2 = q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]
    cr2 = f32(T["center_radius"]) * f32(T["center_radius"])
    assert r2[g["on_radius"][0]] == cr2 and r2[g["off_radius"][0]] > cr2 and np.all(r2[g["cases"]] < cr2)
    assert sq["dmin"] < d2[g["on_radius"][0]] < sq["dmax"]               # dropped only if it goes through the search
    assert d2[g["lonely"][0]] > 25 and r2[g["lonely"][0]] < cr2          # nothing within the largest finite threshold: keep_far
    assert np.all(r2[g["pad"]] > cr2) and len(g["pad"]) > 10
    mm = m.astype(np.float64)
    assert min(np.linalg.norm(mm[i] - mm[j]) for i in range(len(mm)) for j in range(i)) >= 8
    keeps = {}
    for dmin, dmax in THRESHOLD_SETS:
        keep = R.dynamic_keep(m, q, T["center_radius"], dmin, dmax, T["near"])
        assert keep[g["pad"]].all() and keep[g["off_radius"][0]]            # the pad is kept either way ...
        assert np.array_equal(keep[: len(q) - len(g["pad"])], R.dynamic_keep(m, q[: len(q) - len(g["pad"])], T["center_radius"], dmin, dmax, T["near"]))   # ... and touches no case
        assert 0 < keep[g["cases"]].sum() < len(g["cases"])
        keeps[(dmin, dmax)] = keep
    k = keeps[(0.5, 1.0)]                                                  # strict on both sides of every threshold
    assert not k[g["exact"]["near"]].any() and not k[g["below"]["near"]].any() and k[g["above"]["near"]].all()
    assert k[g["below"]["dmin"]].all() and not k[g["exact"]["dmin"]].any() and not k[g["above"]["dmin"]].any()
    assert not k[g["below"]["dmax"]].any() and not k[g["exact"]["dmax"]].any() and k[g["above"]["dmax"]].all()
    assert not k[g["on_radius"][0]]
    lonely = [bool(keeps[s][g["lonely"][0]]) for s in THRESHOLD_SETS]
    assert lonely == [True, False, True, True]                            # keep_far takes both values
    return keeps


def test_ref_dynamic_keep_matches_oracle_on_the_threshold_cloud(oracle):
    keeps = check_threshold_cloud()
    c, mc, qc = _threshold_clouds()
    T = R.THRESHOLDS
    for (dmin, dmax), keep in keeps.items():
        want, applied = oracle.dynamic_filter(mc, qc, T["center_radius"], dmin, dmax, T["near"])
        assert applied
        assert np.array_equal(want["intensity"], np.flatnonzero(keep).astype(f32)), (dmin, dmax)
    assert R.dynamic_keep(c["map"][:0], c["queries"], 40.0, 0.5, 1.0, 0.25).all()      # an empty map keeps everything


def test_seed_partners_are_real():
    """the lattice and the duplicates give every seed test a tied partner with a higher index than the answer"""
    for name in ("lattice", "lattice2"):
        idx, _, cnt, last = R.brute(name)
        assert np.all(last > idx)
    idx, _, cnt, last = R.brute("duplicates")
    assert (last > idx).sum() >= len(idx) * 8 // 9 and np.array_equal(last > idx, cnt > 1)
    for name in SEED_CASES:                                               # (the far seed really is 20 m off, here as on the GPU)
        assert len(_seed_choices(name)) == 7


# ---------------------------------------------------------------- GPU
def _same_grid(gpu_ctx, m, slot=SLOT):
    """the grid the library built IS the one nn1_ref.grid_geometry restates (the planted-property assertions rest on it)"""
    got, want = gpu_ctx.map_grid(slot), R.grid_geometry(m)
    assert got["n"] == len(m) and got["dims"] == want["dims"] and got["n_cells"] == int(np.prod(want["dims"])), (got, want)
    assert np.array_equal(got["o"], want["o"]) and got["cell"] == want["cell"], (got, want)


def _seed_choices(name, frame=None):
    """name -> seeds[k] (original indices; -1 none, -2 the cell seed).  The answer is by definition the LOWEST index of its tied set, so
    'a tied point with a lower index' is the answer itself; the partner with a higher index is the tied set's highest."""
    c = R.case(name, frame)
    idx, d2, cnt, last = R.brute(name, frame)
    m, q = c["map"], c["queries"]
    k, n = len(q), len(m)
    if "far" in c["groups"] and name != "scene":
        far = np.full(k, c["groups"]["far"][0], np.int32)                 # the outlier 20 m off
    else:                                                                 # the scene: some point of the opposite end of the map
        order = np.argsort(m[:, 0])
        far = np.where(q[:, 0] < np.median(m[:, 0]), order[-1 - np.arange(k) % 50], order[np.arange(k) % 50]).astype(np.int32)
    e = (q - m[far]).astype(np.float64)
    assert np.all(np.sqrt((e * e).sum(1)) > 20.0), name
    # (the seed "farther than the cap" is `far` in the run at cap 0.5)
    return dict(none=np.full(k, -1, np.int32), cell=np.full(k, -2, np.int32), answer=idx.astype(np.int32),
                tied_higher=last.astype(np.int32), far=far, n_map=np.full(k, n, np.int32), two_to_30=np.full(k, 2 ** 30, np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_hip_every_form_matches_the_definition(gpu_ctx, name, form):
    check_planted(name)
    c = R.case(name)
    idx, d2, _, _ = R.brute(name)
    gpu_ctx.map_index_set(SLOT, _pcl(c["map"]))
    _same_grid(gpu_ctx, c["map"])
    for cap in R.CAPS:
        got = gpu_ctx.test_nn1(SLOT, c["queries"], cap, form)
        _same_found(got, R.apply_cap(idx, d2, cap), (name, form, cap))
        miss = got[0] < 0
        assert np.all(_bits(got[1])[miss] == _bits(R.not_found_d2(cap))), (name, form, cap)     # as lisreg_nearest documents


@pytest.mark.gpu
def test_hip_the_cap_is_exact(gpu_ctx):
    """d2 == max_dist^2 is found, one float less of max_dist is not; at max_dist = 0 (the search's bound is then a denormal) only a
    coincident point is found."""
    below = float(np.nextafter(f32(0.75), f32(0)))
    origin, q0 = np.zeros((1, 3), f32), np.array([[0.75, 0, 0], [0, 0, 0]], f32)
    # "One float away" is taken at a point at x = 0.75: next to the ORIGIN the neighbouring floats are denormals, whose squares are 0.
    off, q1 = np.array([[0.75, 0, 0]], f32), np.array([[0.75, 0, 0], [np.nextafter(f32(0.75), f32(1)), 0, 0], [below, 0, 0]], f32)
    expect = {}
    for tag, m, q in (("origin", origin, q0), ("off", off, q1)):
        for cap in (0.75, below, 0.0):
            expect[(tag, cap)] = R.nearest(m, q, cap)
    assert expect[("origin", 0.75)][0].tolist() == [0, 0] and expect[("origin", 0.75)][1][0] == f32(0.5625)
    assert expect[("origin", below)][0].tolist() == [-1, 0] and expect[("origin", 0.0)][0].tolist() == [-1, 0]
    assert expect[("off", 0.0)][0].tolist() == [0, -1, -1] and np.all(expect[("off", 0.0)][1][1:] > 0)
    for tag, m, q in (("origin", origin, q0), ("off", off, q1)):
        gpu_ctx.map_index_set(SLOT, _pcl(m))
        runs = [(lambda cap, f=f: gpu_ctx.test_nn1(SLOT, q, cap, f)) for f in FORMS] + [lambda cap: gpu_ctx.nearest(SLOT, _pcl(q), cap)]
        for k, run in enumerate(runs):
            for cap in (0.75, below, 0.0):
                got = run(cap)
                _same_found(got, expect[(tag, cap)], (tag, k, cap))
                miss = got[0] < 0
                assert np.all(_bits(got[1])[miss] == _bits(R.not_found_d2(cap))), (tag, k, cap)      # at cap 0: the smallest denormal
    assert _bits(R.not_found_d2(0.0)) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("form", (0, 4))
@pytest.mark.parametrize("name", SEED_CASES)
def test_hip_the_seed_never_changes_the_result(gpu_ctx, name, form):
    check_planted(name)
    c = R.case(name)
    idx, d2, cnt, last = R.brute(name)
    if name != "scene":
        assert (last > idx).any()
    gpu_ctx.map_index_set(SLOT, _pcl(c["map"]))
    seeds = _seed_choices(name)
    for cap in (1e18, 0.5):                                                # at 0.5 the far seed lies beyond the cap
        want = R.apply_cap(idx, d2, cap)
        plain = gpu_ctx.test_nn1(SLOT, c["queries"], cap, form)
        _same_found(plain, want, (name, form, cap, "no seeds"))
        for kind, s in seeds.items():
            got = gpu_ctx.test_nn1(SLOT, c["queries"], cap, form, s)
            assert np.array_equal(got[0], plain[0]) and np.array_equal(_bits(got[1]), _bits(plain[1])), (name, form, cap, kind)


@pytest.mark.gpu
def test_hip_production_launchers_run_every_lane_count(gpu_ctx, monkeypatch):
    """LISREG_NN1_Q = 1, 4, 8: k_nn1<Q> against the definition, k_dynamic_flags<Q> with the same survivors (the definition's)"""
    for name in ("lattice", "scene"):
        check_planted(name)
        c = R.case(name)
        idx, d2, _, _ = R.brute(name)
        mc = _pcl(c["map"])
        qc = _pcl(c["queries"], intensity=np.arange(len(c["queries"]), dtype=f32))
        gpu_ctx.map_index_set(SLOT, mc)
        keep = R.dynamic_keep(c["map"], c["queries"], 30.0, 0.3, 1.0, 0.05)
        assert name == "lattice" or 0 < keep.sum() < len(keep)
        for lanes in ("1", "4", "8"):
            monkeypatch.setenv("LISREG_NN1_Q", lanes)
            for cap in R.CAPS:
                _same_found(gpu_ctx.nearest(SLOT, qc, cap), R.apply_cap(idx, d2, cap), (name, lanes, cap))
            got, applied = gpu_ctx.dynamic_filter(SLOT, qc, 30.0, 0.3, 1.0, 0.05)
            assert applied and np.array_equal(got["intensity"], np.flatnonzero(keep).astype(f32)), (name, lanes)
        monkeypatch.delenv("LISREG_NN1_Q")


@pytest.mark.gpu
def test_hip_dynamic_filter_at_its_thresholds(gpu_ctx, monkeypatch):
    keeps = check_threshold_cloud()
    c, mc, qc = _threshold_clouds()
    T = R.THRESHOLDS
    gpu_ctx.map_index_set(SLOT, mc)
    _same_grid(gpu_ctx, c["map"])
    for lanes in (None, "1", "4"):
        if lanes:
            monkeypatch.setenv("LISREG_NN1_Q", lanes)
        for (dmin, dmax), keep in keeps.items():
            got, applied = gpu_ctx.dynamic_filter(SLOT, qc, T["center_radius"], dmin, dmax, T["near"])
            want = qc[keep]
            assert applied and len(got) == len(want), (dmin, dmax, lanes, got["intensity"], want["intensity"])
            assert all(np.array_equal(got[f], want[f]) for f in want.dtype.names), (dmin, dmax, lanes)
    monkeypatch.delenv("LISREG_NN1_Q")


@pytest.mark.gpu
def test_hip_test_nn1_argument_errors(gpu_ctx):
    import lisreg
    q = np.zeros((3, 3), f32)
    gpu_ctx.map_index_set(SLOT, _pcl(np.ones((5, 3), f32)))
    with pytest.raises(lisreg.LisregError):
        gpu_ctx.test_nn1(12345, q, 1.0, 4)                                 # no map in the slot
    for form in (2, 3, 5, 16, -1):
        with pytest.raises(lisreg.LisregError):
            gpu_ctx.test_nn1(SLOT, q, 1.0, form)
    for md in (-1.0, float("nan")):
        with pytest.raises(lisreg.LisregError):
            gpu_ctx.test_nn1(SLOT, q, md, 4)
    L, h = lisreg.lib(), gpu_ctx._h
    import ctypes as C
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    assert L.lisreg_test_nn1(h, SLOT, q.ctypes.data_as(fp), 3, 1.0, 4, None, None, None) == lisreg.ERR_ARG      # NULL outputs
    assert L.lisreg_test_nn1(h, SLOT, None, 0, 1.0, 4, None, None, None) == lisreg.OK                            # n = 0 touches nothing
    i, d = gpu_ctx.test_nn1(SLOT, q[:0], 1.0, 0)
    assert len(i) == 0 and len(d) == 0
    gpu_ctx.map_index_set(SLOT, _pcl(np.ones((0, 3), f32)))                # an empty map: nothing found, whatever the seed
    for form in FORMS:
        i, _ = gpu_ctx.test_nn1(SLOT, q, 1e18, form, np.array([-2, 0, 7], np.int32))
        assert i.tolist() == [-1, -1, -1]
