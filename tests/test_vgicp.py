"""lisreg_vgicp_*: VGICP registration on the GPU (lis-slam_amd/csrc/lisreg_vgicp.hip) against its definition, tests/vgicp_ref.py.

The distributions of the scene and of a planted cloud, the voxels, one linearisation, whole alignments, a source without a pair, the
argument errors, device memory, a caller's busy stream.  The CPU side (the restatement against itself, the structs, the golden file) is
tests/test_vgicp_ref.py.

The bounds (set where the feature was specified; every test prints its figures before it asserts):
  neighbour rows   equal, all of them, on the scene (no 20 / 21 gap of the scene is below 3e-6: tests/test_vgicp_ref.py); on the planted
                   cloud wherever the restatement's gap is >= 1e-6, and by the tie rule among the identical points;
  cov6             within 1e-9 absolute (entries <= 1; Jacobi's error is of the order eps / gap with gap >= 7e-3, about 1e-13);
  voxels           ids and counts equal, means within 1e-12 max|coordinate|, cov6 within 1e-9;
  the 28 sums      each within 1e-10 of the restatement's sum of |term|, pair counts equal, two calls bit-identical;
  alignments       converged, iters, n_evals, n_rejected equal, final_transform within 1e-6 entry-wise.  Only cases whose smallest
                   rho-sign and convergence margins exceed 1e-6 in the restatement are used (checked on the CPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import vgicp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "vgicp", "vgicp_cases.npz")
SLOT = 11
K = 20


def _pcl(xyz):
    from lisreg import synth
    return synth.to_pcl(np.ascontiguousarray(xyz, np.float32))


def _records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def _sym(c6):
    C3 = np.zeros((len(c6), 3, 3))
    C3[:, 0, 0], C3[:, 0, 1], C3[:, 0, 2], C3[:, 1, 1], C3[:, 1, 2], C3[:, 2, 2] = c6.T
    C3[:, 1, 0], C3[:, 2, 0], C3[:, 2, 1] = c6[:, 1], c6[:, 2], c6[:, 4]
    return C3


@pytest.fixture(scope="module")
def world():
    """the scene, its restatement target and source and the golden file: made once, read by every test, never changed"""
    W = dict(R.world())
    W["g"] = np.load(GOLDEN)
    return W


@pytest.fixture(scope="module")
def scene_slot(gpu_ctx, world):
    import lisreg
    return gpu_ctx.vgicp_set_target(SLOT, _pcl(world["tgt"]), lisreg.vgicp_default_params())


@pytest.mark.gpu
def test_distributions_of_the_scene(gpu_ctx, world):
    import lisreg
    for what, xyz, D in (("target", world["tgt"], world["T"]["dist"]), ("source", world["src"], world["S"]["dist"])):
        cov, nbr = gpu_ctx.vgicp_covariances(_pcl(xyz), K)
        assert D["gap"].min() >= 1e-6 and np.nanmin(D["eig_gap"]) >= 1e-3, what
        err = np.abs(cov - R.cov6(D["C"])).max()
        print(f"[vgicp] distributions of the scene's {what}: {len(xyz)} points, rows differing {(nbr != D['nbr']).any(1).sum()}, worst cov6 error {err:.3e}")
        assert np.array_equal(nbr, D["nbr"]), what
        assert err <= 1e-9, (what, err)
        d = lisreg.DeviceArray(_records(xyz))                 # device records: the same bits
        cov_d, nbr_d = gpu_ctx.vgicp_covariances((d.ptr, len(xyz)), K)
        assert cov_d.tobytes() == cov.tobytes() and np.array_equal(nbr_d, nbr), what
    assert np.array_equal(world["T"]["dist"]["nbr"].sum(1)[::8], world["g"]["scene_nbr_sum"])


@pytest.mark.gpu
def test_distributions_of_the_planted_cloud(gpu_ctx):
    """a cluster whose neighbours lie across 30 m of empty cells, a coplanar patch, a collinear run, 25 identical points, NaN points"""
    xyz, groups = R.planted_cloud()
    D = R.distributions(xyz, R.params())
    cov, nbr = gpu_ctx.vgicp_covariances(_pcl(xyz), K)
    fin = D["nbr"][:, 0] >= 0
    assert set(np.flatnonzero(~fin)) == set(groups["nan"])
    assert np.isnan(cov[~fin]).all() and (nbr[~fin] == -1).all()
    sure = fin & (D["gap"] >= 1e-6)
    assert sure[groups["base"]].all() and sure[groups["cluster"]].all() and sure[groups["coplanar"]].all()
    assert np.array_equal(nbr[sure], D["nbr"][sure])
    # the cluster's rows: its own ten points, then ten from 30 m away
    far = D["nbr"][groups["cluster"]]
    assert all(np.isin(row, groups["cluster"]).sum() == 10 for row in far)
    # the tie rule: every one of the 25 identical points has the 20 lowest indices of the group, in ascending order
    want = np.sort(groups["identical"])[:K]
    assert all(np.array_equal(nbr[i], want) for i in groups["identical"])
    # every finite point: symmetric by construction (six entries), eigenvalues (1e-3, 1, 1) whatever normal a degenerate neighbourhood gave
    ev = np.linalg.eigvalsh(_sym(cov[fin]))
    e_eig = np.abs(ev - np.array([1e-3, 1.0, 1.0])).max()
    # the values: on exactly the points with a defined normal, which are all points outside the collinear and the identical group
    defined = fin & (D["eig_gap"] >= 1e-3)
    outside = fin.copy()
    outside[groups["collinear"]] = False
    outside[groups["identical"]] = False
    assert np.array_equal(defined, outside)
    e_cov = np.abs(cov[defined] - R.cov6(D["C"][defined])).max()
    print(f"[vgicp] planted cloud: {fin.sum()} finite points, {sure.sum()} rows above the gap bar, worst eigenvalue error {e_eig:.3e}, "
          f"worst cov6 error on the {defined.sum()} points with a defined normal {e_cov:.3e}")
    assert e_eig <= 1e-9 and e_cov <= 1e-9
    # the cell edge of the search grid does not matter
    for edge in (0.37, 1.9):
        cov_e, nbr_e = gpu_ctx.vgicp_covariances(_pcl(xyz), K, cell_edge=edge)
        assert np.array_equal(nbr_e, nbr) and cov_e.tobytes() == cov.tobytes(), edge


@pytest.mark.gpu
@pytest.mark.parametrize("n", [20, 21, 64, 65])
def test_distributions_of_small_clouds(gpu_ctx, n):
    xyz = R.small_cloud(n)
    D = R.distributions(xyz, R.params())
    cov, nbr = gpu_ctx.vgicp_covariances(_pcl(xyz), K)
    sure = D["gap"] >= 1e-6
    assert np.array_equal(nbr[sure], D["nbr"][sure]) and sure.sum() >= n - 2
    if n == K:                                               # every point has all points as neighbours
        assert sure.all() and all(sorted(row) == list(range(n)) for row in nbr)
    assert np.nanmin(D["eig_gap"]) >= 1e-3
    err = np.abs(cov - R.cov6(D["C"])).max()
    print(f"[vgicp] {n} points: worst cov6 error {err:.3e}")
    assert err <= 1e-9


@pytest.mark.gpu
def test_voxels_of_the_scene(gpu_ctx, world, scene_slot):
    T, g = world["T"], world["g"]
    assert scene_slot == dict(dims=[int(v) for v in T["dims"]], n_voxels=1821, n_points=25401)
    V = gpu_ctx.vgicp_get_voxels(SLOT)
    assert np.array_equal(V["cell_ids"], T["cell_ids"]) and np.array_equal(V["counts"], T["counts"])
    e_mean = np.abs(V["means"] - T["means"]).max() / np.abs(world["tgt"]).max()
    e_cov = np.abs(V["cov6"] - R.cov6(T["covs"])).max()
    print(f"[vgicp] voxels of the scene: {len(T['cell_ids'])}, mean error / max|coordinate| {e_mean:.3e}, cov6 error {e_cov:.3e}")
    assert e_mean <= 1e-12 and e_cov <= 1e-9
    assert np.array_equal(V["cell_ids"], g["scene_cell_ids"]) and np.array_equal(V["counts"], g["scene_counts"])
    assert np.abs(V["cov6"][::8] - g["scene_cov6"]).max() <= 1e-9
    assert {True, False} == set((T["counts"] > 48).tolist())            # the lane and the wavefront form


@pytest.mark.gpu
def test_voxels_with_nan_points_and_device_records(gpu_ctx):
    import lisreg
    xyz, groups = R.planted_cloud()
    T = R.build_target(xyz, R.params())
    for fmt in ("host", "device"):
        if fmt == "host":
            info = gpu_ctx.vgicp_set_target(SLOT + 1, _pcl(xyz), lisreg.vgicp_default_params())
        else:
            d = lisreg.DeviceArray(_records(xyz))
            info = gpu_ctx.vgicp_set_target(SLOT + 1, (d.ptr, len(xyz)), lisreg.vgicp_default_params())
        assert info == dict(dims=[int(v) for v in T["dims"]], n_voxels=len(T["cell_ids"]), n_points=len(xyz) - len(groups["nan"])), fmt
        V = gpu_ctx.vgicp_get_voxels(SLOT + 1)
        assert np.array_equal(V["cell_ids"], T["cell_ids"]) and np.array_equal(V["counts"], T["counts"]), fmt
        assert np.abs(V["means"] - T["means"]).max() <= 1e-12 * np.nanmax(np.abs(xyz)), fmt
        # the mean covariance of a voxel is compared where every point in it has a defined normal
        low = np.flatnonzero(~(T["dist"]["eig_gap"] >= 1e-3) & (T["dist"]["nbr"][:, 0] >= 0))
        cells, _, _ = R.NR.voxel_cells(xyz, 1.0)
        clean = ~np.isin(T["cell_ids"], cells[low])
        assert clean.sum() > 100 and np.abs(V["cov6"][clean] - R.cov6(T["covs"])[clean]).max() <= 1e-9, fmt


@pytest.mark.gpu
def test_one_linearisation(gpu_ctx, world, scene_slot):
    import lisreg
    g, src = world["g"], world["src"]
    P = lisreg.vgicp_default_params()
    k, worst = 0, 0.0
    cut = {n: R.prepare_source(src[:n], R.params()) for n in R.LIN_SIZES if n >= K}
    # a source of one point has no distribution (fewer points than k are refused), so the one-pair case is a source of k points of
    # which one lies on the map: the others are 200 m above it, spread out so that the one point's normal stays well defined
    one = src[:K].copy()
    one[1:] = one[0] + (one[1:] - one[0]) * np.float32([50, 50, 1]) + np.float32([0, 0, 200])
    cut[1] = R.prepare_source(one, R.params())
    # (the 1e-10 bar on the sums stands on normals defined to 1e-13: eigen-gaps of 1e-3 and more, as on the whole source)
    assert all(S["dist"]["eig_gap"].min() >= 1e-3 and S["dist"]["gap"].min() >= 1e-6 for S in cut.values())
    for ip, T in enumerate(g["lin_T"]):
        for n in R.LIN_SIZES:
            cloud = one if n == 1 else src[: n or len(src)]
            m = len(cloud)
            d_src = lisreg.DeviceArray(_records(cloud))
            for hess in (1, 0):
                want, wabs, wpairs = g["lin_out"][k], g["lin_abs"][k], int(g["lin_pairs"][k])
                k += 1
                if n == 1:
                    with pytest.raises(lisreg.LisregError):
                        gpu_ctx.vgicp_linearize(SLOT, _pcl(src[:1]), P, T, bool(hess))
                # the golden sums of a cut source are of its points with the WHOLE source's distributions; cut to n points it has other
                # neighbourhoods, so the restatement is asked for the cut source
                if n:
                    ev = R.linearize(world["T"], cut[n], T, bool(hess))
                    want, wabs, wpairs = ev["out"], ev["abs"], ev["n_pairs"]
                    assert wpairs == (1 if n == 1 else wpairs) or ip == 2
                out, pairs = gpu_ctx.vgicp_linearize(SLOT, _pcl(cloud), P, T, bool(hess))
                again, _ = gpu_ctx.vgicp_linearize(SLOT, (d_src.ptr, m), P, T, bool(hess))
                assert pairs == wpairs, (ip, m, hess)
                assert out.tobytes() == again.tobytes(), (ip, m, hess, "two calls (host structs, device records) differ")
                err = np.abs(out - want)
                assert np.all(err <= 1e-10 * wabs), (ip, m, hess, err, wabs)
                if not hess:
                    assert not out[7:].any()
                if wpairs:
                    worst = max(worst, float(np.max(err[wabs > 0] / wabs[wabs > 0])))
                else:
                    assert not out.any() and ip == 2
    print(f"[vgicp] one linearisation: worst |sum - restatement| / sum|term| over {k} cases {worst:.3e}")
    assert k == len(g["lin_out"])


def _apply_f32(F, xyz):
    """transformPointCloud in float, products and sums rounded one by one (lisreg_transform_cloud)"""
    F = np.asarray(F, np.float32)
    x, y, z = (np.asarray(xyz[:, k], np.float32) for k in range(3))
    return np.stack([((F[r, 0] * x + F[r, 1] * y) + F[r, 2] * z) + F[r, 3] for r in range(3)], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(R.ALIGN_CASES)))
def test_alignment_equals_the_restatement(gpu_ctx, world, scene_slot, case):
    import lisreg
    seed, trans, rot, eps = R.ALIGN_CASES[case]
    g = world["g"]
    counts, want = g["align_counts"][case], g["align_T"][case]
    tgt, src, guess, T_true = (world[k] for k in ("tgt", "src", "guess", "T_true")) if seed == 1000 else R.scene(seed, trans, rot)
    slot = SLOT
    if seed != 1000:
        slot = SLOT + 2
        gpu_ctx.vgicp_set_target(slot, _pcl(tgt), lisreg.vgicp_default_params())
    P = lisreg.vgicp_default_params(transformation_epsilon=eps)
    cloud = _pcl(src)
    r = gpu_ctx.vgicp_align(slot, cloud, P, guess, want_aligned=True)
    dT = np.abs(r["T"] - want).max()
    et, er = R.pose_error(r["T"], T_true)
    print(f"[vgicp] align seed {seed} eps {eps}: converged {r['converged']} iters {r['iters']} evals {r['n_evals']} rejected {r['n_rejected']} "
          f"|dT| {dT:.3e}, {1e3 * et:.2f} mm / {1e3 * er:.3f} mrad from the truth")
    assert (int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"]) == tuple(int(v) for v in counts[:5])
    assert dT <= 1e-6, dT
    assert abs(r["error"] - g["align_fig"][case][0]) <= 1e-6 * g["align_fig"][case][0]
    assert np.isfinite(r["T"]).all() and np.array_equal(r["T"][3], [0, 0, 0, 1])
    # aligned_out = the source under final_transform rounded to float; the other fields of the structs are the source's
    al = r["aligned"]
    got = np.stack([al["x"], al["y"], al["z"]], 1)
    assert np.array_equal(got.view(np.uint32), _apply_f32(r["T"].astype(np.float32), src).view(np.uint32))
    assert np.array_equal(al["intensity"], cloud["intensity"]) and np.array_equal(al["label"], cloud["label"])
    # device records give the same bits
    d_src, d_out = lisreg.DeviceArray(_records(src)), lisreg.DeviceArray(np.zeros((len(src), 4), np.float32))
    rd = gpu_ctx.vgicp_align(slot, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    assert rd["T"].tobytes() == r["T"].tobytes() and rd["error"] == r["error"] and rd["lam"] == r["lam"]
    assert (rd["converged"], rd["iters"], rd["n_evals"], rd["n_rejected"]) == (r["converged"], r["iters"], r["n_evals"], r["n_rejected"])
    assert np.array_equal(lisreg.device_to_host(d_out.ptr, (len(src), 4), np.float32)[:, :3].view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_null_guess_is_the_identity_and_no_pair_returns_the_guess(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.vgicp_default_params()
    moved = _apply_f32(world["guess"], world["src"])
    a = gpu_ctx.vgicp_align(SLOT, _pcl(moved), P, None)
    b = gpu_ctx.vgicp_align(SLOT, _pcl(moved), P, np.eye(4, dtype=np.float32))
    assert a["T"].tobytes() == b["T"].tobytes() and (a["iters"], a["n_evals"]) == (b["iters"], b["n_evals"])
    assert a["iters"] >= 2 and a["converged"]
    far = world["guess"].copy()
    far[0, 3] += 100.0
    r = gpu_ctx.vgicp_align(SLOT, _pcl(world["src"]), P, far)
    assert (r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], r["error"]) == (False, 0, 1, 0, 0, 0.0)
    assert np.array_equal(r["T"], far.astype(np.float64))
    # a source with NaN points: they form no pair and do not reach T
    holes = world["src"].copy()
    holes[::7] = np.nan
    r = gpu_ctx.vgicp_align(SLOT, _pcl(holes), P, world["guess"], want_aligned=True)
    assert np.isfinite(r["T"]).all() and r["converged"] and 0 < r["n_pairs_last"] <= len(holes) - len(holes[::7])
    assert np.isnan(r["aligned"]["x"][::7]).all() and np.isfinite(np.delete(r["aligned"]["x"], np.s_[::7])).all()


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, world, scene_slot):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = lisreg.vgicp_default_params()
    tgt, src = _pcl(world["tgt"][:2000]), _pcl(world["src"])
    res = lisreg.VgicpResult()

    def refused(fn, *words):
        with pytest.raises(lisreg.LisregError) as err:
            fn()
        assert err.value.code == lisreg.ERR_ARG, err.value
        for w in words:
            assert w in str(err.value), (w, str(err.value))
    # fewer finite points than k, in a target and in a source (k - 1 refused, k accepted)
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, tgt[:K - 1], P), "fewer finite points")
    few = tgt[:K + 5].copy(); few["x"][:6] = np.nan
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, few, P), "fewer finite points")
    refused(lambda: ctx.vgicp_align(SLOT, src[:K - 1], P), "fewer finite points")
    refused(lambda: ctx.vgicp_linearize(SLOT, src[:K - 1], P, np.eye(4)), "fewer finite points")
    refused(lambda: ctx.vgicp_covariances(src[:K - 1], K), "fewer finite points")
    assert ctx.vgicp_align(SLOT, src[:K], P, world["guess"])["n_evals"] >= 1
    assert ctx.vgicp_set_target(SLOT + 3, tgt[:K], P)["n_points"] == K
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, tgt[:0], P), "n <= 0")
    refused(lambda: ctx.vgicp_align(SLOT, src[:0], P), "n <= 0")
    bad = tgt.copy(); bad["y"][17] = np.inf
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, bad, P), "infinite")
    bad = src.copy(); bad["z"][3] = -np.inf
    refused(lambda: ctx.vgicp_align(SLOT, bad, P), "infinite")
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, tgt, lisreg.vgicp_default_params(resolution=0.0)), "resolution <= 0")
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, tgt, lisreg.vgicp_default_params(resolution=-1.0)), "resolution <= 0")
    refused(lambda: ctx.vgicp_set_target(SLOT + 3, tgt, lisreg.vgicp_default_params(resolution=0.01)), "2^26 cells")
    for k in (3, 33, 0, -1):
        refused(lambda: ctx.vgicp_set_target(SLOT + 3, tgt, lisreg.vgicp_default_params(k_correspondences=k)), "outside 4 .. 32")
        refused(lambda: ctx.vgicp_covariances(tgt, k), "outside 4 .. 32")
    refused(lambda: ctx.vgicp_align(SLOT, src, lisreg.vgicp_default_params(k_correspondences=40)), "outside 4 .. 32")
    refused(lambda: ctx.vgicp_align(SLOT, src, lisreg.vgicp_default_params(resolution=0.5)), "resolution differs")
    refused(lambda: ctx.vgicp_linearize(SLOT, src, lisreg.vgicp_default_params(resolution=2.0), np.eye(4)), "resolution differs")
    refused(lambda: ctx.vgicp_set_target(-1, tgt, P), "slot")
    refused(lambda: ctx.vgicp_set_target(65536, tgt, P), "slot")
    # a slot that was refused, or never set, holds no target; the map-index and the NDT slots are other numberings
    refused(lambda: ctx.vgicp_set_target(SLOT + 4, bad[:0], P), "n <= 0")
    ctx.map_index_set(SLOT + 4, tgt)
    ctx.ndt_set_target(SLOT + 4, tgt, lisreg.ndt_default_params())
    for slot in (SLOT + 4, 4242):
        refused(lambda: ctx.vgicp_align(slot, src, P), "no VGICP target")
        refused(lambda: ctx.vgicp_get_voxels(slot), "no VGICP target")
    vp = C.c_void_p
    sp, n, st = src.ctypes.data_as(vp), len(src), src.dtype.itemsize
    assert L.lisreg_vgicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, None, None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_vgicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_vgicp_align(ctx._h, SLOT, None, n, st, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_vgicp_align(ctx._h, SLOT, sp, n, 8, lisreg.FMT_XYZI, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    # k = 8 and k = 32 run (the two instantiations of the search), and agree with the restatement on a small cloud
    xyz = R.small_cloud(65)
    for k in (8, 32):
        D = R.distributions(xyz, R.params(k_correspondences=k))
        cov, nbr = ctx.vgicp_covariances(_pcl(xyz), k)
        sure = D["gap"] >= 1e-6
        assert np.array_equal(nbr[sure], D["nbr"][sure]) and np.abs(cov - R.cov6(D["C"]))[D["eig_gap"] >= 1e-3].max() <= 1e-9, k
    # the context and the scene's slot stay usable
    g = world["g"]
    r = ctx.vgicp_align(SLOT, src, P, world["guess"])
    assert (r["iters"], r["n_evals"]) == (int(g["align_counts"][3][1]), int(g["align_counts"][3][2]))


@pytest.mark.gpu
def test_twenty_alignments_do_not_grow_device_memory(gpu_ctx, world, scene_slot):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = lisreg.vgicp_default_params()
    src = _pcl(world["src"])
    first = gpu_ctx.vgicp_align(SLOT, src, P, world["guess"], want_aligned=True)          # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        r = gpu_ctx.vgicp_align(SLOT, src, P, world["guess"], want_aligned=True)
    assert free_bytes() == before
    assert r["T"].tobytes() == first["T"].tobytes() and r["aligned"].tobytes() == first["aligned"].tobytes()


import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


@pytest.mark.gpu
def test_alignment_on_a_callers_busy_stream(env, world):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the result equals the idle-stream one (and
    the restatement's), and a context left on its own stream reads the decoy"""
    e = env
    # a short alignment (one outer iteration: the linearisation and one accepted trial), so that the call does not outlast the stall the
    # gate sizes from the idle call
    P = e.lisreg.vgicp_default_params(max_iters=1)
    ref = R.align(world["T"], world["S"], R.params(max_iters=1), world["guess"])
    assert ref["margin_rho"] > 1e-6 and ref["margin_conv"] > 1e-6 and (ref["iters"], ref["n_evals"]) == (1, 2)
    e.ctx.vgicp_set_target(SLOT, _pcl(world["tgt"]), P)
    rs = _records(world["src"])
    guess = world["guess"]

    def make(dst):
        out = e.D(np.zeros_like(rs))

        def run():
            r = e.ctx.vgicp_align(SLOT, (dst.ptr, len(rs)), P, guess, out_ptr=out.ptr)
            return dict(T=r["T"], counts=np.array([r["iters"], r["n_evals"], r["n_pairs_last"]]), error=r["error"])
        return run, (lambda r: dict(res=r, aligned=TCS.to_host(out.ptr, rs.shape)))
    o, _ = TCS.late_case(e, "vgicp_align (device records)", rs, TCS.moved(rs, small=True), make)
    assert list(o["res"]["counts"]) == [ref["iters"], ref["n_evals"], ref["n_pairs_last"]]
    assert np.abs(o["res"]["T"] - ref["T"]).max() <= 1e-6
    assert np.array_equal(o["aligned"][:, :3].view(np.uint32), _apply_f32(o["res"]["T"].astype(np.float32), world["src"]).view(np.uint32))
