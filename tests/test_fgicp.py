"""lisreg_fgicp_*: FastGICP registration on the GPU (lis-slam_amd/csrc/lisreg_fgicp.hip) against its definition, tests/fgicp_ref.py.

The correspondences of the scene and of a planted target, small clouds, one linearisation (with the pairs of one pose and the sums at
another), whole alignments, a source without a pair, the argument errors, device memory, a caller's busy stream.  The CPU side (the
restatement against itself and a kd-tree, the structs, the golden file, the bars on the alignment cases) is tests/test_fgicp_ref.py.

The bounds (set where the feature was specified; every test prints its figures before it asserts):
  correspondences  indices equal wherever the restatement's nearest / second-nearest gap and its cut-off gap are >= 1e-9 (all of them on
                   the planted target, where T is the identity and x' exact: ties go to the lower index); squared distances within 1e-12
                   relative;
  the 28 sums      each within 1e-10 of the restatement's sum of |term|, pair counts equal, two calls bit-identical (the per-pair
                   arithmetic is VGICP's, so its bounds carry over);
  alignments       converged, iters, n_evals, n_rejected, n_pairs_last equal, final_transform within 1e-6 entry-wise, error within 1e-6
                   relative.  Only cases whose rho and convergence margins exceed 1e-6 and whose search margins exceed 1e-9 in the
                   restatement are used (asserted on the CPU)."""
import ctypes as C
import os

import numpy as np
import pytest

import fgicp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fgicp", "fgicp_cases.npz")
SLOT = 13
K = 20
LIN_SIZES = (1, 63, 64, 65, 257, 0)                # source sizes of the one-linearisation cases; 1: the one-pair source, 0: the whole source


def _pcl(xyz):
    from lisreg import synth
    return synth.to_pcl(np.ascontiguousarray(xyz, np.float32))


def _records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def _apply_f32(F, xyz):
    """transformPointCloud in float, products and sums rounded one by one (lisreg_transform_cloud)"""
    F = np.asarray(F, np.float32)
    x, y, z = (np.asarray(xyz[:, k], np.float32) for k in range(3))
    return np.stack([((F[r, 0] * x + F[r, 1] * y) + F[r, 2] * z) + F[r, 3] for r in range(3)], 1)


@pytest.fixture(scope="module")
def world():
    """the scene, its restatement target and source and the golden file: made once, read by every test, never changed"""
    W = dict(R.world())
    W["g"] = np.load(GOLDEN)
    W["poses"] = R.lin_poses(W["guess"], W["T_true"])
    return W


@pytest.fixture(scope="module")
def scene_slot(gpu_ctx, world):
    import lisreg
    return gpu_ctx.fgicp_set_target(SLOT, _pcl(world["tgt"]), lisreg.fgicp_default_params())


@pytest.fixture(scope="module")
def scene_pairs(world):
    """the restatement's pair sets of the whole source at the three poses"""
    return [R.find_pairs(world["T"], world["S"], T, R.params()) for T in world["poses"]]


@pytest.mark.gpu
def test_correspondences_of_the_scene(gpu_ctx, world, scene_slot, scene_pairs):
    import lisreg
    assert scene_slot["n_points"] == 25401 and len(scene_slot["grid_dims"]) == 3 and min(scene_slot["grid_dims"]) >= 1
    P = lisreg.fgicp_default_params()
    src = world["src"]
    d_src = lisreg.DeviceArray(_records(src))
    for ip, (T, want) in enumerate(zip(world["poses"], scene_pairs)):
        idx, sq = gpu_ctx.fgicp_correspondences(SLOT, _pcl(src), P, T)
        sure = (want["row_nn"] >= 1e-9) & (want["row_cut"] >= 1e-9)
        hit = want["idx"] >= 0
        both = hit & (idx >= 0)
        rel = float(np.max(np.abs(sq[both] - want["sq"][both]) / want["sq"][both])) if both.any() else 0.0
        print(f"[fgicp] correspondences of the scene, pose {ip}: {hit.sum()} pairs of {len(src)}, {int((~sure).sum())} rows under a gap bar, "
              f"rows differing {int((idx != want['idx'])[sure].sum())}, worst squared-distance error {rel:.3e} relative")
        assert np.array_equal(idx[sure], want["idx"][sure]), ip
        assert sure.sum() >= len(src) - 2, ip
        assert rel <= 1e-12, (ip, rel)
        assert np.isnan(sq[idx < 0]).all() and np.isfinite(sq[idx >= 0]).all(), ip
        assert np.array_equal(want["idx"][::8], world["g"]["corr_idx"][ip]), ip
        idx_d, sq_d = gpu_ctx.fgicp_correspondences(SLOT, (d_src.ptr, len(src)), P, T)          # device records: the same bits
        assert idx_d.tobytes() == idx.tobytes() and sq_d.tobytes() == sq.tobytes(), ip
    assert (scene_pairs[2]["idx"] == -1).all() and (idx == -1).all()                            # the pose 100 m away


def _planted():
    """(target xyz, queries xyz, named query rows).  The target is vgicp_ref's planted cloud plus float-exact points far from it: two pairs
    of points 2 m apart (the lower index once on the low-x and once on the high-x side) and one point on its own.  The queries (the
    source cloud of the calls: T is the identity, so x' is exact) are planted around them, beyond every face and one corner of the
    target's bounding box, and in the 30 m of empty cells before the cluster; random filler brings the cloud above k finite points."""
    xyz, groups = R.planted_cloud()
    n0 = len(xyz)
    extra = np.float32([[-20, -20, 0], [-18, -20, 0], [-18, -30, 0], [-20, -30, 0], [-40, -40, 0]])
    tgt = np.concatenate([xyz, extra])
    lo, hi = np.nanmin(tgt, 0).astype(np.float64), np.nanmax(tgt, 0).astype(np.float64)
    q, rows = [], {}

    def add(name, pts):
        pts = np.atleast_2d(np.asarray(pts, np.float64))
        rows[name] = np.arange(len(q), len(q) + len(pts))
        q.extend(pts.tolist())
    add("identical", [3.5, 9.5, 0.75])
    add("nan", [[np.nan, 1.0, 1.0], [np.nan] * 3])
    add("mid_a", [-19, -20, 0])
    add("mid_b", [-19, -30, 0])
    add("cut_on", [-45, -40, 0])
    add("cut_in", [np.nextafter(np.float32(-45), np.float32(0)), -40, 0])
    add("cut_on_inside", [-35, -40, 0])                       # the same 5 m from inside the bounding box: decided by the walk, not the box
    add("cut_in_inside", [np.nextafter(np.float32(-35), np.float32(-40)), -40, 0])
    fin = tgt[~np.isnan(tgt).any(1)].astype(np.float64)
    near, far = [], []
    for ax in range(3):
        for side, bound in ((-1.0, lo), (1.0, hi)):
            p = fin[np.argmax(fin[:, ax]) if side > 0 else np.argmin(fin[:, ax])]         # the target's outermost point on this side
            a, b = p.copy(), p.copy()
            a[ax], b[ax] = bound[ax] + side * 1.0, bound[ax] + side * 7.0
            near.append(a); far.append(b)
    add("face_near", near)
    add("face_far", far)
    add("corner_near", hi + 1.0)
    add("corner_far", hi + 10.0)
    add("gap", np.stack([np.linspace(10.0, 34.0, 9), np.full(9, 3.0), np.full(9, 1.0)], 1))
    add("filler", np.random.default_rng(77).uniform(-1.0, 7.0, (24, 3)))
    return tgt, np.asarray(q, np.float32), rows, groups, n0


@pytest.mark.gpu
def test_correspondences_of_the_planted_target(gpu_ctx):
    import lisreg
    tgt, q, rows, groups, n0 = _planted()
    Tt = R.build_target(tgt, R.params())
    assert set(np.flatnonzero(~Tt["ok"])) == set(groups["nan"])
    eye = np.eye(4)
    for kind in (0, 1):
        P = lisreg.fgicp_default_params(kind)
        gpu_ctx.fgicp_set_target(SLOT + 1, _pcl(tgt), P)
        idx, sq = gpu_ctx.fgicp_correspondences(SLOT + 1, _pcl(q), P, eye)
        w_idx, w_sq, _, _ = R.search(Tt, q.astype(np.float64), P.max_correspondence_distance)
        print(f"[fgicp] planted target, kind {kind}: {int((w_idx >= 0).sum())} of {len(q)} queries have a pair, rows differing {int((idx != w_idx).sum())}")
        # T is the identity: x' and every squared distance are exact, so every row is the brute-force one, ties included
        assert np.array_equal(idx, w_idx), kind
        assert np.array_equal(np.isnan(sq), np.isnan(w_sq)) and np.array_equal(sq[idx >= 0], w_sq[idx >= 0]), kind
        assert not np.isin(idx, groups["nan"]).any() and (idx[rows["nan"]] == -1).all(), kind
        assert idx[rows["identical"]][0] == groups["identical"].min() and sq[rows["identical"]][0] == 0.0, kind
        assert idx[rows["mid_a"]][0] == n0 and idx[rows["mid_b"]][0] == n0 + 2 and sq[rows["mid_a"]][0] == 1.0, kind    # the lower index
        if kind == 0:
            assert idx[rows["cut_on"]][0] == -1 and idx[rows["cut_in"]][0] == n0 + 4 and sq[rows["cut_in"]][0] < 25.0    # strict
            assert idx[rows["cut_on_inside"]][0] == -1 and idx[rows["cut_in_inside"]][0] == n0 + 4 and sq[rows["cut_in_inside"]][0] < 25.0
            assert (idx[rows["face_near"]] >= 0).all() and (idx[rows["face_far"]] == -1).all() and idx[rows["corner_far"]][0] == -1
            assert (idx[rows["gap"]] >= 0).any() and (idx[rows["gap"]] == -1).any()
        else:                                             # no cut-off: every finite query has a pair, across any number of empty cells
            finite = ~np.isnan(q).any(1)
            assert (idx[finite] >= 0).all() and idx[rows["cut_on"]][0] == n0 + 4 and sq[rows["cut_on"]][0] == 25.0
            assert np.isin(idx[rows["gap"]][-3:], groups["cluster"]).all()
        # the cell edge of the search grid does not matter
        for edge in (0.37, 1.9):
            info = gpu_ctx.fgicp_set_target(SLOT + 1, _pcl(tgt), P, cell_edge=edge)
            idx_e, sq_e = gpu_ctx.fgicp_correspondences(SLOT + 1, _pcl(q), P, eye)
            assert idx_e.tobytes() == idx.tobytes() and sq_e.tobytes() == sq.tobytes(), (kind, edge, info)


def _compare_sums(tag, got, pairs, ev):
    err = np.abs(got - ev["out"])
    worst = float(np.max(err[ev["abs"] > 0] / ev["abs"][ev["abs"] > 0])) if ev["n_pairs"] else 0.0
    assert pairs == ev["n_pairs"], (tag, pairs, ev["n_pairs"])
    assert np.all(err <= 1e-10 * ev["abs"]), (tag, err, ev["abs"])
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 21, 64, 65])
def test_small_clouds(gpu_ctx, nt):
    """targets of 20 (every point is every point's neighbourhood), 21, 64 and 65 points, sources of 20, 63, 64, 65 and 257"""
    import lisreg
    P = lisreg.fgicp_default_params()
    prm = R.params()
    txyz = R.small_cloud(nt)
    Tt = R.build_target(txyz, prm)
    assert gpu_ctx.fgicp_set_target(SLOT + 2, _pcl(txyz), P)["n_points"] == nt
    T = R.se3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.08])
    worst = 0.0
    for ns in (20, 63, 64, 65, 257):
        sxyz = R.small_cloud(ns, seed=11)
        S = R.prepare_source(sxyz, prm)
        # (the 1e-10 bar on the sums stands on normals defined to 1e-13: eigen-gaps of 1e-3 and more, and neighbour sets decided by 1e-6)
        assert min(S["dist"]["eig_gap"].min(), Tt["dist"]["eig_gap"].min()) >= 1e-3 and min(S["dist"]["gap"].min(), Tt["dist"]["gap"].min()) >= 1e-6
        want = R.find_pairs(Tt, S, T, prm)
        idx, sq = gpu_ctx.fgicp_correspondences(SLOT + 2, _pcl(sxyz), P, T)
        sure = (want["row_nn"] >= 1e-9) & (want["row_cut"] >= 1e-9)
        assert sure.all() and np.array_equal(idx, want["idx"]) and (idx >= 0).all(), (nt, ns)
        assert np.max(np.abs(sq - want["sq"]) / want["sq"]) <= 1e-12, (nt, ns)
        for hess in (True, False):
            ev = R.sums(Tt, S, want, T, hess)
            out, pairs = gpu_ctx.fgicp_linearize(SLOT + 2, _pcl(sxyz), P, T, hess)
            worst = max(worst, _compare_sums((nt, ns, hess), out, pairs, ev))
            assert pairs == ns and (hess or not out[7:].any())
    print(f"[fgicp] target of {nt} points: worst |sum - restatement| / sum|term| {worst:.3e}")


@pytest.mark.gpu
def test_one_linearisation(gpu_ctx, world, scene_slot, scene_pairs):
    import lisreg
    g, src, poses = world["g"], world["src"], world["poses"]
    P = lisreg.fgicp_default_params()
    prm = R.params()
    cut = {n: R.prepare_source(src[:n], prm) for n in LIN_SIZES if n >= K}
    # a source of one point has no distribution (fewer points than k are refused), so the one-pair case is a source of k points of
    # which one lies within reach of the map: the others are 200 m above it, spread out so that the one point's normal stays defined
    one = src[:K].copy()
    one[1:] = one[0] + (one[1:] - one[0]) * np.float32([50, 50, 1]) + np.float32([0, 0, 200])
    cut[1] = R.prepare_source(one, prm)
    cut[0] = world["S"]
    assert all(S["dist"]["eig_gap"].min() >= 1e-3 and S["dist"]["gap"].min() >= 1e-6 for S in cut.values())
    k, worst = 0, 0.0
    for ip, T in enumerate(poses):
        for n in LIN_SIZES:
            cloud = one if n == 1 else src[: n or len(src)]
            m = len(cloud)
            d_src = lisreg.DeviceArray(_records(cloud))
            pairs_ref = scene_pairs[ip] if n == 0 else R.find_pairs(world["T"], cut[n], T, prm)
            assert (pairs_ref["nn_gap"] >= 1e-9 or ip == 2) and pairs_ref["cut_gap"] >= 1e-9, (ip, n)     # (100 m away nothing is a pair)
            for hess in (1, 0):
                ev = R.sums(world["T"], cut[n], pairs_ref, T, bool(hess))
                if n == 0:                                    # the whole source: the golden file's rows
                    row = 2 * ip + (1 - hess)
                    assert np.all(np.abs(ev["out"] - g["lin_out"][row]) <= 1e-11 * g["lin_abs"][row]) and ev["n_pairs"] == g["lin_pairs"][row]
                if n == 1:
                    assert ev["n_pairs"] == (1 if ip < 2 else 0)
                    with pytest.raises(lisreg.LisregError):
                        gpu_ctx.fgicp_linearize(SLOT, _pcl(src[:1]), P, T, bool(hess))
                out, pairs = gpu_ctx.fgicp_linearize(SLOT, _pcl(cloud), P, T, bool(hess))
                again, _ = gpu_ctx.fgicp_linearize(SLOT, (d_src.ptr, m), P, T, bool(hess))
                assert out.tobytes() == again.tobytes(), (ip, m, hess, "two calls (host structs, device records) differ")
                worst = max(worst, _compare_sums((ip, m, hess), out, pairs, ev))
                if not hess:
                    assert not out[7:].any()
                if not ev["n_pairs"]:
                    assert not out.any() and ip == 2
                k += 1
    print(f"[fgicp] one linearisation: worst |sum - restatement| / sum|term| over {k} cases {worst:.3e}")
    assert k == 36


@pytest.mark.gpu
def test_an_error_evaluation_reuses_the_pairs_of_the_linearisation(gpu_ctx, world, scene_slot, scene_pairs):
    """T_pairs != T_eval: pairs and M from the guess, the sums at the truth"""
    import lisreg
    g, src, poses = world["g"], world["src"], world["poses"]
    P = lisreg.fgicp_default_params()
    assert (scene_pairs[0]["idx"] != scene_pairs[1]["idx"]).sum() > 100             # the two poses do pair differently
    for hess in (1, 0):
        ev = R.sums(world["T"], world["S"], scene_pairs[0], poses[1], bool(hess))
        row = 6 + (1 - hess)
        assert np.all(np.abs(ev["out"] - g["lin_out"][row]) <= 1e-11 * g["lin_abs"][row])
        out, pairs = gpu_ctx.fgicp_linearize(SLOT, _pcl(src), P, poses[0], bool(hess), T_eval=poses[1])
        worst = _compare_sums(("reuse", hess), out, pairs, ev)
        fresh, _ = gpu_ctx.fgicp_linearize(SLOT, _pcl(src), P, poses[1], bool(hess))
        same_pose, _ = gpu_ctx.fgicp_linearize(SLOT, _pcl(src), P, poses[0], bool(hess), T_eval=poses[0])
        plain, _ = gpu_ctx.fgicp_linearize(SLOT, _pcl(src), P, poses[0], bool(hess))
        far = np.abs(out - fresh)[:28 if hess else 7]
        print(f"[fgicp] pairs of the guess, sums at the truth (H {hess}): worst error {worst:.3e} of sum|term|; e {out[0]:.6f} against "
              f"{fresh[0]:.6f} of a fresh linearisation at the truth")
        assert far[0] > 1e-6 * ev["abs"][0] and np.sum(far > 1e-10 * ev["abs"][:len(far)]) >= len(far) // 2, \
            "the sums equal a fresh linearisation's: the pairs were not reused"
        assert same_pose.tobytes() == plain.tobytes()


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
        slot = SLOT + 3
        gpu_ctx.fgicp_set_target(slot, _pcl(tgt), lisreg.fgicp_default_params())
    P = lisreg.fgicp_default_params(transformation_epsilon=eps)
    cloud = _pcl(src)
    r = gpu_ctx.fgicp_align(slot, cloud, P, guess, want_aligned=True)
    dT = np.abs(r["T"] - want).max()
    et, er = R.pose_error(r["T"], T_true)
    rel = abs(r["error"] - g["align_fig"][case][0]) / g["align_fig"][case][0]
    print(f"[fgicp] align seed {seed} eps {eps}: converged {r['converged']} iters {r['iters']} evals {r['n_evals']} rejected {r['n_rejected']} "
          f"pairs {r['n_pairs_last']} |dT| {dT:.3e} error off by {rel:.3e}, {1e3 * et:.2f} mm / {1e3 * er:.3f} mrad from the truth")
    assert (int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"]) == tuple(int(v) for v in counts[:5])
    assert dT <= 1e-6, dT
    assert rel <= 1e-6, rel
    assert np.isfinite(r["T"]).all() and np.array_equal(r["T"][3], [0, 0, 0, 1])
    # aligned_out = the source under final_transform rounded to float; the other fields of the structs are the source's
    al = r["aligned"]
    got = np.stack([al["x"], al["y"], al["z"]], 1)
    assert np.array_equal(got.view(np.uint32), _apply_f32(r["T"].astype(np.float32), src).view(np.uint32))
    assert np.array_equal(al["intensity"], cloud["intensity"]) and np.array_equal(al["label"], cloud["label"])
    # device records give the same bits
    d_src, d_out = lisreg.DeviceArray(_records(src)), lisreg.DeviceArray(np.zeros((len(src), 4), np.float32))
    rd = gpu_ctx.fgicp_align(slot, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    assert rd["T"].tobytes() == r["T"].tobytes() and rd["error"] == r["error"] and rd["lam"] == r["lam"]
    assert (rd["converged"], rd["iters"], rd["n_evals"], rd["n_rejected"], rd["n_pairs_last"]) == \
           (r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"])
    assert np.array_equal(lisreg.device_to_host(d_out.ptr, (len(src), 4), np.float32)[:, :3].view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_null_guess_is_the_identity_and_no_pair_returns_the_guess(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.fgicp_default_params()
    moved = _apply_f32(world["guess"], world["src"])
    a = gpu_ctx.fgicp_align(SLOT, _pcl(moved), P, None)
    b = gpu_ctx.fgicp_align(SLOT, _pcl(moved), P, np.eye(4, dtype=np.float32))
    assert a["T"].tobytes() == b["T"].tobytes() and (a["iters"], a["n_evals"]) == (b["iters"], b["n_evals"])
    assert a["iters"] >= 2 and a["converged"]
    far = world["guess"].copy()
    far[0, 3] += 100.0
    r = gpu_ctx.fgicp_align(SLOT, _pcl(world["src"]), P, far)
    assert (r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], r["error"]) == (False, 0, 1, 0, 0, 0.0)
    assert np.array_equal(r["T"], far.astype(np.float64))
    # a source with NaN points: they form no pair and do not reach T
    holes = world["src"].copy()
    holes[::7] = np.nan
    r = gpu_ctx.fgicp_align(SLOT, _pcl(holes), P, world["guess"], want_aligned=True)
    assert np.isfinite(r["T"]).all() and r["converged"] and 0 < r["n_pairs_last"] <= len(holes) - len(holes[::7])
    assert np.isnan(r["aligned"]["x"][::7]).all() and np.isfinite(np.delete(r["aligned"]["x"], np.s_[::7])).all()
    idx, sq = gpu_ctx.fgicp_correspondences(SLOT, _pcl(holes), P, world["guess"])
    assert (idx[::7] == -1).all() and np.isnan(sq[::7]).all() and (np.delete(idx, np.s_[::7]) >= 0).all()


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, world, scene_slot):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = lisreg.fgicp_default_params()
    tgt, src = _pcl(world["tgt"][:2000]), _pcl(world["src"])
    res = lisreg.FgicpResult()

    def refused(fn, *words):
        with pytest.raises(lisreg.LisregError) as err:
            fn()
        assert err.value.code == lisreg.ERR_ARG, err.value
        for w in words:
            assert w in str(err.value), (w, str(err.value))
    # fewer finite points than k, in a target and in a source (k - 1 refused, k accepted)
    refused(lambda: ctx.fgicp_set_target(SLOT + 4, tgt[:K - 1], P), "fewer finite points")
    few = tgt[:K + 5].copy(); few["x"][:6] = np.nan
    refused(lambda: ctx.fgicp_set_target(SLOT + 4, few, P), "fewer finite points")
    refused(lambda: ctx.fgicp_align(SLOT, src[:K - 1], P), "fewer finite points")
    refused(lambda: ctx.fgicp_linearize(SLOT, src[:K - 1], P, np.eye(4)), "fewer finite points")
    refused(lambda: ctx.fgicp_correspondences(SLOT, src[:K - 1], P, np.eye(4)), "fewer finite points")
    assert ctx.fgicp_align(SLOT, src[:K], P, world["guess"])["n_evals"] >= 1
    assert ctx.fgicp_set_target(SLOT + 4, tgt[:K], P)["n_points"] == K
    refused(lambda: ctx.fgicp_set_target(SLOT + 4, tgt[:0], P), "n <= 0")
    refused(lambda: ctx.fgicp_align(SLOT, src[:0], P), "n <= 0")
    bad = tgt.copy(); bad["y"][17] = np.inf
    refused(lambda: ctx.fgicp_set_target(SLOT + 4, bad, P), "infinite")
    bad = src.copy(); bad["z"][3] = -np.inf
    refused(lambda: ctx.fgicp_align(SLOT, bad, P), "infinite")
    for v in (0.0, -1.0, float("nan")):
        refused(lambda: ctx.fgicp_set_target(SLOT + 4, tgt, lisreg.fgicp_default_params(max_correspondence_distance=v)), "max_correspondence_distance <= 0")
        refused(lambda: ctx.fgicp_align(SLOT, src, lisreg.fgicp_default_params(max_correspondence_distance=v)), "max_correspondence_distance <= 0")
    for k in (3, 33, 0, -1):
        refused(lambda: ctx.fgicp_set_target(SLOT + 4, tgt, lisreg.fgicp_default_params(k_correspondences=k)), "outside 4 .. 32")
    refused(lambda: ctx.fgicp_align(SLOT, src, lisreg.fgicp_default_params(k_correspondences=40)), "outside 4 .. 32")
    for kw in (dict(transformation_epsilon=0.0), dict(rotation_epsilon=-1.0), dict(lm_init_lambda_factor=0.0), dict(max_iters=-1),
               dict(lm_max_iterations=0), dict(plane_epsilon=0.0), dict(plane_epsilon=1.5)):
        refused(lambda: ctx.fgicp_align(SLOT, src, lisreg.fgicp_default_params(**kw)), "bad transformation_epsilon")
    refused(lambda: ctx.fgicp_set_target(SLOT + 4, tgt, P, cell_edge=-1.0), "cell_edge < 0")
    refused(lambda: ctx.fgicp_set_target(-1, tgt, P), "slot")
    refused(lambda: ctx.fgicp_set_target(65536, tgt, P), "slot")
    # a slot that was refused, or never set, holds no target; the map-index, the NDT and the VGICP slots are other numberings
    refused(lambda: ctx.fgicp_set_target(SLOT + 5, bad[:0], P), "n <= 0")
    ctx.map_index_set(SLOT + 5, tgt)
    ctx.ndt_set_target(SLOT + 5, tgt, lisreg.ndt_default_params())
    ctx.vgicp_set_target(SLOT + 5, tgt, lisreg.vgicp_default_params())
    for slot in (SLOT + 5, 4242):
        refused(lambda: ctx.fgicp_align(slot, src, P), "no FastGICP target")
        refused(lambda: ctx.fgicp_linearize(slot, src, P, np.eye(4)), "no FastGICP target")
        refused(lambda: ctx.fgicp_correspondences(slot, src, P, np.eye(4)), "no FastGICP target")
    vp = C.c_void_p
    sp, n, st = src.ctypes.data_as(vp), len(src), src.dtype.itemsize
    assert L.lisreg_fgicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, None, None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_align(ctx._h, SLOT, None, n, st, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_align(ctx._h, SLOT, sp, n, 8, lisreg.FMT_XYZI, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_correspondences(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_linearize(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, None, 1, None, None) == lisreg.ERR_ARG
    # k = 8 and k = 32 run (the two instantiations of the distributions' search), and agree with the restatement on small clouds
    txyz, sxyz = R.small_cloud(65), R.small_cloud(64, seed=11)
    T = R.se3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.08])
    for k in (8, 32):
        prm, Pk = R.params(k_correspondences=k), lisreg.fgicp_default_params(k_correspondences=k)
        Tt, S = R.build_target(txyz, prm), R.prepare_source(sxyz, prm)
        assert min(S["dist"]["eig_gap"].min(), Tt["dist"]["eig_gap"].min()) >= 1e-3 and min(S["dist"]["gap"].min(), Tt["dist"]["gap"].min()) >= 1e-6, k
        ctx.fgicp_set_target(SLOT + 4, _pcl(txyz), Pk)
        ev = R.linearize(Tt, S, T, prm, True)
        out, pairs = ctx.fgicp_linearize(SLOT + 4, _pcl(sxyz), Pk, T, True)
        _compare_sums(("k", k), out, pairs, ev)
    # the context and the scene's slot stay usable
    g = world["g"]
    r = ctx.fgicp_align(SLOT, src, P, world["guess"])
    assert (r["iters"], r["n_evals"]) == (int(g["align_counts"][3][1]), int(g["align_counts"][3][2]))


@pytest.mark.gpu
def test_twenty_calls_do_not_grow_device_memory(gpu_ctx, world, scene_slot):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = lisreg.fgicp_default_params()
    src, tgt = _pcl(world["src"]), _pcl(world["tgt"])
    first = gpu_ctx.fgicp_align(SLOT, src, P, world["guess"], want_aligned=True)          # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        r = gpu_ctx.fgicp_align(SLOT, src, P, world["guess"], want_aligned=True)
    assert free_bytes() == before
    assert r["T"].tobytes() == first["T"].tobytes() and r["aligned"].tobytes() == first["aligned"].tobytes()
    info = gpu_ctx.fgicp_set_target(SLOT + 6, tgt, P)
    before = free_bytes()
    for _ in range(20):
        assert gpu_ctx.fgicp_set_target(SLOT + 6, tgt, P) == info
    assert free_bytes() == before
    again = gpu_ctx.fgicp_align(SLOT + 6, src, P, world["guess"])
    assert again["T"].tobytes() == first["T"].tobytes()


import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


@pytest.mark.gpu
def test_alignment_on_a_callers_busy_stream(env, world):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the result equals the idle-stream one (and
    the restatement's), and a context left on its own stream reads the decoy"""
    e = env
    # a short alignment (one outer iteration: the linearisation and one accepted trial), so that the call does not outlast the stall the
    # gate sizes from the idle call
    P = e.lisreg.fgicp_default_params(max_iters=1)
    ref = R.align(world["T"], world["S"], R.params(max_iters=1), world["guess"])
    assert ref["margin_rho"] > 1e-6 and ref["margin_conv"] > 1e-6 and ref["margin_nn"] >= 1e-9 and ref["margin_cut"] >= 1e-9
    assert (ref["iters"], ref["n_evals"]) == (1, 2)
    e.ctx.fgicp_set_target(SLOT, _pcl(world["tgt"]), P)
    rs = _records(world["src"])
    guess = world["guess"]

    def make(dst):
        out = e.D(np.zeros_like(rs))

        def run():
            r = e.ctx.fgicp_align(SLOT, (dst.ptr, len(rs)), P, guess, out_ptr=out.ptr)
            return dict(T=r["T"], counts=np.array([r["iters"], r["n_evals"], r["n_pairs_last"]]), error=r["error"])
        return run, (lambda r: dict(res=r, aligned=TCS.to_host(out.ptr, rs.shape)))
    o, _ = TCS.late_case(e, "fgicp_align (device records)", rs, TCS.moved(rs, small=True), make)
    assert list(o["res"]["counts"]) == [ref["iters"], ref["n_evals"], ref["n_pairs_last"]]
    assert np.abs(o["res"]["T"] - ref["T"]).max() <= 1e-6
    assert np.array_equal(o["aligned"][:, :3].view(np.uint32), _apply_f32(o["res"]["T"].astype(np.float32), world["src"]).view(np.uint32))
