"""lisreg_gicp_*: PCL's GICP on the GPU (lis-slam_amd/csrc/lisreg_gicp.hip) against its definition, tests/gicp_ref.py.

The 74 moments of the scene at the guess, at the truth and 100 m away; the moments against FastGICP's own sums over the same pairs (an
independent GPU path); the source-size edges (the k limit, the wavefront edges, more than 64 partial records), NaN points, cut-offs that
leave exactly 1, 3 and 4 pairs; whole alignments; state, refusals, device memory, a caller's busy stream; the host mirror's program.
The CPU side (the restatement against itself, the bars on the alignment cases, the structs, the golden file, the host BFGS against the
restatement bit for bit) is tests/test_gicp_ref.py and tests/test_gicp_host.py.

The bounds (set where the feature was specified; every test prints its figures before it asserts):
  the 74 moments   each within 1e-10 of the restatement's sum of |term| (the bar of tests/test_fgicp.py::_compare_sums), pair counts
                   equal, two calls bit-identical;
  against FastGICP m f from the moments at T_eval != T_pairs within test_gicp_ref.MOMENT_F_BAR (100 x the measured worst of the moment
                   form against the per-pair float64 form, 1.13e-11) of lisreg_fgicp_linearize's error over the same pairs;
  alignments       converged, iters, inner_iters, n_evals, n_pairs_last, inner_exit equal, final_transform within 1e-6 entry-wise,
                   error within 1e-6 relative, n_rounds == iters (iters + 1 when the loop ends on fewer than 4 pairs).  Only cases
                   whose decision margins exceed 1e-6, whose search margins exceed 1e-9 and which end within 1e-7 of themselves when
                   their moments move by 1e-12 in the restatement are used (asserted on the CPU, tests/test_gicp_ref.py); the family's
                   0.3 m / 2 degree guess is no such case and is held to the truth instead."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gicp_ref as R
from test_gicp_ref import MOMENT_F_BAR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gicp", "gicp_cases.npz")
SLOT = 113
K = 20
T_SMALL = R.F.se3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.08])
COUNT_KEYS = ("converged", "iters", "inner_iters", "n_evals", "n_rounds", "n_pairs_last", "inner_exit")


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


def _bits(r):
    return (r["T"].tobytes(), r["error"], r["last_delta"]) + tuple(int(r[k]) for k in COUNT_KEYS)


def _compare_moments(tag, got, rec, ab):
    err = np.abs(got - rec)
    worst = float(np.max(err[ab > 0] / ab[ab > 0])) if rec[73] else 0.0
    assert got[73] == rec[73], (tag, got[73], rec[73])
    assert np.all(err <= 1e-10 * ab), (tag, err, ab)
    return worst


@pytest.fixture(scope="module")
def world():
    """the scene, its restatement target and source and the golden file: made once, read by every test, never changed"""
    W = dict(R.world())
    W["g"] = np.load(GOLDEN)
    W["poses"] = R.lin_poses(W["guess"], W["T_true"])
    return W


@pytest.fixture(scope="module")
def scene_slot(gpu_ctx, world):
    """a GICP target is a FastGICP slot, set with FastGICP's own defaults (k 20, plane_epsilon = gicp_epsilon = 1e-3)"""
    import lisreg
    return gpu_ctx.fgicp_set_target(SLOT, _pcl(world["tgt"]), lisreg.fgicp_default_params())


@pytest.fixture(scope="module")
def small_sources():
    """the restatement's sources of the size edges (made once): 20 = the k limit, 21, the wavefront edges 63 / 64 / 65, 4 097 = 65
    partial records, so that the total takes its second stride"""
    prm = R.params()
    out = {}
    for ns in (20, 21, 63, 64, 65, 4097):
        xyz = R.small_cloud(ns, seed=11)
        S = R.prepare_source(xyz, prm)
        # (the 1e-10 bar on the sums stands on normals defined to 1e-13: eigen-gaps of 1e-3 and more, and neighbour sets decided by 1e-6)
        assert S["dist"]["eig_gap"].min() >= 1e-3 and S["dist"]["gap"].min() >= 1e-6, ns
        out[ns] = (xyz, S)
    return out


@pytest.mark.gpu
def test_moments_of_the_scene(gpu_ctx, world, scene_slot):
    import lisreg
    g, src = world["g"], world["src"]
    assert scene_slot["n_points"] == 25401 and len(src) == 2939
    P = lisreg.gicp_default_params()
    d_src = lisreg.DeviceArray(_records(src))
    assert np.allclose(g["centre"], R.centre(world["T"]), rtol=0, atol=0)
    for ip, T in enumerate(world["poses"]):
        got = gpu_ctx.gicp_moments(SLOT, _pcl(src), P, T)
        worst = _compare_moments(ip, got, g["mom_rec"][ip], g["mom_abs"][ip])
        print(f"[gicp] moments of the scene, pose {ip}: {int(got[73])} pairs, worst |sum - restatement| / sum|term| {worst:.3e}")
        again = gpu_ctx.gicp_moments(SLOT, (d_src.ptr, len(src)), P, T)                  # device records, a second call: the same bits
        assert again.tobytes() == got.tobytes(), ip
    assert not got.any() and list(g["mom_rec"][:, 73]) == [2939.0, 2939.0, 0.0]          # the pose 100 m away: all 74 zero


@pytest.mark.gpu
def test_moments_against_fastgicps_own_sums(gpu_ctx, world, scene_slot):
    """an independent GPU path over the same pairs: the pairs and their M from T_pairs = the guess, the error at T_eval = X(x) guess.
    FastGICP recomputes x' and d per pair at T_eval; the moments give m f(x) without touching a pair again."""
    import lisreg
    P = lisreg.gicp_default_params()
    Pf = lisreg.fgicp_default_params(max_correspondence_distance=P.max_correspondence_distance)
    G = np.asarray(world["guess"], np.float64)
    c = R.centre(world["T"])
    rec = gpu_ctx.gicp_moments(SLOT, _pcl(world["src"]), P, G)
    worst = 0.0
    for x in ([0.1, -0.05, 0.02, 0.01, -0.02, 0.03], [1e-4, 2e-4, -1e-4, 1e-5, -2e-5, 3e-5], [0.0] * 6):
        T_eval = R.pose_of(x, G)
        out, pairs = gpu_ctx.fgicp_linearize(SLOT, _pcl(world["src"]), Pf, G, False, T_eval=T_eval)
        mf = R.fdf(rec, c, [0.0] * 6, x, False)[0] * rec[73]
        rel = abs(mf - out[0]) / out[0]
        worst = max(worst, rel)
        print(f"[gicp] m f from the moments {mf:.12f} against FastGICP's error {out[0]:.12f} over the same {pairs} pairs at x = {x}: {rel:.3e} relative")
        assert pairs == rec[73] == 2939
    assert worst <= MOMENT_F_BAR, worst


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [20, 21, 64, 65])
def test_source_and_target_size_edges(gpu_ctx, small_sources, nt):
    import lisreg
    P, Pf, prm = lisreg.gicp_default_params(), lisreg.fgicp_default_params(), R.params()
    txyz = R.small_cloud(nt)
    Tt = R.build_target(txyz, prm)
    assert Tt["dist"]["eig_gap"].min() >= 1e-3 and Tt["dist"]["gap"].min() >= 1e-6
    assert gpu_ctx.fgicp_set_target(SLOT + 2, _pcl(txyz), Pf)["n_points"] == nt
    c = R.centre(Tt)
    worst = 0.0
    for ns, (sxyz, S) in small_sources.items():
        pairs = R.find_pairs(Tt, S, T_SMALL, prm)
        assert pairs["nn_gap"] >= 1e-9 and pairs["cut_gap"] >= 1e-9, (nt, ns)
        rec, ab = R.moments(Tt, S, pairs, T_SMALL, c)
        got = gpu_ctx.gicp_moments(SLOT + 2, _pcl(sxyz), P, T_SMALL)
        worst = max(worst, _compare_moments((nt, ns), got, rec, ab))
        assert got[73] == ns
    print(f"[gicp] target of {nt} points, sources of {list(small_sources)}: worst |sum - restatement| / sum|term| {worst:.3e}")
    # the cell edge of the target's search grid does not matter
    sxyz = small_sources[4097][0]
    for edge in (0.37, 1.9):
        gpu_ctx.fgicp_set_target(SLOT + 2, _pcl(txyz), Pf, cell_edge=edge)
        assert gpu_ctx.gicp_moments(SLOT + 2, _pcl(sxyz), P, T_SMALL).tobytes() == got.tobytes(), (nt, edge)


@pytest.mark.gpu
def test_nan_points_and_cut_offs_that_leave_one_three_and_four_pairs(gpu_ctx):
    import lisreg
    Pf, prm = lisreg.fgicp_default_params(), R.params()
    txyz = R.small_cloud(65)
    Tt = R.build_target(txyz, prm)
    gpu_ctx.fgicp_set_target(SLOT + 2, _pcl(txyz), Pf)
    holes = R.small_cloud(74, seed=11)
    holes[::7] = np.nan                                                      # 11 NaN points: 63 finite
    S = R.prepare_source(holes, prm)
    assert S["ok"].sum() == 63 and S["dist"]["eig_gap"][S["ok"]].min() >= 1e-3 and S["dist"]["gap"][S["ok"]].min() >= 1e-6
    c = R.centre(Tt)
    pairs = R.find_pairs(Tt, S, T_SMALL, prm)
    rec, ab = R.moments(Tt, S, pairs, T_SMALL, c)
    got = gpu_ctx.gicp_moments(SLOT + 2, _pcl(holes), lisreg.gicp_default_params(), T_SMALL)
    worst = _compare_moments("holes", got, rec, ab)
    assert got[73] == 63 and np.isfinite(got).all()
    # cut-offs between the sorted nearest distances: exactly 1, 3 and 4 pairs at the guess
    d = np.sort(np.sqrt(pairs["sq"][S["ok"]]))
    guess = T_SMALL.astype(np.float32)
    sq32 = np.sort(R.find_pairs(Tt, S, guess.astype(np.float64), prm)["sq"][S["ok"]])
    seen = []
    for want in (1, 3, 4):
        cut = float(np.sqrt(0.5 * (sq32[want - 1] + sq32[want])))
        prm_c = R.params(max_correspondence_distance=cut)
        ref = R.align(Tt, S, prm_c, guess)
        P = lisreg.gicp_default_params(max_correspondence_distance=cut)
        r = gpu_ctx.gicp_align(SLOT + 2, _pcl(holes), P, guess, want_aligned=True)
        seen.append((want, bool(r["converged"]), r["iters"], r["n_rounds"], r["n_pairs_last"]))
        if want < 4:                                                         # PCL's "need at least 4 points": not converged, the start pose
            assert (r["converged"], r["iters"], r["inner_iters"], r["n_evals"], r["n_rounds"], r["n_pairs_last"], r["inner_exit"]) == \
                   (False, 0, 0, 0, 1, want, -1), r
            assert np.array_equal(r["T"], guess.astype(np.float64)) and r["last_delta"] == 0.0
            assert (ref["converged"], ref["iters"], ref["n_rounds"], ref["n_pairs_last"]) == (0, 0, 1, want)
            assert abs(r["error"] - ref["error"]) <= 1e-10 * ref["error"]
        else:
            assert r["iters"] >= 1 and r["n_rounds"] in (r["iters"], r["iters"] + 1) and r["inner_exit"] >= 0
            assert r["n_rounds"] == r["iters"] + (0 if r["converged"] else 1)
        assert np.isfinite(r["T"]).all() and np.isnan(r["aligned"]["x"][::7]).all() and np.isfinite(np.delete(r["aligned"]["x"], np.s_[::7])).all()
    print(f"[gicp] NaN at every 7th point: worst moment error {worst:.3e} of sum|term|; (pairs wanted, converged, iters, rounds, pairs): {seen}; "
          f"nearest distances {d[:5].round(4).tolist()}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(R.ALIGN_CASES)))
def test_alignment_equals_the_restatement(gpu_ctx, world, scene_slot, case):
    import lisreg
    seed, trans, rot, eps = R.ALIGN_CASES[case]
    g = world["g"]
    counts, want = g["align_counts"][case], g["align_T"][case]
    tgt, src, guess, T_true = R.F.scene(seed, trans, rot)                    # (the cases' guesses are not the scene fixture's)
    slot = SLOT + 3
    gpu_ctx.fgicp_set_target(slot, _pcl(tgt), lisreg.fgicp_default_params())
    P = lisreg.gicp_default_params(transformation_epsilon=eps)
    cloud = _pcl(src)
    r = gpu_ctx.gicp_align(slot, cloud, P, guess, want_aligned=True)
    dT = np.abs(r["T"] - want).max()
    et, er = R.pose_error(r["T"], T_true)
    rel = abs(r["error"] - g["align_fig"][case][0]) / g["align_fig"][case][0]
    print(f"[gicp] align seed {seed} eps {eps}: converged {r['converged']} outer {r['iters']} inner {r['inner_iters']} evals {r['n_evals']} rounds "
          f"{r['n_rounds']} pairs {r['n_pairs_last']} exit {r['inner_exit']} delta {r['last_delta']:.3f} |dT| {dT:.3e} error off by {rel:.3e}, "
          f"{1e3 * et:.2f} mm / {1e3 * er:.3f} mrad from the truth")
    # golden columns: converged, iters, inner_iters, n_evals, n_rounds, n_pairs_last, inner_exit
    assert tuple(int(r[k]) for k in COUNT_KEYS) == tuple(int(v) for v in counts[:7])
    assert r["n_rounds"] == r["iters"]                                       # (no case ends on fewer than 4 pairs)
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
    rd = gpu_ctx.gicp_align(slot, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    assert _bits(rd) == _bits(r)
    assert np.array_equal(lisreg.device_to_host(d_out.ptr, (len(src), 4), np.float32)[:, :3].view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_the_familys_scene_from_its_far_guess_ends_at_the_truth(gpu_ctx, world, scene_slot):
    """the 0.3 m / 2 degree guess of tests/test_fgicp.py.  From this far the first inner minimisations spend their 20 steps unconverged
    and the run is not reproducible to 1e-6 by ANY two summation orders (gicp_ref.ALIGN_CASES' comment: the restatement ends 4e-5 .. 4e-4
    from itself when its moments move by 1e-12), so this run is held to the truth and to the invariants, not to the restatement's digits:
    converged, one round per outer iteration, and at least ten times closer to the truth than the guess in translation — the bar every
    ALIGN_CASES run passes on the CPU."""
    import lisreg
    r = gpu_ctx.gicp_align(SLOT, _pcl(world["src"]), lisreg.gicp_default_params(), world["guess"])
    et, er = R.pose_error(r["T"], world["T_true"])
    et0, er0 = R.pose_error(world["guess"], world["T_true"])
    print(f"[gicp] the family's scene: outer {r['iters']} inner {r['inner_iters']} evals {r['n_evals']} rounds {r['n_rounds']} delta "
          f"{r['last_delta']:.3f}; {1e3 * et:.2f} mm / {1e3 * er:.3f} mrad from the truth (guess {1e3 * et0:.0f} mm / {1e3 * er0:.1f} mrad)")
    assert r["converged"] and 2 <= r["iters"] == r["n_rounds"] <= 30 and r["n_pairs_last"] == len(world["src"]) and r["inner_exit"] in (0, 1, 2)
    assert r["inner_iters"] <= 20 * r["iters"] and r["n_evals"] >= 2 * r["inner_iters"] and (r["last_delta"] < 1.0 or r["iters"] == 30)
    assert et0 >= 10.0 * et and er0 >= 10.0 * er, (et, er, et0, er0)


@pytest.mark.gpu
def test_state_null_guess_repeat_calls_and_the_fastgicp_calls_around(gpu_ctx, world, scene_slot):
    """GICP shares the vg_* staging buffers and the evaluation buffers with FastGICP and its batch: their bits must not change"""
    import lisreg
    P = lisreg.gicp_default_params(kind=1)
    Pf = lisreg.fgicp_default_params()
    src = _pcl(world["src"])
    items = [lisreg.FgicpItem(0, SLOT, world["guess"]), lisreg.FgicpItem(0, SLOT, None)]

    def fastgicp():
        single = gpu_ctx.fgicp_align(SLOT, src, Pf, world["guess"], want_aligned=True)
        res, fit, info = gpu_ctx.fgicp_align_batch([src], items, Pf)
        return (single["T"].tobytes(), single["error"], single["lam"], single["n_evals"], single["aligned"].tobytes(),
                [(b["T"].tobytes(), b["error"], b["n_evals"]) for b in res], fit.tobytes(), info)
    before = fastgicp()
    a = gpu_ctx.gicp_align(SLOT, src, P, world["guess"], want_aligned=True)
    after = fastgicp()
    b = gpu_ctx.gicp_align(SLOT, src, P, world["guess"], want_aligned=True)
    assert before == after == fastgicp()
    assert _bits(a) == _bits(b) and a["aligned"].tobytes() == b["aligned"].tobytes() and a["converged"] and a["iters"] >= 2
    # a NULL guess is the identity
    moved = _pcl(_apply_f32(world["guess"], world["src"]))
    n0 = gpu_ctx.gicp_align(SLOT, moved, P, None)
    n1 = gpu_ctx.gicp_align(SLOT, moved, P, np.eye(4, dtype=np.float32))
    assert _bits(n0) == _bits(n1) and n0["iters"] >= 2 and n0["converged"]
    # the guess 100 m away: no pair, one round, the guess
    far = world["guess"].copy()
    far[0, 3] += 100.0
    r = gpu_ctx.gicp_align(SLOT, src, P, far)
    assert tuple(int(r[k]) for k in COUNT_KEYS) == (0, 0, 0, 0, 1, 0, -1) and r["error"] == 0.0 and np.array_equal(r["T"], far.astype(np.float64))


@pytest.mark.gpu
def test_twenty_calls_do_not_grow_device_memory(gpu_ctx, world, scene_slot):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = lisreg.gicp_default_params(max_iters=2)
    src = _pcl(world["src"])
    first = gpu_ctx.gicp_align(SLOT, src, P, world["guess"], want_aligned=True)          # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        r = gpu_ctx.gicp_align(SLOT, src, P, world["guess"], want_aligned=True)
    assert free_bytes() == before
    assert _bits(r) == _bits(first) and r["aligned"].tobytes() == first["aligned"].tobytes()
    assert (r["converged"], r["iters"], r["n_rounds"]) == (True, 2, 2) and r["last_delta"] >= 1.0     # the cap counts as converged (PCL 1.8)


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, world, scene_slot):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = lisreg.gicp_default_params()
    tgt, src = _pcl(world["tgt"][:2000]), _pcl(world["src"])

    def refused(fn, *words):
        with pytest.raises(lisreg.LisregError) as err:
            fn()
        assert err.value.code == lisreg.ERR_ARG, err.value
        for w in words:
            assert w in str(err.value), (w, str(err.value))
    for call in (lambda s, p: ctx.gicp_align(SLOT, s, p), lambda s, p: ctx.gicp_moments(SLOT, s, p, np.eye(4))):
        refused(lambda: call(src[:K - 1], P), "fewer finite points")
        refused(lambda: call(src[:0], P), "n <= 0")
        bad = src.copy(); bad["z"][3] = -np.inf
        refused(lambda: call(bad, P), "infinite")
        for v in (0.0, -1.0, float("nan")):
            refused(lambda: call(src, lisreg.gicp_default_params(max_correspondence_distance=v)), "max_correspondence_distance <= 0")
        for k in (3, 33):
            refused(lambda: call(src, lisreg.gicp_default_params(k_correspondences=k)), "outside 4 .. 32")
        for kw in (dict(transformation_epsilon=0.0), dict(rotation_epsilon=-1.0), dict(max_iters=0), dict(max_inner_iters=0),
                   dict(gicp_epsilon=0.0), dict(gicp_epsilon=1.5)):
            refused(lambda: call(src, lisreg.gicp_default_params(**kw)), "bad transformation_epsilon")
        for kw in (dict(rho=0.0), dict(sigma=1.0), dict(tau1=1.0), dict(tau2=0.0), dict(tau3=1.0), dict(step_size=0.0), dict(gradient_tol=0.0),
                   dict(order=4), dict(order=1)):
            refused(lambda: call(src, lisreg.gicp_default_params(**kw)), "bad rho")
    assert ctx.gicp_align(SLOT, src[:K], P, world["guess"])["n_rounds"] >= 1
    # the target is a FastGICP slot: the map-index, the NDT and the VGICP slots are other numberings
    ctx.map_index_set(SLOT + 5, tgt)
    ctx.ndt_set_target(SLOT + 5, tgt, lisreg.ndt_default_params())
    ctx.vgicp_set_target(SLOT + 5, tgt, lisreg.vgicp_default_params())
    for slot in (SLOT + 5, 4242, -1):
        refused(lambda: ctx.gicp_align(slot, src, P), "no FastGICP target")
        refused(lambda: ctx.gicp_moments(slot, src, P, np.eye(4)), "no FastGICP target")
    # a refused call leaves the result untouched
    vp = C.c_void_p
    sp, n, st = src.ctypes.data_as(vp), len(src), src.dtype.itemsize
    res = lisreg.GicpResult()
    C.memset(C.byref(res), 0x5a, C.sizeof(res))
    mark = bytes(res)
    out = np.zeros(74)
    dp = C.POINTER(C.c_double)
    assert L.lisreg_gicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, None, None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_align(ctx._h, SLOT, None, n, st, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_align(ctx._h, SLOT, sp, n, 8, lisreg.FMT_XYZI, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_align(ctx._h, 4242, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_gicp_align(ctx._h, SLOT, sp, K - 1, st, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert bytes(res) == mark
    assert L.lisreg_gicp_moments(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, out.ctypes.data_as(dp)) == lisreg.ERR_ARG
    assert L.lisreg_gicp_moments(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), np.eye(4).ctypes.data_as(dp), None) == lisreg.ERR_ARG
    assert not out.any()
    # the context and the scene's slot stay usable
    r, r2 = ctx.gicp_align(SLOT, src, P, world["guess"]), ctx.gicp_align(SLOT, src, P, world["guess"])
    assert r["converged"] and r["n_rounds"] == r["iters"] >= 2 and _bits(r) == _bits(r2)


import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


@pytest.mark.gpu
def test_alignment_on_a_callers_busy_stream(env, world):
    """the source arrives late on the caller's stream, as in tests/test_fgicp.py: the result equals the idle-stream one (and the
    restatement's), and a context left on its own stream reads the decoy"""
    e = env
    # a short alignment (one outer iteration of at most three BFGS steps), so that the call does not outlast the stall the gate sizes
    # from the idle call
    P = e.lisreg.gicp_default_params(max_iters=1, max_inner_iters=3)
    ref = R.align(world["T"], world["S"], R.params(max_iters=1, max_inner_iters=3), world["guess"])
    assert min(ref["decisions"].values()) >= 1e-6 and ref["margin_nn"] >= 1e-9 and ref["margin_cut"] >= 1e-9
    assert (ref["iters"], ref["inner_iters"], ref["n_rounds"], ref["converged"]) == (1, 3, 1, 1)
    e.ctx.fgicp_set_target(SLOT, _pcl(world["tgt"]), e.lisreg.fgicp_default_params())
    rs = _records(world["src"])
    guess = world["guess"]

    def make(dst):
        out = e.D(np.zeros_like(rs))

        def run():
            r = e.ctx.gicp_align(SLOT, (dst.ptr, len(rs)), P, guess, out_ptr=out.ptr)
            return dict(T=r["T"], counts=np.array([r["iters"], r["inner_iters"], r["n_evals"], r["n_pairs_last"]]), error=r["error"])
        return run, (lambda r: dict(res=r, aligned=TCS.to_host(out.ptr, rs.shape)))
    o, _ = TCS.late_case(e, "gicp_align (device records)", rs, TCS.moved(rs, small=True), make)
    assert list(o["res"]["counts"]) == [ref["iters"], ref["inner_iters"], ref["n_evals"], ref["n_pairs_last"]]
    assert np.abs(o["res"]["T"] - ref["T"]).max() <= 1e-6


@pytest.mark.gpu
def test_gicp_smoke_runs():
    exe = os.path.join(HOST, "gicp_smoke")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "gicp_smoke ok" in r.stdout, r.stdout + r.stderr
