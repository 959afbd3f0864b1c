"""lisreg_vgicp_params.neighbor_search: the voxel neighbourhoods DIRECT7 / DIRECT27 of VGICP on the GPU (lis-slam_amd/csrc/
lisreg_vgicp_lane.hpp) against their definition, tests/vgicp_nb_ref.py.  The CPU side (the restatement against itself and
against tests/vgicp_ref.py, the margins of the alignment cases, the census of the border cases, the struct) is tests/test_vgicp_nb_ref.py.

The bounds are the ones §7k set and tests/test_vgicp.py states (every test prints its figures before it asserts):
  the 28 sums      each within 1e-10 of the restatement's sum of |term|, pair counts equal, two calls bit-identical;
  alignments       converged, iters, n_evals, n_rejected, n_pairs_last equal, final_transform within 1e-6 entry-wise, error within 1e-6
                   relative.  Only cases whose smallest rho-sign and convergence margins exceed 1e-6 in the restatement are used (checked
                   on the CPU);
  batch            every field of every result equal to the single call's as raw bytes;
  DIRECT1          neighbor_search 0 and 1 give the same bytes, and the bytes of tests/golden/vgicp/vgicp_direct1_pin.npz, which the
                   library of the commit before the neighbourhoods wrote on an MI355X:

  python tests/test_vgicp_nb.py --write-pin [path]     (with the library to be pinned built in the tree; needs the GPU)"""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":                     # --write-pin: the paths tests/conftest.py gives to pytest
    sys.path[:0] = [os.path.join(ROOT, "lis-slam_amd"), os.path.join(ROOT, "oracle"), ROOT]

import vgicp_batch_ref as B  # noqa: E402
import vgicp_nb_ref as N  # noqa: E402
import vgicp_ref as R  # noqa: E402

PIN = os.path.join(ROOT, "tests", "golden", "vgicp", "vgicp_direct1_pin.npz")
SLOT = 50                                      # VGICP slots 50 ..: the scene, the flat target, scratch
FLAT, SCRATCH = SLOT + 1, SLOT + 2
BAD_MODES = (2, -1, 26, 28)


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
    """every field of a result as raw bytes"""
    return (r["T"].tobytes(), int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"],
            struct.pack("d", r["error"]), struct.pack("d", r["lam"]))


def _raw_align(ctx, slot, cloud, P, guess):
    """the bytes of the lisreg_vgicp_result of one alignment"""
    import lisreg
    res = lisreg.VgicpResult()
    g = np.ascontiguousarray(guess, np.float32).ravel()
    rc = lisreg.lib().lisreg_vgicp_align(ctx._h, slot, cloud.ctypes.data_as(C.c_void_p), len(cloud), cloud.dtype.itemsize, lisreg.FMT_XYZIL,
                                         C.byref(P), g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), None)
    assert rc == lisreg.OK, rc
    return bytes(res)


def _pin_now(ctx, slot):
    """what the pin holds: the result bytes of lisreg_vgicp_align and the 28 doubles and the pair count of lisreg_vgicp_linearize on the
    scene from its guess, with the default parameters (the slot holds the scene's target)"""
    import lisreg
    W = R.world()
    P = lisreg.vgicp_default_params()
    src = _pcl(W["src"])
    out, pairs = ctx.vgicp_linearize(slot, src, P, W["guess"].astype(np.float64), True)
    return dict(align=np.frombuffer(_raw_align(ctx, slot, src, P, W["guess"]), np.uint8), lin=out, pairs=np.int64(pairs))


@pytest.fixture(scope="module")
def world():
    """the scene, its restatement target and source and the golden file: made once, read by every test, never changed"""
    W = dict(R.world())
    W["g"] = np.load(N.GOLDEN)
    return W


@pytest.fixture(scope="module")
def scene_slot(gpu_ctx, world):
    """the target is built with neighbor_search 0: a slot serves every neighbourhood"""
    import lisreg
    return gpu_ctx.vgicp_set_target(SLOT, _pcl(world["tgt"]), lisreg.vgicp_default_params())


@pytest.fixture(scope="module")
def flat_slot(gpu_ctx):
    import lisreg
    F = N.flat_world()
    info = gpu_ctx.vgicp_set_target(FLAT, _pcl(F["tgt"]), lisreg.vgicp_default_params())
    assert info["dims"][2] == 1 and info["dims"] == [int(v) for v in F["T"]["dims"]] and info["n_voxels"] == len(F["T"]["cell_ids"])
    return info


def _check_sums(ctx, slot, cloud, P, T, hess, ev, tag):
    """one linearisation, host structs and device records, against the restatement's evaluation ev; returns the worst relative error"""
    import lisreg
    d_src = lisreg.DeviceArray(_records(cloud))
    out, pairs = ctx.vgicp_linearize(slot, _pcl(cloud), P, T, bool(hess))
    again, pairs2 = ctx.vgicp_linearize(slot, (d_src.ptr, len(cloud)), P, T, bool(hess))
    assert pairs == pairs2 == ev["n_pairs"], (tag, pairs, pairs2, ev["n_pairs"])
    assert out.tobytes() == again.tobytes(), (tag, "two calls (host structs, device records) differ")
    err = np.abs(out - ev["out"])
    assert np.all(err <= 1e-10 * ev["abs"]), (tag, err, ev["abs"])
    if not hess:
        assert not out[7:].any(), tag
    if not ev["n_pairs"]:
        assert not out.any(), tag
        return 0.0
    return float(np.max(err[ev["abs"] > 0] / ev["abs"][ev["abs"] > 0]))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", N.NB_MODES)
def test_one_linearisation(gpu_ctx, world, scene_slot, mode):
    import lisreg
    g = world["g"]
    P = lisreg.vgicp_default_params(neighbor_search=mode)
    cut = N.lin_sources()
    assert all(S["dist"]["eig_gap"].min() >= 1e-3 and S["dist"]["gap"].min() >= 1e-6 for _, S in cut.values())
    per_mode = len(g["lin_out"]) // len(N.NB_MODES)
    k, worst = N.NB_MODES.index(mode) * per_mode, 0.0
    for ip, T in enumerate(g["lin_T"]):
        for n in R.LIN_SIZES:
            for hess in (1, 0):
                ev = dict(out=g["lin_out"][k], abs=g["lin_abs"][k], n_pairs=int(g["lin_pairs"][k]))
                k += 1
                assert (ev["n_pairs"] > 0) == (ip < 2)
                worst = max(worst, _check_sums(gpu_ctx, SLOT, cut[n][0], P, T, hess, ev, (mode, ip, n, hess)))
    print(f"[vgicp_nb] mode {mode}, one linearisation: worst |sum - restatement| / sum|term| over {per_mode} cases {worst:.3e}; "
          f"pairs of the whole source at the guess {int(g['lin_pairs'][N.NB_MODES.index(mode) * per_mode + 2 * len(R.LIN_SIZES) - 2])}")
    assert k == (N.NB_MODES.index(mode) + 1) * per_mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", N.NB_MODES)
def test_grid_borders(gpu_ctx, world, scene_slot, flat_slot, mode):
    """the source one and two cells outside the grid beyond each face; a target one voxel thick; a pose 200 m off; NaN coordinates"""
    import lisreg
    P = lisreg.vgicp_default_params(neighbor_search=mode)
    T0 = world["guess"].astype(np.float64)
    worst = 0.0
    for name, T in N.border_poses(world["T"], world["S"], T0).items():
        c = N.census(world["T"], world["S"], T, mode)
        assert c["outside_pairing"] > 0 and c["inside_clipped"] > 0
        for hess in (1, 0):
            ev = N.linearize(world["T"], world["S"], T, mode, bool(hess))
            assert ev["n_pairs"] == c["pairs"]
            worst = max(worst, _check_sums(gpu_ctx, SLOT, world["src"], P, T, hess, ev, (mode, name, hess)))
        print(f"[vgicp_nb] mode {mode} border {name}: {c}")
    F = N.flat_world()
    xyz, S_nan = N.nan_source()
    for tag, slot, tgt, cloud, S, T in (("flat target", FLAT, F["T"], world["src"], world["S"], T0),
                                        ("NaN coordinates", SLOT, world["T"], xyz, S_nan, T0),
                                        ("200 m off", SLOT, world["T"], world["src"], world["S"], N.far_pose(T0))):
        for hess in (1, 0):
            ev = N.linearize(tgt, S, T, mode, bool(hess))
            worst = max(worst, _check_sums(gpu_ctx, slot, cloud, P, T, hess, ev, (mode, tag, hess)))
        print(f"[vgicp_nb] mode {mode} {tag}: pairs {ev['n_pairs']}")
        assert (ev["n_pairs"] == 0) == (tag == "200 m off")
    print(f"[vgicp_nb] mode {mode} grid borders: worst |sum - restatement| / sum|term| {worst:.3e}")
    # no pair at the guess: zeros, the guess returned, not converged
    far = world["guess"].copy()
    far[0, 3] += 200.0
    r = gpu_ctx.vgicp_align(SLOT, _pcl(world["src"]), P, far)
    assert (r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], r["error"]) == (False, 0, 1, 0, 0, 0.0)
    assert np.array_equal(r["T"], far.astype(np.float64))
    # a source with NaN points: they form no pair and do not reach T
    holes = world["src"].copy()
    holes[::7] = np.nan
    r = gpu_ctx.vgicp_align(SLOT, _pcl(holes), P, world["guess"], want_aligned=True)
    assert np.isfinite(r["T"]).all() and r["iters"] >= 1 and r["n_pairs_last"] > len(holes)
    assert np.isnan(r["aligned"]["x"][::7]).all() and np.isfinite(np.delete(r["aligned"]["x"], np.s_[::7])).all()


_TARGETS = {}


def _slot_of(ctx, tgt):
    """the slot of a target cloud, built once per process (the scenes of the alignment cases share few submaps)"""
    import lisreg
    key = tgt.tobytes()
    if key not in _TARGETS:
        _TARGETS[key] = SCRATCH + 1 + len(_TARGETS)
        ctx.vgicp_set_target(_TARGETS[key], _pcl(tgt), lisreg.vgicp_default_params())
    return _TARGETS[key]


@pytest.mark.gpu
@pytest.mark.parametrize("run", range(len(N.ALIGN_RUNS)), ids=[f"case{k}-mode{m}" for k, m in N.ALIGN_RUNS])
def test_alignment_equals_the_restatement(gpu_ctx, world, run):
    import lisreg
    case, mode = N.ALIGN_RUNS[run]
    g = world["g"]
    counts, want, fig = g["align_counts"][run], g["align_T"][run], g["align_fig"][run]
    assert (int(counts[6]), int(counts[7])) == (case, mode) and fig[2] > 1e-6 and fig[3] > 1e-6
    coarse = case == len(R.ALIGN_CASES)
    seed, trans, rot, eps = (*N.COARSE, R.DEFAULTS["transformation_epsilon"]) if coarse else R.ALIGN_CASES[case]
    tgt, src, guess, T_true = R.scene(seed, trans, rot)
    slot = _slot_of(gpu_ctx, tgt)
    P = lisreg.vgicp_default_params(transformation_epsilon=eps, neighbor_search=mode)
    cloud = _pcl(src)
    r = gpu_ctx.vgicp_align(slot, cloud, P, guess, want_aligned=True)
    dT = np.abs(r["T"] - want).max()
    et, er = R.pose_error(r["T"], T_true)
    print(f"[vgicp_nb] align seed {seed} guess {trans} m / {rot} deg eps {eps} mode {mode}: converged {r['converged']} iters {r['iters']} "
          f"evals {r['n_evals']} rejected {r['n_rejected']} pairs {r['n_pairs_last']} |dT| {dT:.3e}, {1e3 * et:.2f} mm / {1e3 * er:.3f} mrad "
          f"from the truth")
    assert (int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"]) == tuple(int(v) for v in counts[:5])
    assert dT <= 1e-6, dT
    assert abs(r["error"] - fig[0]) <= 1e-6 * fig[0]
    assert np.isfinite(r["T"]).all() and np.array_equal(r["T"][3], [0, 0, 0, 1])
    assert r["n_pairs_last"] > len(src)                                   # pairs, not points
    if coarse:
        # the guess a loop closure really produces: DIRECT27 ends on the truth where DIRECT1 reports convergence metres away
        r1 = gpu_ctx.vgicp_align(slot, cloud, lisreg.vgicp_default_params(), guess)
        e1 = R.pose_error(r1["T"], T_true)[0]
        print(f"[vgicp_nb] the same input with DIRECT1: converged {r1['converged']}, {1e3 * e1:.1f} mm from the truth")
        assert et <= 0.010, et
        assert r1["converged"] and e1 > 1.0
    # aligned_out = the source under final_transform rounded to float; the other fields of the structs are the source's
    al = r["aligned"]
    got = np.stack([al["x"], al["y"], al["z"]], 1)
    assert np.array_equal(got.view(np.uint32), _apply_f32(r["T"].astype(np.float32), src).view(np.uint32))
    assert np.array_equal(al["intensity"], cloud["intensity"]) and np.array_equal(al["label"], cloud["label"])
    # device records give the same bits
    d_src, d_out = lisreg.DeviceArray(_records(src)), lisreg.DeviceArray(np.zeros((len(src), 4), np.float32))
    rd = gpu_ctx.vgicp_align(slot, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    assert _bits(rd) == _bits(r)
    assert np.array_equal(lisreg.device_to_host(d_out.ptr, (len(src), 4), np.float32)[:, :3].view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", N.NB_MODES)
def test_batch_equals_single_calls(gpu_ctx, world, scene_slot, flat_slot, mode):
    """three items over two sources and two slots, one of them without a pair at its guess"""
    import lisreg
    P = lisreg.vgicp_default_params(neighbor_search=mode)
    far = world["guess"].copy()
    far[0, 3] += 200.0
    moved = _apply_f32(world["guess"], world["src"])                      # the source already at the guess: a NULL guess aligns it
    clouds = [world["src"], moved]
    sources = [_pcl(c) for c in clouds]
    targets = {SLOT: world["tgt"], FLAT: N.flat_world()["tgt"]}
    items = [lisreg.VgicpItem(0, SLOT, world["guess"]), lisreg.VgicpItem(0, SLOT, far), lisreg.VgicpItem(1, FLAT, None)]
    res, fit, info = gpu_ctx.vgicp_align_batch(sources, items, P)
    alone = [gpu_ctx.vgicp_align(it.slot, sources[it.source], P, None if it.guess is None else it.guess.reshape(4, 4)) for it in items]
    diff = [k for k, (a, b) in enumerate(zip(res, alone)) if _bits(a) != _bits(b)]
    res2, fit2, info2 = gpu_ctx.vgicp_align_batch(sources, items, P)
    evals = [r["n_evals"] for r in res]
    print(f"[vgicp_nb] batch mode {mode}: evaluations {evals}, pairs {[r['n_pairs_last'] for r in res]}, rounds {info['n_rounds']}, items "
          f"differing from the single calls {diff}, fitness {fit.tolist()}, best {info['best']}")
    assert not diff, diff
    assert fit.tobytes() == fit2.tobytes() and [_bits(r) for r in res2] == [_bits(r) for r in res] and info2 == info
    assert info["n_rounds"] == max(evals) and info["n_sources_staged"] == 2
    r = res[1]
    assert (r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], r["error"]) == (False, 0, 1, 0, 0, 0.0)
    assert np.array_equal(r["T"], far.astype(np.float64))
    assert res[0]["converged"] and res[0]["n_pairs_last"] > len(world["src"]) and res[2]["n_pairs_last"] > 0
    # the fitness pass does not depend on the mode: the scores of the restatement at the returned transforms, and the bytes of a DIRECT1
    # batch that is held at the same transforms (no iteration allowed)
    want = np.array([B.fitness(targets[it.slot], clouds[it.source], r["T"]) for it, r in zip(items, res)])
    rel = np.abs(fit - want) / want
    print(f"[vgicp_nb] batch mode {mode}: worst fitness error {rel.max():.3e} relative")
    assert rel.max() <= 1e-10, rel
    held = [lisreg.VgicpItem(it.source, it.slot, r["T"].astype(np.float32)) for it, r in zip(items, res)]
    resm, fitm, _ = gpu_ctx.vgicp_align_batch(sources, held, lisreg.vgicp_default_params(max_iters=0, neighbor_search=mode))
    res1, fit1, _ = gpu_ctx.vgicp_align_batch(sources, held, lisreg.vgicp_default_params(max_iters=0))
    assert [a["T"].tobytes() for a in resm] == [a["T"].tobytes() for a in res1] and fitm.tobytes() == fit1.tobytes()
    assert all(a["n_pairs_last"] >= b["n_pairs_last"] for a, b in zip(resm, res1)) and resm[0]["n_pairs_last"] > res1[0]["n_pairs_last"]
    # the `best` rule
    conv = [x["converged"] for x in res]
    assert info["best"] == B.best(conv, fit) and info["best"] in (0, 2)


@pytest.mark.gpu
def test_direct1_is_untouched(gpu_ctx, world, scene_slot):
    """neighbor_search 0 and 1 are one code path, and it returns the bytes the library returned before it knew neighbourhoods"""
    import lisreg
    src = _pcl(world["src"])
    P0, P1 = lisreg.vgicp_default_params(), lisreg.vgicp_default_params(neighbor_search=1)
    assert (P0.neighbor_search, P1.neighbor_search) == (0, 1)
    T = world["guess"].astype(np.float64)
    for hess in (True, False):
        a, pa = gpu_ctx.vgicp_linearize(SLOT, src, P0, T, hess)
        b, pb = gpu_ctx.vgicp_linearize(SLOT, src, P1, T, hess)
        assert a.tobytes() == b.tobytes() and pa == pb <= len(src)
    assert _raw_align(gpu_ctx, SLOT, src, P0, world["guess"]) == _raw_align(gpu_ctx, SLOT, src, P1, world["guess"])
    items = [lisreg.VgicpItem(0, SLOT, world["guess"]), lisreg.VgicpItem(0, SLOT, None)]
    r0, f0, i0 = gpu_ctx.vgicp_align_batch([src], items, P0)
    r1, f1, i1 = gpu_ctx.vgicp_align_batch([src], items, P1)
    assert [_bits(r) for r in r0] == [_bits(r) for r in r1] and f0.tobytes() == f1.tobytes() and i0 == i1
    pin, now = np.load(PIN), _pin_now(gpu_ctx, SLOT)
    print(f"[vgicp_nb] DIRECT1 pin: align bytes differing {(pin['align'] != now['align']).sum()} of {len(pin['align'])}, sums differing "
          f"{(pin['lin'].view(np.uint64) != now['lin'].view(np.uint64)).sum()} of 28, pairs {int(pin['pairs'])} / {int(now['pairs'])}")
    assert pin["align"].tobytes() == now["align"].tobytes()
    assert pin["lin"].tobytes() == now["lin"].tobytes() and int(pin["pairs"]) == int(now["pairs"])


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, world, scene_slot):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    src, tgt = _pcl(world["src"]), _pcl(world["tgt"][:2000])
    d_tgt = lisreg.DeviceArray(_records(world["tgt"][:2000]))
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    sp, n, st = src.ctypes.data_as(vp), len(src), src.dtype.itemsize
    T = np.ascontiguousarray(world["guess"], np.float64)

    def message(word="neighbor_search"):
        msg = L.lisreg_last_error(ctx._h).decode()
        assert word in msg, msg
    assert ctx.vgicp_set_target(SCRATCH, tgt, lisreg.vgicp_default_params())["n_points"] == 2000
    before = ctx.vgicp_get_voxels(SCRATCH)
    for bad in BAD_MODES:
        P = lisreg.vgicp_default_params(neighbor_search=bad)
        res = lisreg.VgicpResult()
        C.memset(C.byref(res), 0xAB, C.sizeof(res))
        out_al = np.full(len(src), 7, np.uint8)
        assert L.lisreg_vgicp_align(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
        message()
        assert bytes(res) == b"\xab" * C.sizeof(res) and (out_al == 7).all()
        out, pairs = np.full(28, -7.0), C.c_longlong(-7)
        assert L.lisreg_vgicp_linearize(ctx._h, SLOT, sp, n, st, lisreg.FMT_XYZIL, C.byref(P), T.ctypes.data_as(dp), 1, out.ctypes.data_as(dp),
                                        C.byref(pairs)) == lisreg.ERR_ARG
        message()
        assert (out == -7.0).all() and pairs.value == -7
        ptrs, ns = (vp * 1)(sp), (C.c_int * 1)(n)
        its = (lisreg.VgicpItemC * 1)()
        its[0].source, its[0].slot, its[0].guess = 0, SLOT, None
        resb = (lisreg.VgicpResult * 1)()
        C.memset(resb, 0xAB, C.sizeof(resb))
        fit, info = np.full(1, -7.0), lisreg.VgicpBatchInfo()
        assert L.lisreg_vgicp_align_batch(ctx._h, ptrs, ns, 1, st, lisreg.FMT_XYZIL, its, 1, C.byref(P), resb, fit.ctypes.data_as(dp),
                                          C.byref(info)) == lisreg.ERR_ARG
        message()
        assert bytes(resb) == b"\xab" * C.sizeof(resb) and fit[0] == -7.0 and info.best == -1
        # the calls that build a target check the field too, and a refused build leaves the slot as it was
        info_t = lisreg.VgicpInfo()
        C.memset(C.byref(info_t), 0xAB, C.sizeof(info_t))
        assert L.lisreg_vgicp_set_target(ctx._h, SCRATCH, tgt.ctypes.data_as(vp), len(tgt), tgt.dtype.itemsize, lisreg.FMT_XYZIL, C.byref(P),
                                         C.byref(info_t)) == lisreg.ERR_ARG
        message()
        assert bytes(info_t) == b"\xab" * C.sizeof(info_t)
        with pytest.raises(lisreg.LisregError) as err:
            ctx.vgicp_set_target_batch([(SCRATCH, (d_tgt.ptr, 2000))], P)
        assert err.value.code == lisreg.ERR_ARG and "neighbor_search" in str(err.value), err.value
        after = ctx.vgicp_get_voxels(SCRATCH)
        assert all(np.array_equal(before[k], after[k]) for k in before), bad
    # a slot built with neighbor_search 0, 7 or 27 is the same slot, and a DIRECT27 alignment accepts each
    P27 = lisreg.vgicp_default_params(neighbor_search=27)
    want = _bits(ctx.vgicp_align(SCRATCH, src, P27, world["guess"]))
    for mode in (7, 27):
        ctx.vgicp_set_target(SCRATCH, tgt, lisreg.vgicp_default_params(neighbor_search=mode))
        after = ctx.vgicp_get_voxels(SCRATCH)
        assert all(a.tobytes() == after[k].tobytes() for k, a in before.items()), mode
        assert _bits(ctx.vgicp_align(SCRATCH, src, P27, world["guess"])) == want, mode
    job = ctx.vgicp_set_target_batch([(SCRATCH, (d_tgt.ptr, 2000))], P27)
    assert job[0]["status"] == lisreg.OK and _bits(ctx.vgicp_align(SCRATCH, src, P27, world["guess"])) == want


import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


@pytest.mark.gpu
def test_direct27_alignment_on_a_callers_busy_stream(env, world):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the result equals the idle-stream one (and
    the restatement's), and a context left on its own stream reads the decoy"""
    e = env
    # a short alignment (one outer iteration: the linearisation and one accepted trial), so that the call does not outlast the stall the
    # gate sizes from the idle call
    P = e.lisreg.vgicp_default_params(max_iters=1, neighbor_search=27)
    ref = N.align(world["T"], world["S"], R.params(max_iters=1), 27, world["guess"])
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
    o, _ = TCS.late_case(e, "vgicp_align, DIRECT27 (device records)", rs, TCS.moved(rs, small=True), make)
    assert list(o["res"]["counts"]) == [ref["iters"], ref["n_evals"], ref["n_pairs_last"]] and ref["n_pairs_last"] > len(rs)
    assert np.abs(o["res"]["T"] - ref["T"]).max() <= 1e-6
    assert np.array_equal(o["aligned"][:, :3].view(np.uint32), _apply_f32(o["res"]["T"].astype(np.float32), world["src"]).view(np.uint32))


if __name__ == "__main__":
    # the few lines that made the pin: run with the library of the commit to be pinned built in the tree, on the GPU
    if sys.argv[1:2] == ["--write-pin"]:
        import lisreg
        path = sys.argv[2] if len(sys.argv) > 2 else PIN
        ctx = lisreg.Context(0)
        ctx.vgicp_set_target(SLOT, _pcl(R.world()["tgt"]), lisreg.vgicp_default_params())
        pin = _pin_now(ctx, SLOT)
        ctx.close()
        np.savez_compressed(path, **pin)
        print("wrote", path, os.path.getsize(path), "bytes; pairs", int(pin["pairs"]), "error", pin["lin"][0])
    else:
        print(__doc__)
