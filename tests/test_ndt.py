"""lisreg_ndt_*: NDT registration on the GPU (lis-slam_amd/csrc/lisreg_ndt.hip) against its definition, tests/ndt_ref.py.

CPU: the structs and symbols of include/lisreg.h, the golden file regenerates from the restatement.  GPU: the voxels' Gaussians, one
evaluation of score / gradient / Hessian, whole alignments, the argument errors, device memory, a caller's busy stream.

The bounds (set where the feature was specified; every GPU test prints its figures before it asserts, profiles/ndt.md keeps them):
  means   within 1e-12 max|coordinate|;
  C^-1    within 1e-9 max|C^-1| per voxel (condition number <= 100 after the inflation; a few hundred roundings of 1.1e-16 give
          about 1e-12, the bar leaves three orders);
  each of the 28 sums within 1e-10 of the restatement's sum of |term| for that output (about 1e4 terms at 1.1e-16 each and a 2-ulp
          exp give about 1e-12: two orders), the pair counts equal, two calls bit-identical;
  alignments: iters, n_evals, converged equal, p within 1e-6 m / 1e-6 rad (four orders below transformation_epsilon, far above
          double rounding); line_search = 1 ends within 2 cm / 2 mrad of the true pose.  Only seeds whose smallest line-search /
          convergence decision margin exceeds 1e-6 in the restatement are used (checked on the CPU below)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ndt_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ndt", "ndt_cases.npz")
SYMBOLS = ("lisreg_ndt_default_params", "lisreg_ndt_set_target", "lisreg_ndt_align", "lisreg_ndt_get_voxels", "lisreg_ndt_derivatives")
SLOT = 7


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    """a ctypes mirror of `typedef struct name { ... } name;` parsed from include/lisreg.h"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"double": C.c_double, "int": C.c_int, "float": C.c_float, "long long": C.c_longlong}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"(long long|\w+)\s+(.*)", decl).groups()
        for n in names.split(","):
            m = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?", n)
            fields.append((m.group(1), types[t] * int(m.group(2)) if m.group(2) else types[t]))
    return type(name, (C.Structure,), {"_fields_": fields})


def test_structs_match_the_header():
    import lisreg
    for name, mine, size in (("lisreg_ndt_params", lisreg.NdtParams, 56), ("lisreg_ndt_info", lisreg.NdtInfo, 24),
                             ("lisreg_ndt_result", lisreg.NdtResult, 152)):
        theirs = _header_struct(name)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name
    assert [n for n, _ in lisreg.NdtParams._fields_] == ["resolution", "step_size", "transformation_epsilon", "outlier_ratio",
                                                         "min_covar_eigvalue_mult", "max_iters", "min_points_per_voxel", "line_search", "reserved"]


def test_library_exports_the_ndt_symbols_and_defaults():
    import lisreg
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lisreg.ABI_SYMBOLS, s
        assert re.search(r"^\s*int\s+%s\s*\(" % s, hdr, re.M), s
    p = lisreg.ndt_default_params()
    got = {n: getattr(p, n) for n, _ in p._fields_ if n != "reserved"}
    assert got == R.DEFAULTS
    assert L.lisreg_ndt_default_params(1, C.byref(p)) == lisreg.ERR_ARG and L.lisreg_ndt_default_params(0, None) == lisreg.ERR_ARG
    assert L.lisreg_ndt_set_target(None, 0, None, 0, 0, 0, C.byref(p), None) == lisreg.ERR_ARG
    assert L.lisreg_ndt_align(None, 0, None, 0, 0, 0, C.byref(p), None, None, None) == lisreg.ERR_ARG
    for text in ("registration.cpp:147-155", "subMapOptmizationNode.cpp:2756-2760", "the transform:", "the covariance normalisation:",
                 "the angle chart:", "the line-search flag:"):
        assert text in hdr, text


def test_golden_file_regenerates_from_the_restatement():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    now = R.golden_cases()
    assert sorted(now) == sorted(g.files)
    for k in g.files:
        a, b = g[k], now[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind in "iu":
            assert np.array_equal(a, b), k
    # doubles: LAPACK / BLAS builds may add in another order; everything else is the same arithmetic
    for k in ("planted_means", "scene_means", "planted_icov6", "scene_icov6", "deriv_p"):
        assert np.allclose(g[k], now[k], rtol=1e-11, atol=0), k
    assert np.all(np.abs(g["deriv_out"] - now["deriv_out"]) <= 1e-12 * g["deriv_abs"])
    assert np.allclose(g["deriv_abs"], now["deriv_abs"], rtol=1e-12, atol=0)
    assert np.allclose(g["align_p"][:, :6], now["align_p"][:, :6], rtol=0, atol=1e-8)
    assert np.allclose(g["align_absg"], now["align_absg"], rtol=1e-9, atol=0)
    assert np.all(np.abs(g["align_p"][:, 6] - now["align_p"][:, 6]) <= 1.01 * g["align_absg"] @ np.full(6, 1e-8) + 1e-10 * g["align_p"][:, 6])
    # what the GPU tests stand on
    assert list(g["scene_dims"]) == [23, 24, 14, 1821] and len(g["scene_cell_ids"]) == 1735
    assert list(g["align_counts"][:, 4]) == [735, 735, 734, 735]
    assert (g["align_p"][:, 7] > 1e-6).all()                               # no borderline decision in any of the four runs
    assert (g["align_counts"][:, 2] == 1).all()
    ls1 = [k for k, c in enumerate(R.ALIGN_CASES) if c[3] == 1]
    assert (g["align_p"][ls1, 8] < 0.02).all() and (g["align_p"][ls1, 9] < 0.002).all()
    pairs = g["deriv_pairs"].reshape(4, len(R.DERIV_SIZES), 2)
    assert (pairs[3] == 0).all() and (pairs[:3, -1] > 2000).all() and (pairs[:, :, 0] == pairs[:, :, 1]).all()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
def _pcl(xyz):
    from lisreg import synth
    return synth.to_pcl(np.ascontiguousarray(xyz, np.float32))


def _records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


@pytest.fixture(scope="module")
def world():
    """the scene, its restatement target and the golden file: made once, read by every test, never changed"""
    tgt, src, guess, T_true = R.scene()
    return dict(tgt=tgt, src=src, guess=guess, T_true=T_true, ref=R.build_target(tgt, R.params()), g=np.load(GOLDEN))


@pytest.fixture(scope="module")
def scene_slot(gpu_ctx, world):
    import lisreg
    info = gpu_ctx.ndt_set_target(SLOT, _pcl(world["tgt"]), lisreg.ndt_default_params())
    return info


def _check_voxels(V, T, cloud, what):
    assert np.array_equal(V["cell_ids"], T["cell_ids"]), (what, "valid set")
    assert np.array_equal(V["counts"], T["counts"]), (what, "counts")
    e_mean = np.max(np.abs(V["means"] - T["means"])) / np.nanmax(np.abs(cloud))
    ic = R.icov6(T["icov"])
    e_ic = np.max(np.max(np.abs(V["icov6"] - ic), 1) / np.max(np.abs(ic), 1))
    print(f"[ndt] {what}: {len(T['cell_ids'])} valid voxels, mean error / max|coordinate| {e_mean:.3e}, C^-1 error / max|C^-1| {e_ic:.3e}")
    assert e_mean <= 1e-12, (what, e_mean)
    assert e_ic <= 1e-9, (what, e_ic)


@pytest.mark.gpu
def test_voxels_of_the_scene(gpu_ctx, world, scene_slot):
    T, g = world["ref"], world["g"]
    assert scene_slot == dict(dims=[23, 24, 14], n_voxels=1821, n_valid=1735)
    V = gpu_ctx.ndt_get_voxels(SLOT)
    _check_voxels(V, T, world["tgt"], "scene")
    assert np.array_equal(V["cell_ids"], g["scene_cell_ids"]) and np.array_equal(V["counts"], g["scene_counts"])
    assert np.allclose(V["icov6"][::8], g["scene_icov6"], rtol=0, atol=1e-9 * np.abs(g["scene_icov6"]).max(1, keepdims=True))


@pytest.mark.gpu
def test_voxels_of_the_planted_cloud(gpu_ctx, world):
    """voxels of exactly 5 and 6 points, a coplanar and a collinear voxel (one and two eigenvalues raised), six identical points
    (rejected), NaN points, voxels of 24 / 25 / 48-and-more points (the lane and the wavefront form), one crowded voxel of 3000"""
    import lisreg
    g = world["g"]
    xyz = R.planted_cloud()
    T = R.build_target(xyz, R.params())
    for fmt in ("host", "device"):
        if fmt == "host":
            info = gpu_ctx.ndt_set_target(SLOT + 1, _pcl(xyz), lisreg.ndt_default_params())
        else:
            d = lisreg.DeviceArray(_records(xyz))
            info = gpu_ctx.ndt_set_target(SLOT + 1, (d.ptr, len(xyz)), lisreg.ndt_default_params())
        assert info == dict(dims=[5, 3, 3], n_voxels=10, n_valid=8), fmt
        V = gpu_ctx.ndt_get_voxels(SLOT + 1)
        _check_voxels(V, T, xyz, "planted, " + fmt)
        assert np.array_equal(V["cell_ids"], g["planted_cell_ids"]) and list(V["counts"]) == list(g["planted_counts"])
        assert {6, 9, 12, 24, 25, 40, 70, 3000} == set(V["counts"].tolist())
    # a looser requirement on the points per voxel takes the five-point voxel in, not the six identical points
    info = gpu_ctx.ndt_set_target(SLOT + 1, _pcl(xyz), lisreg.ndt_default_params(min_points_per_voxel=5))
    assert info["n_valid"] == 9


@pytest.mark.gpu
def test_one_evaluation(gpu_ctx, world, scene_slot):
    import lisreg
    g, src = world["g"], world["src"]
    P = lisreg.ndt_default_params()
    k, worst = 0, 0.0
    d_src = lisreg.DeviceArray(_records(src))
    for ip, p in enumerate(g["deriv_p"]):
        for n in R.DERIV_SIZES:
            m = n or len(src)
            for hess in (1, 0):
                want, wabs, wpairs = g["deriv_out"][k], g["deriv_abs"][k], int(g["deriv_pairs"][k])
                k += 1
                out, pairs = gpu_ctx.ndt_derivatives(SLOT, _pcl(src[:m]), P, p, bool(hess))
                again, _ = gpu_ctx.ndt_derivatives(SLOT, (d_src.ptr, m), P, p, bool(hess))
                assert pairs == wpairs, (ip, m, hess)
                assert out.tobytes() == again.tobytes(), (ip, m, hess, "two calls (host structs, device records) differ")
                err = np.abs(out - want)
                assert np.all(err <= 1e-10 * wabs), (ip, m, hess, err, wabs)
                if not hess:
                    assert not out[7:].any()
                if wpairs:
                    worst = max(worst, float(np.max(err[wabs > 0] / wabs[wabs > 0])))
                else:
                    assert not out.any()
    print(f"[ndt] one evaluation: worst |sum - restatement| / sum|term| over {k} cases {worst:.3e}")
    assert k == len(g["deriv_out"])


def _apply_f32(F, xyz):
    """transformPointCloud in float, products and sums rounded one by one (lisreg_transform_cloud)"""
    F = np.asarray(F, np.float32)
    x, y, z = (np.asarray(xyz[:, k], np.float32) for k in range(3))
    return np.stack([((F[r, 0] * x + F[r, 1] * y) + F[r, 2] * z) + F[r, 3] for r in range(3)], 1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(R.ALIGN_CASES)))
def test_alignment_equals_the_restatement(gpu_ctx, world, scene_slot, case):
    import lisreg
    seed, trans, rot, ls = R.ALIGN_CASES[case]
    g = world["g"]
    counts, want = g["align_counts"][case], g["align_p"][case]
    if seed == 1000:
        src, guess, T_true, slot = world["src"], world["guess"], world["T_true"], SLOT
    else:
        tgt, src, guess, T_true = R.scene(seed, trans, rot)
        slot = SLOT + 2
        gpu_ctx.ndt_set_target(slot, _pcl(tgt), lisreg.ndt_default_params())
    P = lisreg.ndt_default_params(line_search=ls)
    cloud = _pcl(src)
    r = gpu_ctx.ndt_align(slot, cloud, P, guess, want_aligned=True)
    dp = np.abs(r["p"] - want[:6])
    et, er = R.pose_error(r["T"], T_true)
    print(f"[ndt] align seed {seed} line_search {ls}: iters {r['iters']} evals {r['n_evals']} |dp| {dp.max():.3e}, {1e3 * et:.2f} mm / {1e3 * er:.3f} mrad from the truth")
    assert (r["iters"], r["n_evals"], int(r["converged"]), r["n_pairs_last"]) == tuple(int(v) for v in counts[:4])
    assert dp.max() <= 1e-6, dp
    # the score at a pose dp away differs by gradient . dp to first order: bounded by the restatement's sum of |term| of every gradient
    # entry at its final pose times |dp| (1 % over for the second order), plus the 1e-10 sum|term| of one evaluation (the score's terms
    # have one sign, so its sum of |term| is |score|)
    assert abs(r["score"] - want[6]) <= 1.01 * float(g["align_absg"][case] @ dp) + 1e-10 * abs(want[6])
    assert r["trans_probability"] == r["score"] / len(src)
    if ls == 1:
        assert et <= 0.02 and er <= 0.002
    assert np.array_equal(r["T"], R.matrix_from_p(r["p"]).astype(np.float32))
    # aligned_out = the source under final_transform; the other fields of the structs are the source's
    al = r["aligned"]
    got = np.stack([al["x"], al["y"], al["z"]], 1)
    assert np.array_equal(got.view(np.uint32), _apply_f32(r["T"], src).view(np.uint32))
    assert np.array_equal(al["intensity"], cloud["intensity"]) and np.array_equal(al["label"], cloud["label"])
    # device records give the same bits
    d_src, d_out = lisreg.DeviceArray(_records(src)), lisreg.DeviceArray(np.zeros((len(src), 4), np.float32))
    rd = gpu_ctx.ndt_align(slot, (d_src.ptr, len(src)), P, guess, out_ptr=d_out.ptr)
    assert rd["p"].tobytes() == r["p"].tobytes() and rd["T"].tobytes() == r["T"].tobytes() and rd["score"] == r["score"]
    assert (rd["iters"], rd["n_evals"], rd["converged"]) == (r["iters"], r["n_evals"], r["converged"])
    assert np.array_equal(lisreg.device_to_host(d_out.ptr, (len(src), 4), np.float32)[:, :3].view(np.uint32), got.view(np.uint32))


@pytest.mark.gpu
def test_null_guess_is_the_identity_and_no_pair_returns_the_guess(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.ndt_default_params()
    # the source moved into the map frame by the guess: aligning it from NULL and from the identity matrix is one computation
    moved = _apply_f32(world["guess"], world["src"])
    a = gpu_ctx.ndt_align(SLOT, _pcl(moved), P, None)
    b = gpu_ctx.ndt_align(SLOT, _pcl(moved), P, np.eye(4, dtype=np.float32))
    assert a["p"].tobytes() == b["p"].tobytes() and a["T"].tobytes() == b["T"].tobytes() and (a["iters"], a["n_evals"]) == (b["iters"], b["n_evals"])
    assert a["iters"] >= 2 and a["converged"]
    # a source with no pair at the guess: converged, no iteration, the guess comes back
    far = world["guess"].copy()
    far[0, 3] += 100.0
    r = gpu_ctx.ndt_align(SLOT, _pcl(world["src"]), P, far)
    assert (r["converged"], r["iters"], r["n_evals"], r["n_pairs_last"], r["score"]) == (True, 0, 1, 0, 0.0)
    assert np.allclose(r["T"], far, rtol=0, atol=1e-6) and np.array_equal(r["T"][:3, 3], far[:3, 3])      # the angles went through their chart


@pytest.mark.gpu
def test_argument_errors(gpu_ctx, world, scene_slot):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = lisreg.ndt_default_params()
    tgt, src = _pcl(world["tgt"][:2000]), _pcl(world["src"])
    res = lisreg.NdtResult()

    def refused(fn, *words):
        with pytest.raises(lisreg.LisregError) as err:
            fn()
        assert err.value.code == lisreg.ERR_ARG, err.value
        for w in words:
            assert w in str(err.value), (w, str(err.value))
    refused(lambda: ctx.ndt_set_target(SLOT + 3, tgt[:0], P), "n <= 0")
    refused(lambda: ctx.ndt_align(SLOT, src[:0], P), "n <= 0")
    refused(lambda: ctx.ndt_derivatives(SLOT, src[:0], P, np.zeros(6)), "n <= 0")
    bad = tgt.copy(); bad["y"][17] = np.inf
    refused(lambda: ctx.ndt_set_target(SLOT + 3, bad, P), "infinite")
    refused(lambda: ctx.ndt_set_target(SLOT + 3, tgt[:5], P), "no valid voxel")
    allnan = tgt[:50].copy(); allnan["x"] = np.nan
    refused(lambda: ctx.ndt_set_target(SLOT + 3, allnan, P), "no valid voxel")
    refused(lambda: ctx.ndt_set_target(SLOT + 3, tgt, lisreg.ndt_default_params(resolution=0.0)), "resolution <= 0")
    refused(lambda: ctx.ndt_set_target(SLOT + 3, tgt, lisreg.ndt_default_params(resolution=-1.0)), "resolution <= 0")
    refused(lambda: ctx.ndt_set_target(SLOT + 3, tgt, lisreg.ndt_default_params(resolution=0.01)), "2^26 cells")
    refused(lambda: ctx.ndt_align(SLOT, src, lisreg.ndt_default_params(resolution=0.5)), "resolution differs")
    refused(lambda: ctx.ndt_derivatives(SLOT, src, lisreg.ndt_default_params(resolution=2.0), np.zeros(6)), "resolution differs")
    refused(lambda: ctx.ndt_set_target(-1, tgt, P), "slot")
    refused(lambda: ctx.ndt_set_target(65536, tgt, P), "slot")
    # a slot that was refused, or never set, holds no target; the map-index slots are another numbering
    ctx.map_index_set(SLOT + 3, tgt)
    for slot in (SLOT + 3, 4242):
        with pytest.raises(lisreg.LisregError) as err:
            ctx.ndt_align(slot, src, P)
        assert err.value.code == lisreg.ERR_NO_TARGET
    assert L.lisreg_ndt_align(ctx._h, SLOT, src.ctypes.data_as(C.c_void_p), len(src), src.dtype.itemsize, lisreg.FMT_XYZIL, None, None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_ndt_align(ctx._h, SLOT, src.ctypes.data_as(C.c_void_p), len(src), src.dtype.itemsize, lisreg.FMT_XYZIL, C.byref(P), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_ndt_align(ctx._h, SLOT, None, len(src), src.dtype.itemsize, lisreg.FMT_XYZIL, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    assert L.lisreg_ndt_align(ctx._h, SLOT, src.ctypes.data_as(C.c_void_p), len(src), 8, lisreg.FMT_XYZI, C.byref(P), None, C.byref(res), None) == lisreg.ERR_ARG
    # the context and the scene's slot stay usable
    g = world["g"]
    r = ctx.ndt_align(SLOT, src, P, world["guess"])
    assert (r["iters"], r["n_evals"]) == (int(g["align_counts"][0][0]), int(g["align_counts"][0][1]))


@pytest.mark.gpu
def test_twenty_alignments_do_not_grow_device_memory(gpu_ctx, world, scene_slot):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = lisreg.ndt_default_params()
    src = _pcl(world["src"])
    first = gpu_ctx.ndt_align(SLOT, src, P, world["guess"], want_aligned=True)          # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        r = gpu_ctx.ndt_align(SLOT, src, P, world["guess"], want_aligned=True)
    assert free_bytes() == before
    assert r["p"].tobytes() == first["p"].tobytes() and r["aligned"].tobytes() == first["aligned"].tobytes()


import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


@pytest.mark.gpu
def test_alignment_on_a_callers_busy_stream(env, world):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the result equals the idle-stream one (and
    the restatement's), and a context left on its own stream reads the decoy"""
    e = env
    # a short alignment (three iterations of one clamped step each, four evaluations): each evaluation is two small launches and a
    # read-back that queue behind the gate's copies, and the default run's 18 of them outlast the stall the gate sizes from the idle call
    P = e.lisreg.ndt_default_params(max_iters=1, line_search=0)
    ref = R.align(world["ref"], world["src"], R.params(max_iters=1, line_search=0), world["guess"])
    assert ref["min_margin"] > 1e-6 and ref["iters"] == 3 and ref["n_evals"] == 4
    e.ctx.ndt_set_target(SLOT, _pcl(world["tgt"]), P)
    rs = _records(world["src"])
    guess = world["guess"]

    def make(dst):
        out = e.D(np.zeros_like(rs))

        def run():
            r = e.ctx.ndt_align(SLOT, (dst.ptr, len(rs)), P, guess, out_ptr=out.ptr)
            return dict(p=r["p"], T=r["T"], counts=np.array([r["iters"], r["n_evals"], r["n_pairs_last"]]), score=r["score"])
        return run, (lambda r: dict(res=r, aligned=TCS.to_host(out.ptr, rs.shape)))
    o, _ = TCS.late_case(e, "ndt_align (device records)", rs, TCS.moved(rs, small=True), make)
    assert list(o["res"]["counts"]) == [ref["iters"], ref["n_evals"], ref["n_pairs_last"]]
    assert np.abs(o["res"]["p"] - ref["p"]).max() <= 1e-6
    assert np.array_equal(o["aligned"][:, :3].view(np.uint32), _apply_f32(o["res"]["T"], world["src"]).view(np.uint32))
