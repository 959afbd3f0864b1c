"""lisreg_gicp_align_batch: PCL's GICP verification of a candidate list as one call (lis-slam_amd/csrc/lisreg_gicp_batch.hip, DESIGN.md
§7r) against single lisreg_gicp_align calls and against its definition, tests/gicp_batch_ref.py.  The CPU side (the structs, the
stepper check, the restatement, the one home of the outer loop and of the lane body) is tests/test_gicp_batch_host.py.

The bounds (set where the feature was specified; every test prints its figures before it asserts):
  against single calls   every lisreg_gicp_result equal as raw bytes (all 176 of them), under the default parameters, kind 1 and
                         max_iters = 1; n_rounds == the largest n_rounds of the items; results, fitness and info bit-identical between
                         two batch calls.  §7q's finding is that a GICP run amplifies 1e-12 in a moment to 1e-4 in the pose: a batch
                         that is "close" to the single call is not a batch of single calls, so nothing here has a tolerance;
  against the restatement   fitness within 1e-10 relative of gicp_batch_ref.fitness at the returned final_transform (a sum of positive
                         terms: the project's sum bar, tests/test_fgicp_batch.py); `best` equal to gicp_batch_ref.best on the returned
                         (converged, fitness).  The alignments themselves are held to the restatement by tests/test_gicp.py (single
                         call) and to the single call by bytes here: no line-search decision is compared a second time;
  against the parent     lisreg_gicp_align and lisreg_gicp_moments equal, as bytes, to what the commit before the batch form wrote into
                         tests/golden/gicp_batch/gicp_parent_outputs.npz (lisreg_gicp_align now runs over GicpStepper).

Shapes (tests/gicp_batch_ref.py holds them): the scene gicp_ref.world(1000, 0.05, 0.3) — target 25 401 points, source 2 939, a guess
tests/test_gicp_ref.py qualifies as stable — and the target of world(1001, 0.02, 0.1) in a second slot; cuts src[::len(src) // ns][:ns]
of 63 (a wavefront short by a lane), 65 (one lane into a second), 129 and 20 (the k_correspondences limit) points, the 129 with three
NaN records (one of them lane 0 of the second wavefront), a guess 100 m off and a source index no item names, passed as NULL.  The
single calls run these in 4 / 4 / 8 / 7 / 9 / 4 / 8 / 1 rounds: the items of a batch finish in five different rounds."""
import ctypes as C
import os

import numpy as np
import pytest

import gicp_batch_ref as B
import gicp_ref as R
import test_caller_stream as TCS
import test_ndt_batch as TNB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
PARENT = os.path.join(ROOT, "tests", "golden", "gicp_batch", "gicp_parent_outputs.npz")
env = TCS.env
ndt_shapes = TNB.shapes
SA, SB, SE, SCUT = 180, 181, 182, 186                   # FastGICP slots: the two scenes, the four edge targets (SE ..), the cut-off target
SLOT_OF = {B.A: SA, B.B: SB}


def _pcl(xyz):
    from lisreg import synth
    return synth.to_pcl(np.ascontiguousarray(xyz, np.float32))


def _records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def _raw_batch(ctx, sources, items, P, want_fitness=True):
    """the raw call: (return code, the results as one bytes object per item, fitness array, info dict)"""
    import lisreg
    L = lisreg.lib()
    vp = C.c_void_p
    stride = next(s.dtype.itemsize for s in sources if s is not None)
    ptrs = (vp * max(len(sources), 1))(*[None if s is None else s.ctypes.data_as(vp) for s in sources])
    ns = (C.c_int * max(len(sources), 1))(*[0 if s is None else len(s) for s in sources])
    its = (lisreg.GicpItemC * max(len(items), 1))()
    for k, it in enumerate(items):
        its[k].source, its[k].slot = it.source, it.slot
        its[k].guess = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
    res = (lisreg.GicpResult * max(len(items), 1))()
    fit = np.full(max(len(items), 1), -7.0)
    info = lisreg.GicpBatchInfo()
    rc = L.lisreg_gicp_align_batch(ctx._h, ptrs, ns, len(sources), stride, lisreg.FMT_XYZIL, its, len(items), C.byref(P), res,
                                   fit.ctypes.data_as(C.POINTER(C.c_double)) if want_fitness else None, C.byref(info))
    size = C.sizeof(lisreg.GicpResult)
    return rc, [bytes(res)[k * size:(k + 1) * size] for k in range(len(items))], fit[:len(items)], \
        dict(best=info.best, n_rounds=info.n_rounds, n_sources_staged=info.n_sources_staged)


def _raw_single(ctx, it, source, P):
    import lisreg
    res = lisreg.GicpResult()
    g = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
    rc = lisreg.lib().lisreg_gicp_align(ctx._h, it.slot, source.ctypes.data_as(C.c_void_p), len(source), source.dtype.itemsize, lisreg.FMT_XYZIL,
                                        C.byref(P), g, C.byref(res), None)
    assert rc == lisreg.OK, lisreg.lib().lisreg_last_error(ctx._h)
    return bytes(res)


def _parse(raw):
    import lisreg
    return [lisreg.GicpResult.from_buffer_copy(b) for b in raw]


def _params(name):
    import lisreg
    kind, kw = next((k, o) for n, k, o in B.PARAM_SETS if n == name)
    return lisreg.gicp_default_params(kind, **kw)


@pytest.fixture(scope="module")
def shapes(gpu_ctx):
    """targets in their slots, the sources (xyz and PCL structs), the guesses and the batch of eight's items: made once, never changed"""
    import lisreg
    sh = B.scene_shapes()
    Pf = lisreg.fgicp_default_params()                   # a GICP target is a FastGICP slot (k 20, plane_epsilon = gicp_epsilon = 1e-3)
    for k, t in enumerate(sh["tgt"]):
        assert gpu_ctx.fgicp_set_target(SLOT_OF[k], _pcl(t), Pf)["n_points"] == 25401
    items = [lisreg.GicpItem(s, SLOT_OF[slot], sh[g]) for s, slot, g in B.EIGHT]
    return dict(tgt={SA: sh["tgt"][0], SB: sh["tgt"][1]}, xyz=sh["xyz"], pcl=[None if x is None else _pcl(x) for x in sh["xyz"]],
                guess=sh["guess"], far=sh["far"], items=items, T_true=sh["T_true"])


@pytest.fixture(scope="module")
def eight(gpu_ctx, shapes):
    """the batch of eight and its eight single calls under the three parameter sets: computed once, read by the tests below"""
    import lisreg
    out = {}
    for name, _, _ in B.PARAM_SETS:
        P = _params(name)
        rc, raw, fit, info = _raw_batch(gpu_ctx, shapes["pcl"], shapes["items"], P)
        assert rc == lisreg.OK, lisreg.lib().lisreg_last_error(gpu_ctx._h)
        alone = [_raw_single(gpu_ctx, it, shapes["pcl"][it.source], P) for it in shapes["items"]]
        out[name] = dict(P=P, raw=raw, fit=fit, info=info, alone=alone)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n, _, _ in B.PARAM_SETS])
def test_a_batch_of_eight_items_equals_the_single_calls(gpu_ctx, shapes, eight, name):
    import lisreg
    e = eight[name]
    items, srcs = shapes["items"], shapes["pcl"]
    diff = [k for k, (a, b) in enumerate(zip(e["raw"], e["alone"])) if a != b]
    res = _parse(e["raw"])
    rounds = [r.n_rounds for r in res]
    rc, raw2, fit2, info2 = _raw_batch(gpu_ctx, srcs, items, e["P"])
    print(f"[gicp_batch] {name}: rounds {rounds}, outer iterations {[r.iters for r in res]}, converged {[r.converged for r in res]}, pairs "
          f"{[r.n_pairs_last for r in res]}, batch rounds {e['info']['n_rounds']}, sources staged {e['info']['n_sources_staged']}, items differing "
          f"from the single calls {diff}, best {e['info']['best']}, fitness {e['fit'].tolist()}")
    assert C.sizeof(lisreg.GicpResult) == 176 and all(len(b) == 176 for b in e["raw"])
    assert not diff, diff
    assert rc == lisreg.OK and raw2 == e["raw"] and fit2.tobytes() == e["fit"].tobytes() and info2 == e["info"]
    assert e["info"]["n_rounds"] == max(rounds), (rounds, e["info"])
    assert e["info"]["n_sources_staged"] == 6                            # the seven sources less the one nobody names
    far = res[B.FAR_ITEM]
    assert (far.converged, far.iters, far.n_rounds, far.n_pairs_last, far.inner_exit) == (0, 0, 1, 0, -1)
    assert np.array_equal(np.array(list(far.final_transform)).reshape(4, 4), shapes["far"].astype(np.float64))
    if name == "cap1":                                                   # the cap ends every item that has pairs after one round, converged
        assert all((r.converged, r.iters, r.n_rounds) == (1, 1, 1) for k, r in enumerate(res) if k != B.FAR_ITEM), rounds
    else:                                                                # the items finish in different rounds
        assert len(set(rounds)) >= 3, rounds
        assert all(r.converged == 1 and r.n_rounds == r.iters for k, r in enumerate(res) if k != B.FAR_ITEM)
    if name == "default":
        assert rounds == [4, 4, 8, 7, 9, 4, 8, 1], rounds               # what the single calls of the parent commit took
    assert res[6].n_pairs_last == 126                                    # the NaN records are no points
    # the Python wrapper gives the same fields
    wres, wfit, winfo = gpu_ctx.gicp_align_batch(srcs, items, e["P"])
    assert winfo == e["info"] and wfit.tobytes() == e["fit"].tobytes()
    for w, r in zip(wres, res):
        assert w["T"].tobytes() == bytes(r.final_transform) and (w["n_rounds"], w["n_evals"], w["inner_exit"]) == (r.n_rounds, r.n_evals, r.inner_exit)
        assert w["error"] == r.error and w["last_delta"] == r.last_delta and w["converged"] == bool(r.converged) and w["n_pairs_last"] == r.n_pairs_last


@pytest.mark.gpu
def test_size_edges_in_one_batch(gpu_ctx):
    """sources of 20 (the k limit), 21, 63, 64, 65 and 4 097 points (65 partial records: the batch totals take their second stride)
    against targets of 20, 21, 64 and 65 points, the shapes of tests/test_gicp.py::small_sources, all 24 in one batch"""
    import lisreg
    P, Pf = lisreg.gicp_default_params(), lisreg.fgicp_default_params()
    for k, nt in enumerate(B.EDGE_NT):
        assert gpu_ctx.fgicp_set_target(SE + k, _pcl(R.small_cloud(nt)), Pf)["n_points"] == nt
    srcs = [_pcl(R.small_cloud(ns, seed=11)) for ns in B.EDGE_NS]
    guess = B.T_SMALL.astype(np.float32)
    items = [lisreg.GicpItem(B.EDGE_NS.index(ns), SE + B.EDGE_NT.index(nt), guess) for ns, nt in B.edge_items()]
    rc, raw, fit, info = _raw_batch(gpu_ctx, srcs, items, P)
    alone = [_raw_single(gpu_ctx, it, srcs[it.source], P) for it in items]
    res = _parse(raw)
    diff = [k for k, (a, b) in enumerate(zip(raw, alone)) if a != b]
    print(f"[gicp_batch] size edges: rounds {[r.n_rounds for r in res]}, pairs {[r.n_pairs_last for r in res]}, batch rounds {info['n_rounds']}, "
          f"items differing from the single calls {diff}")
    assert rc == lisreg.OK and len(items) == 24 and not diff, diff
    assert info["n_rounds"] == max(r.n_rounds for r in res) and info["n_sources_staged"] == 6
    assert [r.n_pairs_last for r in res] == [ns for ns, _ in B.edge_items()]
    g = np.load(PARENT)
    assert [bytes(row) for row in g["edges"]] == alone                   # and the single calls are the parent commit's


@pytest.mark.gpu
def test_cut_offs_that_leave_three_and_four_pairs(gpu_ctx):
    """tests/test_gicp.py's cut-offs as the batch's max_correspondence_distance: 3 pairs at the guess is PCL's "need at least 4 points"
    (converged = 0, n_rounds = iters + 1), 4 pairs runs"""
    import lisreg
    cc = B.cutoff_case()
    gpu_ctx.fgicp_set_target(SCUT, _pcl(cc["tgt"]), lisreg.fgicp_default_params())
    src = _pcl(cc["src"])
    g = np.load(PARENT)
    for want, c in cc["cuts"].items():
        P = lisreg.gicp_default_params(max_correspondence_distance=c)
        items = [lisreg.GicpItem(0, SCUT, cc["guess"]), lisreg.GicpItem(0, SCUT, cc["guess"])]
        rc, raw, fit, info = _raw_batch(gpu_ctx, [src], items, P)
        alone = _raw_single(gpu_ctx, items[0], src, P)
        r = _parse(raw)[0]
        print(f"[gicp_batch] cut-off {c:.6f} ({want} pairs at the guess): converged {r.converged}, outer {r.iters}, rounds {r.n_rounds}, pairs of the "
              f"last round {r.n_pairs_last}, fitness {fit.tolist()}, best {info['best']}")
        assert rc == lisreg.OK and raw == [alone, alone] and alone == bytes(g[f"cut{want}"])
        assert info["n_rounds"] == r.n_rounds and np.isfinite(fit).all()
        if want < 4:
            assert (r.converged, r.iters, r.n_rounds, r.n_pairs_last, r.inner_exit) == (0, 0, 1, 3, -1) and info["best"] == -1
            assert r.n_rounds == r.iters + 1
        else:
            assert r.iters >= 1 and r.n_rounds == r.iters + (0 if r.converged else 1) and r.inner_exit >= 0
            assert info["best"] == (1 if r.converged else -1)            # equal scores go to the later item


@pytest.mark.gpu
def test_fitness_equals_the_restatement(gpu_ctx, shapes, eight):
    e = eight["default"]
    items, xyz = shapes["items"], shapes["xyz"]
    res = _parse(e["raw"])
    T = [np.array(list(r.final_transform)).reshape(4, 4) for r in res]
    want = np.array([B.fitness(shapes["tgt"][it.slot], xyz[it.source], Tk) for it, Tk in zip(items, T)])
    rel = np.abs(e["fit"] - want) / want
    print(f"[gicp_batch] fitness {e['fit'].tolist()}, restatement {want.tolist()}, worst error {rel.max():.3e} relative")
    assert np.isfinite(e["fit"]).all() and rel.max() <= 1e-10, rel
    assert e["fit"][B.FAR_ITEM] > 90.0 ** 2                              # no cut-off: 100 m away still has a score
    # the source with three NaN records is averaged over its 126 points, not its 129 records
    finite = xyz[B.C129N][~np.isnan(xyz[B.C129N]).any(1)]
    assert len(finite) == 126
    w126 = B.fitness(shapes["tgt"][SA], finite, T[6])
    assert abs(e["fit"][6] - w126) <= 1e-10 * w126 and abs(e["fit"][6] - w126 * 126 / 129) > 1e-3 * w126
    # without the fitness pass: the same results and rounds, no winner
    rc, rawn, fitn, infon = _raw_batch(gpu_ctx, shapes["pcl"], items, e["P"], want_fitness=False)
    assert rc == 0 and rawn == e["raw"] and (fitn == -7.0).all() and infon == dict(e["info"], best=-1)
    wres, wfit, winfo = gpu_ctx.gicp_align_batch(shapes["pcl"], items, e["P"], want_fitness=False)
    assert wfit is None and winfo["best"] == -1 and winfo["n_rounds"] == e["info"]["n_rounds"]


@pytest.mark.gpu
def test_best_follows_the_rule(gpu_ctx, shapes, eight):
    import lisreg
    for name, e in eight.items():
        conv = [r.converged for r in _parse(e["raw"])]
        assert e["info"]["best"] == B.best(conv, e["fit"]) >= 0, (name, conv, e["fit"], e["info"])
    # the first item is 100 m off: GICP finds no pair and calls that not converged, so it is skipped whatever its score; of the two equal
    # items behind it the later one wins
    P = eight["default"]["P"]
    items = [lisreg.GicpItem(B.FULL, SA, shapes["far"]), lisreg.GicpItem(B.FULL, SA, shapes["guess"]), lisreg.GicpItem(B.FULL, SA, shapes["guess"])]
    rc, raw, fit, info = _raw_batch(gpu_ctx, shapes["pcl"], items, P)
    conv = [r.converged for r in _parse(raw)]
    print(f"[gicp_batch] best: converged {conv}, fitness {fit.tolist()}, best {info['best']}")
    assert rc == 0 and conv == [0, 1, 1] and fit[0] > 90.0 ** 2 > fit[1] and fit[1:2].tobytes() == fit[2:3].tobytes()
    assert info["best"] == B.best(conv, fit) == 2 and info["n_sources_staged"] == 1
    rc, raw, fit, info = _raw_batch(gpu_ctx, shapes["pcl"], items[:1], P)
    assert rc == 0 and info["best"] == B.best([r.converged for r in _parse(raw)], fit) == -1 and fit[0] > 90.0 ** 2


@pytest.mark.gpu
def test_single_items_and_no_items(gpu_ctx, shapes, eight):
    import lisreg
    L = lisreg.lib()
    srcs, items = shapes["pcl"], shapes["items"]
    e = eight["default"]
    for k in range(len(items)):                                          # every item as a batch of its own
        rc, raw, fit, info = _raw_batch(gpu_ctx, srcs, [items[k]], e["P"])
        r = _parse(raw)[0]
        print(f"[gicp_batch] item {k} alone: rounds {info['n_rounds']}, best {info['best']}, fitness {fit.tolist()}, same bytes as in the batch {raw[0] == e['raw'][k]}")
        assert rc == 0 and raw[0] == e["raw"][k] and fit.tobytes() == e["fit"][k:k + 1].tobytes(), k
        assert info == dict(best=0 if r.converged else -1, n_rounds=r.n_rounds, n_sources_staged=1), (k, info)
    # no items: nothing is read, nothing is refused
    info = lisreg.GicpBatchInfo(best=5, n_rounds=5, n_sources_staged=5)
    assert L.lisreg_gicp_align_batch(gpu_ctx._h, None, None, 0, 0, 0, None, 0, None, None, None, C.byref(info)) == lisreg.OK
    assert (info.best, info.n_rounds, info.n_sources_staged) == (-1, 0, 0)
    rese, fite, infoe = gpu_ctx.gicp_align_batch(srcs, [], e["P"])
    assert rese == [] and len(fite) == 0 and infoe == dict(best=-1, n_rounds=0, n_sources_staged=0)


@pytest.mark.gpu
def test_every_refusal_leaves_the_results_untouched(gpu_ctx, shapes, eight):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = eight["default"]["P"]
    src = shapes["pcl"][B.FULL]
    guess = shapes["guess"]
    ok = lisreg.GicpItem(0, SA, guess)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)

    def call(sources, items, params=P, null=(), counts=None):
        """the raw call with a results array of 0xAB bytes: (return code, results untouched, fitness untouched, info.best)"""
        ptrs = (vp * max(len(sources), 1))(*[None if s is None else (vp(s) if isinstance(s, int) else s.ctypes.data_as(vp)) for s in sources])
        ns = (C.c_int * max(len(sources), 1))(*(counts or [5 if s is None else len(s) for s in sources]))
        its = (lisreg.GicpItemC * max(len(items), 1))()
        for k, it in enumerate(items):
            its[k].source, its[k].slot = it.source, it.slot
            its[k].guess = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
        res = (lisreg.GicpResult * max(len(items), 1))()
        C.memset(res, 0xAB, C.sizeof(res))
        fit = np.full(max(len(items), 1), -7.0)
        info = lisreg.GicpBatchInfo()
        device = any(isinstance(s, int) for s in sources)
        rc = L.lisreg_gicp_align_batch(ctx._h, None if "sources" in null else ptrs, None if "n" in null else ns, len(sources),
                                       16 if device else (src.dtype.itemsize if "stride" not in null else 8),
                                       lisreg.FMT_DEVICE if device else (lisreg.FMT_XYZIL if "stride" not in null else lisreg.FMT_XYZI),
                                       None if "items" in null else its, len(items), None if params is None else C.byref(params),
                                       None if "results" in null else res, fit.ctypes.data_as(dp), C.byref(info))
        return rc, bytes(res) == b"\xab" * C.sizeof(res), bool((fit == -7.0).all()), info.best

    def refused(word, *a, **kw):
        rc, untouched, fit_untouched, best = call(*a, **kw)
        print(f"[gicp_batch] refusal wanted for '{word}': rc {rc}, results untouched {untouched}, fitness untouched {fit_untouched}, best {best}: "
              f"{L.lisreg_last_error(ctx._h).decode()}")
        assert rc == lisreg.ERR_ARG and untouched and fit_untouched and best == -1, (word, rc, untouched, fit_untouched, best)
        msg = L.lisreg_last_error(ctx._h).decode()
        assert "gicp_align_batch" in msg and word in msg, (word, msg)
    for what in ("items", "results", "sources", "n"):
        refused("NULL items", [src], [ok], null=(what,))
    for s in (-1, 1, 7):
        refused("source index", [src], [ok, lisreg.GicpItem(s, SA, None)])
    # the target is a FastGICP slot: the VGICP and NDT slots are other numberings
    ctx.vgicp_set_target(4243, shapes["pcl"][B.C129], lisreg.vgicp_default_params())
    for slot in (4242, 4243, -1):
        refused("no FastGICP target", [src], [ok, lisreg.GicpItem(0, slot, None)])
    # a named source lisreg_gicp_align would refuse, whichever item names it, behind valid ones
    refused("n <= 0", [src, src[:0]], [ok, lisreg.GicpItem(1, SA, None)])
    refused("", [src, None], [ok, lisreg.GicpItem(1, SA, None)])
    refused("", [src], [ok], null=("stride",))
    refused("fewer finite points", [src, src[:19]], [ok, lisreg.GicpItem(1, SA, None)])
    holes = shapes["pcl"][B.C20].copy()
    holes["x"][3] = np.nan                                               # 20 records, 19 points
    refused("fewer finite points", [src, holes], [ok, lisreg.GicpItem(1, SA, None)])
    inf = src.copy()
    inf["z"][3] = -np.inf
    refused("infinite", [src, inf], [ok, lisreg.GicpItem(1, SA, None)])
    # every parameter lisreg_gicp_align refuses
    refused("NULL params", [src], [ok], params=None)
    for v in (0.0, -1.0, float("nan")):
        refused("max_correspondence_distance <= 0", [src], [ok], params=lisreg.gicp_default_params(max_correspondence_distance=v))
    for k in (3, 33):
        refused("outside 4 .. 32", [src], [ok], params=lisreg.gicp_default_params(k_correspondences=k))
    for kw in (dict(transformation_epsilon=0.0), dict(rotation_epsilon=-1.0), dict(max_iters=0), dict(max_inner_iters=0), dict(gicp_epsilon=0.0),
               dict(gicp_epsilon=1.5)):
        refused("bad transformation_epsilon", [src], [ok], params=lisreg.gicp_default_params(**kw))
    for kw in (dict(rho=0.0), dict(sigma=1.0), dict(tau1=1.0), dict(tau2=0.0), dict(tau3=1.0), dict(step_size=0.0), dict(gradient_tol=0.0),
               dict(order=4), dict(order=1)):
        refused("bad rho", [src], [ok], params=lisreg.gicp_default_params(**kw))
    assert L.lisreg_gicp_align_batch(ctx._h, None, None, 0, 0, 0, None, -1, C.byref(P), None, None, None) == lisreg.ERR_ARG
    assert "n_items < 0" in L.lisreg_last_error(ctx._h).decode()
    # more than INT_MAX / 74 wavefronts: 28 341 items over a device source of 2^16 records of zeros (1 024 wavefronts each), refused
    # after the source is staged and before any round
    big = lisreg.DeviceArray(np.zeros((1 << 16, 4), np.float32))
    many = [lisreg.GicpItem(0, SA, None)] * ((2 ** 31 - 1) // 74 // (1 << 10) + 1)
    assert len(many) * (1 << 10) > (2 ** 31 - 1) // 74 >= (len(many) - 1) * (1 << 10)
    refused("too large", [big.ptr], many, counts=[1 << 16])
    # what a single call accepts is not refused: a source of exactly k points; an unnamed NULL source
    rc, untouched, _, best = call([shapes["pcl"][B.C20], None], [lisreg.GicpItem(0, SA, guess)])
    assert rc == lisreg.OK and not untouched and best == 0
    # the context stays usable: the batch of eight gives the bytes it gave before
    e = eight["default"]
    rc, raw, fit, info = _raw_batch(ctx, shapes["pcl"], shapes["items"], P)
    assert rc == lisreg.OK and raw == e["raw"] and fit.tobytes() == e["fit"].tobytes() and info == e["info"]


@pytest.mark.gpu
def test_the_four_families_interleaved_on_one_context(gpu_ctx, shapes, eight, ndt_shapes):
    """GICP, FastGICP, VGICP and NDT batches take turns on one context (the VGICP / FastGICP shapes of tests/test_gicp_batch_shared.py,
    the NDT shapes of tests/test_ndt_batch.py): the driver, its buffers' struct and the fitness kernel are shared, the record width is
    not, and no call leaves anything behind that another reads"""
    import lisreg
    import test_gicp_batch_shared as TS
    import fgicp_ref as FR
    ctx = gpu_ctx
    fam = {}
    for name, set_target, default_params, item, batch in (
            ("fgicp", ctx.fgicp_set_target, lisreg.fgicp_default_params, lisreg.FgicpItem, ctx.fgicp_align_batch),
            ("vgicp", ctx.vgicp_set_target, lisreg.vgicp_default_params, lisreg.VgicpItem, ctx.vgicp_align_batch)):
        Pf = default_params()
        for slot, nt in zip(TS.SLOTS, TS.NT):
            assert set_target(slot, _pcl(FR.small_cloud(nt)), Pf)["n_points"] == nt
        items = [item(s, TS.SLOTS[t], g) for s, t, g in TS.ITEMS]
        fam[name] = (lambda b=batch, i=items, p=Pf, s=[_pcl(FR.small_cloud(ns, seed=11)) for ns in TS.NS]: b(s, i, p))
    Pn = lisreg.ndt_default_params()
    nd_items = [ndt_shapes["items"][k] for k in (0, 1, 2, 5)]
    fam["ndt"] = lambda: TNB._raw_batch(ctx, ndt_shapes["pcl"], nd_items, Pn)[1:]
    picks = (2, 3, 6, 7)                                                 # the cuts of 63 and 65, the NaN cut, the far guess: 8 / 7 / 8 / 1 rounds
    gc_items = [shapes["items"][k] for k in picks]
    fam["gicp"] = lambda: _raw_batch(ctx, shapes["pcl"], gc_items, eight["default"]["P"])[1:]
    runs = {}
    for name in ("gicp", "ndt", "fgicp", "gicp", "vgicp", "ndt", "gicp", "vgicp", "fgicp", "ndt", "fgicp", "gicp"):
        runs.setdefault(name, []).append(fam[name]())
    for name in ("fgicp", "vgicp"):
        first = runs[name][0]
        for res, fit, info in runs[name][1:]:
            assert [TS._bits(r) for r in res] == [TS._bits(r) for r in first[0]] and fit.tobytes() == first[1].tobytes() and info == first[2], name
        assert max(r["n_evals"] for r in first[0]) > 1
    for name in ("ndt", "gicp"):
        first = runs[name][0]
        assert len(runs[name]) >= 3
        for raw, fit, info in runs[name][1:]:
            assert raw == first[0] and fit.tobytes() == first[1].tobytes() and info == first[2], name
    first = runs["gicp"][0]
    print(f"[gicp_batch] interleaved: GICP rounds {first[2]['n_rounds']}, NDT rounds {runs['ndt'][0][2]['n_rounds']}")
    assert first[0] == [eight["default"]["raw"][k] for k in picks] and first[1].tobytes() == eight["default"]["fit"][list(picks)].tobytes()


@pytest.mark.gpu
def test_twenty_batch_calls_do_not_grow_device_memory(gpu_ctx, shapes, eight):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = _params("kind1")
    picks = (1, 3, 5, 6, 7)
    items = [shapes["items"][k] for k in picks]
    first = _raw_batch(gpu_ctx, shapes["pcl"], items, P)                 # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        last = _raw_batch(gpu_ctx, shapes["pcl"], items, P)
    after = free_bytes()
    print(f"[gicp_batch] free device memory before the twenty calls {before}, after {after}; rounds {first[3]['n_rounds']}")
    assert after == before
    assert last[0] == 0 and last[1] == first[1] and last[2].tobytes() == first[2].tobytes() and last[3] == first[3]
    assert first[1] == [eight["kind1"]["raw"][k] for k in picks]
    # a smaller batch afterwards fits into what is there
    _raw_batch(gpu_ctx, shapes["pcl"], items[:1], P)
    assert free_bytes() == before


@pytest.mark.gpu
def test_batch_on_a_callers_busy_stream(env):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the batch's results and scores equal the
    idle-stream ones, and a context left on its own stream reads the decoy"""
    e = env
    # a short alignment (one outer iteration of at most three BFGS steps), as in tests/test_gicp.py
    P = e.lisreg.gicp_default_params(max_iters=1, max_inner_iters=3)
    sh = B.scene_shapes()
    e.ctx.fgicp_set_target(SA, _pcl(sh["tgt"][0]), e.lisreg.fgicp_default_params())
    src = sh["xyz"][B.FULL]
    rs = _records(src)
    near = sh["guess"].copy()
    near[0, 3] += 0.02

    def make(dst):
        def run():
            items = [e.lisreg.GicpItem(0, SA, sh["guess"]), e.lisreg.GicpItem(0, SA, near)]
            res, fit, info = e.ctx.gicp_align_batch([(dst.ptr, len(rs))], items, P)
            return dict(T=np.stack([r["T"] for r in res]), counts=np.array([[r["iters"], r["inner_iters"], r["n_evals"], r["n_pairs_last"]] for r in res]),
                        error=np.array([r["error"] for r in res]), fit=fit, best=info["best"])
        return run, (lambda r: r)
    o, _ = TCS.late_case(e, "gicp_align_batch (device records)", rs, TCS.moved(rs, small=True), make)
    single = e.ctx.gicp_align(SA, _pcl(src), P, sh["guess"])
    assert o["T"][0].tobytes() == single["T"].tobytes() and o["error"][0] == single["error"]
    assert list(o["counts"][0]) == [single["iters"], single["inner_iters"], single["n_evals"], single["n_pairs_last"]] and single["iters"] == 1


@pytest.mark.gpu
def test_the_single_call_still_gives_the_parents_bytes(gpu_ctx, shapes, eight):
    """lisreg_gicp_align now runs over GicpStepper and lisreg_gicp_moments shares its helpers with the batch: both return, byte for byte,
    what the parent commit's build wrote (tests/golden/make_golden_gicp_batch.py)"""
    import lisreg
    g = np.load(PARENT)
    assert os.path.getsize(PARENT) < 64 * 1024
    for name, _, _ in B.PARAM_SETS:
        want = [bytes(row) for row in g["eight_" + name]]
        diff = [k for k, (a, b) in enumerate(zip(eight[name]["alone"], want)) if a != b]
        print(f"[gicp_batch] single calls under {name}: {len(want)} results of 176 bytes, differing from the parent's {diff}")
        assert len(want) == 8 and all(len(b) == 176 for b in want) and not diff, (name, diff)
    P = lisreg.gicp_default_params()
    poses = R.lin_poses(shapes["guess"], shapes["T_true"])
    got = np.stack([gpu_ctx.gicp_moments(SA, shapes["pcl"][B.FULL], P, T) for T in poses])
    assert got.shape == g["moments"].shape == (3, 74) and got.tobytes() == g["moments"].tobytes()
    assert g["moments"][:, 73].tolist() == [2939.0, 2939.0, 0.0]


@pytest.mark.gpu
def test_gicp_batch_smoke_runs():
    import subprocess
    exe = os.path.join(HOST, "gicp_batch_smoke")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "gicp_batch_smoke ok" in r.stdout, r.stdout + r.stderr
