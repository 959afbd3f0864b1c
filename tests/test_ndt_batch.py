"""lisreg_ndt_align_batch: NDT verification of a candidate list as one call (lis-slam_amd/csrc/lisreg_ndt_batch.hip)
against single lisreg_ndt_align calls and against its definition, tests/ndt_batch_ref.py.  The CPU side (the structs, the stepper
check, the restatement, the one home of the loop and of the lane body) is tests/test_ndt_batch_host.py.

The bounds (set where the feature was specified; every test prints its figures before it asserts):
  against single calls   every lisreg_ndt_result equal as raw bytes (all 152 of them), for line_search 1 and 0; n_rounds == the largest
                         n_evals; results, fitness and info bit-identical between two batch calls;
  against the restatement   fitness within 1e-10 relative of ndt_batch_ref.fitness at the returned p (a sum of positive terms: the
                         project's sum bar, tests/test_fgicp_batch.py); `best` equal to ndt_batch_ref.best on the returned
                         (converged, fitness).  The alignments themselves are pinned to the restatement by tests/test_ndt.py (single
                         call) and to the single call by bytes here: no line-search decision is compared a second time;
  lisreg_ndt_set_target    info, voxels and one evaluation equal, as bytes, to what the commit before the search grid was added
                         wrote into tests/golden/ndt_batch/ndt_parent_outputs.npz.

Shapes: the targets ndt_ref.scene(1000) (25 401 points) and scene(1001, 0.5, 3.0); sources cut from the scene's 735-point source as
src[::len(src) // ns][:ns]: 63 (a wavefront short by a lane), 65 (one lane into a second), 129 (one lane into a third), all 735, 1 point,
the 129 with three NaN records (one of them lane 0 of the second wavefront), and a source index no item names, passed as NULL.  On
the CPU ndt_ref.align runs 63 / 65 / 129 / 735 points against the first target in 35 / 14 / 32 / 18 evaluations (line_search = 1) and
13 / 9 / 10 / 38 (line_search = 0), and a guess 100 m away ends after 1: the items of a batch finish in different rounds, and rounds mix
evaluations with and without the Hessian."""
import ctypes as C
import os

import numpy as np
import pytest

import ndt_batch_ref as B
import ndt_ref as R
import test_ndt as TN
import test_caller_stream as TCS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARENT = os.path.join(ROOT, "tests", "golden", "ndt_batch", "ndt_parent_outputs.npz")
env = TCS.env
_pcl, _records = TN._pcl, TN._records
SA, SB, SC, SP = 50, 51, 52, 53                          # NDT slots: the two scenes, the first at another resolution, the planted cloud
S63, S65M, S129, S735, S1, S129N, SNULL = range(7)       # indices into the sources
NAN_AT = (5, 64, 128)


def _cut(src, ns):
    return np.ascontiguousarray(src[::len(src) // ns][:ns])


@pytest.fixture(scope="module")
def shapes(gpu_ctx):
    """targets in their slots, the sources (xyz and PCL structs) and the guesses: made once, never changed"""
    import lisreg
    tgt_a, src, guess, T_true = R.scene()
    tgt_b = R.scene(1001, 0.5, 3.0)[0]
    P = lisreg.ndt_default_params()
    gpu_ctx.ndt_set_target(SA, _pcl(tgt_a), P)
    gpu_ctx.ndt_set_target(SB, _pcl(tgt_b), P)
    holes = _cut(src, 129).copy()
    holes[list(NAN_AT)] = np.nan
    holes[NAN_AT[0], 1] = 0.5                            # (a record with one NaN coordinate is no point either)
    xyz = [_cut(src, 63), TN._apply_f32(guess, _cut(src, 65)), _cut(src, 129), src, _cut(src, 1), holes, None]
    assert [None if x is None else len(x) for x in xyz] == [63, 65, 129, 735, 1, 129, None]
    far = guess.copy()
    far[0, 3] += 100.0
    items = [lisreg.NdtItem(S63, SA, guess), lisreg.NdtItem(S65M, SB, None), lisreg.NdtItem(S129, SA, guess), lisreg.NdtItem(S735, SB, guess),
             lisreg.NdtItem(S735, SA, guess), lisreg.NdtItem(S735, SA, far), lisreg.NdtItem(S1, SB, guess), lisreg.NdtItem(S129N, SA, guess)]
    return dict(tgt={SA: tgt_a, SB: tgt_b}, xyz=xyz, pcl=[None if x is None else _pcl(x) for x in xyz], guess=guess, far=far, items=items)


def _raw_batch(ctx, sources, items, P, want_fitness=True, res_fill=None):
    """the raw call: (return code, the results as one bytes object per item, fitness array, info dict)"""
    import lisreg
    L = lisreg.lib()
    vp = C.c_void_p
    stride = next(s.dtype.itemsize for s in sources if s is not None)
    ptrs = (vp * max(len(sources), 1))(*[None if s is None else s.ctypes.data_as(vp) for s in sources])
    ns = (C.c_int * max(len(sources), 1))(*[0 if s is None else len(s) for s in sources])
    its = (lisreg.NdtItemC * max(len(items), 1))()
    for k, it in enumerate(items):
        its[k].source, its[k].slot = it.source, it.slot
        its[k].guess = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
    res = (lisreg.NdtResult * max(len(items), 1))()
    if res_fill is not None:
        C.memset(res, res_fill, C.sizeof(res))
    fit = np.full(max(len(items), 1), -7.0)
    info = lisreg.NdtBatchInfo()
    rc = L.lisreg_ndt_align_batch(ctx._h, ptrs, ns, len(sources), stride, lisreg.FMT_XYZIL, its, len(items), C.byref(P), res,
                                  fit.ctypes.data_as(C.POINTER(C.c_double)) if want_fitness else None, C.byref(info))
    size = C.sizeof(lisreg.NdtResult)
    return rc, [bytes(res)[k * size:(k + 1) * size] for k in range(len(items))], fit[:len(items)], \
        dict(best=info.best, n_rounds=info.n_rounds, n_sources_staged=info.n_sources_staged)


def _raw_single(ctx, it, source, P):
    import lisreg
    res = lisreg.NdtResult()
    g = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
    rc = lisreg.lib().lisreg_ndt_align(ctx._h, it.slot, source.ctypes.data_as(C.c_void_p), len(source), source.dtype.itemsize, lisreg.FMT_XYZIL,
                                       C.byref(P), g, C.byref(res), None)
    assert rc == lisreg.OK, lisreg.lib().lisreg_last_error(ctx._h)
    return bytes(res)


def _parse(raw):
    import lisreg
    return [lisreg.NdtResult.from_buffer_copy(b) for b in raw]


@pytest.fixture(scope="module")
def eight(gpu_ctx, shapes):
    """the batch of eight under line_search 1 and 0: computed once, read by the tests below"""
    import lisreg
    out = {}
    for ls in (1, 0):
        P = lisreg.ndt_default_params(line_search=ls)
        rc, raw, fit, info = _raw_batch(gpu_ctx, shapes["pcl"], shapes["items"], P)
        assert rc == lisreg.OK, lisreg.lib().lisreg_last_error(gpu_ctx._h)
        out[ls] = dict(P=P, raw=raw, fit=fit, info=info)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("ls", [1, 0])
def test_a_batch_of_eight_items_equals_the_single_calls(gpu_ctx, shapes, eight, ls):
    import lisreg
    e = eight[ls]
    items, srcs = shapes["items"], shapes["pcl"]
    alone = [_raw_single(gpu_ctx, it, srcs[it.source], e["P"]) for it in items]
    diff = [k for k, (a, b) in enumerate(zip(e["raw"], alone)) if a != b]
    res = _parse(e["raw"])
    evals = [r.n_evals for r in res]
    rc, raw2, fit2, info2 = _raw_batch(gpu_ctx, srcs, items, e["P"])
    print(f"[ndt_batch] line_search {ls}: evaluations {evals}, iterations {[r.iters for r in res]}, converged {[r.converged for r in res]}, "
          f"rounds {e['info']['n_rounds']}, sources staged {e['info']['n_sources_staged']}, items differing from the single calls {diff}, "
          f"best {e['info']['best']}, fitness {e['fit'].tolist()}")
    assert C.sizeof(lisreg.NdtResult) == 152 and all(len(b) == 152 for b in e["raw"])
    assert not diff, diff
    assert rc == lisreg.OK and raw2 == e["raw"] and fit2.tobytes() == e["fit"].tobytes() and info2 == e["info"]
    # the items finish in different rounds, and every unfinished one has exactly one evaluation outstanding per round
    assert len(set(evals)) >= 3 and e["info"]["n_rounds"] == max(evals), (evals, e["info"])
    assert e["info"]["n_sources_staged"] == 6                            # the seven sources less the one nobody names
    far = res[5]
    assert (far.converged, far.iters, far.n_evals, far.n_pairs_last, far.score) == (1, 0, 1, 0, 0.0)
    assert res[4].n_evals > 1 and res[3].n_evals > 1                    # one source against the targets of two slots
    # trans_probability divides by the records, NaN ones included
    assert res[7].trans_probability == res[7].score / 129 and res[6].trans_probability == res[6].score / 1
    # the Python wrapper gives the same fields
    wres, wfit, winfo = gpu_ctx.ndt_align_batch(srcs, items, e["P"])
    assert winfo == e["info"] and wfit.tobytes() == e["fit"].tobytes()
    for w, r in zip(wres, res):
        assert w["p"].tobytes() == bytes(r.p) and w["T"].tobytes() == bytes(r.final_transform) and w["n_evals"] == r.n_evals and w["score"] == r.score


@pytest.mark.gpu
@pytest.mark.parametrize("ls", [1, 0])
def test_fitness_equals_the_restatement(gpu_ctx, shapes, eight, ls):
    e = eight[ls]
    items, xyz = shapes["items"], shapes["xyz"]
    res = _parse(e["raw"])
    want = np.array([B.fitness(shapes["tgt"][it.slot], xyz[it.source], np.array(list(r.p))) for it, r in zip(items, res)])
    rel = np.abs(e["fit"] - want) / want
    print(f"[ndt_batch] line_search {ls}: fitness {e['fit'].tolist()}, restatement {want.tolist()}, worst error {rel.max():.3e} relative")
    assert np.isfinite(e["fit"]).all() and rel.max() <= 1e-10, rel
    assert e["fit"][5] > 90.0 ** 2                                      # no cut-off: 100 m away still has a score
    # the source with three NaN records is averaged over its 126 points, not its 129 records
    finite = xyz[S129N][~np.isnan(xyz[S129N]).any(1)]
    assert len(finite) == 126
    w126 = B.fitness(shapes["tgt"][SA], finite, np.array(list(res[7].p)))
    assert abs(e["fit"][7] - w126) <= 1e-10 * w126 and abs(e["fit"][7] - w126 * 126 / 129) > 1e-3 * w126
    # without the fitness pass: the same results and rounds, no winner
    rc, rawn, fitn, infon = _raw_batch(gpu_ctx, shapes["pcl"], items, e["P"], want_fitness=False)
    assert rc == 0 and rawn == e["raw"] and (fitn == -7.0).all() and infon == dict(e["info"], best=-1)
    wres, wfit, winfo = gpu_ctx.ndt_align_batch(shapes["pcl"], items, e["P"], want_fitness=False)
    assert wfit is None and winfo["best"] == -1 and winfo["n_rounds"] == e["info"]["n_rounds"]


@pytest.mark.gpu
def test_best_follows_the_rule(gpu_ctx, shapes, eight):
    import lisreg
    for ls in (1, 0):
        e = eight[ls]
        conv = [r.converged for r in _parse(e["raw"])]
        assert e["info"]["best"] == B.best(conv, e["fit"]), (ls, conv, e["fit"], e["info"])
    # a case whose winner is not item 0: the first item is 100 m off (NDT calls that converged, its score says otherwise), and two
    # equal items behind it, of which the later one wins
    P = eight[1]["P"]
    items = [lisreg.NdtItem(S735, SA, shapes["far"]), lisreg.NdtItem(S735, SA, shapes["guess"]), lisreg.NdtItem(S735, SA, shapes["guess"])]
    rc, raw, fit, info = _raw_batch(gpu_ctx, shapes["pcl"], items, P)
    res = _parse(raw)
    conv = [r.converged for r in res]
    print(f"[ndt_batch] best: converged {conv}, fitness {fit.tolist()}, best {info['best']}")
    assert rc == 0 and conv == [1, 1, 1] and fit[0] > 90.0 ** 2 > fit[1] and fit[1:2].tobytes() == fit[2:3].tobytes()
    assert info["best"] == B.best(conv, fit) == 2 and info["n_sources_staged"] == 1
    rc, raw, fit, info = _raw_batch(gpu_ctx, shapes["pcl"], items[:2], P)
    assert rc == 0 and info["best"] == B.best([r.converged for r in _parse(raw)], fit) == 1


@pytest.mark.gpu
def test_single_item_no_iterations_and_no_items(gpu_ctx, shapes, eight):
    import lisreg
    L = lisreg.lib()
    srcs, items = shapes["pcl"], shapes["items"]
    for ls in (1, 0):
        e = eight[ls]
        for k in (0, 3, 5, 6, 7):                                         # every item as a batch of its own
            rc, raw, fit, info = _raw_batch(gpu_ctx, srcs, [items[k]], e["P"])
            r = _parse(raw)[0]
            assert rc == 0 and raw[0] == e["raw"][k] and fit.tobytes() == e["fit"][k:k + 1].tobytes(), (ls, k)
            assert info == dict(best=0 if r.converged else -1, n_rounds=r.n_evals, n_sources_staged=1), (ls, k, info)
        # max_iters = 0: the end rule fires on the second pass of the loop
        P0 = lisreg.ndt_default_params(line_search=ls, max_iters=0)
        rc, raw, fit, info = _raw_batch(gpu_ctx, srcs, items, P0)
        alone = [_raw_single(gpu_ctx, it, srcs[it.source], P0) for it in items]
        res = _parse(raw)
        print(f"[ndt_batch] max_iters 0, line_search {ls}: iterations {[r.iters for r in res]}, evaluations {[r.n_evals for r in res]}")
        assert rc == 0 and raw == alone and info["n_rounds"] == max(r.n_evals for r in res)
        assert all(r.iters <= 2 for r in res) and res[4].iters == 2 and res[4].converged == 1
    # no items: nothing is read, nothing is refused
    info = lisreg.NdtBatchInfo(best=5, n_rounds=5, n_sources_staged=5)
    assert L.lisreg_ndt_align_batch(gpu_ctx._h, None, None, 0, 0, 0, None, 0, None, None, None, C.byref(info)) == lisreg.OK
    assert (info.best, info.n_rounds, info.n_sources_staged) == (-1, 0, 0)
    rese, fite, infoe = gpu_ctx.ndt_align_batch(srcs, [], eight[1]["P"])
    assert rese == [] and len(fite) == 0 and infoe == dict(best=-1, n_rounds=0, n_sources_staged=0)


@pytest.mark.gpu
def test_every_refusal_leaves_the_results_untouched(gpu_ctx, shapes, eight):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = eight[1]["P"]
    src = shapes["pcl"][S735]
    guess = shapes["guess"]
    ok = lisreg.NdtItem(0, SA, guess)
    vp, dp = C.c_void_p, C.POINTER(C.c_double)

    def call(sources, items, params=P, null=(), counts=None):
        """the raw call with a results array of 0xAB bytes: (return code, results untouched, fitness untouched, info.best)"""
        ptrs = (vp * max(len(sources), 1))(*[None if s is None else (vp(s) if isinstance(s, int) else s.ctypes.data_as(vp)) for s in sources])
        ns = (C.c_int * max(len(sources), 1))(*(counts or [5 if s is None else len(s) for s in sources]))
        its = (lisreg.NdtItemC * max(len(items), 1))()
        for k, it in enumerate(items):
            its[k].source, its[k].slot = it.source, it.slot
            its[k].guess = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
        res = (lisreg.NdtResult * max(len(items), 1))()
        C.memset(res, 0xAB, C.sizeof(res))
        fit = np.full(max(len(items), 1), -7.0)
        info = lisreg.NdtBatchInfo()
        device = any(isinstance(s, int) for s in sources)
        rc = L.lisreg_ndt_align_batch(ctx._h, None if "sources" in null else ptrs, None if "n" in null else ns, len(sources),
                                      16 if device else (src.dtype.itemsize if "stride" not in null else 8),
                                      lisreg.FMT_DEVICE if device else (lisreg.FMT_XYZIL if "stride" not in null else lisreg.FMT_XYZI),
                                      None if "items" in null else its, len(items), None if params is None else C.byref(params),
                                      None if "results" in null else res, fit.ctypes.data_as(dp), C.byref(info))
        return rc, bytes(res) == b"\xab" * C.sizeof(res), bool((fit == -7.0).all()), info.best

    def refused(word, *a, **kw):
        rc, untouched, fit_untouched, best = call(*a, **kw)
        assert rc == lisreg.ERR_ARG and untouched and fit_untouched and best == -1, (word, rc, untouched, fit_untouched, best)
        msg = L.lisreg_last_error(ctx._h).decode()
        assert word in msg, (word, msg)
    for what in ("items", "results", "sources", "n"):
        refused("NULL items", [src], [ok], null=(what,))
    for s in (-1, 1, 7):
        refused("source index", [src], [ok, lisreg.NdtItem(s, SA, None)])
    for slot in (4242, -1):
        refused("no NDT target", [src], [ok, lisreg.NdtItem(0, slot, None)])
    # a slot built at another resolution among slots at the params': the batch has one set of params, so it is refused, whichever side
    # the params take
    P2 = lisreg.ndt_default_params(resolution=2.0)
    ctx.ndt_set_target(SC, _pcl(shapes["tgt"][SA]), P2)
    refused("resolution differs", [src], [ok, lisreg.NdtItem(0, SC, guess), ok])
    refused("resolution differs", [src], [lisreg.NdtItem(0, SC, guess), ok], params=P2)
    # a named source lisreg_ndt_align would refuse, whichever item names it, behind valid ones
    refused("n <= 0", [src, src[:0]], [ok, lisreg.NdtItem(1, SA, None)])
    refused("", [src, None], [ok, lisreg.NdtItem(1, SA, None)])
    refused("", [src], [ok], null=("stride",))
    refused("NULL params", [src], [ok], params=None)
    for kw, word in ((dict(resolution=0.0), "resolution <= 0"), (dict(outlier_ratio=1.5), "outlier_ratio"), (dict(step_size=0.0), "bad step_size"),
                     (dict(transformation_epsilon=0.0), "bad step_size"), (dict(max_iters=-1), "bad step_size"), (dict(resolution=0.5), "resolution differs")):
        refused(word, [src], [ok], params=lisreg.ndt_default_params(**kw))
    assert L.lisreg_ndt_align_batch(ctx._h, None, None, 0, 0, 0, None, -1, C.byref(P), None, None, None) == lisreg.ERR_ARG
    # more than INT_MAX / 29 wavefronts: 4 521 items over a source of 2^20 records (16 384 wavefronts each), refused before any round
    big = lisreg.DeviceArray(np.zeros((1 << 20, 4), np.float32))
    many = [lisreg.NdtItem(0, SA, None)] * ((2 ** 31 - 1) // 29 // (1 << 14) + 1)
    assert len(many) * (1 << 14) > (2 ** 31 - 1) // 29 >= (len(many) - 1) * (1 << 14)
    refused("too large", [big.ptr], many, counts=[1 << 20])
    # what a single call accepts is not refused: a source of NaN records only, a source of one point; an unnamed NULL source
    allnan = src[:70].copy()
    allnan["x"] = np.nan
    rc, untouched, _, best = call([allnan, src[:1], None], [lisreg.NdtItem(0, SA, guess), lisreg.NdtItem(1, SA, guess)])
    assert rc == lisreg.OK and not untouched
    single = ctx.ndt_align(SA, allnan, P, guess)
    assert (single["converged"], single["n_evals"], single["n_pairs_last"]) == (True, 1, 0)
    # the context stays usable: the batch of eight gives the bytes it gave before
    rc, raw, fit, info = _raw_batch(ctx, shapes["pcl"], shapes["items"], P)
    assert rc == lisreg.OK and raw == eight[1]["raw"] and fit.tobytes() == eight[1]["fit"].tobytes() and info == eight[1]["info"]


@pytest.mark.gpu
def test_the_three_families_interleaved_on_one_context(gpu_ctx, shapes, eight):
    """NDT, VGICP and FastGICP batches take turns on one context (the VGICP / FastGICP shapes of tests/test_gicp_batch_shared.py): the
    driver, its buffers' struct and the fitness kernel are shared, and no call leaves anything behind that another reads"""
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
    nd_items = [shapes["items"][k] for k in (0, 1, 2, 5)]
    fam["ndt"] = lambda: _raw_batch(ctx, shapes["pcl"], nd_items, eight[1]["P"])[1:]
    runs = {}
    for name in ("ndt", "fgicp", "vgicp", "ndt", "vgicp", "fgicp", "ndt", "fgicp"):
        runs.setdefault(name, []).append(fam[name]())
    for name in ("fgicp", "vgicp"):
        first = runs[name][0]
        for res, fit, info in runs[name][1:]:
            assert [TS._bits(r) for r in res] == [TS._bits(r) for r in first[0]] and fit.tobytes() == first[1].tobytes() and info == first[2], name
        assert max(r["n_evals"] for r in first[0]) > 1
    first = runs["ndt"][0]
    for raw, fit, info in runs["ndt"][1:]:
        assert raw == first[0] and fit.tobytes() == first[1].tobytes() and info == first[2]
    assert first[0] == [eight[1]["raw"][k] for k in (0, 1, 2, 5)] and first[1].tobytes() == eight[1]["fit"][[0, 1, 2, 5]].tobytes()


@pytest.mark.gpu
def test_twenty_batch_calls_do_not_grow_device_memory(gpu_ctx, shapes, eight):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = lisreg.ndt_default_params(line_search=0)
    items = [shapes["items"][k] for k in (1, 2, 4, 5, 7)]
    first = _raw_batch(gpu_ctx, shapes["pcl"], items, P)                # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        last = _raw_batch(gpu_ctx, shapes["pcl"], items, P)
    assert free_bytes() == before
    assert last[0] == 0 and last[1] == first[1] and last[2].tobytes() == first[2].tobytes() and last[3] == first[3]
    assert first[1] == [eight[0]["raw"][k] for k in (1, 2, 4, 5, 7)]
    # a smaller batch afterwards fits into what is there
    _raw_batch(gpu_ctx, shapes["pcl"], items[:1], P)
    assert free_bytes() == before


@pytest.mark.gpu
def test_batch_on_a_callers_busy_stream(env):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the batch's results and scores equal the
    idle-stream ones, and a context left on its own stream reads the decoy"""
    e = env
    tgt, src, guess, _ = R.scene()
    P = e.lisreg.ndt_default_params(max_iters=1, line_search=0)          # a short alignment, as in tests/test_ndt.py
    e.ctx.ndt_set_target(SA, _pcl(tgt), P)
    rs = _records(src)
    near = guess.copy()
    near[0, 3] += 0.02

    def make(dst):
        def run():
            items = [e.lisreg.NdtItem(0, SA, guess), e.lisreg.NdtItem(0, SA, near)]
            res, fit, info = e.ctx.ndt_align_batch([(dst.ptr, len(rs))], items, P)
            return dict(p=np.stack([r["p"] for r in res]), T=np.stack([r["T"] for r in res]),
                        counts=np.array([[r["iters"], r["n_evals"], r["n_pairs_last"]] for r in res]),
                        score=np.array([r["score"] for r in res]), fit=fit, best=info["best"])
        return run, (lambda r: r)
    o, _ = TCS.late_case(e, "ndt_align_batch (device records)", rs, TCS.moved(rs, small=True), make)
    single = e.ctx.ndt_align(SA, _pcl(src), P, guess)
    assert o["p"][0].tobytes() == single["p"].tobytes() and o["score"][0] == single["score"] and list(o["counts"][0][:2]) == [3, 4]


@pytest.mark.gpu
def test_set_target_still_gives_the_parents_voxels_and_sums(gpu_ctx):
    """the search grid lisreg_ndt_set_target now keeps changes nothing of what it returned before: info, the voxels and one evaluation
    equal, as bytes, the arrays the parent commit's build wrote (the planted cloud of tests/test_ndt.py and the scene)"""
    import lisreg
    g = np.load(PARENT)
    assert os.path.getsize(PARENT) < 256 * 1024
    P = lisreg.ndt_default_params()
    tgt, src, guess, _ = R.scene()
    planted = R.planted_cloud()
    fin = planted[~np.isnan(planted).any(1)]
    for name, cloud, s in (("planted", planted, np.ascontiguousarray(fin[::7])), ("scene", tgt, src)):
        info = gpu_ctx.ndt_set_target(SP, _pcl(cloud), P)
        assert info["dims"] + [info["n_voxels"], info["n_valid"]] == g[name + "_info"].tolist(), name
        V = gpu_ctx.ndt_get_voxels(SP)
        for k in ("cell_ids", "counts", "means", "icov6"):
            assert V[k].dtype == g[name + "_" + k].dtype and V[k].tobytes() == g[name + "_" + k].tobytes(), (name, k)
        for h in (1, 0):
            out, pairs = gpu_ctx.ndt_derivatives(SP, _pcl(s), P, g[name + "_p"], bool(h))
            assert np.r_[out, float(pairs)].tobytes() == g[f"{name}_deriv{h}"].tobytes(), (name, h)
        assert g[name + "_deriv1"][28] > 0
    assert g["scene_info"].tolist() == [23, 24, 14, 1821, 1735] and g["planted_info"].tolist() == [5, 3, 3, 10, 8]
