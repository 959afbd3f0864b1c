"""lisreg_vgicp_align_batch: VGICP verification of a candidate list as one call (lis-slam_amd/csrc/lisreg_vgicp_batch.hip)
against single lisreg_vgicp_align calls and against its definition, tests/vgicp_batch_ref.py.  The CPU side (the structs, the
restatement, the shared headers) is tests/test_vgicp_batch_host.py.

The bounds (set where the feature was specified; every test prints its figures before it asserts):
  against single calls   every field of every result equal as raw bytes; n_rounds == the largest n_evals; fitness bit-identical
                         between two batch calls;
  against the restatement   the bars of tests/test_vgicp.py for alignments (counts equal, final_transform within 1e-6 entry-wise, error
                         within 1e-6 relative) on the golden cases of tests/golden/vgicp/vgicp_cases.npz; fitness within 1e-10 relative
                         of vgicp_batch_ref.fitness at the returned final_transform (a sum of positive terms: the project's sum bar);
                         `best` equal, with the restatement's two smallest scores among the converged items more than 1e-6 relative apart.

The four alignment cases of §7k do not share transformation_epsilon (5e-4, 5e-4, 5e-4, 0.01), and a batch has one set of params: the
four sources are aligned as one batch under either epsilon, each against the target of its own slot.  Under 5e-4 the first three are
the golden rows (23 / 29 / 17 evaluations: the items drop out in different rounds), under 0.01 the fourth is."""
import ctypes as C
import struct

import numpy as np
import pytest

import vgicp_batch_ref as B
import vgicp_ref as R
import test_vgicp as TV
import test_caller_stream as TCS

world = TV.world
scene_slot = TV.scene_slot
env = TCS.env
_pcl, _records, SLOT, K = TV._pcl, TV._records, TV.SLOT, TV.K
CASE = 30                                               # VGICP slots 30 .. 33: the targets of the four alignment cases
SMALL = 40                                              # VGICP slots 40 .. 43: the small targets
NT, NS = (20, 21, 64, 65), (20, 63, 64, 65, 257)
GUESS = R.se3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.08]).astype(np.float32)


def _bits(r):
    """every field of a result as raw bytes"""
    return (r["T"].tobytes(), int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"],
            struct.pack("d", r["error"]), struct.pack("d", r["lam"]))


def _singles(ctx, sources, items, P):
    return [ctx.vgicp_align(it.slot, sources[it.source], P, None if it.guess is None else it.guess.reshape(4, 4)) for it in items]


def _assert_equals_singles(ctx, sources, items, P, tag):
    res, fit, info = ctx.vgicp_align_batch(sources, items, P)
    alone = _singles(ctx, sources, items, P)
    diff = [k for k, (a, b) in enumerate(zip(res, alone)) if _bits(a) != _bits(b)]
    res2, fit2, info2 = ctx.vgicp_align_batch(sources, items, P)
    evals = [r["n_evals"] for r in res]
    print(f"[vgicp_batch] {tag}: {len(items)} items, evaluations {min(evals)} .. {max(evals)}, rounds {info['n_rounds']}, sources staged "
          f"{info['n_sources_staged']}, items differing from the single calls {diff}, best {info['best']}")
    assert not diff, (tag, diff)
    assert fit.tobytes() == fit2.tobytes() and [_bits(r) for r in res2] == [_bits(r) for r in res] and info2 == info, tag
    assert info["n_rounds"] == max(evals), (tag, info, evals)
    assert np.isfinite(fit).all() and (fit >= 0).all(), tag
    return res, fit, info


@pytest.fixture(scope="module")
def cases(gpu_ctx, world):
    """the targets (each in its own slot), sources and guesses of §7k's four alignment cases"""
    import lisreg
    out = []
    for k, (seed, trans, rot, eps) in enumerate(R.ALIGN_CASES):
        tgt, src, guess, T_true = (world[q] for q in ("tgt", "src", "guess", "T_true")) if seed == 1000 else R.scene(seed, trans, rot)
        gpu_ctx.vgicp_set_target(CASE + k, _pcl(tgt), lisreg.vgicp_default_params())
        out.append(dict(tgt=tgt, src=src, guess=guess, eps=eps, slot=CASE + k))
    return out


@pytest.fixture(scope="module")
def small_slots(gpu_ctx):
    import lisreg
    P = lisreg.vgicp_default_params()
    for k, nt in enumerate(NT):
        assert gpu_ctx.vgicp_set_target(SMALL + k, _pcl(R.small_cloud(nt)), P)["n_points"] == nt
    return [_pcl(R.small_cloud(ns, seed=11)) for ns in NS]


@pytest.mark.gpu
@pytest.mark.parametrize("eps", [5.0e-4, 0.01])
def test_the_four_cases_as_one_batch_equal_single_calls_and_the_restatement(gpu_ctx, world, cases, eps):
    import lisreg
    P = lisreg.vgicp_default_params(transformation_epsilon=eps)
    sources = [_pcl(c["src"]) for c in cases]
    items = [lisreg.VgicpItem(k, c["slot"], c["guess"]) for k, c in enumerate(cases)]
    res, fit, info = _assert_equals_singles(gpu_ctx, sources, items, P, f"the four cases, eps {eps}")
    # reversed order, and every item as a batch of its own
    rres, rfit, rinfo = _assert_equals_singles(gpu_ctx, sources, items[::-1], P, f"the four cases reversed, eps {eps}")
    assert [_bits(r) for r in rres[::-1]] == [_bits(r) for r in res] and rfit[::-1].tobytes() == fit.tobytes()
    for k in range(len(items)):
        one, f1, i1 = gpu_ctx.vgicp_align_batch(sources, [items[k]], P)
        assert _bits(one[0]) == _bits(res[k]) and f1.tobytes() == fit[k:k + 1].tobytes(), k
        assert i1 == dict(best=0 if one[0]["converged"] else -1, n_rounds=one[0]["n_evals"], n_sources_staged=1), (k, i1)
    # against the restatement: the golden rows of the cases this epsilon belongs to
    g = world["g"]
    for k, c in enumerate(cases):
        if c["eps"] != eps:
            continue
        r, counts = res[k], g["align_counts"][k]
        dT, rel = np.abs(r["T"] - g["align_T"][k]).max(), abs(r["error"] - g["align_fig"][k][0]) / g["align_fig"][k][0]
        print(f"[vgicp_batch] case {k}: evals {r['n_evals']} |dT| {dT:.3e} error off by {rel:.3e}")
        assert (int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"]) == tuple(int(v) for v in counts[:5])
        assert dT <= 1e-6 and rel <= 1e-6, (k, dT, rel)
    if eps != R.ALIGN_CASES[0][3]:
        return
    assert [r["n_evals"] for r in res[:3]] == [23, 29, 17]              # the items drop out in different rounds
    want = np.array([B.fitness(c["tgt"], c["src"], r["T"]) for c, r in zip(cases, res)])
    rel = np.abs(fit - want) / want
    conv = [r["converged"] for r in res]
    two = np.unique(want[np.array(conv, bool)])[:2]                      # (cases 0 and 3 are one scene: equal scores, a tie for the later)
    print(f"[vgicp_batch] fitness {fit.tolist()}, worst error {rel.max():.3e} relative, the two smallest {(two[1] - two[0]) / two[1]:.3e} apart")
    assert rel.max() <= 1e-10, rel
    assert len(two) == 2 and (two[1] - two[0]) / two[1] > 1e-6
    assert info["best"] == B.best(conv, want)
    assert rinfo["best"] == B.best(conv[::-1], want[::-1])               # (the tie of cases 0 and 3 goes to the later item either way)


@pytest.mark.gpu
def test_mixed_shapes_in_one_batch(gpu_ctx, small_slots):
    """every small source against every small target: entries of 1, 1, 1, 2 and 5 workgroups side by side"""
    import lisreg
    P = lisreg.vgicp_default_params()
    items = [lisreg.VgicpItem(s, SMALL + t, GUESS) for s in range(len(NS)) for t in range(len(NT))]
    res, fit, info = _assert_equals_singles(gpu_ctx, small_slots, items, P, "mixed shapes")
    assert info["n_sources_staged"] == len(NS) and max(r["n_evals"] for r in res) > 1 and max(r["n_pairs_last"] for r in res) > 0
    # shuffled: the 257-point source between the 63- and the 65-point one, entries of one source apart from each other
    order = np.random.default_rng(20).permutation(len(items)).tolist()
    res2, fit2, _ = _assert_equals_singles(gpu_ctx, small_slots, [items[k] for k in order], P, "mixed shapes, shuffled")
    assert [_bits(r) for r in res2] == [_bits(res[k]) for k in order] and fit2.tobytes() == fit[order].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("n_items", [65, 130])
def test_more_entries_than_a_wavefront(gpu_ctx, small_slots, n_items):
    import lisreg
    P = lisreg.vgicp_default_params()
    rng = np.random.default_rng(600 + n_items)
    items = []
    for k in range(n_items):
        d = np.r_[rng.uniform(-3e-3, 3e-3, 3), rng.uniform(-0.03, 0.03, 3)]              # a few mrad, a few cm
        items.append(lisreg.VgicpItem(k % len(NS), SMALL + (k // len(NS)) % len(NT), (R.se3_exp(d) @ GUESS.astype(np.float64)).astype(np.float32)))
    res, fit, info = _assert_equals_singles(gpu_ctx, small_slots, items, P, f"{n_items} items")
    assert info["n_sources_staged"] == len(NS) and len({_bits(r) for r in res}) > n_items // 2


@pytest.mark.gpu
def test_an_item_that_finishes_at_once_in_the_middle(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.vgicp_default_params()
    far = world["guess"].copy()
    far[0, 3] += 100.0
    moved = TV._apply_f32(world["guess"], world["src"])                   # the source already at the guess: a NULL guess aligns it
    sources = [_pcl(world["src"]), _pcl(moved)]
    items = [lisreg.VgicpItem(0, SLOT, world["guess"]), lisreg.VgicpItem(0, SLOT, far), lisreg.VgicpItem(1, SLOT, None),
             lisreg.VgicpItem(0, SLOT, world["guess"])]
    res, fit, info = _assert_equals_singles(gpu_ctx, sources, items, P, "no pair in the middle")
    r = res[1]
    assert (r["converged"], r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"], r["error"]) == (False, 0, 1, 0, 0, 0.0)
    assert np.array_equal(r["T"], far.astype(np.float64)) and fit[1] > 50.0 ** 2         # no cut-off: it still has a score
    assert res[0]["converged"] and res[2]["converged"] and res[2]["iters"] >= 2 and _bits(res[0]) == _bits(res[3])
    assert info["best"] in (0, 2, 3) and info["best"] == B.best([x["converged"] for x in res], fit)


@pytest.mark.gpu
def test_shared_duplicated_and_unreferenced_sources(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.vgicp_default_params(max_iters=2)
    src = _pcl(world["src"])
    rng = np.random.default_rng(9)
    guesses = [(R.se3_exp(np.r_[rng.uniform(-2e-3, 2e-3, 3), rng.uniform(-0.02, 0.02, 3)]) @ world["guess"].astype(np.float64)).astype(np.float32)
               for _ in range(8)]
    items = [lisreg.VgicpItem(0, SLOT, g) for g in guesses]
    res, fit, info = _assert_equals_singles(gpu_ctx, [src], items, P, "one source, eight items")
    assert info["n_sources_staged"] == 1
    # the same cloud listed twice; between them a source nobody names, which is too small for any distribution: neither staged nor refused
    twice = [lisreg.VgicpItem(0 if k % 2 else 2, SLOT, g) for k, g in enumerate(guesses)]
    res2, fit2, info2 = gpu_ctx.vgicp_align_batch([src, src[:K - 1], src.copy()], twice, P)
    assert [_bits(r) for r in res2] == [_bits(r) for r in res] and fit2.tobytes() == fit.tobytes()
    assert info2["n_sources_staged"] == 2 and info2["best"] == info["best"]
    res3, _, info3 = gpu_ctx.vgicp_align_batch([src[:3], src], [lisreg.VgicpItem(1, SLOT, guesses[0])], P)
    assert _bits(res3[0]) == _bits(res[0]) and info3["n_sources_staged"] == 1
    # device records give the same bytes
    d_src = lisreg.DeviceArray(_records(world["src"]))
    res4, fit4, _ = gpu_ctx.vgicp_align_batch([(d_src.ptr, len(src))], items, P)
    assert [_bits(r) for r in res4] == [_bits(r) for r in res] and fit4.tobytes() == fit.tobytes()


@pytest.mark.gpu
def test_best_rule_on_the_device_path(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.vgicp_default_params()
    src = _pcl(world["src"])
    items = [lisreg.VgicpItem(0, SLOT, world["guess"])] * 2
    res, fit, info = gpu_ctx.vgicp_align_batch([src], items, P)
    assert res[0]["converged"] and fit[0:1].tobytes() == fit[1:2].tobytes() and info["best"] == 1     # equal scores: the later item
    # an item that has not converged holds the lowest score (the true pose, no iterations allowed): computed, and passed over
    P0 = lisreg.vgicp_default_params(max_iters=0)
    res0, fit0, info0 = gpu_ctx.vgicp_align_batch([src], [lisreg.VgicpItem(0, SLOT, world["T_true"])] * 2, P0)
    assert info0["best"] == -1 and info0["n_rounds"] == 1 and not res0[0]["converged"] and res0[0]["n_evals"] == 1
    assert np.array_equal(res0[0]["T"], world["T_true"].astype(np.float32).astype(np.float64)) and 0 < fit0[0]
    want0 = B.fitness(world["tgt"], world["src"], res0[0]["T"])
    assert abs(fit0[0] - want0) <= 1e-10 * want0
    resn, fitn, infon = gpu_ctx.vgicp_align_batch([src], items, P, want_fitness=False)
    assert fitn is None and infon["best"] == -1 and [_bits(r) for r in resn] == [_bits(r) for r in res] and infon["n_rounds"] == info["n_rounds"]
    rese, fite, infoe = gpu_ctx.vgicp_align_batch([src], [], P)
    assert rese == [] and len(fite) == 0 and infoe == dict(best=-1, n_rounds=0, n_sources_staged=0)


@pytest.mark.gpu
def test_an_unconverged_item_with_the_lowest_score_is_not_the_best(gpu_ctx, world, scene_slot):
    """one outer iteration under epsilons of 5 cm and 10 mrad.  From the guess (0.3 m, 2 degrees off) the one step is far above them: not
    converged, but it ends close to the solution on the dense submap.  From the solution against every eighth point of the submap the
    step is below them: converged, with the larger score of a sparse target.  The loop's test passes the lower score over."""
    import lisreg
    src = _pcl(world["src"])
    solved = gpu_ctx.vgicp_align(SLOT, src, lisreg.vgicp_default_params(), world["guess"])
    assert solved["converged"]
    P1 = lisreg.vgicp_default_params(max_iters=1, transformation_epsilon=0.05, rotation_epsilon=0.01)
    sparse = world["tgt"][::8]
    gpu_ctx.vgicp_set_target(SLOT + 8, _pcl(sparse), P1)
    at_solution = solved["T"].astype(np.float32)
    items = [lisreg.VgicpItem(0, SLOT + 8, at_solution), lisreg.VgicpItem(0, SLOT, world["guess"]), lisreg.VgicpItem(0, SLOT + 8, at_solution)]
    res, fit, info = _assert_equals_singles(gpu_ctx, [src], items, P1, "unconverged with the lowest score")
    conv = [r["converged"] for r in res]
    want = np.array([B.fitness(sparse, world["src"], res[0]["T"]), B.fitness(world["tgt"], world["src"], res[1]["T"])])[[0, 1, 0]]
    print(f"[vgicp_batch] converged {conv}, fitness {fit.tolist()}, restatement {want.tolist()}, best {info['best']}")
    assert np.abs(fit - want).max() <= 1e-10 * want.max()
    assert conv == [True, False, True] and want[1] < want[0] * (1 - 1e-6)   # what the case is made for
    assert info["best"] == B.best(conv, want) == 2


@pytest.mark.gpu
def test_nan_holes_in_a_source_and_a_target(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.vgicp_default_params()
    holes_s, holes_t = world["src"].copy(), world["tgt"].copy()
    holes_s[::7] = np.nan
    holes_t[::5] = np.nan
    gpu_ctx.vgicp_set_target(SLOT + 7, _pcl(holes_t), P)
    sources = [_pcl(holes_s), _pcl(world["src"])]
    items = [lisreg.VgicpItem(0, SLOT, world["guess"]), lisreg.VgicpItem(1, SLOT + 7, world["guess"]), lisreg.VgicpItem(0, SLOT + 7, world["guess"])]
    res, fit, info = _assert_equals_singles(gpu_ctx, sources, items, P, "NaN holes")
    assert all(np.isfinite(r["T"]).all() and r["converged"] for r in res)
    assert 0 < res[0]["n_pairs_last"] <= len(holes_s) - len(holes_s[::7])
    want = np.array([B.fitness(world["tgt"], holes_s, res[0]["T"]), B.fitness(holes_t, world["src"], res[1]["T"]), B.fitness(holes_t, holes_s, res[2]["T"])])
    rel = np.abs(fit - want) / want
    print(f"[vgicp_batch] NaN holes: fitness {fit.tolist()}, worst error {rel.max():.3e} relative")
    assert rel.max() <= 1e-10, rel


@pytest.mark.gpu
def test_every_refusal_leaves_the_results_untouched(gpu_ctx, world, scene_slot):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    P = lisreg.vgicp_default_params()
    src = _pcl(world["src"])
    ok = lisreg.VgicpItem(0, SLOT, world["guess"])
    vp, dp = C.c_void_p, C.POINTER(C.c_double)

    def call(sources, items, params=P, null=()):
        """the raw call with a results array of 0xAB bytes: (return code, results untouched, fitness untouched, info.best)"""
        ptrs = (vp * max(len(sources), 1))(*[s.ctypes.data_as(vp) if s is not None else None for s in sources])
        ns = (C.c_int * max(len(sources), 1))(*[len(s) if s is not None else 5 for s in sources])
        its = (lisreg.VgicpItemC * max(len(items), 1))()
        for k, it in enumerate(items):
            its[k].source, its[k].slot = it.source, it.slot
            its[k].guess = None if it.guess is None else it.guess.ctypes.data_as(C.POINTER(C.c_float))
        res = (lisreg.VgicpResult * max(len(items), 1))()
        C.memset(res, 0xAB, C.sizeof(res))
        fit = np.full(max(len(items), 1), -7.0)
        info = lisreg.VgicpBatchInfo()
        rc = L.lisreg_vgicp_align_batch(ctx._h, None if "sources" in null else ptrs, None if "n" in null else ns, len(sources),
                                        src.dtype.itemsize if "stride" not in null else 8,
                                        lisreg.FMT_XYZIL if "stride" not in null else lisreg.FMT_XYZI, None if "items" in null else its, len(items),
                                        None if params is None else C.byref(params), None if "results" in null else res,
                                        fit.ctypes.data_as(dp), C.byref(info))
        return rc, bytes(res) == b"\xab" * C.sizeof(res), bool((fit == -7.0).all()), info.best

    def refused(word, *a, **kw):
        rc, untouched, fit_untouched, best = call(*a, **kw)
        assert rc == lisreg.ERR_ARG and untouched and fit_untouched and best == -1, (word, rc, untouched, fit_untouched, best)
        msg = L.lisreg_last_error(ctx._h).decode()
        assert word in msg, (word, msg)
    for what in ("items", "results", "sources", "n"):
        refused("NULL items", [src], [ok], null=(what,))
    for s in (-1, 1, 7):
        refused("source index", [src], [ok, lisreg.VgicpItem(s, SLOT, None)])
    for slot in (4242, -1):
        refused("no VGICP target", [src], [ok, lisreg.VgicpItem(0, slot, None)])
    # a slot built at another resolution among slots at the params': the batch has one set of params, so it is refused, whichever
    # side the params take
    ctx.vgicp_set_target(SLOT + 9, _pcl(world["tgt"]), lisreg.vgicp_default_params(resolution=2.0))
    refused("resolution differs", [src], [ok, lisreg.VgicpItem(0, SLOT + 9, world["guess"]), ok])
    refused("resolution differs", [src], [lisreg.VgicpItem(0, SLOT + 9, world["guess"]), ok], params=lisreg.vgicp_default_params(resolution=2.0))
    # a named source lisreg_vgicp_align would refuse, whichever item names it, behind valid ones
    bad = src.copy(); bad["z"][3] = -np.inf
    refused("fewer finite points", [src, src[:K - 1]], [ok, lisreg.VgicpItem(1, SLOT, None)])
    refused("infinite", [src, bad], [ok, lisreg.VgicpItem(1, SLOT, None)])
    refused("n <= 0", [src, src[:0]], [ok, lisreg.VgicpItem(1, SLOT, None)])
    refused("", [src, None], [ok, lisreg.VgicpItem(1, SLOT, None)])
    refused("", [src], [ok], null=("stride",))
    refused("NULL params", [src], [ok], params=None)
    for kw, word in ((dict(resolution=0.0), "resolution <= 0"), (dict(k_correspondences=40), "outside 4 .. 32"),
                     (dict(max_iters=-1), "bad transformation_epsilon"), (dict(lm_max_iterations=0), "bad transformation_epsilon"),
                     (dict(resolution=0.5), "resolution differs")):
        refused(word, [src], [ok], params=lisreg.vgicp_default_params(**kw))
    assert L.lisreg_vgicp_align_batch(ctx._h, None, None, 0, 0, 0, None, -1, C.byref(P), None, None, None) == lisreg.ERR_ARG
    # n_items == 0 is no refusal, whatever else is NULL; and the context stays usable
    info = lisreg.VgicpBatchInfo(best=5, n_rounds=5)
    assert L.lisreg_vgicp_align_batch(ctx._h, None, None, 0, 0, 0, None, 0, None, None, None, C.byref(info)) == lisreg.OK
    assert (info.best, info.n_rounds, info.n_sources_staged) == (-1, 0, 0)
    rc, untouched, fit_untouched, best = call([src], [ok])
    assert rc == lisreg.OK and not untouched and not fit_untouched and best == 0


@pytest.mark.gpu
def test_twenty_batch_calls_do_not_grow_device_memory(gpu_ctx, world, scene_slot, small_slots):
    import lisreg
    hip = lisreg.hip_runtime()

    def free_bytes():
        fr, tot = C.c_size_t(), C.c_size_t()
        assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
        return fr.value
    P = lisreg.vgicp_default_params()
    sources = [_pcl(world["src"]), small_slots[4]]
    items = [lisreg.VgicpItem(0, SLOT, world["guess"]), lisreg.VgicpItem(1, SMALL + 3, GUESS), lisreg.VgicpItem(0, SLOT, None)]
    first = gpu_ctx.vgicp_align_batch(sources, items, P)                   # every buffer of the call is made
    before = free_bytes()
    for _ in range(20):
        res, fit, info = gpu_ctx.vgicp_align_batch(sources, items, P)
    assert free_bytes() == before
    assert [_bits(r) for r in res] == [_bits(r) for r in first[0]] and fit.tobytes() == first[1].tobytes() and info == first[2]
    # a smaller batch afterwards fits into what is there
    gpu_ctx.vgicp_align_batch(sources[1:], [lisreg.VgicpItem(0, SMALL, GUESS)], P)
    assert free_bytes() == before


@pytest.mark.gpu
def test_profiling_reports_the_batch_in_the_slots_of_the_single_call(gpu_ctx, world, scene_slot):
    import lisreg
    P = lisreg.vgicp_default_params()
    src = _pcl(world["src"])
    items = [lisreg.VgicpItem(0, SLOT, world["guess"])] * 3
    gpu_ctx.set_profiling(True)
    try:
        res, fit, info = gpu_ctx.vgicp_align_batch([src], items, P)
        t = gpu_ctx.timing()
        resn, _, infon = gpu_ctx.vgicp_align_batch([src], items, P, want_fitness=False)
        tn = gpu_ctx.timing()
    finally:
        gpu_ctx.set_profiling(False)
    print(f"[vgicp_batch] timing of 3 items: {t}; without the fitness pass: {tn}")
    assert t["assoc_launches"] == info["n_rounds"] and t["solve_launches"] == 1          # one interval per round; the fitness search
    assert t["assoc_ms"] > 0 and t["solve_ms"] > 0 and t["index_ms"] > 0
    assert tn["assoc_launches"] == infon["n_rounds"] and tn["solve_launches"] == 0 and tn["assoc_ms"] > 0 and tn["index_ms"] > 0


@pytest.mark.gpu
def test_the_kept_grid_changes_nothing_of_the_single_call_paths(gpu_ctx, world):
    """lisreg_vgicp_set_target followed by the existing single-call paths still returns the golden rows"""
    import lisreg
    g = world["g"]
    P = lisreg.vgicp_default_params(transformation_epsilon=R.ALIGN_CASES[3][3])
    info = gpu_ctx.vgicp_set_target(SLOT + 10, _pcl(world["tgt"]), P)
    assert info == dict(dims=[int(v) for v in world["T"]["dims"]], n_voxels=1821, n_points=25401)
    V = gpu_ctx.vgicp_get_voxels(SLOT + 10)
    assert np.array_equal(V["cell_ids"], g["scene_cell_ids"]) and np.array_equal(V["counts"], g["scene_counts"])
    assert np.abs(V["cov6"][::8] - g["scene_cov6"]).max() <= 1e-9
    r = gpu_ctx.vgicp_align(SLOT + 10, _pcl(world["src"]), P, world["guess"])
    counts = g["align_counts"][3]
    assert (int(r["converged"]), r["iters"], r["n_evals"], r["n_rejected"], r["n_pairs_last"]) == tuple(int(v) for v in counts[:5])
    assert np.abs(r["T"] - g["align_T"][3]).max() <= 1e-6 and abs(r["error"] - g["align_fig"][3][0]) <= 1e-6 * g["align_fig"][3][0]
    out, pairs = gpu_ctx.vgicp_linearize(SLOT + 10, _pcl(world["src"]), P, g["lin_T"][0], True)
    k = len(R.LIN_SIZES) * 2 - 2                                           # the whole source at the first pose, with the Hessian
    assert pairs == int(g["lin_pairs"][k]) and np.all(np.abs(out - g["lin_out"][k]) <= 1e-10 * g["lin_abs"][k])


@pytest.mark.gpu
def test_batch_on_a_callers_busy_stream(env, world):
    """the source arrives late on the caller's stream, as in tests/test_caller_stream.py: the batch's results and scores equal the
    idle-stream ones, and a context left on its own stream reads the decoy"""
    e = env
    P = e.lisreg.vgicp_default_params(max_iters=1)                        # a short alignment, as in tests/test_vgicp.py
    e.ctx.vgicp_set_target(SLOT, _pcl(world["tgt"]), P)
    rs = _records(world["src"])
    near = world["guess"].copy()
    near[0, 3] += 0.02

    def make(dst):
        def run():
            items = [e.lisreg.VgicpItem(0, SLOT, world["guess"]), e.lisreg.VgicpItem(0, SLOT, near)]
            res, fit, info = e.ctx.vgicp_align_batch([(dst.ptr, len(rs))], items, P)
            return dict(T=np.stack([r["T"] for r in res]), counts=np.array([[r["iters"], r["n_evals"], r["n_pairs_last"]] for r in res]),
                        error=np.array([r["error"] for r in res]), fit=fit, best=info["best"])
        return run, (lambda r: r)
    o, _ = TCS.late_case(e, "vgicp_align_batch (device records)", rs, TCS.moved(rs, small=True), make)
    single = e.ctx.vgicp_align(SLOT, _pcl(world["src"]), P, world["guess"])
    assert o["T"][0].tobytes() == single["T"].tobytes() and o["error"][0] == single["error"] and list(o["counts"][0][:2]) == [1, 2]
