"""The two batch verifiers on ONE context (lis-slam_amd/csrc/lisreg_batch_driver.hpp): lisreg_fgicp_align_batch and
lisreg_vgicp_align_batch run through one host driver, keep their buffers in two instances of one struct and score with one fitness
kernel.  These tests guard that sharing: a call of one family leaves nothing behind that a call of the other (or the next call of its
own) reads.  The families on their own are tests/test_fgicp_batch.py and tests/test_vgicp_batch.py.

The bounds: every field of every result equal as raw bytes and fitness bit-identical between the runs of a family, and equal to the
single call's bytes; FastGICP's fitness within 1e-10 relative of fgicp_batch_ref.fitness at the returned final_transform, the bound of
tests/test_fgicp_batch.py (a sum of positive terms: the project's sum bar).

Shapes: targets of 64 and 65 points; sources of 63, 65 and 129 points (a wavefront short by a lane, one lane into a second, one lane
into a third); four items per family, among them a NULL guess and a guess 100 m away (no pair)."""
import numpy as np
import pytest

import fgicp_batch_ref as FB
import fgicp_ref as FR
import test_fgicp_batch as TFB

_pcl, _bits, GUESS = TFB._pcl, TFB._bits, TFB.GUESS
SLOTS = (70, 71)                                        # in either family's numbering: the targets of 64 and of 65 points
NT, NS = (64, 65), (63, 65, 129)
FAR = GUESS.copy()
FAR[0, 3] += 100.0
ITEMS = ((0, 0, GUESS), (1, 1, FAR), (2, 0, None), (1, 1, GUESS))      # (source, target, guess)


@pytest.fixture(scope="module")
def both(gpu_ctx):
    """per family: (batch call, single call, params, items); and the sources, which the families share"""
    import lisreg
    ctx = gpu_ctx
    fam = {}
    for name, set_target, default_params, item, batch, single in (
            ("fgicp", ctx.fgicp_set_target, lisreg.fgicp_default_params, lisreg.FgicpItem, ctx.fgicp_align_batch, ctx.fgicp_align),
            ("vgicp", ctx.vgicp_set_target, lisreg.vgicp_default_params, lisreg.VgicpItem, ctx.vgicp_align_batch, ctx.vgicp_align)):
        P = default_params()
        for slot, nt in zip(SLOTS, NT):
            assert set_target(slot, _pcl(FR.small_cloud(nt)), P)["n_points"] == nt
        fam[name] = dict(batch=batch, single=single, P=P, items=[item(s, SLOTS[t], g) for s, t, g in ITEMS])
    return fam, [_pcl(FR.small_cloud(ns, seed=11)) for ns in NS]


@pytest.mark.gpu
def test_the_two_families_on_one_context_do_not_disturb_each_other(both):
    fam, sources = both
    order = ("fgicp", "vgicp", "fgicp", "vgicp")
    runs = [(name, fam[name]["batch"](sources, fam[name]["items"], fam[name]["P"])) for name in order]
    for name, f in fam.items():
        (res, fit, info), (res2, fit2, info2) = [r for n, r in runs if n == name]
        alone = [f["single"](it.slot, sources[it.source], f["P"], None if it.guess is None else it.guess.reshape(4, 4)) for it in f["items"]]
        diff2 = [k for k, (a, b) in enumerate(zip(res, res2)) if _bits(a) != _bits(b)]
        diff1 = [k for k, (a, b) in enumerate(zip(res, alone)) if _bits(a) != _bits(b)]
        evals = [r["n_evals"] for r in res]
        print(f"[gicp_batch_shared] {name}: evaluations {evals}, rounds {info['n_rounds']}, fitness {fit.tolist()}, items differing "
              f"between the two runs {diff2}, from the single calls {diff1}")
        assert not diff2 and not diff1, (name, diff2, diff1)
        assert fit.tobytes() == fit2.tobytes() and info == info2, name
        assert info["n_rounds"] == max(evals) and info["n_sources_staged"] == len(NS), (name, info)
        far = res[1]                                                     # the guess without a pair: over after one evaluation, still scored
        assert (far["converged"], far["iters"], far["n_evals"], far["n_pairs_last"]) == (False, 0, 1, 0) and fit[1] > 90.0 ** 2, name
        assert max(evals) > 1 and np.isfinite(fit).all(), name


@pytest.mark.gpu
def test_fgicp_fitness_with_and_without_the_fitness_pass_in_between(both):
    fam, sources = both
    f = fam["fgicp"]
    res, fit, info = f["batch"](sources, f["items"], f["P"])
    resn, fitn, infon = f["batch"](sources, f["items"], f["P"], want_fitness=False)
    res2, fit2, info2 = f["batch"](sources, f["items"], f["P"])
    want = np.array([FB.fitness(FR.small_cloud(NT[t]), FR.small_cloud(NS[s], seed=11), r["T"]) for (s, t, _), r in zip(ITEMS, res)])
    rel = np.abs(fit - want) / want
    print(f"[gicp_batch_shared] fgicp fitness {fit.tolist()}, worst error {rel.max():.3e} relative")
    assert rel.max() <= 1e-10, rel
    assert fit.tobytes() == fit2.tobytes() and info == info2 and [_bits(r) for r in res2] == [_bits(r) for r in res]
    assert fitn is None and infon["best"] == -1 and infon["n_rounds"] == info["n_rounds"] and [_bits(r) for r in resn] == [_bits(r) for r in res]
