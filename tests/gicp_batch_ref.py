"""The definition of lisreg_gicp_align_batch, in numpy float64: the candidate loop of detectLoopClosureForSubMap
(src/node/subMapOptmizationNode.cpp:2779-2846 of the reference) with the one verifier whose block is live in
select_registration_method ("GICP", src/core/registration.cpp:137-146), over tests/gicp_ref.py and tests/fgicp_batch_ref.py, which this
file imports and does not change.

  * results: item k is gicp_ref.align of its source against its target from its guess — the batch is DEFINED as the loop of single
    alignments;
  * fitness(target, source, T) is fgicp_batch_ref.fitness over the source's finite points at the item's double final_transform
    T = X(x) G: the mean of the squared distance from x' = ((R0 a0 + R1 a1) + R2 a2) + t (in double from the float coordinates) to the
    nearest finite target point, ((dx dx + dy dy) + dz dz) in double from the float coordinates, without a cut-off — PCL's
    getFitnessScore() default (max_range = DBL_MAX), as §7m reads it.  Computed for every item, converged or not;
  * best(converged, fitness) is fgicp_batch_ref.best, unchanged: :2834-2840 — bestScore starts at DBL_MAX; the items are walked in
    order; one that has not converged, or whose score is ABOVE the best so far, is skipped; any other one becomes the best.  Equal
    scores therefore go to the later item; -1 when nothing converged.

One difference from NDT (tests/ndt_batch_ref.py): a GICP item that ends on fewer than 4 pairs (PCL's "need at least 4 points", a guess
100 m off among them) has converged = 0, where an NDT item without a pair "converges" at once.  Such an item is skipped by `best`, and
it still gets a score.

The second half of the file holds the shapes the batch's tests and tests/golden/make_golden_gicp_batch.py share, so that the golden
file and the tests cannot drift apart."""
import numpy as np

import fgicp_batch_ref as FB
import gicp_ref as R

DBL_MAX = FB.DBL_MAX
best = FB.best
fitness = FB.fitness


def align_batch(targets, sources, items, prm, want_fitness=True):
    """targets: slot -> (xyz float32, gicp_ref.build_target of it); sources: a list of (xyz float32, gicp_ref.prepare_source of it);
    items: a list of (source index, slot, guess or None).  Returns (results, fitness or None, best)."""
    results, scores = [], []
    for s, slot, guess in items:
        r = R.align(targets[slot][1], sources[s][1], prm, guess)
        results.append(r)
        if want_fitness:
            scores.append(fitness(targets[slot][0], sources[s][0], r["T"]))
    if not want_fitness:
        return results, None, -1
    return results, np.array(scores), best([r["converged"] for r in results], scores)


# ---- the shapes of the tests (tests/test_gicp_batch.py, tests/test_gicp_batch_host.py, tests/golden/make_golden_gicp_batch.py) ----------
SCENE = (1000, 0.05, 0.3)                  # gicp_ref.ALIGN_CASES[0]: target 25 401 points, source 2 939, a guess tests/test_gicp_ref.py qualifies
SCENE_B = (1001, 0.02, 0.1)                # the second slot's target
FULL, C63, C65, C129, C20, C129N, SNULL = range(7)        # indices into the sources
NAN_AT = (5, 64, 128)                      # of the 129-point cut: one of them lane 0 of the second wavefront
A, B = 0, 1                                # the two scene slots, as the items name them (the tests map them to slot numbers)
EIGHT = ((FULL, A, "guess"), (FULL, B, "guess"), (C63, A, "guess"), (C65, A, "guess"), (C129, A, "guess"), (C20, A, "guess"),
         (C129N, A, "guess"), (FULL, A, "far"))
FAR_ITEM = 7
PARAM_SETS = (("default", 0, {}), ("kind1", 1, {}), ("cap1", 0, dict(max_iters=1)))     # name, kind, overrides
EDGE_NS = (20, 21, 63, 64, 65, 4097)       # tests/test_gicp.py::small_sources: 4 097 = 65 partial records
EDGE_NT = (20, 21, 64, 65)
T_SMALL = R.F.se3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.08])


def cut(src, ns):
    return np.ascontiguousarray(src[::len(src) // ns][:ns])


def scene_sources(src):
    """the sources of the batch of eight: all of it, the cuts, the 129-point cut with three NaN records, one nobody names"""
    holes = cut(src, 129).copy()
    holes[list(NAN_AT)] = np.nan
    holes[NAN_AT[0], 1] = 0.5              # (a record with one NaN coordinate is no point either)
    out = [src, cut(src, 63), cut(src, 65), cut(src, 129), cut(src, 20), holes, None]
    assert [None if x is None else len(x) for x in out] == [2939, 63, 65, 129, 20, 129, None]
    return out


def scene_shapes():
    """raw clouds only (no restatement): dict(tgt = [A's, B's], xyz = the sources, guess, far)"""
    tgt_a, src, guess, T_true = R.F.scene(*SCENE)
    tgt_b = R.F.scene(*SCENE_B)[0]
    far = np.array(guess, np.float32).copy()
    far[0, 3] += 100.0
    return dict(tgt=[tgt_a, tgt_b], xyz=scene_sources(src), guess=np.asarray(guess, np.float32), far=far, T_true=T_true)


def edge_items():
    """(source size, target size) of the size-edge batch, in item order: every source against every target"""
    return [(ns, nt) for nt in EDGE_NT for ns in EDGE_NS]


def cutoff_case():
    """tests/test_gicp.py's cut-offs: the 74-point cloud with every 7th point NaN against the 65-point target from T_SMALL, and the
    max_correspondence_distance that leaves exactly 3 and exactly 4 pairs at the guess.  dict(tgt, src, guess, cuts = {3: , 4: })"""
    prm = R.params()
    txyz = R.small_cloud(65)
    Tt = R.build_target(txyz, prm)
    holes = R.small_cloud(74, seed=11)
    holes[::7] = np.nan
    S = R.prepare_source(holes, prm)
    guess = T_SMALL.astype(np.float32)
    sq32 = np.sort(R.find_pairs(Tt, S, guess.astype(np.float64), prm)["sq"][S["ok"]])
    return dict(tgt=txyz, src=holes, guess=guess, cuts={w: float(np.sqrt(0.5 * (sq32[w - 1] + sq32[w]))) for w in (3, 4)})
