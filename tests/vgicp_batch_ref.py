"""The definition of lisreg_vgicp_align_batch, in numpy float64: the candidate loop of detectLoopClosureForSubMap
(src/node/subMapOptmizationNode.cpp:2779-2846 of the reference) with the verifier of :2771 (FAST_VGICP), over tests/vgicp_ref.py and
tests/fgicp_batch_ref.py, which this file imports and does not change.

  * results: item k is vgicp_ref.align of its source against its target from its guess — the batch is DEFINED as the loop of single
    alignments;
  * fitness(target, source, T) is fgicp_batch_ref.fitness, unchanged: the mean, over the source's finite points, of the squared distance
    from x' = ((R0 a0 + R1 a1) + R2 a2) + t (in double from the float coordinates) to the nearest finite target point,
    ((dx dx + dy dy) + dz dz) in double from the float coordinates, without a cut-off.  This is the same reading of PCL's
    getFitnessScore() default (max_range = DBL_MAX) as §7m's: the score is a property of the two clouds and the pose, not of the
    verifier, so VGICP's voxels play no part in it.  Computed for every item, converged or not;
  * best(converged, fitness) is fgicp_batch_ref.best, unchanged: :2834-2840 — bestScore starts at DBL_MAX; the items are walked in
    order; one that has not converged, or whose score is ABOVE the best so far, is skipped; any other one becomes the best.  Equal
    scores therefore go to the later item; -1 when nothing converged."""
import numpy as np

import fgicp_batch_ref as FB
import vgicp_ref as R

DBL_MAX = FB.DBL_MAX
fitness = FB.fitness
best = FB.best


def align_batch(targets, sources, items, prm, want_fitness=True):
    """targets: slot -> (xyz float32, vgicp_ref.build_target of it); sources: a list of (xyz float32, prepare_source of it); items: a list
    of (source index, slot, guess or None).  Returns (results, fitness or None, best)."""
    results, scores = [], []
    for s, slot, guess in items:
        r = R.align(targets[slot][1], sources[s][1], prm, guess)
        results.append(r)
        if want_fitness:
            scores.append(fitness(targets[slot][0], sources[s][0], r["T"]))
    if not want_fitness:
        return results, None, -1
    return results, np.array(scores), best([r["converged"] for r in results], scores)
