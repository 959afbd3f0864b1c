"""The definition of lisreg_ndt_align_batch, in numpy float64: the candidate loop of detectLoopClosureForSubMap
(src/node/subMapOptmizationNode.cpp:2779-2846 of the reference) with the verifier the reference names first
(select_registration_method("NDT"), src/core/registration.cpp:147-155), over tests/ndt_ref.py and tests/fgicp_batch_ref.py, which this
file imports and does not change.

  * results: item k is ndt_ref.align of its source against its target from its guess — the batch is DEFINED as the loop of single
    alignments;
  * fitness(target, source, p) is fgicp_batch_ref.fitness over the source's finite points at the pose the evaluations use, R and t of
    ndt_ref.pose_matrices(p) in double (x' = Rx(a) Ry(b) Rz(c) x + t), not the float final_transform: the mean of the squared distance
    from x' = ((R0 a0 + R1 a1) + R2 a2) + t (in double from the float coordinates) to the nearest finite target point,
    ((dx dx + dy dy) + dz dz) in double from the float coordinates, without a cut-off.  This is the same reading of PCL's
    getFitnessScore() default (max_range = DBL_MAX) as §7m's: the score is a property of the two clouds and the pose, not of the
    verifier, so NDT's voxels play no part in it.  Computed for every item, converged or not (a source with no pair at its guess
    "converges" at once in NDT: its score says how far off it is);
  * best(converged, fitness) is fgicp_batch_ref.best, unchanged: :2834-2840 — bestScore starts at DBL_MAX; the items are walked in
    order; one that has not converged, or whose score is ABOVE the best so far, is skipped; any other one becomes the best.  Equal
    scores therefore go to the later item; -1 when nothing converged."""
import numpy as np

import fgicp_batch_ref as FB
import ndt_ref as R

DBL_MAX = FB.DBL_MAX
best = FB.best


def fitness(tgt_xyz32, src_xyz32, p):
    """at the 4x4 of the pose p = (tx, ty, tz, a, b, c) in double, as the evaluations transform the source"""
    return FB.fitness(tgt_xyz32, src_xyz32, R.matrix_from_p(np.asarray(p, np.float64)))


def align_batch(targets, sources, items, prm, want_fitness=True):
    """targets: slot -> (xyz float32, ndt_ref.build_target of it); sources: a list of xyz float32 arrays; items: a list of (source index,
    slot, guess or None).  Returns (results, fitness or None, best)."""
    results, scores = [], []
    for s, slot, guess in items:
        r = R.align(targets[slot][1], sources[s], prm, guess)
        results.append(r)
        if want_fitness:
            scores.append(fitness(targets[slot][0], sources[s], r["p"]))
    if not want_fitness:
        return results, None, -1
    return results, np.array(scores), best([r["converged"] for r in results], scores)
