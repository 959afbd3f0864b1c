"""The definition of lisreg_fgicp_align_batch, in numpy float64: the candidate loop of detectLoopClosureForSubMap
(src/node/subMapOptmizationNode.cpp:2779-2846 of the reference) over tests/fgicp_ref.py, which this file imports and does not change.

  * results: item k is fgicp_ref.align of its source against its target from its guess — the batch is DEFINED as the loop of single
    alignments;
  * fitness(target, source, T): the mean, over the source's finite points, of the squared distance from x' = ((R0 a0 + R1 a1) + R2 a2) + t
    (in double from the float coordinates) to the nearest finite target point, ((dx dx + dy dy) + dz dz) in double from the float
    coordinates — fgicp_ref's search without the cut-off, which is how the host mirror already reads PCL's getFitnessScore() default
    (max_range = DBL_MAX).  Computed for every item, converged or not;
  * best(converged, fitness): :2834-2840 — bestScore starts at DBL_MAX; the items are walked in order; one that has not converged, or
    whose score is ABOVE the best so far, is skipped; any other one becomes the best.  Equal scores therefore go to the later item;
    -1 when nothing converged."""
import numpy as np

import fgicp_ref as R

DBL_MAX = float(np.finfo(np.float64).max)


def fitness(tgt_xyz32, src_xyz32, T, chunk=256):
    tgt = np.asarray(tgt_xyz32, np.float32).reshape(-1, 3)
    src = np.asarray(src_xyz32, np.float32).reshape(-1, 3)
    b = tgt[~np.isnan(tgt).any(1)].astype(np.float64)
    a = src[~np.isnan(src).any(1)].astype(np.float64)
    xt = R.transform_points(np.asarray(T, np.float64), a)
    total = 0.0
    for i in range(0, len(xt), chunk):
        q = xt[i:i + chunk]
        dx, dy, dz = b[None, :, 0] - q[:, 0:1], b[None, :, 1] - q[:, 1:2], b[None, :, 2] - q[:, 2:3]
        total += float(((dx * dx + dy * dy) + dz * dz).min(axis=1).sum())
    return total / len(xt)


def best(converged, scores):
    best_k, best_score = -1, DBL_MAX
    for k, (c, s) in enumerate(zip(converged, scores)):
        if not c or s > best_score:
            continue
        best_score, best_k = s, k
    return best_k


def align_batch(targets, sources, items, prm, want_fitness=True):
    """targets: slot -> (xyz float32, fgicp_ref.build_target of it); sources: a list of (xyz float32, prepare_source of it); items: a list
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
