"""What lisreg_icp_gn_match_batch computes, as a definition: the candidate loop of detectLoopClosureForSubMapICP
(src/node/subMapOptmizationNode.cpp:2496-2621) over OptimizedICPGN (src/core/registration.cpp:19-115).

The reference keeps `static OptimizedICPGN myICP(30, 10)` and, per candidate, calls SetTargetCloud, Match, GetFitnessScore and
HasConverged, then applies the `best` rule of :2551-2558:

    double bestScore = DBL_MAX;   int best = -1;
    for every candidate k, in order:
        if (!HasConverged() || score > bestScore) continue;      // HasConverged() returns true: it drops out
        bestScore = score; best = k;

with score the FLOAT GetFitnessScore() returns, compared in double.  So an equal score goes to the LATER candidate, a NaN score is
taken (NaN > x is false) and +inf is skipped (inf > DBL_MAX).  The verifier holds no state from one Match to the next, so the batch is
the loop of single matches: oracle.icp_gn_match, the CPU restatement of registration.cpp:19-115."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)


def best_of(scores):
    """the index :2551-2558 ends with for these fitness scores (floats), -1 for none"""
    best_score, best = DBL_MAX, -1
    for k, s in enumerate(scores):
        s = float(np.float32(s))
        if s > best_score:
            continue
        best_score, best = s, k
    return best


def match_batch(oracle, targets, sources, items, max_iterations, max_correspond_distance):
    """targets: {slot: cloud}; items: (source index, slot, predict_pose or None).  Returns (results, best)."""
    eye = np.eye(4, dtype=np.float32)
    results = [oracle.icp_gn_match(targets[slot], sources[s], max_iterations, max_correspond_distance, eye if pose is None else pose)
               for s, slot, pose in items]
    return results, best_of([r["fitness"] for r in results])
