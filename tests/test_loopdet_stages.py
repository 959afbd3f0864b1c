"""Loop detection stage by stage: the yaw search and ICP (k_loop_icp), the scores (k_loop_score) and the selection with its matched
transforms (k_loop_select) against the restatement applied to the device's own input to each stage (loopdet_stage_ref.forced_check),
with no allowance: shifts, ICP counters and selections are equal, scores to the double's bits.  The inputs are the three-lap drive of
test_loopdet_kinds, extended by a slightly negative yaw difference, and crafted frames for the branches a random drive misses: ties of
every shift, ties of every fourth, equal candidates, thresholds met exactly, no yaw shift, empty sector clouds, empty descriptors.
The CPU tests run the restatement alone and assert that each case still reaches the branch it exists for."""
import numpy as np
import pytest

import loopdet_ref as R
import loopdet_kinds_ref as K
import loopdet_stage_ref as S

ALL_CASES = ["drive"] + S.CRAFTED
DB = {name: 11 + (j % 5) for j, name in enumerate(ALL_CASES)}          # databases 11 .. 15: the other loop-detection tests use 0 .. 10


# ---- CPU: the fixtures reach their branches --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ALL_CASES)
def test_case_reaches_its_branch_in_the_restatement(name, oracle):
    """EPSCGenerationKinds with the oracle's ICP on the case's frames: the ties exist, the pairs are gated, NO_SHIFT is reached ...;
    for the drive: at least 40 candidates, every descriptor kind selected at least 10 times, a wrapped yaw above 331 sectors and a
    yaw difference beyond pi."""
    if name == "strict":
        S.strict_runs(lambda params, label_thr: S.reference(name, oracle, params, label_thr))
    else:
        S.CHECKS[name](S.reference(name, oracle))


@pytest.mark.parametrize("name", ALL_CASES)
def test_selection_glue_equals_the_restatement(name, oracle):
    ref = S.reference(name, oracle)
    for k, (o, ms) in enumerate(zip(ref["out"], ref["matches"])):
        cands = [(c["history_id"], [c["score"][kk] for kk in range(6)] + [c["pos_distance"]]) for c in o["candidates"]]
        got = S.select(cands, ref["params"][2], ref["label_thr"])
        assert [(a, b, S.bits(c)) for a, b, c in got] == [(a, b, S.bits(c)) for a, b, c in ms], (name, k)


@pytest.mark.parametrize("name", ALL_CASES)
def test_reference_stays_inside_the_edge_cap_under_one_atan2_ulp(name, oracle, monkeypatch):
    """the forced check allows the device's pair descriptor 16 cells off the restatement's (an atan2f ulp at a sector edge): with
    its own arctan2 one float32 ulp up or down, the restatement moves no more cells than that for any pair of the case (none at all
    on the crafted frames, whose points keep a quarter of a degree from every edge)."""
    ref = S.reference(name, oracle)
    frames = S.case_frames(name)
    worst = 0
    for up in (False, True):
        monkeypatch.setattr(R, "np", S.OneUlpNumpy(up))
        for r in ref["records"]:
            f = frames[r["frame"]]
            moved = K.all_descriptors(f["corner"], f["surf"], f["semantic"], r["icp"]["T"])
            worst = max([worst] + [int(np.count_nonzero(moved[kk] != r["D"][kk])) for kk in range(6)])
        monkeypatch.undo()
    assert worst <= (S.EDGE_CAP if name == "drive" else 0), worst


# ---- GPU: every stage against the restatement on the device's own input ----------------------------------------------------------

@pytest.mark.gpu
def test_forced_drive(gpu_ctx, oracle):
    """the 73-key-frame drive, all seven kinds: 47 candidates, every kind selected 47 times (SSC 39).  The largest difference of a
    matched rotation entry from K.planar on the device's own transform, over the drive and the crafted cases on an MI355X, is
    5.96e-8 (one float32 ulp below 1); the bound is 1e-5, derived: a few ulp of pi from atan2f and a few ulp of 1 from sinf / cosf
    stay below 2e-6 (forced checks)."""
    S.check_drive(S.reference("drive", oracle))
    run = S.forced_check(gpu_ctx, oracle, "drive", DB["drive"])
    print("forced drive: candidates", run["n_cand"], "selected per kind", run["selected"].tolist(), "largest rotation difference", run["rot"])
    S.check_drive(run)
    assert all(run["selected"][:6] >= 10), run["selected"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", S.CRAFTED)
def test_forced_crafted(name, gpu_ctx, oracle):
    if name == "strict":
        S.strict_runs(lambda params, label_thr: S.forced_check(gpu_ctx, oracle, name, DB[name], params, label_thr))
        return
    S.CHECKS[name](S.reference(name, oracle))
    run = S.forced_check(gpu_ctx, oracle, name, DB[name])
    print("forced", name, ": candidates", run["n_cand"], "largest rotation difference", run["rot"])
    S.CHECKS[name](run)
