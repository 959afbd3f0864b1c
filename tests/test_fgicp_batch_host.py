"""lisreg_fgicp_align_batch without a GPU: the resumable Levenberg-Marquardt stepper against lm_optimise on scripted
evaluations, the structs and the symbol of include/lisreg.h, and tests/fgicp_batch_ref.py (the fitness score against a kd-tree, the
`best` rule on score lists made by hand, the batch as the loop of single alignments).  The GPU side is tests/test_fgicp_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fgicp_batch_ref as B
import fgicp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
BRANCHES = ("no_pair", "max_iters_zero", "converged", "rejected_while_converged", "not_positive_definite", "out_of_trials", "max_iters")


def test_the_stepper_reproduces_lm_optimise_on_scripted_evaluations(tmp_path):
    """800 seeded scripts of out[29] records: the same requests (the bytes of T, the with_hessian flag) and the same bytes in every field
    of LmResult, and every way out of the loop taken at least once (the program exits non-zero at the first script that differs)"""
    exe = str(tmp_path / "lm_stepper_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, os.path.join(HOST, "lm_stepper_check.cpp"), "-o", exe])
    r = subprocess.run([exe, "800"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "lm_stepper_check ok" in r.stdout, r.stdout + r.stderr
    m = re.search(r"scripts (\d+) calls (\d+) rejected (\d+)", r.stdout)
    assert m and int(m.group(1)) == 800 and int(m.group(2)) > 1600 and int(m.group(3)) > 0
    hits = {k: int(v) for k, v in re.findall(r"hit (\w+) (\d+)", r.stdout)}
    assert set(hits) == set(BRANCHES), hits
    for name in BRANCHES:
        assert hits[name] > 0, (name, hits)
    assert sum(hits.values()) == 800
    # (g++ compiled it: the header has no HIP in it) it builds on lisreg_vgicp_host.hpp and defines no loop of its own helpers
    text = open(os.path.join(CSRC, "lisreg_lm_stepper.hpp")).read()
    assert '#include "lisreg_vgicp_host.hpp"' in text and "hip_runtime" not in text and "__device__" not in text


def _struct_from_header(name):
    """a ctypes mirror of `typedef struct name { ... } name;` parsed from include/lisreg.h (ints, doubles, pointers)"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.match(r"(?:const\s+)?(\w+)\s*(\*?)\s*(\w+)$", decl)
        assert m, decl
        fields.append((m.group(3), C.c_void_p if m.group(2) else {"int": C.c_int, "double": C.c_double, "float": C.c_float}[m.group(1)]))
    return type(name, (C.Structure,), {"_fields_": fields})


def test_structs_and_symbol_match_the_header():
    import lisreg
    for name, mine, size in (("lisreg_fgicp_item", lisreg.FgicpItemC, 16), ("lisreg_fgicp_batch_info", lisreg.FgicpBatchInfo, 16)):
        theirs = _struct_from_header(name)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name
    assert [(n, getattr(lisreg.FgicpItemC, n).offset) for n, _ in lisreg.FgicpItemC._fields_] == [("source", 0), ("slot", 4), ("guess", 8)]
    assert [n for n, _ in lisreg.FgicpBatchInfo._fields_] == ["best", "n_rounds", "n_sources_staged", "reserved"]
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    assert hasattr(L, "lisreg_fgicp_align_batch") and "lisreg_fgicp_align_batch" in lisreg.ABI_SYMBOLS
    assert re.search(r"^\s*int\s+lisreg_fgicp_align_batch\s*\(", hdr, re.M)
    block = hdr[hdr.index("§7m"):hdr.index("loop-closure candidate detection: FEPSC")]
    for text in ("subMapOptmizationNode.cpp:2779-2846", ":2834-2840", "tests/fgicp_batch_ref.py", "getFitnessScore"):
        assert text in block, text
    # no context: refused before anything is read
    assert L.lisreg_fgicp_align_batch(None, None, None, 0, 0, 0, None, 0, None, None, None, None) == lisreg.ERR_ARG
    it = lisreg.FgicpItem(2, 5, np.eye(4))
    assert (it.source, it.slot) == (2, 5) and it.guess.dtype == np.float32 and it.guess.shape == (16,) and lisreg.FgicpItem(0, 0).guess is None


def test_fitness_equals_the_kd_trees_on_the_scene():
    from scipy.spatial import cKDTree
    W = R.world()
    tgt, src = W["tgt"], W["src"]
    tree = cKDTree(tgt.astype(np.float64))
    for T in (W["guess"].astype(np.float64), W["T_true"]):
        d, _ = tree.query(R.transform_points(T, src.astype(np.float64)), k=1)
        want = float(np.mean(d * d))
        got = B.fitness(tgt, src, T)
        print(f"[fgicp_batch_ref] fitness {got:.9e} against the kd-tree's {want:.9e}")
        assert abs(got - want) <= 1e-12 * want
    assert B.fitness(tgt, src, W["T_true"]) < 0.5 * B.fitness(tgt, src, W["guess"].astype(np.float64))
    # NaN points are no points, in either cloud; no cut-off: a source 100 m away still has a score
    holes_t, holes_s = tgt.copy(), src.copy()
    holes_t[::5] = np.nan
    holes_s[::7] = np.nan
    d, _ = cKDTree(np.delete(tgt, np.s_[::5], 0).astype(np.float64)).query(
        R.transform_points(W["T_true"], np.delete(src, np.s_[::7], 0).astype(np.float64)), k=1)
    assert abs(B.fitness(holes_t, holes_s, W["T_true"]) - np.mean(d * d)) <= 1e-12 * np.mean(d * d)
    far = W["T_true"].copy()
    far[0, 3] += 100.0
    assert B.fitness(tgt, src, far) > 50.0 ** 2
    # the same search as fgicp_ref's, without its cut-off
    p = R.find_pairs(W["T"], W["S"], W["T_true"], R.params(1))
    assert (p["idx"] >= 0).all() and abs(B.fitness(tgt, src, W["T_true"]) - p["sq"].mean()) <= 1e-12 * p["sq"].mean()


def test_best_rule_on_score_lists_made_by_hand():
    assert B.best([1, 1, 1], [0.3, 0.1, 0.2]) == 1
    assert B.best([1, 1, 1], [0.2, 0.1, 0.1]) == 2                      # a tie: `score > bestScore` does not skip it, the later one wins
    assert B.best([1, 1], [0.1, 0.1]) == 1
    assert B.best([0, 0, 0], [0.1, 0.2, 0.3]) == -1                     # none converged
    assert B.best([1, 0, 1], [0.3, 0.01, 0.2]) == 2                     # the lowest score belongs to an item that did not converge
    assert B.best([0, 1, 0], [0.01, 5.0, 0.02]) == 1
    assert B.best([], []) == -1
    assert B.best([1], [B.DBL_MAX]) == 0 and B.best([1], [np.inf]) == -1  # bestScore starts at DBL_MAX


def test_the_batch_is_the_loop_of_single_alignments():
    """small clouds: two targets, two sources, four items (one from a guess without a pair, one with a NULL guess)"""
    prm = R.params(max_iters=3)
    tg = {s: (R.small_cloud(n), R.build_target(R.small_cloud(n), prm)) for s, n in ((3, 64), (9, 65))}
    sr = [(R.small_cloud(n, seed=11), R.prepare_source(R.small_cloud(n, seed=11), prm)) for n in (63, 65)]
    g = R.se3_exp(np.r_[0.02, -0.03, 0.05, 0.1, -0.05, 0.08]).astype(np.float32)
    far = g.copy()
    far[0, 3] += 100.0
    items = [(0, 3, g), (1, 9, far), (1, 3, None), (0, 9, g)]
    res, fit, best = B.align_batch(tg, sr, items, prm)
    for (s, slot, guess), r, f in zip(items, res, fit):
        alone = R.align(tg[slot][1], sr[s][1], prm, guess)
        assert np.array_equal(alone["T"], r["T"]) and alone["n_evals"] == r["n_evals"] and alone["error"] == r["error"]
        assert f == B.fitness(tg[slot][0], sr[s][0], r["T"])
    assert (res[1]["converged"], res[1]["iters"], res[1]["n_evals"]) == (0, 0, 1) and np.array_equal(res[1]["T"], far.astype(np.float64))
    assert fit[1] > 90.0 ** 2 and best == B.best([r["converged"] for r in res], fit) and best != 1
    assert B.align_batch(tg, sr, items, prm, want_fitness=False)[1:] == (None, -1)


def test_fgicp_batch_smoke_compiles_and_the_mirror_has_the_verifier():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists (builds it if the tree is fresh)
    subprocess.check_call(["make", "-s", "-C", HOST, "fgicp_batch_smoke"])
    assert os.path.exists(os.path.join(HOST, "fgicp_batch_smoke"))
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    body = hdr[hdr.index("class FastGicpVerifier"):hdr.index("// OptimizedICPGN")]
    for name in ("setCandidateTarget", "addCandidate", "clearCandidates", "alignAll", "best", "result", "fitness", "hasConverged",
                 "lisreg_fgicp_align_batch"):
        assert name in body, name


@pytest.mark.gpu
def test_fgicp_batch_smoke_runs():
    exe = os.path.join(HOST, "fgicp_batch_smoke")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "fgicp_batch_smoke ok" in r.stdout, r.stdout + r.stderr
