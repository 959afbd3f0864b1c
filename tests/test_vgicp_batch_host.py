"""lisreg_vgicp_align_batch without a GPU: the structs and the symbol of include/lisreg.h, and tests/vgicp_batch_ref.py
(the batch as the loop of single alignments, the fitness score against a kd-tree, the `best` rule on score lists made by hand), the
shared headers of the two batch units, the smoke program of the host mirror.  The GPU side is tests/test_vgicp_batch.py; the
Levenberg-Marquardt stepper the batch drives is covered by tests/test_fgicp_batch_host.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import vgicp_batch_ref as B
import vgicp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HOST = os.path.join(ROOT, "lis-slam_amd", "host")


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
    for name, mine, size in (("lisreg_vgicp_item", lisreg.VgicpItemC, 16), ("lisreg_vgicp_batch_info", lisreg.VgicpBatchInfo, 16)):
        theirs = _struct_from_header(name)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name
    assert [(n, getattr(lisreg.VgicpItemC, n).offset) for n, _ in lisreg.VgicpItemC._fields_] == [("source", 0), ("slot", 4), ("guess", 8)]
    assert [n for n, _ in lisreg.VgicpBatchInfo._fields_] == ["best", "n_rounds", "n_sources_staged", "reserved"]
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    assert hasattr(L, "lisreg_vgicp_align_batch") and "lisreg_vgicp_align_batch" in lisreg.ABI_SYMBOLS
    assert re.search(r"^\s*int\s+lisreg_vgicp_align_batch\s*\(", hdr, re.M)
    block = hdr[hdr.index("§7n: VGICP verification"):hdr.index("§7l: FastGICP registration")]
    for text in ("subMapOptmizationNode.cpp:2779-2846", ":2834-2840", ":2771", "tests/vgicp_batch_ref.py", "getFitnessScore"):
        assert text in block, text
    # the section follows §7k's, and the timing comment names the batch
    assert hdr.index("§7k: voxelised GICP") < hdr.index("§7n: VGICP verification")
    assert "lisreg_vgicp_align_batch" in hdr[hdr.index("Per-kernel timing"):hdr.index("int  lisreg_set_profiling")]
    # no context: refused before anything is read
    assert L.lisreg_vgicp_align_batch(None, None, None, 0, 0, 0, None, 0, None, None, None, None) == lisreg.ERR_ARG
    it = lisreg.VgicpItem(2, 5, np.eye(4))
    assert (it.source, it.slot) == (2, 5) and it.guess.dtype == np.float32 and it.guess.shape == (16,) and lisreg.VgicpItem(0, 0).guess is None


def test_the_batch_is_the_loop_of_single_alignments():
    """small clouds: two targets, two sources, two items for the comparison (and two more: a guess without a pair, a NULL guess)"""
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
        assert alone["converged"] == r["converged"] and alone["iters"] == r["iters"]
        assert f == B.fitness(tg[slot][0], sr[s][0], r["T"])
    assert res[0]["n_evals"] > 1 and res[3]["n_evals"] > 1
    assert (res[1]["converged"], res[1]["iters"], res[1]["n_evals"]) == (0, 0, 1) and np.array_equal(res[1]["T"], far.astype(np.float64))
    assert fit[1] > 90.0 ** 2 and best == B.best([r["converged"] for r in res], fit) and best != 1
    assert B.align_batch(tg, sr, items, prm, want_fitness=False)[1:] == (None, -1)


def test_fitness_equals_the_kd_trees_on_the_scene():
    from scipy.spatial import cKDTree
    W = R.world()
    tgt, src = W["tgt"], W["src"]
    tree = cKDTree(tgt.astype(np.float64))
    for T in (W["guess"].astype(np.float64), W["T_true"]):
        d, _ = tree.query(R.transform_points(T, src.astype(np.float64)), k=1)
        want = float(np.mean(d * d))
        got = B.fitness(tgt, src, T)
        print(f"[vgicp_batch_ref] fitness {got:.9e} against the kd-tree's {want:.9e}")
        assert abs(got - want) <= 1e-12 * want
    assert B.fitness(tgt, src, W["T_true"]) < 0.5 * B.fitness(tgt, src, W["guess"].astype(np.float64))
    # NaN points are no points, in the target, in the source, in both; no cut-off: a source 100 m away still has a score
    holes_t, holes_s = tgt.copy(), src.copy()
    holes_t[::5] = np.nan
    holes_s[::7] = np.nan
    cut_t, cut_s = np.delete(tgt, np.s_[::5], 0).astype(np.float64), np.delete(src, np.s_[::7], 0).astype(np.float64)
    for ht, hs, ct, cs in ((holes_t, src, cut_t, src.astype(np.float64)), (tgt, holes_s, tgt.astype(np.float64), cut_s), (holes_t, holes_s, cut_t, cut_s)):
        d, _ = cKDTree(ct).query(R.transform_points(W["T_true"], cs), k=1)
        assert abs(B.fitness(ht, hs, W["T_true"]) - np.mean(d * d)) <= 1e-12 * np.mean(d * d)
    far = W["T_true"].copy()
    far[0, 3] += 100.0
    assert B.fitness(tgt, src, far) > 50.0 ** 2


def test_best_rule_on_score_lists_made_by_hand():
    assert B.best([1, 1, 1], [0.3, 0.1, 0.2]) == 1
    assert B.best([1, 1, 1], [0.2, 0.1, 0.1]) == 2                      # a tie: `score > bestScore` does not skip it, the later one wins
    assert B.best([1, 1], [0.1, 0.1]) == 1
    assert B.best([0, 0, 0], [0.1, 0.2, 0.3]) == -1                     # none converged
    assert B.best([1, 0, 1], [0.3, 0.01, 0.2]) == 2                     # the lowest score belongs to an item that did not converge
    assert B.best([0, 1, 0], [0.01, 5.0, 0.02]) == 1
    assert B.best([], []) == -1
    assert B.best([1], [B.DBL_MAX]) == 0 and B.best([1], [np.inf]) == -1  # bestScore starts at DBL_MAX


def test_the_restatement_is_fgicp_batch_refs_reading():
    import fgicp_batch_ref as FB
    assert B.fitness is FB.fitness and B.best is FB.best and B.DBL_MAX == FB.DBL_MAX
    assert "getFitnessScore" in B.__doc__ and "max_range = DBL_MAX" in B.__doc__


def test_both_units_share_one_copy_of_the_lane_body_and_of_the_round_helpers():
    """the per-lane arithmetic and the totals exist once in the sources, and every unit that inlines them is built without contraction"""
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    for needle, home in (("void vg_linearize_lane(", "lisreg_vgicp_lane.hpp"), ("struct VoxelView {", "lisreg_ctx.hpp"),
                         ("struct VgPose {", "lisreg_vgicp_lane.hpp"), ("int fg_entry_of(", "lisreg_batch_rounds.hpp"),
                         ("void k_fgicp_total_batch(", "lisreg_batch_rounds.hpp"),
                         # the fp64 butterfly, the strided total and the lane / wavefront threshold of the voxel statistics
                         ("for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);", "lisreg_fp64_sums.hpp"),
                         ("for (int k = 0; k < W; ++k) acc[k] += part[(size_t)b * W + k];", "lisreg_fp64_sums.hpp"),
                         ("kVoxelBig = 48", "lisreg_fp64_sums.hpp"),
                         # the dense-table limit and the read-back of the voxel count (the multi form reads its counts another way)
                         ("max_cells = 1LL << 26", "lisreg_api_cloud.hip"), ("vox_slot.as<int>() + ", "lisreg_api_cloud.hip")):
        assert [f for f, t in text.items() if needle in t] == [home], needle
    sums = text["lisreg_fp64_sums.hpp"]
    assert re.search(r"double wave_sum\(double v\)\s*\{\s*#pragma unroll\s*for \(int d = 32; d > 0; d >>= 1\) v \+= __shfl_xor\(v, d\);", sums)
    # no other butterfly in the verifiers' units: they call the header's; and none of them builds a dense table of its own
    for unit in ("lisreg_ndt.hip", "lisreg_vgicp.hip", "lisreg_fgicp.hip", "lisreg_vgicp_lane.hpp", "lisreg_fgicp_lane.hpp", "lisreg_batch_rounds.hpp",
                 "lisreg_fgicp_batch.hip", "lisreg_vgicp_batch.hip", "lisreg_batch_driver.hpp"):
        assert "__shfl_xor" not in text[unit] and "<< 26" not in text[unit] and "Big = " not in text[unit], unit
    assert "sum_records<W>(part + (size_t)p0 * W, n_part, acc);" in text["lisreg_batch_rounds.hpp"]
    assert "sum_records<kEvalOut>(part, n_part, acc);" in text["lisreg_vgicp.hip"]
    # VGICP's 28 terms are written once: the weight of a pair (the square root of the voxel's point count) occurs in the lane header only
    assert [f for f, t in text.items() if "sqrt(rec[9])" in t] == ["lisreg_vgicp_lane.hpp"]
    for unit in ("lisreg_vgicp.hip", "lisreg_vgicp_batch.hip"):
        assert '#include "lisreg_vgicp_lane.hpp"' in text[unit] and "vg_linearize_lane<HESS>(" in text[unit], unit
    # the host side of a call exists once: the totals of a round are launched from the driver header only, and both units include it
    for needle in ("k_fgicp_total_batch<kOut>", "k_fgicp_total_batch<1>", "int batch_align("):
        assert [f for f, t in text.items() if needle in t] == ["lisreg_batch_driver.hpp"], needle
    for unit in ("lisreg_fgicp_batch.hip", "lisreg_vgicp_batch.hip"):
        assert '#include "lisreg_batch_rounds.hpp"' in text[unit] and '#include "lisreg_batch_driver.hpp"' in text[unit], unit
        assert text[unit].count("batch_align<") == 1, unit
    # one fitness kernel, defined beside the totals and launched from the driver
    assert [f for f, t in text.items() if re.search(r"void k_\w*fitness_batch\(", t)] == ["lisreg_batch_rounds.hpp"]
    assert len(re.findall(r"void k_\w*fitness_batch\(", text["lisreg_batch_rounds.hpp"])) == 1
    assert [f for f, t in text.items() if re.search(r"k_\w*fitness_batch<<<", t)] == ["lisreg_batch_driver.hpp"]
    # one Levenberg-Marquardt loop: solve_damped is defined once and called from one place, the stepper
    calls = {f: t.count("solve_damped(") for f, t in text.items() if "solve_damped(" in t}
    assert calls == {"lisreg_vgicp_host.hpp": 1, "lisreg_lm_stepper.hpp": 1}, calls
    assert "bool solve_damped(" in text["lisreg_vgicp_host.hpp"]
    # one copy of the aligned-cloud output: its stride-wise loop occurs once, in emit_aligned (lisreg_transform_cloud, which takes a
    # 6-DoF pose and host structs without staging them, keeps the loop of its own), and no aligner transforms a cloud itself
    loops = {f: t.count("if (o != b) memcpy(o + (size_t)i * (size_t)stride") for f, t in text.items()}
    assert {f: k for f, k in loops.items() if k} == {"lisreg_api_ctx.hip": 1, "lisreg_api_cloud.hip": 1}, loops
    assert text["lisreg_api_cloud.hip"].count("int lisreg_transform_cloud(") == 1 and "int emit_aligned(" in text["lisreg_api_ctx.hip"]
    for unit, sites in (("lisreg_vgicp.hip", 1), ("lisreg_fgicp.hip", 1), ("lisreg_ndt.hip", 1), ("lisreg_api_map.hip", 2)):
        assert text[unit].count("emit_aligned(") == sites and "launch_transform_cloud(" not in text[unit], unit
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_vgicp_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    for unit in ("lisreg_vgicp", "lisreg_vgicp_batch", "lisreg_fgicp_batch"):
        assert re.search(r"^FPC_%s := off$" % unit, mk, re.M), unit
    assert "lisreg_vgicp_lane.hpp" in re.search(r"^HDR_lisreg_vgicp := (.*)$", mk, re.M).group(1)
    hdrs = re.search(r"^HDR_lisreg_vgicp_batch := (.*)$", mk, re.M).group(1).split()
    assert {"lisreg_batch_driver.hpp", "lisreg_batch_rounds.hpp", "lisreg_vgicp_lane.hpp", "lisreg_fgicp_lane.hpp", "lisreg_lm_stepper.hpp"} <= set(hdrs)
    hdrs = re.search(r"^HDR_lisreg_fgicp_batch := (.*)$", mk, re.M).group(1).split()
    assert {"lisreg_batch_driver.hpp", "lisreg_batch_rounds.hpp", "lisreg_lm_stepper.hpp"} <= set(hdrs)
    for unit in ("lisreg_vgicp", "lisreg_fgicp"):
        assert "lisreg_lm_stepper.hpp" in re.search(r"^HDR_%s := (.*)$" % unit, mk, re.M).group(1), unit
    # the batch unit keeps to the constraints of its kernels
    body = text["lisreg_vgicp_batch.hip"]
    assert "__shared__" not in body and "atomicAdd" not in body and "atomicCAS" not in body


def test_vgicp_batch_smoke_compiles_and_the_mirror_has_the_verifier():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists (builds it if the tree is fresh)
    subprocess.check_call(["make", "-s", "-C", HOST, "vgicp_batch_smoke"])
    assert os.path.exists(os.path.join(HOST, "vgicp_batch_smoke"))
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    body = hdr[hdr.index("class VgicpVerifier"):hdr.index("// OptimizedICPGN")]
    for name in ("setResolution", "setCorrespondenceRandomness", "setTransformationEpsilon", "setRotationEpsilon", "setMaximumIterations",
                 "setCandidateTarget", "addCandidate", "clearCandidates", "alignAll", "best", "result", "fitness", "hasConverged",
                 "lisreg_vgicp_align_batch"):
        assert name in body, name


@pytest.mark.gpu
def test_vgicp_batch_smoke_runs():
    exe = os.path.join(HOST, "vgicp_batch_smoke")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "vgicp_batch_smoke ok" in r.stdout, r.stdout + r.stderr
