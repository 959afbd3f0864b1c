"""lisreg_ndt_align_batch without a GPU: the structs and the symbol of include/lisreg.h, the stepper check program
(NdtStepper against the closed form of its loop, host/ndt_stepper_check.cpp), tests/ndt_batch_ref.py (the `best` rule on score lists
made by hand, the fitness score against a brute-force nearest distance), the one home of the Newton loop and of the lane body, the
smoke program of the host mirror.  The GPU side is tests/test_ndt_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ndt_batch_ref as B
import ndt_ref as R

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
    for name, mine, size in (("lisreg_ndt_item", lisreg.NdtItemC, 16), ("lisreg_ndt_batch_info", lisreg.NdtBatchInfo, 16)):
        theirs = _struct_from_header(name)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name
    assert [(n, getattr(lisreg.NdtItemC, n).offset) for n, _ in lisreg.NdtItemC._fields_] == [("source", 0), ("slot", 4), ("guess", 8)]
    assert [n for n, _ in lisreg.NdtBatchInfo._fields_] == ["best", "n_rounds", "n_sources_staged", "reserved"]
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    assert hasattr(L, "lisreg_ndt_align_batch") and "lisreg_ndt_align_batch" in lisreg.ABI_SYMBOLS
    assert re.search(r"^\s*int\s+lisreg_ndt_align_batch\s*\(", hdr, re.M)
    block = hdr[hdr.index("§7o: NDT verification"):hdr.index("§7k: voxelised GICP")]
    for text in ("subMapOptmizationNode.cpp:2779-2846", ":2834-2840", "registration.cpp:147-155", "tests/ndt_batch_ref.py", "getFitnessScore",
                 "NOT the float", "NaN records included", "INT_MAX / 29"):
        assert text in block, text
    # the section follows §7j's NDT block, whose set_target comment names the memory the slot now keeps, and the timing comment names the batch
    assert hdr.index("§7j: Normal Distributions Transform") < hdr.index("§7o: NDT verification") < hdr.index("§7k: voxelised GICP")
    assert "16 bytes per finite point and 4 per grid cell" in hdr[hdr.index("/* setInputTarget + setResolution"):hdr.index("int  lisreg_ndt_set_target")]
    assert "lisreg_ndt_align_batch" in hdr[hdr.index("Per-kernel timing"):hdr.index("int  lisreg_set_profiling")]
    # no context: refused before anything is read
    assert L.lisreg_ndt_align_batch(None, None, None, 0, 0, 0, None, 0, None, None, None, None) == lisreg.ERR_ARG
    it = lisreg.NdtItem(2, 5, np.eye(4))
    assert (it.source, it.slot) == (2, 5) and it.guess.dtype == np.float32 and it.guess.shape == (16,) and lisreg.NdtItem(0, 0).guess is None


def test_ndt_stepper_check_compiles_without_warnings_and_passes(tmp_path):
    """the resumable loop asks what the closed loop asks and ends where it ends, bit for bit, on every script; every case of the
    trial value, every interval update and every way out occurred (but the one the program's header explains)"""
    exe = str(tmp_path / "ndt_stepper_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe, os.path.join(HOST, "ndt_stepper_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ndt_stepper_check ok" in r.stdout, r.stdout + r.stderr
    hits = {k: int(v) for k, v in re.findall(r" (\w+)=(\d+)", r.stdout)}
    assert len(hits) == 21 and int(re.search(r"scripts (\d+)", r.stdout).group(1)) >= 300
    for name, count in hits.items():
        assert count > 0 or name == "interval_converged", (name, hits)
    few = subprocess.run([exe, "40"], capture_output=True, text=True, timeout=60)
    assert few.returncode == 0 and "scripts 40 " in few.stdout and "ndt_stepper_check ok" in few.stdout
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^ndt_stepper_check: ndt_stepper_check.cpp ../csrc/lisreg_ndt_stepper.hpp ../csrc/lisreg_ndt_host.hpp$", mk, re.M)
    assert "ndt_stepper_check" in re.search(r"^all:(.*)$", mk, re.M).group(1)


def test_best_rule_on_score_lists_made_by_hand():
    assert B.best([1, 1, 1], [0.3, 0.1, 0.2]) == 1
    assert B.best([1, 1, 1], [0.2, 0.1, 0.1]) == 2                      # a tie: `score > bestScore` does not skip it, the later one wins
    assert B.best([1, 1], [0.1, 0.1]) == 1
    assert B.best([0, 0, 0], [0.1, 0.2, 0.3]) == -1                     # none converged
    assert B.best([1, 0, 1], [0.3, 0.01, 0.2]) == 2                     # the lowest score belongs to an item that did not converge
    assert B.best([0, 1, 0], [0.01, 5.0, 0.02]) == 1
    assert B.best([], []) == -1
    assert B.best([1], [B.DBL_MAX]) == 0 and B.best([1], [np.inf]) == -1  # bestScore starts at DBL_MAX
    import fgicp_batch_ref as FB
    assert B.best is FB.best and B.DBL_MAX == FB.DBL_MAX
    assert "getFitnessScore" in B.__doc__ and "max_range = DBL_MAX" in B.__doc__ and "not the float final_transform" in B.__doc__


def test_fitness_ignores_nan_records_and_equals_brute_force():
    """65 source points against 64 target points: the mean over the finite source points of the smallest squared distance"""
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-5, 5, (64, 3)).astype(np.float32)
    src = rng.uniform(-5, 5, (65, 3)).astype(np.float32)
    p = np.array([0.3, -0.2, 0.1, 0.02, -0.03, 0.05])
    Rm = R.pose_matrices(p)[0]

    def brute(t32, s32):
        t, s = t32[~np.isnan(t32).any(1)].astype(np.float64), s32[~np.isnan(s32).any(1)].astype(np.float64)
        x = s @ Rm.T + p[:3]
        return float(np.mean(((x[:, None, :] - t[None, :, :]) ** 2).sum(2).min(1)))
    got, want = B.fitness(tgt, src, p), brute(tgt, src)
    print(f"[ndt_batch_ref] fitness {got:.12e} against brute force {want:.12e}")
    assert abs(got - want) <= 1e-12 * want
    holes = src.copy()
    holes[[0, 7, 64]] = np.nan
    holes[9, 1] = np.nan
    assert abs(B.fitness(tgt, holes, p) - brute(tgt, holes)) <= 1e-12 * brute(tgt, holes)
    assert abs(B.fitness(tgt, holes, p) - B.fitness(tgt, np.delete(src, [0, 7, 9, 64], 0), p)) <= 1e-12 * want
    far = p + np.array([100.0, 0, 0, 0, 0, 0])
    assert B.fitness(tgt, src, far) > 90.0 ** 2                         # no cut-off
    # the pose is the evaluations', not the float matrix: p's rotation in double
    assert np.array_equal(R.matrix_from_p(p)[:3, :3], Rm)


def test_the_batch_is_the_loop_of_single_alignments():
    """a small planted target, two sources, three items (one far away: converged at once, with a score)"""
    prm = R.params(max_iters=2)
    xyz = R.planted_cloud()
    tg = {4: (xyz, R.build_target(xyz, prm))}
    fin = xyz[~np.isnan(xyz).any(1)]
    sr = [fin[::40][:63].copy(), fin[::30][:65].copy()]
    g = R.matrix_from_p(np.array([0.05, -0.04, 0.03, 0.01, -0.02, 0.015])).astype(np.float32)
    far = g.copy()
    far[0, 3] += 100.0
    items = [(0, 4, g), (1, 4, far), (1, 4, None)]
    res, fit, best = B.align_batch(tg, sr, items, prm)
    for (s, slot, guess), r, f in zip(items, res, fit):
        alone = R.align(tg[slot][1], sr[s], prm, guess)
        assert np.array_equal(alone["p"], r["p"]) and (alone["n_evals"], alone["iters"], alone["converged"]) == (r["n_evals"], r["iters"], r["converged"])
        assert f == B.fitness(tg[slot][0], sr[s], r["p"])
    assert (res[1]["converged"], res[1]["iters"], res[1]["n_evals"]) == (1, 0, 1) and fit[1] > 90.0 ** 2
    assert best == B.best([r["converged"] for r in res], fit)
    assert B.align_batch(tg, sr, items, prm, want_fitness=False)[1:] == (None, -1)


def test_the_newton_loop_and_the_lane_body_have_one_home():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    # the line search is defined once and called from one place, both in the stepper; the stateless pieces stay in the host header
    sites = {f: len(re.findall(r"\bline_search_mt\(", t)) for f, t in text.items() if re.search(r"\bline_search_mt\(", t)}
    assert sites == {"lisreg_ndt_stepper.hpp": 2}, sites
    assert "bool line_search_mt()" in text["lisreg_ndt_stepper.hpp"] and text["lisreg_ndt_stepper.hpp"].count("return line_search_mt();") == 1
    for needle, home in (("solve_step(Hm, g, delta)", "lisreg_ndt_stepper.hpp"), ("struct NdtStepper {", "lisreg_ndt_stepper.hpp"),
                         ("bool trial_value(", "lisreg_ndt_host.hpp"), ("bool update_interval(", "lisreg_ndt_host.hpp"),
                         ("void ndt_eval_lane(", "lisreg_ndt_lane.hpp"), ("struct NdtGauss {", "lisreg_ndt_lane.hpp"),
                         ("int lisreg::vg_search_grid(", "lisreg_vgicp.hip"), ("cell *= 1.26;", "lisreg_vgicp.hip")):
        assert [f for f, t in text.items() if needle in t] == [home], needle
    assert "ndt_optimise(" in text["lisreg_ndt.hip"] and "while (!converged)" not in text["lisreg_ndt.hip"]
    # every unit that holds an NDT evaluation kernel includes the lane header and calls its body; the Makefile knows
    units = sorted(f for f, t in text.items() if re.search(r"void k_ndt_eval\w*\(", t))
    assert units == ["lisreg_ndt.hip", "lisreg_ndt_batch.hip"], units
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_ndt_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    for unit in units:
        assert '#include "lisreg_ndt_lane.hpp"' in text[unit] and text[unit].count("ndt_eval_lane<HESS>(") == 1, unit
        name = unit[:-4]
        assert re.search(r"^FPC_%s := off$" % name, mk, re.M), unit
        hdrs = re.search(r"^HDR_%s := (.*)$" % name, mk, re.M).group(1).split()
        assert {"lisreg_ndt_lane.hpp", "lisreg_ndt_stepper.hpp", "lisreg_ndt_host.hpp", "lisreg_fp64_sums.hpp"} <= set(hdrs), unit
    hdrs = re.search(r"^HDR_lisreg_ndt_batch := (.*)$", mk, re.M).group(1).split()
    assert {"lisreg_batch_driver.hpp", "lisreg_batch_rounds.hpp", "lisreg_fgicp_lane.hpp", "lisreg_lm_stepper.hpp"} <= set(hdrs)
    # NDT goes through the shared driver, and its batch unit keeps to the constraints of its kernels
    body = text["lisreg_ndt_batch.hip"]
    assert body.count("batch_align<") == 1 and '#include "lisreg_batch_driver.hpp"' in body and '#include "lisreg_batch_rounds.hpp"' in body
    assert "__shared__" not in body and "atomicAdd" not in body and "atomicCAS" not in body and "__shfl_xor" not in body
    # both the distributions and the NDT target build their grid with the one helper
    assert text["lisreg_vgicp.hip"].count("vg_search_grid(c, ") == 1 and text["lisreg_ndt.hip"].count("vg_search_grid(c, ") == 1


def test_ndt_batch_smoke_compiles_and_the_mirror_has_the_verifier():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists (builds it if the tree is fresh)
    subprocess.check_call(["make", "-s", "-C", HOST, "ndt_batch_smoke"])
    assert os.path.exists(os.path.join(HOST, "ndt_batch_smoke"))
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    body = hdr[hdr.index("class NdtVerifier"):hdr.index("// OptimizedICPGN")]
    for name in ("setResolution", "setStepSize", "setTransformationEpsilon", "setMaximumIterations", "setLineSearch", "setCandidateTarget",
                 "addCandidate", "clearCandidates", "alignAll", "best", "result", "fitness", "hasConverged", "lisreg_ndt_align_batch"):
        assert name in body, name
    assert hdr.index("class VgicpVerifier") < hdr.index("class NdtVerifier")


@pytest.mark.gpu
def test_ndt_batch_smoke_runs():
    exe = os.path.join(HOST, "ndt_batch_smoke")
    assert os.path.exists(exe)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "ndt_batch_smoke ok" in r.stdout, r.stdout + r.stderr
