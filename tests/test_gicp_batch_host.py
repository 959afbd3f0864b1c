"""lisreg_gicp_align_batch without a GPU: the structs and the symbol of include/lisreg.h, the stepper check program
(GicpStepper against the outer loop written out, host/gicp_stepper_check.cpp), tests/gicp_batch_ref.py (the `best` rule on score lists
made by hand, the fitness score against a brute-force nearest distance, the round counts of the batch of eight's items), the one home
of the outer loop and of the lane body, the Makefile lines, the smoke program of the host mirror.  The GPU side is
tests/test_gicp_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import gicp_batch_ref as B
import gicp_ref as R
from test_ndt_batch_host import _struct_from_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
PARENT = os.path.join(ROOT, "tests", "golden", "gicp_batch", "gicp_parent_outputs.npz")


def test_structs_and_symbol_match_the_header():
    import lisreg
    for name, mine, size in (("lisreg_gicp_item", lisreg.GicpItemC, 16), ("lisreg_gicp_batch_info", lisreg.GicpBatchInfo, 16)):
        theirs = _struct_from_header(name)
        assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name
    assert [(n, getattr(lisreg.GicpItemC, n).offset) for n, _ in lisreg.GicpItemC._fields_] == [("source", 0), ("slot", 4), ("guess", 8)]
    assert [n for n, _ in lisreg.GicpBatchInfo._fields_] == ["best", "n_rounds", "n_sources_staged", "reserved"]
    assert C.sizeof(lisreg.GicpResult) == 176
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    assert hasattr(L, "lisreg_gicp_align_batch") and "lisreg_gicp_align_batch" in lisreg.ABI_SYMBOLS
    assert re.search(r"^\s*int\s+lisreg_gicp_align_batch\s*\(", hdr, re.M)
    # the §7r block sits between §7q and the FEPSC section and says what the call is
    assert hdr.index("§7q: PCL's GICP registration") < hdr.index("§7r: PCL's GICP verification") < hdr.index("loop-closure candidate detection: FEPSC")
    block = hdr[hdr.index("§7r: PCL's GICP verification"):hdr.index("loop-closure candidate detection: FEPSC")]
    for text in ("subMapOptmizationNode.cpp:2779-2846", ":2834-2840", "registration.cpp:137-146", "The DEFINITION is tests/gicp_batch_ref.py",
                 "getFitnessScore", "176 bytes", "INT_MAX / 74", "592", "64 per finite source point", "fewer than 4 pairs", "n_items < 0",
                 "largest n_rounds", "fewer finite points than"):
        assert text in re.sub(r"\s*\n \* ", " ", block), text
    assert "no batch form yet" not in hdr
    assert "lisreg_gicp_align_batch" in hdr[hdr.index("Per-kernel timing"):hdr.index("int  lisreg_set_profiling")]
    # no context: refused before anything is read
    assert L.lisreg_gicp_align_batch(None, None, None, 0, 0, 0, None, 0, None, None, None, None) == lisreg.ERR_ARG
    it = lisreg.GicpItem(2, 5, np.eye(4))
    assert (it.source, it.slot) == (2, 5) and it.guess.dtype == np.float32 and it.guess.shape == (16,) and lisreg.GicpItem(0, 0).guess is None


def test_gicp_stepper_check_compiles_without_warnings_and_passes(tmp_path):
    """the resumable loop asks what the written-out loop asks and ends where it ends, bit for bit, on every script; every way out
    occurred"""
    exe = str(tmp_path / "gicp_stepper_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-I" + CSRC, "-o", exe,
                           os.path.join(HOST, "gicp_stepper_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "gicp_stepper_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    census = re.search(r"^census over (\d+) scripts \((\d+) rounds, at most (\d+) in one\):(.*)$", r.stdout, re.M)
    assert census and int(census.group(1)) >= 60 and int(census.group(2)) > int(census.group(1))
    hits = {k: int(v) for k, v in re.findall(r" (\w+)=(\d+)", census.group(4))}
    for name in ("delta", "cap1", "cap3", "few_first", "few_later"):
        assert hits[name] >= 1, (name, hits)
    few = subprocess.run([exe, "60"], capture_output=True, text=True, timeout=60)
    assert few.returncode == 0 and "census over 60 scripts" in few.stdout and "gicp_stepper_check ok" in few.stdout
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^gicp_stepper_check: gicp_stepper_check.cpp ../csrc/lisreg_gicp_stepper.hpp ../csrc/lisreg_gicp_host.hpp$", mk, re.M)
    rule = mk[mk.index("gicp_stepper_check: gicp_stepper_check.cpp"):].split("\n")[1]
    assert "-Wall -Wextra -Werror" in rule and "-llisreg" not in rule
    assert "gicp_stepper_check" in re.search(r"^all:(.*)$", mk, re.M).group(1) and "gicp_batch_smoke" in re.search(r"^all:(.*)$", mk, re.M).group(1)


def test_best_rule_on_score_lists_made_by_hand():
    assert B.best([1, 1, 1], [0.3, 0.1, 0.2]) == 1
    assert B.best([1, 1, 1], [0.2, 0.1, 0.1]) == 2                      # a tie: `score > bestScore` does not skip it, the later one wins
    assert B.best([1, 1], [0.1, 0.1]) == 1
    assert B.best([0, 0, 0], [0.1, 0.2, 0.3]) == -1                     # none converged
    assert B.best([1, 0, 1], [0.3, 0.01, 0.2]) == 2                     # the lowest score belongs to an item that did not converge
    assert B.best([0, 1, 0], [0.01, 5.0, 0.02]) == 1
    assert B.best([0, 1, 1], [1.0e4, 0.2, 0.2]) == 2                    # the far item of the GPU test: not converged, then a tie
    assert B.best([], []) == -1
    assert B.best([1], [B.DBL_MAX]) == 0 and B.best([1], [np.inf]) == -1  # bestScore starts at DBL_MAX
    import fgicp_batch_ref as FB
    assert B.best is FB.best and B.fitness is FB.fitness and B.DBL_MAX == FB.DBL_MAX
    doc = re.sub(r"\s+", " ", B.__doc__)
    for text in ("getFitnessScore", "max_range = DBL_MAX", "final_transform", "fewer than 4 pairs", "converged = 0", "skipped by `best`",
                 "still gets a score", "registration.cpp:137-146"):
        assert text in doc, text


def test_fitness_ignores_nan_records_and_equals_brute_force():
    """65 source points against 64 target points: the mean over the finite source points of the smallest squared distance"""
    rng = np.random.default_rng(5)
    tgt = rng.uniform(-5, 5, (64, 3)).astype(np.float32)
    src = rng.uniform(-5, 5, (65, 3)).astype(np.float32)
    T = R.pose_of([0.3, -0.2, 0.1, 0.02, -0.03, 0.05], np.eye(4))

    def brute(t32, s32, M=T):
        t, s = t32[~np.isnan(t32).any(1)].astype(np.float64), s32[~np.isnan(s32).any(1)].astype(np.float64)
        x = s @ M[:3, :3].T + M[:3, 3]
        return float(np.mean(((x[:, None, :] - t[None, :, :]) ** 2).sum(2).min(1)))
    got, want = B.fitness(tgt, src, T), brute(tgt, src)
    print(f"[gicp_batch_ref] fitness {got:.12e} against brute force {want:.12e}")
    assert abs(got - want) <= 1e-12 * want
    holes = src.copy()
    holes[[0, 7, 64]] = np.nan
    holes[9, 1] = np.nan
    assert abs(B.fitness(tgt, holes, T) - brute(tgt, holes)) <= 1e-12 * brute(tgt, holes)
    assert abs(B.fitness(tgt, holes, T) - B.fitness(tgt, np.delete(src, [0, 7, 9, 64], 0), T)) <= 1e-12 * want
    far = T.copy()
    far[0, 3] += 100.0
    assert B.fitness(tgt, src, far) > 90.0 ** 2                         # no cut-off


def test_the_batch_is_the_loop_of_single_alignments_and_its_items_end_in_different_rounds():
    """the cuts and the far guess of the batch of eight through the restatement (the full source's count is read from the file the
    parent commit's build wrote: its CPU run takes 6 s): the rounds the issue lists, at least 3 distinct"""
    import lisreg
    W = R.world(*B.SCENE)
    prm = R.params()
    xyz = B.scene_sources(W["src"])
    far = np.array(W["guess"], np.float32).copy()
    far[0, 3] += 100.0
    picks = (B.C63, B.C65, B.C129, B.C20)
    sources = {s: (xyz[s], R.prepare_source(xyz[s], prm)) for s in picks}
    sources[B.FULL] = (xyz[B.FULL], W["S"])
    items = [(s, 0, W["guess"]) for s in picks] + [(B.FULL, 0, far)]
    res, fit, best = B.align_batch({0: (W["tgt"], W["T"])}, sources, items, prm)
    rounds = [r["n_rounds"] for r in res]
    g = np.load(PARENT)
    full = lisreg.GicpResult.from_buffer_copy(bytes(g["eight_default"][0]))
    print(f"[gicp_batch_ref] rounds of the cuts 63 / 65 / 129 / 20 and of the far guess {rounds}, of the full source (parent's GPU run) {full.n_rounds}; "
          f"fitness {fit.tolist()}, best {best}")
    assert rounds == [8, 7, 9, 4, 1] and full.n_rounds == 4 == int(np.load(os.path.join(ROOT, "tests", "golden", "gicp", "gicp_cases.npz"))["align_counts"][0][4])
    assert len(set(rounds + [full.n_rounds])) >= 3
    assert [r["converged"] for r in res] == [1, 1, 1, 1, 0]
    r = res[4]
    assert (r["iters"], r["n_pairs_last"], r["inner_exit"]) == (0, 0, -1) and fit[4] > 90.0 ** 2 and best == B.best([x["converged"] for x in res], fit) != 4
    for (s, slot, guess), r, f in zip(items[:1] + items[4:], res[:1] + res[4:], [fit[0], fit[4]]):
        alone = R.align(W["T"], sources[s][1], prm, guess)
        assert np.array_equal(alone["T"], r["T"]) and (alone["n_rounds"], alone["iters"], alone["converged"]) == (r["n_rounds"], r["iters"], r["converged"])
        assert f == B.fitness(W["tgt"], sources[s][0], r["T"])
    assert B.align_batch({0: (W["tgt"], W["T"])}, sources, items[4:], prm, want_fitness=False)[1:] == (None, -1)
    # the GPU's single calls of the parent commit took the same rounds (items 2 .. 5 and 7 of the batch of eight)
    gpu = [lisreg.GicpResult.from_buffer_copy(bytes(row)).n_rounds for row in g["eight_default"]]
    assert [gpu[k] for k in (2, 3, 4, 5, 7)] == rounds


def test_the_outer_loop_and_the_lane_body_have_one_home():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    step, unit, batch, driver = (text[f] for f in ("lisreg_gicp_stepper.hpp", "lisreg_gicp.hip", "lisreg_gicp_batch.hip", "lisreg_batch_driver.hpp"))
    # the stepper keeps the host header's rules and writes no second minimiser
    assert "hip" not in re.sub(r"//.*", "", step).lower() and "__device__" not in step and "static " not in re.sub(r"static constexpr", "", step)
    assert '#include "lisreg_gicp_host.hpp"' in step and "struct GicpStepper {" in step and "int gicp_closed_loop(" in step
    assert len(re.findall(r"\binner\(", step)) == 1 and "line_search" not in step and "bfgs_minimise" not in step
    for needle, home in (("int line_search(", "lisreg_gicp_host.hpp"), ("double bfgs_minimise(", "lisreg_gicp_host.hpp"),
                         ("struct GicpStepper {", "lisreg_gicp_stepper.hpp"), ("void gicp_moments_lane(", "lisreg_gicp_lane.hpp"),
                         ("void k_gicp_moments(", "lisreg_gicp.hip"), ("void k_gicp_moments_batch(", "lisreg_gicp_batch.hip"),
                         ("int lisreg::gc_check_params(", "lisreg_gicp.hip"), ("GicpCentre gicp_centre_of(", "lisreg_gicp_lane.hpp"),
                         ("int stage_distributions(", "lisreg_batch_driver.hpp")):
        assert [f for f, t in text.items() if needle in t] == [home], needle
    # the outer loop's end rule is called from the stepper only; the single aligner is the closed loop over it
    calls = {f: len(re.findall(r"(?<!double )\bouter_delta\(", t)) for f, t in text.items()}
    assert {f: k for f, k in calls.items() if k} == {"lisreg_gicp_stepper.hpp": 1}, calls
    assert "gicp_closed_loop(" in unit and "for (;;)" not in unit and "inner(rec" not in unit
    # the lane body is called once in each of the two units; the bounding-box centre and the parameter checks are shared
    for body in (unit, batch):
        assert '#include "lisreg_gicp_lane.hpp"' in body and '#include "lisreg_gicp_stepper.hpp"' in body
        assert len(re.findall(r"(?<!void )\bgicp_moments_lane\(", body)) == 1 and body.count("gicp_centre_of(") >= 1 and "gc_check_params(" in body
    assert sorted(f for f, t in text.items() if re.search(r"(?<!void )\bgicp_moments_lane\(", t) and f.endswith(".hip")) == ["lisreg_gicp.hip", "lisreg_gicp_batch.hip"]
    assert unit.count("<<<") == 2 and batch.count("<<<") == 1
    # the batch unit goes through the shared driver and keeps to the constraints of its kernel
    assert batch.count("batch_align<") == 1 and '#include "lisreg_batch_driver.hpp"' in batch and '#include "lisreg_batch_rounds.hpp"' in batch
    for word in ("__shared__", "atomic", "asm", "__shfl", "mfma"):
        assert word not in batch.lower(), word
    assert "fg_entry_of(" in batch and "kFitnessTotalsApart = true" in batch and "kRec = kGicpRec" in batch
    # the driver takes the record width from the family
    assert "constexpr int kOut = F::kRec;" in driver and "INT_MAX / kOut" in driver and "29" not in re.sub(r"//.*", "", driver)
    assert "kRec = vgicp_host::kOut" in driver and "kRec = kNdtOut" in text["lisreg_ndt_batch.hip"]
    assert "lisreg::BatchBufs fgb, vgb, ndb, gcb;" in text["lisreg_ctx.hpp"]


def test_the_makefile_knows_the_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_gicp_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert re.search(r"^FPC_lisreg_gicp_batch := off$", mk, re.M)
    hdrs = re.search(r"^HDR_lisreg_gicp_batch := (.*)$", mk, re.M).group(1).split()
    assert {"lisreg_fp64_sums.hpp", "lisreg_batch_driver.hpp", "lisreg_batch_rounds.hpp", "lisreg_gicp_lane.hpp", "lisreg_gicp_stepper.hpp",
            "lisreg_gicp_host.hpp", "lisreg_fgicp_lane.hpp", "lisreg_lm_stepper.hpp", "lisreg_vgicp_host.hpp"} <= set(hdrs)
    assert "lisreg_gicp_stepper.hpp" in re.search(r"^HDR_lisreg_gicp := (.*)$", mk, re.M).group(1).split()
    for h in hdrs:
        assert os.path.exists(os.path.join(CSRC, h)), h
    ignore = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "lis-slam_amd/host/gicp_stepper_check" in ignore and "lis-slam_amd/host/gicp_batch_smoke" in ignore


def test_gicp_batch_smoke_compiles_and_the_mirror_has_the_verifier():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists (builds it if the tree is fresh)
    subprocess.check_call(["make", "-s", "-C", HOST, "gicp_batch_smoke"])
    exe = os.path.join(HOST, "gicp_batch_smoke")
    assert os.path.exists(exe)
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    assert hdr.index("class NdtVerifier") < hdr.index("class GicpVerifier") < hdr.index("// OptimizedICPGN")
    body = hdr[hdr.index("class GicpVerifier"):hdr.index("// OptimizedICPGN")]
    for name in ("setMaxCorrespondenceDistance", "setCorrespondenceRandomness", "setTransformationEpsilon", "setRotationEpsilon", "setMaximumIterations",
                 "setMaximumOptimizerIterations", "setCandidateTarget", "addCandidate", "clearCandidates", "alignAll", "best", "result", "fitness",
                 "hasConverged", "lisreg_gicp_align_batch", "lisreg_fgicp_set_target", "tp.plane_epsilon = prm_.gicp_epsilon"):
        assert name in body, name
    if lisreg.lib().lisreg_device_count() == 0:    # without a device the program fails loudly and says so
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "failed loudly as designed" in r.stdout, r.stdout + r.stderr
