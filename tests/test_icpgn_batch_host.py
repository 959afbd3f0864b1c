"""lisreg_icp_gn_match_batch without a GPU: the structs and the symbol of include/lisreg.h, tests/icpgn_batch_ref.py
(the `best` rule on score lists made by hand, the batch as the loop of single matches), the one home of the per-lane body and of the
solve step, the Makefile lines, the smoke program of the host mirror.  The GPU side is tests/test_icpgn_batch.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import icpgn_batch_ref as B
from test_ndt_batch_host import _struct_from_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
f32 = np.float32
FLT_MAX = float(np.finfo(np.float32).max)


def test_structs_and_symbol_match_the_header():
    import lisreg
    for name, mine, size in (("lisreg_icpgn_item", lisreg.IcpGnItemC, 16), ("lisreg_icpgn_batch_info", lisreg.IcpGnBatchInfo, 16),
                             ("lisreg_icpgn_result", lisreg.IcpGnResult, 80)):
        theirs = _struct_from_header(name) if size == 16 else None
        if theirs is not None:
            assert [(n, getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
                   [(n, getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
            assert C.sizeof(theirs) == size, name
        assert C.sizeof(mine) == size, name
    assert [(n, getattr(lisreg.IcpGnItemC, n).offset) for n, _ in lisreg.IcpGnItemC._fields_] == [("source", 0), ("slot", 4), ("predict_pose", 8)]
    assert [n for n, _ in lisreg.IcpGnBatchInfo._fields_] == ["best", "n_sources_staged", "n_syncs", "reserved"]
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    assert hasattr(L, "lisreg_icp_gn_match_batch") and "lisreg_icp_gn_match_batch" in lisreg.ABI_SYMBOLS
    assert re.search(r"^\s*int\s+lisreg_icp_gn_match_batch\s*\(", hdr, re.M)
    # the declaration sits next to the single call's and its comment states the contract
    assert hdr.index("int  lisreg_icp_gn_match(") < hdr.index("int  lisreg_icp_gn_match_batch(") < hdr.index("§7j: Normal Distributions Transform")
    block = re.sub(r"\s*\n \*\s+", " ", hdr[hdr.index("int  lisreg_icp_gn_match("):hdr.index("int  lisreg_icp_gn_match_batch(")])
    for text in ("subMapOptmizationNode.cpp:2496-2621", ":2551-2558", "Batch equals single", "in all bytes of lisreg_icpgn_result", ":49-50",
                 "staged once", "neither checked nor staged", "DBL_MAX", "a NaN score is taken", "equal scores go to the later item",
                 "n_items < 0", "max_iterations > 100000", "32-bit counts", "best = -1", "no per-item transformed_out",
                 "n_syncs = max_iterations / 64 + 1", "lisreg_set_stream", "grow-only", "4 bytes"):
        assert text in block, text
    # no context: refused before anything is read
    assert L.lisreg_icp_gn_match_batch(None, None, None, 0, 0, 0, None, 0, 0, 0.0, None, None) == lisreg.ERR_ARG
    bad = C.cast(C.c_void_p(8), C.POINTER(lisreg.IcpGnItemC))
    assert L.lisreg_icp_gn_match_batch(None, None, None, 3, 32, 1, bad, 5, 30, 10.0, None, None) == lisreg.ERR_ARG
    it = lisreg.IcpGnItem(2, 5, np.eye(4))
    assert (it.source, it.slot) == (2, 5) and lisreg.IcpGnItem(0, 0).predict_pose is None


def test_best_rule_on_score_lists_made_by_hand():
    assert B.best_of([0.3, 0.1, 0.2]) == 1
    assert B.best_of([0.2, 0.1, 0.1]) == 2                     # a tie: `score > bestScore` does not skip it, the later item wins
    assert B.best_of([0.1, 0.1]) == 1
    assert B.best_of([FLT_MAX, 3.0e38]) == 1 and B.best_of([FLT_MAX]) == 0      # FLT_MAX as the first score is taken: it is below DBL_MAX
    assert B.best_of([np.inf]) == -1 and B.best_of([np.inf, 0.5, np.inf]) == 1   # inf > DBL_MAX: skipped
    assert B.best_of([np.nan]) == 0                            # NaN > x is false: taken
    assert B.best_of([0.5, np.nan]) == 1                       # ... and it becomes bestScore, against which nothing is greater
    assert B.best_of([np.nan, 0.5]) == 1
    assert B.best_of([]) == -1
    assert B.DBL_MAX == np.finfo(np.float64).max
    doc = re.sub(r"\s+", " ", B.__doc__)
    for text in ("subMapOptmizationNode.cpp:2496-2621", "registration.cpp:19-115", ":2551-2558", "myICP(30, 10)", "LATER candidate",
                 "NaN score is taken", "oracle.icp_gn_match"):
        assert text in doc, text


def test_the_refs_batch_is_the_loop_of_oracle_matches_on_three_small_items(oracle):
    from test_icp import _case
    tgt, src, _ = _case(63, n_map=5000, hw=(8, 240))
    tgt2, _, _ = _case(63, n_map=3000, hw=(8, 240))
    far = src.copy(); far["x"] += f32(1000.0)
    cut = np.ascontiguousarray(src[:65])
    T0 = np.eye(4, dtype=f32); T0[0, 3] = 0.05
    items = [(0, 7, T0), (1, 8, None), (2, 7, T0)]
    res, best = B.match_batch(oracle, {7: tgt, 8: tgt2}, [src, cut, far], items, 5, 4.0)
    alone = [oracle.icp_gn_match(tgt, src, 5, 4.0, T0), oracle.icp_gn_match(tgt2, cut, 5, 4.0, np.eye(4, dtype=f32)),
             oracle.icp_gn_match(tgt, far, 5, 4.0, T0)]
    for a, b in zip(res, alone):
        assert a["T"].tobytes() == b["T"].tobytes() and (a["steps_applied"], a["n_corr_last"]) == (b["steps_applied"], b["n_corr_last"])
        assert f32(a["fitness"]).tobytes() == f32(b["fitness"]).tobytes()
    assert res[0]["steps_applied"] == 5 and res[2]["steps_applied"] == 0 and res[2]["n_corr_last"] == 0
    assert best == B.best_of([r["fitness"] for r in alone]) and best in (0, 1)
    # listing an item twice makes a tie: the later copy wins
    res2, best2 = B.match_batch(oracle, {7: tgt, 8: tgt2}, [src, cut, far], [items[best], items[2], items[best]], 5, 4.0)
    assert best2 == 2 and res2[0]["fitness"] == res2[2]["fitness"]
    assert B.match_batch(oracle, {}, [], [], 5, 4.0) == ([], -1)


def _calls(text, name):
    """call sites of a function: its name followed by `(` or `<Q>(`, the definition itself left out"""
    return len(re.findall(r"\b%s(?:<\w+>)?\(" % name, text)) - len(re.findall(r"(?:void|int) %s\(" % name, text))


def test_the_lane_body_and_the_solve_step_have_one_home_and_both_kernels_call_them():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    nn1 = text["lisreg_nn1.hip"]
    for needle in ("int icpgn_lane(", "void icpgn_row(", "void icpgn_solve_step(", "void icp_fitness_row(", "void icp_fit_total(",
                   "void k_icpgn_assoc(", "void k_icpgn_assoc_b(", "void k_icpgn_solve(", "void k_icpgn_solve_b(", "void k_icpgn_fit_b(",
                   "void k_icpgn_fit_reduce_b("):
        assert [f for f, t in text.items() if needle in t] == ["lisreg_nn1.hip"] and nn1.count(needle) == 1, needle

    def kernel(name):
        start = re.search(r"(?:void|int) %s\(" % name, nn1).start()
        return nn1[start:nn1.index("\n}\n", start)]
    for single, batch, fn in (("k_icpgn_assoc", "k_icpgn_assoc_b", "icpgn_lane"), ("k_icpgn_assoc", "k_icpgn_assoc_b", "icpgn_row"),
                              ("k_icpgn_solve", "k_icpgn_solve_b", "icpgn_solve_step"), ("k_icp_fitness", "k_icpgn_fit_b", "icp_fitness_row"),
                              ("k_icp_fit_reduce", "k_icpgn_fit_reduce_b", "icp_fit_total")):
        assert _calls(kernel(single), fn) == 1 and _calls(kernel(batch), fn) == 1, (single, batch, fn)
        assert _calls(nn1, fn) == 2, fn
    # the arithmetic itself is written once: the Jacobian block, the pivoted LU and the SO3 update
    assert nn1.count("A[r][0] = -(R1 * p.z - R2 * p.y);") == 1 and nn1.count("// PartialPivLU") == 1 and nn1.count("if (theta < 1e-5f)") == 1
    # the batch kernels find their item through the block table, wave-uniform, and sum with the single call's tree
    for k in ("k_icpgn_assoc_b", "k_icpgn_fit_b"):
        body = kernel(k)
        assert "icp_locate(items, n_items, &blk)" in body and body.count("__builtin_amdgcn_readfirstlane") == 2, k
        assert "wave_sum_up" not in body and "icp_row256" not in body, k
    for k in ("k_icpgn_assoc_b", "k_icpgn_solve_b", "k_icpgn_fit_b", "k_icpgn_fit_reduce_b", "icpgn_lane", "icpgn_row", "icpgn_solve_step"):
        for word in ("atomic", "asm"):
            assert word not in kernel(k).lower(), (k, word)
    assert not re.search(r"void k_\w*fitness_batch\(", nn1)
    # the entry point is a unit of its own, with buffers of its own; the launchers are declared in the internal header
    unit = text["lisreg_api_icpgn.hip"]
    assert [f for f, t in text.items() if "int lisreg_icp_gn_match_batch(" in t] == ["lisreg_api_icpgn.hip"]
    assert "<<<" not in unit and "launch_icpgn_batch_iteration(" in unit and "launch_icpgn_batch_fitness(" in unit
    for buf in ("icp_state", "icp_partials", "icp_cur", "icp_items", "mp_pts"):
        assert buf not in unit, buf
    for decl in ("void launch_icpgn_batch_iteration(", "void launch_icpgn_batch_fitness(", "struct IcpGnItem {"):
        assert decl in text["lisreg_internal.hpp"], decl
    assert "gnb_tab, gnb_part, gnb_nn" in text["lisreg_ctx.hpp"]
    # one host synchronisation outside the bounding one and the read-back: none
    assert unit.count("hipStreamSynchronize(") == 2 and unit.count("++n_syncs") == 2


def test_the_makefile_knows_the_unit():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1).split()
    assert "lisreg_api_icpgn.hip" in srcs and "lisreg_nn1.hip" in srcs
    assert re.search(r"^FPC_lisreg_nn1 := off$", mk, re.M)                     # the kernels' unit stays uncontracted
    hm = open(os.path.join(HOST, "Makefile")).read()
    assert "icpgn_batch_smoke" in re.search(r"^all:(.*)$", hm, re.M).group(1).split()
    assert re.search(r"^icpgn_batch_smoke: icpgn_batch_smoke.cpp lis_slam_registration.hpp", hm, re.M)
    assert "lis-slam_amd/host/icpgn_batch_smoke" in open(os.path.join(ROOT, ".gitignore")).read().split()


def test_icpgn_batch_smoke_compiles_and_the_mirror_has_the_verifier():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists
    subprocess.check_call(["make", "-s", "-C", HOST, "icpgn_batch_smoke"])
    exe = os.path.join(HOST, "icpgn_batch_smoke")
    assert os.path.exists(exe)
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    assert hdr.index("class GicpVerifier") < hdr.index("// OptimizedICPGN") < hdr.index("class OptimizedICPGN") < hdr.index("class IcpGnVerifier")
    body = hdr[hdr.index("class IcpGnVerifier"):hdr.index("SURVEY.md §8 f-3 composite")]
    for name in ("setCandidateTarget", "addCandidate", "clearCandidates", "matchAll", "best", "result", "fitness", "lisreg_icp_gn_match_batch",
                 "lisreg_map_index_set"):
        assert name in body, name
    if lisreg.lib().lisreg_device_count() == 0:    # without a device the program fails loudly and says so
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "failed loudly as designed" in r.stdout, r.stdout + r.stderr
