"""The host half of PCL's GICP (lis-slam_amd/csrc/lisreg_gicp_host.hpp) — no GPU:

  * lisreg_gicp_inner (the header as liblisreg.so carries it) against tests/gicp_ref.py on the golden moment records of every outer
    iteration of every alignment case.  The header is the restatement's inner minimisation operation for operation, both sides call
    the same libm for sin / cos / sqrt and neither is built with contraction, so the bar is EQUALITY: every count, the exit and every
    bit of the accepted state and of f;
  * lis-slam_amd/host/gicp_bfgs_check.cpp, the stand-alone program over the header alone: compiles with -Wall -Wextra -Werror and
    passes its own checks (monotone f, Fletcher's two tests on Success, the trial limits, the moment gradient against differences);
  * lis-slam_amd/host/gicp_smoke.cpp and the GicpRegistration of the host mirror compile with plain g++ (tests/test_gicp.py runs the
    program on a GPU box)."""
import os
import re
import subprocess

import numpy as np

import gicp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "gicp", "gicp_cases.npz")


def test_inner_minimisation_equals_the_restatement_bit_for_bit():
    import lisreg
    g = np.load(GOLDEN)
    assert len(g["inner_rec"]) == int(g["align_counts"][:, 1].sum()) == 19          # one record per outer iteration of every case
    differing = []
    for k, (rec, c, x0, x1, cnt, case) in enumerate(zip(g["inner_rec"], g["inner_centre"], g["inner_x0"], g["inner_x1"], g["inner_counts"],
                                                         g["inner_case"])):
        P = lisreg.gicp_default_params(transformation_epsilon=R.ALIGN_CASES[case][3])
        got = lisreg.gicp_inner(rec, c, x0, P)
        ref = R.inner(rec, [float(v) for v in c], [float(v) for v in x0], R.params())
        same = ((got["iters"], got["n_f"], got["n_df"], got["exit"]) == (ref["iters"], ref["n_f"], ref["n_df"], ref["exit"]) == tuple(int(v) for v in cnt)
                and got["x"].tobytes() == np.array(ref["x"]).tobytes() == x1.tobytes() and got["f"] == ref["f"])
        if not same:
            differing.append((k, int(case), got, ref))
    print(f"[gicp_host] lisreg_gicp_inner against gicp_ref.inner on {len(g['inner_rec'])} golden records: {len(differing)} differ")
    assert not differing, differing[:2]
    # the counts of an alignment are the sums over its records
    for case, row in enumerate(g["align_counts"]):
        sel = g["inner_case"] == case
        assert row[2] == g["inner_counts"][sel, 0].sum() and row[3] == g["inner_counts"][sel, 1:3].sum() and row[6] == g["inner_counts"][sel, 3][-1]


def test_inner_refuses_what_it_cannot_minimise():
    import ctypes as C
    import lisreg
    L, P = lisreg.lib(), lisreg.gicp_default_params()
    dp = C.POINTER(C.c_double)
    rec, c, x = np.zeros(74), np.zeros(3), np.zeros(6)
    args = lambda: (rec.ctypes.data_as(dp), c.ctypes.data_as(dp), x.ctypes.data_as(dp), C.byref(P), x.ctypes.data_as(dp), None, None)
    assert L.lisreg_gicp_inner(*args()) == lisreg.ERR_ARG                           # no pair
    rec[73] = float("nan")
    assert L.lisreg_gicp_inner(*args()) == lisreg.ERR_ARG
    g = np.load(GOLDEN)
    rec = g["inner_rec"][0].copy()
    assert L.lisreg_gicp_inner(*args()) == lisreg.OK                                # counts and f may be NULL
    assert L.lisreg_gicp_inner(None, c.ctypes.data_as(dp), x.ctypes.data_as(dp), C.byref(P), x.ctypes.data_as(dp), None, None) == lisreg.ERR_ARG


def test_the_host_header_is_device_free_and_has_one_home():
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    host = text["lisreg_gicp_host.hpp"]
    assert "hip" not in re.sub(r"//.*", "", host).lower() and "__device__" not in host and "static " not in re.sub(r"static constexpr", "", host)
    for needle, home in (("int line_search(", "lisreg_gicp_host.hpp"), ("double bfgs_minimise(", "lisreg_gicp_host.hpp"),
                         ("void gicp_moments_lane(", "lisreg_gicp_lane.hpp"), ("void k_gicp_moments(", "lisreg_gicp.hip"),
                         ("int record_totals(", "lisreg_fp64_sums.hpp")):
        assert [f for f, t in text.items() if needle in t] == [home], needle
    unit, lane = text["lisreg_gicp.hip"], text["lisreg_gicp_lane.hpp"]
    # the shared copies, not second ones: FastGICP's search and pair matrix, the header's butterfly and total, the family's staging
    for needle in ("fg_pairs_lane(", "fg_transform(", "wave_sum("):
        assert needle in lane, needle
    for needle in ("sum_records<kGicpRec>(", "record_totals<kGicpRec>(", "stage_records(", "vg_distributions(", "fg_find_target(", "fg_target_view(",
                   "guess_to_T0(", "emit_aligned("):
        assert needle in unit, needle
    for body in (unit, lane):
        assert "__shfl" not in body and "__shared__" not in body and "atomic" not in body and "asm" not in body and "mfma" not in body.lower()
    assert unit.count("<<<") == 2                                                  # the moments launch and the total: nothing else per round
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_gicp.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1) and re.search(r"^FPC_lisreg_gicp := off$", mk, re.M)
    hdrs = re.search(r"^HDR_lisreg_gicp := (.*)$", mk, re.M).group(1).split()
    assert {"lisreg_fp64_sums.hpp", "lisreg_fgicp_lane.hpp", "lisreg_gicp_lane.hpp", "lisreg_gicp_host.hpp"} <= set(hdrs)


def test_gicp_bfgs_check_compiles_warning_free_and_passes():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert re.search(r"^gicp_bfgs_check: gicp_bfgs_check.cpp ../csrc/lisreg_gicp_host.hpp$", mk, re.M)
    rule = mk[mk.index("gicp_bfgs_check: gicp_bfgs_check.cpp"):].split("\n")[1]
    assert "-Wall -Wextra -Werror" in rule and "-llisreg" not in rule
    subprocess.check_call(["make", "-s", "-C", HOST, "gicp_bfgs_check"])
    r = subprocess.run([os.path.join(HOST, "gicp_bfgs_check")], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "gicp_bfgs_check ok" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    census = re.search(r"^census over (\d+) runs \(most trials of one line search (\d+)\):(.*)$", r.stdout, re.M)
    assert census and int(census.group(1)) >= 100 and int(census.group(2)) <= 100
    seen = dict(re.findall(r"(\w+:\w+) (\d+)", census.group(3)))
    for name in ("bracket:rho", "bracket:sigma", "bracket:slope", "section:shrink", "section:sigma", "section:flip", "section:noprogress",
                 "inner:gradient", "inner:cap", "inner:noprogress"):
        assert int(seen[name]) >= 1, name


def test_gicp_smoke_compiles_and_the_mirror_has_the_registration():
    import lisreg
    lisreg.lib()                                   # makes sure liblisreg.so exists (builds it if the tree is fresh)
    subprocess.check_call(["make", "-s", "-C", HOST, "gicp_smoke"])
    exe = os.path.join(HOST, "gicp_smoke")
    assert os.path.exists(exe)
    hdr = open(os.path.join(HOST, "lis_slam_registration.hpp")).read()
    body = hdr[hdr.index("class GicpRegistration"):hdr.index("// ---- DESIGN.md §7m")]
    for name in ("setMaxCorrespondenceDistance", "setMaximumIterations", "setTransformationEpsilon", "setEuclideanFitnessEpsilon",
                 "setRANSACIterations", "setInputTarget", "setInputSource", "align", "hasConverged", "getFitnessScore",
                 "getFinalTransformation", "lisreg_gicp_align", "lisreg_fgicp_set_target", "lisreg_nearest"):
        assert name in body, name
    if lisreg.lib().lisreg_device_count() == 0:    # without a device the program fails loudly and says so
        r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "failed loudly as designed" in r.stdout, r.stdout + r.stderr
