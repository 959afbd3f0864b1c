"""plan_split_uneven (lis-slam_amd/csrc/lisreg_batch_plan.hpp), the cut of a free-running interleaved run, against a brute-force search:
lis-slam_amd/host/split_uneven_check.cpp builds as plain host code — no HIP call, no library of the project — and finds on 4000 random item
tables, for nine target shares each, that the cut is an item boundary, that no part is under a quarter of the workgroups, that it is
plan_split's answer exactly when no boundary qualifies, and that it is the qualifying boundary nearest the share; and that split_form /
plan_run_split — whether a run is cut at all: the option, and under the default the floor of 16384 workgroups, the bound of 64 registrations,
the fixed iteration count and the other contexts — give what a hand-written table of edges and a restatement over random arguments give."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_split_uneven_check_compiles_without_warnings_and_passes(tmp_path):
    exe = str(tmp_path / "split_uneven_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__",
                           "-I" + HIP_INCLUDE, "-I" + CSRC, "-o", exe, os.path.join(HOST, "split_uneven_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "split_uneven_check ok" in r.stdout, r.stdout + r.stderr
    assert "tables 4000 " in r.stdout
    hits = dict(re.findall(r" ([\w+-]+)=(\d+)", r.stdout))
    for edge in ("no_boundary_qualifies", "even_cut_also_none", "uneven_where_even_is_none", "same_as_even", "differs_from_even", "tie_takes_earlier",
                 "exactly_a_quarter", "empty_items", "two_items", "one_item", "no_items", "big_batch", "auto_split", "auto_refused_by_items",
                 "auto_refused_by_floor", "auto_refused_by_free_iters", "auto_refused_by_other_context"):
        assert int(hits[edge]) > 0, (edge, r.stdout)


def test_the_check_is_built_with_the_host_programs():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert "split_uneven_check" in re.search(r"^all:(.*)$", mk, re.M).group(1)
    assert re.search(r"^split_uneven_check: split_uneven_check.cpp ../csrc/lisreg_batch_plan.hpp", mk, re.M)
    src = open(os.path.join(HOST, "split_uneven_check.cpp")).read()
    assert '#include "lisreg_batch_plan.hpp"' in src and not re.search(r"\bhip[A-Z]\w*\(", src)      # no HIP API call
