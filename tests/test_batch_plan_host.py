"""The batch pipeline's planning functions (lis-slam_amd/csrc/lisreg_batch_plan.hpp) against the closed form of the loops they were cut
out of: lis-slam_amd/host/batch_plan_check.cpp builds as plain host code — no HIP call, no library of the project — and finds every
table of 2400 random batches equal to the byte, with every edge it aims at met."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HIP_INCLUDE = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "include")


def test_batch_plan_check_compiles_without_warnings_and_passes(tmp_path):
    exe = str(tmp_path / "batch_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-D__HIP_PLATFORM_AMD__",
                           "-I" + HIP_INCLUDE, "-I" + CSRC, "-o", exe, os.path.join(HOST, "batch_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "batch_plan_check ok" in r.stdout, r.stdout + r.stderr
    assert "batches 2400 " in r.stdout
    hits = dict(re.findall(r" ([\w+-]+)=(\d+)", r.stdout))
    for edge in ("empty_segment", "seg_256k-1", "seg_256k", "seg_256k+1", "lanes_q_8", "src_131071", "src_131072", "src_131073", "refused_2e9",
                 "slot_unset", "slot_out_of_range", "tile_grew_twice", "nx_above_max_strips", "nx_below_max_strips", "ny_1", "ystrip_1_by_nz",
                 "strip_cells_set_2_targets", "strip_cells_set_3_targets", "strip_cells_unset_2_targets", "strip_cells_unset_3_targets",
                 "split_lop_sided", "split_at_quarter"):
        assert int(hits[edge]) > 0, (edge, r.stdout)


def test_the_check_is_built_with_the_host_programs():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert "batch_plan_check" in re.search(r"^all:(.*)$", mk, re.M).group(1)
    assert re.search(r"^batch_plan_check: batch_plan_check.cpp ../csrc/lisreg_batch_plan.hpp", mk, re.M)
    src = open(os.path.join(HOST, "batch_plan_check.cpp")).read()
    assert '#include "lisreg_batch_plan.hpp"' in src and not re.search(r"\bhip[A-Z]\w*\(", src)      # no HIP API call
