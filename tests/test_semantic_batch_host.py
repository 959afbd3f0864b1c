"""The device-free side of lisreg_semantic_split_batch and lisreg_concat_device_batch: lis-slam_amd/csrc/lisreg_semantic_batch_plan.hpp
(argument validation, overlap sweep, class table, frame and tile tables, sizes) is plain C++ and
lis-slam_amd/host/semantic_batch_plan_check.cpp holds it against brute force on random batches — no HIP header, no library of the
project; and the header, the library and the binding agree on what the two entry points are."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")


def struct_fields(hdr, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[\d+\]", "", d.split()[-1]).lstrip("*") for d in body.replace("\n", " ").split(";") if d.strip()]


def test_header_library_and_binding_agree():
    """fails without the feature: the symbols, their declarations, the job structs' layouts, the limits, the methods"""
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    L = lisreg.lib()
    for sym in ("lisreg_semantic_split_batch", "lisreg_concat_device_batch"):
        assert sym in lisreg.ABI_SYMBOLS and hasattr(L, sym)
    assert re.search(r"int\s+lisreg_semantic_split_batch\(lisreg_ctx\* ctx, int n_frames, lisreg_semantic_job\* jobs,\s*"
                     r"const uint32_t\* using_label[^)]*\);", hdr)
    assert re.search(r"int\s+lisreg_concat_device_batch\(lisreg_ctx\* ctx, int n_jobs, lisreg_concat_job\* jobs\);", hdr)
    assert int(re.search(r"#define LISREG_SEMANTIC_BATCH_MAX (\d+)", hdr).group(1)) == lisreg.SEMANTIC_BATCH_MAX == 256
    assert int(re.search(r"#define LISREG_CONCAT_BATCH_MAX (\d+)", hdr).group(1)) == lisreg.CONCAT_BATCH_MAX == 1024
    plan = open(os.path.join(CSRC, "lisreg_semantic_batch_plan.hpp")).read()
    threads = int(re.search(r"constexpr int\s+kSbThreads\s*=\s*(\d+);", plan).group(1))
    rounds = int(re.search(r"constexpr int\s+kSbRounds\s*=\s*(\d+);", plan).group(1))
    assert re.search(r"constexpr int\s+kSbTile\s*=\s*kSbThreads \* kSbRounds;", plan)
    assert lisreg.SEMANTIC_BATCH_TILE == threads * rounds
    # lisreg_semantic_job, LP64: in@0 n@8 out@16 (80 bytes) status@96, sizeof 104
    assert struct_fields(hdr, "lisreg_semantic_job") == ["in", "n", "out", "status"]
    J = lisreg.SemanticJob
    assert [f[0].rstrip("_") for f in J._fields_] == ["in", "n", "out", "status"]
    assert [getattr(J, f[0]).offset for f in J._fields_] == [0, 8, 16, 96] and C.sizeof(J) == 104 and C.sizeof(lisreg.SemanticOut) == 80
    # lisreg_concat_job, LP64: in[8]@0 n[8]@64 k@96 out@104 out_capacity@112 n_out@116, sizeof 120
    assert struct_fields(hdr, "lisreg_concat_job") == ["in", "n", "k", "out", "out_capacity", "n_out"]
    K = lisreg.ConcatJob
    assert [f[0].rstrip("_") for f in K._fields_] == ["in", "n", "k", "out", "out_capacity", "n_out"]
    assert [getattr(K, f[0]).offset for f in K._fields_] == [0, 64, 96, 104, 112, 116] and C.sizeof(K) == 120
    assert hasattr(lisreg.Context, "semantic_split_batch_device") and hasattr(lisreg.Context, "concat_device_batch")


def test_plan_check_compiles_without_warnings_and_passes(tmp_path):
    exe = str(tmp_path / "semantic_batch_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HOST, "semantic_batch_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "semantic_batch_plan_check ok" in r.stdout, r.stdout + r.stderr
    hits = dict(re.findall(r" ([\w+-]+)=(\d+)", r.stdout))
    for edge in ("empty_frame", "n_tile-1", "n_tile", "n_tile+1", "one_frame", "256_frames", "257_frames", "negative_n", "null_in", "null_jobs",
                 "negative_cap", "total_above_2e9", "out_meets_own_in", "out_meets_other_in", "out_meets_out_same_job", "out_meets_out_other_job",
                 "in_meets_in_allowed", "touching_ranges_allowed", "null_class", "all_classes_null", "custom_map", "concat_k_9",
                 "concat_short_capacity", "concat_overlap", "concat_1024_jobs", "concat_1025_jobs", "concat_empty_middle"):
        assert int(hits[edge]) > 0, (edge, r.stdout)


def test_the_check_is_built_with_the_host_programs():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert "semantic_batch_plan_check" in re.search(r"^all:(.*)$", mk, re.M).group(1)
    assert re.search(r"^semantic_batch_plan_check: semantic_batch_plan_check.cpp ../csrc/lisreg_semantic_batch_plan.hpp", mk, re.M)
    assert "lis-slam_amd/host/semantic_batch_plan_check\n" in open(os.path.join(ROOT, ".gitignore")).read()
    src = open(os.path.join(HOST, "semantic_batch_plan_check.cpp")).read()
    assert '#include "lisreg_semantic_batch_plan.hpp"' in src and "int main()" in src and not re.search(r"\bhip[A-Z]\w*\(", src)


def test_the_unit_is_in_the_library_and_the_plan_is_plain_cpp():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_semantic_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    assert re.search(r"^HDR_lisreg_semantic_batch := .*lisreg_semantic_batch_plan.hpp", mk, re.M)
    plan = open(os.path.join(CSRC, "lisreg_semantic_batch_plan.hpp")).read()
    assert "hip/" not in plan and not re.search(r"\bhip[A-Z]\w*\(", plan) and "__global__" not in plan and "__device__" not in plan
    unit = open(os.path.join(CSRC, "lisreg_semantic_batch.hip")).read()
    assert '#include "lisreg_semantic_batch_plan.hpp"' in unit and "atomic" not in unit.split("namespace {", 1)[1]      # no atomic decides a place
