"""The device-free side of lisreg_voxel_downsample_batch: lis-slam_amd/csrc/lisreg_voxel_batch_plan.hpp (argument validation, overlap
sweep, offsets, chunk table, bucket budget, scratch sizes) is plain C++ and lis-slam_amd/host/voxel_batch_plan_check.cpp holds it against
brute force on random batches — no HIP header, no library of the project; and the header, the library and the binding agree on what
the entry point is."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")


def test_plan_check_compiles_without_warnings_and_passes(tmp_path):
    exe = str(tmp_path / "voxel_batch_plan_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + CSRC, "-o", exe,
                           os.path.join(HOST, "voxel_batch_plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "voxel_batch_plan_check ok" in r.stdout, r.stdout + r.stderr
    hits = dict(re.findall(r" ([\w+-]+)=(\d+)", r.stdout))
    for edge in ("empty_cloud", "n_256k-1", "n_256k", "n_256k+1", "one_cloud", "1024_clouds", "1025_clouds", "negative_n", "leaf_zero", "leaf_nan",
                 "bad_fmt", "null_in", "null_out", "null_jobs", "negative_capacity", "total_above_2e9", "out_meets_own_in", "out_meets_other_in",
                 "out_meets_out", "in_meets_in_allowed", "touching_ranges_allowed", "bucket_cap_binds", "min_buckets"):
        assert int(hits[edge]) > 0, (edge, r.stdout)


def test_the_check_is_built_with_the_host_programs():
    mk = open(os.path.join(HOST, "Makefile")).read()
    assert "voxel_batch_plan_check" in re.search(r"^all:(.*)$", mk, re.M).group(1)
    assert re.search(r"^voxel_batch_plan_check: voxel_batch_plan_check.cpp ../csrc/lisreg_voxel_batch_plan.hpp", mk, re.M)
    src = open(os.path.join(HOST, "voxel_batch_plan_check.cpp")).read()
    assert '#include "lisreg_voxel_batch_plan.hpp"' in src and not re.search(r"\bhip[A-Z]\w*\(", src)      # no HIP API call
    plan = open(os.path.join(CSRC, "lisreg_voxel_batch_plan.hpp")).read()
    assert "hip/" not in plan and not re.search(r"\bhip[A-Z]\w*\(", plan)                                  # plain C++


def test_the_unit_is_built_without_contraction():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_voxel_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    assert re.search(r"^FPC_lisreg_voxel_batch := off$", mk, re.M)


def test_header_library_and_binding_agree():
    """the binding test that fails without the feature: the symbol, its declaration, the job struct's layout and the batch limit"""
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    assert "lisreg_voxel_downsample_batch" in lisreg.ABI_SYMBOLS
    assert re.search(r"int\s+lisreg_voxel_downsample_batch\(lisreg_ctx\* ctx, int n_clouds, lisreg_voxel_job\* jobs, int fmt\);", hdr)
    assert hasattr(lisreg.lib(), "lisreg_voxel_downsample_batch")
    assert int(re.search(r"#define LISREG_VOXEL_BATCH_MAX (\d+)", hdr).group(1)) == lisreg.VOXEL_BATCH_MAX == 1024
    body = re.search(r"typedef struct lisreg_voxel_job \{(.*?)\} lisreg_voxel_job;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [d.split()[-1].lstrip("*") for d in body.replace("\n", " ").split(";") if d.strip()]
    assert fields == ["in", "n", "leaf", "out", "out_capacity", "n_out", "status"]
    assert [f[0].rstrip("_") for f in lisreg.VoxelJob._fields_] == fields
    # x86-64 / LP64 layout of the C struct: pointer 0, int 8, float 12, pointer 16, int 24, 28, 32; 40 bytes
    J = lisreg.VoxelJob
    assert [getattr(J, f[0]).offset for f in J._fields_] == [0, 8, 12, 16, 24, 28, 32] and C.sizeof(J) == 40
    assert hasattr(lisreg.Context, "voxel_downsample_batch_device")
