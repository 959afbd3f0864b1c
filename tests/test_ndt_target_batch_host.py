"""The device-free side of lisreg_ndt_set_target_batch: the header, the library and the binding agree on the entry
points, the two constants and the job struct; the unit is built like lisreg_ndt.hip, whose voxel kernels share its per-voxel body; the
voxel sort of a batch of targets exists once, in the header both voxel-keeping target batches include."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HDR = os.path.join(ROOT, "include", "lisreg.h")
CTYPE = {"int": C.c_int, "const void*": C.c_void_p}
SYMBOLS = ("lisreg_ndt_set_target_batch", "lisreg_ndt_get_target", "lisreg_ndt_target_batch_counts")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}


def test_the_header_declares_the_entry_points():
    hdr = re.sub(r"\s+", " ", open(HDR).read())
    assert ("int lisreg_ndt_set_target_batch(lisreg_ctx* ctx, int n_targets, lisreg_ndt_target_job* jobs, "
            "const lisreg_ndt_params* params);") in hdr
    assert ("int lisreg_ndt_get_target(lisreg_ctx* ctx, int slot, lisreg_ndt_info* info, int voxel_dims[3], int voxel_min_b[3], "
            "double* resolution, float geom[11], int grid_dims[3], int* n_points, int* n_records, float* sorted_xyzw, int* cell_start, "
            "int* table, int* record_cells, int* record_flags, double* records, int capacity_points, int capacity_cells, "
            "int capacity_table, int capacity_records);") in hdr
    assert "int lisreg_ndt_target_batch_counts(const lisreg_ctx* ctx, int* enqueues, int* synchronisations);" in hdr
    assert int(re.search(r"#define LISREG_NDT_TARGET_BATCH_MAX (\d+)", hdr).group(1)) == 1024
    assert int(re.search(r"#define LISREG_NDT_TARGET_BATCH_MAX_POINTS (\d+)", hdr).group(1)) == 134217728
    # the block sits behind lisreg_ndt_align_batch
    assert hdr.index("int lisreg_ndt_align_batch(") < hdr.index("§7v") < hdr.index("int lisreg_ndt_set_target_batch(")


def test_the_job_struct_of_the_header_is_the_bindings():
    import lisreg
    hdr = open(HDR).read()
    body = re.search(r"typedef struct lisreg_ndt_target_job \{(.*?)\} lisreg_ndt_target_job;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [re.sub(r"\s+", " ", d).strip() for d in body.split(";") if d.strip()]
    fields = [(d.rsplit(" ", 1)[0], d.rsplit(" ", 1)[1]) for d in decls]
    assert [f[1] for f in fields] == ["slot", "n", "cloud", "status", "info"]
    assert [f[0] for f in fields] == ["int", "int", "const void*", "int", "lisreg_ndt_info"]
    # the x86-64 / LP64 layout of the C struct, worked out from the declarations: every member at the next multiple of its alignment
    info_body = re.search(r"typedef struct lisreg_ndt_info \{(.*?)\} lisreg_ndt_info;", hdr, re.S).group(1)
    info_decl = re.sub(r"/\*.*?\*/", "", info_body, flags=re.S)
    info_ints = sum(int(m.group(1) or 1) for m in re.finditer(r"\bint\s+\w+(?:\[(\d+)\])?\s*;", info_decl))
    assert [d.split()[0] for d in info_decl.split(";") if d.strip()] == ["int"] * 4              # nothing but ints in it
    assert info_ints == 6 and C.sizeof(lisreg.NdtInfo) == 4 * info_ints
    off, offsets, align_max = 0, [], 1
    for ctype, _ in fields:
        size, align = (4 * info_ints, 4) if ctype == "lisreg_ndt_info" else (C.sizeof(CTYPE[ctype]), C.alignment(CTYPE[ctype]))
        off = (off + align - 1) // align * align
        offsets.append(off)
        off += size
        align_max = max(align_max, align)
    size = (off + align_max - 1) // align_max * align_max
    J = lisreg.NdtTargetJob
    assert [f[0] for f in J._fields_] == [f[1] for f in fields]
    assert [getattr(J, f[0]).offset for f in J._fields_] == offsets and C.sizeof(J) == size
    assert offsets == [0, 4, 8, 8 + C.sizeof(C.c_void_p), 12 + C.sizeof(C.c_void_p)]
    assert lisreg.NDT_TARGET_BATCH_MAX == int(re.search(r"#define LISREG_NDT_TARGET_BATCH_MAX (\d+)", hdr).group(1))
    assert lisreg.NDT_TARGET_BATCH_MAX_POINTS == int(re.search(r"#define LISREG_NDT_TARGET_BATCH_MAX_POINTS (\d+)", hdr).group(1))
    for name in ("ndt_set_target_batch", "ndt_get_target", "ndt_target_batch_counts"):
        assert hasattr(lisreg.Context, name), name


def test_the_library_exports_the_symbols():
    import lisreg
    out = subprocess.run(["nm", "-D", "--defined-only", lisreg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in SYMBOLS:
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym), sym
        assert re.search(rf" T {sym}$", out, re.M), sym
    # without a context none computes
    L = lisreg.lib()
    N = None
    assert L.lisreg_ndt_set_target_batch(None, 0, None, None) == lisreg.ERR_ARG
    assert L.lisreg_ndt_get_target(None, 0, N, N, N, N, N, N, N, N, N, N, N, N, N, N, 0, 0, 0, 0) == lisreg.ERR_ARG
    e, s = C.c_int(0), C.c_int(0)
    assert L.lisreg_ndt_target_batch_counts(None, C.byref(e), C.byref(s)) == lisreg.ERR_ARG


def test_the_unit_is_built_like_the_single_call():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_ndt_target_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    fpc = {u: re.search(rf"^FPC_{u} := (\w+)$", mk, re.M).group(1) for u in ("lisreg_ndt", "lisreg_ndt_target_batch")}
    assert fpc == {"lisreg_ndt": "off", "lisreg_ndt_target_batch": "off"}
    assert "-fno-slp-vectorize" in re.search(r"^CXXFLAGS\s*=(.*)$", mk, re.M).group(1)           # every unit's, the single call's among them
    # one compile rule for every unit: no rule of its own gives the new unit other flags
    assert "lisreg_ndt_target_batch.o" not in mk and len(re.findall(r"^\$\(OUTDIR\)/%\.o:", mk, re.M)) == 1


def test_the_gaussian_and_the_per_voxel_body_exist_once():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    text = _sources()
    for unit in ("lisreg_ndt", "lisreg_ndt_target_batch"):
        hdrs = re.search(rf"^HDR_{unit} :=(.*)$", mk, re.M).group(1).split()
        assert "lisreg_ndt_voxel_lane.hpp" in hdrs and "lisreg_fp64_sums.hpp" in hdrs and "lisreg_jacobi3.hpp" in hdrs, unit
        assert '#include "lisreg_ndt_voxel_lane.hpp"' in text[unit + ".hip"] and "ndt_voxel_lane<WAVE, " in text[unit + ".hip"], unit
    assert [f for f, t in text.items() if re.search(r"\bbool ndt_gaussian\(", t)] == ["lisreg_ndt_voxel_lane.hpp"]
    assert [f for f, t in text.items() if re.search(r"void ndt_voxel_lane\(", t)] == ["lisreg_ndt_voxel_lane.hpp"]
    # the body's own statements: the second-moment sums and the two counts
    assert [f for f, t in text.items() if "c00 += d0 * d0;" in t] == ["lisreg_ndt_voxel_lane.hpp"]
    assert [f for f, t in text.items() if "ndt_count(&counters[1], ok);" in t] == ["lisreg_ndt_voxel_lane.hpp"]
    assert sorted(f for f, t in text.items() if "ndt_gaussian(" in t) == ["lisreg_ndt_voxel_lane.hpp"]
    # the launch shells stay family-agnostic
    assert "Ndt" not in re.sub(r"//.*", "", text["lisreg_fp64_sums.hpp"]) and "k_voxel_stats_small_dev" in text["lisreg_fp64_sums.hpp"]


def test_the_voxel_sort_of_a_batch_exists_once():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    text = _sources()
    for unit in ("lisreg_vgicp_target_batch", "lisreg_ndt_target_batch"):
        hdrs = re.search(rf"^HDR_{unit} :=(.*)$", mk, re.M).group(1).split()
        assert "lisreg_voxel_sort_batch.hpp" in hdrs and "lisreg_target_batch_shared.hpp" in hdrs and "lisreg_voxel_shared.hpp" in hdrs, unit
        assert '#include "lisreg_voxel_sort_batch.hpp"' in text[unit + ".hip"] and '#include "lisreg_target_batch_shared.hpp"' in text[unit + ".hip"], unit
        assert "launch_voxel_sort_targets(" in text[unit + ".hip"] and "k_vt_fill<<<" in text[unit + ".hip"], unit
        assert "static __device__ __forceinline__ uint32_t key(" in text[unit + ".hip"], unit     # what differs: where a record's key comes from
    for kernel in ("k_vt_keys", "k_vt_scatter", "k_vt_rank", "k_vt_heads", "k_vt_finish", "k_vt_starts", "k_vt_fill"):
        assert [f for f, t in text.items() if re.search(rf"void {kernel}\(", t)] == ["lisreg_voxel_sort_batch.hpp"], kernel
    # phases A and B: still one copy, which the NDT unit runs without the distributions
    for kernel in ("k_ft_tiles", "k_ft_stats", "k_ft_compact", "k_ft_knn"):
        assert [f for f, t in text.items() if re.search(rf"void {kernel}\(", t)] == ["lisreg_target_batch_shared.hpp"], kernel
    assert "ft_phase_b(c, F, 0, enq)" in text["lisreg_ndt_target_batch.hip"] and "k_ft_knn" not in text["lisreg_ndt_target_batch.hip"]
    # the geometry of both grids: the single call's functions
    assert "voxel_table_geometry(" in text["lisreg_ndt_target_batch.hip"] and "vg_grid_geometry(" in text["lisreg_ndt_target_batch.hip"]
    assert sum(t.count("fabs(lo) < 2.0e9") for t in text.values()) == 1
