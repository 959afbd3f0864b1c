"""The device-free side of lisreg_fgicp_set_target_batch: the header, the library and the binding agree on the two entry
points and on the job struct; the unit is built like lisreg_vgicp.hip, whose kernel shares its per-lane body; and the one grid-geometry
function (vg_grid_geometry of lis-slam_amd/csrc/lisreg_vgicp.hip, lifted out of vg_search_grid) gives the values of the arithmetic it replaced."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lis-slam_amd", "csrc")
HDR = os.path.join(ROOT, "include", "lisreg.h")
CTYPE = {"int": C.c_int, "float": C.c_float, "const void*": C.c_void_p, "lisreg_fgicp_info": None}


def test_the_header_declares_both_entry_points():
    hdr = re.sub(r"\s+", " ", open(HDR).read())
    assert ("int lisreg_fgicp_set_target_batch(lisreg_ctx* ctx, int n_targets, lisreg_fgicp_target_job* jobs, "
            "const lisreg_fgicp_params* params);") in hdr
    assert ("int lisreg_fgicp_get_target(lisreg_ctx* ctx, int slot, lisreg_fgicp_info* info, float geom[11], float* sorted_xyzw, "
            "int* cell_start, int* orig, double* cov6, int capacity_points, int capacity_cells);") in hdr
    assert int(re.search(r"#define LISREG_FGICP_TARGET_BATCH_MAX (\d+)", hdr).group(1)) >= 256
    assert int(re.search(r"#define LISREG_FGICP_TARGET_BATCH_MAX_POINTS (\d+)", hdr).group(1)) >= 1 << 25


def test_the_job_struct_of_the_header_is_the_bindings():
    import lisreg
    hdr = open(HDR).read()
    body = re.search(r"typedef struct lisreg_fgicp_target_job \{(.*?)\} lisreg_fgicp_target_job;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [re.sub(r"\s+", " ", d).strip() for d in body.split(";") if d.strip()]
    fields = [(d.rsplit(" ", 1)[0], d.rsplit(" ", 1)[1]) for d in decls]
    assert [f[1] for f in fields] == ["slot", "n", "cloud", "cell_edge", "status", "info"]
    assert [f[0] for f in fields] == ["int", "int", "const void*", "float", "int", "lisreg_fgicp_info"]
    # the x86-64 / LP64 layout of the C struct, worked out from the declarations: every member at the next multiple of its alignment
    info_body = re.search(r"typedef struct lisreg_fgicp_info \{(.*?)\} lisreg_fgicp_info;", hdr, re.S).group(1)
    info_ints = sum(int(m.group(1) or 1) for m in re.finditer(r"\bint\s+\w+(?:\[(\d+)\])?\s*;", re.sub(r"/\*.*?\*/", "", info_body, flags=re.S)))
    assert info_ints == 4 and C.sizeof(lisreg.FgicpInfo) == 16
    off, offsets, align_max = 0, [], 1
    for ctype, _ in fields:
        size, align = (16, 4) if ctype == "lisreg_fgicp_info" else (C.sizeof(CTYPE[ctype]), C.alignment(CTYPE[ctype]))
        off = (off + align - 1) // align * align
        offsets.append(off)
        off += size
        align_max = max(align_max, align)
    size = (off + align_max - 1) // align_max * align_max
    J = lisreg.FgicpTargetJob
    assert [f[0] for f in J._fields_] == [f[1] for f in fields]
    assert [getattr(J, f[0]).offset for f in J._fields_] == offsets == [0, 4, 8, 16, 20, 24] and C.sizeof(J) == size == 40
    assert lisreg.FGICP_TARGET_BATCH_MAX == int(re.search(r"#define LISREG_FGICP_TARGET_BATCH_MAX (\d+)", hdr).group(1))
    assert lisreg.FGICP_TARGET_BATCH_MAX_POINTS == int(re.search(r"#define LISREG_FGICP_TARGET_BATCH_MAX_POINTS (\d+)", hdr).group(1))
    assert hasattr(lisreg.Context, "fgicp_set_target_batch") and hasattr(lisreg.Context, "fgicp_get_target")


def test_the_library_exports_both_symbols():
    import lisreg
    for sym in ("lisreg_fgicp_set_target_batch", "lisreg_fgicp_get_target", "lisreg_fgicp_grid_geometry", "lisreg_fgicp_target_batch_counts"):
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym), sym
    out = subprocess.run(["nm", "-D", "--defined-only", lisreg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T lisreg_fgicp_set_target_batch$", out, re.M) and re.search(r" T lisreg_fgicp_get_target$", out, re.M)
    # without a context neither computes
    assert lisreg.lib().lisreg_fgicp_set_target_batch(None, 0, None, None) == lisreg.ERR_ARG
    assert lisreg.lib().lisreg_fgicp_get_target(None, 0, None, None, None, None, None, None, 0, 0) == lisreg.ERR_ARG


def test_the_unit_is_built_like_the_single_calls():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "lisreg_fgicp_target_batch.hip" in re.search(r"^SRCS\s*=(.*)$", mk, re.M).group(1)
    assert re.search(r"^FPC_lisreg_fgicp_target_batch := off$", mk, re.M) and re.search(r"^FPC_lisreg_vgicp := off$", mk, re.M)
    for unit in ("lisreg_vgicp", "lisreg_fgicp_target_batch"):
        hdrs = re.search(rf"^HDR_{unit} :=(.*)$", mk, re.M).group(1).split()
        assert "lisreg_vg_knn_lane.hpp" in hdrs, unit
        src = open(os.path.join(CSRC, unit + ".hip")).read()
        assert '#include "lisreg_vg_knn_lane.hpp"' in src and "vg_knn_lane<" in src and "vg_grid_geometry(" in src, unit
    # one copy of the lane arithmetic (the header) and of the geometry choice (a function of lisreg_vgicp.hip, declared in lisreg_ctx.hpp)
    text = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))}
    assert [f for f, t in text.items() if "slack = 1.0e-3 * (double)A.cell" in t] == ["lisreg_vg_knn_lane.hpp"]            # the shell walk's slack
    assert [f for f, t in text.items() if "void lisreg::vg_grid_geometry(" in t] == ["lisreg_vgicp.hip"]
    assert [f for f, t in text.items() if "cell *= 1.26;" in t] == ["lisreg_vgicp.hip"] and text["lisreg_vgicp.hip"].count("cell *= 1.26;") == 1
    assert "void vg_grid_geometry(const float bb[6], int m, float edge, VgGrid* g);" in text["lisreg_ctx.hpp"]


# ---- the grid geometry ------------------------------------------------------------------------------------------------------------------
def parent_geometry(bb, m, edge):
    """the arithmetic vg_search_grid held inline before the function was lifted out (lisreg_vgicp.hip), operation for operation: doubles,
    the float box entries widened first; returns (nx, ny, nz, cell as float32, 1 / cell in float32)"""
    bb = np.asarray(bb, np.float32)
    ex = [float(bb[3]) - float(bb[0]), float(bb[4]) - float(bb[1]), float(bb[5]) - float(bb[2])]
    cell = float(np.float32(edge))
    if not cell > 0:
        area = max(ex[0], 1.0e-3) * max(ex[1], 1.0e-3)
        cell = math.sqrt(4.0 * area / float(m))
    cell = max(cell, 1.0e-4)
    while True:
        nx, ny, nz = math.floor(ex[0] / cell) + 1, math.floor(ex[1] / cell) + 1, math.floor(ex[2] / cell) + 1
        if nx <= 2048 and ny <= 2048 and nz <= 2048 and nx * ny * nz <= float(1 << 22):
            break
        cell *= 1.26
    c32 = np.float32(cell)
    return int(nx), int(ny), int(nz), c32, np.float32(1.0) / c32


# (bb, m, edge) -> dims, cell bits, inv_cell bits: written down from parent_geometry (the assertion below re-runs it)
GEOMETRY_TABLE = [
    # the scene's order of magnitude, from the density
    (((-30.5, -28.25, -2.0, 33.0, 31.5, 9.75), 25401, 0.0), (83, 78, 16, 0x3F45E11A, 0x3FA5988C)),
    # forced edges
    (((0.0, 0.0, 0.0, 6.0, 6.0, 2.0), 700, 0.37), (17, 17, 6, 0x3EBD70A4, 0x402CF915)),
    (((-40.0, 3.0, 0.0, -35.0, 12.0, 3.0), 900, 1.9), (3, 5, 2, 0x3FF33333, 0x3F06BCA2)),
    # a flat cloud: nz = 1
    (((0.0, 0.0, 1.5, 8.0, 8.0, 1.5), 400, 0.0), (11, 11, 1, 0x3F4CCCCD, 0x3FA00000)),
    # a degenerate extent: one point repeated (the footprint falls back to 1e-3 x 1e-3), and a line along z
    (((2.0, 3.0, 4.0, 2.0, 3.0, 4.0), 20, 0.0), (1, 1, 1, 0x39EA77FE, 0x450BC117)),
    (((2.0, 3.0, 0.0, 2.0, 3.0, 50.0), 64, 0.0), (1, 1, 1967, 0x3CD05322, 0x421D4AFB)),
    # more than 2^22 cells at the first edge: the edge grows by 1.26 until the grid fits
    (((0.0, 0.0, 0.0, 100.0, 100.0, 100.0), 200000, 0.0), (141, 141, 141, 0x3F35C251, 0x3FB4485B)),
    (((0.0, 0.0, 0.0, 80.0, 80.0, 40.0), 1000, 0.05), (200, 200, 100, 0x3ECCEA60, 0x401FE8E8)),
    # more than 2048 cells on an axis
    (((0.0, 0.0, 0.0, 1000.0, 1.0, 1.0), 5000, 0.1), (1984, 2, 2, 0x3F011291, 0x3FFDDF6E)),
    # the smallest edge
    (((0.0, 0.0, 0.0, 1.0e-3, 1.0e-3, 0.0), 100, 1.0e-5), (11, 11, 1, 0x38D1B717, 0x461C4000)),
]


def _bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def test_grid_geometry_gives_the_values_of_the_inline_code_it_replaced():
    import lisreg
    seen_cells, seen_dim, seen_flat = False, False, False
    for (bb, m, edge), want in GEOMETRY_TABLE:
        nx, ny, nz, cell, inv = parent_geometry(bb, m, edge)
        got = (nx, ny, nz, _bits(cell), _bits(inv))
        dims, gcell, ginv = lisreg.fgicp_grid_geometry(bb, m, edge)
        lib = (*dims, _bits(gcell), _bits(ginv))
        print(f"[fgicp_target_batch] grid of {bb}, m {m}, edge {edge}: parent {got[:3]} {got[3]:#x} {got[4]:#x}, library {lib[:3]} {lib[3]:#x} {lib[4]:#x}")
        assert got == want, ("the table is not the parent's arithmetic", bb, m, edge, got)
        assert lib == want, (bb, m, edge)
        first = float(np.float32(edge)) if edge > 0 else math.sqrt(4.0 * max(bb[3] - bb[0], 1e-3) * max(bb[4] - bb[1], 1e-3) / m)
        ex = [bb[3] - bb[0], bb[4] - bb[1], bb[5] - bb[2]]
        n0 = [math.floor(e / max(first, 1e-4)) + 1 for e in ex]
        seen_cells |= max(n0) <= 2048 and n0[0] * n0[1] * n0[2] > 1 << 22
        seen_dim |= max(n0) > 2048
        seen_flat |= nz == 1 and ex[2] == 0
    assert seen_cells and seen_dim and seen_flat
    # refused: what the callers never pass
    L = lisreg.lib()
    dims, cell = (C.c_int * 3)(), (C.c_float * 2)()
    for bb, m, edge in (((0, 0, 0, -1, 1, 1), 10, 0.0), ((0, 0, 0, 1, 1, 1), 0, 0.0), ((0, 0, 0, 1, 1, 1), 10, -1.0),
                        ((0, 0, 0, float("inf"), 1, 1), 10, 0.0), ((float("nan"), 0, 0, 1, 1, 1), 10, 0.0)):
        arr = np.array(bb, np.float32)
        assert L.lisreg_fgicp_grid_geometry(arr.ctypes.data_as(C.POINTER(C.c_float)), m, edge, dims, cell) == lisreg.ERR_ARG
