"""Process teardown: every way a host process can end with liblisreg.so in it must exit with status 0.

Round 3's GPU run passed all its tests and then aborted at interpreter exit (glibc "double free or corruption", status 134).  The
backtrace (tests/probes/abrt_bt.c, LD_PRELOAD) put the abort in the static destructor of librocm_smi64's std::map<DevInfoTypes, ...>:
lisreg_comm_* had dlopen'ed the SYSTEM librccl.so RTLD_GLOBAL (which brings the system librocm_smi64.so.1), a later test imported
torch, whose wheel carries its own librocm_smi64 (soname .so.7) — the global copy interposed the wheel's symbols and both destructors
freed the same map.  The same two lines reproduce it without liblisreg in the process at all.  Fixed on both sides: the library now
reuses an RCCL the process already has and otherwise loads one RTLD_LOCAL; the GPU tests no longer import torch.

Each case below is a fresh interpreter (subprocess), because the thing under test is its exit status.
"""
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PRELUDE = f"""
import sys
sys.path.insert(0, {os.path.join(ROOT, "lis-slam_amd")!r})
import ctypes as C
import numpy as np
"""


def run_case(body: str, timeout: int = 300):
    code = PRELUDE + textwrap.dedent(body)
    env = dict(os.environ)
    env.setdefault("MALLOC_CHECK_", "3")                 # glibc aborts on the first inconsistent free, not on a later one
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    return r


def check(r, marker="CASE_DONE"):
    assert marker in r.stdout, f"the case did not reach its end:\n{r.stdout}\n{r.stderr}"
    assert r.returncode == 0, f"exit status {r.returncode}\n--- stdout\n{r.stdout}\n--- stderr\n{r.stderr[-3000:]}"


SMALL_BATCH = """
import lisreg
from lisreg import synth
cases = [synth.make_case(h=64, w=900, m_points=40000, scan_seed=3900 + i) for i in range(6)]
p = lisreg.default_params(1); p.fixed_iters = 2
n = len(cases)
T0 = np.stack([c["T_init"] for c in cases]).astype(np.float32)
def items():
    arr, keep = (lisreg.Item * n)(), []
    for i, c in enumerate(cases):
        sc = np.ascontiguousarray(c["src_corner"]); ss = np.ascontiguousarray(c["src_surf"]); keep += [sc, ss]
        arr[i].src_corner = sc.ctypes.data_as(C.c_void_p); arr[i].n_corner = len(sc)
        arr[i].src_surf = ss.ctypes.data_as(C.c_void_p); arr[i].n_surf = len(ss)
        arr[i].stride_bytes = sc.dtype.itemsize; arr[i].fmt = lisreg.FMT_XYZI
    return arr, keep
"""


@pytest.mark.gpu
def test_create_stage_run_destroy_exits_cleanly():
    """create -> stage_host_items (feeder threads, copy stream, pinned staging) -> prepare / run / fetch -> destroy -> exit."""
    check(run_case(SMALL_BATCH + """
ctx = lisreg.Context(0)
ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
arr, keep = items()
staged = (lisreg.Item * n)()
assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
assert ctx._L.lisreg_batch_prepare(ctx._h, n, staged, C.byref(p), T0.ctypes.data_as(C.POINTER(C.c_float))) == 0
assert ctx._L.lisreg_batch_run(ctx._h) == 0
ctx._n_items = n
T, st = ctx.batch_fetch()
assert all(s["status"] == 0 for s in st)
ctx.close()
print("CASE_DONE")
"""))


@pytest.mark.gpu
def test_destroy_with_uploads_still_in_flight_exits_cleanly():
    """destroy right after staging: the copy stream still carries uploads out of the pinned buffers that are about to be freed."""
    check(run_case(SMALL_BATCH + """
for rep in range(3):
    ctx = lisreg.Context(0)
    ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
    arr, keep = items()
    staged = (lisreg.Item * n)()
    assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
    assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
    ctx.close()
print("CASE_DONE")
"""))


@pytest.mark.gpu
def test_leaked_context_exits_cleanly():
    """a context that is never destroyed (feeder threads parked on their condition variable, device memory live) at process exit."""
    check(run_case(SMALL_BATCH + """
ctx = lisreg.Context(0)
ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
arr, keep = items()
staged = (lisreg.Item * n)()
assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
ctx._h = None            # leak it: no lisreg_destroy, neither now nor from __del__
leak2 = lisreg.Context(0)   # and one that reaches __del__ during interpreter shutdown
print("CASE_DONE")
"""))


@pytest.mark.gpu
def test_stage_error_paths_leave_no_live_job():
    """bad arguments after a good call, then a good call again: the thread pool and its tables survive refused calls."""
    check(run_case(SMALL_BATCH + """
ctx = lisreg.Context(0)
ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
arr, keep = items()
staged = (lisreg.Item * n)()
assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
bad, _ = items(); bad[2].stride_bytes = 4
assert ctx._L.lisreg_stage_host_items(ctx._h, n, bad, staged) != 0
bad2, _ = items(); bad2[1].src_surf = None
assert ctx._L.lisreg_stage_host_items(ctx._h, n, bad2, staged) != 0
for _ in range(4):
    assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
assert ctx._L.lisreg_batch_prepare(ctx._h, n, staged, C.byref(p), T0.ctypes.data_as(C.POINTER(C.c_float))) == 0
assert ctx._L.lisreg_batch_run(ctx._h) == 0
ctx._n_items = n
T, st = ctx.batch_fetch()
assert all(s["status"] == 0 for s in st)
ctx.close()
print("CASE_DONE")
"""))


@pytest.mark.gpu
def test_native_rccl_then_exit_is_clean():
    """lisreg_comm_* with one rank (librccl loaded by the library), context destroyed, exit."""
    check(run_case("""
import lisreg
ctx = lisreg.Context(0)
ctx.comm_init(0, 1, lisreg.comm_unique_id())
out = lisreg.DeviceArray(np.zeros((2, 12), np.float32))
src = lisreg.DeviceArray(np.arange(24, dtype=np.float32).reshape(2, 12))
ctx.gather_results(src.ptr, 2, out.ptr)
assert np.array_equal(lisreg.device_to_host(out.ptr, (2, 12)), np.arange(24, dtype=np.float32).reshape(2, 12))
ctx.close()
print("CASE_DONE")
"""))


# free(1) - free(N) of the case below on the commit before the owners (bytes), and the smallest non-zero step hipMemGetInfo took there
# (around one 64-byte lisreg.DeviceArray, grown until the reading moved): both measured on an MI355X, see the docstring
PARENT_DROP_BYTES = 16777216
MEMINFO_STEP_BYTES = 2097152


@pytest.mark.gpu
def test_destroy_gives_device_memory_back():
    """6 cycles of create -> every subsystem that owns device memory -> destroy in one process: registrations on cell rows (search_mode 5)
    and on the graph (3), a staged host batch (feeder), lisreg_upload_cloud, the voxel grid single and multi, feature extraction with
    de-skew, the semantic split, a local map, a key-frame ring pushed past 19 frames, a map index with one ICP alignment, a loop database
    grown past 64 frames.  Free device memory (hipMemGetInfo) is read after the destroy of cycle 1 and of cycle 6: a resource that a
    context does not give back costs five times its size between the two readings.
    Measured on the commit before the owners: drop = free(1) - free(6) = 16777216 bytes (all of it between cycles 1 and 2: the five
    readings after that are equal, so it is the runtime settling, not something a context keeps), smallest non-zero step of
    hipMemGetInfo = 2097152 bytes; the bar is their sum.  With the owners: the same six readings, drop 16777216."""
    r = run_case(SMALL_BATCH + """
from lisreg import replay
hip = lisreg.hip_runtime()
def free_bytes():
    fr, tot = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(fr), C.byref(tot)) == 0
    return fr.value
case = synth.make_case(h=16, w=450, m_points=20000, scan_seed=1500)
labelled = next(iter(replay.synthetic_drive(1, h=32, w=900, car=False)))[0]
raw = synth.make_raw_scan(16, 450, 7400)
t_imu = 100.0 - 0.01 + np.arange(70) / 500.0
rot = np.zeros((70, 3)); rot[:, 2] = 0.6 * (t_imu - t_imu[0])         # integrated IMU rotation: a steady yaw rate
drive = synth.make_loop_drive(22, 3, h=16, w=361)
assert len(drive) > 64
# the test's own device arrays live across all cycles: they are in both readings
rec = lisreg.pack_device_records(labelled)
vin = [lisreg.DeviceArray(rec), lisreg.DeviceArray(rec[: len(rec) // 2])]
vout = [lisreg.DeviceArray(np.zeros_like(rec)), lisreg.DeviceArray(np.zeros_like(rec))]
up = lisreg.DeviceArray(np.zeros((len(labelled), 4), np.float32))
def cycle():
    ctx = lisreg.Context(0)
    p1 = lisreg.default_params(1)
    ctx.set_option("search_mode", 5)
    ctx.set_target(case["tgt_corner"], case["tgt_surf"])
    ctx.align(case["src_corner"], case["src_surf"], case["T_init"], p1)
    assert ctx.front_end() == 5
    ctx.set_option("search_mode", 3)
    ctx.align(case["src_corner"], case["src_surf"], case["T_init"], p1)
    assert ctx.front_end() == 3
    ctx.set_option("search_mode", 4)
    ctx.set_target(cases[0]["tgt_corner"], cases[0]["tgt_surf"])
    arr, keep = items()
    staged = (lisreg.Item * n)()
    assert ctx._L.lisreg_stage_host_items(ctx._h, n, arr, staged) == 0
    assert ctx._L.lisreg_batch_prepare(ctx._h, n, staged, C.byref(p), T0.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert ctx._L.lisreg_batch_run(ctx._h) == 0
    ctx._n_items = n
    T, st = ctx.batch_fetch()
    assert all(s["status"] == 0 for s in st)
    assert ctx.upload_cloud(labelled, up.ptr) == len(labelled)
    rc, vox = ctx.voxel_downsample(case["tgt_surf"], 0.4)
    assert rc == 0 and 0 < len(vox) < len(case["tgt_surf"])
    nd = ctx.voxel_downsample_multi_device([a.ptr for a in vin], [len(rec), len(rec) // 2], [0.4, 0.2], [o.ptr for o in vout], [len(rec)] * 2)
    assert all(k > 0 for k in nd)
    feat = ctx.extract_features(raw, lisreg.FeatureParams(16, 450, 1, 0.0, 70.0, 1.0, 0.1),
                                lisreg.make_deskew(t_imu, rot[:, 0], rot[:, 1], rot[:, 2], 100.0))
    assert len(feat["deskewed"]) > 1000
    parts = ctx.semantic_split(labelled)                     # dynamic, ground, building, pole, outlier
    assert sum(len(q) for q in parts) == len(labelled)
    lm = lisreg.localmap_default_params()
    pose = np.array([0, 0, 0.01, 0.2, -0.1, 0.0], np.float32)
    ctx.localmap_reset(0)
    ctx.localmap_insert(0, [parts[0], parts[3], parts[1], parts[2], parts[4]], pose, lm)      # map order: dynamic, pole, ground, building, outlier
    assert ctx.localmap_extract(0, pose, lm, target_slot=3)["n_target_surf"] > 1000
    for k in range(22):
        kf = ctx.keyframes_push(0, case["src_corner"], case["src_surf"], np.array([0, 0, 0.01 * k, 0.1 * k, 0, 0], np.float32))
    assert kf["n_keyframes"] == 19
    assert ctx.keyframes_target(0, 0.2, 0.4, target_slot=1)["n_target_surf"] > 0
    ctx.map_index_set(0, case["tgt_surf"])
    ctx.icp_align(0, case["src_surf"], lisreg.icp_default_params(0))
    ctx.loopdet_reset(0)
    assert len(ctx.loopdet_detect([(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in drive], db_id=0)) == len(drive)
    ctx.close()
N = 6
# the smallest non-zero step of hipMemGetInfo: a small allocation, grown until the reading moves
step, probes, size = 0, [], 64
while step == 0 and size <= 2 ** 28:
    f0 = free_bytes()
    probes.append(lisreg.DeviceArray(np.zeros(size, np.uint8)))
    step = f0 - free_bytes()
    size *= 4
for a in probes: a.free()
free_after = []
for i in range(N):
    cycle()
    free_after.append(free_bytes())
print("FREE_AFTER", free_after)
print("MEMINFO_STEP", step)
print("DROP", free_after[0] - free_after[-1])
print("CASE_DONE")
""", timeout=900)
    print(r.stdout[-2000:])
    check(r)
    drop = int(r.stdout.split("DROP")[1].split()[0])
    assert drop <= PARENT_DROP_BYTES + MEMINFO_STEP_BYTES, (drop, r.stdout[-2000:])


def _have_torch():
    try:
        import importlib.util
        return importlib.util.find_spec("torch") is not None
    except Exception:
        return False


@pytest.mark.gpu
@pytest.mark.skipif(not _have_torch(), reason="torch not installed")
def test_native_rccl_then_torch_import_exits_cleanly():
    """The sequence that aborted round 3's GPU run at exit: the library's RCCL first, then `import torch` (a second set of ROCm
    libraries from the wheel) in the same process.  torch may or may not find the GPU behind a foreign HIP runtime — not our business —
    but the process must end with status 0."""
    check(run_case("""
import lisreg
ctx = lisreg.Context(0)
ctx.comm_init(0, 1, lisreg.comm_unique_id())
ctx.close()
import torch
try:
    t = torch.zeros(1024).pin_memory()
except Exception as e:
    print("torch behind the system HIP runtime:", type(e).__name__)
print("CASE_DONE")
"""))


@pytest.mark.gpu
@pytest.mark.skipif(not _have_torch(), reason="torch not installed")
def test_torch_first_then_native_rccl_exits_cleanly():
    """bench.py's order: torch (with its own HIP runtime and RCCL) first, liblisreg after it; lisreg_comm_* must pick up the RCCL that
    is already in the process (RTLD_NOLOAD) instead of loading the system's next to it."""
    r = run_case("""
import torch
torch.zeros(8, device="cuda:0").sum().item()
import lisreg
ctx = lisreg.Context(0)
ctx.comm_init(0, 1, lisreg.comm_unique_id())
out = lisreg.DeviceArray(np.zeros((2, 12), np.float32))
src = lisreg.DeviceArray(np.arange(24, dtype=np.float32).reshape(2, 12))
ctx.gather_results(src.ptr, 2, out.ptr)
assert np.array_equal(lisreg.device_to_host(out.ptr, (2, 12)), np.arange(24, dtype=np.float32).reshape(2, 12))
ctx.close()
maps = open("/proc/self/maps").read()
rccl = sorted({l.split()[-1] for l in maps.splitlines() if "librccl" in l})
print("rccl copies:", rccl)
assert len(rccl) == 1, rccl
print("CASE_DONE")
""")
    check(r)


def test_teardown_cases_need_a_gpu_and_say_so():
    """CPU box: lisreg_create refuses to run without a device (no fallback) and the interpreter still exits with status 0."""
    r = run_case("""
import lisreg
try:
    lisreg.Context(0)
    print("a device is visible")
except lisreg.LisregError as e:
    print("refused:", e)
print("CASE_DONE")
""")
    check(r)
