"""CPU restatement of the reference's laser pretreatment — the yardstick of lisreg_pretreat (tests/test_pretreat.py).

LaserPretreatment::Pretreatment (reference src/core/laserPretreatment.cpp:4-81; the same loop at :84-161 and twice inline in
src/node/laserPretreatmentNode.cpp:60-219; removeClosedPointCloud in src/include/laserPretreatment.h:25-54), restated from knowledge of
the C++ expressions with their float / double steps:

  1. removeNaNFromPointCloud (:10): keep a point only if x, y, z are all finite.
  2. removeClosedPointCloud (h:40-42): r2 = (x*x + y*y) + z*z in float; drop if r2 < min*min or r2 > max*max (float products).
  3. (:14-18) startOri = -atan2f(y0, x0) of the first survivor of 1-2, endOri = (float)(-atan2f(yl, xl) + 2 pi) of the last; the
     difference endOri - startOri is a float subtraction compared against the doubles 3 pi / pi; endOri -= / += 2 pi is a double sum
     rounded to float.
  4. (:30) angle = atanf(z / sqrtf(x*x + y*y)) * 180 / M_PI: float product with 180, double division by M_PI, stored as float.
     ring (:33-56): 16: int((angle + 15) / 2 + 0.5), float sum and quotient, + 0.5 in double, drop if > 15 or < 0;
     32: int((angle + 92.0/3.0) * 3.0 / 4.0) in double, drop if > 31 or < 0; 64: angle >= -8.83 ? int((2 - angle) * 3.0 + 0.5) :
     32 + int((-8.83 - angle) * 2.0 + 0.5) with `2 - angle` a float difference, drop if angle > 2 || angle < -24.33 || ring > 50 ||
     ring < 0.  int() truncates toward zero.  A NaN angle converts to INT_MIN on x86 and fails `ring < 0`: dropped.
  5. (:62-76) ori = -atan2f(y, x); the halfPassed state machine; relTime float; time = (float)(scanPeriod * relTime), double product.
     A point dropped in step 4 `continue`s before this.
  6. kept points in input order.

A float libm function is DEFINED as the correctly rounded value (the double function rounded once to float), as everywhere in this
repository; sqrtf and float division are exact by IEEE.  An empty cloud after steps 1-2 (the reference reads points[0] there: undefined)
is defined as: nothing kept, startOri = endOri = 0, half_index = -1.

Two forms: `pretreat_sequential` is the literal loop with its halfPassed flag; `pretreat_vectorised` is the parallel form the HIP kernels
implement (halfPassed is monotone: with a_i the first-branch ori of kept point i and k = min{i kept: a_i - startOri > pi}, points i <= k
take the first branch and points i > k the second).  Both return the same dict."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
PI = f64(math.pi)
TWO_PI = f64(2) * PI
SCAN_PERIOD = 0.1                       # laserPretreatment.h:12


def _survivors(raw, min_range, max_range):
    """steps 1-2 on an (n, 4) float32 array: boolean mask"""
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(over="ignore", invalid="ignore"):
        r2 = (x * x + y * y) + z * z                                   # float32 throughout
    mn, mx = f32(min_range) * f32(min_range), f32(max_range) * f32(max_range)
    with np.errstate(invalid="ignore"):
        ok &= ~(r2 < mn) & ~(r2 > mx)
    return ok


def _libm(fn, *args):
    """A double libm function, element by element through the C library (numpy's own vector loops may use other implementations
    that differ in the last ulp from one CPU to the next)"""
    arrs = [np.atleast_1d(np.asarray(a, f64)) for a in args]
    return np.fromiter((fn(*v) for v in zip(*[a.tolist() for a in arrs])), f64, count=len(arrs[0]))


def _neg_atan2f(y, x):
    """-atan2f(y, x) on float32 arrays"""
    return -_libm(math.atan2, y, x).astype(f32)


def _ends(raw, ok):
    """step 3: (startOri, endOri, end_branch) — end_branch 0: no adjustment, 1: -= 2 pi, 2: += 2 pi"""
    idx = np.flatnonzero(ok)
    if len(idx) == 0:
        return f32(0), f32(0), 0
    a, b = raw[idx[0]], raw[idx[-1]]
    start = _neg_atan2f(a[1], a[0])[0]
    end = f32(f64(_neg_atan2f(b[1], b[0])[0]) + TWO_PI)
    branch = 0
    if f64(f32(end - start)) > f64(3) * PI:
        end, branch = f32(f64(end) - TWO_PI), 1
    elif f64(f32(end - start)) < PI:
        end, branch = f32(f64(end) + TWO_PI), 2
    return start, end, branch


def _angle(raw):
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ratio = z / np.sqrt(x * x + y * y)                             # float32
        at = _libm(math.atan, ratio).astype(f32)
        return ((at * f32(180)).astype(f64) / PI).astype(f32)


def _trunc(v):
    """int(double) for finite values in int range (the callers mask NaN first)"""
    return np.trunc(v).astype(np.int64)


def _rings(angle, n_scan):
    """step 4: (ring, keep)"""
    nan = np.isnan(angle)
    a32 = np.where(nan, f32(0), angle).astype(f32)
    a = a32.astype(f64)
    if n_scan == 16:
        ring = _trunc(((a32 + f32(15)) / f32(2)).astype(f64) + f64(0.5))
        keep = ~((ring > 15) | (ring < 0))
    elif n_scan == 32:
        ring = _trunc((a + f64(92.0) / f64(3.0)) * f64(3.0) / f64(4.0))
        keep = ~((ring > 31) | (ring < 0))
    elif n_scan == 64:
        up = _trunc((f32(2) - a32).astype(f64) * f64(3.0) + f64(0.5))
        lo = 32 + _trunc((f64(-8.83) - a) * f64(2.0) + f64(0.5))
        ring = np.where(a >= f64(-8.83), up, lo)
        keep = ~((a > f64(2)) | (a < f64(-24.33)) | (ring > 50) | (ring < 0))
    else:
        raise ValueError("wrong scan number")                          # ROS_BREAK (:57-60)
    return ring, keep & ~nan


def _result(raw, kept_idx, ring, time, start, end, half_index, end_branch):
    kept_idx = np.asarray(kept_idx, np.int64)
    return dict(index=kept_idx, ring=np.asarray(ring, np.uint16), time=np.asarray(time, f32), xyzi=raw[kept_idx].copy(),
                start_ori=f32(start), end_ori=f32(end), half_index=int(half_index), end_branch=end_branch)


def pretreat_sequential(raw, n_scan=64, min_range=0.0, max_range=70.0, scan_period=SCAN_PERIOD):
    """The literal loop (:23-78) over the survivors of steps 1-2, one point at a time, with the halfPassed flag."""
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4)
    ok = _survivors(raw, min_range, max_range)
    start, end, branch = _ends(raw, ok)
    idx = np.flatnonzero(ok)
    ring_all, keep_all = _rings(_angle(raw[idx]), n_scan) if len(idx) else (np.zeros(0, np.int64), np.zeros(0, bool))
    half_passed, half_index = False, -1
    out_i, out_r, out_t = [], [], []
    for j, i in enumerate(idx):
        if not keep_all[j]:
            continue                                                    # count--; continue (:36-37, 43-44, 53-54)
        ori = f32(-f32(math.atan2(float(raw[i, 1]), float(raw[i, 0]))))
        if not half_passed:
            if f64(ori) < f64(start) - PI / f64(2):
                ori = f32(f64(ori) + TWO_PI)
            elif f64(ori) > f64(start) + PI * f64(3) / f64(2):
                ori = f32(f64(ori) - TWO_PI)
            if f64(f32(ori - start)) > PI:
                half_passed, half_index = True, len(out_i)
        else:
            ori = f32(f64(ori) + TWO_PI)
            if f64(ori) < f64(end) - PI * f64(3) / f64(2):
                ori = f32(f64(ori) + TWO_PI)
            elif f64(ori) > f64(end) + PI / f64(2):
                ori = f32(f64(ori) - TWO_PI)
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = f32(f32(ori - start) / f32(end - start))
        out_i.append(i); out_r.append(ring_all[j]); out_t.append(f32(f64(scan_period) * f64(rel)))
    return _result(raw, out_i, out_r, out_t, start, end, half_index, branch)


def pretreat_vectorised(raw, n_scan=64, min_range=0.0, max_range=70.0, scan_period=SCAN_PERIOD):
    """The parallel form: index reductions for first / last / k, a compaction, per-point arithmetic."""
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4)
    ok = _survivors(raw, min_range, max_range)
    start, end, branch = _ends(raw, ok)
    ring, keep = _rings(_angle(raw), n_scan)
    keep &= ok
    ori = _neg_atan2f(raw[:, 1], raw[:, 0])
    o64 = ori.astype(f64)
    a = np.where(o64 < f64(start) - PI / f64(2), (o64 + TWO_PI).astype(f32),
                 np.where(o64 > f64(start) + PI * f64(3) / f64(2), (o64 - TWO_PI).astype(f32), ori)).astype(f32)
    with np.errstate(invalid="ignore"):
        flips = keep & ((a - start).astype(f32).astype(f64) > PI)
    k = int(np.flatnonzero(flips)[0]) if flips.any() else -1
    b = (o64 + TWO_PI).astype(f32)
    b64 = b.astype(f64)
    b = np.where(b64 < f64(end) - PI * f64(3) / f64(2), (b64 + TWO_PI).astype(f32),
                 np.where(b64 > f64(end) + PI / f64(2), (b64 - TWO_PI).astype(f32), b)).astype(f32)
    first_half = np.arange(len(raw)) <= k if k >= 0 else np.ones(len(raw), bool)
    o = np.where(first_half, a, b).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = ((o - start).astype(f32) / f32(end - start)).astype(f32)
    time = (f64(scan_period) * rel.astype(f64)).astype(f32)
    idx = np.flatnonzero(keep)
    half_index = int(np.searchsorted(idx, k)) if k >= 0 else -1
    return _result(raw, idx, ring[idx], time[idx], start, end, half_index, branch)


def to_xyzirt(res, dtype):
    """The result as PointXYZIRT structs (`dtype`: lisreg.synth.XYZIRT_DTYPE)."""
    out = np.zeros(len(res["index"]), dtype)
    out["x"], out["y"], out["z"], out["intensity"] = res["xyzi"][:, 0], res["xyzi"][:, 1], res["xyzi"][:, 2], res["xyzi"][:, 3]
    out["ring"], out["time"] = res["ring"], res["time"]
    return out


def same(a, b):
    """bit-for-bit equality of two results; returns the name of the first field that differs, or None"""
    for key in ("index", "ring"):
        if not np.array_equal(a[key], b[key]):
            return key
    for key in ("time", "xyzi"):
        if a[key].shape != b[key].shape or not np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)):
            return key
    for key in ("start_ori", "end_ori"):
        if f32(a[key]).view(np.uint32) != f32(b[key]).view(np.uint32):
            return key
    return None if a["half_index"] == b["half_index"] else "half_index"


def make_sweep(seed, n_scan, order="ring", span=2.0, n_az=120, beams=None, inject=True, bad_ends=False, half_turn=False, az0=None):
    """A seeded raw sweep (n, 4) float32: `beams` elevation rows x n_az azimuth steps covering `span` x pi radians clockwise (the
    reference negates atan2, so time grows with decreasing atan2), noisy ranges; order 'ring' (ring-major), 'time' (azimuth-major) or
    'shuffled'; optionally NaN / inf / zero points injected and invalid first / last points.  az0: azimuth of the first column (seeded
    when None).  The lowest rows lie below each table, the next ones of the 16 and 32 tables inside the window where the ring expression
    is in (-1, 0) and truncates to ring 0."""
    rng = np.random.default_rng(seed)
    beams = beams or n_scan
    lo, hi = {16: (-19.5, 17.5), 32: (-33.0, 12.0), 64: (-26.0, 4.0)}[n_scan]        # a little beyond each table on both sides
    el = np.radians(np.linspace(lo, hi, beams))
    total = (0.8 if half_turn else span) * np.pi
    az0 = rng.uniform(-np.pi, np.pi) if az0 is None else az0
    az = az0 - np.linspace(0.0, total, n_az, endpoint=False)
    E, A = np.meshgrid(el, az, indexing="ij")                         # ring-major
    E = E + rng.normal(0, 0.002, E.shape)
    R = rng.uniform(2.0, 60.0, E.shape)
    R[rng.random(E.shape) < 0.02] = 90.0                               # beyond max_range
    x, y, z = R * np.cos(E) * np.cos(A), R * np.cos(E) * np.sin(A), R * np.sin(E)
    if order == "time":
        x, y, z = x.T, y.T, z.T
    pts = np.stack([x.ravel(), y.ravel(), z.ravel(), rng.uniform(0, 1, x.size)], 1).astype(f32)
    if order == "shuffled":
        pts = pts[rng.permutation(len(pts))]
    if inject:
        m = len(pts)
        for val, cnt in ((np.nan, 7), (np.inf, 5), (-np.inf, 3)):
            pts[rng.integers(0, m, cnt), rng.integers(0, 3, cnt)] = val
        pts[rng.integers(0, m, 6), :3] = 0.0                           # NaN angle when min_range is 0
    if bad_ends:
        pts[0, 0] = np.nan; pts[1, :3] = 0.0; pts[1, 0] = 500.0; pts[-1, 2] = np.inf; pts[-2, :3] = (0.0, 400.0, 0.0)
    return pts
