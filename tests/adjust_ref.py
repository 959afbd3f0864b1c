"""CPU restatement of the reference's constant-velocity motion compensation — the yardstick of lisreg_adjust_cloud
(tests/test_adjust_cloud.py).

DistortionAdjust::SetMotionInfo / AdjustCloud / UpdateMatrix (reference src/core/distortionAdjust.cpp:412-480), restated from knowledge
of the C++ expressions and of Eigen's with their float / double steps:

  0. SetMotionInfo (:412-417): scan_period_ is a float; velocity_ and angular_rate_ are Vector3f filled by `<<` from doubles — each rate is
     rounded to float once.
  1. (:437) the loop starts at point_index = 1: point 0 is dropped, the output holds max(n - 1, 0) points in input order.
  2. (:447) real_time = (float)((double)time - (double)scan_period_ / 2.0): `scan_period_ / 2.0` and the difference are double.
  3. (:473) angle = angular_rate_ * real_time: three float products.
  4. (:474-476) three AngleAxisf about UnitZ, UnitY, UnitX; (:478) `t_Vz * t_Vy * t_Vx` converts each to a Quaternionf
     (ha = 0.5f * angle, w = cosf(ha), vec = sinf(ha) * axis: three float products with the axis' 0 / 1 entries, which keep the sign of the
     zeros) and forms two Hamilton products, (qz * qy) * qx, each in the scalar order
        w = aw*bw - ax*bx - ay*by - az*bz        x = aw*bx + ax*bw + ay*bz - az*by
        y = aw*by + ay*bw + az*bx - ax*bz        z = aw*bz + az*bw + ax*by - ay*bx
     evaluated left to right in float, every product and sum rounded on its own.
  5. `t_V = quaternion` (AngleAxis::operator=(QuaternionBase), Eigen 3.3): n = vec.norm() = sqrtf(x*x + (y*y + z*z)); if n < FLT_EPSILON,
     n = vec.stableNorm() (m = max |component|; 0 when m == 0, else inv = 1 / m — FLT_MAX with m = 1 / FLT_MAX when that quotient
     overflows —, m * sqrtf of the same sum of squares over vec * inv); if n != 0: angle = 2 * atan2f(n, |w|), n = -n if w < 0,
     axis = vec / n (three float divisions); else angle = 0, axis = (1, 0, 0).
  6. (:479) t_V.matrix() = AngleAxis::toRotationMatrix: s = sinf(angle), c = cosf(angle), sin_axis = s * axis, cos1_axis = (1 - c) * axis;
     tmp = cos1_axis.x * axis.y: R01 = tmp - sin_axis.z, R10 = tmp + sin_axis.z; tmp = cos1_axis.x * axis.z: R02 = tmp + sin_axis.y,
     R20 = tmp - sin_axis.y; tmp = cos1_axis.y * axis.z: R12 = tmp - sin_axis.x, R21 = tmp + sin_axis.x; diagonal = cos1_axis * axis + c.
  7. (:454) rotated = R * p: row i gives (R[i][0] * x + R[i][1] * y) + R[i][2] * z in float.
  8. (:455) adjusted = rotated + velocity_ * real_time: a float product and a float sum per coordinate.
  9. (:460-462) intensity, ring and time are copied.

Eigen is not installed next to this repository, so NONE of steps 4-7 could be checked against Eigen itself: they are the reading this
file picks.  Where Eigen builds offer another one: the SSE path of the quaternion product (Eigen/src/Geometry/arch/Geometry_SSE.h)
adds its products in another order than step 4's scalar path; Eigen 3.2's AngleAxis::operator= is `n2 = vec.squaredNorm(); if n2 <
dummy_precision: angle 0, axis (1, 0, 0); else angle = 2 * acosf(min(max(w, -1), 1)), axis = vec / sqrtf(n2)` in place of step 5; and the
3 x 3 product of step 7 may be summed as R[i][0] * x + (R[i][1] * y + R[i][2] * z) by a build that vectorises it.  All of these differ
from the reading here by float rounding of a rotation, i.e. by a few ulp of the coordinate (bounded against a float64 closed form in
tests/test_adjust_cloud.py), except Eigen 3.2's threshold: it returns the identity for |angle| below about 2e-3 rad, where this reading
still rotates.

A float libm function (sinf, cosf, atan2f) is DEFINED as the correctly rounded value (the double function rounded once to float), as
everywhere in this repository; sqrtf and float division are exact by IEEE.

Two forms: `adjust_sequential` is the reference's loop line by line on numpy float32 scalars with its branches as `if`s;
`adjust_vectorised` is the form the HIP kernel implements (one lane per point, every branch a select).  Both return the same dict, and
both count which branch of step 5 every point took (`census`)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
EPS = f32(np.finfo(np.float32).eps)
FLT_MAX = f32(np.finfo(np.float32).max)
SCAN_PERIOD = f32(0.1)                  # distortionAdjust.cpp:246
BRANCHES = ("zero", "stable_norm", "w_negative", "plain")


def _libm(fn, *args):
    """A double libm function, element by element through the C library (as tests/pretreat_ref.py), rounded once to float"""
    arrs = [np.atleast_1d(np.asarray(a, f64)) for a in args]
    return np.fromiter((fn(*v) for v in zip(*[a.tolist() for a in arrs])), f64, count=len(arrs[0])).astype(f32)


def _rates(motion):
    """step 0: (scan_period, velocity[3], angular_rate[3]) as float32"""
    sp, v, w = motion
    return f32(sp), np.asarray(v, f64).astype(f32), np.asarray(w, f64).astype(f32)


def _quat_mul(a, b):
    """step 4's Hamilton product, left to right; works on float32 scalars and arrays alike"""
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return (aw * bw - ax * bx - ay * by - az * bz,
            aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx)


# ---- the reference's loop --------------------------------------------------------------------------------------------------
def _sin(x): return f32(math.sin(float(x)))
def _cos(x): return f32(math.cos(float(x)))


def _axis_quat(angle, axis):
    ha = f32(0.5) * angle
    s = _sin(ha)
    return (_cos(ha), s * f32(axis[0]), s * f32(axis[1]), s * f32(axis[2]))


def _update_matrix(rate, real_time, census):
    """UpdateMatrix (:471-480): the 3 x 3 float matrix as nested tuples"""
    ang = (rate[0] * real_time, rate[1] * real_time, rate[2] * real_time)
    q = _quat_mul(_quat_mul(_axis_quat(ang[2], (0, 0, 1)), _axis_quat(ang[1], (0, 1, 0))), _axis_quat(ang[0], (1, 0, 0)))
    w, x, y, z = q
    n = f32(np.sqrt(x * x + (y * y + z * z)))
    branch = "plain"
    if n < EPS:
        branch = "stable_norm"
        m = max(abs(x), abs(y), abs(z))
        if m > f32(0):
            with np.errstate(over="ignore"):
                inv = f32(1) / m
            if inv > FLT_MAX:
                inv = FLT_MAX
                m = f32(1) / FLT_MAX
            sx, sy, sz = x * inv, y * inv, z * inv
            n = m * f32(np.sqrt(sx * sx + (sy * sy + sz * sz)))
        else:
            n = f32(0)
    if n != f32(0):
        angle = f32(2) * f32(math.atan2(float(n), float(abs(w))))
        if w < f32(0):
            n = -n
            branch = "w_negative" if branch == "plain" else branch
        ax, ay, az = x / n, y / n, z / n
    else:
        branch = "zero"
        angle, ax, ay, az = f32(0), f32(1), f32(0), f32(0)
    census[branch] += 1
    s, c = _sin(angle), _cos(angle)
    sx, sy, sz = s * ax, s * ay, s * az
    k = f32(1) - c
    cx, cy, cz = k * ax, k * ay, k * az
    t01, t02, t12 = cx * ay, cx * az, cy * az
    return ((cx * ax + c, t01 - sz, t02 + sy),
            (t01 + sz, cy * ay + c, t12 - sx),
            (t02 - sy, t12 + sx, cz * az + c))


def adjust_sequential(xyz, time, motion):
    """AdjustCloud (:419-469) one point at a time.  xyz: (n, 3) float32, time: (n,) float32, motion: (scan_period, v[3], w[3])."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    time = np.ascontiguousarray(time, f32).reshape(-1)
    sp, vel, rate = _rates(motion)
    census = dict.fromkeys(BRANCHES, 0)
    out = np.zeros((max(len(xyz) - 1, 0), 3), f32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(1, len(xyz)):
            real_time = f32(f64(time[i]) - f64(sp) / f64(2.0))
            R = _update_matrix(rate, real_time, census)
            x, y, z = xyz[i]
            for r in range(3):
                rotated = (R[r][0] * x + R[r][1] * y) + R[r][2] * z
                out[i - 1, r] = rotated + vel[r] * real_time
    return dict(xyz=out, index=np.arange(1, len(xyz), dtype=np.int64), census=census)


# ---- the kernel's form -----------------------------------------------------------------------------------------------------
def adjust_vectorised(xyz, time, motion):
    """The same arithmetic for all points at once, every branch a select."""
    xyz = np.ascontiguousarray(xyz, f32).reshape(-1, 3)
    time = np.ascontiguousarray(time, f32).reshape(-1)
    sp, vel, rate = _rates(motion)
    p, t = xyz[1:], time[1:]
    one, zero = f32(1), f32(0)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        rt = (t.astype(f64) - f64(sp) / f64(2.0)).astype(f32)
        quats = []
        for k, axis in ((2, (0, 0, 1)), (1, (0, 1, 0)), (0, (1, 0, 0))):
            ha = f32(0.5) * (rate[k] * rt)
            s = _libm(math.sin, ha)
            quats.append((_libm(math.cos, ha), s * f32(axis[0]), s * f32(axis[1]), s * f32(axis[2])))
        w, x, y, z = _quat_mul(_quat_mul(quats[0], quats[1]), quats[2])
        n0 = np.sqrt(x * x + (y * y + z * z))
        small = n0 < EPS
        m0 = np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
        inv = one / m0
        over = inv > FLT_MAX
        inv = np.where(over, FLT_MAX, inv)
        m = np.where(over, one / FLT_MAX, m0)
        sx, sy, sz = x * inv, y * inv, z * inv
        stable = np.where(m0 > zero, m * np.sqrt(sx * sx + (sy * sy + sz * sz)), zero).astype(f32)
        n = np.where(small, stable, n0).astype(f32)
        nz = n != zero
        angle = np.where(nz, f32(2) * _libm(math.atan2, n, np.abs(w)), zero).astype(f32)
        neg = nz & (w < zero)
        n = np.where(neg, -n, n)
        ax = np.where(nz, x / n, one).astype(f32)
        ay = np.where(nz, y / n, zero).astype(f32)
        az = np.where(nz, z / n, zero).astype(f32)
        s, c = _libm(math.sin, angle), _libm(math.cos, angle)
        sx, sy, sz = s * ax, s * ay, s * az
        k1 = one - c
        cx, cy, cz = k1 * ax, k1 * ay, k1 * az
        t01, t02, t12 = cx * ay, cx * az, cy * az
        R = ((cx * ax + c, t01 - sz, t02 + sy), (t01 + sz, cy * ay + c, t12 - sx), (t02 - sy, t12 + sx, cz * az + c))
        out = np.zeros((len(p), 3), f32)
        for r in range(3):
            out[:, r] = ((R[r][0] * p[:, 0] + R[r][1] * p[:, 1]) + R[r][2] * p[:, 2]) + vel[r] * rt
    census = dict(zero=int((~nz).sum()), stable_norm=int((small & nz).sum()), w_negative=int((neg & ~small).sum()),
                  plain=int((nz & ~small & ~neg).sum()))
    return dict(xyz=out, index=np.arange(1, len(xyz), dtype=np.int64), census=census)


def adjust_structs(cloud, motion, form=adjust_vectorised):
    """The restatement on a PointXYZIRT struct array (lisreg.synth.XYZIRT_DTYPE): the adjusted struct array."""
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(f32) if len(cloud) else np.zeros((0, 3), f32)
    res = form(xyz, cloud["time"], motion)
    out = cloud[1:].copy()
    out["x"], out["y"], out["z"] = res["xyz"][:, 0], res["xyz"][:, 1], res["xyz"][:, 2]
    return out


def closed_form(xyz, time, motion):
    """Independent float64 closed form: Rz(wz t) Ry(wy t) Rx(wx t) p + v t with t = time - scan_period / 2, from the float32 rates."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3).astype(f64)[1:]
    sp, vel, rate = _rates(motion)
    t = np.asarray(time, f32).astype(f64)[1:] - f64(sp) / 2.0
    a, b, g = rate[0].astype(f64) * t, rate[1].astype(f64) * t, rate[2].astype(f64) * t
    ca, sa, cb, sb, cg, sg = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(g), np.sin(g)
    R = np.empty((len(t), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sb, cb * sa, cb * ca
    return np.einsum("nij,nj->ni", R, xyz) + vel.astype(f64)[None, :] * t[:, None]


def same(a, b):
    """bit-for-bit equality of two results' coordinates and equal censuses"""
    return (a["xyz"].shape == b["xyz"].shape and np.array_equal(a["xyz"].view(np.uint32), b["xyz"].view(np.uint32))
            and a["census"] == b["census"])


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------
def make_points(seed, n, max_range=70.0, scan_period=0.1):
    """n seeded points up to max_range with times in [0, scan_period): ((n, 3) float32, (n,) float32, intensity, ring)"""
    rng = np.random.default_rng(seed)
    r = rng.uniform(1.0, max_range, n)
    az, el = rng.uniform(-np.pi, np.pi, n), np.radians(rng.uniform(-25.0, 15.0, n))
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(f32)
    time = np.sort(rng.uniform(0.0, scan_period, n)).astype(f32)
    return xyz, time, rng.uniform(0, 1, n).astype(f32), rng.integers(0, 64, n).astype(np.uint16)


# name -> (scan_period, linear velocity, angular velocity); the first four are the golden file's motions
MOTIONS = {
    "drive":      (0.1, (12.5, -0.8, 0.15), (0.02, -0.015, 0.45)),          # a turn at speed
    "all_axes":   (0.1, (-3.0, 4.0, 1.0), (1.3, -0.9, 1.7)),                # rates about all three axes at once
    "zero":       (0.1, (7.0, -2.0, 0.5), (0.0, 0.0, 0.0)),                 # n == 0: identity rotation, p + v * real_time
    "tiny_rate":  (0.1, (0.0, 0.0, 0.0), (0.0, 0.0, 1e-6)),                 # n < epsilon: stableNorm
    "fast_yaw":   (0.1, (1.0, 2.0, 3.0), (0.0, 0.0, 100.0)),                # w < 0: cos(2.5) < 0 at real_time = 0.05
}
GOLDEN_MOTIONS = ("drive", "all_axes", "zero", "tiny_rate")
GOLDEN_SEED, GOLDEN_N = 20260, 500


def golden_arrays():
    """what tests/golden/adjust_cloud.npz holds, regenerated: the sweep, the four motions and the restatement's outputs"""
    xyz, time, inten, ring = make_points(GOLDEN_SEED, GOLDEN_N)
    d = dict(xyz=xyz, time=time, intensity=inten, ring=ring,
             motions=np.array([[MOTIONS[k][0], *MOTIONS[k][1], *MOTIONS[k][2]] for k in GOLDEN_MOTIONS], f64))
    for k in GOLDEN_MOTIONS:
        d["out_" + k] = adjust_vectorised(xyz, time, MOTIONS[k])["xyz"]
    return d
