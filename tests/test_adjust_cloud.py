"""Constant-velocity motion compensation (lisreg_adjust_cloud, lisreg_adjust_cloud_batch).

The yardstick is tests/adjust_ref.py, the numpy restatement of DistortionAdjust::AdjustCloud / UpdateMatrix: its literal loop and the
form the HIP kernel implements must agree bit for bit on inputs that take every branch, it must stay within float rounding of an
independent float64 closed form, and the golden file must regenerate from it — the CPU tests of this file, with the ABI checks.  The
GPU tests, which hold the library against the restatement bit for bit, are in tests/test_motion_adjust.py and
tests/test_motion_stream.py: this file sorts in front of tests/test_caller_stream.py, whose side-stream cases need to find the process
without a context made before theirs, so it makes none."""
import ctypes as C
import os
import re

import numpy as np
import adjust_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adjust", "adjust_cloud.npz")
NEW_SYMBOLS = ("lisreg_extract_features_deskew_batch", "lisreg_default_motion", "lisreg_adjust_cloud", "lisreg_adjust_cloud_batch")

# max |restatement - float64 closed form| over closed_form_cases(), measured on the CPU: 1.34e-5 m (float rounding of a rotation at
# 70 m: an ulp of 64 m is 7.6e-6 m); the assertion allows four times that, for other seeds
CLOSED_FORM_MEASURED = 1.34e-5
CLOSED_FORM_BOUND = 4 * CLOSED_FORM_MEASURED


def cpu_cases():
    """(name, xyz, time, motion): the golden sweep under its four motions, under the fast yaw, and with every time = scan_period / 2"""
    xyz, time, _, _ = A.make_points(A.GOLDEN_SEED, A.GOLDEN_N)
    out = [(k, xyz, time, A.MOTIONS[k]) for k in A.MOTIONS]
    mid = np.full(len(time), np.float32(np.float32(0.1) / np.float32(2)), np.float32)
    out.append(("real_time_0", xyz, mid, A.MOTIONS["all_axes"]))
    return out


def closed_form_cases():
    """physical motions (rates <= 2 rad/s, speeds <= 30 m/s) on points up to 70 m"""
    rng = np.random.default_rng(77)
    out = []
    for seed in range(8):
        xyz, time, _, _ = A.make_points(300 + seed, 2000)
        out.append((xyz, time, (0.1, tuple(rng.uniform(-30 / np.sqrt(3), 30 / np.sqrt(3), 3)), tuple(rng.uniform(-2 / np.sqrt(3), 2 / np.sqrt(3), 3)))))
    out.append((*A.make_points(310, 2000)[:2], (0.1, (30.0, 0.0, 0.0), (0.0, 0.0, 2.0))))
    out.append((*A.make_points(311, 2000)[:2], (0.1, (0.0, -30.0, 0.0), (2.0, 0.0, 0.0))))
    out.append((*A.make_points(312, 2000)[:2], (0.1, (0.0, 0.0, 30.0), (0.0, -2.0, 0.0))))
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    """ctypes mirror of `typedef struct <name> { ... }` as include/lisreg.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "void*": C.c_void_p, "float*": C.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"(\w+\s*\*?)\s+(.*)", decl).groups()
        for n in names.split(","):
            arr = re.match(r"(\w+)\[(\d+)\]", n.strip())
            ct = types[t.replace(" ", "")]
            fields.append((arr.group(1), ct * int(arr.group(2))) if arr else (n.strip(), ct))
    return type(name, (C.Structure,), {"_fields_": fields})


def test_header_structs_and_symbols():
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for mine, name in ((lisreg.Motion, "lisreg_motion"), (lisreg.AdjustOut, "lisreg_adjust_out")):
        theirs = _header_struct(name)
        assert C.sizeof(mine) == C.sizeof(theirs), name
        assert [(n, getattr(mine, n).offset) for n, _ in mine._fields_] == [(n, getattr(theirs, n).offset) for n, _ in theirs._fields_], name
    assert C.sizeof(lisreg.Motion) == 56 and C.sizeof(lisreg.AdjustOut) == 24
    for sym in NEW_SYMBOLS:
        assert re.search(r"^\s*int\s+%s\s*\(" % sym, hdr, re.M), sym
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym), sym


def test_default_motion_and_null_context():
    import lisreg
    L = lisreg.lib()
    m = lisreg.Motion()
    m.scan_period, m.linear_velocity[1], m.angular_velocity[2] = 7.0, 1.0, 2.0
    assert L.lisreg_default_motion(C.byref(m)) == lisreg.OK
    assert np.float32(m.scan_period).view(np.uint32) == np.float32(0.1).view(np.uint32)
    assert list(m.linear_velocity) == [0.0, 0.0, 0.0] and list(m.angular_velocity) == [0.0, 0.0, 0.0]
    assert L.lisreg_default_motion(None) == lisreg.ERR_ARG
    ao = lisreg.AdjustOut()
    assert L.lisreg_adjust_cloud(None, None, 0, 32, lisreg.FMT_XYZIRT, None, C.byref(m), C.byref(ao)) == lisreg.ERR_ARG
    assert L.lisreg_adjust_cloud_batch(None, 0, None, None, None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_extract_features_deskew_batch(None, 0, None, None, None, None, None) == lisreg.ERR_ARG
    mk = lisreg.make_motion((1, 2, 3), (4, 5, 6))
    assert list(mk.linear_velocity) == [1.0, 2.0, 3.0] and list(mk.angular_velocity) == [4.0, 5.0, 6.0]


def test_sequential_form_equals_vectorised_form_on_every_branch():
    census = dict.fromkeys(A.BRANCHES, 0)
    for name, xyz, time, motion in cpu_cases():
        a, b = A.adjust_sequential(xyz, time, motion), A.adjust_vectorised(xyz, time, motion)
        assert A.same(a, b), name
        assert len(a["xyz"]) == len(xyz) - 1 and np.array_equal(a["index"], np.arange(1, len(xyz)))       # point 0 is gone
        assert sum(a["census"].values()) == len(xyz) - 1
        for k in census:
            census[k] += a["census"][k]
        sp, vel, rate = A._rates(motion)
        rt = (time[1:].astype(np.float64) - np.float64(sp) / 2.0).astype(np.float32)
        if name == "zero":                                                    # n == 0: the identity, p + v * real_time in float exactly
            assert a["census"]["zero"] == len(xyz) - 1
            want = xyz[1:] + vel[None, :] * rt[:, None]
            assert want.dtype == np.float32 and np.array_equal(a["xyz"].view(np.uint32), want.view(np.uint32))
        if name == "real_time_0":                                             # real_time = 0: nothing moves
            assert (rt == 0).all() and a["census"]["zero"] == len(xyz) - 1
            assert np.array_equal(a["xyz"], xyz[1:])
        if name == "tiny_rate":
            assert a["census"]["stable_norm"] > 400
        if name == "fast_yaw":
            assert a["census"]["w_negative"] > 100 and a["census"]["plain"] > 100
    print("census", census)
    assert all(v > 0 for v in census.values()), census                         # every branch of the quaternion -> angle-axis step is taken
    assert len(A.adjust_vectorised(np.zeros((0, 3)), np.zeros(0), A.MOTIONS["drive"])["xyz"]) == 0
    assert len(A.adjust_sequential(np.ones((1, 3)), np.zeros(1), A.MOTIONS["drive"])["xyz"]) == 0


def test_restatement_against_float64_closed_form():
    """max |adjust_ref - Rz(wz t) Ry(wy t) Rx(wx t) p - v t| over the physical cases (rates <= 2 rad/s, speeds <= 30 m/s, points up to
    70 m), measured on the CPU: 1.34e-5 m.  The bound is four times that: the deviation is float rounding of a rotation at 70 m and
    scales with neither rate nor speed; the margin covers other seeds."""
    worst = 0.0
    for xyz, time, motion in closed_form_cases():
        assert np.linalg.norm(xyz, axis=1).max() <= 70.0 and np.linalg.norm(xyz, axis=1).max() > 60.0
        assert np.linalg.norm(motion[1]) <= 30.0 + 1e-9 and np.linalg.norm(motion[2]) <= 2.0 + 1e-9
        got = A.adjust_vectorised(xyz, time, motion)["xyz"].astype(np.float64)
        worst = max(worst, float(np.abs(got - A.closed_form(xyz, time, motion)).max()))
    print("closed form: max deviation %.3e m, bound %.3e m" % (worst, CLOSED_FORM_BOUND))
    assert worst <= CLOSED_FORM_BOUND
    for name in ("fast_yaw", "tiny_rate", "zero"):                             # the branch cases stay a rotation too
        xyz, time, _, _ = A.make_points(A.GOLDEN_SEED, A.GOLDEN_N)
        got = A.adjust_vectorised(xyz, time, A.MOTIONS[name])["xyz"].astype(np.float64)
        assert np.abs(got - A.closed_form(xyz, time, A.MOTIONS[name])).max() <= CLOSED_FORM_BOUND, name


def test_golden_file_regenerates():
    g = np.load(GOLDEN)
    want = A.golden_arrays()
    assert sorted(g.files) == sorted(want)
    assert os.path.getsize(GOLDEN) < 100 * 1024 and len(g["xyz"]) == A.GOLDEN_N and len(g["motions"]) == 4
    for k, v in want.items():
        assert g[k].dtype == v.dtype and g[k].shape == v.shape and g[k].tobytes() == v.tobytes(), k
