"""The (cloud, n, stride, fmt) contract of every entry point that takes one: which arguments are refused, with which return code, and
that a refused call leaves the context as it was.

Every entry point below gets the same ten calls with an unusable or unusual cloud argument; the return code of each is compared with
the literal table EXPECT, and after each of them one valid call on a 4-point cloud (a 4-point target and a 4-point source where both are
needed) must give, byte for byte, what the same valid call gives on a context that never saw a refused call.

EXPECT was recorded from the commit before the argument checks were gathered into lisreg::check_cloud (lisreg_api_ctx.hip): it pins what
the entry points did then, including where they differ from one another — lisreg_set_target, lisreg_voxel_downsample and
lisreg_transform_cloud read any fmt they do not know as XYZI structs, lisreg_keyframes_push does not ask XYZIL structs for the stride
their label needs, lisreg_target_from_classes clamps a negative count to zero, the k = 1 map functions and NDT take XYZIRT structs (they
read x, y, z), the local maps and the key-frame ring do not.  No message text is compared.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, NOT_ENOUGH, ARG = 0, 1, -1
XYZI, XYZIL, DEVICE, XYZIRT, DEVICE_XYZI, PACKED = 0, 1, 2, 3, 4, 5

# four points that span a volume (an NDT voxel of them has a positive-definite covariance); the sources sit a few centimetres off
TGT = np.array([[1.0, 1.0, 1.0], [2.0, 1.5, 1.2], [1.3, 2.2, 1.1], [1.7, 1.9, 2.4]], np.float32)
SRC = TGT + np.array([0.03, -0.02, 0.01], np.float32)


def records(xyz, stride=32, fmt=XYZI):
    """Host structs of `stride` bytes in the layout of `fmt`: x y z in front, then whatever of intensity (byte 16, or 12 for
    XYZI_PACKED), label / ring (byte 20) and time (byte 24) the stride has room for; 64 spare bytes behind the last record."""
    n = len(xyz)
    buf = np.zeros(n * max(stride, 0) + 64, np.uint8)
    for i in range(n):
        def put(off, arr):
            b = np.asarray(arr).tobytes()
            if off + len(b) <= stride:
                buf[i * stride + off:i * stride + off + len(b)] = np.frombuffer(b, np.uint8)
        put(0, xyz[i].astype(np.float32))
        put(12 if fmt == PACKED else 16, np.float32(0.25 * (i + 1)))
        if fmt in (XYZIL, XYZIRT):
            put(20, np.uint16(9 + 31 * i if fmt == XYZIL else i))       # labels 9, 40, 71, 102: & 31 they are 9, 8, 7, 6
        if fmt == XYZIRT:
            put(24, np.float32(0.01 * i))
    return buf


# the calls every entry point gets: (name, n, cloud given?, stride, fmt); fmt None = the format of the entry point's valid call, so that
# the first three are refused (or not) for their count and pointer alone
CASES = (
    ("n < 0",                  -1, True,  32, None),
    ("NULL cloud, n > 0",       4, False, 32, None),
    ("n == 0",                  0, True,  32, None),
    ("unknown fmt",             4, True,  32, 99),
    ("XYZI, stride 11",         4, True,  11, XYZI),
    ("XYZI, stride 19",         4, True,  19, XYZI),        # (one byte short of the intensity, for those who read it)
    ("XYZIL, stride 21",        4, True,  21, XYZIL),
    ("XYZIRT, stride 21",       4, True,  21, XYZIRT),
    ("XYZI_PACKED, stride 15",  4, True,  15, PACKED),
    ("XYZIRT, stride 32",       4, True,  32, XYZIRT),
)

# Return codes of CASES, in that order, as the parent of the commit that introduced lisreg::check_cloud returned them.
EXPECT = {
    # entry point               n<0  NULL n==0 fmt?  I11  I19  L21  R21  P15  R32
    "set_target":             (ARG, ARG, OK,  OK,  ARG, OK,  ARG, OK,  OK,  OK),
    "target_from_classes":    (OK,  OK,  OK,  OK,  ARG, OK,  ARG, OK,  OK,  OK),
    "voxel_downsample":       (ARG, ARG, OK,  OK,  ARG, OK,  ARG, OK,  OK,  OK),
    "transform_cloud":        (ARG, ARG, OK,  OK,  ARG, OK,  OK,  OK,  OK,  OK),
    "extract_features":       (ARG, ARG, OK,  ARG, ARG, ARG, ARG, ARG, ARG, OK),
    "semantic_split":         (ARG, ARG, OK,  ARG, ARG, ARG, ARG, ARG, ARG, ARG),
    "map_index_set":          (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "map_index_set_batch":    (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "nearest":                (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "dynamic_filter":         (ARG, ARG, NOT_ENOUGH, ARG, ARG, NOT_ENOUGH, ARG, NOT_ENOUGH, ARG, NOT_ENOUGH),
    "bbx_filter":             (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "cloud_bounds":           (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "icp_align":              (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "icp_align_batch":        (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "icp_gn_match":           (ARG, ARG, OK,  ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "localmap_insert":        (ARG, ARG, OK,  ARG, ARG, OK,  ARG, ARG, ARG, ARG),
    "submap_insert":          (ARG, ARG, OK,  ARG, ARG, OK,  ARG, ARG, ARG, ARG),
    "keyframes_push":         (ARG, ARG, OK,  ARG, ARG, OK,  OK,  ARG, ARG, ARG),
    "ndt_set_target":         (ARG, ARG, ARG, ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "ndt_derivatives":        (ARG, ARG, ARG, ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "ndt_align":              (ARG, ARG, ARG, ARG, ARG, OK,  ARG, OK,  ARG, OK),
    "upload_cloud":           (ARG, ARG, OK,  ARG, ARG, OK,  ARG, ARG, ARG, ARG),
    "pretreat":               (ARG, ARG, OK,  ARG, ARG, ARG, ARG, ARG, ARG, ARG),
    "rangenet_project":       (ARG, ARG, OK,  ARG, ARG, ARG, ARG, ARG, ARG, ARG),
}

fp = C.POINTER(C.c_float)
dp = C.POINTER(C.c_double)


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def raw(obj):
    return np.frombuffer(bytes(obj), np.uint8).copy()


class Env:
    """One context and what the entry points under test need around their cloud argument."""

    def __init__(self):
        import lisreg
        self.m = lisreg
        self.L = lisreg.lib()
        h = C.c_void_p()
        assert self.L.lisreg_create(0, C.byref(h)) == OK
        self.h = h
        self.tgt = records(TGT)
        self.pose = np.array([0.01, -0.02, 0.03, 0.1, 0.2, -0.1], np.float32)
        self.eye = np.eye(4, dtype=np.float32)
        self.ndt_p = lisreg.ndt_default_params(0, resolution=10.0, min_points_per_voxel=4, max_iters=3)
        self.icp_p = lisreg.icp_default_params(0)
        self.icp_p.max_iters = 3
        self.lm_p = lisreg.localmap_default_params()
        self.dev = lisreg.DeviceArray(np.zeros((8, 4), np.float32))

    def close(self):
        self.dev.free()
        self.L.lisreg_destroy(self.h)

    # what some entry points need set before their valid call
    def map_target(self):
        assert self.L.lisreg_map_index_set(self.h, 1, vp(self.tgt), 4, 32, XYZI) == OK

    def ndt_target(self):
        assert self.L.lisreg_ndt_set_target(self.h, 0, vp(self.tgt), 4, 32, XYZI, C.byref(self.ndt_p), None) == OK

    def nearest_of_src(self, slot):
        idx, sqd = np.full(4, -7, np.int32), np.full(4, -7, np.float32)
        q = records(SRC)
        assert self.L.lisreg_nearest(self.h, slot, vp(q), 4, 32, XYZI, 10.0, vp(idx), vp(sqd)) == OK
        return [idx, sqd]


# Every entry: f(env, cloud, n, stride, fmt) -> (return code, [what the call wrote]).  `cloud` is a numpy byte buffer or None.
def e_set_target(e, cl, n, st, fmt):
    rc = e.L.lisreg_set_target(e.h, vp(cl), n, vp(cl), n, st, fmt)
    dims, geom, pts = np.zeros(5, np.int32), np.zeros(4, np.float32), np.zeros((8, 4), np.float32)
    if rc == OK:
        assert e.L.lisreg_get_target_index(e.h, 0, 1, dims.ctypes.data_as(C.POINTER(C.c_int)), geom.ctypes.data_as(fp), vp(pts), 8, None, 0) == OK
    return rc, [dims, geom, pts]


def e_target_from_classes(e, cl, n, st, fmt):
    rc = e.L.lisreg_target_from_classes(e.h, 0, vp(cl), n, vp(cl), n, None, 0, None, 0, st, fmt)
    dims, pts = np.zeros(5, np.int32), np.zeros((8, 4), np.float32)
    if rc == OK:
        assert e.L.lisreg_get_target_index(e.h, 0, 1, dims.ctypes.data_as(C.POINTER(C.c_int)), None, vp(pts), 8, None, 0) == OK
    return rc, [dims, pts]


def e_voxel_downsample(e, cl, n, st, fmt):
    out, n_out = np.zeros(8 * 32 + 64, np.uint8), C.c_int(-7)
    rc = e.L.lisreg_voxel_downsample(e.h, vp(cl), n, st, fmt, 0.5, vp(out), 8, C.byref(n_out))
    return rc, [out, np.int32(n_out.value)]


def e_transform_cloud(e, cl, n, st, fmt):
    out = np.zeros(8 * 32 + 64, np.uint8)
    rc = e.L.lisreg_transform_cloud(e.h, vp(cl), n, st, fmt, e.pose.ctypes.data_as(fp), vp(out))
    return rc, [out]


def e_extract_features(e, cl, n, st, fmt):
    P = e.m.FeatureParams()
    assert e.L.lisreg_default_feature_params(C.byref(P)) == OK
    P.n_scan, P.horizon_scan, P.downsample_rate = 16, 64, 1
    o = e.m.FeatureOut()
    bufs = [np.zeros(8 * 32 + 64, np.uint8) for _ in range(5)]
    for name, b in zip(("deskewed", "corner", "surface", "corner_sharp", "surface_sharp"), bufs):
        setattr(o, name, b.ctypes.data); setattr(o, "cap_" + name, 8); setattr(o, "n_" + name, -7)
    rc = e.L.lisreg_extract_features(e.h, vp(cl), n, st, fmt, C.byref(P), C.byref(o))
    return rc, bufs + [np.array([o.n_deskewed, o.n_corner, o.n_surface, o.n_corner_sharp, o.n_surface_sharp])]


def e_semantic_split(e, cl, n, st, fmt):
    o = e.m.SemanticOut()
    bufs = [np.zeros(8 * 32 + 64, np.uint8) for _ in range(5)]
    for k in range(5):
        o.cloud[k], o.cap[k], o.n[k] = bufs[k].ctypes.data, 8, -7
    rc = e.L.lisreg_semantic_split(e.h, vp(cl), n, st, fmt, None, C.byref(o))
    return rc, bufs + [np.array(list(o.n))]


def e_map_index_set(e, cl, n, st, fmt):
    rc = e.L.lisreg_map_index_set(e.h, 2, vp(cl), n, st, fmt)
    return rc, (e.nearest_of_src(2) if rc == OK and n > 0 else [])


def e_map_index_set_batch(e, cl, n, st, fmt):
    slots, clouds, counts = (C.c_int * 1)(3), (C.c_void_p * 1)(cl.ctypes.data if cl is not None else None), (C.c_int * 1)(n)
    rc = e.L.lisreg_map_index_set_batch(e.h, 1, slots, clouds, counts, st, fmt)
    return rc, (e.nearest_of_src(3) if rc == OK and n > 0 else [])


def e_nearest(e, cl, n, st, fmt):
    idx, sqd = np.full(8, -7, np.int32), np.full(8, -7, np.float32)
    rc = e.L.lisreg_nearest(e.h, 1, vp(cl), n, st, fmt, 10.0, vp(idx), vp(sqd))
    return rc, [idx, sqd]


def e_dynamic_filter(e, cl, n, st, fmt):
    out, n_out = np.zeros(8 * 32 + 64, np.uint8), C.c_int(-7)
    rc = e.L.lisreg_dynamic_filter(e.h, 1, vp(cl), n, st, fmt, 0.5, 0.1, 1.0, 0.05, vp(out), C.byref(n_out))
    return rc, [out, np.int32(n_out.value)]


def e_bbx_filter(e, cl, n, st, fmt):
    out, n_out = np.zeros(8 * 32 + 64, np.uint8), C.c_int(-7)
    bounds = np.array([0.0, 0.0, 0.0, 1.8, 3.0, 3.0], np.float64)
    rc = e.L.lisreg_bbx_filter(e.h, vp(cl), n, st, fmt, bounds.ctypes.data_as(dp), 0, vp(out), C.byref(n_out))
    return rc, [out, np.int32(n_out.value)]


def e_cloud_bounds(e, cl, n, st, fmt):
    b = np.zeros(6, np.float64)
    rc = e.L.lisreg_cloud_bounds(e.h, vp(cl), n, st, fmt, b.ctypes.data_as(dp))
    return rc, [b]


def e_icp_align(e, cl, n, st, fmt):
    res, out = e.m.IcpResult(), np.zeros(8 * 32 + 64, np.uint8)
    rc = e.L.lisreg_icp_align(e.h, 1, vp(cl), n, st, fmt, C.byref(e.icp_p), None, C.byref(res), vp(out))
    return rc, [raw(res), out]


def e_icp_align_batch(e, cl, n, st, fmt):
    items = (e.m.IcpItem * 1)()
    items[0].source, items[0].n, items[0].slot, items[0].guess = (cl.ctypes.data if cl is not None else None), n, 1, None
    res = (e.m.IcpResult * 1)()
    rc = e.L.lisreg_icp_align_batch(e.h, items, 1, st, fmt, C.byref(e.icp_p), 0, res)
    return rc, [raw(res)]


def e_icp_gn_match(e, cl, n, st, fmt):
    res, out = e.m.IcpGnResult(), np.zeros(8 * 32 + 64, np.uint8)
    rc = e.L.lisreg_icp_gn_match(e.h, 1, vp(cl), n, st, fmt, 3, 4.0, e.eye.ctypes.data_as(fp), C.byref(res), vp(out))
    return rc, [raw(res), out]


def _class_clouds(cl, n):
    p = cl.ctypes.data if cl is not None else None
    return (C.c_void_p * 5)(p, p, p, p, p), (C.c_int * 5)(n, n, n, n, n)


def e_localmap_insert(e, cl, n, st, fmt):
    assert e.L.lisreg_localmap_reset(e.h, 0) == OK
    clouds, counts = _class_clouds(cl, n)
    info = e.m.LocalMapInfo()
    rc = e.L.lisreg_localmap_insert(e.h, 0, clouds, counts, st, fmt, e.pose.ctypes.data_as(fp), C.byref(e.lm_p), C.byref(info))
    return rc, [raw(info)]


def e_submap_insert(e, cl, n, st, fmt):
    assert e.L.lisreg_localmap_reset(e.h, 1) == OK
    clouds, counts = _class_clouds(cl, n)
    info = e.m.SubmapInfo()
    rc = e.L.lisreg_submap_insert(e.h, 1, clouds, counts, st, fmt, e.pose.ctypes.data_as(fp), e.pose.ctypes.data_as(fp), C.byref(e.lm_p), C.byref(info))
    return rc, [raw(info)]


def e_keyframes_push(e, cl, n, st, fmt):
    assert e.L.lisreg_keyframes_reset(e.h, 0) == OK
    info = e.m.KeyframesInfo()
    rc = e.L.lisreg_keyframes_push(e.h, 0, vp(cl), n, vp(cl), n, st, fmt, e.pose.ctypes.data_as(fp), 19, C.byref(info))
    if rc == OK:
        assert e.L.lisreg_keyframes_target(e.h, 0, 0.4, 0.8, -1, C.byref(info)) == OK
    return rc, [raw(info)]


def e_ndt_set_target(e, cl, n, st, fmt):
    info = e.m.NdtInfo()
    rc = e.L.lisreg_ndt_set_target(e.h, 1, vp(cl), n, st, fmt, C.byref(e.ndt_p), C.byref(info))
    return rc, [raw(info)]


def e_ndt_derivatives(e, cl, n, st, fmt):
    p, out, pairs = np.zeros(6, np.float64), np.zeros(28, np.float64), C.c_longlong(-7)
    rc = e.L.lisreg_ndt_derivatives(e.h, 0, vp(cl), n, st, fmt, C.byref(e.ndt_p), p.ctypes.data_as(dp), 1, out.ctypes.data_as(dp), C.byref(pairs))
    return rc, [out, np.int64(pairs.value)]


def e_ndt_align(e, cl, n, st, fmt):
    res, out = e.m.NdtResult(), np.zeros(8 * 32 + 64, np.uint8)
    rc = e.L.lisreg_ndt_align(e.h, 0, vp(cl), n, st, fmt, C.byref(e.ndt_p), e.eye.ctypes.data_as(fp), C.byref(res), vp(out))
    return rc, [raw(res), out]


def e_upload_cloud(e, cl, n, st, fmt):
    rc = e.L.lisreg_upload_cloud(e.h, vp(cl), n, st, fmt, C.c_void_p(e.dev.ptr))
    return rc, [e.dev.download(4)]


def e_pretreat(e, cl, n, st, fmt):
    P = e.m.PretreatParams()
    assert e.L.lisreg_default_pretreat_params(C.byref(P)) == OK
    P.n_scan = 16
    o, buf = e.m.PretreatOut(), np.zeros(8 * 32 + 64, np.uint8)
    o.cloud, o.capacity, o.n = buf.ctypes.data, 8, -7
    rc = e.L.lisreg_pretreat(e.h, vp(cl), n, st, fmt, C.byref(P), C.byref(o))
    return rc, [buf, np.array([o.n, o.half_index]), np.array([o.start_ori, o.end_ori], np.float32)]


def e_rangenet_project(e, cl, n, st, fmt):
    P = e.m.RangenetParams()
    assert e.L.lisreg_default_rangenet_params(C.byref(P)) == OK
    P.img_h, P.img_w = 4, 16
    D = e.m.DeviceArray
    tensor, mask, pix = D(np.zeros((5 * 64, 1), np.float32)), D(np.zeros((16, 1), np.float32)), D(np.zeros((8, 1), np.float32))
    o = e.m.RangenetOut()
    o.tensor, o.invalid_mask, o.pixel_index, o.n_valid = tensor.ptr, mask.ptr, pix.ptr, -7
    rc = e.L.lisreg_rangenet_project(e.h, vp(cl), n, st, fmt, C.byref(P), C.byref(o))
    got = [tensor.download(5 * 64), mask.download(16), pix.download(4), np.int32(o.n_valid)]
    for d in (tensor, mask, pix):
        d.free()
    return rc, got


# entry point -> (the call, the valid call's fmt, what to set on a context before the valid call can run)
ENTRIES = {
    "set_target": (e_set_target, XYZI, None),
    "target_from_classes": (e_target_from_classes, XYZI, None),
    "voxel_downsample": (e_voxel_downsample, XYZI, None),
    "transform_cloud": (e_transform_cloud, XYZI, None),
    "extract_features": (e_extract_features, XYZIRT, None),
    "semantic_split": (e_semantic_split, XYZIL, None),
    "map_index_set": (e_map_index_set, XYZI, None),
    "map_index_set_batch": (e_map_index_set_batch, XYZI, None),
    "nearest": (e_nearest, XYZI, Env.map_target),
    "dynamic_filter": (e_dynamic_filter, XYZI, Env.map_target),
    "bbx_filter": (e_bbx_filter, XYZI, None),
    "cloud_bounds": (e_cloud_bounds, XYZI, None),
    "icp_align": (e_icp_align, XYZI, Env.map_target),
    "icp_align_batch": (e_icp_align_batch, XYZI, Env.map_target),
    "icp_gn_match": (e_icp_gn_match, XYZI, Env.map_target),
    "localmap_insert": (e_localmap_insert, XYZIL, None),
    "submap_insert": (e_submap_insert, XYZIL, None),
    "keyframes_push": (e_keyframes_push, XYZI, None),
    "ndt_set_target": (e_ndt_set_target, XYZI, None),
    "ndt_derivatives": (e_ndt_derivatives, XYZI, Env.ndt_target),
    "ndt_align": (e_ndt_align, XYZI, Env.ndt_target),
    "upload_cloud": (e_upload_cloud, XYZIL, None),
    "pretreat": (e_pretreat, XYZI, None),
    "rangenet_project": (e_rangenet_project, XYZI, None),
}
# the clouds of the valid calls: the target where the entry point makes one, the source where it reads one against a target
VALID_XYZ = {name: (SRC if ENTRIES[name][2] is not None else TGT) for name in ENTRIES}


def test_the_table_names_every_entry_point_and_case():
    assert set(EXPECT) == set(ENTRIES)
    assert all(len(row) == len(CASES) for row in EXPECT.values())


def observe(name):
    """The return codes of CASES on one context, and after each case the valid call's (return code, outputs)."""
    call, vfmt, setup = ENTRIES[name]
    valid_cloud = records(VALID_XYZ[name], 32, vfmt)
    e = Env()
    try:
        if setup:
            setup(e)
        codes, after = [], []
        for _, n, given, stride, fmt in CASES:
            fmt = vfmt if fmt is None else fmt
            cloud = records(TGT, stride, fmt) if given else None
            codes.append(call(e, cloud, n, stride, fmt)[0])
            after.append(call(e, valid_cloud, 4, 32, vfmt))
        return codes, after
    finally:
        e.close()


def reference(name):
    """The valid call on a context that saw nothing else."""
    call, vfmt, setup = ENTRIES[name]
    e = Env()
    try:
        if setup:
            setup(e)
        return call(e, records(VALID_XYZ[name], 32, vfmt), 4, 32, vfmt)
    finally:
        e.close()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_cloud_arguments(name):
    ref_rc, ref_out = reference(name)
    assert ref_rc in (OK, NOT_ENOUGH), (name, ref_rc)            # (lisreg_dynamic_filter leaves a cloud of ten points or fewer alone: 1)
    codes, after = observe(name)
    print(name, "return codes:", dict(zip((c[0] for c in CASES), codes)))
    assert tuple(codes) == EXPECT[name], (name, dict(zip((c[0] for c in CASES), zip(codes, EXPECT[name]))))
    for (case, *_), (rc, out) in zip(CASES, after):
        assert rc == ref_rc, (name, case, rc)
        assert len(out) == len(ref_out)
        for k, (a, b) in enumerate(zip(out, ref_out)):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (name, "after", case, "output", k)
