"""numpy restatement of the reference's global-map assembly — publishGlobalMap (src/node/subMapOptmizationNode.cpp:3553-3574) and the PCD
export (:3502-3514): walk the listed submaps in order, transformPointCloud each of the five class clouds (dynamic, pole, ground, building,
outlier) by the submap's pose, concatenate.  TEST INFRASTRUCTURE ONLY.

A class cloud is an (n, 4) float32 array of 16-byte records: x, y, z and the payload word (the label), which is carried as uint32 bits.
The matrix comes from oracle/lisreg_numpy.py; every coordinate is ((m0 x + m1 y) + m2 z) + m3 in float32 with each product and sum
rounded on its own (numpy rounds every float32 operation; there is no fused multiply-add here).

About the poses the tests use: numpy's float32 sin / cos are not libm's sinf / cosf (they differ in the last bit on roughly one argument in
seven), and lisreg_numpy.pose_to_matrix associates A * D * F as (A * D) * F where the C code forms A * (D * F).  A bit-for-bit comparison
of clouds is therefore only meaningful for poses on which the two formulations of the matrix agree bit for bit, so agreed_poses() draws
angle triples until lisreg_numpy and the C oracle (orc_pose_to_matrix, libm) give the same twelve floats.  The choice looks at the two
references only, never at the code under test; about one triple in five is kept, over the whole +-pi range.  Translations are copied
into the matrix as they are and are not restricted."""
import ctypes as C

import numpy as np

import lisreg_numpy as LN

f32 = np.float32
RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("w", "<u4")])     # one 16-byte record, for the oracle's strided loops
CLASSES = 5


def transform_records(rec, M):
    """rec (n, 4) float32, M (3, 4) float32 -> the moved records; the payload word is copied as bits"""
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    M = np.asarray(M, f32)
    out = np.empty_like(rec)
    x, y, z = rec[:, 0], rec[:, 1], rec[:, 2]
    with np.errstate(all="ignore"):
        for r in range(3):
            out[:, r] = ((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3]
    out.view(np.uint32)[:, 3] = rec.view(np.uint32)[:, 3]
    return out


def global_map(store, map_ids, poses, class_mask=31):
    """store: {map id: [five (n, 4) float32 class arrays]}; poses: [len(map_ids), 6] {roll, pitch, yaw, x, y, z}, or None for no
    arithmetic at all.  Returns (cloud (N, 4) float32, int64 segment starts [len(map_ids) * 5 + 1]): segment 5 * i + k is class k of
    map_ids[i] under poses[i]; a masked-out or empty class is an empty segment (:3560-3571)."""
    parts, off, total = [], [], 0
    for i, mid in enumerate(map_ids):
        M = None if poses is None else LN.pose_to_matrix(np.asarray(poses[i], f32))
        for k in range(CLASSES):
            off.append(total)
            if not (class_mask >> k) & 1:
                continue
            rec = np.ascontiguousarray(store[mid][k], f32).reshape(-1, 4)
            parts.append(rec.copy() if M is None else transform_records(rec, M))
            total += len(rec)
    off.append(total)
    cloud = np.concatenate(parts) if parts else np.zeros((0, 4), f32)
    return np.ascontiguousarray(cloud, f32).reshape(-1, 4), np.asarray(off, np.int64)


def to_xyzil(cloud):
    """the (N, 4) records as 32-byte PointXYZIL structs the way lisreg_submap_gather writes them: x, y, z, the low 16 bits of the payload
    as the uint16 label at byte 20, zeros everywhere else (the store has no intensity).  Returned as (N, 8) uint32 words."""
    c = np.ascontiguousarray(cloud, f32).reshape(-1, 4).view(np.uint32)
    out = np.zeros((len(c), 8), np.uint32)
    out[:, :3] = c[:, :3]
    out[:, 5] = c[:, 3] & 0xFFFF
    return out


def same_bits(a, b):
    """None if the two (N, 4) clouds are equal word for word — where `b` (the restatement) has a NaN coordinate `a` must have a NaN, any
    NaN — else a short description of the first difference"""
    a = np.ascontiguousarray(a, f32).reshape(-1, 4)
    b = np.ascontiguousarray(b, f32).reshape(-1, 4)
    if a.shape != b.shape:
        return "shapes %s / %s" % (a.shape, b.shape)
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    nan = np.isnan(b)
    nan[:, 3] = False                                   # the payload is bits, never a number
    ok = np.where(nan, np.isnan(a), ua == ub)
    if ok.all():
        return None
    r, c = np.argwhere(~ok)[0]
    return "row %d word %d: %08x / %08x (%d words differ)" % (r, c, ua[r, c], ub[r, c], int((~ok).sum()))


def c_matrix(pose):
    """the C oracle's matrix (libm trigonometry) as (3, 4) float32"""
    import oracle_ctypes as oc
    fp = C.POINTER(C.c_float)
    T = np.ascontiguousarray(pose, f32)
    M = np.zeros(12, f32)
    oc.lib().orc_pose_to_matrix(T.ctypes.data_as(fp), M.ctypes.data_as(fp))
    return M.reshape(3, 4)


def agreed_poses(rng, n, max_angle=np.pi, max_trans=500.0):
    """n poses {roll, pitch, yaw, x, y, z} with angles in +-max_angle and translations in +-max_trans whose matrix is the same bits from
    lisreg_numpy and from the C oracle (see the module docstring)"""
    out = []
    while len(out) < n:
        T = np.concatenate([rng.uniform(-max_angle, max_angle, 3), rng.uniform(-max_trans, max_trans, 3)]).astype(f32)
        if np.array_equal(LN.pose_to_matrix(T).view(np.uint32), c_matrix(T).view(np.uint32)):
            out.append(T)
    return np.stack(out) if out else np.zeros((0, 6), f32)


def oracle_transform(rec, pose):
    """oracle_ctypes.transform_cloud (the C oracle's transformPointCloud) on 16-byte records"""
    import oracle_ctypes as oc
    rec = np.ascontiguousarray(rec, f32).reshape(-1, 4)
    if len(rec) == 0:
        return rec.copy()
    out = oc.transform_cloud(rec.view(RECORD).reshape(-1), np.asarray(pose, f32))
    return np.ascontiguousarray(out).view(f32).reshape(-1, 4)


def make_store(rng, counts, spread=60.0):
    """{map id: five (n, 4) float32 class arrays} for counts = {map id: five counts}: coordinates within +-spread, labels 0-19 in the
    payload bits"""
    store = {}
    for mid, cnt in counts.items():
        cls = []
        for n in cnt:
            rec = np.zeros((int(n), 4), f32)
            rec[:, :3] = rng.uniform(-spread, spread, (int(n), 3)).astype(f32)
            rec.view(np.uint32)[:, 3] = rng.integers(0, 20, int(n), dtype=np.uint32)
            cls.append(rec)
        store[mid] = cls
    return store
