"""CPU restatement of EPSCGeneration::loopDetection with FEPSC (src/core/epscGeneration.cpp:84-120, 258-401, 478-607, 633-660,
663-992) in numpy, with the float32 / float64 types of the reference's x86 build.  The 2-D ICP is the oracle's
pcl::IterativeClosestPoint restatement (oracle_ctypes.icp_align) with PCL's defaults.  One deliberate deviation, shared with the
library: globalICP's shifted column is wrapped modulo 360 (the reference wraps once and reads past its row).

Clouds are (corner, surf, semantic) arrays of PCL structs (fields x, y, z and, for semantic, label)."""
import ctypes
import ctypes.util
import math

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float


def atan2f(y, x):
    """the C library's atan2f, which pcl::getTranslationAndEulerAngles calls on floats (numpy's float32 arctan2 may differ by an ulp)."""
    return np.float32(_libm.atan2f(float(y), float(x)))


RINGS, SECTORS, CELLS, PROJ = 20, 80, 1600, 360
MAX_DIS, MIN_DIS = 60.0, 3.0
RING_STEP = (MAX_DIS - MIN_DIS) / RINGS
SECTOR_STEP = 2 * math.pi / SECTORS
STEP360 = np.float32(2.0 * math.pi / 360.0)
PROJ_LABELS = (13, 14, 16, 18, 19)
USING_LABEL = {1: 10, 2: 10, 3: 10, 4: 10, 5: 10, 6: 10, 7: 10, 8: 10, 9: 40, 10: 40, 11: 40, 12: 70, 13: 50, 14: 50, 15: 70,
               16: 81, 17: 70, 18: 81, 19: 81}     # config/label.yaml using_label; a std::map: anything else maps to 0
NO_SHIFT = -2 ** 31
F32 = np.float32


def _xyz(cloud):
    return (np.asarray(cloud["x"], F32), np.asarray(cloud["y"], F32), np.asarray(cloud["z"], F32))


def apply_matrix(M, x, y, z):
    """mat4_apply: ((m0 x + m1 y) + m2 z) + m3 in float32, no contraction."""
    M = np.asarray(M, F32).reshape(-1)
    return tuple(((M[4 * r] * x + M[4 * r + 1] * y) + M[4 * r + 2] * z) + M[4 * r + 3] for r in range(3))


def _moved(cloud, M):
    x, y, z = _xyz(cloud)
    return (x, y, z) if M is None else apply_matrix(M, x, y, z)


def bins(x, y):
    """ring, sector (int64, -1 where the point is skipped) as calculateEPSC forms them."""
    with np.errstate(invalid="ignore"):
        d = np.sqrt(x * x + y * y).astype(np.float64)
        ok = (d < MAX_DIS) & (d >= MIN_DIS)
        ring = np.floor((d - MIN_DIS) / RING_STEP)
        ang = math.pi + np.arctan2(y, x).astype(np.float64)
        sec = np.floor(ang / SECTOR_STEP)
    ok &= (ring >= 0) & (ring < RINGS) & (sec >= 0) & (sec < SECTORS)
    return np.where(ok, ring, -1).astype(np.int64), np.where(ok, sec, -1).astype(np.int64)


def _count(ring, sec, mask=None):
    ok = ring >= 0 if mask is None else (ring >= 0) & mask
    h = np.zeros(CELLS, np.int64)
    np.add.at(h, ring[ok] * SECTORS + sec[ok], 1)
    return (h & 255).astype(np.int64)          # uchar ++ wraps


def _ratio(psc, esc):
    return ((100 * psc) // (1 + esc) & 255).astype(np.uint8)       # int division, stored to uchar


_LABEL_TAB = np.array([USING_LABEL.get(v, 0) for v in range(65536)], np.int64)     # uint16 labels


def label_map(labels):
    return _LABEL_TAB[np.asarray(labels, np.int64)]


def descriptors(corner, surf, semantic, M=None):
    """calculateEPSC / calculateSEPSC / calculateFEPSC of the three clouds moved by M (None: as they are): uint8 [20, 80] each."""
    rc, sc = bins(*_moved(corner, M)[:2])
    rs, ss = bins(*_moved(surf, M)[:2])
    epsc = _ratio(_count(rs, ss), _count(rc, sc))
    x, y, _ = _moved(semantic, M)
    r, s = bins(x, y)
    m = label_map(semantic["label"]) if len(semantic) else np.zeros(0, np.int64)
    sepsc = _ratio(_count(r, s, (m == 40) | (m == 50)), _count(r, s, m == 81))
    fepsc = (sepsc.astype(np.float64) * 0.4 + epsc.astype(np.float64) * 0.6).astype(np.uint8)
    return fepsc.reshape(RINGS, SECTORS), epsc.reshape(RINGS, SECTORS), sepsc.reshape(RINGS, SECTORS)


def project(semantic, M=None):
    """project(): float32 [360, 4] of (count, x, y, label) of the last point (input order) of labels {13, 14, 16, 18, 19}."""
    out = np.zeros((PROJ, 4), F32)
    if len(semantic) == 0:
        return out
    x, y, _ = _moved(semantic, M)
    lab = np.asarray(semantic["label"], np.int64)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt(x * x + y * y)
        ang = (math.pi + np.arctan2(y, x).astype(np.float64)).astype(F32)
        sec = np.floor(ang / STEP360)
    ok = np.isin(lab, PROJ_LABELS) & ~(dist.astype(np.float64) < 1e-2) & (dist == dist) & (sec >= 0) & (sec < PROJ)
    idx = np.nonzero(ok)[0]
    s = sec[idx].astype(np.int64)
    np.add.at(out[:, 0], s, F32(1))
    last = np.full(PROJ, -1, np.int64)
    np.maximum.at(last, s, idx)
    hit = last >= 0
    out[hit, 1], out[hit, 2], out[hit, 3] = x[last[hit]], y[last[hit]], lab[last[hit]].astype(F32)
    return out


def wrap_yaw(yaw_diff):
    """globalICP :262-265: float wrapped through double once each way; tmp_id = floor(angle / step)."""
    a = F32(yaw_diff)
    if float(a) >= 2.0 * math.pi:
        a = F32(float(a) - 2.0 * math.pi)
    if a < 0:
        a = F32(float(a) + 2.0 * math.pi)
    return a, int(np.floor(a / STEP360))


def yaw_search(hist_proj, cur_proj, yaw_diff):
    """(shift or NO_SHIFT, float32 angle = shift * step or wrapped yaw * step) of the 60-shift count search, modulo-360 columns."""
    a, tmp_id = wrap_yaw(yaw_diff)
    c1, c2 = hist_proj[:, 0], cur_proj[:, 0]
    sim, angle, shift = 100000.0, a, NO_SHIFT
    j = np.arange(PROJ)
    for i in range(tmp_id - 30, tmp_id + 30):
        dc = F32(np.abs(c1 - c2[(j + i) % PROJ]).astype(np.float64).sum())     # exact: small integers
        if float(dc) < sim:
            sim, angle, shift = float(dc), F32(i), i
    return shift, F32(angle * STEP360)


def rot_z(angle):
    """Eigen AngleAxisf(angle, UnitZ()).toRotationMatrix() as a 4 x 4 float32."""
    c, s = F32(np.cos(F32(angle))), F32(np.sin(F32(angle)))
    R = np.eye(4, dtype=F32)
    R[0, 0], R[0, 1], R[1, 0], R[1, 1], R[2, 2] = c, -s, s, c, (F32(1) - c) + c
    return R


def mat_mul(A, B):
    """float32 4 x 4 product with ((a0 b0 + a1 b1) + a2 b2) + a3 b3 per entry."""
    A, B = np.asarray(A, F32), np.asarray(B, F32)
    C = np.zeros((4, 4), F32)
    for r in range(4):
        for c in range(4):
            C[r, c] = ((A[r, 0] * B[0, c] + A[r, 1] * B[1, c]) + A[r, 2] * B[2, c]) + A[r, 3] * B[3, c]
    return C


def global_icp(hist_proj, cur_proj, yaw_diff, oracle):
    """globalICP: dict(shift, angle, T = trans * trans1, state, iters, n_corr)."""
    shift, angle = yaw_search(hist_proj, cur_proj, yaw_diff)
    from lisreg import synth
    c, s = F32(np.cos(angle)), F32(np.sin(angle))
    h = hist_proj[hist_proj[:, 3] > 0]
    k = cur_proj[cur_proj[:, 3] > 0]
    tgt = np.stack([h[:, 1], h[:, 2], np.zeros(len(h), F32)], 1)
    src = np.stack([k[:, 1] * c - k[:, 2] * s, k[:, 1] * s + k[:, 2] * c, np.zeros(len(k), F32)], 1).astype(F32)
    p = oracle.icp_default_params(0)
    p.max_corr_dist, p.max_iters, p.transformation_epsilon, p.euclidean_fitness_epsilon = math.sqrt(np.finfo(np.float64).max), 10, 0.0, \
        -np.finfo(np.float64).max
    if len(tgt) == 0 or len(src) == 0:
        r = dict(T=np.eye(4, dtype=F32), state=5, iters=0, n_corr_last=0)
    else:
        r = oracle.icp_align(synth.to_pcl(tgt), synth.to_pcl(src), p)
    R1 = rot_z(angle)
    T = np.eye(4, dtype=F32)
    T[:3, :3] = mat_mul(np.vstack([r["T"][:3], [0, 0, 0, 1]]), R1)[:3, :3]
    T[:3, 3] = r["T"][:3, 3]
    return dict(shift=shift, angle=angle, T=T, state=r["state"], iters=r["iters"], n_corr=r["n_corr_last"])


def distance(desc1, desc2):
    """calculateDistance: (score = 1 - min difference, shift of the first strict minimum)."""
    d1, d2 = desc1.astype(np.int64), desc2.astype(np.int64)
    diff, best_shift = 1.0, 0
    for i in range(-10, 10):
        cols = (np.arange(SECTORS) + i) % SECTORS
        t = float(np.abs(d1 - d2[:, cols]).sum()) / (SECTORS * RINGS * 255)
        if t < diff:
            diff, best_shift = t, i
    return 1 - diff, best_shift


def matched_transform(T):
    """:860-870 — translation (x, y, 0) of T, rotation about z by atan2(T10, T00)."""
    yaw = atan2f(T[1, 0], T[0, 0])
    M = rot_z(yaw)
    M[0, 3], M[1, 3] = T[0, 3], T[1, 3]
    return M


class EPSCGeneration:
    """loopDetection with UsingFEPSCFlag; params: (skip_neighbour_distance, inflation_covariance, distance_threshold)."""

    def __init__(self, oracle, params=(20.0, 0.01, 0.75)):
        self.oracle = oracle
        self.skip, self.infl, self.thr = params
        self.pos, self.yaw, self.travel, self.proj, self.fepsc = [], [], [], [], []

    @staticmethod
    def pose(odom):
        o = np.asarray(odom, F32).reshape(-1, 4)
        return F32(o[0, 3]), F32(o[1, 3]), atan2f(o[1, 0], o[0, 0])

    def gate(self, x_t, y_t):
        """push the travel distance, return the gated history ids (measured against the previous key frame)."""
        if not self.travel:
            self.travel.append(0.0)
        else:
            px, py = self.pos[-1]
            dx, dy = px - float(x_t), py - float(y_t)
            self.travel.append(self.travel[-1] + math.sqrt(dx * dx + dy * dy + 0.0))
        out = []
        for i, (hx, hy) in enumerate(self.pos):
            delta = self.travel[-1] - self.travel[i]
            ex, ey = hx - self.pos[-1][0], hy - self.pos[-1][1]
            if delta > self.skip and math.sqrt(ex * ex + ey * ey + 0.0) < delta * self.infl:
                out.append(i)
        return out

    def loop_detection(self, corner, surf, semantic, odom):
        """returns dict(current_frame_id, matched_frame_id, matched_transform, score, candidates=[...])."""
        x_t, y_t, yaw_t = self.pose(odom)
        cur_proj = project(semantic)
        cands = []
        best, best_id, best_T = 0.0, -1, np.eye(4, dtype=F32)
        current = len(self.pos)
        for i in self.gate(x_t, y_t):
            g = global_icp(self.proj[i], cur_proj, F32(yaw_t - self.yaw[i]), self.oracle)
            f, _, _ = descriptors(corner, surf, semantic, g["T"])
            score, sshift = distance(self.fepsc[i], f)
            g.update(history_id=i, score=score, score_shift=sshift)
            cands.append(g)
            if score > self.thr and score > best:
                best, best_id, best_T = score, i, matched_transform(g["T"])
        self.pos.append((float(x_t), float(y_t)))
        self.yaw.append(yaw_t)
        self.proj.append(cur_proj)
        self.fepsc.append(descriptors(corner, surf, semantic)[0])
        return dict(current_frame_id=current, matched_frame_id=best_id, matched_transform=best_T, score=best, candidates=cands)
