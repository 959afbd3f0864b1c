"""CPU restatement of the other six loopDetection selectors (src/core/epscGeneration.cpp:403-476, 564-589, 611-660, 663-992) on top
of loopdet_ref: calculateSC / calculateISC / calculateSSC, calculateLabelSim, the per-kind angles and transforms and the matched list
in push order.  Types are those of the reference's x86 build: SC's CV_16S matrix is read and written with at<char> / at<unsigned
char> (a 20 x 80 byte matrix), float-to-int conversions of NaN or out-of-range values give INT_MIN.  One deliberate deviation, shared
with the library: SSC labels >= 20 (past order_vec) count as order 0."""
import math

import numpy as np

import loopdet_ref as R

ISC, SC, EPSC, SEPSC, FEPSC, SSC, POSE = range(7)          # kind index = bit position of LISREG_LOOP_*
NAMES = ("isc", "sc", "epsc", "sepsc", "fepsc", "ssc", "pose")
ALL = 127
INT_MIN = -2 ** 31
LABEL_THRESHOLD = 0.79
ORDER = np.zeros(65536, np.int64)
ORDER[:20] = [0, 0, 0, 0, 0, 0, 0, 0, 0, 10, 11, 12, 13, 15, 16, 14, 17, 9, 18, 19]     # order_vec (epscGeneration.h:24-25)


def x86_int(t):
    """cvttsd2si / cvttss2si of an array: truncation toward zero, INT_MIN for NaN and out-of-range values."""
    t = np.asarray(t)
    with np.errstate(invalid="ignore"):
        ok = (t > -2147483649.0) & (t < 2147483648.0)
        return np.where(ok, np.trunc(np.where(ok, t, 0)), INT_MIN).astype(np.int64)


def sc_values(z):
    """z_temp = (int)(100.0 * (z + LIDAR_HEIGHT) / 8.0), in double."""
    return x86_int(100.0 * (np.asarray(z, np.float32).astype(np.float64) + 5.0) / 8.0)


def isc_values(intensity):
    """intensity_temp = (int)(255 * intensity), a float product."""
    with np.errstate(invalid="ignore", over="ignore"):
        return x86_int(np.float32(255) * np.asarray(intensity, np.float32))


def _cells(cloud, M):
    x, y, z = R._moved(cloud, M)
    ring, sec = R.bins(x, y)
    return np.where(ring >= 0, ring * R.SECTORS + sec, -1), z


def fold_sequential(cells, values, signed):
    """the reference's loop: `if (cell < v) cell = v` with the cell a signed char (SC) or an unsigned char (ISC)."""
    out = np.zeros(R.CELLS, np.int64)
    for c, v in zip(cells, values):
        if c < 0:
            continue
        cur = out[c]
        if cur < v:
            b = int(v) & 255
            out[c] = b - 256 if signed and b >= 128 else b
    return (out & 255).astype(np.uint8)


def fold_indexed(cells, values, signed):
    """the same fold, index-ordered (the device's form): the last resetting value (SC v >= 128, ISC v >= 256), read back as a
    signed / unsigned byte, or 0; then the maximum of it and every in-range value after it (SC -128 .. 127, ISC 0 .. 255)."""
    cells = np.asarray(cells, np.int64)
    values = np.asarray(values, np.int64)
    lo, hi = (-128, 127) if signed else (0, 255)
    idx = np.arange(len(cells))
    ok = cells >= 0
    last = np.full(R.CELLS, -1, np.int64)
    rs = ok & (values > hi)
    np.maximum.at(last, cells[rs], idx[rs])
    start = np.zeros(R.CELLS, np.int64)
    has = last >= 0
    b = values[last[has]] & 255
    start[has] = np.where(signed & (b >= 128), b - 256, b)
    inr = ok & (values >= lo) & (values <= hi)
    inr[inr] &= idx[inr] > last[cells[inr]]
    np.maximum.at(start, cells[inr], values[inr])
    return (start & 255).astype(np.uint8)


def sc(semantic, M=None):
    """calculateSC of the semantic cloud moved by M: uint8 [20, 80] (the bytes of the signed chars)."""
    cells, z = _cells(semantic, M)
    return fold_indexed(cells, sc_values(z), True).reshape(R.RINGS, R.SECTORS)


def isc(semantic, M=None):
    """calculateISC (INTEGER_INTENSITY undefined): uint8 [20, 80]."""
    cells, _ = _cells(semantic, M)
    return fold_indexed(cells, isc_values(semantic["intensity"]), False).reshape(R.RINGS, R.SECTORS)


def ssc(semantic, M=None):
    """calculateSSC: per cell the label of the largest order (order > 0; ties keep the first point, of the same label)."""
    out = np.zeros(R.CELLS, np.int64)
    if len(semantic) == 0:
        return out.astype(np.uint8).reshape(R.RINGS, R.SECTORS)
    cells, _ = _cells(semantic, M)
    lab = np.asarray(semantic["label"], np.int64)
    order = ORDER[lab]
    ok = (cells >= 0) & (order > 0)
    best = np.zeros(R.CELLS, np.int64)
    np.maximum.at(best, cells[ok], order[ok])
    inv = np.zeros(20, np.int64)
    inv[ORDER[9:20]] = np.arange(9, 20)          # order -> label; order 0 -> no label
    return inv[best].astype(np.uint8).reshape(R.RINGS, R.SECTORS)


def ssc_sequential(semantic, M=None):
    """calculateSSC as the reference's loop (for the CPU tests): strictly greater order replaces the stored label."""
    out = np.zeros(R.CELLS, np.int64)
    cells, _ = _cells(semantic, M)
    for c, lab in zip(cells, np.asarray(semantic["label"], np.int64)):
        if ORDER[lab] > 0 and c >= 0 and ORDER[lab] > ORDER[out[c]]:
            out[c] = lab
    return out.astype(np.uint8).reshape(R.RINGS, R.SECTORS)


def all_descriptors(corner, surf, semantic, M=None):
    """every kind's descriptor (by kind index ISC .. SSC) of the clouds moved by M."""
    f, e, s = R.descriptors(corner, surf, semantic, M)
    return {ISC: isc(semantic, M), SC: sc(semantic, M), EPSC: e, SEPSC: s, FEPSC: f, SSC: ssc(semantic, M)}


def label_sim(d1, d2):
    """calculateLabelSim: equal cells over cells not zero in both, in double; 0 / 0 is NaN."""
    d1, d2 = np.asarray(d1), np.asarray(d2)
    valid = ~((d1 == 0) & (d2 == 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.float64(np.count_nonzero(valid & (d1 == d2))) / np.float64(np.count_nonzero(valid)))


def distance_angle(desc1, desc2, angle):
    """calculateDistance with its angle argument: (score, shift, angle + shift * sector_step if a shift improved on 1.0)."""
    score, shift = R.distance(desc1, desc2)
    return score, shift, (float(angle) + shift * R.SECTOR_STEP) if score > 0 else float(angle)


def planar(T, angle):
    """Identity().translation() << T.x, T.y, 0; rotate(AngleAxisf((float)angle, UnitZ()))."""
    M = R.rot_z(np.float32(angle))
    M[0, 3], M[1, 3] = T[0, 3], T[1, 3]
    return M


class EPSCGenerationKinds(R.EPSCGeneration):
    """loopDetection with the kinds of a LISREG_LOOP_* mask; loop_detection returns dict(current_frame_id, matches=[(kind, history_id,
    transform, score)], candidates=[dict(history_id, T, pos_distance, score={kind: s}, shift={kind: i}, angle={kind: the angle of its transform})])."""

    def __init__(self, oracle, kinds=1 << FEPSC, params=(20.0, 0.01, 0.75), label_threshold=LABEL_THRESHOLD):
        super().__init__(oracle, params)
        self.kinds = kinds
        self.label_thr = label_threshold
        self.db = {k: [] for k in range(6)}

    def on(self, k):
        return bool((self.kinds >> k) & 1)

    def loop_detection(self, corner, surf, semantic, odom):
        x_t, y_t, yaw_t = self.pose(odom)
        cur_proj = R.project(semantic)
        current = len(self.pos)
        best = {k: (0.0, -1, None) for k in range(6)}
        pose_best = (1000000.0, -1, None)
        cands = []
        gated = self.gate(x_t, y_t)
        for i in gated:
            yaw_diff = np.float32(yaw_t - self.yaw[i])
            g = R.global_icp(self.proj[i], cur_proj, yaw_diff, self.oracle)
            T = g["T"]
            angle = R.atan2f(T[1, 0], T[0, 0])
            d = all_descriptors(corner, surf, semantic, T)
            ex, ey = self.pos[i][0] - self.pos[-1][0], self.pos[i][1] - self.pos[-1][1]
            pos_distance = math.sqrt(ex * ex + ey * ey + 0.0)
            c = dict(history_id=i, T=T, pos_distance=pos_distance, score={}, shift={}, angle={}, g=g)
            for k in (ISC, SC, EPSC, SEPSC, FEPSC):
                if not self.on(k):
                    continue
                seed = float(yaw_diff) if k == EPSC else float(angle)
                s, sh, a = distance_angle(self.db[k][i], d[k], seed)
                c["score"][k], c["shift"][k], c["angle"][k] = s, sh, (float(angle) if k == FEPSC else a)
                if s > self.thr and s > best[k][0]:
                    best[k] = (s, i, planar(T, angle if k == FEPSC else a))
            if self.on(SSC):
                s = label_sim(self.db[SSC][i], d[SSC])
                c["score"][SSC], c["shift"][SSC] = s, 0
                if s > self.label_thr and s > best[SSC][0]:
                    best[SSC] = (s, i, T.copy())
            if self.on(POSE) and pos_distance < pose_best[0]:
                pose_best = (pos_distance, i, T.copy())
            cands.append(c)
        self.pos.append((float(x_t), float(y_t)))
        self.yaw.append(yaw_t)
        self.proj.append(cur_proj)
        own = all_descriptors(corner, surf, semantic)
        matches = []
        for k in range(6):
            if self.on(k):
                self.db[k].append(own[k])
                if best[k][1] != -1:
                    matches.append((k, best[k][1], best[k][2], best[k][0]))
        if self.on(POSE) and pose_best[1] != -1:
            matches.append((POSE, pose_best[1], pose_best[2], pose_best[0]))
        self.fepsc.append(own[FEPSC])
        return dict(current_frame_id=current, matches=matches, candidates=cands)
