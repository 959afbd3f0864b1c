"""Sequential replay on the HIP path (BASELINE.json configs[2]): the frame loop of SubMapOptmizationNode::makeSubMapThread
(/root/reference/src/node/subMapOptmizationNode.cpp:597-755) with every cloud operation done by liblisreg on the GPU:

  per frame   semantic split (categoryMapping, semanticFusionNode.cpp:173-189) -> per-class voxel grids (keyframeInit :806-811)
              -> pose guess (updateInitialGuess :984-1020) -> lisreg_localmap_extract (extractSlidingCloud :1369-1432 + both
              target indexes) -> label-weighted registration, copy #2 (:1509-1541) -> lisreg_localmap_insert
              (SubMapManager::insert_local_map, subMap.h:979-1059)

The local map lives in HBM from the first frame to the last.

Second loop (BASELINE.json configs[0], no labels needed): the scan-to-map odometry of odomEstimationNode
(/root/reference/src/node/odomEstimationNode.cpp:164-232) on raw sweeps:

  per frame   range-image projection + LOAM features (LaserProcessing, laserProcessing.cpp:467-713 -> lisreg_extract_features)
              -> pose guess (updateInitialGuess :298-419) -> target = the <= 19 newest keyframes, newest first, voxel grids 0.2 / 0.4 m
              (:185-207) -> source voxel grids (currentCloudInit :260-281) -> registration, copy #1 (:596-626)
              -> keyframe gate and saveKeyFrames (:213-226, 421-468: transformPointCloud into the map frame, keep < 20)

Also here: the synthetic drives used when no dataset is mounted, the KITTI / SemanticKITTI readers (incl. the ring assignment of
laserPretreatmentNode.cpp:60-140, which KITTI's .bin files need), and the trajectory writer in the reference's format
(transformFusion, :5079-5179).  This module is host-side driver code (the reference's ROS nodes, minus ROS): every cloud
operation is a liblisreg call; what it computes itself is bookkeeping on 6-vectors and the reader's per-point ring number."""
from __future__ import annotations

import os
import sys
import time

import numpy as np

from . import synth

CLASSES = ("dynamic", "pole", "ground", "building", "outlier")
FRAME_LEAF = dict(dynamic=0.2, pole=0.05, ground=0.6, building=0.4, outlier=0.6)      # keyframeInit :806-811

# config/label.yaml:110-144 `learning_map`: SemanticKITTI raw ids -> the 20 RangeNet++ classes the reference's nodes see
LEARNING_MAP = {0: 0, 1: 0, 10: 1, 11: 2, 13: 5, 15: 3, 16: 5, 18: 4, 20: 5, 30: 6, 31: 7, 32: 8, 40: 9, 44: 10, 48: 11, 49: 12,
                50: 13, 51: 14, 52: 0, 60: 9, 70: 15, 71: 16, 72: 17, 80: 18, 81: 19, 99: 0, 252: 1, 253: 7, 254: 6, 255: 8,
                256: 5, 257: 5, 258: 4, 259: 5}


# ---- inputs ---------------------------------------------------------------------------------------------------------
def synthetic_drive(n_frames: int, h: int = 64, w: int = 1800, step: float = 0.45, seed: int = 7, car: bool = True):
    """A labelled drive through the synthetic room of synth.py: frame k is an H x W sweep from a pose that advances `step`
    metres per frame on a gently curving path (first pose level, yaw 0, so the map frame equals the first sensor frame).
    Labels are RangeNet classes: pole 18, road 9, building 13; floor returns inside a rectangle that moves with the frames
    are relabelled car (1) so that the dynamic class and the map-based dynamic removal are exercised.
    Yields (cloud PointXYZIL struct array, T_true relative to frame 0)."""
    x0, y0 = -14.0, -6.0
    for k in range(n_frames):
        yaw = 0.35 * np.sin(0.08 * k)
        x = x0 + step * k * np.cos(0.12) - 0.0
        y = y0 + step * k * np.sin(0.12) + 1.5 * np.sin(0.05 * k)
        T_world = np.array([0.0, 0.0, yaw, x, y, synth.SENSOR_Z])
        sc = synth.make_scan(h, w, seed * 1000 + k, labelled=True, T_true=T_world)
        cloud = synth.concat_clouds([sc["corner"], sc["surf"]])
        if car:
            M = synth.pose_matrix(T_world)
            xyz = synth.pcl_xyz(cloud).astype(np.float64) @ M[:3, :3].T + M[:3, 3]
            cx, cy = x + 6.0 + 0.5 * k * 0.2, y + 2.5
            in_car = (np.abs(xyz[:, 0] - cx) < 2.0) & (np.abs(xyz[:, 1] - cy) < 0.9) & (cloud["label"] == synth.LABEL_GROUND)
            cloud["label"][in_car] = 1
        T_rel = np.array([0.0, 0.0, yaw, x - x0, y - y0, 0.0])                 # frame 0 has yaw 0
        yield cloud, T_rel


def read_kitti_frame(bin_path: str, label_path: str | None):
    """velodyne/*.bin (float32 x y z remission) + labels/*.label (uint32: low 16 bits = SemanticKITTI class) ->
    PointXYZIL struct array carrying the RangeNet class id the reference's semantic node would publish."""
    raw = np.fromfile(bin_path, np.float32).reshape(-1, 4)
    lab = np.zeros(len(raw), np.uint16)
    if label_path and os.path.exists(label_path):
        sem = np.fromfile(label_path, np.uint32) & 0xFFFF
        lut = np.zeros(65536, np.uint16)
        for k, v in LEARNING_MAP.items():
            lut[k] = v
        lab = lut[sem]
    return synth.to_pcl(raw[:, :3].copy(), lab, raw[:, 3].copy())


def kitti_sequence(root: str, seq: str, max_frames: int | None = None):
    """Yields labelled frames of <root>/sequences/<seq>/{velodyne,labels} in order."""
    d = os.path.join(root, "sequences", seq)
    names = sorted(f[:-4] for f in os.listdir(os.path.join(d, "velodyne")) if f.endswith(".bin"))
    for i, nm in enumerate(names):
        if max_frames is not None and i >= max_frames:
            return
        yield read_kitti_frame(os.path.join(d, "velodyne", nm + ".bin"), os.path.join(d, "labels", nm + ".label")), None


def write_trajectory(path: str, poses):
    """transformFusion's file format (:5079-5179): per pose one line with the 12 entries of H_init^-1 * H (row-major 3 x 4),
    scientific notation, 6 digits."""
    H0 = None
    with open(path, "w") as f:
        for T in poses:
            H = synth.pose_matrix(np.asarray(T, np.float64))
            if H0 is None:
                H0 = np.linalg.inv(H)
            R = H0 @ H
            f.write(" ".join(f"{R[i, j]:.6e}" for i in range(3) for j in range(4)) + "\n")


# ---- raw sweeps (no labels): pretreatment + drive -----------------------------------------------------------------------
def kitti_rings(raw: np.ndarray, n_scan: int = 64, min_range: float = 0.0, max_range: float = 70.0) -> np.ndarray:
    """laserPretreatmentNode.cpp:60-140 for an HDL-64 sweep without a ring channel (KITTI velodyne/*.bin: x y z remission):
    NaN and range filter (removeClosedPointCloud, laserPretreatment.h:26-54), ring from the elevation angle with the reference's
    two-slope table, rings > 50 and angles outside [-24.33, 2] dropped.  Returns a PointXYZIRT struct array (time 0: no de-skewing
    without IMU), points in input order."""
    assert n_scan == 64, "the reference's table for KITTI is the N_SCAN == 64 branch"
    raw = np.asarray(raw, np.float32).reshape(-1, 4)
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    ok = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    r2 = x * x + y * y + z * z
    ok &= ~(r2 < np.float32(min_range) * np.float32(min_range)) & ~(r2 > np.float32(max_range) * np.float32(max_range))
    with np.errstate(divide="ignore", invalid="ignore"):
        angle = (np.arctan(z / np.sqrt(x * x + y * y)) * np.float32(180.0) / np.float32(np.pi)).astype(np.float32)
    upper = angle >= np.float32(-8.83)
    with np.errstate(invalid="ignore"):
        ring = np.where(upper, ((np.float32(2) - angle) * np.float32(3.0) + np.float32(0.5)).astype(np.int64),
                        n_scan // 2 + ((np.float32(-8.83) - angle) * np.float32(2.0) + np.float32(0.5)).astype(np.int64))
    ok &= ~((angle > 2) | (angle < np.float32(-24.33)) | (ring > 50) | (ring < 0)) & np.isfinite(angle)
    out = np.zeros(int(ok.sum()), synth.XYZIRT_DTYPE)
    out["x"], out["y"], out["z"], out["intensity"] = x[ok], y[ok], z[ok], raw[ok, 3]
    out["ring"] = ring[ok].astype(np.uint16)
    return out


def kitti_raw_sequence(root: str, seq: str, max_frames: int | None = None, pretreated: bool = True):
    """Yields the sweeps of <root>/sequences/<seq>/velodyne in order: pretreated on the host (PointXYZIRT, kitti_rings), or — pretreated=False —
    the raw (n, 4) float32 arrays as they are in the files, for RawOdomReplayer."""
    d = os.path.join(root, "sequences", seq, "velodyne")
    names = sorted(f for f in os.listdir(d) if f.endswith(".bin"))
    for i, nm in enumerate(names):
        if max_frames is not None and i >= max_frames:
            return
        raw = np.fromfile(os.path.join(d, nm), np.float32).reshape(-1, 4)
        yield (kitti_rings(raw) if pretreated else raw), None


def synthetic_raw_drive(n_frames: int, h: int = 64, w: int = 1800, step: float = 0.45, seed: int = 11):
    """Unlabelled sweeps (PointXYZIRT, ring-major as a spinning lidar delivers them) along the path of synthetic_drive."""
    x0, y0 = -14.0, -6.0
    for k in range(n_frames):
        yaw = 0.35 * np.sin(0.08 * k)
        x = x0 + step * k * np.cos(0.12)
        y = y0 + step * k * np.sin(0.12) + 1.5 * np.sin(0.05 * k)
        T_world = np.array([0.0, 0.0, yaw, x, y, synth.SENSOR_Z])
        sc = synth.make_scan(h, w, seed * 1000 + k, T_true=T_world)
        both = synth.concat_clouds([sc["corner"], sc["surf"]])
        xyz = synth.pcl_xyz(both)
        el = np.degrees(np.arctan2(xyz[:, 2], np.hypot(xyz[:, 0], xyz[:, 1])))
        ring = np.clip(np.rint((el + 24.8) / (26.8 / (h - 1))), 0, h - 1).astype(np.uint16)
        order = np.lexsort((np.arctan2(xyz[:, 1], xyz[:, 0]), ring))
        out = np.zeros(len(xyz), synth.XYZIRT_DTYPE)
        out["x"], out["y"], out["z"] = xyz[order, 0], xyz[order, 1], xyz[order, 2]
        out["ring"] = ring[order]
        yield out, np.array([0.0, 0.0, yaw, x - x0, y - y0, 0.0])


def xyzi_of(cloud) -> np.ndarray:
    """pcl::fromROSMsg(cloud_info.cloud_corner, PointCloud<PointXYZI>): keep x, y, z, intensity (odomEstimationNode.cpp:266-267)."""
    xyz = np.stack([cloud["x"], cloud["y"], cloud["z"]], 1).astype(np.float32)
    return synth.to_pcl(xyz, None, np.asarray(cloud["intensity"], np.float32))


ODOM = dict(corner_leaf=0.2, surf_leaf=0.4, key_dist=1.4, key_yaw=0.5, max_keyframes=19)      # params.yaml:132-141


def increment(T_from, T_to) -> np.ndarray:
    """calculateTranslation (odomEstimationNode.cpp:284-295): transBack^-1 * transTobe as (roll, pitch, yaw, x, y, z)."""
    A, B = synth.pose_matrix(np.asarray(T_from, np.float64)), synth.pose_matrix(np.asarray(T_to, np.float64))
    F = np.linalg.inv(A) @ B
    return np.array([np.arctan2(F[2, 1], F[2, 2]), np.arcsin(-F[2, 0]), np.arctan2(F[1, 0], F[0, 0]), F[0, 3], F[1, 3], F[2, 3]])


class OdomReplayer:
    """laserCloudInfoHandler's state (odomEstimationNode.cpp:164-232): transformTobeMapped, the previous pose, the keyframe
    clouds in the map frame (<= 19), transformPriFrame, keyFrameId.  Everything that touches a cloud runs in liblisreg."""

    def __init__(self, ctx, feature_params=None, target_slot: int = 0, ring_id: int = 0):
        import lisreg
        self.ctx, self.slot = ctx, target_slot
        self.params = lisreg.default_params(1)
        self.fp = feature_params or lisreg.default_feature_params()
        self.T = np.zeros(6, np.float32)
        self.T_last = None
        self.calls = 0
        self.ring = ring_id
        ctx.keyframes_reset(ring_id)
        self.T_pri = np.zeros(6, np.float32)
        self.key_id = 0
        self.k = 0

    def _guess(self):
        """updateInitialGuess without IMU / odometry input (:298-384): call 1 initialises, call 2 records, then constant velocity."""
        import lisreg
        self.calls += 1
        if self.calls == 1:
            return
        if self.T_last is None:
            self.T_last = self.T.copy()
            return
        g = lisreg.predict_pose(self.T_last, self.T)
        self.T_last = self.T.copy()
        self.T = g

    def _save_keyframe(self, corner, surf):
        """saveKeyFrames (:421-468): the frame's FULL feature clouds, transformed into the map frame; fewer than 20 are kept —
        in HBM (lisreg_keyframes_push)."""
        self.ctx.keyframes_push(self.ring, corner, surf, self.T, ODOM["max_keyframes"])
        self.T_pri = self.T.copy()
        self.key_id += 1

    def step(self, sweep) -> dict:
        t0 = time.perf_counter()
        f = self.ctx.extract_features(sweep, self.fp)
        corner, surf = xyzi_of(f["corner"]), xyzi_of(f["surface"])
        self._guess()
        rec = dict(frame=self.k, n_corner=len(corner), n_surf=len(surf), guess=self.T.copy(), stats=None, keyframe=False)
        if self.k == 0:                                             # FirstFlag branch (:178-186)
            self._save_keyframe(corner, surf)
            rec["keyframe"] = True
        else:
            # target = the kept key frames, newest first, voxel grids, both indexes (:185-207, 602-603) — assembled in HBM
            info = self.ctx.keyframes_target(self.ring, ODOM["corner_leaf"], ODOM["surf_leaf"], self.slot)
            sc = self.ctx.voxel_downsample(corner, ODOM["corner_leaf"])[1] if len(corner) else corner
            ss = self.ctx.voxel_downsample(surf, ODOM["surf_leaf"])[1] if len(surf) else surf
            T, st, _ = self.ctx.align(sc, ss, self.T, self.params)
            self.T = T.astype(np.float32)
            rec.update(stats=st, n_target_corner=info["n_target_corner"], n_target_surf=info["n_target_surf"],
                       n_src_corner=len(sc), n_src_surf=len(ss))
            if st["status"] == 0 and (st["deltaR"] < 0.005 or st["deltaT"] < 0.05):                       # :213-226
                inc = increment(self.T_pri, self.T)
                if self.key_id <= 5 or abs(inc[2]) >= ODOM["key_yaw"] or abs(inc[3]) >= ODOM["key_dist"] or abs(inc[4]) >= ODOM["key_dist"]:
                    self._save_keyframe(corner, surf)
                    rec["keyframe"] = True
        rec.update(T=self.T.copy(), key_id=self.key_id, ms=1e3 * (time.perf_counter() - t0))
        self.k += 1
        return rec


class DeviceOdomReplayer(OdomReplayer):
    """The odometry loop with the frame's clouds kept in HBM: the sweep goes up once as (x, y, z, ring) records, the feature
    clouds, their voxel grids, the registration sources and the key frame never come back.  Same kernels, same order, same poses."""

    def __init__(self, ctx, feature_params=None, target_slot: int = 0, ring_id: int = 0):
        super().__init__(ctx, feature_params, target_slot, ring_id)
        import lisreg
        self.cap = self.fp.n_scan * self.fp.horizon_scan
        z = np.zeros((self.cap, 4), np.float32)
        self.raw = lisreg.DeviceArray(np.zeros((2 * self.cap, 4), np.float32))
        self.names = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
        self.feat = {k: lisreg.DeviceArray(z) for k in self.names}
        self.ds_c, self.ds_s = lisreg.DeviceArray(z), lisreg.DeviceArray(z)

    def _save_keyframe_device(self, n_c, n_s):
        self.ctx.keyframes_push_device(self.ring, self.feat["corner"].ptr, n_c, self.feat["surface"].ptr, n_s, self.T, ODOM["max_keyframes"])
        self.T_pri = self.T.copy()
        self.key_id += 1

    def _front(self, sweep) -> dict:
        """the sweep into HBM and through the feature extraction: the counts of the five clouds"""
        n = len(sweep)
        assert n <= 2 * self.cap
        self.ctx.upload_cloud(sweep, self.raw.ptr)                   # (x, y, z, ring) records
        return self.ctx.extract_features_device(self.raw.ptr, n, self.fp, {k: v.ptr for k, v in self.feat.items()}, self.cap)

    def step(self, sweep) -> dict:
        t0 = time.perf_counter()
        cnt = self._front(sweep)
        n_c, n_s = cnt["corner"], cnt["surface"]
        self._guess()
        rec = dict(frame=self.k, n_corner=n_c, n_surf=n_s, guess=self.T.copy(), stats=None, keyframe=False)
        if self.k == 0:
            self._save_keyframe_device(n_c, n_s)
            rec["keyframe"] = True
        else:
            info = self.ctx.keyframes_target(self.ring, ODOM["corner_leaf"], ODOM["surf_leaf"], self.slot)
            nsc, nss = self.ctx.voxel_downsample_multi_device([self.feat["corner"].ptr, self.feat["surface"].ptr], [n_c, n_s],
                                                              [ODOM["corner_leaf"], ODOM["surf_leaf"]], [self.ds_c.ptr, self.ds_s.ptr],
                                                              [self.cap, self.cap], intensity=True)
            T, st = self.ctx.align_device(self.ds_c.ptr, nsc, self.ds_s.ptr, nss, self.T, self.params)
            self.T = T.astype(np.float32)
            rec.update(stats=st, n_target_corner=info["n_target_corner"], n_target_surf=info["n_target_surf"], n_src_corner=nsc, n_src_surf=nss)
            if st["status"] == 0 and (st["deltaR"] < 0.005 or st["deltaT"] < 0.05):
                inc = increment(self.T_pri, self.T)
                if self.key_id <= 5 or abs(inc[2]) >= ODOM["key_yaw"] or abs(inc[3]) >= ODOM["key_dist"] or abs(inc[4]) >= ODOM["key_dist"]:
                    self._save_keyframe_device(n_c, n_s)
                    rec["keyframe"] = True
        rec.update(T=self.T.copy(), key_id=self.key_id, ms=1e3 * (time.perf_counter() - t0))
        self.k += 1
        return rec


class RawOdomReplayer(DeviceOdomReplayer):
    """DeviceOdomReplayer fed with RAW sweeps — (n, 4) float32 arrays x y z intensity, a KITTI velodyne file as it is: the 16-byte records
    go to HBM untouched, lisreg_pretreat derives ring and time there (laserPretreatmentNode), and the ring records (with the times, when
    `deskew_of` returns a Deskew for the frame) go to the feature extraction.  No host pass over the sweep."""

    def __init__(self, ctx, feature_params=None, target_slot: int = 0, ring_id: int = 0, pretreat_params=None, deskew_of=None):
        super().__init__(ctx, feature_params, target_slot, ring_id)
        import lisreg
        self.pp = pretreat_params or lisreg.default_pretreat_params(self.fp.n_scan)
        self.raw_in = lisreg.DeviceArray(np.zeros((2 * self.cap, 4), np.float32))
        self.time = lisreg.DeviceArray(np.zeros(2 * self.cap, np.float32))
        self.deskew_of = deskew_of                                   # frame number -> lisreg.Deskew (time_device is filled in here) or None
        self.pretreat = None                                         # the last frame's pretreatment result

    def _front(self, sweep) -> dict:
        import ctypes as C
        sweep = np.ascontiguousarray(sweep, np.float32).reshape(-1, 4)
        n = len(sweep)
        assert n <= 2 * self.cap
        self.ctx.upload_cloud(sweep, self.raw_in.ptr)                # the records as they are
        self.pretreat = self.ctx.pretreat_device(self.raw_in.ptr, n, self.pp, self.raw.ptr, self.time.ptr, 2 * self.cap)
        dk = self.deskew_of(self.k) if self.deskew_of else None
        if dk is not None:
            dk.time_device = C.cast(C.c_void_p(self.time.ptr), C.POINTER(C.c_float))
        return self.ctx.extract_features_device(self.raw.ptr, self.pretreat["n"], self.fp, {k: v.ptr for k, v in self.feat.items()}, self.cap,
                                                deskew=dk)


def replay_odom(ctx, sweeps, feature_params=None, on_frame=None, device_resident: bool = False, raw_input: bool = False):
    r = RawOdomReplayer(ctx, feature_params) if raw_input else DeviceOdomReplayer(ctx, feature_params) if device_resident else OdomReplayer(ctx, feature_params)
    out = []
    for sw in sweeps:
        rec = r.step(sw)
        out.append(rec)
        if on_frame:
            on_frame(rec)
    return out


# ---- the frame loop -------------------------------------------------------------------------------------------------
class Replayer:
    """makeSubMapThread's state: transformTobeSubMapped, the previous pose, the local map (device object `map_id` of `ctx`).

    labeller: optional callable `logits_ptr = labeller(tensor_ptr)` — the caller's segmentation model on device pointers (the 5 x H x W
    float input tensor in, the n_classes x H x W float logits out, written when it returns).  With it, step() takes an UNLABELLED sweep
    ((n, 4) float32 x y z intensity, or PCL structs) and labels it on the device through Context.rangenet_project_device /
    rangenet_label_device (`rangenet_params`, default lisreg.default_rangenet_params()) in place of labels from a file.  Without it
    nothing changes."""

    def __init__(self, ctx, variant: int = 2, map_id: int = 0, target_slot: int = 0, labeller=None, rangenet_params=None):
        import lisreg
        self.ctx, self.map_id, self.slot = ctx, map_id, target_slot
        self.labeller, self.rn_params, self._rn = labeller, rangenet_params, None
        self.params = lisreg.default_params(variant)
        self.lm_params = lisreg.localmap_default_params()
        self.T = np.zeros(6, np.float32)
        self.T_last = None
        self.k = 0
        self.guess_obj = None
        ctx.localmap_reset(map_id)

    def _label_on_device(self, cloud, raw_ptr=None, capacity=None):
        """project -> labeller -> label: returns (device pointer of the labelled records, n).  `raw_ptr`: a device buffer of `capacity`
        records to upload the sweep into (one of our own otherwise)."""
        import lisreg
        cloud = np.ascontiguousarray(cloud)
        if cloud.dtype.names:                                          # PCL structs: x y z + intensity at byte 16 -> packed records
            cloud = np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["intensity"]], 1)
        cloud = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        n = len(cloud)
        if self.rn_params is None:
            self.rn_params = lisreg.default_rangenet_params()
        P = self.rn_params
        hw = P.img_h * P.img_w
        if self._rn is None or self._rn["cap"] < n or self._rn["hw"] != hw:
            cap = max(n, capacity or 0, 1)
            self._rn = dict(cap=cap, hw=hw, tensor=lisreg.DeviceArray(np.zeros(5 * hw, np.float32)), mask=lisreg.DeviceArray(np.zeros(hw, np.uint8)),
                            pix=lisreg.DeviceArray(np.zeros(cap, np.int32)), lab=lisreg.DeviceArray(np.zeros((cap, 4), np.float32)),
                            raw=None if raw_ptr else lisreg.DeviceArray(np.zeros((cap, 4), np.float32)))
        b = self._rn
        src = raw_ptr if raw_ptr else b["raw"].ptr
        if n:
            self.ctx.upload_cloud(cloud, src)
        self.n_valid_pixels = self.ctx.rangenet_project_device(src, n, P, b["tensor"].ptr, b["mask"].ptr, b["pix"].ptr)
        logits_ptr = int(self.labeller(b["tensor"].ptr))
        self.ctx.rangenet_label_device(src, n, b["pix"].ptr, b["mask"].ptr, logits_ptr, P, b["lab"].ptr)
        return b["lab"].ptr, n, cloud

    def _split_and_downsample(self, cloud):
        if self.labeller is not None:                                  # labels from the model instead of from a file
            import lisreg
            ptr, n, raw = self._label_on_device(cloud)
            rec = lisreg.device_to_host(ptr, (max(n, 1), 4), np.float32)[:n]
            cloud = synth.to_pcl(raw[:, :3], rec[:, 3].view(np.uint32).astype(np.uint16), raw[:, 3])
        parts = self.ctx.semantic_split(cloud)                      # dynamic, ground, building, pole, outlier
        full = dict(dynamic=parts[0], ground=parts[1], building=parts[2], pole=parts[3], outlier=parts[4])
        down = {k: (self.ctx.voxel_downsample(c, FRAME_LEAF[k])[1] if len(c) else c) for k, c in full.items()}
        return full, down

    def _initial_guess(self, guess_input):
        """updateInitialGuess as a whole (:896-1032) when the frame comes with cloudInfo's IMU / odometry fields; returns the lisreg.Imu
        that transformUpdate blends with, or None"""
        import lisreg
        if self.guess_obj is None:
            self.guess_obj = lisreg.InitialGuess(1)
        self.T, _ = self.guess_obj.update(self.T, **guess_input)
        if guess_input.get("imu_available"):
            return lisreg.Imu(1, float(guess_input["imu_rpy"][0]), float(guess_input["imu_rpy"][1]))
        return None

    def step(self, cloud, guess_input=None) -> dict:
        import lisreg
        t0 = time.perf_counter()
        full, down = self._split_and_downsample(cloud)
        rec = dict(frame=self.k)
        imu = self._initial_guess(guess_input) if guess_input is not None else None
        if self.k == 0:                                             # subMapFirstFlag branch (:634-651)
            rec.update(T=self.T.copy(), guess=self.T.copy(), stats=None)
        else:
            if guess_input is not None:
                guess = self.T.copy()
            elif self.T_last is None:                               # updateInitialGuess: the first call only records (:1003-1011)
                self.T_last = self.T.copy()
                guess = self.T.copy()
            else:
                guess = lisreg.predict_pose(self.T_last, self.T)
                self.T_last = self.T.copy()
            info = self.ctx.localmap_extract(self.map_id, guess, self.lm_params, self.slot)
            src_c = down["pole"]                                                              # currentCloudInit :866-868
            src_s = synth.concat_clouds([down["dynamic"], down["building"], down["ground"]])   # :873-889
            T, st, _ = self.ctx.align(src_c, src_s, guess, self.params, imu=imu)
            self.T = T.astype(np.float32)
            rec.update(T=self.T.copy(), guess=guess.copy(), stats=st, n_target_corner=info["n_target_corner"],
                       n_target_surf=info["n_target_surf"], n_src_corner=len(src_c), n_src_surf=len(src_s), crop=info["crop"])
        info = self.ctx.localmap_insert(self.map_id, [full[c] for c in CLASSES], self.T, self.lm_params)
        rec.update(n_map=info["n"], feature_point_num=info["feature_point_num"], bound=info["bound"], ms=1e3 * (time.perf_counter() - t0))
        self.k += 1
        return rec


class DeviceReplayer(Replayer):
    """The same loop with every cloud of the frame kept in HBM between the steps: the sweep goes up once as 16-byte records
    (label in the payload), categoryMapping, the per-class voxel grids, the source assembly, the registration and the map insert
    all take device pointers.  Only counts and the pose come back.  Same kernels in the same order as Replayer: the poses are
    bit-identical (tests/test_replay.py)."""

    def __init__(self, ctx, variant: int = 2, map_id: int = 0, target_slot: int = 0, capacity: int = 1 << 18, labeller=None,
                 rangenet_params=None):
        super().__init__(ctx, variant, map_id, target_slot, labeller, rangenet_params)
        import lisreg
        z = np.zeros((capacity, 4), np.float32)
        self.cap = capacity
        self.raw = lisreg.DeviceArray(z)
        self.full = [lisreg.DeviceArray(z) for _ in range(5)]       # dynamic, ground, building, pole, outlier (categoryMapping order)
        self.down = [lisreg.DeviceArray(z) for _ in range(5)]
        self.src_s = lisreg.DeviceArray(z)

    def step(self, cloud) -> dict:
        import lisreg
        t0 = time.perf_counter()
        n = len(cloud)
        assert n <= self.cap
        if self.labeller is not None:                                  # the sweep goes up unlabelled; the labelled records stay in HBM
            labelled_ptr, n, _ = self._label_on_device(cloud, self.raw.ptr, self.cap)
        else:
            self.ctx.upload_cloud(cloud, self.raw.ptr)
            labelled_ptr = self.raw.ptr
        nf = self.ctx.semantic_split_device(labelled_ptr, n, [b.ptr for b in self.full], self.cap)
        order = ("dynamic", "ground", "building", "pole", "outlier")
        leaf = [FRAME_LEAF[k] for k in order]
        nd = self.ctx.voxel_downsample_multi_device([self.full[k].ptr for k in range(5)], nf, leaf, [self.down[k].ptr for k in range(5)], [self.cap] * 5)
        rec = dict(frame=self.k)
        if self.k == 0:
            rec.update(T=self.T.copy(), guess=self.T.copy(), stats=None)
        else:
            if self.T_last is None:
                self.T_last = self.T.copy()
                guess = self.T.copy()
            else:
                guess = lisreg.predict_pose(self.T_last, self.T)
                self.T_last = self.T.copy()
            info = self.ctx.localmap_extract(self.map_id, guess, self.lm_params, self.slot)
            # currentCloudInit (:866-889): corner = pole; surf = dynamic + building + ground
            off = self.ctx.concat_device([self.down[k].ptr for k in (0, 2, 1)], [nd[k] for k in (0, 2, 1)], self.src_s.ptr)
            T, st = self.ctx.align_device(self.down[3].ptr, nd[3], self.src_s.ptr, off, guess, self.params)
            self.T = T.astype(np.float32)
            rec.update(T=self.T.copy(), guess=guess.copy(), stats=st, n_target_corner=info["n_target_corner"],
                       n_target_surf=info["n_target_surf"], n_src_corner=nd[3], n_src_surf=off, crop=info["crop"])
        # append_feature order of the map: dynamic, pole, ground, building, outlier
        idx = (0, 3, 1, 2, 4)
        info = self.ctx.localmap_insert_device(self.map_id, [self.full[k].ptr for k in idx], [nf[k] for k in idx], self.T, self.lm_params)
        rec.update(n_map=info["n"], feature_point_num=info["feature_point_num"], bound=info["bound"], ms=1e3 * (time.perf_counter() - t0))
        self.k += 1
        return rec


def replay(ctx, frames, variant: int = 2, on_frame=None, device_resident: bool = False, guess_inputs=None):
    """guess_inputs: per frame the cloudInfo fields of updateInitialGuess (dict: odom_available, imu_available, imu_rpy, initial_guess);
    host-cloud replayer only"""
    r = DeviceReplayer(ctx, variant) if (device_resident and guess_inputs is None) else Replayer(ctx, variant)
    out = []
    for k, cloud in enumerate(frames):
        rec = r.step(cloud) if guess_inputs is None else r.step(cloud, guess_inputs[k])
        out.append(rec)
        if on_frame:
            on_frame(rec)
    return out


def _chain_roofline(ctx, make_replayer, frames, src_points_of):
    """A second, untimed pass over the same frames with HIP events around every correspondence launch (lisreg_set_profiling): the
    dominant kernel of the chain against the HBM roofline, algorithmic bytes = 96 B x (source points x executed GN iterations)."""
    r = make_replayer()
    ctx.set_profiling(True)
    ms, launches, pt_iters = 0.0, 0, 0
    for cloud in frames:
        rec = r.step(cloud)
        t = ctx.timing()
        if rec.get("stats"):
            ms += t["assoc_ms"]; launches += int(t["assoc_launches"])
            pt_iters += src_points_of(rec) * int(rec["stats"]["iters"])
    ctx.set_profiling(False)
    if launches == 0 or ms <= 0:
        return None
    achieved = 96.0 * pt_iters / (ms * 1e-3) / 1e9
    return dict(bound="hbm", kernel="k_assoc_walk (eight lanes per query) + k_rows_reduce", achieved=round(achieved, 2), peak=8000.0, unit="GB/s",
                frac=round(achieved / 8000.0, 5), traffic=None, avg_launch_ms=round(ms / launches, 4), launches=launches,
                algorithmic_bytes_per_launch=int(96 * pt_iters / launches),
                note="a frame's registration is a few thousand source points: launch-latency bound, the fraction says how far a single small "
                     "registration is from the bandwidth the batched path reaches; launches include the no-op launches between host looks at the "
                     "finished-counter")


def bench_sequence(device: int, steps: int = 20, warmup: int = 2, roofline: bool = True) -> dict:
    """bench.py --workload cfg3: frames/s of the synthetic drive on the HIP chain (host-inclusive: every frame's sweep crosses
    PCIe, as in the reference's node).  Returns the bench line plus `_frames` / `_recs` (the inputs and the HIP chain's records)
    for bench.py's CPU-baseline leg.  roofline=False skips the second, profiled pass over the frames."""
    import lisreg
    n = max(steps, 1) + warmup                  # exactly `steps` timed frames after the warm-up ones
    frames = [c for c, _ in synthetic_drive(n)]
    truth = [t for _, t in synthetic_drive(n)]
    ctx = lisreg.Context(device)
    r = DeviceReplayer(ctx, 2)
    recs = []
    t0 = None
    import gc
    for k, cloud in enumerate(frames):
        if k == warmup:
            # the interpreter's generation-2 collection is a 35 ms pause in a process that has torch loaded (bench.py) — one such pause
            # inside 50 frames of 1.3 ms read as 2.0 ms per frame; the loop allocates no cycles, so the collector rests while it is timed
            gc.collect(); gc.disable()
            t0 = time.perf_counter()
        recs.append(r.step(cloud))
    dt = time.perf_counter() - t0
    gc.enable()
    err = max(float(np.abs(np.asarray(rec["T"], np.float64)[3:5] - truth[rec["frame"]][3:5]).max()) for rec in recs)
    roof = _chain_roofline(ctx, lambda: DeviceReplayer(ctx, 2), frames, lambda rec: int(rec["n_src_corner"]) + int(rec["n_src_surf"])) if roofline else None
    ctx.close()
    # (the CPU baseline of this line — the oracle chain on the first frames — is timed by bench.py: this package never touches oracle/)
    cpu = None
    return {"metric": "sequential scan-to-local-map registrations/sec (synthetic drive, semantic mask on)",
            "value": round((n - warmup) / dt, 2), "unit": "frames/s", "steps": steps, "warmup": warmup,
            "ms_per_step": round(1e3 * dt / (n - warmup), 3), "higher_is_better": True, "vs_baseline": None, "dtype": "f32",
            "data": "synthetic", "config": {"workload": "configs[2] synthetic stand-in: 64x1800 labelled sweeps, host clouds in, "
                                                        "device-resident sliding local map, copy #2 parameters, early exit"},
            "roofline": roof, "cpu_baseline": cpu,
            "accuracy": {"max_xy_err_vs_truth_m": err, "frames": n,
                         "iters": [rec["stats"]["iters"] for rec in recs if rec["stats"]]},
            "_frames": list(frames), "_recs": recs}


def bench_odometry(device: int, steps: int = 20, warmup: int = 2, roofline: bool = True) -> dict:
    """bench.py --workload odom: frames/s of the raw-sweep odometry chain on the HIP path (host-inclusive: every sweep crosses
    PCIe, features and keyframes come back to the host driver as in the reference's node graph).  roofline: see bench_sequence."""
    import lisreg
    n = max(steps, 1) + warmup                  # exactly `steps` timed frames after the warm-up ones
    frames, truth = zip(*synthetic_raw_drive(n))
    ctx = lisreg.Context(device)
    r = DeviceOdomReplayer(ctx)
    recs, t0 = [], None
    import gc
    for k, sw in enumerate(frames):
        if k == warmup:
            gc.collect(); gc.disable()              # see bench_sequence
            t0 = time.perf_counter()
        recs.append(r.step(sw))
    dt = time.perf_counter() - t0
    gc.enable()
    err = max(float(np.abs(np.asarray(rec["T"], np.float64)[3:5] - truth[rec["frame"]][3:5]).max()) for rec in recs)
    roof = (_chain_roofline(ctx, lambda: DeviceOdomReplayer(ctx), frames, lambda rec: int(rec.get("n_src_corner", 0)) + int(rec.get("n_src_surf", 0)))
            if roofline else None)
    ctx.close()
    cpu = None                                  # timed by bench.py (see bench_sequence)
    return {"metric": "sequential scan-to-map odometry frames/sec (synthetic raw drive, no labels)",
            "value": round((n - warmup) / dt, 2), "unit": "frames/s", "steps": steps, "warmup": warmup,
            "ms_per_step": round(1e3 * dt / (n - warmup), 3), "higher_is_better": True, "vs_baseline": None, "dtype": "f32",
            "data": "synthetic", "config": {"workload": "configs[0] as a sequence: raw 64x1800 sweeps in, range image + LOAM features, "
                                                        "voxel grids, copy #1 registration against <= 19 keyframes, early exit"},
            "roofline": roof, "cpu_baseline": cpu,
            "accuracy": {"max_xy_err_vs_truth_m": err, "frames": n, "keyframes": int(sum(rec["keyframe"] for rec in recs)),
                         "iters": [rec["stats"]["iters"] for rec in recs if rec["stats"]]},
            "_frames": list(frames), "_recs": recs}
