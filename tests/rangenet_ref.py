"""CPU restatement of the host code the reference wraps around its RangeNet++ network — the yardstick of lisreg_rangenet_project and
lisreg_rangenet_label (tests/test_rangenet.py).

NetTensorRT::doProjection and the host halves of NetTensorRT::infer (reference src/segnet/netTensorRT.cpp:143-300, :333-354, :403-428)
and the argmax of RangenetAPI::infer (src/core/rangenetAPI.cpp:50-73, :103-110), restated from knowledge of the C++ expressions with
their float / double steps:

  1. (:146-148) fov_up = (float)(_fov_up / 180.0 * M_PI), fov_down likewise: double quotient and product rounded to float;
     fov = fabsf(fov_down) + fabsf(fov_up), a float sum.
  2. (:167) range = sqrtf((x*x + y*y) + z*z) in float.
  3. (:177-178) yaw = -atan2f(y, x); pitch = asinf(z / range), a float quotient (NaN for a point at the origin).
  4. (:192-193) proj_x = (float)(0.5 * ((double)yaw / M_PI + 1.0)); proj_y = (float)(1.0 - (double)((pitch + fabsf(fov_down)) / fov)),
     the inner sum and quotient float.
  5. (:196-207) proj_x *= _img_w, proj_y *= _img_h (`float * int`: float products); floorf; std::min(size - 1.0f, v) is
     `v < size - 1 ? v : size - 1`, std::max(0.0f, v) is `0 < v ? v : 0`: a NaN proj_y becomes row H - 1.
  6. (:272-294) points assigned to pixel y * W + x in order of decreasing range, later assignments overwrite: a pixel keeps its point of
     smallest range.  sort_indexes is an unstable std::sort: the reference does not say which of several points of exactly equal range
     in one pixel is kept.  DEFINED here as the one of highest input index — a stable sort assigned in order.
  7. (:341) a pixel is invalid when all five values (range, x, y, z, intensity) convert to the int 0 (the lambda takes `int i`): every
     empty pixel, and a pixel whose winner has range < 1 and |intensity| < 1.  Invalid pixels carry five zeros, the others
     (v - mean[c]) / std[c] in float; the tensor is channel-major, 5 x H x W.
  8. (:420-428) logits of invalid pixels replaced by {1, 0, ..., 0}; a point takes the vector of its own pixel, whoever won it.
  9. (rangenetAPI.cpp:62-72) prob = 0, label = 0; for j: if (prob <= logit[j]) { label = j; prob = logit[j]; } — the last of equal maxima
     wins, all-negative logits give 0, a NaN logit is never taken.

A float libm function is DEFINED as the correctly rounded value (the double function rounded once to float), as everywhere in this
repository; sqrtf and float division are exact by IEEE.  Defined where the reference is undefined: a point with a non-finite x, y, z or
intensity takes no part in the projection (pixel index -1, label 0); H * W <= 2^24 (the reference forms the index in float);
n_classes <= 32.

Two forms that must agree bit for bit: `project_literal` / `label_literal` are the loops (sort by decreasing range, assign in order; one
logit vector per point, the argmax loop), `project_parallel` / `label_parallel` the form the HIP kernels implement (a per-pixel minimum
over the key (range bits << 32 | ~index); a per-pixel argmax and a per-point gather).  The per-point arithmetic of steps 2-5 and the
per-pixel arithmetic of step 7 carry no order and are shared."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
PI = f64(math.pi)


class Params:
    """lisreg_rangenet_params"""

    def __init__(self, img_h=64, img_w=2048, fov_up=3.0, fov_down=-25.0, means=(0.0,) * 5, stds=(1.0,) * 5, n_classes=20):
        self.img_h, self.img_w, self.fov_up, self.fov_down, self.n_classes = int(img_h), int(img_w), float(fov_up), float(fov_down), int(n_classes)
        self.means, self.stds = np.asarray(means, f32), np.asarray(stds, f32)
        assert 1 <= self.img_h and 1 <= self.img_w and self.img_h * self.img_w <= 1 << 24 and 1 <= self.n_classes <= 32


def _libm(fn, *args):
    """A double libm function, element by element through the C library (as tests/pretreat_ref.py)"""
    arrs = [np.atleast_1d(np.asarray(a, f64)) for a in args]
    return np.fromiter((fn(*v) for v in zip(*[a.tolist() for a in arrs])), f64, count=len(arrs[0]))


def _asin(v):
    return math.asin(v) if -1.0 <= v <= 1.0 else math.nan               # C's asin: NaN for NaN and outside [-1, 1]


def fov(P):
    """step 1: (fabsf(fov_down), fov) as floats"""
    up = f32(f64(P.fov_up) / f64(180.0) * PI)
    down = f32(f64(P.fov_down) / f64(180.0) * PI)
    return np.abs(down), f32(np.abs(down) + np.abs(up))


def per_point(raw, P):
    """steps 2-5 for every point of an (n, 4) float32 array: dict of finite (bool), range (float32), col_raw / row_raw (floorf before the
    clamps; float32, NaN possible), pixel_index (int32, -1 for a non-finite point)"""
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4)
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    finite = np.isfinite(raw).all(1)
    fda, fv = fov(P)
    with np.errstate(all="ignore"):
        rng = np.sqrt((x * x + y * y) + z * z)                            # float32 throughout
        yaw = -_libm(math.atan2, y, x).astype(f32)
        pitch = _libm(_asin, z / rng).astype(f32)
        px = (f64(0.5) * (yaw.astype(f64) / PI + f64(1.0))).astype(f32)
        py = (f64(1.0) - ((pitch + fda) / fv).astype(f64)).astype(f32)
        col_raw = np.floor(px * f32(P.img_w))
        row_raw = np.floor(py * f32(P.img_h))
        wm1, hm1 = f32(P.img_w) - f32(1.0), f32(P.img_h) - f32(1.0)
        col = np.where(col_raw < wm1, col_raw, wm1)
        col = np.where(f32(0.0) < col, col, f32(0.0))
        row = np.where(row_raw < hm1, row_raw, hm1)
        row = np.where(f32(0.0) < row, row, f32(0.0))
    pix = (row * f32(P.img_w) + col).astype(np.int32)                   # exact: H * W <= 2^24
    pix[~finite] = -1
    return dict(finite=finite, range=rng.astype(f32), col_raw=col_raw, row_raw=row_raw, pixel_index=pix)


def _int_zero(v):
    """(int)v == 0 for the values that have an int; NaN / inf (undefined in the reference) count as non-zero"""
    with np.errstate(invalid="ignore"):
        return np.abs(v) < f32(1.0)


def _image(raw, pp, winner, P):
    """step 7 from the per-pixel winner (point index, -1: empty)"""
    hw = P.img_h * P.img_w
    has = winner >= 0
    w = np.where(has, winner, 0)
    vals = np.zeros((5, hw), f32)
    if len(raw):
        vals[0] = np.where(has, pp["range"][w], f32(0))
        for c in range(4):
            vals[c + 1] = np.where(has, raw[w, c], f32(0))
    invalid = _int_zero(vals).all(0)
    with np.errstate(all="ignore"):
        norm = ((vals - P.means[:, None]) / P.stds[:, None]).astype(f32)
    tensor = np.where(invalid[None, :], f32(0), norm).astype(f32).reshape(5, P.img_h, P.img_w)
    return dict(pixel_index=pp["pixel_index"], tensor=tensor, invalid_mask=invalid.astype(np.uint8), n_valid=int((~invalid).sum()),
                winner=winner.astype(np.int64))


def project_literal(raw, P):
    """The loops: sort by decreasing range (stable), assign in order, later assignments overwrite."""
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4)
    pp = per_point(raw, P)
    idx = [int(i) for i in np.flatnonzero(pp["finite"])]
    rng = pp["range"].tolist()
    order = sorted(idx, key=lambda i: -rng[i])                          # Python's sort is stable
    winner = [-1] * (P.img_h * P.img_w)
    pix = pp["pixel_index"].tolist()
    for i in order:
        winner[pix[i]] = i
    return _image(raw, pp, np.asarray(winner, np.int64), P)


def project_parallel(raw, P):
    """A per-pixel minimum over the key (range bits << 32 | ~index): smallest range, then highest index."""
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4)
    pp = per_point(raw, P)
    idx = np.flatnonzero(pp["finite"])
    empty = np.uint64(0xFFFFFFFFFFFFFFFF)
    keys = np.full(P.img_h * P.img_w, empty, np.uint64)
    key = (pp["range"][idx].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (~idx.astype(np.uint32)).astype(np.uint64)
    np.minimum.at(keys, pp["pixel_index"][idx], key)
    winner = np.where(keys == empty, -1, (~(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)).astype(np.int64))
    return _image(raw, pp, winner, P)


def label_literal(pixel_index, invalid_mask, logits, P):
    """One logit vector per point, the argmax loop of rangenetAPI.cpp:62-72.  Returns (labels per point, None)."""
    hw = P.img_h * P.img_w
    lg = np.ascontiguousarray(logits, f32).reshape(P.n_classes, hw)
    invalid_output = [1.0] + [0.0] * (P.n_classes - 1)
    labels = np.zeros(len(pixel_index), np.uint32)
    for i, pix in enumerate(np.asarray(pixel_index).tolist()):
        if pix < 0:
            continue                                                    # a non-finite point: label 0
        vec = invalid_output if invalid_mask[pix] else lg[:, pix].tolist()
        prob, label = 0.0, 0
        for j, v in enumerate(vec):
            if prob <= v:
                label, prob = j, v
        labels[i] = label
    return labels, None


def label_parallel(pixel_index, invalid_mask, logits, P):
    """A per-pixel argmax into the label image, a per-point gather.  Returns (labels per point, label image H x W uint8)."""
    hw = P.img_h * P.img_w
    lg = np.ascontiguousarray(logits, f32).reshape(P.n_classes, hw)
    prob, label = np.zeros(hw, f32), np.zeros(hw, np.uint8)
    for j in range(P.n_classes):
        with np.errstate(invalid="ignore"):
            take = prob <= lg[j]
        label = np.where(take, np.uint8(j), label)
        prob = np.where(take, lg[j], prob)
    label = np.where(np.asarray(invalid_mask, bool), np.uint8(0), label).astype(np.uint8)
    pix = np.asarray(pixel_index, np.int64)
    labels = np.where(pix >= 0, label[np.where(pix >= 0, pix, 0)], 0).astype(np.uint32) if len(pix) else np.zeros(0, np.uint32)
    return labels, label.reshape(P.img_h, P.img_w)


def same_projection(a, b):
    """bit-for-bit equality of two projections; the name of the first field that differs, or None"""
    for key in ("pixel_index", "invalid_mask", "winner"):
        if not np.array_equal(a[key], b[key]):
            return key
    if not np.array_equal(a["tensor"].view(np.uint32), b["tensor"].view(np.uint32)):
        return "tensor"
    return None if a["n_valid"] == b["n_valid"] else "n_valid"


def stand_in_logits(tensor, P, seed):
    """Logits without a network: a fixed seeded 5 -> n_classes linear map of the input tensor (float32, computed here on the host; the
    same array goes to the library and to the restatement, so its own rounding does not matter), with planted pixels: all-negative
    vectors, tied maxima (two and three classes), a NaN where the maximum would be, a NaN next to a tie.  Returns (logits C x H x W,
    dict of the planted pixel sets)."""
    rng = np.random.default_rng(seed)
    hw = P.img_h * P.img_w
    A = rng.normal(0, 1, (P.n_classes, 5)).astype(f32)
    b = rng.normal(0, 0.5, P.n_classes).astype(f32)
    with np.errstate(all="ignore"):
        lg = (A @ tensor.reshape(5, hw).astype(f32) + b[:, None]).astype(f32)
    pick = rng.permutation(hw)[: min(hw, 400)]
    parts = np.array_split(pick, 4)
    planted = dict(negative=parts[0], tie=parts[1], nan_max=parts[2], nan_tie=parts[3])
    lg[:, parts[0]] = -np.abs(np.nan_to_num(lg[:, parts[0]], nan=1.0, posinf=1.0, neginf=-1.0)) - f32(0.25)
    C = P.n_classes
    for k, p in enumerate(parts[1]):
        top = f32(np.nanmax(np.where(np.isfinite(lg[:, p]), lg[:, p], f32(0))) + f32(1.0))
        cls = rng.choice(C, size=min(C, 2 + k % 2), replace=False)
        lg[cls, p] = top
    for p in parts[2]:
        col = np.where(np.isfinite(lg[:, p]), lg[:, p], -np.inf)
        lg[int(np.argmax(col)), p] = np.nan
    for p in parts[3]:
        top = f32(np.nanmax(np.where(np.isfinite(lg[:, p]), lg[:, p], f32(0))) + f32(2.0))
        cls = rng.choice(C, size=min(C, 3), replace=False)
        lg[cls[:-1], p] = top
        lg[cls[-1], p] = np.nan
    return lg.reshape(C, P.img_h, P.img_w), planted


def inject(raw, seed, P):
    """The cases that decide results, appended to / scattered over a sweep: duplicated points (exact range ties in one pixel, different
    intensities), points at the origin, near points of range < 1 with |intensity| < 1 (a non-empty invalid pixel) and with intensity
    >= 1 (a valid one), elevations above and below the field of view, x < 0 with y = +0 / -0 (the yaw seam), non-finite points."""
    rng = np.random.default_rng(seed)
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4).copy()
    extra = []
    dup = raw[rng.integers(0, len(raw), 12)].copy()                     # later copies: higher index, other intensity
    dup[:, 3] = rng.uniform(2.0, 3.0, len(dup)).astype(f32)
    extra.append(dup)
    extra.append(np.array([[0, 0, 0, 0.5], [0, 0, 0, 3.0], [0, 0, 0, 0.25]], f32))             # the last one wins: invalid pixel
    az = rng.uniform(-3.0, 3.0, 8)
    el = np.radians(rng.uniform(-20.0, 0.0, 8))
    r = rng.uniform(0.2, 0.9, 8)
    near = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el), np.where(np.arange(8) % 2 == 0, 0.3, 4.0)], 1).astype(f32)
    extra.append(near)
    for deg in (12.0, 35.0, -33.0, -60.0, 90.0, -90.0):                # outside 3 .. -25 degrees (and straight up / down)
        e, a, d = np.radians(deg), rng.uniform(-3.0, 3.0), rng.uniform(5.0, 30.0)
        extra.append(np.array([[d * np.cos(e) * np.cos(a), d * np.cos(e) * np.sin(a), d * np.sin(e), 0.7]], f32))
    seam = np.array([[-7.0, 0.0, -0.5, 0.4], [-7.5, -0.0, -0.5, 0.4], [-9.0, -0.0, -1.0, 0.6], [-9.5, 0.0, -1.0, 0.6]], f32)
    extra.append(seam)
    out = np.concatenate([raw] + extra)
    out = out[rng.permutation(len(out))]
    m = len(out)
    for val, cnt in ((np.nan, 5), (np.inf, 3), (-np.inf, 2)):
        out[rng.integers(0, m, cnt), rng.integers(0, 4, cnt)] = val      # the intensity too
    return np.ascontiguousarray(out, f32)
