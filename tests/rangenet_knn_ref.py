"""CPU restatement of the kNN label clean-up of RangeNet++ — the yardstick of lisreg_rangenet_label_knn (tests/test_rangenet_knn.py).

The reference tree has no text for this step (its vendored wrapper never reads the `post: KNN: params:` block of the model's
arch_cfg.yaml), so it is DEFINED here and at the kNN section of lis-slam_amd/csrc/lisreg_rangenet.hip, after the authors' published
post-processing, restated from knowledge.  With S = search, C = n_classes, window cell j = 0 .. S*S - 1 at row offset
j // S - (S - 1) // 2 and column offset j % S - (S - 1) // 2:

  1. Label image: steps 8-9 of tests/rangenet_ref.py (label_parallel); invalid pixels are 0.
  2. Range image: per pixel the smallest range = sqrtf((x*x + y*y) + z*z) in float (the projection's expression: the winner's range bit
     for bit) over the points with that pixel_index; points with pixel_index -1 take no part; a pixel no point fell into has range
     +inf.  The invalid mask plays no part in the range image.
  3. Weights: g_j = exp(-(dx*dx + dy*dy) / (2 sigma^2)) in double through the C library's exp, summed in the order of j;
     w_j = (float)(1.0 - g_j / sum g), rounded once.
  4. Per point with pixel_index >= 0 and a finite own range r: every window cell takes range and label of its pixel; a cell outside the
     image takes range 0 and label 0 (zero padding in rows and columns, no wrap at the azimuth seam); the centre cell's range is replaced
     by r, its label stays the pixel's.  d_j = fabsf(range_j - r) * w_j in float: +inf for an empty pixel, never NaN.
  5. Selection: the knn cells smallest in (d_j, then j): a tie in d goes to the lower window position.
  6. Vote: a selected cell with cutoff > 0 and d_j > cutoff votes for nobody, every other selected cell for its label.
  7. Result: the class in 1 .. C - 1 with the most votes, lowest id on a tie; class 0 never wins; a point with no vote for any class
     1 .. C - 1 gets no_vote_label (1: the authors' argmax + 1 over all-zero counts; 0, the default: the outlier class).
  8. A point with pixel_index -1 gets 0; a point whose own range is not finite keeps its pixel's label of step 1.

Limits: search in {1, 3, 5, 7}; 1 <= knn <= min(search^2, 16); sigma finite and > 0; 0 <= no_vote_label < C; C >= 2.

Three forms that must agree: `knn_literal` (a loop per point, a stable sort over (d, j)), `knn_parallel` (the form the HIP kernels take:
the range image by np.minimum.at on the bit patterns, a vectorised gather, selection and vote) and `knn_torch` (F.unfold with zero
padding, topk(largest=False), scatter_add_, on the same weight table; torch.topk does not define its tie order, so it is only used on
inputs for which `boundary_ties` is 0)."""
import math

import numpy as np

import rangenet_ref as R

f32, f64 = np.float32, np.float64
INF_BITS = np.uint32(0x7F800000)


class Knn:
    """lisreg_rangenet_knn_params"""

    def __init__(self, knn=5, search=5, sigma=1.0, cutoff=1.0, no_vote_label=0):
        self.knn, self.search, self.sigma, self.cutoff, self.no_vote_label = int(knn), int(search), f32(sigma), f32(cutoff), int(no_vote_label)
        assert self.search in (1, 3, 5, 7) and 1 <= self.knn <= min(self.search ** 2, 16)
        assert np.isfinite(self.sigma) and self.sigma > 0 and self.no_vote_label >= 0


def offsets(S):
    """(row offsets, column offsets) of the window cells j = 0 .. S*S - 1"""
    j = np.arange(S * S)
    return j // S - (S - 1) // 2, j % S - (S - 1) // 2


def weights(K):
    """step 3: the S*S float32 weights"""
    dy, dx = offsets(K.search)
    s = float(K.sigma)                                                   # the float's value as a double
    g = [math.exp(-float(x * x + y * y) / (2.0 * s * s)) for y, x in zip(dy.tolist(), dx.tolist())]
    total = 0.0
    for v in g:
        total += v
    return np.array([1.0 - v / total for v in g], f64).astype(f32)


def point_range(raw):
    """sqrtf((x*x + y*y) + z*z) in float32"""
    raw = np.ascontiguousarray(raw, f32).reshape(-1, 4)
    x, y, z = raw[:, 0], raw[:, 1], raw[:, 2]
    with np.errstate(all="ignore"):
        return np.sqrt((x * x + y * y) + z * z).astype(f32)


def range_image(raw, pixel_index, P):
    """step 2 the way the kernels do it: a per-pixel minimum over the bit patterns (non-negative floats order like their bits)"""
    pix = np.asarray(pixel_index, np.int64)
    img = np.full(P.img_h * P.img_w, INF_BITS, np.uint32)
    sel = pix >= 0
    np.minimum.at(img, pix[sel], point_range(raw)[sel].view(np.uint32))
    return img.view(f32).reshape(P.img_h, P.img_w)


def range_image_literal(raw, pixel_index, P):
    """step 2 as a loop over the points"""
    img = [math.inf] * (P.img_h * P.img_w)
    for pix, r in zip(np.asarray(pixel_index).tolist(), point_range(raw).tolist()):
        if pix >= 0 and r < img[pix]:
            img[pix] = r
    return np.array(img, f32).reshape(P.img_h, P.img_w)


def _check(P, K):
    assert P.n_classes >= 2 and K.no_vote_label < P.n_classes


def knn_literal(raw, pixel_index, invalid_mask, logits, P, K):
    """The loop per point.  Returns (labels per point uint32, label image H x W uint8, range image H x W float32)."""
    _check(P, K)
    _, image = R.label_parallel(pixel_index, invalid_mask, logits, P)
    rimg = range_image_literal(raw, pixel_index, P)
    S, H, W, C = K.search, P.img_h, P.img_w, P.n_classes
    dy, dx = offsets(S)
    w = weights(K)
    own = point_range(raw)
    labels = np.zeros(len(own), np.uint32)
    for i, pix in enumerate(np.asarray(pixel_index).tolist()):
        if pix < 0:
            continue
        y0, x0 = divmod(pix, W)
        if not np.isfinite(own[i]):
            labels[i] = image[y0, x0]
            continue
        r = own[i]
        cells = []
        for j in range(S * S):
            y, x = y0 + int(dy[j]), x0 + int(dx[j])
            inside = 0 <= y < H and 0 <= x < W
            rj = rimg[y, x] if inside else f32(0.0)
            lj = int(image[y, x]) if inside else 0
            if j == (S * S) // 2:
                rj = r
            with np.errstate(all="ignore"):
                d = f32(np.abs(f32(rj - r)) * w[j])
            cells.append((float(d), j, lj))
        cells.sort(key=lambda c: c[0])                                   # Python's sort is stable: ties stay in order of j
        votes = [0] * C
        for d, j, lj in cells[: K.knn]:
            if K.cutoff > 0 and d > float(K.cutoff):
                continue
            votes[lj] += 1
        best, best_n = K.no_vote_label, 0
        for c in range(1, C):
            if votes[c] > best_n:
                best, best_n = c, votes[c]
        labels[i] = best
    return labels, image, rimg


def window(raw, pixel_index, image, rimg, P, K):
    """steps 4 for all points at once: (D (n, S*S) float32, L (n, S*S) int64, usable (n,) bool: pixel_index >= 0 and finite own range)"""
    S, H, W = K.search, P.img_h, P.img_w
    dy, dx = offsets(S)
    pix = np.asarray(pixel_index, np.int64)
    own = point_range(raw)
    safe = np.where(pix >= 0, pix, 0)
    Y, X = (safe // W)[:, None] + dy[None, :], (safe % W)[:, None] + dx[None, :]
    inside = (Y >= 0) & (Y < H) & (X >= 0) & (X < W)
    flat = np.where(inside, Y * W + X, 0)
    Rw = np.where(inside, rimg.ravel()[flat], f32(0.0)).astype(f32)
    L = np.where(inside, image.ravel()[flat], 0).astype(np.int64)
    Rw[:, (S * S) // 2] = own
    with np.errstate(all="ignore"):
        D = (np.abs(Rw - own[:, None]) * weights(K)[None, :]).astype(f32)
    return D, L, (pix >= 0) & np.isfinite(own)


def knn_parallel(raw, pixel_index, invalid_mask, logits, P, K):
    """The form the kernels take.  Returns (labels, label image, range image)."""
    _check(P, K)
    _, image = R.label_parallel(pixel_index, invalid_mask, logits, P)
    rimg = range_image(raw, pixel_index, P)
    pix = np.asarray(pixel_index, np.int64)
    n, C = len(pix), P.n_classes
    if n == 0:
        return np.zeros(0, np.uint32), image, rimg
    D, L, usable = window(raw, pixel_index, image, rimg, P, K)
    order = np.argsort(np.where(np.isnan(D), f32(np.inf), D), axis=1, kind="stable")[:, : K.knn]      # (d, then j)
    d_sel, l_sel = np.take_along_axis(D, order, 1), np.take_along_axis(L, order, 1)
    voting = ~((K.cutoff > 0) & (d_sel > K.cutoff))
    votes = np.zeros((n, C), np.int64)
    for a in range(K.knn):
        np.add.at(votes, (np.arange(n)[voting[:, a]], l_sel[voting[:, a], a]), 1)
    top = votes[:, 1:].argmax(1) + 1                                     # the first maximum: the lowest class id
    voted = np.where(votes[:, 1:].max(1) > 0, top, K.no_vote_label)
    own_pixel = np.where(pix >= 0, image.ravel()[np.where(pix >= 0, pix, 0)], 0)
    return np.where(usable, voted, own_pixel).astype(np.uint32), image, rimg


def boundary_ties(raw, pixel_index, invalid_mask, logits, P, K):
    """The points for which the order of equal distances decides the vote: the knn-th and (knn+1)-th smallest d are equal and finite, and
    the cells of that distance carry different labels.  (Rows of unusable points count too: their windows are formed all the same.)"""
    if K.knn >= K.search ** 2 or len(pixel_index) == 0:
        return 0
    _, image = R.label_parallel(pixel_index, invalid_mask, logits, P)
    D, L, usable = window(raw, pixel_index, image, range_image(raw, pixel_index, P), P, K)
    Ds = np.sort(np.where(np.isnan(D), f32(np.inf), D), axis=1)
    dk = Ds[:, K.knn - 1]
    tied = (dk == Ds[:, K.knn]) & np.isfinite(dk)
    group = D == dk[:, None]
    lmax, lmin = np.where(group, L, -1).max(1), np.where(group, L, 1 << 30).min(1)
    return int((usable & tied & (lmax != lmin)).sum())


def knn_torch(raw, pixel_index, invalid_mask, logits, P, K):
    """The independent form, shaped like the authors' module: unfold the range and label images with zero padding, take each point's
    column, topk of the weighted distances, scatter_add_ of ones into a (C + 1) x n vote table whose extra row collects the cells beyond
    the cutoff.  Returns the labels."""
    import torch
    import torch.nn.functional as F
    _check(P, K)
    _, image = R.label_parallel(pixel_index, invalid_mask, logits, P)
    rimg = range_image(raw, pixel_index, P)
    S, C = K.search, P.n_classes
    pix = torch.from_numpy(np.asarray(pixel_index, np.int64))
    own = torch.from_numpy(point_range(raw))
    usable = (pix >= 0) & torch.isfinite(own)
    idx = pix[usable]
    r = own[usable]
    pad = (S - 1) // 2
    un_r = F.unfold(torch.from_numpy(rimg.copy())[None, None], kernel_size=(S, S), padding=(pad, pad))[0]          # S*S x H*W
    un_l = F.unfold(torch.from_numpy(image.astype(np.float32))[None, None], kernel_size=(S, S), padding=(pad, pad))[0]
    win_r, win_l = un_r[:, idx].clone(), un_l[:, idx].long()
    win_r[(S * S) // 2] = r
    d = torch.abs(win_r - r[None, :]) * torch.from_numpy(weights(K))[:, None]
    d_sel, j_sel = d.topk(K.knn, dim=0, largest=False)
    l_sel = torch.gather(win_l, 0, j_sel)
    if K.cutoff > 0:
        l_sel = torch.where(d_sel > float(K.cutoff), torch.full_like(l_sel, C), l_sel)
    votes = torch.zeros((C + 1, len(idx)), dtype=torch.int64)
    votes.scatter_add_(0, l_sel, torch.ones_like(l_sel))
    body = votes[1:C]
    voted = torch.where(body.max(0).values > 0, body.argmax(0) + 1, torch.full((len(idx),), K.no_vote_label, dtype=torch.int64))
    out = np.where(np.asarray(pixel_index) >= 0, image.ravel()[np.where(np.asarray(pixel_index) >= 0, pixel_index, 0)], 0).astype(np.uint32)
    out[usable.numpy()] = voted.numpy().astype(np.uint32)
    return out
