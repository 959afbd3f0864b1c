"""The kNN label clean-up of RangeNet++ (lisreg_rangenet_label_knn): a vote among the knn cells of a search x search window of the range
image that are nearest to the point in range.

The yardstick is tests/rangenet_knn_ref.py, where the step is defined: its literal form (a loop per point, a stable sort over (d, j)),
the form the HIP kernels take (a range image by a minimum over bit patterns, a vectorised selection and vote) and an independent torch
form (F.unfold, topk, scatter_add_) must agree (CPU tests), hand-written planted cases pin down every rule of the definition, and the
library must equal the restatement for single calls, in a batch, between other RangeNet++ calls on one context and on a caller's busy
stream (GPU tests).  Every comparison is exact: integer labels equal, floats bit-equal; no tolerance anywhere."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import pretreat_ref as PR
import rangenet_knn_ref as KR
import rangenet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rangenet", "rangenet_knn_16x128.npz")
MEANS = (12.12, 10.88, 0.23, -1.04, 0.21)
STDS = (12.32, 11.47, 6.91, 0.86, 0.16)
# (knn, search, sigma, cutoff): the defaults, a small window, the largest window without a cutoff, and knn = 1.  make_sweep plants points
# of exactly equal range (its 90 m returns), so with knn = 1 and a window of more than one cell the first and second place tie at d = 0
# between cells of different labels: a DEFINED tie, which the literal and the kernel form (and the library) must resolve alike, but which
# torch.topk does not define.  The torch form therefore takes knn = 1 with search = 1, the other two forms also knn = 1 with search = 5.
SETS = ((5, 5, 1.0, 1.0), (3, 3, 0.5, 0.5), (7, 7, 2.0, 0.0), (1, 1, 1.0, 1.0))
TIED_SET = (1, 5, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def seeded(which):
    """The seeded sweeps with the injected deciding cases, projected by the restatement, with stand-in logits: 16 x 128 (seed 301) and
    32 x 1024 (seed 302).  Cached and never modified."""
    seed, h, w, ns, n_az, fov, order = {"16x128": (301, 16, 128, 16, 200, (15.0, -15.0), "shuffled"),
                                        "32x1024": (302, 32, 1024, 32, 110, (10.67, -30.67), "time")}[which]
    P = R.Params(h, w, fov[0], fov[1], MEANS, STDS, 20)
    raw = R.inject(PR.make_sweep(seed, ns, order, n_az=n_az), seed, P)
    ref = R.project_parallel(raw, P)
    lg, _ = R.stand_in_logits(ref["tensor"], P, 7000 + seed)
    for a in (raw, ref["pixel_index"], ref["invalid_mask"], lg):
        a.setflags(write=False)
    return dict(raw=raw, P=P, pix=ref["pixel_index"], mask=ref["invalid_mask"], lg=lg)


def _args(c):
    return c["raw"], c["pix"], c["mask"], c["lg"], c["P"]


@functools.lru_cache(maxsize=None)
def seeded_want(which, kset, no_vote):
    c = seeded(which)
    return KR.knn_parallel(*_args(c), KR.Knn(*kset, no_vote))


# ---- planted cases: a few pixels each, the expected labels written out by hand ----------------------------------------------------
def scene(h, w, n_classes, pixel_labels, points, invalid=()):
    """pixel_labels: {(row, col): class}; every other pixel gets all-negative logits (label 0).  points: [((row, col) or None, range)],
    a point at (range, 0, 0) so that its float range is `range` exactly; None: pixel index -1."""
    P = R.Params(h, w, n_classes=n_classes)
    lg = np.full((n_classes, h, w), -1.0, np.float32)
    for (y, x), c in pixel_labels.items():
        lg[c, y, x] = 1.0
    mask = np.zeros(h * w, np.uint8)
    for (y, x) in invalid:
        mask[y * w + x] = 1
    raw = np.zeros((len(points), 4), np.float32)
    pix = np.zeros(len(points), np.int32)
    for i, (at, r) in enumerate(points):
        raw[i] = (r, 0.0, 0.0, 0.5)
        pix[i] = -1 if at is None else at[0] * w + at[1]
    return raw, pix, mask, lg, P


def planted_cases():
    """[(name, (raw, pix, mask, lg, P), Knn, expected labels)]"""
    out = []
    # S = 3, sigma = 1: the edge cells (j = 1, 3, 5, 7) share one weight, the corner cells another
    # an exact tie in d at the knn-th place between j = 3 (class 2) and j = 5 (class 3): the lower j is selected
    s = scene(3, 3, 4, {(1, 0): 2, (1, 2): 3}, [((1, 1), 10.0), ((1, 0), 12.0), ((1, 2), 12.0)])
    out.append(("tie_at_kth_place", s, KR.Knn(2, 3, 1.0, 0.0, 0), [2, 2, 3]))
    # one vote for class 3 (the centre) and one for class 1: the lower id wins
    s = scene(3, 3, 4, {(1, 1): 3, (1, 0): 1}, [((1, 1), 10.0), ((1, 0), 10.5)])
    out.append(("vote_tie_lower_id", s, KR.Knn(2, 3, 1.0, 0.0, 0), [1, 1]))
    # the centre's pixel is labelled 0 and both neighbours lie beyond the cutoff: nobody votes
    pts = [((1, 1), 10.0), ((1, 0), 20.0), ((1, 2), 30.0)]
    for nv in (0, 1):
        s = scene(3, 3, 4, {(1, 0): 2, (1, 2): 2}, pts)
        out.append((f"all_beyond_cutoff_no_vote_{nv}", s, KR.Knn(3, 3, 1.0, 0.5, nv), [nv, 2, 2]))
    s = scene(3, 3, 4, {(1, 0): 2, (1, 2): 2}, pts)
    out.append(("same_scene_without_cutoff", s, KR.Knn(3, 3, 1.0, 0.0, 0), [2, 2, 2]))
    # every vote goes to class 0: an invalid pixel whose logits say class 3, and a pixel of all-negative logits
    for nv in (0, 1):
        s = scene(3, 3, 4, {(1, 1): 3}, [((1, 1), 10.0), ((1, 0), 10.25)], invalid=[(1, 1)])
        out.append((f"all_votes_for_class_0_no_vote_{nv}", s, KR.Knn(2, 3, 1.0, 0.0, nv), [nv, nv]))
    # windows over the four corners and two edges of a 4 x 6 image: the cells outside are zero padding (range 0, label 0) — a wrap at the
    # azimuth seam or over the rows would bring in the other corners at d = 0, a flat index pix + 1 the pixel (1, 0)
    s = scene(4, 6, 8, {(0, 0): 3, (0, 5): 2, (3, 0): 4, (3, 5): 5, (0, 3): 6, (1, 0): 7},
              [((0, 0), 0.5), ((0, 5), 0.5), ((3, 0), 0.5), ((3, 5), 0.5), ((0, 3), 0.5), ((1, 0), 0.5)])
    out.append(("edges_and_corners", s, KR.Knn(3, 3, 1.0, 0.0, 0), [3, 2, 4, 5, 6, 3]))
    # an image smaller than the window: 2 x 8 with search 5
    s = scene(2, 8, 4, {(0, 3): 1, (1, 3): 2, (0, 4): 2}, [((0, 3), 5.0), ((1, 3), 5.2), ((0, 4), 5.1)])
    out.append(("image_smaller_than_window", s, KR.Knn(5, 5, 1.0, 0.0, 0), [2, 2, 2]))
    # search = 1: the point's own pixel votes alone
    for nv in (0, 1):
        s = scene(2, 2, 4, {(0, 0): 3}, [((0, 0), 4.0), ((0, 1), 4.0), ((0, 0), 9.0)])
        out.append((f"search_1_no_vote_{nv}", s, KR.Knn(1, 1, 1.0, 1.0, nv), [3, nv, 3]))
    # a wall point (class 13, 20.1 m) seen past a pole (class 18, 5 m) that won its pixel, the wall on both sides at 20 m
    labels = {(y, 2): 18 for y in range(3)}
    labels.update({(y, x): 13 for y in range(3) for x in (1, 3)})
    pts = [((y, 2), 5.0) for y in range(3)] + [((y, x), 20.0) for y in range(3) for x in (1, 3)] + [((1, 2), 20.125)]
    s = scene(3, 5, 20, labels, pts)
    out.append(("lost_pixel_between_two_surfaces", s, KR.Knn(3, 3, 1.0, 1.0, 0), [18] * 3 + [13] * 6 + [13]))
    # finite coordinates whose squares overflow: the point keeps its pixel's label; its neighbour sees an empty (+inf) pixel, never a NaN
    s = scene(3, 3, 6, {(1, 1): 4, (1, 0): 2}, [((1, 1), 3.0e38), ((1, 0), 10.0)])
    s[0][0, 1] = 3.0e38
    out.append(("overflowing_range", s, KR.Knn(2, 3, 1.0, 0.0, 1), [4, 2]))
    # a point the projection left out (pixel index -1) gets 0, its coordinates pass bit for bit
    s = scene(3, 3, 4, {(1, 1): 2}, [((1, 1), 10.0), (None, 10.0)])
    s[0][1, :3] = (np.nan, -np.inf, 7.0)
    out.append(("pixel_index_minus_one", s, KR.Knn(2, 3, 1.0, 0.0, 1), [2, 0]))
    return out


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_literal_form_equals_kernel_form():
    for which in ("16x128", "32x1024"):
        c = seeded(which)
        assert (c["P"].img_h, c["P"].img_w) == tuple(int(v) for v in which.split("x"))
        plain, image = R.label_parallel(c["pix"], c["mask"], c["lg"], c["P"])
        for kset in SETS + (TIED_SET,):
            for nv in (0, 1):
                K = KR.Knn(*kset, nv)
                a, img_a, rng_a = KR.knn_literal(*_args(c), K)
                b, img_b, rng_b = seeded_want(which, kset, nv)
                assert np.array_equal(a, b), (which, kset, nv, int((a != b).sum()))
                assert np.array_equal(img_a, image) and np.array_equal(img_b, image)
                assert np.array_equal(rng_a.view(np.uint32), rng_b.view(np.uint32)), (which, kset)
                assert (a[c["pix"] < 0] == 0).all() and a.max() < c["P"].n_classes
        # the range image is the projection winner's range, bit for bit, and +inf where no point fell
        proj = R.project_parallel(c["raw"], c["P"])
        won = proj["winner"] >= 0
        rimg = seeded_want(which, SETS[0], 0)[2].ravel()
        assert np.array_equal(rimg[won].view(np.uint32), KR.point_range(c["raw"])[proj["winner"][won]].view(np.uint32))
        assert np.isposinf(rimg[~won]).all() and (~won).sum() > 0
    c = seeded("16x128")
    print("points:", len(c["raw"]), len(seeded("32x1024")["raw"]))
    assert (len(c["raw"]), len(seeded("32x1024")["raw"])) == (3233, 3553)
    # the clean-up does something, and the defined tie occurs where knn = 1 meets a wider window
    plain, _ = R.label_parallel(c["pix"], c["mask"], c["lg"], c["P"])
    changed = int((seeded_want("16x128", SETS[0], 0)[0] != plain).sum())
    print("labels changed by the defaults on 16 x 128:", changed, "of", len(plain))
    assert changed > 0
    assert KR.boundary_ties(*_args(c), KR.Knn(*TIED_SET, 0)) > 0


TORCH_FORM = """
import sys
sys.path.insert(0, {tests!r})
import numpy as np
import rangenet_knn_ref as KR
import rangenet_ref as R
z = np.load({inp!r})
out = dict()
for which in ("16x128", "32x1024"):
    h, w = (int(v) for v in which.split("x"))
    P = R.Params(h, w, n_classes=int(z[which + "_lg"].shape[0]))
    for k, kset in enumerate({sets!r}):
        for nv in (0, 1):
            out["%s_%d_%d" % (which, k, nv)] = KR.knn_torch(z[which + "_raw"], z[which + "_pix"], z[which + "_mask"], z[which + "_lg"], P,
                                                          KR.Knn(*kset, nv))
np.savez({outp!r}, **out)
print("FORM_DONE")
"""


def _have_torch():
    try:
        import importlib.util
        return importlib.util.find_spec("torch") is not None
    except Exception:
        return False


@pytest.mark.skipif(not _have_torch(), reason="torch not installed")
def test_torch_form_equals_literal_form(tmp_path):
    """The independent torch form (unfold, topk, scatter_add_) on the CPU, in a fresh interpreter: the suite's own process does not
    import torch (tests/test_teardown.py).  torch.topk leaves the order of equal values open, so the inputs it is given carry no point
    whose knn-th and (knn+1)-th distances tie between cells of different labels: asserted first."""
    data = dict()
    for which in ("16x128", "32x1024"):
        c = seeded(which)
        for kset in SETS:
            n_ties = KR.boundary_ties(*_args(c), KR.Knn(*kset, 0))
            print(which, kset, "ties that decide a vote:", n_ties)
            assert n_ties == 0, (which, kset)
        data.update({which + "_raw": c["raw"], which + "_pix": c["pix"], which + "_mask": c["mask"], which + "_lg": c["lg"]})
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    np.savez(inp, **data)
    code = textwrap.dedent(TORCH_FORM.format(tests=os.path.join(ROOT, "tests"), inp=inp, outp=outp, sets=SETS))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert "FORM_DONE" in r.stdout and r.returncode == 0, f"exit status {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
    got = np.load(outp)
    for which in ("16x128", "32x1024"):
        for k, kset in enumerate(SETS):
            for nv in (0, 1):
                want = KR.knn_literal(*_args(seeded(which)), KR.Knn(*kset, nv))[0]
                assert np.array_equal(got["%s_%d_%d" % (which, k, nv)], want), (which, kset, nv)


def test_planted_cases_give_the_labels_written_by_hand():
    names = [name for name, _, _, _ in planted_cases()]
    assert len(names) == len(set(names)) >= 14
    for name, s, K, want in planted_cases():
        got, _, _ = KR.knn_literal(*s, K)
        assert got.tolist() == want, (name, got.tolist(), want)
        assert KR.knn_parallel(*s, K)[0].tolist() == want, name


def test_weights_equal_the_restatement_to_the_bit():
    import lisreg
    for search in (1, 3, 5, 7):
        for sigma in (1.0, 0.5, 2.0, 0.1, 1e-3, 37.5, 3.0e38, 1e-30):
            K = lisreg.default_rangenet_knn_params()
            K.search, K.sigma = search, sigma
            got = lisreg.rangenet_knn_weights(K)
            want = KR.weights(KR.Knn(1, search, sigma))
            assert got.shape == (search * search,) and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (search, sigma, got, want)
            assert (got >= 0).all() and (got <= 1).all() and got[(search * search) // 2] == got.min()
    assert np.array_equal(KR.weights(KR.Knn(1, 1, 1.0)), np.zeros(1, np.float32))
    w = KR.weights(KR.Knn(5, 5, 1.0)).reshape(5, 5)
    assert np.array_equal(w, w.T) and np.array_equal(w, w[::-1]) and w[0, 0] == w.max()
    # out of range: nothing is written
    buf = np.full(49, -3.0, np.float32)
    for search, sigma in ((2, 1.0), (9, 1.0), (5, 0.0), (5, -1.0), (5, np.nan), (5, np.inf)):
        K = lisreg.RangenetKnnParams(5, search, sigma, 1.0, 0)
        lisreg.lib().lisreg_rangenet_knn_weights(C.byref(K), buf.ctypes.data_as(C.POINTER(C.c_float)))
        assert (buf == -3.0).all(), (search, sigma)
        with pytest.raises(lisreg.LisregError):
            lisreg.rangenet_knn_weights(K)


def _header_struct(name):
    """ctypes mirror of `typedef struct <name> { ... }` as include/lisreg.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int": C.c_int, "float": C.c_float, "double": C.c_double}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"(\w+)\s+(.*)", decl).groups()
        fields += [(n.strip(), types[t]) for n in names.split(",")]
    return type(name, (C.Structure,), {"_fields_": fields})


def test_abi_declares_knn_and_struct_matches_header():
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    for sym, ret in (("lisreg_default_rangenet_knn_params", "int"), ("lisreg_rangenet_knn_weights", "void"), ("lisreg_rangenet_label_knn", "int"),
                     ("lisreg_rangenet_label_knn_batch", "int")):
        assert re.search(r"^\s*%s\s+%s\s*\(" % (ret, sym), hdr, re.M), sym
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym)
    assert ("int lisreg_rangenet_label_knn(lisreg_ctx* ctx, const void* cloud, int n, int fmt, const int* pixel_index, const unsigned char* "
            "invalid_mask, const float* logits, const lisreg_rangenet_params* params, const lisreg_rangenet_knn_params* knn_params, void* "
            "labelled_out, unsigned char* label_image_out);") in flat
    assert ("int lisreg_rangenet_label_knn_batch(lisreg_ctx* ctx, int n_sweeps, const void* const* sweeps, const int* n, const int* const* "
            "pixel_index, const unsigned char* const* invalid_mask, const float* const* logits, const lisreg_rangenet_params* params, const "
            "lisreg_rangenet_knn_params* knn_params, void* const* labelled_out, unsigned char* const* label_image_out);") in flat
    assert "void lisreg_rangenet_knn_weights(const lisreg_rangenet_knn_params* knn_params, float* out );" in flat
    theirs = _header_struct("lisreg_rangenet_knn_params")
    mine = lisreg.RangenetKnnParams
    assert [n for n, _ in mine._fields_] == ["knn", "search", "sigma", "cutoff", "no_vote_label"]
    assert [(n, t, getattr(mine, n).offset) for n, t in mine._fields_] == [(n, t, getattr(theirs, n).offset) for n, t in theirs._fields_]
    assert C.sizeof(mine) == C.sizeof(theirs) == 20
    p = lisreg.default_rangenet_knn_params()
    assert (p.knn, p.search, p.sigma, p.cutoff, p.no_vote_label) == (5, 5, 1.0, 1.0, 0)
    L = lisreg.lib()
    rp = lisreg.default_rangenet_params()
    assert L.lisreg_default_rangenet_knn_params(None) == lisreg.ERR_ARG
    assert L.lisreg_rangenet_label_knn(None, None, 0, lisreg.FMT_DEVICE_XYZI, None, None, None, C.byref(rp), C.byref(p), None, None) == lisreg.ERR_ARG
    assert L.lisreg_rangenet_label_knn_batch(None, 0, None, None, None, None, None, C.byref(rp), C.byref(p), None, None) == lisreg.ERR_ARG
    for name in ("rangenet_label_knn_device", "rangenet_label_knn_batch_device"):
        assert callable(getattr(lisreg.Context, name))


def test_golden_case_reproduces():
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 100 * 1024 and len(g["raw"]) <= 4000
    sibling = np.load(os.path.join(os.path.dirname(GOLDEN), "rangenet_16x128.npz"))                # the logits are stored there only
    assert np.array_equal(sibling["raw"].view(np.uint32), g["raw"].view(np.uint32)) and np.array_equal(sibling["labels"], g["labels"])
    logits = sibling["logits"]
    P = R.Params(16, 128, float(g["fov"][0]), float(g["fov"][1]), g["means"], g["stds"], int(logits.shape[0]))
    proj = R.project_parallel(g["raw"], P)
    assert np.array_equal(proj["pixel_index"], g["pixel_index"]) and np.array_equal(proj["invalid_mask"], g["invalid_mask"])
    k = g["knn_params"]
    K = KR.Knn(int(k[0]), int(k[1]), float(k[2]), float(k[3]), int(k[4]))
    assert (K.knn, K.search, float(K.sigma), float(K.cutoff), K.no_vote_label) == (5, 5, 1.0, 1.0, 0)
    for form in (KR.knn_literal, KR.knn_parallel):
        labels, image, rimg = form(g["raw"], g["pixel_index"], g["invalid_mask"], logits, P, K)
        assert np.array_equal(labels, g["knn_labels"]), form.__name__
        assert np.array_equal(image, g["label_image"]) and np.array_equal(rimg.view(np.uint32), g["range_image"].view(np.uint32))
    assert (g["knn_labels"] != g["labels"]).sum() > 0 and len(np.unique(g["knn_labels"])) >= 5


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _cparams(P):
    import lisreg
    p = lisreg.default_rangenet_params(P.img_h, P.img_w)
    p.fov_up, p.fov_down, p.n_classes = P.fov_up, P.fov_down, P.n_classes
    for k in range(5):
        p.means[k], p.stds[k] = float(P.means[k]), float(P.stds[k])
    return p


def _cknn(K):
    import lisreg
    return lisreg.RangenetKnnParams(K.knn, K.search, float(K.sigma), float(K.cutoff), K.no_vote_label)


class Uploaded:
    """a sweep, its pixel indices, mask and logits in device memory"""

    def __init__(self, raw, pix, mask, lg):
        import lisreg
        self.n = len(raw)
        self.raw = np.ascontiguousarray(raw, np.float32).reshape(-1, 4)
        self.din = lisreg.DeviceArray(self.raw if self.n else np.zeros((1, 4), np.float32))
        self.pix = lisreg.DeviceArray(np.ascontiguousarray(pix, np.int32) if self.n else np.zeros(1, np.int32))
        self.mask = lisreg.DeviceArray(np.ascontiguousarray(mask, np.uint8))
        self.lg = lisreg.DeviceArray(np.ascontiguousarray(lg, np.float32))


def _run(ctx, u, P, K, fmt=None, image=True):
    """one lisreg_rangenet_label_knn call into sentinel-filled outputs: (records (n, 4), label image or None)"""
    import lisreg
    out = lisreg.DeviceArray(np.full((max(u.n, 1), 4), -7.5, np.float32))
    img = lisreg.DeviceArray(np.full(P.img_h * P.img_w, 0xEE, np.uint8)) if image else None
    ctx.rangenet_label_knn_device(u.din.ptr, u.n, u.pix.ptr, u.mask.ptr, u.lg.ptr, _cparams(P), _cknn(K), out.ptr, img.ptr if image else None,
                                  fmt=lisreg.FMT_DEVICE_XYZI if fmt is None else fmt)
    rec = lisreg.device_to_host(out.ptr, (max(u.n, 1), 4), np.float32)[: u.n]
    return rec, (lisreg.device_to_host(img.ptr, (P.img_h, P.img_w), np.uint8) if image else None)


def _check(rec, img, raw, want, want_img, what):
    assert np.array_equal(rec[:, :3].view(np.uint32), np.ascontiguousarray(raw, np.float32)[:, :3].view(np.uint32)), (what, "xyz")
    got = rec[:, 3].view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (what, "labels", len(bad), bad[:8], got[bad[:8]], np.asarray(want)[bad[:8]])
    if img is not None:
        assert np.array_equal(img, want_img), (what, "label image")


@pytest.mark.gpu
def test_hip_equals_restatement_on_seeded_cases(gpu_ctx):
    import lisreg
    for which in ("16x128", "32x1024"):
        c = seeded(which)
        u = Uploaded(c["raw"], c["pix"], c["mask"], c["lg"])
        for k, kset in enumerate(SETS + (TIED_SET,)):
            for nv in (0, 1):
                want, want_img, _ = seeded_want(which, kset, nv)
                fmt = lisreg.FMT_DEVICE if (k + nv) % 2 else lisreg.FMT_DEVICE_XYZI            # both input formats
                rec, img = _run(gpu_ctx, u, c["P"], KR.Knn(*kset, nv), fmt=fmt, image=bool(nv))
                _check(rec, img, c["raw"], want, want_img, (which, kset, nv))


@pytest.mark.gpu
def test_hip_equals_literal_form_on_planted_cases(gpu_ctx):
    import lisreg
    for name, s, K, want in planted_cases():
        raw, pix, mask, lg, P = s
        lit, want_img, _ = KR.knn_literal(*s, K)
        assert lit.tolist() == want, name
        u = Uploaded(raw, pix, mask, lg)
        for fmt in (lisreg.FMT_DEVICE_XYZI, lisreg.FMT_DEVICE):
            rec, img = _run(gpu_ctx, u, P, K, fmt=fmt)
            _check(rec, img, raw, np.asarray(want, np.uint32), want_img, (name, fmt))


@pytest.mark.gpu
def test_hip_row_stride_on_a_64x2048_image(gpu_ctx):
    """a 64 x 600 sweep in a 64 x 2048 image: rows 2048 pixels apart, most pixels empty"""
    from lisreg import replay
    sw = next(iter(replay.synthetic_raw_drive(1, 64, 600)))[0]
    raw = np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32)
    assert len(raw) > 0.9 * 64 * 600
    P = R.Params(64, 2048, 3.0, -25.0, MEANS, STDS, 20)
    ref = R.project_parallel(raw, P)
    lg, _ = R.stand_in_logits(ref["tensor"], P, 7400)
    plain, _ = R.label_parallel(ref["pixel_index"], ref["invalid_mask"], lg, P)
    u = Uploaded(raw, ref["pixel_index"], ref["invalid_mask"], lg)
    for kset in (SETS[0], SETS[2]):
        K = KR.Knn(*kset, 0)
        want, want_img, _ = KR.knn_parallel(raw, ref["pixel_index"], ref["invalid_mask"], lg, P, K)
        assert (want != plain).sum() > 0
        rec, img = _run(gpu_ctx, u, P, K)
        _check(rec, img, raw, want, want_img, ("64x2048", kset))


@pytest.mark.gpu
def test_hip_batch_of_eight_equals_single_calls(gpu_ctx):
    import lisreg
    ctx = gpu_ctx
    c = seeded("32x1024")
    P = c["P"]
    hw = P.img_h * P.img_w
    other = seeded("16x128")["raw"]
    raws = [c["raw"], np.zeros((0, 4), np.float32), other, c["raw"][:257], c["raw"][:256], other[:1], c["raw"][::3], other[:1000]]
    assert len(raws) == 8 and len({len(r) for r in raws}) == 8
    us, refs = [], []
    for s, r in enumerate(raws):
        ref = R.project_parallel(r, P)
        lg, _ = R.stand_in_logits(ref["tensor"], P, 7500 + s)
        us.append(Uploaded(r, ref["pixel_index"], ref["invalid_mask"], lg))
        refs.append((ref, lg))
    for rep, kset in enumerate((SETS[0], TIED_SET)):
        K = KR.Knn(*kset, rep)
        outs = [lisreg.DeviceArray(np.full((max(u.n, 1), 4), -7.5, np.float32)) for u in us]
        imgs = [lisreg.DeviceArray(np.full(hw, 0xEE, np.uint8)) for _ in us]
        ctx.rangenet_label_knn_batch_device([u.din.ptr for u in us], [u.n for u in us], [u.pix.ptr for u in us], [u.mask.ptr for u in us],
                                            [u.lg.ptr for u in us], _cparams(P), _cknn(K), [o.ptr for o in outs], [i.ptr for i in imgs] if rep else None)
        for s, u in enumerate(us):
            rec, img = _run(ctx, u, P, K)
            a = lisreg.device_to_host(outs[s].ptr, (max(u.n, 1), 4), np.float32)[: u.n]
            assert np.array_equal(a.view(np.uint32), rec.view(np.uint32)), ("batch against single", rep, s)
            want, want_img, _ = KR.knn_parallel(raws[s], refs[s][0]["pixel_index"], refs[s][0]["invalid_mask"], refs[s][1], P, K)
            _check(a, lisreg.device_to_host(imgs[s].ptr, (P.img_h, P.img_w), np.uint8) if rep else None, raws[s], want, want_img, ("batch", rep, s))


@pytest.mark.gpu
def test_hip_knn_between_other_calls_does_not_leak(gpu_ctx):
    """project, kNN label, project, plain label in a row on one context, two different sweeps and two image sizes, then the other way
    round: every result equals its restatement — what the kNN call shares with its neighbours (the sweep table, the label image and the
    range image in the context's scratch) carries nothing over."""
    import lisreg
    ctx = gpu_ctx
    a, b = seeded("32x1024"), seeded("16x128")

    def project(c):
        P = c["P"]
        hw = P.img_h * P.img_w
        din = lisreg.DeviceArray(c["raw"])
        t, m = lisreg.DeviceArray(np.full(5 * hw, -7.5, np.float32)), lisreg.DeviceArray(np.full(hw, 0x5A, np.uint8))
        px = lisreg.DeviceArray(np.full(len(c["raw"]), -99, np.int32))
        nv = ctx.rangenet_project_device(din.ptr, len(c["raw"]), _cparams(P), t.ptr, m.ptr, px.ptr)
        ref = R.project_parallel(c["raw"], P)
        assert nv == ref["n_valid"]
        assert np.array_equal(lisreg.device_to_host(t.ptr, (5, P.img_h, P.img_w), np.float32).view(np.uint32), ref["tensor"].view(np.uint32))
        assert np.array_equal(lisreg.device_to_host(m.ptr, (hw,), np.uint8), c["mask"])
        assert np.array_equal(lisreg.device_to_host(px.ptr, (len(c["raw"]),), np.int32), c["pix"])
        return din, m, px

    def knn(c, io, kset):
        din, m, px = io
        P, K = c["P"], KR.Knn(*kset, 0)
        dlg, out = lisreg.DeviceArray(c["lg"]), lisreg.DeviceArray(np.full((len(c["raw"]), 4), -7.5, np.float32))
        ctx.rangenet_label_knn_device(din.ptr, len(c["raw"]), px.ptr, m.ptr, dlg.ptr, _cparams(P), _cknn(K), out.ptr)       # no image: scratch
        want, _, _ = KR.knn_parallel(*_args(c), K)
        _check(lisreg.device_to_host(out.ptr, (len(c["raw"]), 4), np.float32), None, c["raw"], want, None, ("knn", kset))

    def plain(c, io):
        din, m, px = io
        P = c["P"]
        dlg, out = lisreg.DeviceArray(c["lg"]), lisreg.DeviceArray(np.full((len(c["raw"]), 4), -7.5, np.float32))
        ctx.rangenet_label_device(din.ptr, len(c["raw"]), px.ptr, m.ptr, dlg.ptr, _cparams(P), out.ptr)
        want, _ = R.label_parallel(c["pix"], c["mask"], c["lg"], P)
        _check(lisreg.device_to_host(out.ptr, (len(c["raw"]), 4), np.float32), None, c["raw"], want, None, "plain")
    for first, second in ((a, b), (b, a)):
        knn(first, project(first), SETS[2])
        plain(second, project(second))
        io = project(second)
        knn(second, io, SETS[0])
        plain(second, io)
        knn(second, io, TIED_SET)


import test_caller_stream as TCS  # noqa: E402  (late_case and its module-scoped `env` fixture: the gate of tests/stream_gate.py)

env = TCS.env


@pytest.mark.gpu
def test_hip_on_a_callers_busy_stream(env):
    """the logits arrive late on the caller's stream, as in tests/test_caller_stream.py: the result equals the idle-stream one, and a
    context left on its own stream reads the decoy"""
    e = env
    c = seeded("16x128")
    P, K = c["P"], KR.Knn(*SETS[0], 0)
    n, hw = len(c["raw"]), c["P"].img_h * c["P"].img_w
    din, pix, mask = e.D(c["raw"]), e.D(c["pix"]), e.D(c["mask"])
    decoy = R.stand_in_logits(R.project_parallel(c["raw"], P)["tensor"], P, 7777)[0]

    def make(dst):
        out, img = e.D(np.zeros((n, 4), np.float32)), e.D(np.zeros(hw, np.uint8))
        return (lambda: e.ctx.rangenet_label_knn_device(din.ptr, n, pix.ptr, mask.ptr, dst.ptr, _cparams(P), _cknn(K), out.ptr, img.ptr)), \
               (lambda _: dict(rec=TCS.to_host(out.ptr, (n, 4)), img=TCS.to_host(img.ptr, (P.img_h, P.img_w), np.uint8)))
    o, _ = TCS.late_case(e, "rangenet_label_knn_device", np.asarray(c["lg"]), decoy, make)
    want, want_img, _ = seeded_want("16x128", SETS[0], 0)
    _check(o["rec"], o["img"], c["raw"], want, want_img, "busy stream")


@pytest.mark.gpu
def test_hip_argument_errors(gpu_ctx):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    c = seeded("16x128")
    P = c["P"]
    n = len(c["raw"])
    u = Uploaded(c["raw"], c["pix"], c["mask"], c["lg"])
    out = lisreg.DeviceArray(np.full((n, 4), -7.5, np.float32))
    img = lisreg.DeviceArray(np.full(16 * 128, 0xEE, np.uint8))
    good = lisreg.default_rangenet_knn_params()

    def label(n=n, cloud=u.din.ptr, pix=u.pix.ptr, mask=u.mask.ptr, logits=u.lg.ptr, o=out.ptr, im=None, fmt=lisreg.FMT_DEVICE_XYZI, knn=good,
              params=None):
        cp = _cparams(P) if params is None else params
        return L.lisreg_rangenet_label_knn(ctx._h, C.c_void_p(cloud), n, fmt, C.c_void_p(pix), C.c_void_p(mask), C.c_void_p(logits), C.byref(cp),
                                           C.byref(knn) if knn is not None else None, C.c_void_p(o), C.c_void_p(im))
    assert label(n=-1) == lisreg.ERR_ARG and label(cloud=None) == lisreg.ERR_ARG and label(pix=None) == lisreg.ERR_ARG
    assert label(mask=None) == lisreg.ERR_ARG and label(logits=None) == lisreg.ERR_ARG and label(o=None) == lisreg.ERR_ARG
    assert label(knn=None) == lisreg.ERR_ARG and label(fmt=lisreg.FMT_XYZI) == lisreg.ERR_ARG
    for bad in (dict(search=4), dict(search=2), dict(search=0), dict(search=9), dict(search=3, knn=10), dict(search=5, knn=17), dict(search=7, knn=17),
                dict(knn=0), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(no_vote_label=20),
                dict(no_vote_label=-1)):
        q = lisreg.default_rangenet_knn_params()
        for k, v in bad.items():
            setattr(q, k, v)
        assert label(knn=q) == lisreg.ERR_ARG, bad
    one_class = _cparams(P)
    one_class.n_classes = 1
    assert label(params=one_class) == lisreg.ERR_ARG
    # overlapping buffers: the records on an input, the image on the mask, the image on the records
    assert label(o=u.din.ptr) == lisreg.ERR_ARG and label(o=u.lg.ptr) == lisreg.ERR_ARG and label(im=u.mask.ptr) == lisreg.ERR_ARG
    assert label(im=out.ptr + 16) == lisreg.ERR_ARG
    # a refused call writes nothing
    assert (lisreg.device_to_host(out.ptr, (n, 4), np.float32) == -7.5).all() and (lisreg.device_to_host(img.ptr, (16 * 128,), np.uint8) == 0xEE).all()
    with pytest.raises(lisreg.LisregError) as err:
        ctx.rangenet_label_knn_batch_device([u.din.ptr] * 257, [1] * 257, [u.pix.ptr] * 257, [u.mask.ptr] * 257, [u.lg.ptr] * 257, _cparams(P), good,
                                            [out.ptr] * 257)
    assert err.value.code == lisreg.ERR_ARG
    with pytest.raises(lisreg.LisregError) as err:                                               # two sweeps writing one output
        ctx.rangenet_label_knn_batch_device([u.din.ptr] * 2, [n] * 2, [u.pix.ptr] * 2, [u.mask.ptr] * 2, [u.lg.ptr] * 2, _cparams(P), good, [out.ptr] * 2)
    assert err.value.code == lisreg.ERR_ARG
    # the context stays usable
    assert label(im=img.ptr) == lisreg.OK and label(fmt=lisreg.FMT_DEVICE, n=0) == lisreg.OK
    want, want_img, _ = seeded_want("16x128", SETS[0], 0)
    _check(lisreg.device_to_host(out.ptr, (n, 4), np.float32), lisreg.device_to_host(img.ptr, (16, 128), np.uint8), c["raw"], want, want_img, "after errors")
