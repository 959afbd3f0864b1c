"""RangeNet++ around the network (lisreg_rangenet_project / lisreg_rangenet_label): range-image projection and point labelling.

The yardstick is tests/rangenet_ref.py, the numpy restatement of NetTensorRT::doProjection, the host halves of NetTensorRT::infer and
RangenetAPI::infer's argmax: its literal form (sort by decreasing range, assign in order; one logit vector per point) and the parallel
form the HIP kernels implement (a per-pixel key minimum; a per-pixel argmax and a gather) must agree bit for bit (CPU tests), and the
library must equal it bit for bit for every input format, in a batch, in two calls in a row, chained between the feature extraction and
lisreg_semantic_split, and through torch tensors (GPU tests).  Every comparison is exact: integers equal, floats bit-equal."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import numpy as np
import pytest

import pretreat_ref as PR
import rangenet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "rangenet", "rangenet_16x128.npz")
MEANS = (12.12, 10.88, 0.23, -1.04, 0.21)           # a model's per-channel statistics look like this (stand-ins, not the reference's)
STDS = (12.32, 11.47, 6.91, 0.86, 0.16)


def small_cases():
    """(raw, Params) of >= 20 seeded sweeps at 64 x 2048, 32 x 1024 and 16 x 128, every one with the injected deciding cases"""
    out, seed = [], 100
    for (h, w, ns, n_az, fov) in ((64, 2048, 64, 150, (3.0, -25.0)), (32, 1024, 32, 110, (10.67, -30.67)), (16, 128, 16, 200, (15.0, -15.0))):
        for k, order in enumerate(("ring", "time", "shuffled", "ring", "time", "shuffled", "ring")):
            seed += 1
            P = R.Params(h, w, fov[0], fov[1], MEANS if k % 2 else (0.0,) * 5, STDS if k % 2 else (1.0,) * 5, 20 if k % 3 else 7)
            raw = PR.make_sweep(seed, ns, order, n_az=n_az)
            out.append((R.inject(raw, seed, P), P))
    return out


def full_size_raw(h, w, frames=1):
    """synthetic_raw_drive with ring and time discarded: (n, 4) float32 x y z intensity"""
    from lisreg import replay
    return [np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32)
            for sw, _ in replay.synthetic_raw_drive(frames, h, w)]


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_literal_form_equals_parallel_form():
    cases = small_cases()
    assert len(cases) >= 20 and {(P.img_h, P.img_w) for _, P in cases} == {(64, 2048), (32, 1024), (16, 128)}
    seen = dict(shared=0, ties=0, origin=0, near_invalid=0, near_valid=0, above=0, below=0, seam=0, nonfinite=0, nan_row=0)
    for k, (raw, P) in enumerate(cases):
        a, b = R.project_literal(raw, P), R.project_parallel(raw, P)
        assert R.same_projection(a, b) is None, (k, R.same_projection(a, b))
        pp = R.per_point(raw, P)
        fin, pix, rng = pp["finite"], pp["pixel_index"], pp["range"]
        hw = P.img_h * P.img_w
        assert (pix[~fin] == -1).all() and (pix[fin] >= 0).all() and (pix[fin] < hw).all()
        hits = np.bincount(pix[fin], minlength=hw)
        seen["shared"] += int((hits >= 2).sum())
        assert np.array_equal(a["winner"] >= 0, hits > 0)
        # exact range ties inside one pixel: the winner is the tied point of highest index
        idx = np.flatnonzero(fin)
        pairs = (pix[idx].astype(np.uint64) << np.uint64(32)) | rng[idx].view(np.uint32).astype(np.uint64)
        uniq, inv, cnt = np.unique(pairs, return_inverse=True, return_counts=True)
        for u in np.flatnonzero(cnt >= 2):
            members = idx[inv == u]
            p = int(pix[members[0]])
            if rng[members[0]] == rng[a["winner"][p]]:                      # the tie is the pixel's smallest range
                seen["ties"] += 1
                assert a["winner"][p] == members.max()
        # every winner is a point of smallest range of its pixel
        best = np.full(hw, np.inf)
        np.minimum.at(best, pix[idx], rng[idx].astype(np.float64))
        won = a["winner"] >= 0
        assert np.array_equal(rng[a["winner"][won]].astype(np.float64), best[won])
        origin = fin & (raw[:, 0] == 0) & (raw[:, 1] == 0) & (raw[:, 2] == 0)
        seen["origin"] += int(origin.sum())
        seen["nan_row"] += int(np.isnan(pp["row_raw"][origin]).sum())
        assert (pix[origin] // P.img_w == P.img_h - 1).all()                # a NaN proj_y: row H - 1
        wr = np.where(won, rng[np.where(won, a["winner"], 0)], np.float32(9))
        near = won & (wr < 1)
        seen["near_invalid"] += int((near & (a["invalid_mask"] == 1)).sum())
        seen["near_valid"] += int((near & (a["invalid_mask"] == 0) & (np.abs(raw[np.where(won, a["winner"], 0), 3]) >= 1)).sum())
        assert ((a["invalid_mask"] == 1) == (~won | (near & (np.abs(raw[np.where(won, a["winner"], 0), 3]) < 1)))).all()
        assert a["n_valid"] == int((a["invalid_mask"] == 0).sum())
        assert (a["tensor"].reshape(5, hw)[:, a["invalid_mask"] == 1] == 0).all()
        with np.errstate(invalid="ignore"):
            above, below = fin & (pp["row_raw"] < 0), fin & (pp["row_raw"] > P.img_h - 1)
            seam = fin & (raw[:, 0] < 0) & (raw[:, 1] == 0) & (pp["col_raw"] > P.img_w - 1)
        seen["above"] += int(above.sum()); seen["below"] += int(below.sum()); seen["seam"] += int(seam.sum())
        assert (pix[above] // P.img_w == 0).all() and (pix[below] // P.img_w == P.img_h - 1).all() and (pix[seam] % P.img_w == P.img_w - 1).all()
        seen["nonfinite"] += int((~fin).sum())
        # labelling: the two forms on stand-in logits
        lg, planted = R.stand_in_logits(a["tensor"], P, 7000 + k)
        la, _ = R.label_literal(a["pixel_index"], a["invalid_mask"], lg, P)
        lb, img = R.label_parallel(a["pixel_index"], a["invalid_mask"], lg, P)
        assert np.array_equal(la, lb), k
        assert (img.ravel()[a["invalid_mask"] == 1] == 0).all() and (lb[~fin] == 0).all()
        assert len(np.unique(lb)) >= 3
    assert all(v > 0 for v in seen.values()), seen                            # none of the deciding cases is absent


def test_argmax_edge_cases():
    P = R.Params(1, 4, n_classes=5)
    nan = np.nan
    lg = np.array([[-1.0, 0.5, 0.25, 0.0],
                   [-2.0, 2.0, nan, 0.0],
                   [-0.5, 2.0, 0.75, -1.0],
                   [-3.0, 1.0, nan, 0.0],
                   [-0.1, 2.0, 0.5, -2.0]], np.float32).reshape(5, 1, 4)
    pix, mask = np.array([0, 1, 2, 3, -1, 1], np.int32), np.zeros(4, np.uint8)
    want = [0, 4, 2, 3, 0, 4]             # all negative: 0; tied maxima: the last; NaN skipped; zeros tie with prob = 0: the last; no pixel: 0
    for form in (R.label_literal, R.label_parallel):
        assert form(pix, mask, lg, P)[0].tolist() == want, form.__name__
    masked = np.array([0, 1, 0, 0], np.uint8)                                # an invalid pixel: {1, 0, ...} gives 0
    for form in (R.label_literal, R.label_parallel):
        assert form(pix, masked, lg, P)[0].tolist() == [0, 0, 2, 3, 0, 0]
    assert R.label_parallel(pix, masked, lg, P)[1].tolist() == [[0, 0, 2, 3]]


def test_golden_case_reproduces():
    g = np.load(GOLDEN)
    raw = g["raw"]
    assert len(raw) <= 4000 and os.path.getsize(GOLDEN) < 400 * 1024
    P = R.Params(16, 128, float(g["fov"][0]), float(g["fov"][1]), g["means"], g["stds"], int(g["logits"].shape[0]))
    for form in (R.project_literal, R.project_parallel):
        r = form(raw, P)
        assert np.array_equal(r["pixel_index"], g["pixel_index"]) and np.array_equal(r["invalid_mask"], g["invalid_mask"])
        assert np.array_equal(r["tensor"].view(np.uint32), g["tensor"].view(np.uint32)) and r["n_valid"] == int(g["n_valid"][0])
    for form in (R.label_literal, R.label_parallel):
        labels, img = form(g["pixel_index"], g["invalid_mask"], g["logits"], P)
        assert np.array_equal(labels, g["labels"])
        assert img is None or np.array_equal(img, g["label_image"])
    assert (g["pixel_index"] == -1).sum() > 0 and len(np.unique(g["labels"])) >= 5


def _header_struct(name):
    """ctypes mirror of `typedef struct <name> { ... }` as include/lisreg.h declares it (arrays as `float means[5]`)"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "void*": C.c_void_p, "float*": C.c_void_p, "int*": C.c_void_p,
             "unsignedchar*": C.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"((?:unsigned\s+)?\w+\s*\*?)\s*(.*)", decl).groups()
        for n in names.split(","):
            m = re.match(r"(\w+)(?:\[(\d+)\])?$", n.strip())
            ct = types[t.replace(" ", "")]
            fields.append((m.group(1), ct * int(m.group(2)) if m.group(2) else ct))
    return type(name, (C.Structure,), {"_fields_": fields})


def test_abi_declares_rangenet_and_structs_match_header():
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for sym in ("lisreg_default_rangenet_params", "lisreg_rangenet_project", "lisreg_rangenet_project_batch", "lisreg_rangenet_label",
                "lisreg_rangenet_label_batch"):
        assert re.search(r"^\s*int\s+%s\s*\(" % sym, hdr, re.M), sym
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym)
    for mine, name in ((lisreg.RangenetParams, "lisreg_rangenet_params"), (lisreg.RangenetOut, "lisreg_rangenet_out")):
        theirs = _header_struct(name)
        assert C.sizeof(mine) == C.sizeof(theirs), name
        assert [(n, getattr(mine, n).offset) for n, _ in mine._fields_] == [(n, getattr(theirs, n).offset) for n, _ in theirs._fields_], name
    assert C.sizeof(lisreg.RangenetParams) == 72 and C.sizeof(lisreg.RangenetOut) == 32
    p = lisreg.default_rangenet_params()
    assert (p.img_h, p.img_w, p.fov_up, p.fov_down, p.n_classes) == (64, 2048, 3.0, -25.0, 20)
    assert list(p.means) == [0.0] * 5 and list(p.stds) == [1.0] * 5
    L = lisreg.lib()
    assert L.lisreg_default_rangenet_params(None) == lisreg.ERR_ARG
    ro = lisreg.RangenetOut()
    assert L.lisreg_rangenet_project(None, None, 0, 16, lisreg.FMT_DEVICE_XYZI, C.byref(p), C.byref(ro)) == lisreg.ERR_ARG
    assert L.lisreg_rangenet_project_batch(None, 0, None, None, C.byref(p), None) == lisreg.ERR_ARG
    assert L.lisreg_rangenet_label(None, None, 0, lisreg.FMT_DEVICE_XYZI, None, None, None, C.byref(p), None, None) == lisreg.ERR_ARG
    assert L.lisreg_rangenet_label_batch(None, 0, None, None, None, None, None, C.byref(p), None, None) == lisreg.ERR_ARG


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _cparams(P):
    import lisreg
    p = lisreg.default_rangenet_params(P.img_h, P.img_w)
    p.fov_up, p.fov_down, p.n_classes = P.fov_up, P.fov_down, P.n_classes
    for k in range(5):
        p.means[k], p.stds[k] = float(P.means[k]), float(P.stds[k])
    return p


class Buffers:
    """the three output buffers of lisreg_rangenet_project for a sweep of n points, pre-filled with a sentinel"""

    def __init__(self, n, P, fill=-7.5):
        import lisreg
        self.n, self.P, self.hw = n, P, P.img_h * P.img_w
        self.tensor = lisreg.DeviceArray(np.full(5 * self.hw, fill, np.float32))
        self.mask = lisreg.DeviceArray(np.full(self.hw, 0x5A, np.uint8))
        self.pix = lisreg.DeviceArray(np.full(max(n, 1), -99, np.int32))

    def fetch(self, n_valid):
        import lisreg
        return dict(tensor=lisreg.device_to_host(self.tensor.ptr, (5, self.P.img_h, self.P.img_w), np.float32),
                    invalid_mask=lisreg.device_to_host(self.mask.ptr, (self.hw,), np.uint8),
                    pixel_index=lisreg.device_to_host(self.pix.ptr, (max(self.n, 1),), np.int32)[: self.n], n_valid=n_valid)


def _check_projection(got, ref, what):
    assert np.array_equal(got["pixel_index"], ref["pixel_index"]), (what, "pixel_index", int((got["pixel_index"] != ref["pixel_index"]).sum()))
    assert np.array_equal(got["invalid_mask"], ref["invalid_mask"]), (what, "mask", int((got["invalid_mask"] != ref["invalid_mask"]).sum()))
    assert got["n_valid"] == ref["n_valid"], (what, got["n_valid"], ref["n_valid"])
    bad = np.flatnonzero(got["tensor"].view(np.uint32).ravel() != ref["tensor"].view(np.uint32).ravel())
    assert len(bad) == 0, (what, "tensor", len(bad), got["tensor"].ravel()[bad[:5]], ref["tensor"].ravel()[bad[:5]])


def _all_formats(ctx, raw, P, what):
    import lisreg
    from lisreg import synth
    ref = R.project_parallel(raw, P)
    cp = _cparams(P)
    b = Buffers(len(raw), P)
    _check_projection(b.fetch(ctx.rangenet_project(raw, cp, b.tensor.ptr, b.mask.ptr, b.pix.ptr)), ref, (what, "packed"))
    b = Buffers(len(raw), P)
    pcl = synth.to_pcl(raw[:, :3], None, raw[:, 3])                            # PCL PointXYZI: intensity at byte 16
    _check_projection(b.fetch(ctx.rangenet_project(pcl, cp, b.tensor.ptr, b.mask.ptr, b.pix.ptr)), ref, (what, "xyzi"))
    b = Buffers(len(raw), P)
    din = lisreg.DeviceArray(raw if len(raw) else np.zeros((1, 4), np.float32))
    _check_projection(b.fetch(ctx.rangenet_project_device(din.ptr, len(raw), cp, b.tensor.ptr, b.mask.ptr, b.pix.ptr)), ref, (what, "device"))
    return ref, din, b


def _label_and_check(ctx, raw, din, b, ref, P, seed, what):
    """stand-in logits of the restatement's tensor, uploaded; lisreg_rangenet_label against the restatement"""
    import lisreg
    lg, planted = R.stand_in_logits(ref["tensor"], P, seed)
    want, want_img = R.label_parallel(ref["pixel_index"], ref["invalid_mask"], lg, P)
    dlg = lisreg.DeviceArray(lg)
    out = lisreg.DeviceArray(np.full((max(len(raw), 1), 4), -7.5, np.float32))
    img = lisreg.DeviceArray(np.full(P.img_h * P.img_w, 0xEE, np.uint8))
    ctx.rangenet_label_device(din.ptr, len(raw), b.pix.ptr, b.mask.ptr, dlg.ptr, _cparams(P), out.ptr, img.ptr)
    rec = lisreg.device_to_host(out.ptr, (max(len(raw), 1), 4), np.float32)[: len(raw)]
    assert np.array_equal(rec[:, :3].view(np.uint32), raw[:, :3].view(np.uint32)), what         # NaN / inf coordinates too
    assert np.array_equal(rec[:, 3].view(np.uint32), want), (what, int((rec[:, 3].view(np.uint32) != want).sum()))
    assert np.array_equal(lisreg.device_to_host(img.ptr, (P.img_h, P.img_w), np.uint8), want_img), what
    out2 = lisreg.DeviceArray(np.full((max(len(raw), 1), 4), -7.5, np.float32))                 # without the label image
    ctx.rangenet_label_device(din.ptr, len(raw), b.pix.ptr, b.mask.ptr, dlg.ptr, _cparams(P), out2.ptr)
    assert np.array_equal(lisreg.device_to_host(out2.ptr, (max(len(raw), 1), 4), np.float32)[: len(raw)].view(np.uint32), rec.view(np.uint32)), what
    hit = ref["invalid_mask"] == 0
    for key in ("negative", "tie", "nan_max", "nan_tie"):
        assert hit[planted[key]].sum() > 0, (what, key)                          # the planted vectors sit on valid pixels too
    return want, lg


def _golden():
    g = np.load(GOLDEN)
    return g, R.Params(16, 128, float(g["fov"][0]), float(g["fov"][1]), g["means"], g["stds"], int(g["logits"].shape[0]))


@pytest.mark.gpu
def test_hip_project_and_label_equal_restatement_on_seeded_and_golden_cases(gpu_ctx):
    for k, (raw, P) in enumerate(small_cases()):
        ref, din, b = _all_formats(gpu_ctx, raw, P, ("seeded", k))
        _label_and_check(gpu_ctx, raw, din, b, ref, P, 7000 + k, ("seeded", k))
    g, P = _golden()
    ref, din, b = _all_formats(gpu_ctx, g["raw"], P, "golden")
    assert np.array_equal(ref["tensor"].view(np.uint32), g["tensor"].view(np.uint32))
    import lisreg
    dlg = lisreg.DeviceArray(g["logits"])
    out = lisreg.DeviceArray(np.zeros((len(g["raw"]), 4), np.float32))
    img = lisreg.DeviceArray(np.zeros(16 * 128, np.uint8))
    gpu_ctx.rangenet_label_device(din.ptr, len(g["raw"]), b.pix.ptr, b.mask.ptr, dlg.ptr, _cparams(P), out.ptr, img.ptr)
    assert np.array_equal(lisreg.device_to_host(out.ptr, (len(g["raw"]), 4), np.float32)[:, 3].view(np.uint32), g["labels"])
    assert np.array_equal(lisreg.device_to_host(img.ptr, (16, 128), np.uint8), g["label_image"])


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,fov", [(64, 1800, (3.0, -25.0)), (128, 2048, (3.0, -25.0))])
def test_hip_equals_restatement_on_full_size_sweeps(gpu_ctx, h, w, fov):
    raws = full_size_raw(h, w, 2)
    assert len(raws[0]) > 0.9 * h * w
    for f, raw in enumerate(raws):
        P = R.Params(h, w, fov[0], fov[1], MEANS if f else (0.0,) * 5, STDS if f else (1.0,) * 5, 20)
        ref, din, b = _all_formats(gpu_ctx, raw, P, ("full", h, w, f))
        assert ref["n_valid"] > 0.5 * h * w
        _label_and_check(gpu_ctx, raw, din, b, ref, P, 7100 + f, ("full", h, w, f))


@pytest.mark.gpu
def test_hip_two_calls_in_a_row_do_not_leak(gpu_ctx):
    """The pixel keys are put back in place by the call itself: a dense sweep, then a sparse one into the same context (and a smaller and
    a larger image after it) — nothing of the earlier call shows in the later one."""
    dense = full_size_raw(64, 1800)[0]
    P = R.Params(64, 1800)
    _all_formats(gpu_ctx, dense, P, "dense")
    sparse = np.ascontiguousarray(dense[::97][:500])
    ref, _, _ = _all_formats(gpu_ctx, sparse, P, "sparse after dense")
    assert ref["n_valid"] <= 500
    ref, _, _ = _all_formats(gpu_ctx, np.zeros((0, 4), np.float32), P, "empty after sparse")
    assert ref["n_valid"] == 0 and (ref["invalid_mask"] == 1).all() and (ref["tensor"] == 0).all()
    _all_formats(gpu_ctx, sparse, R.Params(16, 128), "smaller image")
    _all_formats(gpu_ctx, dense[:3000], R.Params(128, 2048), "larger image")
    _all_formats(gpu_ctx, sparse, P, "sparse again")


@pytest.mark.gpu
def test_hip_batch_of_eight_equals_single_calls(gpu_ctx):
    import lisreg
    ctx = gpu_ctx
    g, _ = _golden()
    P = R.Params(32, 1024, 10.67, -30.67, MEANS, STDS, 20)
    cp = _cparams(P)
    cases = small_cases()
    raws = [cases[7][0], np.zeros((0, 4), np.float32), g["raw"], full_size_raw(16, 450)[0], cases[8][0][:257], cases[9][0][:256], cases[10][0][:1],
            cases[11][0][:3000]]
    assert len(raws) == 8 and len({len(r) for r in raws}) == 8
    hw, S = P.img_h * P.img_w, len(raws)
    dins = [lisreg.DeviceArray(r if len(r) else np.zeros((1, 4), np.float32)) for r in raws]
    single, refs = [], []
    for r, d in zip(raws, dins):
        b = Buffers(len(r), P)
        got = b.fetch(ctx.rangenet_project_device(d.ptr, len(r), cp, b.tensor.ptr, b.mask.ptr, b.pix.ptr))
        refs.append(R.project_parallel(r, P))
        _check_projection(got, refs[-1], ("single", len(r)))
        single.append(got)
    lgs = [R.stand_in_logits(ref["tensor"], P, 7200 + s)[0] for s, ref in enumerate(refs)]
    dlgs = [lisreg.DeviceArray(lg) for lg in lgs]
    for rep in range(2):                                                       # twice: the second batch finds the first one's leftovers
        tensor = lisreg.DeviceArray(np.full((S, 5, P.img_h, P.img_w), float(rep + 2), np.float32))
        bs = [Buffers(len(r), P, fill=float(rep + 2)) for r in raws]
        nv = ctx.rangenet_project_batch_device([d.ptr for d in dins], [len(r) for r in raws], cp, tensor.ptr, [b.mask.ptr for b in bs], [b.pix.ptr for b in bs])
        all_t = lisreg.device_to_host(tensor.ptr, (S, 5, P.img_h, P.img_w), np.float32)
        for s in range(S):
            got = bs[s].fetch(nv[s])
            got["tensor"] = all_t[s]
            _check_projection(got, single[s], ("batch", rep, s))
        outs = [lisreg.DeviceArray(np.full((max(len(r), 1), 4), -7.5, np.float32)) for r in raws]
        imgs = [lisreg.DeviceArray(np.full(hw, 0xEE, np.uint8)) for _ in raws]
        ctx.rangenet_label_batch_device([d.ptr for d in dins], [len(r) for r in raws], [b.pix.ptr for b in bs], [b.mask.ptr for b in bs],
                                        [d.ptr for d in dlgs], cp, [o.ptr for o in outs], [i.ptr for i in imgs] if rep else None)
        for s, r in enumerate(raws):
            one = lisreg.DeviceArray(np.full((max(len(r), 1), 4), -7.5, np.float32))
            ctx.rangenet_label_device(dins[s].ptr, len(r), bs[s].pix.ptr, bs[s].mask.ptr, dlgs[s].ptr, cp, one.ptr)
            a = lisreg.device_to_host(outs[s].ptr, (max(len(r), 1), 4), np.float32)[: len(r)]
            b1 = lisreg.device_to_host(one.ptr, (max(len(r), 1), 4), np.float32)[: len(r)]
            want, want_img = R.label_parallel(refs[s]["pixel_index"], refs[s]["invalid_mask"], lgs[s], P)
            assert np.array_equal(a.view(np.uint32), b1.view(np.uint32)), ("label batch", rep, s)
            assert np.array_equal(a[:, 3].view(np.uint32), want), ("label batch", rep, s)
            if rep:
                assert np.array_equal(lisreg.device_to_host(imgs[s].ptr, (P.img_h, P.img_w), np.uint8), want_img), ("label image", s)


@pytest.mark.gpu
def test_hip_argument_errors(gpu_ctx):
    import lisreg
    ctx, L = gpu_ctx, lisreg.lib()
    raw = small_cases()[14][0]
    P = R.Params(16, 128)
    cp = _cparams(P)
    b = Buffers(len(raw), P)
    din = lisreg.DeviceArray(raw)

    def project(n=len(raw), cloud=din.ptr, tensor=b.tensor.ptr, mask=b.mask.ptr, pix=b.pix.ptr, params=cp, fmt=lisreg.FMT_DEVICE_XYZI):
        ro = lisreg.RangenetOut(C.c_void_p(tensor), C.c_void_p(mask), C.c_void_p(pix), 0)
        return L.lisreg_rangenet_project(ctx._h, C.c_void_p(cloud), n, 16, fmt, C.byref(params) if params is not None else None, C.byref(ro))
    assert project() == lisreg.OK
    before = b.fetch(0)
    assert project(n=-1) == lisreg.ERR_ARG and project(cloud=None) == lisreg.ERR_ARG and project(params=None) == lisreg.ERR_ARG
    assert project(tensor=None) == lisreg.ERR_ARG and project(mask=None) == lisreg.ERR_ARG and project(pix=None) == lisreg.ERR_ARG
    assert project(fmt=lisreg.FMT_DEVICE) == lisreg.ERR_ARG and project(fmt=lisreg.FMT_XYZIL) == lisreg.ERR_ARG
    for bad in (dict(img_h=0), dict(img_w=-3), dict(img_h=4097, img_w=4096), dict(n_classes=0), dict(n_classes=33)):
        q = _cparams(P)
        for k, v in bad.items():
            setattr(q, k, v)
        assert project(params=q) == lisreg.ERR_ARG, bad
    # overlapping buffers: an output on the input, two outputs on each other
    assert project(tensor=din.ptr) == lisreg.ERR_ARG and project(pix=din.ptr + 16) == lisreg.ERR_ARG
    assert project(mask=b.tensor.ptr + 4 * 2048) == lisreg.ERR_ARG and project(pix=b.tensor.ptr + 5 * 4 * 2048 - 4) == lisreg.ERR_ARG
    after = b.fetch(0)
    for key in ("tensor", "invalid_mask", "pixel_index"):
        assert np.array_equal(before[key].view(np.uint8), after[key].view(np.uint8)), key    # a refused call writes nothing
    assert np.array_equal(lisreg.device_to_host(din.ptr, raw.shape, np.float32).view(np.uint32), raw.view(np.uint32))
    dlg = lisreg.DeviceArray(np.zeros((20, 16, 128), np.float32))
    out = lisreg.DeviceArray(np.zeros((len(raw), 4), np.float32))

    def label(n=len(raw), cloud=din.ptr, pix=b.pix.ptr, mask=b.mask.ptr, logits=dlg.ptr, o=out.ptr, img=None, fmt=lisreg.FMT_DEVICE_XYZI):
        return L.lisreg_rangenet_label(ctx._h, C.c_void_p(cloud), n, fmt, C.c_void_p(pix), C.c_void_p(mask), C.c_void_p(logits), C.byref(cp),
                                       C.c_void_p(o), C.c_void_p(img))
    assert label() == lisreg.OK and label(fmt=lisreg.FMT_DEVICE) == lisreg.OK
    assert label(n=-1) == lisreg.ERR_ARG and label(cloud=None) == lisreg.ERR_ARG and label(pix=None) == lisreg.ERR_ARG
    assert label(mask=None) == lisreg.ERR_ARG and label(logits=None) == lisreg.ERR_ARG and label(o=None) == lisreg.ERR_ARG
    assert label(fmt=lisreg.FMT_XYZI) == lisreg.ERR_ARG
    assert label(o=din.ptr) == lisreg.ERR_ARG and label(o=dlg.ptr) == lisreg.ERR_ARG and label(img=b.mask.ptr) == lisreg.ERR_ARG
    many = [din.ptr] * 257
    with pytest.raises(lisreg.LisregError) as e:
        ctx.rangenet_project_batch_device(many, [1] * 257, cp, b.tensor.ptr, [b.mask.ptr] * 257, [b.pix.ptr] * 257)
    assert e.value.code == lisreg.ERR_ARG
    with pytest.raises(lisreg.LisregError) as e:                                                # two sweeps writing one mask
        t2 = lisreg.DeviceArray(np.zeros((2, 5, 16, 128), np.float32))
        p2 = lisreg.DeviceArray(np.zeros(len(raw), np.int32))
        ctx.rangenet_project_batch_device([din.ptr, din.ptr], [len(raw)] * 2, cp, t2.ptr, [b.mask.ptr, b.mask.ptr], [b.pix.ptr, p2.ptr])
    assert e.value.code == lisreg.ERR_ARG


def _imu_tables(seed, t0=100.0, n=70, rate=500.0):
    """integrated IMU rotation like imuDeskewInfo builds it (the construction of tests/test_pretreat.py)"""
    rng = np.random.default_rng(seed)
    t = t0 - 0.01 + np.arange(n) / rate
    w = np.stack([0.05 * np.sin(6 * (t - t0)), 0.03 * np.cos(4 * (t - t0)), 0.6 + 0.2 * np.sin(3 * (t - t0))], 1) + rng.normal(0, 0.01, (n, 3))
    rot = np.zeros((n, 3))
    rot[1:] = np.cumsum(w[1:] * np.diff(t)[:, None], 0)
    return t, rot


@pytest.mark.gpu
def test_chain_pretreat_features_project_label_split(gpu_ctx):
    """raw sweep -> pretreat_device -> extract_features_device (de-skewed cloud) -> rangenet_project_device -> stand-in logits ->
    rangenet_label_device -> semantic_split_device, nothing but the stand-in logits crossing the link, against the host path: the same
    de-skewed records through the restatement and Context.semantic_split.  The de-skewed records carry the ring in their payload; the
    projection reads those 32 bits as the intensity channel on both paths."""
    import lisreg
    from lisreg import synth
    ctx = gpu_ctx
    h, w = 64, 1800
    raw = full_size_raw(h, w)[0]
    n = len(raw)
    din = lisreg.DeviceArray(raw)
    pre, tm = lisreg.DeviceArray(np.zeros((n, 4), np.float32)), lisreg.DeviceArray(np.zeros(n, np.float32))
    info = ctx.pretreat_device(din.ptr, n, lisreg.default_pretreat_params(64), pre.ptr, tm.ptr, n)
    names = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
    cap = h * w
    outs = {k: lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for k in names}
    t, rot = _imu_tables(95)
    dk = lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0, time_device_ptr=tm.ptr)
    nd = ctx.extract_features_device(pre.ptr, info["n"], lisreg.FeatureParams(h, w, 2, 0.0, 70.0, 1.0, 0.1), {k: v.ptr for k, v in outs.items()}, cap, dk)
    m = nd["deskewed"]
    assert m > 20000
    P = R.Params(h, w, 3.0, -25.0, MEANS, STDS, 20)
    cp = _cparams(P)
    b = Buffers(m, P)
    n_valid = ctx.rangenet_project_device(outs["deskewed"].ptr, m, cp, b.tensor.ptr, b.mask.ptr, b.pix.ptr)
    # the host path
    cloud = lisreg.device_to_host(outs["deskewed"].ptr, (cap, 4), np.float32)[:m]
    ref = R.project_parallel(cloud, P)
    _check_projection(b.fetch(n_valid), ref, "chain")
    lg, _ = R.stand_in_logits(ref["tensor"], P, 7300)
    labels, _ = R.label_parallel(ref["pixel_index"], ref["invalid_mask"], lg, P)
    using = [(10, 40, 50, 81, 0)[j % 5] for j in range(32)]
    want = ctx.semantic_split(synth.to_pcl(cloud[:, :3], labels.astype(np.uint16)), using)
    # the device path
    dlg = lisreg.DeviceArray(lg)
    lab = lisreg.DeviceArray(np.zeros((m, 4), np.float32))
    ctx.rangenet_label_device(outs["deskewed"].ptr, m, b.pix.ptr, b.mask.ptr, dlg.ptr, cp, lab.ptr)
    five = [lisreg.DeviceArray(np.zeros((m, 4), np.float32)) for _ in range(5)]
    counts = ctx.semantic_split_device(lab.ptr, m, [f.ptr for f in five], m, using)
    assert counts == [len(c) for c in want] and sum(counts) == m and min(counts) > 0, counts
    for k in range(5):
        got = lisreg.device_to_host(five[k].ptr, (m, 4), np.float32)[: counts[k]]
        assert np.array_equal(got[:, :3].view(np.uint32), synth.pcl_xyz(want[k]).view(np.uint32)), k
        assert np.array_equal(got[:, 3].view(np.uint32), want[k]["label"].astype(np.uint32)), k


@pytest.mark.gpu
@pytest.mark.parametrize("device_resident", [False, True])
def test_replayer_with_a_labeller_equals_replayer_fed_with_the_restatements_labels(gpu_ctx, device_resident):
    """replay.Replayer / DeviceReplayer with `labeller`: unlabelled sweeps, labels from project -> labeller -> label on the device, against
    the same replayer fed with clouds labelled through the restatement.  The stand-in network answers every pixel with the one-hot file
    label of the point that won it, so the drive keeps its poles, road and walls and the registrations succeed."""
    import lisreg
    from lisreg import replay
    P = R.Params(32, 1024)
    cp = _cparams(P)
    hw = P.img_h * P.img_w
    frames = [c for c, _ in replay.synthetic_drive(4, 32, 900)]
    raws, logits, labelled = [], [], []
    for cloud in frames:
        raw = np.ascontiguousarray(np.stack([cloud["x"], cloud["y"], cloud["z"], cloud["intensity"]], 1), np.float32)
        ref = R.project_parallel(raw, P)
        won = np.flatnonzero(ref["winner"] >= 0)
        lg = np.zeros((P.n_classes, hw), np.float32)
        lg[cloud["label"][ref["winner"][won]], won] = 1.0
        lab = cloud.copy()
        lab["label"] = R.label_parallel(ref["pixel_index"], ref["invalid_mask"], lg, P)[0]
        raws.append(raw); logits.append(lg); labelled.append(lab)
        assert {1, 9, 13, 18} <= set(np.unique(lab["label"]).tolist())
    dlg = lisreg.DeviceArray(logits[0])
    calls = []

    def labeller(tensor_ptr):
        k = len(calls)
        calls.append(lisreg.device_to_host(tensor_ptr, (5, hw), np.float32))
        dlg.upload(logits[k])
        return dlg.ptr
    cls = replay.DeviceReplayer if device_resident else replay.Replayer
    a = cls(gpu_ctx, labeller=labeller, rangenet_params=cp)
    got = [a.step(raw) for raw in raws]
    b = cls(gpu_ctx)
    want = [b.step(lab) for lab in labelled]
    assert len(calls) == len(frames)
    for k, (x, y) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(x["T"], np.float32).view(np.uint32), np.asarray(y["T"], np.float32).view(np.uint32)), (k, x["T"], y["T"])
        assert (x["n_map"], x["feature_point_num"]) == (y["n_map"], y["feature_point_num"]), k
        if k > 0:
            assert x["stats"]["status"] == 0 and x["stats"]["iters"] == y["stats"]["iters"], (k, x["stats"], y["stats"])
            assert (x["n_src_corner"], x["n_src_surf"]) == (y["n_src_corner"], y["n_src_surf"]), k


TORCH_CASE = """
import os, sys
sys.path.insert(0, os.path.join({root!r}, "lis-slam_amd")); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import torch
if not torch.cuda.is_available():
    print("NO_TORCH_DEVICE"); sys.exit(0)
import lisreg
import rangenet_ref as R
from lisreg import replay
H, W, C_ = 64, 1800, 20
sw = next(iter(replay.synthetic_raw_drive(1, H, W)))[0]
raw = np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32)
P = R.Params(H, W, 3.0, -25.0, {means!r}, {stds!r}, C_)
cp = lisreg.default_rangenet_params(H, W)
for k in range(5):
    cp.means[k], cp.stds[k] = float(P.means[k]), float(P.stds[k])
ctx = lisreg.Context(0)
dev = torch.device("cuda:0")
cloud = torch.from_numpy(raw).to(dev)
tensor = torch.empty((5, H, W), device=dev, dtype=torch.float32)
mask = torch.empty((H * W,), device=dev, dtype=torch.uint8)
pix = torch.empty((len(raw),), device=dev, dtype=torch.int32)
torch.cuda.synchronize()
n_valid = ctx.rangenet_project_device(cloud.data_ptr(), len(raw), cp, tensor.data_ptr(), mask.data_ptr(), pix.data_ptr())
ref = R.project_parallel(raw, P)
assert n_valid == ref["n_valid"]
assert np.array_equal(tensor.cpu().numpy().view(np.uint32), ref["tensor"].view(np.uint32))
assert np.array_equal(mask.cpu().numpy(), ref["invalid_mask"]) and np.array_equal(pix.cpu().numpy(), ref["pixel_index"])
g = torch.Generator().manual_seed(5)
conv = torch.nn.Conv2d(5, C_, 1, bias=True)
with torch.no_grad():
    conv.weight.copy_(torch.randn((C_, 5, 1, 1), generator=g)); conv.bias.copy_(0.5 * torch.randn((C_,), generator=g))
    logits = conv.to(dev)(tensor[None])[0].contiguous()
torch.cuda.synchronize()
out = torch.empty((len(raw), 4), device=dev, dtype=torch.float32)
img = torch.empty((H, W), device=dev, dtype=torch.uint8)
ctx.rangenet_label_device(cloud.data_ptr(), len(raw), pix.data_ptr(), mask.data_ptr(), logits.data_ptr(), cp, out.data_ptr(), img.data_ptr())
want, want_img = R.label_parallel(ref["pixel_index"], ref["invalid_mask"], logits.cpu().numpy(), P)
rec = out.cpu().numpy()
assert np.array_equal(rec[:, :3].view(np.uint32), raw[:, :3].view(np.uint32))
assert np.array_equal(rec[:, 3].view(np.uint32), want) and np.array_equal(img.cpu().numpy(), want_img)
assert len(np.unique(want)) >= 5
ctx.close()
print("CASE_DONE")
"""


def _have_torch():
    try:
        import importlib.util
        return importlib.util.find_spec("torch") is not None
    except Exception:
        return False


@pytest.mark.gpu
@pytest.mark.skipif(not _have_torch(), reason="torch not installed")
def test_torch_tensors_in_and_out_through_data_ptr():
    """The input tensor written into a torch.empty((5, H, W)) through data_ptr(), logits from a torch 1 x 1 convolution with fixed
    weights handed back by data_ptr() after torch.cuda.synchronize(); the labels equal the restatement's argmax over THOSE logits (copied
    to the host), so the convolution's own rounding does not matter.  A fresh interpreter with torch imported first, as bench.py does
    (tests/test_teardown.py: the suite's own process does not import torch)."""
    code = textwrap.dedent(TORCH_CASE.format(root=ROOT, means=MEANS, stds=STDS))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    if "NO_TORCH_DEVICE" in r.stdout:
        pytest.skip("torch sees no device")
    assert "CASE_DONE" in r.stdout and r.returncode == 0, f"exit status {r.returncode}\n{r.stdout}\n{r.stderr[-3000:]}"
