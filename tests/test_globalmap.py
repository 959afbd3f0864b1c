"""The global map assembled on the GPU from the resident submaps (lisreg_submap_gather): chosen classes of a list of submaps, each under
its own pose, as one cloud in one launch.

The yardstick is tests/globalmap_ref.py, the numpy restatement of publishGlobalMap (src/node/subMapOptmizationNode.cpp:3553-3574).  On the
CPU it is checked against the C oracle's transformPointCloud and against a golden file; on the GPU the library must equal it — and the
per-class localmap_get + lisreg_transform_cloud path it replaces — bit for bit: coordinates compared as uint32, NaN where the restatement
has NaN, the payload word as bits.  Poses come from globalmap_ref.agreed_poses (its module docstring says why)."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import globalmap_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "globalmap", "globalmap_small.npz")
HOST = os.path.join(ROOT, "lis-slam_amd", "host")
if GOLDEN_DIR not in sys.path:
    sys.path.insert(0, GOLDEN_DIR)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    """ctypes mirror of `typedef struct <name> { ... }` as include/lisreg.h declares it"""
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    types = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "void*": C.c_void_p}
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        t, names = re.match(r"(\w+\s*\*?)\s+(.*)", decl).groups()
        for n in names.split(","):
            fields.append((n.strip(), types[t.replace(" ", "")]))
    return type(name, (C.Structure,), {"_fields_": fields})


def test_abi_declares_gather_and_struct_matches_header():
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for sym in ("lisreg_default_gather_params", "lisreg_submap_gather_count", "lisreg_submap_gather"):
        assert re.search(r"^\s*int\s+%s\s*\(" % sym, hdr, re.M), sym
        assert sym in lisreg.ABI_SYMBOLS and hasattr(lisreg.lib(), sym)
    for k, name in enumerate(("DYNAMIC", "POLE", "GROUND", "BUILDING", "OUTLIER")):
        assert re.search(r"#define\s+LISREG_CLS_%s\s+%du\b" % (name, 1 << k), hdr) and getattr(lisreg, "CLS_" + name) == 1 << k
    assert re.search(r"#define\s+LISREG_CLS_ALL\s+31u\b", hdr) and lisreg.CLS_ALL == 31
    theirs = _header_struct("lisreg_gather_params")
    mine = lisreg.GatherParams
    assert C.sizeof(mine) == C.sizeof(theirs) == 12
    assert [(n, getattr(mine, n).offset) for n, _ in mine._fields_] == [(n, getattr(theirs, n).offset) for n, _ in theirs._fields_]
    assert [n for n, _ in mine._fields_] == ["class_mask", "out_fmt", "chunk_points"]
    p = lisreg.GatherParams(7, 7, 7)
    assert lisreg.lib().lisreg_default_gather_params(C.byref(p)) == lisreg.OK
    assert (p.class_mask, p.out_fmt, p.chunk_points) == (31, lisreg.FMT_DEVICE, 0)
    assert lisreg.lib().lisreg_default_gather_params(None) == lisreg.ERR_ARG


def test_binding_has_the_gather_methods():
    import lisreg
    for name in ("submap_gather_count", "submap_gather", "submap_gather_device"):
        assert callable(getattr(lisreg.Context, name, None)), name


def _golden():
    import make_golden_globalmap as G
    g = np.load(GOLDEN)
    return G, g, G.store_of(g)


def test_restatement_equals_oracle_transform_per_class(oracle):
    _, g, store = _golden()
    ids, poses = g["ids"], g["poses"]
    for mask in (31, 21):
        cloud, off = R.global_map(store, ids, poses, mask)
        assert len(off) == len(ids) * 5 + 1 and off[-1] == len(cloud)
        moved = 0
        for i, mid in enumerate(ids):
            for k in range(5):
                seg = cloud[off[5 * i + k]:off[5 * i + k + 1]]
                if not (mask >> k) & 1:
                    assert len(seg) == 0
                    continue
                want = R.oracle_transform(store[int(mid)][k], poses[i])
                assert np.array_equal(seg.view(np.uint32), want.view(np.uint32)), (mask, i, k)
                moved += len(seg)
        assert moved == len(cloud) > 1000
    # no poses: the records themselves, end to end
    cloud, off = R.global_map(store, ids, None, 31)
    assert np.array_equal(cloud.view(np.uint32), np.concatenate([store[int(m)][k] for m in ids for k in range(5)]).view(np.uint32))


def test_golden_globalmap_reproduces(oracle):
    G, g, store = _golden()
    assert os.path.getsize(GOLDEN) <= 100 * 1024
    again = G.make()
    assert sorted(again) == sorted(g.files)
    for name in g.files:
        a, b = np.ascontiguousarray(again[name]), np.ascontiguousarray(g[name])
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
    for mask in (31, 21):
        cloud, off = R.global_map(store, g["ids"], g["poses"], mask)
        assert R.same_bits(cloud, g["cloud%d" % mask]) is None and np.array_equal(off, g["off%d" % mask])
    assert np.abs(g["poses"][:, :3]).max() > 2.0 and np.abs(g["poses"][:, 3:]).max() > 250.0


# ---- GPU -------------------------------------------------------------------------------------------------------------------
BOUNDARY_COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099)
ZERO_POSE = np.zeros(6, np.float32)


def _install(ctx, store):
    """the store's class arrays as resident submaps (fisrt_submap: appended as they are); returns what localmap_get reads back"""
    import lisreg
    prm = lisreg.localmap_default_params()
    back = {}
    for mid, cls in store.items():
        ctx.localmap_reset(mid)
        counts = [len(c) for c in cls]
        if sum(counts):
            dev = [lisreg.DeviceArray(c) if len(c) else None for c in cls]
            info = ctx.submap_insert_device(mid, [d.ptr if d else 0 for d in dev], counts, None, ZERO_POSE, prm)
            assert info["n"] == counts
            for d in dev:
                if d:
                    d.free()
        back[mid] = [ctx.localmap_get(mid, k).copy() for k in range(5)]
        for k in range(5):
            assert np.array_equal(back[mid][k].view(np.uint32), np.ascontiguousarray(cls[k], np.float32).reshape(-1, 4).view(np.uint32))
    return back


def _gather_dev(ctx, ids, poses, mask=31, fmt=None, extra=0):
    """a device-destination gather read back: ((N, 4) float32 records or (N, 8) uint32 struct words, offsets)"""
    import lisreg
    fmt = lisreg.FMT_DEVICE if fmt is None else fmt
    need, off0 = ctx.submap_gather_count(ids, mask)
    words = 8 if fmt == lisreg.FMT_XYZIL else 4
    buf = lisreg.DeviceArray(np.zeros((need + extra + 1, words), np.float32))
    n, off = ctx.submap_gather_device(ids, poses, buf.ptr, need + extra, mask, fmt)
    assert n == need and np.array_equal(off, off0)
    out = lisreg.device_to_host(buf.ptr, (max(n, 1), words), np.float32 if words == 4 else np.uint32)[:n]
    buf.free()
    return out, off


def _per_class_path(ctx, store, ids, poses, mask):
    """what the gather replaces: per class, localmap_get + lisreg_transform_cloud on device records, concatenated on the host"""
    import lisreg
    parts = []
    for i, mid in enumerate(ids):
        for k in range(5):
            rec = ctx.localmap_get(int(mid), k)
            if not (mask >> k) & 1 or len(rec) == 0:
                continue
            a, b = lisreg.DeviceArray(rec), lisreg.DeviceArray(np.zeros_like(rec))
            ctx.transform_cloud_device(a.ptr, len(rec), poses[i], b.ptr)
            parts.append(b.download(len(rec)))
            a.free(); b.free()
    return np.concatenate(parts) if parts else np.zeros((0, 4), np.float32)


@pytest.fixture(scope="module")
def boundary_maps(gpu_ctx, oracle):
    rng = np.random.default_rng(7101)
    draw = np.concatenate([rng.permutation(BOUNDARY_COUNTS) for _ in range(4)])[:35]          # every count at least three times
    assert set(draw.tolist()) == set(BOUNDARY_COUNTS)
    store = R.make_store(rng, {110 + m: draw[5 * m:5 * m + 5] for m in range(7)})
    back = _install(gpu_ctx, store)
    ids = np.arange(110, 117)
    poses = R.agreed_poses(rng, 7)
    assert np.abs(poses[:, :3]).max() > 2.5 and np.abs(poses[:, 3:]).max() > 400.0
    return back, ids, poses


@pytest.mark.gpu
@pytest.mark.parametrize("mask", [31, 15, 2, 21, 0])
def test_boundaries(gpu_ctx, boundary_maps, mask):
    import lisreg
    store, ids, poses = boundary_maps
    want, woff = R.global_map(store, ids, poses, mask)
    n, off = gpu_ctx.submap_gather_count(ids, mask)
    assert n == len(want) and np.array_equal(off, woff)
    got, goff = _gather_dev(gpu_ctx, ids, poses, mask)
    assert np.array_equal(goff, woff)
    assert R.same_bits(got, want) is None, R.same_bits(got, want)
    old = _per_class_path(gpu_ctx, store, ids, poses, mask)
    assert np.array_equal(got.view(np.uint32), old.view(np.uint32))
    got32, goff = _gather_dev(gpu_ctx, ids, poses, mask, lisreg.FMT_XYZIL)
    assert np.array_equal(goff, woff) and np.array_equal(got32, R.to_xyzil(want))
    if mask == 0:
        assert n == 0 and not off.any()


@pytest.mark.gpu
def test_many_segments(gpu_ctx, oracle):
    rng = np.random.default_rng(7102)
    counts = {}
    for m in range(60):
        c = rng.integers(1, 300, 5)
        c[rng.random(5) < 0.12] = 0
        counts[200 + m] = c if m % 10 else np.zeros(5, np.int64)          # six submaps are empty altogether
    store = _install(gpu_ctx, R.make_store(rng, counts))
    ids = rng.integers(200, 260, 300)
    ids[:60] = rng.permutation(np.arange(200, 260))                       # every submap is named, most of them several times
    rng.shuffle(ids)
    poses = R.agreed_poses(rng, 300)
    want, woff = R.global_map(store, ids, poses, 31)
    assert len(woff) == 1501 and int((np.diff(woff) > 0).sum()) > 1024 and int((np.diff(woff) == 0).sum()) > 100
    got, goff = _gather_dev(gpu_ctx, ids, poses, 31)
    assert np.array_equal(goff, woff)
    assert R.same_bits(got, want) is None, R.same_bits(got, want)


SPECIAL_PAYLOADS = (0x00000012, 0x7FC00001, 0xFFFFFFFF)


def _special_store(rng):
    n = 700
    rec = np.zeros((n, 4), np.float32)
    rec[:, :3] = rng.uniform(-50, 50, (n, 3)).astype(np.float32)
    u = rec.view(np.uint32)
    u[:, 3] = np.asarray(SPECIAL_PAYLOADS, np.uint32)[np.arange(n) % 3]
    specials = np.array([0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC01234, 0x7F800001], np.uint32)     # -0.0, +-inf, NaNs
    for j in range(60):
        u[5 + 7 * j, j % 3] = specials[j % len(specials)]
    u[3, :3] = 0x80000000                                                  # a whole point of -0.0
    return {300: [rec[:100], rec[100:165], rec[165:421], rec[421:422], rec[422:]]}


@pytest.mark.gpu
def test_special_values_and_payload_bits(gpu_ctx, oracle):
    import lisreg
    rng = np.random.default_rng(7103)
    store = _install(gpu_ctx, _special_store(rng))
    ids = [300, 300]
    every = np.concatenate([store[300][k] for k in range(5)] * 2)
    # no poses: every word comes out as it went in, NaN bit patterns and -0.0 included
    got, _ = _gather_dev(gpu_ctx, ids, None, 31)
    assert np.array_equal(got.view(np.uint32), every.view(np.uint32))
    host, _ = gpu_ctx.submap_gather(ids, None, 31)
    assert np.array_equal(host.view(np.uint32), every.view(np.uint32))
    assert (got.view(np.uint32)[:, :3] == 0x80000000).any() and np.isnan(got[:, :3]).any() and np.isinf(got[:, :3]).any()
    # with poses: the restatement's bits, NaN where it has NaN, and the same payload words untouched
    poses = R.agreed_poses(rng, 2)
    want, _ = R.global_map(store, ids, poses, 31)
    got, _ = _gather_dev(gpu_ctx, ids, poses, 31)
    assert R.same_bits(got, want) is None, R.same_bits(got, want)
    assert np.array_equal(got.view(np.uint32)[:, 3], every.view(np.uint32)[:, 3])
    assert set(np.unique(got.view(np.uint32)[:, 3]).tolist()) == set(SPECIAL_PAYLOADS)
    assert np.isnan(want[:, :3]).any()
    got32, _ = _gather_dev(gpu_ctx, ids, None, 31, lisreg.FMT_XYZIL)
    assert np.array_equal(got32, R.to_xyzil(every))


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [7000, 1000, 0])
def test_host_destination(gpu_ctx, oracle, chunk):
    import lisreg
    rng = np.random.default_rng(7104)
    counts = {400 + m: rng.integers(400, 1700, 5) for m in range(5)}
    store = _install(gpu_ctx, R.make_store(rng, counts))
    ids = [402, 400, 404, 401, 403]
    poses = R.agreed_poses(rng, 5)
    want, woff = R.global_map(store, ids, poses, 31)
    assert 20000 < len(want) < 30000
    dev, _ = _gather_dev(gpu_ctx, ids, poses, 31)
    assert R.same_bits(dev, want) is None
    host, off = gpu_ctx.submap_gather(ids, poses, 31, lisreg.FMT_DEVICE, chunk)
    assert np.array_equal(off, woff) and np.array_equal(host.view(np.uint32), dev.view(np.uint32))
    pinned = lisreg.PinnedArray(np.zeros((len(want), 4), np.float32))          # a registered host destination is a host destination
    n, _ = gpu_ctx.submap_gather_device(ids, poses, pinned.ptr, len(want), 31, lisreg.FMT_DEVICE, chunk)
    assert n == len(want) and np.array_equal(pinned.array.view(np.uint32).reshape(-1, 4), dev.view(np.uint32))
    pinned.free()
    dev32, _ = _gather_dev(gpu_ctx, ids, poses, 31, lisreg.FMT_XYZIL)
    host32, _ = gpu_ctx.submap_gather(ids, poses, 31, lisreg.FMT_XYZIL, chunk)
    assert host32.dtype.itemsize == 32 and np.array_equal(host32.view(np.uint32).reshape(-1, 8), dev32)
    assert np.array_equal(host32["x"].view(np.uint32), dev.view(np.uint32)[:, 0]) and not host32["intensity"].any()
    assert np.array_equal(host32["label"], (dev.view(np.uint32)[:, 3] & 0xFFFF).astype(np.uint16))


@pytest.mark.gpu
def test_past_four_gigabytes(gpu_ctx, oracle):
    import lisreg
    hip = lisreg.hip_runtime()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    if free.value < 8 << 30:
        pytest.skip("less than 8 GB of device memory free")
    rng = np.random.default_rng(7105)
    per, reps = 250000, 1100
    store = _install(gpu_ctx, R.make_store(rng, {500: (50000,) * 5}))
    ids = np.full(reps, 500, np.int32)
    pool = R.agreed_poses(rng, 37)
    poses = np.stack([np.concatenate([pool[i % 37, :3], [0.4 * i - 200.0, 300.0 - 0.5 * i, 0.01 * i]]) for i in range(reps)]).astype(np.float32)
    n_total = per * reps
    assert n_total * 16 > 2 ** 32
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(n_total * 16)) == 0
    try:
        n, off = gpu_ctx.submap_gather_device(ids, poses, ptr.value, n_total)
        assert n == n_total and off[-1] == n_total
        assert np.array_equal(off, np.arange(reps * 5 + 1, dtype=np.int64) * 50000)
        for start in (0, 2 ** 28 - 2048, n_total - 4096):
            i0, i1 = start // per, (start + 4095) // per
            want, _ = R.global_map(store, ids[i0:i1 + 1], poses[i0:i1 + 1], 31)
            want = want[start - i0 * per:start - i0 * per + 4096]
            got = lisreg.device_to_host(ptr.value + start * 16, (4096, 4))
            assert R.same_bits(got, want) is None, (start, R.same_bits(got, want))
    finally:
        hip.hipDeviceSynchronize()
        hip.hipFree(ptr)


@pytest.mark.gpu
def test_back_to_back(gpu_ctx, boundary_maps, oracle):
    import lisreg
    store, ids, poses = boundary_maps
    rng = np.random.default_rng(7106)
    jobs = []
    for j in range(3):                                                      # the third reuses the first one's staging slot
        pick = rng.permutation(7)[:4 + j]
        jobs.append((ids[pick], R.agreed_poses(rng, len(pick)), (31, 15, 21)[j]))
    bufs = []
    for jid, jposes, mask in jobs:                                          # issued back to back: nothing is read or waited for in between
        need, _ = gpu_ctx.submap_gather_count(jid, mask)
        buf = lisreg.DeviceArray(np.zeros((need + 1, 4), np.float32))
        n, _ = gpu_ctx.submap_gather_device(jid, jposes, buf.ptr, need, mask)
        bufs.append((buf, n))
    for (jid, jposes, mask), (buf, n) in zip(jobs, bufs):
        want, _ = R.global_map(store, jid, jposes, mask)
        got = lisreg.device_to_host(buf.ptr, (max(n, 1), 4))[:n]           # synchronises the device first
        assert R.same_bits(got, want) is None, (mask, R.same_bits(got, want))
        buf.free()


@pytest.mark.gpu
def test_errors_leave_out_untouched(gpu_ctx, boundary_maps):
    import lisreg
    L = lisreg.lib()
    store, ids, poses = boundary_maps
    h = gpu_ctx._h
    ip, fp, llp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_longlong)
    need, _ = gpu_ctx.submap_gather_count(ids, 31)
    sentinel = np.full((need + 8, 4), 0x5A5A5A5A, np.uint32).view(np.float32)
    dev = lisreg.DeviceArray(sentinel)
    host = sentinel.copy()
    prm = lisreg.GatherParams(31, lisreg.FMT_DEVICE, 0)
    T = np.ascontiguousarray(poses, np.float32)

    def call(id_list, n_maps=None, params=prm, out=None, cap=need + 8, with_poses=True):
        a = np.ascontiguousarray(id_list, np.int32)
        n = C.c_longlong(-7)
        rc = L.lisreg_submap_gather(h, len(a) if n_maps is None else n_maps, a.ctypes.data_as(ip), T.ctypes.data_as(fp) if with_poses else None,
                                    C.byref(params) if params is not None else None, out, cap, C.byref(n), None)
        return rc, n.value

    def untouched():
        return (np.array_equal(lisreg.device_to_host(dev.ptr, sentinel.shape).view(np.uint32), sentinel.view(np.uint32)) and
                np.array_equal(host.view(np.uint32), sentinel.view(np.uint32)))

    for out in (C.c_void_p(dev.ptr), host.ctypes.data_as(C.c_void_p)):
        for bad_ids in ([110, 999, 111], [110, 5000], [-1], [1023]):        # never created / out of range
            assert call(bad_ids, out=out)[0] == lisreg.ERR_NO_TARGET and untouched()
        rc, n = call(ids, out=out, cap=need - 1)                            # too small: the need comes back
        assert rc == lisreg.ERR_ARG and n == need and untouched()
        rc, n = call(ids, out=out, cap=0)
        assert rc == lisreg.ERR_ARG and n == need and untouched()
        assert call(ids, n_maps=0, out=out) == (lisreg.OK, 0) and untouched()
        assert call(ids, params=lisreg.GatherParams(0, lisreg.FMT_DEVICE, 0), out=out) == (lisreg.OK, 0) and untouched()
        assert call(ids, n_maps=-1, out=out)[0] == lisreg.ERR_ARG and untouched()
        assert call(ids, params=None, out=out)[0] == lisreg.ERR_ARG and untouched()
        assert call(ids, params=lisreg.GatherParams(32, lisreg.FMT_DEVICE, 0), out=out)[0] == lisreg.ERR_ARG and untouched()
        assert call(ids, params=lisreg.GatherParams(63, lisreg.FMT_DEVICE, 0), out=out)[0] == lisreg.ERR_ARG and untouched()
        assert call(ids, params=lisreg.GatherParams(31, lisreg.FMT_XYZI, 0), out=out)[0] == lisreg.ERR_ARG and untouched()
    n = C.c_longlong(-7)
    a = np.ascontiguousarray([110, 999], np.int32)
    assert L.lisreg_submap_gather_count(h, 2, a.ctypes.data_as(ip), 31, C.byref(n), None) == lisreg.ERR_NO_TARGET
    assert L.lisreg_submap_gather_count(h, 1, a.ctypes.data_as(ip), 64, C.byref(n), None) == lisreg.ERR_ARG
    assert L.lisreg_submap_gather_count(h, -1, a.ctypes.data_as(ip), 31, C.byref(n), None) == lisreg.ERR_ARG
    assert L.lisreg_submap_gather_count(h, 0, None, 31, C.byref(n), None) == lisreg.OK and n.value == 0
    with pytest.raises(lisreg.LisregError) as e:
        gpu_ctx.submap_gather([110, 999])
    assert e.value.code == lisreg.ERR_NO_TARGET
    # and the buffers still work afterwards
    rc, n_ok = call(ids, out=C.c_void_p(dev.ptr))
    assert rc == lisreg.OK and n_ok == need
    want, _ = R.global_map(store, ids, poses, 31)
    assert R.same_bits(lisreg.device_to_host(dev.ptr, (need, 4)), want) is None
    dev.free()


@pytest.mark.gpu
def test_store_unchanged(gpu_ctx, oracle):
    import lisreg
    rng = np.random.default_rng(7108)
    store = _install(gpu_ctx, R.make_store(rng, {600: rng.integers(800, 2500, 5), 601: rng.integers(800, 2500, 5)}, spread=20.0))
    pre_pose = np.array([0.01, -0.02, 0.3, 1.0, -2.0, 0.1], np.float32)
    cur_pose = np.array([-0.02, 0.01, 0.35, 3.0, -1.0, 0.0], np.float32)

    def extract():
        x = gpu_ctx.submap_extract(600, 601, pre_pose, cur_pose, target_slot=-1)
        clouds = [gpu_ctx.localmap_get(600, 5).copy(), gpu_ctx.localmap_get(600, 6).copy(),
                  lisreg.device_to_host(x["src_corner_ptr"], (max(x["n_src_corner"], 1), 4))[:x["n_src_corner"]],
                  lisreg.device_to_host(x["src_surf_ptr"], (max(x["n_src_surf"], 1), 4))[:x["n_src_surf"]]]
        return x, clouds

    xa, ca = extract()
    assert xa["n_target_surf"] > 100 and xa["n_src_surf"] > 10
    before = {m: [gpu_ctx.localmap_get(m, k).copy() for k in range(5)] for m in (600, 601)}
    poses = R.agreed_poses(rng, 3)
    want, _ = R.global_map(store, [601, 600, 601], poses, 31)
    for fmt in (lisreg.FMT_DEVICE, lisreg.FMT_XYZIL):
        _gather_dev(gpu_ctx, [601, 600, 601], poses, 31, fmt)
        gpu_ctx.submap_gather([601, 600, 601], poses, 31, fmt, 3000)
    got, _ = _gather_dev(gpu_ctx, [601, 600, 601], poses, 31)
    assert R.same_bits(got, want) is None
    for m in (600, 601):
        for k in range(5):
            now = gpu_ctx.localmap_get(m, k)
            assert np.array_equal(now.view(np.uint32), before[m][k].view(np.uint32)) and np.array_equal(now.view(np.uint32), store[m][k].view(np.uint32))
    xb, cb = extract()
    for key in ("n_target_corner", "n_target_surf", "n_src_corner", "n_src_surf"):
        assert xa[key] == xb[key], key
    assert np.array_equal(xa["isect"], xb["isect"]) and np.array_equal(xa["isect_local"], xb["isect_local"])
    for a, b in zip(ca, cb):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _build_host():
    import lisreg
    lisreg.lib()
    subprocess.check_call(["make", "-s", "-C", HOST])


def test_globalmap_smoke_compiles():
    _build_host()
    assert os.path.exists(os.path.join(HOST, "globalmap_smoke"))


@pytest.mark.gpu
def test_globalmap_smoke_runs():
    _build_host()
    r = subprocess.run([os.path.join(HOST, "globalmap_smoke")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "globalmap_smoke ok" in r.stdout, r.stdout + r.stderr
