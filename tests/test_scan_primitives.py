"""The three primitives under every subsystem — exclusive scan, its pair form, the bounding-box reduction — at every regime of their own.

`exclusive_scan` (lisreg_index.hip) has three forms chosen by size alone, each tiled kernel a vector and a scalar path chosen by pointer
alignment and tile fill, the pair form of the cell rows a dispatch of its own; the bounding-box kernels cap their grids and read larger
clouds with a grid stride.  The hook `lisreg_test_scan` runs the scan as production dispatches it (no forced form, the thresholds as
they stand), so the sizes below are what selects the form: the CPU tests read the three constants out of the source and fail until
SIZES straddles every boundary they imply.  Reference: numpy.cumsum in int64, asserted to stay below 2^31, cast to int32; every
comparison is exact.

The same regimes through public entry points: the compaction of bbx_filter (flags -> scan -> index list -> gather) against the numpy
mask applied to the records, compared as bytes; cloud_bounds and the 64-workgroup box forms (voxel_downsample_multi_device,
map_index_set_batch) on clouds whose extremes sit where a dropped stride tail or a dropped partial row would lose them."""
import functools
import os
import re

import numpy as np
import pytest

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INDEX_SRC = os.path.join(ROOT, "lis-slam_amd", "csrc", "lisreg_index.hip")

# ---------------------------------------------------------------- the size table (literal: it has to FOLLOW the constants, see the CPU tests)
SIZES = (0, 1, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049,
         8191, 8192, 8193,                       # the round boundary of k_scan_small
         16383, 16384, 16385,                    # the last small size, the first tiled size
         18431, 18433, 204799, 204801,           # 2048 k -+ 1 for k = 9 and 100
         4194303, 4194304, 4194305,              # 2048 tiles
         8388607, 8388608,                       # the last fused size
         8388609,                                # the first three-launch size: 4097 tiles, three rounds of k_scan_tops
         8390657)                                # 4098 tiles
BIG = 1 << 20                                    # above this: three value patterns, so that the file stays fast
INT_MAX = 2 ** 31 - 1


def scan_constants():
    """kScanBlock, kScanItems, kScanTile, kScanFusedMaxTiles, kScanSmallMax as lisreg_index.hip defines them, and the entries k_scan_small
    takes per round."""
    text = open(INDEX_SRC).read()
    env = {}
    for name, expr in re.findall(r"constexpr\s+int\s+(kScan\w+)\s*=\s*([^;]+);", text):
        assert re.fullmatch(r"[\w\s*+()-]+", expr), (name, expr)
        env[name] = int(eval(expr, {"__builtins__": {}}, dict(env)))
    m = re.search(r"__launch_bounds__\((\d+)\)\s*void\s+k_scan_small\b", text)
    assert m and re.search(r"b0\s*\+=\s*%s\s*\*\s*kScanItems" % m.group(1), text), "k_scan_small: threads x items per round not found"
    env["small_round"] = int(m.group(1)) * env["kScanItems"]
    return env


def scan_form(n, k):
    """the form exclusive_scan dispatches for n entries: 'small', 'fused' or 'three'"""
    if n <= k["kScanSmallMax"]:
        return "small"
    return "fused" if -(-n // k["kScanTile"]) <= k["kScanFusedMaxTiles"] else "three"


# ---------------------------------------------------------------- value patterns
def _last_tile_start(n, tile=2048):
    return ((n - 1) // tile) * tile if n > 0 else 0


def _pattern(name, n):
    """int32[n], or None where the pattern needs a larger n.  Every total stays below 2^31 - 1 (255 x 8 390 657 = 2 139 617 535)."""
    rng = np.random.default_rng(n * 131 + sum(map(ord, name)))
    v = np.zeros(n, np.int32)
    if name == "zeros":
        return v
    if name == "ones":
        return v + 1
    if name == "rand01_sparse":
        return (rng.random(n) < 0.01).astype(np.int32)
    if name == "rand01":
        return (rng.random(n) < 0.5).astype(np.int32)
    if name == "rand255":
        return rng.integers(0, 256, n, dtype=np.int32)
    if name == "one_first":
        if n < 1: return None
        v[0] = 1; return v
    if name == "one_last":
        if n < 2: return None
        v[n - 1] = 1; return v
    b = _last_tile_start(n)
    if name == "one_tile_last":                  # the last slot in front of the last tile boundary inside the array
        if b < 1: return None
        v[b - 1] = 1; return v
    if name == "one_tile_first":                 # the first slot behind it
        if b < 1: return None
        v[b] = 1; return v
    if name == "big":                            # a partial sum that a narrowed or float accumulator cannot carry
        if b < 2048: return None
        v[2047] = 2000000000; v[b:] = 1; return v
    raise KeyError(name)


PATTERNS = ("zeros", "ones", "rand01_sparse", "rand01", "rand255", "one_first", "one_last", "one_tile_last", "one_tile_first", "big")
PATTERNS_BIG = ("rand01", "rand255", "big")
OFFSETS = ((1, 0), (0, 1), (3, 3), (1, 2))


def _ref(v):
    s = np.concatenate([[0], np.cumsum(v, dtype=np.int64)])
    assert s[-1] < 2 ** 31
    return s.astype(np.int32)


# ---------------------------------------------------------------- CPU: the table follows the constants
def test_size_table_straddles_every_threshold():
    k = scan_constants()
    tile, small, fused, rnd = k["kScanTile"], k["kScanSmallMax"], k["kScanFusedMaxTiles"], k["small_round"]
    assert tile == k["kScanBlock"] * k["kScanItems"]
    boundaries = {
        "one tile": tile,
        "a round of k_scan_small": rnd,
        "the last small size (kScanSmallMax)": small,
        "a round of k_scan_tops / 2048 tiles": tile * tile,
        "the last fused size (kScanFusedMaxTiles tiles)": fused * tile,
    }
    for what, c in boundaries.items():
        for n in (c - 1, c, c + 1):
            assert n in SIZES, f"{what}: boundary {c} moved, SIZES lacks {n}"
    for kk in (9, 100):                                              # tile boundaries inside the tiled form, partial last tile on either side
        assert kk * tile - 1 in SIZES and kk * tile + 1 in SIZES and kk * tile > small
    assert (fused + 1) * tile + 1 in SIZES                           # one tile more than the first three-launch size
    forms = [scan_form(n, k) for n in SIZES]
    assert SIZES == tuple(sorted(SIZES)) and forms == sorted(forms, key=("small", "fused", "three").index)
    assert scan_form(small, k) == "small" and scan_form(small + 1, k) == "fused"
    assert scan_form(fused * tile, k) == "fused" and scan_form(fused * tile + 1, k) == "three"
    assert forms.count("three") >= 2
    # k_scan_tops scans `tile` totals per round: the first three-launch size must need more than one round, or its carry is never used
    assert -(-(fused + 1) // tile) >= 2
    assert rnd < small, "k_scan_small must run more than one round somewhere"
    for a, b in PAIR_SIZES:                                          # the pair form: one tile, both orders, the fused limit and the fall-back
        assert max(a, b) > 0
    assert (tile, tile + 1) in PAIR_SIZES and (tile + 1, tile) in PAIR_SIZES
    assert (small + 1, 5) in PAIR_SIZES and (fused * tile, tile + 1) in PAIR_SIZES and (fused * tile + 1, 100) in PAIR_SIZES


def test_value_patterns_fit_int32():
    assert 255 * max(SIZES) <= INT_MAX and 255 * max(max(p) for p in PAIR_SIZES) <= INT_MAX
    for n in [s for s in SIZES if s <= BIG]:
        for name in PATTERNS:
            v = _pattern(name, n)
            if v is not None:
                assert v.dtype == np.int32 and len(v) == n and v.min(initial=0) >= 0 and int(v.sum(dtype=np.int64)) <= INT_MAX
    v = _pattern("big", 8390657)
    assert int(v.sum(dtype=np.int64)) == 2000000000 + 1 and v[2047] == 2000000000 and v[8390656] == 1
    assert {n for n in SIZES if _pattern("big", n) is not None} == {n for n in SIZES if n > 2048}
    # a float accumulator loses the ones behind 2e9; a 16-bit one the 2e9 itself
    assert f32(2000000000) + f32(1) == f32(2000000000)
    r = _ref(np.array([3, 0, 5], np.int32))
    assert r.tolist() == [0, 3, 3, 8] and r.dtype == np.int32


PAIR_SIZES = ((0, 2049), (2049, 0), (1, 1), (2048, 2049), (2049, 2048), (16385, 5), (8388608, 2049), (8388609, 100))


# ---------------------------------------------------------------- GPU: the hook
def _check(got, v, what):
    want = _ref(v)
    if not np.array_equal(got, want):
        i = int(np.flatnonzero(got != want)[0])
        raise AssertionError(f"{what}: first difference at out[{i}]: got {got[i]}, want {want[i]} (n = {len(v)})")


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_hip_exclusive_scan(gpu_ctx, n):
    for name in (PATTERNS if n <= BIG else PATTERNS_BIG):
        v = _pattern(name, n)
        if v is None:
            continue
        _check(gpu_ctx.test_scan(v), v, f"{name}, out of place")
        _check(gpu_ctx.test_scan(v, in_place=True), v, f"{name}, in place")
    v = _pattern("rand01", n)
    for io, oo in OFFSETS:                                           # either pointer off 16 bytes: the scalar path of every tiled kernel
        _check(gpu_ctx.test_scan(v, in_offset=io, out_offset=oo), v, f"rand01, offsets ({io}, {oo})")
    _check(gpu_ctx.test_scan(v, in_offset=3, out_offset=3, in_place=True), v, "rand01, in place at offset 3")


@pytest.mark.gpu
@pytest.mark.parametrize("n0,n1", PAIR_SIZES)
def test_hip_exclusive_scan_pair(gpu_ctx, n0, n1):
    # different patterns in the two halves: a half that read the other's tile totals would show
    for p0, p1 in (("rand255", "rand01"), ("rand01", "ones"), ("zeros", "rand255")):
        v = [_pattern(p0, n0), _pattern(p1, n1)]
        runs = [dict(), dict(in_place=True), dict(in_offset=1, out_offset=2)] if p0 == "rand255" else [dict()]
        for kw in runs:
            got = gpu_ctx.test_scan(v[0], v[1], **kw)
            for h in range(2):
                if len(v[h]) == 0:
                    assert got[h] is None                            # off, as in production: neither written nor returned
                else:
                    _check(got[h], v[h], f"half {h} of ({p0}, {p1}) {kw}")


@pytest.mark.gpu
def test_hip_test_scan_argument_errors(gpu_ctx):
    import ctypes as C
    import lisreg
    L, h = gpu_ctx._L, gpu_ctx._h
    ip = C.POINTER(C.c_int)
    a = np.arange(5, dtype=np.int32); o = np.zeros(6, np.int32); o1 = np.zeros(6, np.int32)
    A, O, O1 = a.ctypes.data_as(ip), o.ctypes.data_as(ip), o1.ctypes.data_as(ip)
    bad = [
        (None, 5, None, 0, 0, 0, 0, O, None),                        # NULL input
        (A, 5, None, 0, 0, 0, 0, None, None),                        # NULL output
        (A, 0, None, 0, 0, 0, 0, None, None),                        # ... also for n0 = 0: out0[0] is written
        (A, 5, A, 5, 0, 0, 0, O, None),                              # NULL output of the second half
        (A, -1, None, 0, 0, 0, 0, O, None), (A, 5, A, -1, 0, 0, 0, O, O1),      # negative sizes
        (A, 5, None, 3, 0, 0, 0, O, None),                           # n1 without in1
        (A, 5, None, 0, 4, 0, 0, O, None), (A, 5, None, 0, -1, 0, 0, O, None),
        (A, 5, None, 0, 0, 4, 0, O, None), (A, 5, None, 0, 0, -1, 0, O, None),  # offsets outside 0 .. 3
        (A, 5, None, 0, 1, 2, 1, O, None),                           # in place with differing offsets
    ]
    for args in bad:
        assert L.lisreg_test_scan(h, *args) == lisreg.ERR_ARG, args
    assert np.all(o == 0)
    with pytest.raises(lisreg.LisregError):
        gpu_ctx.test_scan(a, in_offset=2, out_offset=1, in_place=True)
    e = gpu_ctx.test_scan(a[:0])                                     # n0 = 0 is valid
    assert e.tolist() == [0]
    assert gpu_ctx.test_scan(a[:0], in_offset=2, out_offset=2, in_place=True).tolist() == [0]
    assert L.lisreg_test_scan(h, None, 0, None, 0, 0, 0, 0, O, None) == lisreg.OK and o[0] == 0
    assert gpu_ctx.test_scan(a[:0], a[:0]) == (None, None)           # both halves off: nothing runs
    assert L.lisreg_test_scan(h, None, 0, A, 5, 0, 0, 0, None, O) == lisreg.OK and o.tolist() == [0, 0, 1, 3, 6, 10]


# ---------------------------------------------------------------- GPU: compaction through bbx_filter / bbx_filter_device
# Faces exactly representable in float, except max_y: a double between 2.0f and the next float, so 2.0f is inside and the next float is not.
BOX = np.array([-1.0, -2.0, -0.5, 1.0, 2.0 + 1e-9, 0.5])
HALF = np.array([1.0, 2.0, 0.5], f32)
BBX_SIZES = (1, 2047, 2048, 2049, 16384, 16385, 65537, 8390657)
SETS_ALL = ("none", "all", "first", "last", "every2048")
SETS_SMALL = SETS_ALL + ("half", "alternating")
WEIRD_W = np.array([0x7fc00000, 0xff800000, 0x7f800001, 0xffffffff, 0x7f800000, 0x80000000], np.uint32)      # NaNs, infinities, -0


@functools.lru_cache(maxsize=1)
def _bbx_body(n):
    """Two candidate positions per record — well inside the box (at least half of every half-width from a face) and well outside (one
    coordinate two to three half-widths out) — and payload bits, some of them non-finite."""
    rng = np.random.default_rng(7000 + n)
    inside = (rng.uniform(-0.5, 0.5, (n, 3)) * HALF).astype(f32)
    outside = inside.copy()
    ax = rng.integers(0, 3, n)
    outside[np.arange(n), ax] = (rng.choice(np.array([-1.0, 1.0]), n) * rng.uniform(2.0, 3.0, n) * HALF[ax]).astype(f32)
    w = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    at = rng.integers(0, n, min(n, 64))
    w[at] = WEIRD_W[np.arange(len(at)) % len(WEIRD_W)]
    return inside, outside, w


def _survivors(name, n):
    i = np.arange(n)
    if name == "none": return np.zeros(n, bool)
    if name == "all": return np.ones(n, bool)
    if name == "first": return i == 0
    if name == "last": return i == n - 1
    if name == "every2048": return i % 2048 == 0
    if name == "half": return np.random.default_rng(n).random(n) < 0.5
    if name == "alternating": return i % 2 == 0
    raise KeyError(name)


def _bbx_case(name, n):
    """records [n, 4] float32 whose points inside BOX (strictly) are exactly the survivor set `name`; points exactly on each face planted
    among the outside ones (a coordinate equal to its bound is not inside), 2.0f below the in-between max_y among the inside ones."""
    inside, outside, w = _bbx_body(n)
    want_in = _survivors(name, n)
    xyz = np.where(want_in[:, None], inside, outside)
    out_at, in_at = np.flatnonzero(~want_in), np.flatnonzero(want_in)
    faces = [(0, f32(-1.0)), (1, f32(-2.0)), (2, f32(-0.5)), (0, f32(1.0)), (2, f32(0.5)), (1, np.nextafter(f32(2.0), f32(3.0)))]
    if len(out_at):
        spots = out_at[np.unique(np.linspace(0, len(out_at) - 1, min(len(out_at), 3 * len(faces))).astype(int))]
        for j, at in enumerate(spots):
            ax, val = faces[j % len(faces)]
            xyz[at] = inside[at]; xyz[at, ax] = val
    if len(in_at):
        at = in_at[len(in_at) // 2]
        xyz[at, 1] = f32(2.0)
    rec = np.empty((n, 4), f32)
    rec[:, :3] = xyz
    rec[:, 3] = w.view(f32)
    p = xyz.astype(np.float64)
    mask = np.all((p > BOX[:3]) & (p < BOX[3:]), axis=1)             # the reference: float coordinates against double bounds, strictly
    assert np.array_equal(mask, want_in)
    # every point that is not on a face is far from all of them: at least a quarter of a half-width
    gap = np.minimum(np.abs(p - BOX[:3]), np.abs(p - BOX[3:])).min(1)
    assert np.all((gap < 1e-6) | (gap >= 0.24 * HALF.min()))
    return rec, mask


XYZI32 = np.dtype({"names": ["x", "y", "z", "intensity"], "formats": ["<f4"] * 4, "offsets": [0, 4, 8, 16], "itemsize": 32})


@pytest.mark.gpu
@pytest.mark.parametrize("n,name", [(n, s) for n in BBX_SIZES for s in (SETS_SMALL if n < BIG else SETS_ALL)])
def test_hip_bbx_filter_compaction(gpu_ctx, n, name):
    import lisreg
    rec, mask = _bbx_case(name, n)
    bits = rec.view(np.uint32)
    din, dout = lisreg.DeviceArray(rec), lisreg.DeviceArray(np.zeros_like(rec))
    # host structs: 32 bytes, the padding filled too (the survivors are moved as whole records)
    raw = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8) if n < BIG else np.zeros((n, 32), np.uint8)
    cloud = raw.view(XYZI32).reshape(n)
    cloud["x"], cloud["y"], cloud["z"], cloud["intensity"] = rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3]
    for delete in (False, True):
        keep = mask != delete
        want = bits[keep]
        m = gpu_ctx.bbx_filter_device(din.ptr, n, BOX, delete, dout.ptr)
        assert m == len(want)
        assert np.array_equal(lisreg.device_to_host(dout.ptr, (m, 4), np.uint32), want)          # same records, same order, every bit
        got = gpu_ctx.bbx_filter(cloud, BOX, delete)
        assert len(got) == len(want) and np.array_equal(got.view(np.uint8).reshape(-1, 32), raw[keep])
    for delete in (False, True):                                     # in place (device records): out == in
        din.upload(rec)
        want = bits[mask != delete]
        m = gpu_ctx.bbx_filter_device(din.ptr, n, BOX, delete, din.ptr)
        assert m == len(want)
        assert np.array_equal(lisreg.device_to_host(din.ptr, (m, 4), np.uint32), want)
    din.free(); dout.free()


# ---------------------------------------------------------------- GPU: cloud_bounds (256 workgroups: a grid stride above 65 536 points)
BOUNDS_SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 131073, 200000)
PLANT_AT = (0, 255, 256, 65535, 65536, 65537, 131071)


def _plant_indices(n, rot):
    """where the six extremes (min x, y, z, max x, y, z) go: distinct points where the cloud has six of the listed indices, and never the
    minimum and the maximum of one coordinate in one point unless the cloud IS one point"""
    avail = sorted({i for i in PLANT_AT + (n - 1,) if i < n})
    k = len(avail)
    idx = [avail[(e + (e // 3 if k == 3 else 0) + rot) % k] for e in range(6)]
    assert k == 1 or all(idx[e] != idx[e + 3] for e in range(3))
    assert k < 6 or len(set(idx)) == 6
    return idx


def _extreme_cloud(n, seed, idx, reach=20.0, half=10.0):
    """uniform in a cube of half-width `half`; extreme e sits at idx[e], `reach` + e away from the centre, alone out there"""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-half, half, (n, 3)).astype(f32)
    for e, at in enumerate(idx):
        xyz[at, e % 3] = f32((reach + e) * (-1.0 if e < 3 else 1.0))
    return xyz


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOUNDS_SIZES)
def test_hip_cloud_bounds_planted_extremes(gpu_ctx, n):
    from lisreg import synth
    for rot in range(4):                                             # which coordinate sits at which index rotates
        idx = _plant_indices(n, rot)
        xyz = _extreme_cloud(n, 100 * n + rot, idx)
        want = np.concatenate([xyz.min(0), xyz.max(0)]).astype(np.float64)
        if n > 1:
            for e, at in enumerate(idx):                             # each extreme is held by the planted point alone
                col = xyz[:, e % 3]
                assert (col == want[e]).sum() == 1 and col[at] == want[e]
        got = gpu_ctx.cloud_bounds(synth.to_pcl(xyz))
        assert np.array_equal(got, want), (n, rot, idx, got, want)


def test_planted_cases_are_what_they_claim():
    """the constructions' own assertions (survivor sets decided by the reference alone, extremes held by one point each), without a device"""
    for n in [s for s in BBX_SIZES if s < BIG]:
        for name in SETS_SMALL:
            rec, mask = _bbx_case(name, n)
            assert rec.shape == (n, 4) and mask.sum() == _survivors(name, n).sum()
    assert not np.all(np.isfinite(_bbx_case("half", 2049)[0][:, 3]))
    for n in BOUNDS_SIZES:
        seen = set()
        for rot in range(4):
            idx = _plant_indices(n, rot)
            seen.update(idx)
            xyz = _extreme_cloud(n, 100 * n + rot, idx)
            assert np.abs(xyz).max() == f32(25.0) and (n <= 6 or np.abs(xyz).min() < 10.0)
        assert seen == {i for i in PLANT_AT + (n - 1,) if i < n}     # over the rotations every listed index holds an extreme
    clouds = _multi_clouds()
    assert len(clouds) == 8 and sorted(len(r) for r in clouds)[:2] == [0, 1] and all(16385 <= len(r) <= 40000 for r in clouds if len(r) > 1)


# ---------------------------------------------------------------- GPU: the 64-workgroup forms (a grid stride above 16 384 points per cloud)
MULTI_N = (24001, 0, 16385, 1, 40000, 16386, 32769, 16387)          # kVoxelMultiMax = 8 clouds: one empty, one single point
LEAF = 0.5


@functools.lru_cache(maxsize=1)
def _multi_clouds():
    """records [n, 4] per cloud: the body uniform in a 6 m cube (10 to 25 points per 0.5 m voxel), and in every coordinate ONE extreme — the
    minimum or the maximum, rotating — held alone by a point at index 16 384, 16 385 or n - 1, more than two leaves beyond the body"""
    out = []
    for s, n in enumerate(MULTI_N):
        rng = np.random.default_rng(9100 + s)
        rec = np.zeros((n, 4), f32)
        rec[:, :3] = rng.uniform(-3.0, 3.0, (n, 3)).astype(f32)
        rec[:, 3] = rng.integers(0, 4, n).astype(np.uint32).view(f32)                   # label bits (the voxel takes the majority)
        if n > 16384:
            spots = sorted({i for i in (16384, 16385, n - 1) if i < n})
            for c in range(3):
                at = spots[(c + s) % len(spots)]
                sign = -1.0 if (c + s) % 2 else 1.0
                rec[at, c] = f32(sign * (3.0 + 2.2 * LEAF + 0.07 * c))
                col = rec[:, c]
                assert at >= 16384 and (np.abs(col) >= 3.0 + 2.0 * LEAF).sum() == 1
        out.append(rec)
    return out


@pytest.mark.gpu
def test_hip_voxel_multi_boxes_equal_single_calls(gpu_ctx):
    import lisreg
    clouds = _multi_clouds()
    ins = [lisreg.DeviceArray(r if len(r) else np.zeros((1, 4), f32)) for r in clouds]
    outs = [lisreg.DeviceArray(np.zeros((max(len(r), 1), 4), f32)) for r in clouds]
    single = []
    for r, a, o in zip(clouds, ins, outs):
        rc, m = gpu_ctx.voxel_downsample_device(a.ptr, len(r), LEAF, o.ptr, max(len(r), 1))
        assert rc == 0
        single.append(lisreg.device_to_host(o.ptr, (m, 4), np.uint32))
    assert [len(x) for x in single][1] == 0 and len(single[3]) == 1 and all(300 < len(x) < 4000 for x, r in zip(single, clouds) if len(r) > 1)
    for o in outs:
        o.upload(np.zeros(o.shape, f32))
    counts = gpu_ctx.voxel_downsample_multi_device([a.ptr for a in ins], [len(r) for r in clouds], [LEAF] * len(clouds),
                                                   [o.ptr for o in outs], [max(len(r), 1) for r in clouds])
    assert counts == [len(x) for x in single]
    for s, (o, want) in enumerate(zip(outs, single)):
        assert np.array_equal(lisreg.device_to_host(o.ptr, (len(want), 4), np.uint32), want), f"cloud {s} (n = {len(clouds[s])})"


@pytest.mark.gpu
def test_hip_map_index_batch_grids_equal_single_calls(gpu_ctx):
    from lisreg import synth
    clouds = [synth.to_pcl(r[:, :3]) for r in _multi_clouds()]
    slots, ones = list(range(900, 900 + len(clouds))), list(range(920, 920 + len(clouds)))
    gpu_ctx.map_index_set_batch(slots, clouds)
    for cl, a, b in zip(clouds, slots, ones):
        gpu_ctx.map_index_set(b, cl)
        ga, gb = gpu_ctx.map_grid(a), gpu_ctx.map_grid(b)
        assert ga["n"] == gb["n"] == len(cl) and ga["dims"] == gb["dims"] and ga["n_cells"] == gb["n_cells"], (len(cl), ga, gb)
        assert np.array_equal(ga["o"], gb["o"]) and ga["cell"] == gb["cell"], (len(cl), ga, gb)
        if len(cl):                                                  # the grid starts at the minimum and reaches every planted extreme
            xyz = synth.pcl_xyz(cl)
            hi = ga["o"].astype(np.float64) + np.array(ga["dims"]) * float(ga["cell"])
            assert np.array_equal(ga["o"], xyz.min(0)) and np.all(xyz.max(0) <= hi)
    for s in slots + ones:                                           # hand the memory back
        gpu_ctx.map_index_set(s, clouds[1])
