"""The inputs tests/test_icpgn_batch.py and tests/golden/make_golden_icpgn_batch.py share, and the single call as its 80 result bytes.

Small scene: test_icp._case, targets of 5 000 and 30 000 points in two slots, eight sources — the full 16 x 450 sweep, cuts of 1, 63,
64, 65, 255 and 257 points (wavefront and workgroup edges) and the sweep moved 1 000 m away (no correspondences, no step).
Large scene: sources of 249 999, 250 000 and 500 000 random points (the sizes at which icp_lanes changes) against 2 000 target points."""
import ctypes as C

import numpy as np

f32 = np.float32
SLOT_A, SLOT_B, SLOT_L = 41, 42, 43
PARAM_SETS = ((12, 4.0), (3, 25.0))
CUTS = (1, 63, 64, 65, 255, 257)
LARGE_N = (249999, 250000, 500000)
LARGE_PARAMS = (2, 25.0)

_small = None
_large = None


def small_scene():
    """(target A, target B, [eight sources], [three poses])"""
    global _small
    if _small is None:
        from lisreg import synth
        from test_icp import _case
        tgt_a, src, _ = _case(81, n_map=5000, hw=(16, 450))
        tgt_b, _, _ = _case(81, n_map=30000, hw=(16, 450))
        sources = [src]
        for k in CUTS:
            sources.append(np.ascontiguousarray(src[:: max(len(src) // k, 1)][:k]))
            assert len(sources[-1]) == k
        far = src.copy(); far["x"] += f32(1000.0)
        sources.append(far)
        poses = [synth.pose_matrix(p).astype(f32) for p in ([0.0, 0.0, 0.01, 0.05, -0.05, 0.0], [0.01, -0.01, 0.0, -0.1, 0.08, 0.02],
                                                            [0.0, 0.005, -0.02, 0.2, 0.1, -0.03])]
        _small = (tgt_a, tgt_b, sources, poses)
    return _small


def small_items():
    """(source index, slot, pose index or None) of the batch of eight: both slots, differing poses, one of them NULL"""
    return [(0, SLOT_A, 0), (1, SLOT_B, None), (2, SLOT_A, 1), (3, SLOT_B, 2), (4, SLOT_A, 0), (5, SLOT_B, 1), (6, SLOT_A, 2), (7, SLOT_B, 0)]


def large_scene():
    """(target of 2 000 points, [three sources])"""
    global _large
    if _large is None:
        from lisreg import synth
        rng = np.random.default_rng(7)
        box = lambda n: (rng.random((n, 3)) * np.array([40.0, 40.0, 4.0]) - np.array([20.0, 20.0, 2.0])).astype(f32)
        tgt = synth.to_pcl(box(2000))
        _large = (tgt, [synth.to_pcl(box(n)) for n in LARGE_N])
    return _large


def set_targets(ctx, large=False):
    if large:
        ctx.map_index_set(SLOT_L, large_scene()[0])
    else:
        tgt_a, tgt_b, _, _ = small_scene()
        ctx.map_index_set(SLOT_A, tgt_a)
        ctx.map_index_set(SLOT_B, tgt_b)


def single_bytes(ctx, slot, source, iters, max_d, pose=None):
    """lisreg_icp_gn_match through the C ABI: the 80 bytes of lisreg_icpgn_result.  source: PCL structs or (device_ptr, n)."""
    import lisreg
    res = lisreg.IcpGnResult()
    g = np.ascontiguousarray(np.eye(4, dtype=f32) if pose is None else pose, f32).ravel()
    ptr, n, stride, fmt, _keep = ctx._cloud_args(source)
    ctx._chk(ctx._L.lisreg_icp_gn_match(ctx._h, slot, ptr, n, stride, fmt, iters, max_d, g.ctypes.data_as(C.POINTER(C.c_float)),
                                        C.byref(res), None))
    return bytes(res)


def small_single_all(ctx):
    """[parameter set][item] -> 80 bytes, by single calls"""
    _, _, sources, poses = small_scene()
    return [[single_bytes(ctx, slot, sources[s], it, md, None if p is None else poses[p]) for s, slot, p in small_items()]
            for it, md in PARAM_SETS]


def large_single_all(ctx):
    _, sources = large_scene()
    return [single_bytes(ctx, SLOT_L, s, LARGE_PARAMS[0], LARGE_PARAMS[1], None) for s in sources]
