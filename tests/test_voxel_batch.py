"""lisreg_voxel_downsample_batch: up to 1024 device clouds through one launch sequence and one host synchronisation.

The contract is per cloud: out[0 .. n_out), n_out and status are, byte for byte, what lisreg_voxel_downsample gives for that cloud alone.
Every case runs the batch and the single calls on sentinel-filled output arenas (the clouds' outputs lie back to back, so a voxel
written past a cloud's count or into a neighbour shows) and compares the whole arenas as bytes, the counts and the statuses; the cases
named below also hold the batch against the CPU oracle (order and labels exactly, centroids bit for bit, as tests/test_voxel.py does).
No case feeds a NaN coordinate: those are outside the equality contract."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
SENTINEL = f32(-12345.678)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def scan():
    """the surface cloud of synth.make_scan(32, 900): about 20 k points, intensities drawn, labels mixed inside voxels"""
    from lisreg import synth
    c = synth.make_scan(32, 900, 4100, labelled=True)["surf"].copy()
    rng = np.random.default_rng(4100)
    c["intensity"] = rng.uniform(0, 255, len(c)).astype(f32)
    flip = rng.random(len(c)) < 0.3
    c["label"][flip] = rng.integers(0, 20, int(flip.sum())).astype(np.uint16)
    return c


def records(cloud, intensity):
    """(n, 4) device records of a PCL struct array: payload = the label bits, or the float intensity"""
    import lisreg
    rec = lisreg.pack_device_records(cloud)
    if intensity:
        rec[:, 3] = cloud["intensity"]
    return rec


def one_voxel(p, seed, tie=(7, 2)):
    """p points inside the 0.4 m voxel [2.8, 3.2) x [-2.4, -2.0) x [0.4, 0.8); the two labels of `tie` have equal counts, the larger one
    first in input order, and (p odd) one point carries a third label: the vote must fall to the smaller of the two"""
    from lisreg import synth
    rng = np.random.default_rng(seed)
    xyz = (np.array([2.8, -2.4, 0.4]) + rng.uniform(0.02, 0.38, (p, 3))).astype(f32)
    lab = np.array([tie[0]] * (p // 2) + [tie[1]] * (p // 2) + [11] * (p % 2), np.uint16)
    c = synth.to_pcl(xyz, lab)
    c["intensity"] = rng.uniform(0, 255, p).astype(f32)
    return c


def box_cloud(n, seed, size=(100.0, 100.0, 30.0), shift=(0.0, 0.0, 0.0)):
    from lisreg import synth
    rng = np.random.default_rng(seed)
    xyz = (rng.uniform(-0.5, 0.5, (n, 3)) * np.array(size) + np.array(shift)).astype(f32)
    c = synth.to_pcl(xyz, rng.integers(0, 20, n).astype(np.uint16))
    c["intensity"] = rng.uniform(0, 255, n).astype(f32)
    return c


class Arenas:
    """the batch's inputs back to back in one device buffer, its outputs (capacity records each, sentinel-filled) back to back in another"""

    def __init__(self, recs, caps):
        import lisreg
        self.ns = [len(r) for r in recs]
        self.caps = list(caps)
        self.in_off = np.concatenate([[0], np.cumsum(self.ns)]).astype(np.int64)
        self.out_off = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        live = [np.ascontiguousarray(r, f32).reshape(-1, 4) for r in recs if len(r)]
        self.d_in = lisreg.DeviceArray(np.concatenate(live) if live else np.zeros((1, 4), f32))
        self.d_out = lisreg.DeviceArray(np.full((max(int(self.out_off[-1]), 1), 4), SENTINEL, f32))
        self.in_ptrs = [self.d_in.ptr + 16 * int(o) for o in self.in_off[:-1]]
        self.out_ptrs = [self.d_out.ptr + 16 * int(o) for o in self.out_off[:-1]]

    def outputs(self):
        got = self.d_out.download(max(int(self.out_off[-1]), 1))
        return [got[int(a):int(b)] for a, b in zip(self.out_off[:-1], self.out_off[1:])]

    def free(self):
        self.d_in.free(); self.d_out.free()


def run_batch(ctx, recs, leafs, intensity, caps=None):
    A = Arenas(recs, caps if caps is not None else [len(r) for r in recs])
    n_out, status = ctx.voxel_downsample_batch_device(A.in_ptrs, A.ns, leafs, A.out_ptrs, A.caps, intensity=intensity)
    outs = A.outputs()
    A.free()
    return n_out, status, outs


def run_singles(ctx, recs, leafs, intensity, caps=None):
    """the same clouds through voxel_downsample_device one by one; a refused cloud: its error code as the status, n_out None"""
    import lisreg
    A = Arenas(recs, caps if caps is not None else [len(r) for r in recs])
    n_out, status = [], []
    for s in range(len(recs)):
        try:
            rc, n = ctx.voxel_downsample_device(A.in_ptrs[s], A.ns[s], leafs[s], A.out_ptrs[s], A.caps[s], intensity=intensity)
        except lisreg.LisregError as ex:
            rc, n = ex.code, None
        n_out.append(n); status.append(rc)
    outs = A.outputs()
    A.free()
    return n_out, status, outs


def check(ctx, recs, leafs, intensity, caps=None):
    """batch == singles: statuses, counts (where the single call reports one) and every byte of every output slice, sentinels included"""
    b_n, b_st, b_out = run_batch(ctx, recs, leafs, intensity, caps)
    s_n, s_st, s_out = run_singles(ctx, recs, leafs, intensity, caps)
    assert b_st == s_st, (b_st, s_st)
    for k, (bn, sn) in enumerate(zip(b_n, s_n)):
        assert sn is None or bn == sn, (k, bn, sn)
    for k, (bo, so) in enumerate(zip(b_out, s_out)):
        assert bo.shape == so.shape and bo.tobytes() == so.tobytes(), ("cloud", k, "n_out", b_n[k], "first difference at record",
                                                                       int(np.argmax((bits(bo) != bits(so)).any(1))) if len(bo) else -1)
    return b_n, b_st, b_out


def check_oracle(oracle, cloud, leaf, intensity, out, n_out):
    """order and labels exactly, centroids (and the intensity average) bit for bit"""
    rc, want = oracle.voxel_grid(cloud, leaf, fmt=0 if intensity else 1)
    assert rc == 0 and n_out == len(want)
    got = out[:n_out]
    assert np.array_equal(got[:, 0], want["x"]) and np.array_equal(got[:, 1], want["y"]) and np.array_equal(got[:, 2], want["z"])
    if intensity:
        assert np.array_equal(got[:, 3], want["intensity"])
    else:
        assert np.array_equal(bits(got[:, 3]) & 0xffff, want["label"].astype(np.uint32))


@pytest.mark.parametrize("intensity", [False, True])
@pytest.mark.parametrize("k", [1, 2, 8, 9, 513])
def test_cloud_counts(oracle, gpu_ctx, scan, k, intensity):
    """1, 2, 8, 9 (past the multi form's 8) and 513 clouds (1 - 40 points each: only tables hold that many)"""
    import lisreg
    if k == 513:
        rng = np.random.default_rng(513)
        sizes = rng.integers(1, 41, k)
        starts = rng.integers(0, len(scan) - 40, k)
        clouds = [scan[a:a + n] for a, n in zip(starts, sizes)]
    else:
        step = len(scan) // k
        clouds = [scan[s * step:(s + 1) * step][:2500 + 17 * s] for s in range(k)]
    leafs = [(0.2, 0.4)[s % 2] for s in range(k)]
    n_out, status, outs = check(gpu_ctx, [records(c, intensity) for c in clouds], leafs, intensity)
    assert status == [lisreg.OK] * k and all(0 < n <= len(c) for n, c in zip(n_out, clouds))
    for s in {0, k - 1}:
        check_oracle(oracle, clouds[s], leafs[s], intensity, outs[s], n_out[s])


@pytest.mark.parametrize("intensity", [False, True])
def test_mixed_sizes_in_one_batch(oracle, gpu_ctx, scan, intensity):
    """0, 1 and 2 points (the two in one voxel), 255 / 256 / 257 (the chunk) and the whole scan cloud, in one batch"""
    import lisreg
    two = one_voxel(2, 1)
    clouds = [scan[:0], scan[5:6], two, scan[100:355], scan[400:656], scan[700:957], scan, scan[:0], scan[1000:1001]]
    leafs = [0.4, 0.4, 0.4, 0.2, 0.4, 0.2, 0.4, 0.2, 0.2]
    n_out, status, outs = check(gpu_ctx, [records(c, intensity) for c in clouds], leafs, intensity)
    assert status == [lisreg.OK] * len(clouds)
    assert n_out[0] == n_out[7] == 0 and n_out[1] == n_out[2] == n_out[8] == 1 and 1000 < n_out[6] < len(scan)
    assert np.array_equal(outs[1][0, :3], records(scan[5:6], intensity)[0, :3])
    check_oracle(oracle, scan, 0.4, intensity, outs[6], n_out[6])
    check_oracle(oracle, two, 0.4, intensity, outs[2], n_out[2])


@pytest.mark.parametrize("total", [2047, 2048, 2049])
def test_batch_total_on_the_scan_tile(gpu_ctx, scan, total):
    """the batch's point count on either side of the 2048-entry tile of the head scan"""
    import lisreg
    sizes = [0, 1, 2, 255, 256, 257]
    sizes.append(total - sum(sizes))
    clouds, a = [], 0
    for n in sizes:
        clouds.append(scan[a:a + n]); a += n
    n_out, status, _ = check(gpu_ctx, [records(c, False) for c in clouds], [0.2, 0.4, 0.4, 0.2, 0.4, 0.2, 0.4], False)
    assert status == [lisreg.OK] * 7 and sum(len(c) for c in clouds) == total and n_out[0] == 0


@pytest.mark.parametrize("intensity", [False, True])
def test_one_voxel_populations_around_the_wavefront_path(oracle, gpu_ctx, intensity):
    """all points of a cloud in one voxel: 24 | 25 (kVoteBig: one thread | one wavefront), 64 | 65 (the wavefront's LDS round) and 300;
    tied labels: the smaller wins"""
    import lisreg
    pops = [24, 25, 64, 65, 300]
    clouds = [one_voxel(p, 50 + p) for p in pops]
    n_out, status, outs = check(gpu_ctx, [records(c, intensity) for c in clouds], [0.4] * 5, intensity)
    assert status == [lisreg.OK] * 5 and n_out == [1] * 5
    for c, o in zip(clouds, outs):
        check_oracle(oracle, c, 0.4, intensity, o, 1)
        if not intensity:
            assert int(bits(o[:1, 3])[0] & 0xffff) == 2            # 7 and 2 tie, 7 comes first in the input: the smaller label wins


def test_equal_keys_across_a_cloud_boundary(gpu_ctx):
    """three copies of a one-voxel cloud in a row: every cloud ends and begins at voxel index 0 — three outputs of one point each"""
    import lisreg
    c = one_voxel(7, 3)
    n_out, status, outs = check(gpu_ctx, [records(c, False)] * 3, [0.4] * 3, False)
    assert status == [lisreg.OK] * 3 and n_out == [1, 1, 1]
    assert outs[0].tobytes() == outs[1].tobytes() == outs[2].tobytes()


def test_index_spaces_that_sum_past_32_bits(oracle, gpu_ctx):
    """16 clouds over a 100 x 100 x 30 m box at leaf 0.1: about 3e8 voxel indices each (below int32), 4.8e9 in all — no joint index"""
    import lisreg
    from lisreg import synth
    clouds = [box_cloud(300 + 7 * s, 900 + s) for s in range(16)]
    spans = []
    for c in clouds:
        xyz = synth.pcl_xyz(c)
        inv = f32(1) / f32(0.1)
        div = np.floor(xyz.max(0) * inv).astype(np.int64) - np.floor(xyz.min(0) * inv).astype(np.int64) + 1
        spans.append(int(div[0] * div[1] * div[2]))
    assert max(spans) < 2 ** 31 and sum(spans) >= 2 ** 32, spans
    n_out, status, outs = check(gpu_ctx, [records(c, False) for c in clouds], [0.1] * 16, False)
    assert status == [lisreg.OK] * 16
    check_oracle(oracle, clouds[15], 0.1, False, outs[15], n_out[15])


@pytest.mark.parametrize("intensity", [False, True])
def test_leaf_too_small_in_the_middle(gpu_ctx, scan, intensity):
    """leaf 0.001 on the scan cloud overflows int32: that cloud is copied and reports LISREG_LEAF_TOO_SMALL, its neighbours are gridded"""
    import lisreg
    clouds = [scan[:3000], scan, scan[3000:7000]]
    recs = [records(c, intensity) for c in clouds]
    n_out, status, outs = check(gpu_ctx, recs, [0.4, 0.001, 0.2], intensity)
    assert status == [lisreg.OK, lisreg.LEAF_TOO_SMALL, lisreg.OK] and n_out[1] == len(scan)
    assert outs[1].tobytes() == recs[1].tobytes()
    assert 0 < n_out[0] < 3000 and 0 < n_out[2] < 4000


def test_capacity_one_short(gpu_ctx, scan):
    """the cloud in the middle has room for one voxel less than it needs: LISREG_ERR_ARG, n_out = the count needed, not a byte written;
    the others are gridded and the call itself returns LISREG_OK (the binding would raise otherwise)"""
    import lisreg
    clouds = [scan[:4000], scan[4000:9000], scan[9000:12000]]
    recs = [records(c, False) for c in clouds]
    leafs = [0.4, 0.4, 0.2]
    need, status, _ = run_batch(gpu_ctx, recs, leafs, False)
    assert status == [lisreg.OK] * 3
    caps = [len(recs[0]), need[1] - 1, len(recs[2])]
    n_out, status, outs = check(gpu_ctx, recs, leafs, False, caps)
    assert status == [lisreg.OK, lisreg.ERR_ARG, lisreg.OK] and n_out == need
    assert np.all(outs[1] == SENTINEL) and len(outs[1]) == need[1] - 1
    # the same for a cloud that would be copied: it needs out_capacity >= n
    n_out, status, outs = check(gpu_ctx, recs, [0.4, 0.001, 0.2], False, [len(recs[0]), len(recs[1]) - 1, len(recs[2])])
    assert status == [lisreg.OK, lisreg.ERR_ARG, lisreg.OK] and n_out[1] == len(recs[1]) and np.all(outs[1] == SENTINEL)


def test_infinite_coordinate(gpu_ctx, scan):
    """one inf coordinate: LISREG_ERR_ARG for that cloud only, n_out 0, nothing written"""
    import lisreg
    recs = [records(scan[:3000], False), records(scan[3000:6000], False), records(scan[6000:9000], False)]
    recs[1][1234, 1] = np.inf
    n_out, status, outs = check(gpu_ctx, recs, [0.4, 0.4, 0.4], False)
    assert status == [lisreg.OK, lisreg.ERR_ARG, lisreg.OK] and n_out[1] == 0 and np.all(outs[1] == SENTINEL)
    assert n_out[0] > 0 and n_out[2] > 0


@pytest.mark.parametrize("intensity", [False, True])
def test_mixed_leaves(oracle, gpu_ctx, scan, intensity):
    import lisreg
    leafs = [0.05, 0.2, 0.4, 0.6, 2.0]
    clouds = [scan[1000 * s:1000 * s + 9000] for s in range(5)]
    n_out, status, outs = check(gpu_ctx, [records(c, intensity) for c in clouds], leafs, intensity)
    assert status == [lisreg.OK] * 5
    for c, lf, o, n in zip(clouds, leafs, outs, n_out):
        check_oracle(oracle, c, lf, intensity, o, n)


def test_repeat_calls_and_stale_scratch(gpu_ctx, scan):
    """a large batch, then a small one on the same context (scratch sized and filled by the large one), then the large one again:
    the same batch gives identical bytes, and each equals its single calls"""
    big = [records(scan[500 * s:500 * s + 6000], False) for s in range(12)]
    big_leafs = [(0.2, 0.4, 0.6)[s % 3] for s in range(12)]
    small = [records(scan[:40], False), records(one_voxel(30, 9), False)]
    first = check(gpu_ctx, big, big_leafs, False)
    check(gpu_ctx, small, [0.4, 0.4], False)
    again = run_batch(gpu_ctx, big, big_leafs, False)
    assert first[0] == again[0] and first[1] == again[1]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first[2], again[2]))


@pytest.mark.parametrize("intensity", [False, True])
def test_clouds_far_from_the_origin(oracle, gpu_ctx, intensity):
    """8 000 m out (tests/test_far_frame.py's `edge` frame): floorf(x * inv_leaf) is about 160 000 at leaf 0.05 and min_b is negative on
    two axes"""
    import lisreg
    shift = (8000.0, -8000.0, -200.0)
    clouds = [box_cloud(4000, 70, (60.0, 60.0, 8.0), shift), box_cloud(3000, 71, (20.0, 20.0, 4.0), shift), box_cloud(5000, 72, (80.0, 80.0, 10.0), shift)]
    leafs = [0.4, 0.05, 0.2]
    n_out, status, outs = check(gpu_ctx, [records(c, intensity) for c in clouds], leafs, intensity)
    assert status == [lisreg.OK] * 3
    for c, lf, o, n in zip(clouds, leafs, outs, n_out):
        check_oracle(oracle, c, lf, intensity, o, n)


from test_caller_stream import env  # noqa: E402,F401  (the busy caller's stream: gate, context and stream of tests/test_caller_stream.py)


def test_on_a_callers_busy_stream(env, oracle):
    """tests/test_caller_stream.py section A for this entry point: one cloud of the batch arrives LATE on the caller's busy stream; the
    ordered run gives the idle-stream bytes, the control run (context on its own stream) the decoy's"""
    from test_caller_stream import labelled_cloud, late_case, moved, records_pcl, same, to_host
    e = env
    rec, other = labelled_cloud(43), labelled_cloud(44, 3001)
    n, m = len(rec), len(other)
    d_other = e.D(other)

    def make(dst):
        outs = [e.D(np.zeros((m, 4), f32)), e.D(np.zeros((n, 4), f32)), e.D(np.zeros((m, 4), f32))]
        run = lambda: e.ctx.voxel_downsample_batch_device([d_other.ptr, dst.ptr, d_other.ptr], [m, n, m], [0.2, 0.4, 0.6], [o.ptr for o in outs], [m, n, m])
        fetch = lambda r: dict(n_out=r[0], status=r[1], clouds=[to_host(o.ptr, (c, 4))[:k] for o, c, k in zip(outs, (m, n, m), r[0])])
        return run, fetch
    o, od = late_case(e, "voxel_downsample_batch_device", rec, moved(rec), make)
    assert o["status"] == [0, 0, 0] and same(o["clouds"][0], od["clouds"][0]) and same(o["clouds"][2], od["clouds"][2])
    for g, cloud, leaf in zip(o["clouds"], (other, rec, other), (0.2, 0.4, 0.6)):
        _, do = oracle.voxel_grid(records_pcl(cloud), leaf)
        assert len(g) == len(do) and np.array_equal(g[:, 0], do["x"]) and np.array_equal(g[:, 1], do["y"]) and np.array_equal(g[:, 2], do["z"])
        assert np.array_equal(bits(g[:, 3]) & 0xffff, do["label"].astype(np.uint32))


def test_argument_errors_touch_nothing(gpu_ctx, scan):
    """refused before the first launch, with every buffer as it was and the job named in the text"""
    import lisreg
    recs = [records(scan[:2000], False), records(scan[2000:5000], False)]

    def refused(word, ns=None, leafs=(0.4, 0.2), n_clouds=None, out_ptrs=None):
        A = Arenas(recs, [len(r) for r in recs])
        k = n_clouds if n_clouds is not None else 2
        ins = (A.in_ptrs * k)[:k]
        outs = (out_ptrs(A) if out_ptrs else A.out_ptrs * k)[:k]
        with pytest.raises(lisreg.LisregError) as ex:
            gpu_ctx.voxel_downsample_batch_device(ins, ((ns or A.ns) * k)[:k], (list(leafs) * k)[:k], outs, (A.caps * k)[:k])
        assert ex.value.code == lisreg.ERR_ARG and word in str(ex.value), str(ex.value)
        assert all(np.all(o == SENTINEL) for o in A.outputs())
        got_in = A.d_in.download(int(A.in_off[-1]))
        assert got_in.tobytes() == np.concatenate(recs).tobytes()
        A.free()
    refused("job 1", out_ptrs=lambda A: [A.out_ptrs[0], A.in_ptrs[0] + 16 * 100])       # an out inside another job's in
    refused("job 1", out_ptrs=lambda A: [A.out_ptrs[0], A.out_ptrs[0] + 16 * (A.caps[0] - 1)])     # an out on another job's out
    refused("job 0", out_ptrs=lambda A: [A.in_ptrs[0], A.out_ptrs[1]])                  # in place
    refused("n_clouds", n_clouds=1025)
    refused("job 1", ns=[2000, -1])
    refused("job 0", leafs=(0.0, 0.2))
    # and the context still works
    n_out, status, _ = check(gpu_ctx, recs, [0.4, 0.2], False)
    assert status == [lisreg.OK] * 2


def test_end_to_end_from_feature_extraction(gpu_ctx):
    """three 16 x 450 sweeps through extract_features_batch_device; their corner and surface clouds, where the extraction left them,
    through the batch call (leaves 0.2 / 0.4, .w averaged): the six results equal the six single calls"""
    import lisreg
    from lisreg import synth
    h, w = 16, 450
    names = ("deskewed", "corner", "surface", "corner_sharp", "surface_sharp")
    sweeps = [synth.make_raw_scan(h, w, 8800 + k) for k in range(3)]
    recs = []
    for c in sweeps:
        r = np.zeros((len(c), 4), f32)
        r[:, 0], r[:, 1], r[:, 2] = c["x"], c["y"], c["z"]
        r[:, 3] = c["ring"].astype(np.uint32).view(f32)
        recs.append(r)
    cap = h * w
    dins = [lisreg.DeviceArray(r) for r in recs]
    outs = [{k: lisreg.DeviceArray(np.zeros((cap, 4), f32)) for k in names} for _ in sweeps]
    counts = gpu_ctx.extract_features_batch_device([d.ptr for d in dins], [len(r) for r in recs], lisreg.FeatureParams(h, w, 1, 0.0, 70.0, 1.0, 0.1),
                                                   [{k: v.ptr for k, v in o.items()} for o in outs], cap)
    in_ptrs = [outs[s][k].ptr for s in range(3) for k in ("corner", "surface")]
    ns = [counts[s][k] for s in range(3) for k in ("corner", "surface")]
    leafs = [0.2, 0.4] * 3
    assert min(ns) > 0
    d_out = lisreg.DeviceArray(np.full((sum(ns), 4), SENTINEL, f32))
    off = np.concatenate([[0], np.cumsum(ns)])
    out_ptrs = [d_out.ptr + 16 * int(o) for o in off[:-1]]
    n_out, status = gpu_ctx.voxel_downsample_batch_device(in_ptrs, ns, leafs, out_ptrs, ns, intensity=True)
    got = d_out.download(sum(ns))
    d_one = lisreg.DeviceArray(np.full((sum(ns), 4), SENTINEL, f32))
    for j in range(6):
        rc, n1 = gpu_ctx.voxel_downsample_device(in_ptrs[j], ns[j], leafs[j], d_one.ptr + 16 * int(off[j]), ns[j], intensity=True)
        assert (rc, n1) == (status[j], n_out[j]) == (lisreg.OK, n_out[j]) and 0 < n1 <= ns[j]
    assert got.tobytes() == d_one.download(sum(ns)).tobytes()
