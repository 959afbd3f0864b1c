"""lisreg_extract_features_deskew_batch: the IMU de-skew of lisreg_extract_features_deskew applied per sweep inside the batched extraction.

The bar is exact.  Every sweep of a batch must be byte for byte what extract_features_device(..., deskew) gives for that sweep alone
(which tests/test_features.py and tests/test_features_structured.py hold against the oracle), the coordinates of every output list must
equal oracle.deskew_points, a sweep that is not de-skewed must get extract_features_batch_device's bytes, and nothing of one sweep's
table, time stamp or start rotation may reach another sweep (the same batch in reverse order)."""
import ctypes as C

import numpy as np
import pytest

from test_features import NAMES, _imu_tables, _records
from test_features_structured import SMALL, STAMPS, T_SCAN, _edge_times, _imu_rot, fparams, sweep

pytestmark = pytest.mark.gpu
EDGE_KINDS = ("before", "after", "on_stamp", "on_first_stamp", "on_last_stamp")
SENTINEL = -7.5


class Sweep:
    """one sweep of a batch: the cloud (PointXYZIRT structs), its own IMU tables and time stamp; in HBM: records and times"""

    def __init__(self, name, c, stamps, rot, t_scan, enabled=True):
        import lisreg
        self.name, self.c, self.stamps, self.rot, self.t_scan, self.enabled = name, c, np.asarray(stamps, np.float64), np.asarray(rot, np.float64), t_scan, enabled
        self.n = len(c)
        self.din = lisreg.DeviceArray(_records(c)) if self.n else None
        self.dtime = lisreg.DeviceArray(np.ascontiguousarray(c["time"])) if self.n else None

    def deskew(self, mod, device=True):
        kw = dict(time_device_ptr=self.dtime.ptr if self.dtime else 0) if device else {}
        return mod.make_deskew(self.stamps, self.rot[:, 0], self.rot[:, 1], self.rot[:, 2], self.t_scan, enabled=self.enabled, **kw)


def _outs(cap, count=1, fill=0.0):
    import lisreg
    return [{k: lisreg.DeviceArray(np.full((cap, 4), fill, np.float32)) for k in NAMES} for _ in range(count)]


def _fetch(out, counts, cap):
    import lisreg
    return {k: lisreg.device_to_host(out[k].ptr, (cap, 4))[: counts[k]] for k in NAMES}


def run_batch(ctx, sweeps, pg, cap, deskews="own"):
    """the batch call: per sweep a dict list name -> (count, 4) records"""
    import lisreg
    outs = _outs(cap, len(sweeps))
    dks = [s.deskew(lisreg) for s in sweeps] if deskews == "own" else deskews
    counts = ctx.extract_features_deskew_batch_device([s.din.ptr if s.din else 0 for s in sweeps], [s.n for s in sweeps], pg, dks,
                                                      [{k: v.ptr for k, v in o.items()} for o in outs], cap)
    return [_fetch(o, n, cap) for o, n in zip(outs, counts)]


def run_single(ctx, s, pg, cap):
    import lisreg
    out = _outs(cap)[0]
    counts = ctx.extract_features_device(s.din.ptr if s.din else 0, s.n, pg, {k: v.ptr for k, v in out.items()}, cap, s.deskew(lisreg))
    return _fetch(out, counts, cap)


def same_lists(a, b):
    return all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in NAMES)


def check_against_oracle(oracle, s, po, got, what):
    """index lists and payloads = the oracle's on the raw sweep; coordinates = oracle.deskew_points"""
    ro = oracle.extract_features(s.c, po)
    rec = _records(s.c)
    moved = dict(zip((int(i) for i in ro["deskewed"]), oracle.deskew_points(s.c, s.deskew(oracle, device=False), ro["deskewed"]))) if s.n else {}
    for k in NAMES:
        assert len(got[k]) == len(ro[k]), (what, k, len(got[k]), len(ro[k]))
        want = rec[ro[k]].copy()
        if len(want):
            want[:, :3] = np.stack([moved[int(i)] for i in ro[k]])
        assert got[k].tobytes() == want.tobytes(), (what, k)
    return ro


def ten_sweeps():
    base = sweep(**SMALL[0])
    rot = _imu_rot(len(STAMPS))
    out = []
    for j, kind in enumerate(EDGE_KINDS):                                       # each with its own time stamp and its own table
        c = base.copy()
        c["time"] = _edge_times(len(c), kind)[0]
        out.append(Sweep(kind, c, STAMPS + j, rot * (1.0 + 0.25 * j), T_SCAN + j))
    c = base.copy()
    c["time"] = _edge_times(len(c), "on_stamp")[0]
    out.append(Sweep("one_entry", c, STAMPS[:1] + 7, rot[5:6], T_SCAN + 7))
    out.append(Sweep("disabled", c.copy(), STAMPS, rot, T_SCAN, enabled=False))
    out.append(Sweep("empty", c[:0].copy(), STAMPS, rot, T_SCAN))
    out.append(Sweep("thirty", c[:30].copy(), STAMPS + 3, -rot, T_SCAN + 3))
    sh = sweep(**SMALL[2]).copy()
    sh["time"] = _edge_times(len(sh), "after")[0]
    for f in ("x", "y", "z"):
        sh[f][:3] *= np.float32(100.0)                                          # the first three input points are out of range: no pixel
    out.append(Sweep("shuffled", sh, STAMPS + 9, rot * 0.5, T_SCAN + 9))
    return out


def test_ten_sweeps_equal_their_single_calls_and_the_oracle_in_both_orders(oracle, gpu_ctx):
    import lisreg
    sweeps = ten_sweeps()
    assert len(sweeps) == 10
    pg, po, cap = fparams(lisreg, 16, 450), fparams(oracle, 16, 450), 16 * 450
    forward = run_batch(gpu_ctx, sweeps, pg, cap)
    backward = run_batch(gpu_ctx, sweeps[::-1], pg, cap)[::-1]
    plain = run_batch(gpu_ctx, sweeps, pg, cap, deskews=None)
    for s, got, rev, raw in zip(sweeps, forward, backward, plain):
        assert same_lists(got, run_single(gpu_ctx, s, pg, cap)), (s.name, "batch differs from the single call")
        assert same_lists(got, rev), (s.name, "the sweep's bytes depend on its place in the batch")
        ro = check_against_oracle(oracle, s, po, got, s.name)
        if s.name in EDGE_KINDS:
            assert ro["deskewed"].min() == 0 and np.abs(got["deskewed"][:, :3] - raw["deskewed"][:, :3]).max() > 0.5
        if s.name == "shuffled":
            assert ro["deskewed"].min() > 2 and np.abs(got["deskewed"][:, :3] - raw["deskewed"][:, :3]).max() > 0.2
        if s.name == "disabled":
            assert same_lists(got, raw)
        if s.name == "empty":
            assert all(len(got[k]) == 0 for k in NAMES)
    assert len(forward[8]["deskewed"]) > 0 and len(forward[0]["corner"]) > 0
    # the per-sweep tables differ: two edge sweeps with the same points do not get the same coordinates
    assert forward[0]["deskewed"].shape != forward[1]["deskewed"].shape or forward[0]["deskewed"].tobytes() != forward[1]["deskewed"].tobytes()


def test_non_monotone_stamps_follow_the_linear_scan(oracle, gpu_ctx):
    """findRotation's linear scan defines the result: tables whose stamps are not sorted"""
    import lisreg
    base = sweep(**SMALL[0])
    rot = _imu_rot(len(STAMPS))
    sweeps = []
    for j, perm_seed in enumerate((1, 2)):
        c = base.copy()
        c["time"] = _edge_times(len(c), "on_stamp")[0]
        p = np.random.default_rng(perm_seed).permutation(len(STAMPS))
        sweeps.append(Sweep(f"perm{j}", c, STAMPS[p], rot, T_SCAN))
        assert np.any(np.diff(STAMPS[p]) < 0)
    pg, po, cap = fparams(lisreg, 16, 450), fparams(oracle, 16, 450), 16 * 450
    for s, got in zip(sweeps, run_batch(gpu_ctx, sweeps, pg, cap)):
        assert same_lists(got, run_single(gpu_ctx, s, pg, cap)), s.name
        check_against_oracle(oracle, s, po, got, s.name)


def test_no_enabled_sweep_gives_the_plain_batch(gpu_ctx):
    import lisreg
    sweeps = ten_sweeps()[:4]
    pg, cap = fparams(lisreg, 16, 450), 16 * 450
    outs = _outs(cap, len(sweeps))
    counts = gpu_ctx.extract_features_batch_device([s.din.ptr for s in sweeps], [s.n for s in sweeps], pg, [{k: v.ptr for k, v in o.items()} for o in outs], cap)
    want = [_fetch(o, n, cap) for o, n in zip(outs, counts)]
    for s in sweeps:
        s.enabled = False
    for deskews in (None, "own", [None] * len(sweeps)):
        got = run_batch(gpu_ctx, sweeps, pg, cap, deskews=deskews)
        assert all(same_lists(g, w) for g, w in zip(got, want)), deskews
    assert len(want[0]["corner"]) > 0


def test_four_full_size_sweeps(oracle, gpu_ctx):
    """64 x 1800, rate 2, the _imu_tables construction of tests/test_features.py, a table and a time stamp per sweep"""
    import lisreg
    from lisreg import synth
    h, w, rate = 64, 1800, 2
    sweeps = []
    for j in range(4):
        t, rot = _imu_tables(40 + j, t0=100.0 + j, n=70 - 9 * j)
        sweeps.append(Sweep(f"full{j}", synth.make_raw_scan(h, w, 7600 + j, shuffle=(j == 3)), t, rot, 100.0 + j))
    pg, po, cap = fparams(lisreg, h, w, rate), fparams(oracle, h, w, rate), h * w
    for s, got in zip(sweeps, run_batch(gpu_ctx, sweeps, pg, cap)):
        assert same_lists(got, run_single(gpu_ctx, s, pg, cap)), s.name
        check_against_oracle(oracle, s, po, got, s.name)
        assert len(got["deskewed"]) > 20000 and len(got["corner"]) > 0


def test_enabled_sweep_without_a_pixel_owner(gpu_ctx):
    import lisreg
    base = sweep(**SMALL[0])
    rot = _imu_rot(len(STAMPS))
    far = base.copy()
    for f in ("x", "y", "z"):
        far[f] *= np.float32(100.0)
    far["time"] = _edge_times(len(far), "on_stamp")[0]
    near = base.copy()
    near["time"] = far["time"]
    sweeps = [Sweep("far", far, STAMPS, rot, T_SCAN), Sweep("near", near, STAMPS, rot, T_SCAN), Sweep("far2", far.copy(), STAMPS, rot, T_SCAN)]
    pg, cap = fparams(lisreg, 16, 450), 16 * 450
    got = run_batch(gpu_ctx, sweeps, pg, cap)
    assert all(len(got[0][k]) == 0 and len(got[2][k]) == 0 for k in NAMES)
    assert same_lists(got[1], run_single(gpu_ctx, sweeps[1], pg, cap)) and len(got[1]["deskewed"]) > 1000


@pytest.mark.parametrize("h,w,ns,rate", [(64, 1800, 64, 2), (16, 450, 16, 1)])
def test_hand_over_from_pretreat_batch(gpu_ctx, h, w, ns, rate):
    """lisreg_pretreat_batch's record and time_device outputs feed the batch directly; per sweep the result is the host-struct single
    call's of tests/test_pretreat.py::test_hand_over_to_feature_extraction_with_deskew"""
    import lisreg
    import pretreat_ref as R
    from lisreg import replay, synth
    ctx = gpu_ctx
    raws = [np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"], sw["intensity"]], 1), np.float32) for sw, _ in replay.synthetic_raw_drive(2, h, w)]
    tabs = [_imu_tables(31 + ns + j, t0=100.0 + j) for j in range(len(raws))]
    fp = lisreg.FeatureParams(h, w, rate, 0.0, 70.0, 1.0, 0.1)
    cap = max(len(r) for r in raws)
    din = [lisreg.DeviceArray(r) for r in raws]
    rec = [lisreg.DeviceArray(np.zeros((cap, 4), np.float32)) for _ in raws]
    tim = [lisreg.DeviceArray(np.zeros(cap, np.float32)) for _ in raws]
    infos = ctx.pretreat_batch_device([d.ptr for d in din], [len(r) for r in raws], lisreg.default_pretreat_params(ns), [d.ptr for d in rec],
                                      [d.ptr for d in tim], cap)
    dks = [lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0 + j, time_device_ptr=tim[j].ptr) for j, (t, rot) in enumerate(tabs)]
    fcap = h * w
    outs = _outs(fcap, len(raws))
    counts = ctx.extract_features_deskew_batch_device([d.ptr for d in rec], [i["n"] for i in infos], fp, dks, [{k: v.ptr for k, v in o.items()} for o in outs], fcap)
    for j, raw in enumerate(raws):
        host = R.to_xyzirt(R.pretreat_vectorised(raw, ns), synth.XYZIRT_DTYPE)
        t, rot = tabs[j]
        want = ctx.extract_features(host, fp, lisreg.make_deskew(t, rot[:, 0], rot[:, 1], rot[:, 2], 100.0 + j))
        plain = ctx.extract_features(host, fp)
        assert np.abs(synth.pcl_xyz(want["deskewed"]) - synth.pcl_xyz(plain["deskewed"])).max() > 0.05
        got = _fetch(outs[j], counts[j], fcap)
        for k in NAMES:
            assert counts[j][k] == len(want[k]) and (k != "deskewed" or len(want[k]) > 1000), (j, k)
            assert np.array_equal(got[k][:, :3].view(np.uint32), synth.pcl_xyz(want[k]).view(np.uint32)), (j, k)
            assert np.array_equal(got[k][:, 3].view(np.uint32), want[k]["ring"].astype(np.uint32)), (j, k)


def test_refusals_leave_the_outputs_untouched(gpu_ctx):
    import lisreg
    ctx = gpu_ctx
    sweeps = ten_sweeps()[:3]
    pg, cap = fparams(lisreg, 16, 450), 16 * 450

    def refused(dks):
        outs = _outs(cap, len(sweeps), fill=SENTINEL)
        with pytest.raises(lisreg.LisregError) as e:
            ctx.extract_features_deskew_batch_device([s.din.ptr for s in sweeps], [s.n for s in sweeps], pg, dks, [{k: v.ptr for k, v in o.items()} for o in outs], cap)
        assert e.value.code == lisreg.ERR_ARG
        for o in outs:
            for k in NAMES:
                assert (lisreg.device_to_host(o[k].ptr, (cap, 4)) == SENTINEL).all()
    good = [s.deskew(lisreg) for s in sweeps]
    no_time = [s.deskew(lisreg) for s in sweeps]
    no_time[2].time_device = None                                              # an enabled sweep without time_device
    refused(no_time)
    no_table = [s.deskew(lisreg) for s in sweeps]
    no_table[1].imu_rot_y = None                                               # NULL tables
    refused(no_table)
    negative = [s.deskew(lisreg) for s in sweeps]
    negative[0].imu_pointer_cur = -1
    refused(negative)
    S = 257                                                                    # more sweeps than a call takes
    with pytest.raises(lisreg.LisregError) as e:
        ctx.extract_features_deskew_batch_device([sweeps[0].din.ptr] * S, [sweeps[0].n] * S, pg, None, [{}] * S, cap)
    assert e.value.code == lisreg.ERR_ARG
    assert len(run_batch(ctx, sweeps, pg, cap, deskews=good)[0]["deskewed"]) > 1000   # the same arguments, intact, pass
