"""Free-running parts of a batch cut by plan_split_uneven ("interleave" = 2), the even halves of "interleave" = 1 and the unsplit run give
the same bits; the last solve of a fixed-iteration run also finalizes and resets its registrations (no k_finalize launch), per part when
the run is split.

Shapes of test_gpu_batch.test_interleaved_halves_do_not_change_results: scans of 16 x 300 against a 30 k-point target, one lane per
query, "interleave_min_blocks" = 4, five fixed iterations.  Batches of 2 and 3 registrations have one and two item boundaries — the ones
where the quarter rule can leave plan_split_uneven nothing but plan_split's answer."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BIG = 1 << 30


@functools.lru_cache(maxsize=None)
def _world():
    """the target and eight scans, made once: (tc, ts, cases)"""
    from lisreg import synth
    tc, ts = synth.make_submap(30000, 42)
    out = []
    for i in range(8):
        sc = synth.make_scan(16, 300, 4000 + i)
        out.append(dict(src_corner=sc["corner"], src_surf=sc["surf"],
                        T_init=synth.perturb_pose(sc["T_true"], np.random.default_rng(i)), T_true=sc["T_true"]))
    return tc, ts, out


def _blocks(case):
    return (len(case["src_corner"]) + 255) // 256 + (len(case["src_surf"]) + 255) // 256


def _even_cut(cases):
    """plan_split restated: the first item boundary at or past the middle of the workgroups, none if a half is under a quarter"""
    begin = np.concatenate([[0], np.cumsum([_blocks(c) for c in cases])])
    n = int(begin[-1])
    for i in range(1, len(cases)):
        if begin[i] * 2 >= n:
            b = int(begin[i])
            return 0 if (b * 4 < n or (n - b) * 4 < n) else b
    return 0


def _fixed(iters=5):
    import lisreg
    p = lisreg.default_params(1)
    p.fixed_iters = iters
    return p


def _ctx(front, xo, il, min_blocks=4):
    import lisreg
    c = lisreg.Context(0)
    c.set_option("search_mode", front); c.set_option("xcd_order", xo); c.set_option("lanes_per_query", 1)
    c.set_option("interleave", il); c.set_option("interleave_min_blocks", min_blocks)
    return c


@pytest.mark.parametrize("front", [1, 3, 5])
@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_cut_position_does_not_change_results(gpu_ctx, n, front):
    tc, ts, world = _world()
    cases = world[:n]
    T0 = np.array([c["T_init"] for c in cases])
    n_blocks = sum(_blocks(c) for c in cases)
    engaged = int(_even_cut(cases) > 0 and n_blocks >= 4)
    assert engaged == 1, "these batches are meant to be split"
    for xo in (0, 1):
        out = {}
        for il in (0, 1, 2):
            c = _ctx(front, xo, il)
            c.set_target(tc, ts)
            out[il] = c.align_batch(cases, T0, _fixed())
            assert c.get_option("interleaved_now") == (engaged if il else 0), (n, front, xo, il)
            c.close()
        for il in (1, 2):
            assert np.array_equal(out[0][0], out[il][0]), (n, front, xo, il)
            assert out[0][1] == out[il][1], (n, front, xo, il)


class _Device:
    """the first n scans as device records (batch_prepare_device)"""

    def __init__(self, cases):
        import lisreg
        D = lisreg.DeviceArray
        self.recs = [(D(lisreg.pack_device_records(c["src_corner"])), D(lisreg.pack_device_records(c["src_surf"]))) for c in cases]
        self.items = [dict(corner_ptr=a.ptr, n_corner=a.shape[0], surf_ptr=b.ptr, n_surf=b.shape[0]) for a, b in self.recs]
        self.T0 = np.array([c["T_init"] for c in cases], np.float32)


def _step(c):
    c.batch_run()
    return c.batch_fetch()


@pytest.mark.parametrize("front,xo", [(5, 1), (3, 1), (1, 0)])
def test_split_then_not_then_split_on_one_prepared_batch(gpu_ctx, front, xo):
    """One prepared batch run with "interleave" 2, 0, 2: each run equals a fresh unsplit context's (the dispatch tables of a split run are
    kept for the runs after it: an unsplit run in between must not read them, and the split run behind it must get its own back)."""
    tc, ts, world = _world()
    d = _Device(world[:5])
    ref_c = _ctx(front, xo, 0, BIG)
    ref_c.set_target(tc, ts); ref_c.batch_prepare_device(d.items, d.T0, _fixed())
    ref = _step(ref_c)
    assert ref_c.get_option("interleaved_now") == 0
    ref_c.close()
    for rebuild in (0, 1):
        c = _ctx(front, xo, 2)
        c.set_option("rebuild_targets_each_run", rebuild)
        c.set_target(tc, ts); c.batch_prepare_device(d.items, d.T0, _fixed())
        for il, want in ((2, 1), (2, 1), (0, 0), (0, 0), (2, 1), (1, 1), (2, 1)):
            c.set_option("interleave", il)
            got = _step(c)
            assert c.get_option("interleaved_now") == want, (front, xo, rebuild, il)
            assert np.array_equal(got[0], ref[0]) and got[1] == ref[1], (front, xo, rebuild, il)
        c.close()


def test_last_solve_finalizes_and_resets(gpu_ctx):
    """Results and the reset state after one, two and three consecutive batch_runs of one prepared batch — split (each part's last solve
    finalizes its registrations) and kept unsplit by "interleave_min_blocks" — against an early-stopping lisreg_align_batch of the same
    items, which keeps the separate finalize kernel (five iterations at most and convergence bounds nothing passes: the same five steps).
    A registration that fails the feature-count guard (never solved: its record comes from the solve kernel's early way out) and one with
    an IMU blend are among the items."""
    import lisreg
    tc, ts, world = _world()
    cases = [dict(c) for c in world[:6]]
    cases[2]["src_surf"] = cases[2]["src_surf"][:50]              # surf_min = 100: the guard fails
    cases[5]["src_surf"] = cases[5]["src_surf"][:60]              # ... and for the last registration of the second part
    imu = lisreg.Imu(); imu.imu_available = 1; imu.imu_roll_init = 0.01; imu.imu_pitch_init = -0.02
    cases[1]["imu"] = imu; cases[4]["imu"] = imu
    d = _Device(cases)
    for k in (1, 4):
        d.items[k]["imu"] = imu
    p = _fixed(); p.use_imu_blend = 1
    p_free = lisreg.default_params(1); p_free.use_imu_blend = 1
    p_free.max_iters = 5; p_free.conv_deg = 0.0; p_free.conv_cm = 0.0
    c = _ctx(5, 1, 0)
    c.set_target(tc, ts)
    ref = c.align_batch(cases, d.T0, p_free)
    c.close()
    assert [s["status"] for s in ref[1]] == [0, 0, lisreg.NOT_ENOUGH_FEATURES, 0, 0, lisreg.NOT_ENOUGH_FEATURES]
    assert all(s["iters"] == 5 for k, s in enumerate(ref[1]) if k not in (2, 5))
    assert np.array_equal(ref[0][2], d.T0[2]) and np.array_equal(ref[0][5], d.T0[5])
    for il, min_blocks, want in ((2, 4, 1), (2, BIG, 0), (0, 4, 0)):
        c = _ctx(5, 1, il, min_blocks)
        c.set_target(tc, ts); c.batch_prepare_device(d.items, d.T0, p)
        for runs in (1, 2, 3):
            for _ in range(runs):
                c.batch_run()
            got = c.batch_fetch()
            assert c.get_option("interleaved_now") == want, (il, min_blocks, runs)
            assert np.array_equal(got[0], ref[0]), (il, min_blocks, runs, np.flatnonzero((got[0] != ref[0]).any(1)))
            assert got[1] == ref[1], (il, min_blocks, runs)
        # the early-stopping entry point on the same context afterwards: it finds the done counter as a reset leaves it
        again = c.align_batch(cases, d.T0, p_free)
        assert np.array_equal(again[0], ref[0]) and again[1] == ref[1], (il, min_blocks)
        c.close()


def _tiled_records(cloud, n):
    """n device records made of the cloud's points over and over"""
    import lisreg
    rec = lisreg.pack_device_records(cloud)
    return lisreg.DeviceArray(np.ascontiguousarray(np.resize(rec, (n, 4))))


def test_default_splits_from_its_floor_and_only_there(gpu_ctx):
    """ "interleave" left at its default 0: the library itself runs a fixed-iteration batch as two free-running parts from 16384 workgroups
    up, up to 64 registrations and while no other context runs batches in between, and nothing else.  Batches at the edges — 64
    registrations of 1 + 255 workgroups = 16384 exactly, one workgroup fewer, 65 registrations — made of one scan's points tiled (the items share two device clouds
    and differ in their initial poses), one iteration against the 30 k-point target.  Split and unsplit runs of the same items give the
    same bits."""
    import lisreg
    from lisreg import synth
    tc, ts, world = _world()
    corner = _tiled_records(world[0]["src_corner"], 256)
    surf = _tiled_records(world[0]["src_surf"], 255 * 256)

    def batch(n, surf_blocks, short_last=False):
        items = [dict(corner_ptr=corner.ptr, n_corner=256, surf_ptr=surf.ptr, n_surf=surf_blocks * 256) for _ in range(n)]
        if short_last:
            items[-1]["n_surf"] -= 256
        T0 = np.array([synth.perturb_pose(world[0]["T_true"], np.random.default_rng(100 + i)) for i in range(n)], np.float32)
        return items, T0

    def run(items, T0, params, opts=()):
        c = lisreg.Context(0)
        for k, v in opts:
            c.set_option(k, v)
        c.set_target(tc, ts)
        c.batch_prepare_device(items, T0, params)
        c.batch_run(); c.batch_run()              # (the second run finds what the first one's last solve left)
        out = c.batch_fetch()
        state = (c.get_option("interleaved_now"), c.get_option("lanes_per_query"))
        c.close()
        return out, state

    one = _fixed(1)
    free = lisreg.default_params(1); free.max_iters = 1
    items, T0 = batch(64, 255)
    assert sum((it["n_corner"] + 255) // 256 + (it["n_surf"] + 255) // 256 for it in items) == 16384
    split, st = run(items, T0, one)
    assert st == (1, 1), st
    whole, st = run(items, T0, one, (("interleave_min_blocks", BIG),))
    assert st == (0, 1), st
    assert np.array_equal(split[0], whole[0]) and split[1] == whole[1]
    assert all(s["status"] == 0 and s["iters"] == 1 for s in split[1])
    halves, st = run(items, T0, one, (("interleave", 1),))
    assert st == (1, 1) and np.array_equal(halves[0], whole[0]) and halves[1] == whole[1]
    _, st = run(items, T0, free)                                          # no fixed iteration count
    assert st == (0, 1), st
    short, st = run(*batch(64, 255, short_last=True), one)               # 16383 workgroups
    assert st == (0, 1), st
    assert np.array_equal(short[0][:63], whole[0][:63])
    past, st = run(*batch(65, 255), one)                                 # 65 registrations: unsplit (as are configs[3]'s 256)
    assert st == (0, 1), st
    assert np.array_equal(past[0][:64], whole[0]) and past[1][:64] == whole[1]
    # the synchronous entry point (host clouds in, prepare, one run, fetch): the library's own split is for lisreg_batch_run only
    tile = lambda cloud, n: np.ascontiguousarray(cloud[np.arange(n) % len(cloud)])            # (keeps the point struct's stride)
    host = [dict(src_corner=tile(world[0]["src_corner"], 256), src_surf=tile(world[0]["src_surf"], 255 * 256))] * 64
    c = lisreg.Context(0)
    c.set_target(tc, ts)
    for _ in range(2):
        sync = c.align_batch(host, T0, one)
        assert c.get_option("interleaved_now") == 0
        assert np.array_equal(sync[0], whole[0]) and sync[1] == whole[1]
    c.set_option("interleave", 2)
    sync = c.align_batch(host, T0, one)
    assert c.get_option("interleaved_now") == 1 and np.array_equal(sync[0], whole[0]) and sync[1] == whole[1]
    c.close()
    # another context running batches in between: the process overlaps its batches itself, and the library leaves its own split alone
    a, b = lisreg.Context(0), lisreg.Context(0)
    for c in (a, b):
        c.set_target(tc, ts); c.batch_prepare_device(items, T0, one)
    seen = []
    for c in (a, a, b, a, a):
        c.batch_run()
        seen.append(c.get_option("interleaved_now"))
    assert seen[1:] == [1, 0, 0, 1], seen                  # (the first run: whoever ran last in this process)
    for c in (a, b):
        got = c.batch_fetch()
        assert np.array_equal(got[0], whole[0]) and got[1] == whole[1]
        c.close()


@pytest.mark.parametrize("n", [2, 3])
def test_lop_sided_boundaries_leave_the_batch_uncut(gpu_ctx, n):
    """Two and three registrations whose only item boundaries leave a part under a quarter of the workgroups (the last ones cut down to
    a workgroup or two): plan_split_uneven has plan_split's answer to give, which is "no cut" — the run is unsplit under "interleave" 1 and
    2, with the bits of "interleave" 0."""
    tc, ts, world = _world()
    cases = [dict(c) for c in world[:n]]
    for c in cases[1:]:
        c["src_corner"] = c["src_corner"][:40]; c["src_surf"] = c["src_surf"][:150 if n == 3 else 300]
    blocks = [_blocks(c) for c in cases]
    assert _even_cut(cases) == 0 and all(b * 4 < sum(blocks) for b in (sum(blocks[1:]), blocks[-1])), blocks
    T0 = np.array([c["T_init"] for c in cases])
    out = {}
    for il in (0, 1, 2):
        c = _ctx(5, 1, il)
        c.set_target(tc, ts)
        out[il] = c.align_batch(cases, T0, _fixed())
        assert c.get_option("interleaved_now") == 0, (n, il)
        c.close()
    for il in (1, 2):
        assert np.array_equal(out[0][0], out[il][0]) and out[0][1] == out[il][1], (n, il)
