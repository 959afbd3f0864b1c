"""What the NDT, VGICP and FastGICP verifiers share (the voxel table of voxel_table_build, the evaluation buffers of
eval_totals, the sort scratch) must keep: NDT and VGICP see one table of a cloud, an evaluation carries nothing over from the one
before it, and a built table survives the next users of the scratch it was built in.  Every comparison is of bytes."""
import numpy as np
import pytest

import fgicp_ref as FR
import ndt_ref as NR
import vgicp_ref as VR

SLOT = 21
SIZES = (64, 0, 65)            # of ndt_ref.DERIV_SIZES / vgicp_ref.LIN_SIZES: one workgroup, the whole source (0), two workgroups


def _pcl(xyz):
    from lisreg import synth
    return synth.to_pcl(np.ascontiguousarray(xyz, np.float32))


def _records(xyz):
    rec = np.zeros((len(xyz), 4), np.float32)
    rec[:, :3] = xyz
    return rec


def two_family_cloud():
    """ndt_ref.planted_cloud() without its NaN rows (NDT keeps such records in the sort, VGICP compacts them away: without them both
    sort the same records in the same order), plus a voxel of 48 and one of 49 points: the two sides of the lane / wavefront split"""
    xyz = NR.planted_cloud()
    xyz = xyz[~np.isnan(xyz).any(1)]
    rng = np.random.default_rng(7)
    extra = [np.array(corner) + rng.uniform(0.05, 0.95, (n, 3)) for corner, n in (((20.0, 10.0, 10.0), 48), ((22.0, 10.0, 10.0), 49))]
    return np.ascontiguousarray(np.concatenate([xyz] + extra).astype(np.float32))


def test_the_two_restatements_see_the_cloud_as_the_gpu_test_expects():
    xyz = two_family_cloud()
    assert xyz.shape == (3294, 3)
    N = NR.build_target(xyz, NR.params())
    V = VR.build_target(xyz, VR.params())
    n_ids, v_ids = np.asarray(N["cell_ids"]), np.asarray(V["cell_ids"])
    assert len(n_ids) == 10 and len(v_ids) == 12 and np.isin(n_ids, v_ids).all()
    at = np.searchsorted(v_ids, n_ids)
    assert sorted(np.asarray(N["counts"]).tolist()) == [6, 9, 12, 24, 25, 40, 48, 49, 70, 3000]
    assert np.array_equal(np.asarray(V["counts"])[at], N["counts"])
    assert np.abs(np.asarray(V["means"])[at] - N["means"]).max() == 0.0


@pytest.mark.gpu
def test_ndt_and_vgicp_see_one_table(gpu_ctx):
    import lisreg
    xyz = two_family_cloud()
    d = lisreg.DeviceArray(_records(xyz))
    for fmt, cloud in (("host", _pcl(xyz)), ("device", (d.ptr, len(xyz)))):
        gpu_ctx.ndt_set_target(SLOT, cloud, lisreg.ndt_default_params())
        gpu_ctx.vgicp_set_target(SLOT, cloud, lisreg.vgicp_default_params())
        N, V = gpu_ctx.ndt_get_voxels(SLOT), gpu_ctx.vgicp_get_voxels(SLOT)
        assert len(N["cell_ids"]) == 10 and len(V["cell_ids"]) == 12, fmt
        assert np.isin(N["cell_ids"], V["cell_ids"]).all(), fmt
        at = np.searchsorted(V["cell_ids"], N["cell_ids"])
        assert sorted(N["counts"].tolist()) == [6, 9, 12, 24, 25, 40, 48, 49, 70, 3000], fmt
        assert np.array_equal(V["counts"][at], N["counts"]), fmt
        print(f"[voxel table] {fmt}: max |mean(NDT) - mean(VGICP)| on the common cells {np.abs(V['means'][at] - N['means']).max():.3e}")
        assert V["means"][at].tobytes() == N["means"].tobytes(), fmt          # both divide the same ordered sum by the same count


@pytest.fixture(scope="module")
def scenes():
    """the scene of each family's own tests and the pose its evaluations are made at: made once, never changed"""
    n_tgt, n_src, n_guess, _ = NR.scene()
    vw, fw = VR.world(), FR.world()
    return dict(ndt=(n_tgt, n_src, NR.p_from_matrix(n_guess)), vgicp=(vw["tgt"], vw["src"], np.asarray(vw["guess"], np.float64)),
                fgicp=(fw["tgt"], fw["src"], np.asarray(fw["guess"], np.float64)))


def _set_target(ctx, family, slot, tgt):
    import lisreg
    P = getattr(lisreg, family + "_default_params")()
    getattr(ctx, family + "_set_target")(slot, _pcl(tgt), P)
    return P


def _evaluate(ctx, family, slot, P, src, pose):
    if family == "ndt":
        return ctx.ndt_derivatives(slot, _pcl(src), P, pose, True)
    return getattr(ctx, family + "_linearize")(slot, _pcl(src), P, pose, True)


@pytest.mark.gpu
def test_the_shared_evaluation_buffers_carry_nothing_over(scenes):
    """the three families alternate on one context; each family's source size goes 64, whole, 65 (the families one step apart, so that a
    large call is always followed by a one- or two-workgroup call of another family).  Every output equals that of a context that has
    made no other evaluation."""
    import lisreg
    families = ("ndt", "vgicp", "fgicp")
    mixed = lisreg.Context(0)
    params = {f: _set_target(mixed, f, SLOT, scenes[f][0]) for f in families}
    got = []
    for t in range(12):
        f = families[t % 3]
        size = SIZES[(t // 3 + t % 3) % 3]
        _, src, pose = scenes[f]
        got.append((f, size, _evaluate(mixed, f, SLOT, params[f], src[:size or len(src)], pose)))
    mixed.close()
    large = [t for t in range(11) if got[t][1] == 0]
    assert len(large) == 4 and all(got[t + 1][1] in (64, 65) and got[t + 1][0] != got[t][0] for t in large)
    alone = {}
    for f, size, _ in got:
        if (f, size) in alone:
            continue
        ctx = lisreg.Context(0)
        P = _set_target(ctx, f, SLOT, scenes[f][0])
        _, src, pose = scenes[f]
        alone[(f, size)] = _evaluate(ctx, f, SLOT, P, src[:size or len(src)], pose)
        ctx.close()
    assert len(alone) == 9
    for t, (f, size, (out, pairs)) in enumerate(got):
        want, want_pairs = alone[(f, size)]
        assert pairs == want_pairs and out.tobytes() == want.tobytes(), (t, f, size)
    assert all(alone[(f, 0)][1] > 64 for f in families)            # the whole sources do make pairs


@pytest.mark.gpu
def test_a_built_table_survives_the_next_users_of_the_scratch(gpu_ctx, scenes):
    import lisreg
    other = _pcl(VR.planted_cloud()[0][:600])

    def ndt_reads():
        V = gpu_ctx.ndt_get_voxels(SLOT + 1)
        out, pairs = gpu_ctx.ndt_derivatives(SLOT + 1, _pcl(scenes["ndt"][1]), Pn, scenes["ndt"][2], True)
        return [V[k].tobytes() for k in ("cell_ids", "counts", "means", "icov6")] + [out.tobytes(), pairs]

    def vgicp_reads():
        V = gpu_ctx.vgicp_get_voxels(SLOT + 2)
        out, pairs = gpu_ctx.vgicp_linearize(SLOT + 2, _pcl(scenes["vgicp"][1]), Pv, scenes["vgicp"][2], True)
        return [V[k].tobytes() for k in ("cell_ids", "counts", "means", "cov6")] + [out.tobytes(), pairs]

    Pn = _set_target(gpu_ctx, "ndt", SLOT + 1, scenes["ndt"][0])
    before = ndt_reads()
    rc, down = gpu_ctx.voxel_downsample(other, 0.4)
    assert rc == lisreg.OK and 0 < len(down) < len(other)
    Pv = _set_target(gpu_ctx, "vgicp", SLOT + 2, scenes["vgicp"][0])
    _set_target(gpu_ctx, "fgicp", SLOT + 2, scenes["fgicp"][0])
    assert ndt_reads() == before
    before = vgicp_reads()
    _set_target(gpu_ctx, "ndt", SLOT + 3, NR.planted_cloud())
    assert vgicp_reads() == before
