"""Writes tests/golden/gicp_batch/gicp_parent_outputs.npz: what lisreg_gicp_align and lisreg_gicp_moments of the commit BEFORE the batch
form returned on the MI355X, as raw bytes, for every item and parameter set tests/test_gicp_batch.py uses (the shapes are
tests/gicp_batch_ref.py's) — the pin that lets lisreg_gicp_align be rewritten over GicpStepper without changing a bit.  Run with the
parent commit's build on the GPU; it uses the single calls only.

  eight_<set>    [8, 176] uint8: the batch of eight's items alone, under the parameter sets default / kind1 / cap1
  edges          [24, 176]: the size-edge items (sources of 20 .. 4 097 points against targets of 20 .. 65)
  cut3, cut4     [176]: the cut-offs that leave exactly 3 and 4 pairs
  moments        [3, 74] float64: lisreg_gicp_moments of the scene at gicp_ref.lin_poses

  python tests/golden/make_golden_gicp_batch.py"""
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "lis-slam_amd"))

import gicp_batch_ref as B  # noqa: E402
import gicp_ref as R  # noqa: E402

SLOT = 170


def main():
    import lisreg
    from lisreg import synth
    L = lisreg.lib()
    ctx = lisreg.Context(0)

    def pcl(xyz):
        return synth.to_pcl(np.ascontiguousarray(xyz, np.float32))

    def single(slot, cloud, P, guess):
        res = lisreg.GicpResult()
        g = np.ascontiguousarray(guess, np.float32).ravel()
        rc = L.lisreg_gicp_align(ctx._h, slot, cloud.ctypes.data_as(C.c_void_p), len(cloud), cloud.dtype.itemsize, lisreg.FMT_XYZIL, C.byref(P),
                                 g.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), None)
        assert rc == lisreg.OK, L.lisreg_last_error(ctx._h)
        assert C.sizeof(res) == 176
        return np.frombuffer(bytes(res), np.uint8), res

    out = {}
    Pf = lisreg.fgicp_default_params()
    sh = B.scene_shapes()
    for k, t in enumerate(sh["tgt"]):
        ctx.fgicp_set_target(SLOT + k, pcl(t), Pf)
    clouds = [None if x is None else pcl(x) for x in sh["xyz"]]
    for name, kind, kw in B.PARAM_SETS:
        P = lisreg.gicp_default_params(kind, **kw)
        rows = []
        for s, slot, g in B.EIGHT:
            raw, res = single(SLOT + slot, clouds[s], P, sh[g])
            rows.append(raw)
            print(f"{name}: source {s} slot {slot} {g}: converged {res.converged} outer {res.iters} rounds {res.n_rounds} pairs {res.n_pairs_last} "
                  f"exit {res.inner_exit}")
        out["eight_" + name] = np.stack(rows)
    P = lisreg.gicp_default_params()
    poses = R.lin_poses(sh["guess"], sh["T_true"])
    out["moments"] = np.stack([ctx.gicp_moments(SLOT, clouds[B.FULL], P, T) for T in poses])
    print("pairs of the moment cases:", out["moments"][:, 73].tolist())
    rows = []
    for nt in B.EDGE_NT:
        ctx.fgicp_set_target(SLOT + 2, pcl(R.small_cloud(nt)), Pf)
        for ns in B.EDGE_NS:
            raw, res = single(SLOT + 2, pcl(R.small_cloud(ns, seed=11)), P, B.T_SMALL.astype(np.float32))
            rows.append(raw)
            print(f"edges: {ns} points against {nt}: converged {res.converged} outer {res.iters} rounds {res.n_rounds} pairs {res.n_pairs_last}")
    out["edges"] = np.stack(rows)
    cc = B.cutoff_case()
    ctx.fgicp_set_target(SLOT + 2, pcl(cc["tgt"]), Pf)
    for want, c in cc["cuts"].items():
        raw, res = single(SLOT + 2, pcl(cc["src"]), lisreg.gicp_default_params(max_correspondence_distance=c), cc["guess"])
        out[f"cut{want}"] = raw
        print(f"cut-off {c:.6f}: {res.n_pairs_last} pairs, converged {res.converged}, outer {res.iters}, rounds {res.n_rounds}")
    ctx.close()
    path = os.path.join(HERE, "gicp_batch", "gicp_parent_outputs.npz")
    if os.environ.get("GICP_BATCH_GOLDEN_OUT"):                  # (a run that must not write into the tree)
        path = os.environ["GICP_BATCH_GOLDEN_OUT"]
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 64 * 1024


if __name__ == "__main__":
    main()
