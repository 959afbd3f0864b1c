"""The two new batch entry points on a caller's BUSY stream (lisreg_set_stream): lisreg_adjust_cloud_batch and
lisreg_extract_features_deskew_batch get their input LATE, the way section A of tests/test_caller_stream.py does it for every other
device entry point — the input buffer holds a decoy, the real records arrive behind a stall on the caller's stream, and the result must
be the real input's (ordered run), while a context left on its own stream returns the decoy's (control run).

The harness, its module-scoped fixture and the decoy are test_caller_stream's; this module runs after it, so the streams it makes do not
change which hardware queues that module's own streams land on."""
import numpy as np
import pytest

import adjust_ref as A
import test_motion_adjust as AC
import test_deskew_batch as DB
from test_caller_stream import env, late_case, moved  # noqa: F401  (env: the module-scoped fixture)

pytestmark = pytest.mark.gpu
NAMES = DB.NAMES


def test_adjust_cloud_batch_reads_a_late_input(env):
    """lisreg_adjust_cloud_batch on a caller's stream (lisreg_set_stream), built like section A of tests/test_caller_stream.py: the
    records of both sweeps arrive behind a stall on that stream, and the result must be the real input's, not the decoy's"""
    from stream_gate import to_host
    e = env
    clouds = [AC._sweeps()["full16"], AC._sweeps()["n257"]]
    names = ("drive", "all_axes")
    Ms = [AC._motion(m) for m in names]
    ns = [len(c) for c in clouds]
    cap = max(ns)
    raw = np.concatenate([AC._records(c) for c in clouds])
    times = [e.D(np.ascontiguousarray(c["time"])) for c in clouds]

    def make(dst):
        outs = [e.D(np.zeros((cap, 4), np.float32)) for _ in clouds]
        otim = [e.D(np.zeros(cap, np.float32)) for _ in clouds]

        def fetch(counts):
            return dict(counts=list(counts), rec=[to_host(o.ptr, (cap, 4))[:k] for o, k in zip(outs, counts)],
                        time=[to_host(o.ptr, (cap,))[:k] for o, k in zip(otim, counts)])
        return (lambda: e.ctx.adjust_cloud_batch_device([dst.ptr, dst.ptr + 16 * ns[0]], ns, [t.ptr for t in times], Ms, [o.ptr for o in outs],
                                                        [o.ptr for o in otim], cap)), fetch
    o, _ = late_case(e, "adjust_cloud_batch_device", raw, moved(raw), make)
    for s, c in enumerate(clouds):
        want = A.adjust_structs(c, A.MOTIONS[names[s]])
        assert o["counts"][s] == len(want)
        assert np.array_equal(o["rec"][s][:, :3].view(np.uint32), np.stack([want["x"], want["y"], want["z"]], 1).view(np.uint32)), s
        assert np.array_equal(o["time"][s].view(np.uint32), want["time"].view(np.uint32)), s


def test_deskew_batch_reads_a_late_input(env):
    """lisreg_extract_features_deskew_batch on a caller's stream (lisreg_set_stream), built like section A of
    tests/test_caller_stream.py: both sweeps' records arrive behind a stall on that stream; the result must be the real input's"""
    import lisreg
    from stream_gate import to_host
    e = env
    sweeps = DB.ten_sweeps()[2:4]
    pg, cap = DB.fparams(lisreg, 16, 450), 16 * 450
    ns = [s.n for s in sweeps]
    raw = np.concatenate([DB._records(s.c) for s in sweeps])
    dks = [s.deskew(lisreg) for s in sweeps]

    def make(dst):
        outs = [{k: e.D(np.zeros((cap, 4), np.float32)) for k in NAMES} for _ in sweeps]

        def fetch(counts):
            return [{k: to_host(o[k].ptr, (cap, 4))[: n[k]] for k in NAMES} for o, n in zip(outs, counts)]
        return (lambda: e.ctx.extract_features_deskew_batch_device([dst.ptr, dst.ptr + 16 * ns[0]], ns, pg, dks,
                                                                   [{k: v.ptr for k, v in o.items()} for o in outs], cap)), fetch
    got, _ = late_case(e, "extract_features_deskew_batch_device", raw, moved(raw, small=True), make)
    for s, g in zip(sweeps, got):
        assert DB.same_lists(g, DB.run_single(e.ctx, s, pg, cap)), s.name
        assert len(g["deskewed"]) > 1000
