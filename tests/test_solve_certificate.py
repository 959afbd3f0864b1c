"""The iteration-0 solve where its conditioning certificate decides (lisreg_solve.hip: k_solve).

The certificate — a 6x6 Cholesky of AtA - (eig_thresh + 2e-5 trace) I in double, on the second wavefront beside the first one's QR
solve — only says "well conditioned" or not; a "not" falls through to the restatement of cv::eigen, which decides the same.  So on
matrices whose smallest eigenvalue sits on either side of the certificate's shift, and of the threshold itself, the first step must be
the oracle's to the bit whichever way the certificate went: the degenerate flag, matP where the step is degenerate, X and the pose.

test_solve_step.py's matrices, reference chain and row packing are used as they are; this file adds a finer ladder across the shift, more
rows per registration than one round of loads takes in, and registrations that do not solve at iteration 0 (too few correspondences: the
certificate must not run, or must not matter) next to ones that do."""
import functools

import numpy as np
import pytest

from helpers import copy_params
from test_solve_step import T_START, chain_params, oracle_chain, pack_rows, same_bits, sym_matrix

f32, f64 = np.float32, np.float64
LADDER = [0.0] + [s * d for d in (1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1) for s in (1.0, -1.0)]


@functools.lru_cache(maxsize=None)
def ladder(thr):
    """[(name, AtA, AtB, count)]: lambda_min = the certificate's shift x (1 + f) and the threshold x (1 + f), f over LADDER"""
    out, seed = [], 7000
    for s in (1.0, 100.0, 1e4):
        rest = [500.0, 1e3 * s, 2e3 * s, 2e4 * s, 5e4 * s]
        for f in LADDER:
            lm_shift = (thr + 2e-5 * (1 + f) * sum(rest)) / (1 - 2e-5 * (1 + f))
            for what, lm in (("shift", lm_shift), ("threshold", thr * (1 + f))):
                for kind in ("rot", "diag", "perm"):
                    seed += 1
                    A = sym_matrix([lm] + rest, seed, kind)
                    b = (A.astype(f64) @ (np.random.default_rng(seed).normal(size=6) * 1e-2)).astype(f32)
                    out.append((f"s{s:g} {what} {f:+g} {kind}", A, b, 49 if seed % 11 == 0 else 60))
    return out


@functools.lru_cache(maxsize=None)
def ladder_reference(thr, emulate):
    import oracle_ctypes as oc
    oc.build()
    p = chain_params(oc, thr, emulate)
    return [oracle_chain(oc, p, [(A, b, cnt)], T_START) for _, A, b, cnt in ladder(thr)]


def test_the_ladder_reaches_both_verdicts_on_both_sides():
    """CPU: the oracle's first step is degenerate on some of the ladder and not on the rest, around the shift and around the threshold"""
    for thr in (100.0, 10.0):
        ref = ladder_reference(thr, 1)
        deg = {"shift": [0, 0], "threshold": [0, 0]}
        for (name, _, _, cnt), (recs, _) in zip(ladder(thr), ref):
            if cnt >= 50:
                deg[name.split()[1]][recs[0]["deg"]] += 1
        assert deg["threshold"][0] >= 20 and deg["threshold"][1] >= 20, deg
        assert deg["shift"][0] >= 60 and deg["shift"][1] == 0, deg           # (the shift lies above the threshold: never degenerate there)


@pytest.mark.gpu
@pytest.mark.parametrize("thr,emulate", [(100.0, 1), (10.0, 0)])
def test_first_step_equals_oracle_across_the_certificate(gpu_ctx, oracle, thr, emulate):
    import lisreg
    cases = ladder(thr)
    ref = ladder_reference(thr, emulate)
    p = copy_params(chain_params(oracle, thr, emulate), lisreg.Params)
    n_rows = np.array([(1, 2, 17, 40, 513)[i % 5] for i in range(len(cases))], np.int32)       # (513: more than one round of 512 rows)
    rows = pack_rows([[(A, b, cnt)] for _, A, b, cnt in cases], n_rows)
    dev = gpu_ctx.test_solve_steps(n_rows, rows, np.tile(T_START, (len(cases), 1)), p)
    n_deg = n_not = n_skipped = 0
    for i, ((name, _, _, cnt), (recs, res)) in enumerate(zip(cases, ref)):
        r, tr, stt = recs[0], dev["trace"][i, 0], dev["state"][i, 0]
        assert tr[0] == cnt and tr[55] == r["solved"] == (1 if cnt >= 50 else 0), (name, tr[0], tr[55])
        assert stt[48] == r["deg"], (name, stt[48], r["deg"])
        assert same_bits(tr[43:49], r["X"]) and same_bits(tr[49:55], r["T"]), (name, tr[43:55], r["X"], r["T"])
        assert same_bits(stt[49:51], [r["dR"], r["dT"]]) and (stt[52], stt[53], stt[54]) == (r["done"], r["iters"], r["any"]), name
        if r["deg"]:
            assert same_bits(stt[:36], r["P"]), (name, stt[:36].reshape(6, 6), r["P"].reshape(6, 6))
        elif r["solved"]:
            assert np.array_equal(stt[:36].reshape(6, 6), np.eye(6, dtype=f32)) or same_bits(stt[:36], r["P"]), name      # the certificate's I, or cv's V^-1 V
        out = dev["results"][i]
        assert same_bits(out[:6], res["T"]) and (out[6], out[9], out[10], out[11]) == (res["iters"], res["deg"], res["n_corr"], res["status"]), name
        n_deg += int(r["deg"] and r["solved"]); n_not += int(r["solved"] and not r["deg"]); n_skipped += int(not r["solved"])
    assert n_deg >= 20 and n_not >= 80 and n_skipped >= 5, (n_deg, n_not, n_skipped)
