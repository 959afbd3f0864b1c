"""The Gauss-Newton step kernels (lisreg_solve.hip: k_solve, k_finalize) tested directly, on caller-given normal equations.

`lisreg_test_solve_steps` runs the PRODUCTION kernels (reset, solve x steps, finalize) on partial rows the test supplies; the
reference is the oracle's own step, `orc_lm_step` (the tail of orc_align's loop body, which orc_align itself calls), chained by
`oracle_chain` below with orc_align's loop control, plus `orc_transform_update` and `synth.pose_matrix` — never a second copy of the
arithmetic.  lisreg_solve.hip is compiled without contraction and restates cv::solve / cv::eigen / cv::Mat::inv operation for
operation with IEEE division and square root, so device and oracle must agree BIT FOR BIT on X, T, deltaR, deltaT, the flags and
counters, and on matP wherever the scene is degenerate.

Yardstick checks (CPU, no mark):
  * the chain reproduces orc_align's own trace bit for bit (a level scene, the oblique corridor);
  * on the crafted matrices the oracle's degenerate flag equals the float64 one wherever every eigenvalue is at least
    2e-6 * lambda_max from the threshold (cv::eigen's float Jacobi was measured off by at most 5.5 * 2^-24 * lambda_max);
  * on EVERY crafted matrix the oracle flags degenerate, its matP is the float64 projector onto the top 6 - k eigenvectors (k = the
    number of rows the oracle zeroed, read off its matP) within K_BAR * 2^-24 * lambda_max / gap, gap = the distance between the last kept
    and the first zeroed eigenvalue.  Measured over this file's own matrices (132 at eig_thresh 100, 130 at 10, threshold-hugging ones
    included): K = 0.26 at most (profiles/solve_step.md); K_BAR = 4 x that.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import copy_params, pose_err

f32, f64 = np.float32, np.float64
K_BAR = 1.04           # 4 x the 0.26 measured on the CPU over all 262 degenerate matrices below (profiles/solve_step.md)
DELTAS = [0.0] + [s * d for d in (1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 3e-2) for s in (1.0, -1.0)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- crafted normal equations -----------------------------------------------------------------------------------------------------
def sym_matrix(lams, seed, kind="rot"):
    """Q diag(lams) Q^T rounded to float32; Q from the QR of a seeded normal matrix ("rot"), the identity ("diag") or a permutation."""
    rng = np.random.default_rng(seed)
    if kind == "rot":
        Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    elif kind == "perm":
        Q = np.eye(6)[rng.permutation(6)]
    else:
        Q = np.eye(6)
    A = Q @ np.diag(np.asarray(lams, f64)) @ Q.T
    return ((A + A.T) * 0.5).astype(f32)


def rhs_steps(A, seed, scales=(1e-2, 1e-3, 1e-6)):
    """AtB of three steps: A x_s with |x_s| ~ scales — two steps that move the pose, one below the convergence bounds."""
    rng = np.random.default_rng(seed + 77)
    return [(A.astype(f64) @ (rng.normal(size=6) * s)).astype(f32) for s in scales]


@functools.lru_cache(maxsize=None)
def crafted(thr):
    """[(name, AtA float32 6x6, [AtB of step 0, 1, 2], [count of step 0, 1, 2], degenerate_in)] for eig_thresh = thr"""
    out = []

    def add(name, A, seed, counts=(60, 60, 60), deg_in=0):
        out.append((name, A, rhs_steps(A, seed), list(counts), deg_in))

    seed = 1000
    for s in (1.0, 100.0, 1e4):
        rest = [500.0, 1e3 * s, 2e3 * s, 2e4 * s, 5e4 * s]
        for d in DELTAS:
            for kind in ("rot", "rot", "diag", "perm"):
                seed += 1
                add(f"s{s:g} d{d:+g} {kind}", sym_matrix([thr * (1 + d)] + rest, seed, kind), seed)
        # the Cholesky shortcut's hand-over: lambda_min = thr + 2e-5 * trace * f, trace including lambda_min itself
        for f in (1 + 1e-3, 1 - 1e-3, 1 + 1e-6, 1 - 1e-6):
            lm = (thr + 2e-5 * f * sum(rest)) / (1 - 2e-5 * f)
            for kind in ("rot", "rot", "diag", "perm"):
                seed += 1
                add(f"s{s:g} hand-over {f - 1:+g} {kind}", sym_matrix([lm] + rest, seed, kind), seed)
        # two and three eigenvalues below the threshold, repeated ones among them
        for low in ([0.3 * thr, 0.6 * thr], [0.4 * thr, 0.4 * thr], [0.2 * thr, 0.5 * thr, 0.8 * thr], [0.7 * thr] * 3,
                    [0.99 * thr, 0.995 * thr]):
            for kind in ("rot", "rot", "perm"):
                seed += 1
                add(f"s{s:g} low {low} {kind}", sym_matrix(low + rest[len(low) - 1:], seed, kind), seed)
    # rank 3 (three exact zeros on the diagonal, in every arrangement of a few permutations) and the zero matrix: singular solve, X = 0
    for k in range(4):
        seed += 1
        add(f"rank3 perm {k}", sym_matrix([0.0, 0.0, 0.0, 1e3, 2e4, 5e4], seed, "perm"), seed)
    Z = np.zeros((6, 6), f32)
    out.append(("zero", Z, [np.full(6, v, f32) for v in (1.0, -2.0, 0.5)], [60, 60, 60], 0))
    # counts against min_corr = 50; a carried-in isDegenerate with the first step a no-op
    A = sym_matrix([thr * 2, 500.0, 1e3, 2e3, 2e4, 5e4], 4242, "rot")
    for counts in ((49, 49, 49), (50, 50, 50), (51, 51, 51), (49, 50, 51)):
        add(f"counts {counts}", A, 4242, counts)
    for deg_in in (0, 1):
        add(f"carried {deg_in}", A, 4243, (49, 51, 51), deg_in)
        add(f"carried {deg_in} never", A, 4244, (10, 20, 49), deg_in)
    return out


def chain_params(oc, thr=100.0, emulate=1, **kw):
    p = oc.default_params(1)
    p.eig_thresh, p.emulate_matp_shadow = thr, emulate
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def oracle_chain(oc, p, steps, T_init, deg_in=0, guard_ok=True, imu=None):
    """orc_align's loop (odomEstimationNode.cpp:606-626) around orc_lm_step on given (AtA, AtB, n_sel) per step: one record per step
    (what the registration looks like after it) and the result record after orc_transform_update."""
    bound = p.fixed_iters if p.fixed_iters > 0 else p.max_iters
    T = np.array(T_init, f32); P = np.zeros(36, f32)
    st = dict(deg=int(deg_in), dR=f32(100), dT=f32(100), n_corr=0, any=0, done=0 if guard_ok else 1, iters=0)
    it, recs = 0, []
    for A, b, n_sel in steps:
        rec = dict(ran=not st["done"], solved=0, X=np.zeros(6, f32))
        if not st["done"]:
            st["n_corr"] = int(n_sel)
            r = oc.lm_step(A, b, n_sel, it, p, T, P, st["deg"])
            fin = False
            if r["solved"]:
                T, P = r["T"], r["P"]
                st.update(deg=r["degenerate"], dR=r["deltaR"], dT=r["deltaT"], any=1)
                rec.update(solved=1, X=r["X"])
                if r["conv"] and p.fixed_iters <= 0:
                    st["iters"] = it; fin = True                    # break: iterCount is not incremented
            it += 1
            if not fin and it >= bound:
                st["iters"] = bound; fin = True
            st["done"] = 1 if fin else 0
        rec.update(T=T.copy(), P=P.copy(), **st)
        recs.append(rec)
    Tf = T.copy()
    if guard_ok:
        oc.lib().orc_transform_update(C.byref(p), C.byref(imu) if imu is not None else None, Tf.ctypes.data_as(C.POINTER(C.c_float)))
    status = 1 if not guard_ok else (0 if st["any"] else 2)
    return recs, dict(T=Tf, status=status, **st)


T_START = np.array([0.02, -0.03, 0.4, 1.0, -2.0, 0.5], f32)


@functools.lru_cache(maxsize=None)
def crafted_reference(thr, emulate):
    """the oracle's chain over crafted(thr), computed once and shared by the CPU and GPU tests"""
    import oracle_ctypes as oc
    oc.build()
    p = chain_params(oc, thr, emulate)
    return [oracle_chain(oc, p, list(zip([A] * 3, bs, counts)), T_START, deg_in) for _, A, bs, counts, deg_in in crafted(thr)]


def float64_spectrum(A, thr):
    """(eigenvalues ascending, eigenvectors, clear): clear = every eigenvalue at least 2e-6 * lambda_max away from the threshold"""
    w, v = np.linalg.eigh(A.astype(f64))
    lmax = max(abs(w).max(), 1e-300)
    return w, v, bool((np.abs(w - thr) >= 2e-6 * lmax).all())


# ---- CPU: the yardstick ------------------------------------------------------------------------------------------------------------
def corridor(name):
    from lisreg import synth
    return {"oblique": lambda: synth.make_corridor_case(n_src=1200),
            "oblique tilted": lambda: synth.make_corridor_case(n_src=1200, tilt=(0.25, -0.2)),
            "no floor": lambda: synth.make_corridor_case(angle=1.1, floor=False),
            "short": lambda: synth.make_corridor_case(length=6.0, n_src=600),
            "hugging 95": lambda: synth.make_corridor_case(n_src=1600, tilt=(0.25, -0.2)),
            "hugging 99": lambda: synth.make_corridor_case(n_src=1650, tilt=(0.25, -0.2)),
            "hugging 102": lambda: synth.make_corridor_case(n_src=1650)}[name]()


@pytest.mark.parametrize("scene,emulate", [("level", 1), ("oblique", 1), ("oblique", 0), ("no floor", 0)])
def test_chained_step_reproduces_orc_align(oracle, scene, emulate):
    from lisreg import synth
    case = synth.make_case(h=16, w=450, m_points=20000, scan_seed=1000) if scene == "level" else corridor(scene)
    p = oracle.default_params(1); p.emulate_matp_shadow = emulate
    T, st, tr = oracle.align(case["tgt_corner"], case["tgt_surf"], case["src_corner"], case["src_surf"], case["T_init"], p)
    steps = [(r[1:37], r[37:43], int(r[0])) for r in tr]
    recs, res = oracle_chain(oracle, p, steps, case["T_init"])
    assert len(recs) == len(tr) >= 2
    for k, r in enumerate(recs):
        assert r["ran"] and r["solved"] == tr[k, 55] == 1
        assert same_bits(r["X"], tr[k, 43:49]) and same_bits(r["T"], tr[k, 49:55]), k
    assert recs[-1]["done"] == 1 and not any(r["done"] for r in recs[:-1])
    assert (res["iters"], res["deg"], res["n_corr"], res["status"]) == (st["iters"], st["degenerate"], st["n_corr_last"], st["status"])
    assert same_bits(res["T"], T) and same_bits([res["dR"], res["dT"]], [st["deltaR"], st["deltaT"]])
    if scene != "level":
        assert st["degenerate"] == 1 and (st["iters"] == 1) == bool(emulate)


@pytest.mark.parametrize("thr", [100.0, 10.0])
def test_oracle_degenerate_flag_is_the_float64_one(thr):
    ref = crafted_reference(thr, 1)
    n_clear = n_deg = 0
    for (name, A, _, counts, _), (recs, _) in zip(crafted(thr), ref):
        if counts[0] < 50:
            continue
        w, _, clear = float64_spectrum(A, thr)
        if clear:
            n_clear += 1; n_deg += int(w[0] < thr)
            assert recs[0]["deg"] == int(w[0] < thr), (name, w)
    assert n_clear >= 60 and 20 <= n_deg <= n_clear - 20, (n_clear, n_deg)      # both verdicts are well populated


@pytest.mark.parametrize("thr", [100.0, 10.0])
def test_oracle_projector_is_the_float64_one(thr):
    """EVERY matrix the oracle flags degenerate: k = the number of eigenvector rows it zeroed, read off its own matP (a projector of rank
    6 - k: k = 6 - trace); compared with the float64 projector onto the top 6 - k eigenvectors, gap = the distance between the last
    kept and the first zeroed eigenvalue.  Which side of the threshold a hugging eigenvalue fell is the flag test's business, not this one's."""
    ref = crafted_reference(thr, 0)
    worst_k, n, n_hug = 0.0, 0, 0
    for (name, A, _, counts, _), (recs, _) in zip(crafted(thr), ref):
        if counts[0] < 50 or not recs[0]["deg"]:
            continue
        w, v, clear = float64_spectrum(A, thr)                      # ascending
        P = recs[0]["P"].reshape(6, 6).astype(f64)
        k = 6 - int(round(np.trace(P)))
        assert 1 <= k <= 6 and abs(np.trace(P) - (6 - k)) < 1e-3, (name, np.trace(P))
        if k == 6:
            assert not P.any(), name
            continue
        Pf = v[:, k:] @ v[:, k:].T
        err = np.abs(P - Pf).max()
        gap = w[k] - w[k - 1]
        kk = err * gap / (2.0 ** -24 * abs(w).max())
        worst_k = max(worst_k, kk); n += 1; n_hug += int(not clear)
        assert kk <= K_BAR, (name, kk, err, gap)
    print(f"eig_thresh {thr:g}: matP against the float64 projector on {n} degenerate matrices ({n_hug} with an eigenvalue within 2e-6 lambda_max "
          f"of the threshold), worst K = {worst_k:.2f} (bar {K_BAR:g})")
    assert n >= 100 and n_hug >= 60


def test_singular_normal_equations_give_a_zero_step():
    for (name, A, _, _, _), (recs, res) in zip(crafted(100.0), crafted_reference(100.0, 1)):
        if name.startswith("rank3") or name == "zero":
            assert recs[0]["solved"] and recs[0]["deg"] == 1 and not recs[0]["X"].any() and same_bits(recs[0]["T"], T_START), name
            assert recs[0]["done"] == 1 and res["iters"] == 0


# ---- GPU: the device against the chain, bit for bit ---------------------------------------------------------------------------------
def pack_rows(step_lists, n_rows):
    """rows[n_steps, sum(n_rows), 28]: item i's (AtA, AtB, count) of a step goes into row i % n_rows[i] of its block, the others stay 0"""
    n_steps = len(step_lists[0])
    begin = np.concatenate([[0], np.cumsum(n_rows)])
    rows = np.zeros((n_steps, int(begin[-1]), 28), f64)
    iu = np.triu_indices(6)
    for i, steps in enumerate(step_lists):
        r = int(begin[i]) + i % int(n_rows[i])
        for s, (A, b, cnt) in enumerate(steps):
            rows[s, r, :21] = np.asarray(A, f32).reshape(6, 6)[iu]
            rows[s, r, 21:27] = b
            rows[s, r, 27] = cnt
    return rows


def within_one_ulp(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return bool((np.abs(a.astype(f64) - b.astype(f64)) <= np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(f64)).all())


def slerps(p, imu, guard_ok=True):
    """does transformUpdate run the IMU slerp (double sin / acos / asin / atan2) on this item? (odomEstimationNode.cpp:979-981)"""
    return bool(guard_ok and p.use_imu_blend and imu is not None and imu.imu_available and abs(f32(imu.imu_pitch_init)) < f32(1.4))


def compare_with_chain(dev, ref, names, slerp=None):
    """device output of lisreg_test_solve_steps against oracle_chain's records, item by item and step by step"""
    n_p = 0
    for i, (recs, res) in enumerate(ref):
        tag = names[i]
        for s, r in enumerate(recs):
            tr, stt = dev["trace"][i, s], dev["state"][i, s]
            if not r["ran"]:
                assert not tr.any(), (tag, s)
            else:
                assert tr[0] == r["n_corr"] and tr[55] == r["solved"], (tag, s, tr[0], tr[55])
                assert same_bits(tr[43:49], r["X"]), (tag, s, tr[43:49], r["X"])
                assert same_bits(tr[49:55], r["T"]), (tag, s, tr[49:55], r["T"])
            assert (stt[48], stt[51], stt[52], stt[53], stt[54]) == (r["deg"], r["n_corr"], r["done"], r["iters"], r["any"]), (tag, s, stt[48:56], r)
            assert same_bits(stt[49:51], [r["dR"], r["dT"]]), (tag, s)
            if r["deg"]:
                assert same_bits(stt[:36], r["P"]), (tag, s, stt[:36].reshape(6, 6), r["P"].reshape(6, 6))
                n_p += 1
        out = dev["results"][i]
        assert same_bits(out[2:6], res["T"][2:6]), (tag, out, res)
        # roll and pitch: one float ulp where the slerp ran (the device's double libm is not correctly rounded), else clamped or passed through: equal
        assert within_one_ulp(out[:2], res["T"][:2]) if (slerp is not None and slerp[i]) else same_bits(out[:2], res["T"][:2]), (tag, out[:2], res["T"][:2])
        assert (out[6], out[9], out[10], out[11]) == (res["iters"], res["deg"], res["n_corr"], res["status"]), (tag, out, res)
        assert same_bits(out[7:9], [res["dR"], res["dT"]]), tag
    return n_p


@pytest.mark.gpu
@pytest.mark.parametrize("thr,emulate", [(100.0, 1), (100.0, 0), (10.0, 1), (10.0, 0)])
def test_device_step_equals_oracle_on_crafted_matrices(gpu_ctx, oracle, thr, emulate):
    import lisreg
    cases = crafted(thr)
    ref = crafted_reference(thr, emulate)
    p = copy_params(chain_params(oracle, thr, emulate), lisreg.Params)
    n_rows = np.array([1 + i % 3 for i in range(len(cases))], np.int32)
    rows = pack_rows([list(zip([A] * 3, bs, counts)) for _, A, bs, counts, _ in cases], n_rows)
    dev = gpu_ctx.test_solve_steps(n_rows, rows, np.tile(T_START, (len(cases), 1)), p, degenerate_in=[c[4] for c in cases])
    n_p = compare_with_chain(dev, ref, [c[0] for c in cases])
    # what the two settings pin: with the quirk every degenerate item stands still at step 1 and finishes there; without it matP persists
    n_deg = 0
    for (name, _, _, counts, deg_in), (recs, res) in zip(cases, ref):
        if min(counts) >= 50 and recs[0]["deg"] and recs[0]["X"].any():
            n_deg += 1
            if emulate:
                assert not recs[1]["X"].any() and res["iters"] == 1, name
            else:
                assert recs[1]["X"].any() and same_bits(recs[1]["P"], recs[0]["P"]) and res["iters"] >= 2, name
    assert n_deg >= 40 and n_p >= 100
    # a carried-in isDegenerate whose first solve is step 1: the zero matP projects the step away, under either setting
    for (name, _, _, _, _), (recs, res) in zip(cases, ref):
        if name == "carried 1":
            assert not recs[0]["solved"] and recs[1]["solved"] and recs[1]["deg"] == 1 and not recs[1]["X"].any() and res["iters"] == 1


@pytest.mark.gpu
def test_device_step_loop_control(gpu_ctx, oracle):
    """fixed_iters > 0 (no early finish), the bound reached before the steps run out, an item that fails the feature-count guard"""
    import lisreg
    cases = [c for c in crafted(100.0) if c[0].startswith(("s1 d", "counts", "carried", "zero"))]
    names = [c[0] for c in cases]
    steps = [list(zip([A] * 3, bs, counts)) for _, A, bs, counts, _ in cases]
    n_rows = np.array([1 + (i + 1) % 2 for i in range(len(cases))], np.int32)
    rows = pack_rows(steps, n_rows)
    T0 = np.tile(T_START, (len(cases), 1))
    for kw in (dict(fixed_iters=3), dict(max_iters=2), dict(fixed_iters=2), dict(max_iters=3, emulate=0)):
        po = chain_params(oracle, 100.0, kw.pop("emulate", 1), **kw)
        bound = po.fixed_iters if po.fixed_iters > 0 else po.max_iters
        ref = [oracle_chain(oracle, po, st, T_START, c[4]) for st, c in zip(steps, cases)]
        dev = gpu_ctx.test_solve_steps(n_rows, rows, T0, copy_params(po, lisreg.Params), degenerate_in=[c[4] for c in cases])
        compare_with_chain(dev, ref, names)
        if po.fixed_iters > 0:
            assert all(res["iters"] == bound and recs[bound - 1]["done"] and not recs[bound - 2]["done"] for recs, res in ref)
        assert (dev["results"][:, 6] <= bound).all() and (dev["results"][:, 6] == bound).any()
        if bound == 2:
            assert not dev["trace"][:, 2].any()                      # nothing runs past the bound
    # the guard (n_sc > edge_min && n_ss > surf_min): status 1, T untouched, never solved, whatever the rows hold
    po = chain_params(oracle, 100.0, 1)
    n_ss = np.array([100 if i % 2 else 101 for i in range(len(cases))], np.int32)
    imu = [lisreg.Imu(1, 0.3, -0.2)] * len(cases)
    ref = [oracle_chain(oracle, po, st, T_START, c[4], guard_ok=bool(n_ss[i] > 100), imu=oracle.Imu(1, 0.3, -0.2))
           for i, (st, c) in enumerate(zip(steps, cases))]
    dev = gpu_ctx.test_solve_steps(n_rows, rows, T0, copy_params(po, lisreg.Params), degenerate_in=[c[4] for c in cases],
                                   n_sc=np.zeros(len(cases), np.int32), n_ss=n_ss, imu=imu)
    compare_with_chain(dev, ref, names, slerp=[slerps(po, oracle.Imu(1, 0.3, -0.2), bool(n_ss[i] > 100)) for i in range(len(cases))])
    failed = n_ss <= 100
    assert (dev["results"][failed, 11] == 1).all() and (dev["results"][~failed, 11] != 1).all()
    assert same_bits(dev["results"][failed, :6], T0[failed]) and not dev["trace"][failed].any() and not dev["state"][failed, :, 54].any()


ROW_COUNTS = [1, 15, 16, 17, 31, 32, 33, 511, 512, 513, 1023, 1024, 1025, 1537]


@pytest.mark.gpu
def test_partial_row_sum_covers_every_row(gpu_ctx):
    """kSolveThreads = 512 is 16 row groups with 32 rows in flight per thread: one pass takes 512 rows.  Small integers per (row, column)
    make the exact sum order-independent: AtA, AtB and the count of the trace must be those integers."""
    import lisreg
    n_rows = np.array(ROW_COUNTS + ROW_COUNTS[::-1] + [513, 1, 1025, 16], np.int32)
    total = int(n_rows.sum())
    g = np.arange(total)[:, None]; col = np.arange(28)[None, :]
    rows = ((g * 7 + col * 13 + (g // 5) * col) % 97 - 48).astype(f64)
    rows[:, 27] = 1 + np.arange(total) % 3
    p = lisreg.default_params(1); p.min_corr = 1
    dev = gpu_ctx.test_solve_steps(n_rows, rows[None], np.zeros((len(n_rows), 6), f32), p)
    begin = np.concatenate([[0], np.cumsum(n_rows)])
    iu = np.triu_indices(6)
    for i in range(len(n_rows)):
        exact = rows[begin[i]:begin[i + 1]].astype(np.int64).sum(0)
        tr = dev["trace"][i, 0]
        U = np.zeros((6, 6), np.int64); U[iu] = exact[:21]; S = U + np.triu(U, 1).T
        assert tr[0] == exact[27] and tr[55] == 1, (i, n_rows[i], tr[0], exact[27])
        assert np.array_equal(tr[1:37], S.astype(f32).ravel()), (i, n_rows[i], tr[1:37].reshape(6, 6), S)
        assert np.array_equal(tr[37:43], exact[21:27].astype(f32)), (i, n_rows[i])
        assert dev["state"][i, 0, 51] == exact[27]


FIN_ROT_TOL, FIN_Z_TOL = f32(0.01), f32(2.5)


def finalize_cases():
    """[(name, T before transformUpdate, imu (available, roll, pitch) or None, parameter overrides)]"""
    out = []
    tol = dict(rotation_tol=float(FIN_ROT_TOL), z_tol=float(FIN_Z_TOL))
    for r in (0.5, -0.5, FIN_ROT_TOL, -FIN_ROT_TOL, 0.005):
        for z in (3.0, -3.0, FIN_Z_TOL, -FIN_Z_TOL, 1.0):
            out.append((f"clamp {r} {z}", [r, -r, 0.4, 1.0, 2.0, z], None, tol))
            out.append((f"clamp imu {r} {z}", [r, -r, 0.4, 1.0, 2.0, z], (1, 0.02, -0.015), tol))
    for tr, ir in ((3.0, -3.0), (-3.0, 3.0), (3.1, -3.1), (2.0, -2.0), (1.0, -3.0)):           # d < 0: the shortest path crosses +-pi
        out.append((f"across pi {tr} {ir}", [tr, 0.1, 0.4, 1, 2, 3], (1, ir, 0.2), {}))
        out.append((f"pitch across pi {tr} {ir}", [0.1, tr, 0.4, 1, 2, 3], (1, 0.2, np.sign(ir) * 1.3), {}))
    for v in (0.0, 0.25, -1.0, 3.0):                                                         # theta == 0 (exactly so at 0)
        out.append((f"equal {v}", [v, min(v, 1.3), 0.4, 1, 2, 3], (1, v, min(v, 1.3)), {}))
    for ip in (1.39, 1.4, 1.41, -1.39, -1.4, -1.41):                                         # |imu_pitch_init| < 1.4f
        out.append((f"imu pitch {ip}", [0.3, 0.2, 0.4, 1, 2, 3], (1, -0.2, ip), {}))
    # These only APPROACH the gimbal branch of getRPY (|m20| >= 1); they do not cover it.  The float nearest pi/2 is 4.4e-8 away, so sin(pitch)
    # is 1 - 9.5e-16 in double and |m20| stays below 1; the |imu_pitch_init| < 1.4 gate keeps a slerp from landing on pi/2 otherwise.  The
    # branch cannot be reached through float poses and stays unexercised on the device.
    for tp in (1.5707964, -1.5707964):
        for w in (0.0, 1e-8, 0.1, 1.0):
            out.append((f"near gimbal {tp} w {w}", [0.3, tp, 0.4, 1, 2, 3], (1, 0.1, 0.5), dict(imu_rpy_weight=w)))
    out.append(("no blend", [0.3, 0.2, 0.4, 1, 2, 3], (1, -0.2, 0.5), dict(use_imu_blend=0)))
    out.append(("imu not available", [0.3, 0.2, 0.4, 1, 2, 3], (0, -0.2, 0.5), {}))
    out.append(("weights", [0.3, 0.2, 0.4, 1, 2, 3], (1, -0.2, 0.5), dict(imu_rpy_weight=0.5)))
    return out


@pytest.mark.gpu
def test_finalize_equals_transform_update(gpu_ctx, oracle):
    """k_finalize (IMU slerp, clamps) against orc_transform_update: every case once after a solved step with X = 0 (status 0) and once
    never solved (status 2: transformUpdate still runs, as in the reference, :622)."""
    import lisreg
    cases = finalize_cases()
    groups = {}
    for c in cases:
        groups.setdefault(tuple(sorted(c[3].items())), []).append(c)
    Z = np.zeros((6, 6), f32); b = np.ones(6, f32)
    n_moved = 0
    for key, grp in groups.items():
        po = chain_params(oracle, 100.0, 1, **dict(key))
        items = [(c, cnt) for c in grp for cnt in (60, 10)]
        steps = [[(Z, b, cnt)] for _, cnt in items]
        T0 = np.array([c[1] for c, _ in items], f32)
        imus_o = [oracle.Imu(*c[2]) if c[2] else None for c, _ in items]
        ref = [oracle_chain(oracle, po, st, T0[i], imu=imus_o[i]) for i, st in enumerate(steps)]
        n_rows = np.ones(len(items), np.int32)
        dev = gpu_ctx.test_solve_steps(n_rows, pack_rows(steps, n_rows), T0, copy_params(po, lisreg.Params),
                                       imu=[lisreg.Imu(*c[2]) if c[2] else None for c, _ in items])
        compare_with_chain(dev, ref, [f"{c[0]} count {cnt}" for c, cnt in items], slerp=[slerps(po, m) for m in imus_o])
        for i, (c, cnt) in enumerate(items):
            assert dev["results"][i, 11] == (0 if cnt >= 50 else 2)
            n_moved += int(not same_bits(dev["results"][i, :6], T0[i]))
    assert n_moved >= len(cases)                   # the cases do act: most poses leave transformUpdate changed
    # the clamps as such (oracle and device agree above; this pins the values)
    po = chain_params(oracle, 100.0, 1, rotation_tol=float(FIN_ROT_TOL), z_tol=float(FIN_Z_TOL))
    _, res = oracle_chain(oracle, po, [(Z, b, 60)], np.array([0.5, -0.5, 0.4, 1, 2, -3], f32))
    assert same_bits(res["T"], [FIN_ROT_TOL, -FIN_ROT_TOL, f32(0.4), 1, 2, -FIN_Z_TOL])


@pytest.mark.gpu
def test_pose_cache_at_non_level_poses(gpu_ctx):
    """The 3 x 4 matrix k_solve leaves for the next correspondence launch (write_pose_cache from the device's sinf / cosf) against the
    float64 matrix of the same float32 pose.  Rotation entries: at most three trigonometric factors of <= 2 ulp each plus the roundings of
    two products and a sum, all of magnitude <= 1: 16 * 2^-24.  Translation: the pose's own floats."""
    import lisreg
    from lisreg import synth
    ang = [s * a for a in (0.3, 0.8, 1.2) for s in (1, -1)]
    poses = np.array([[r, p, y, 1.5, -2.5, 0.75] for r in ang for p in ang for y in (3.1, -3.1, 1.6, -1.6, 0.4)], f32)
    n = len(poses)
    steps = [[(np.zeros((6, 6), f32), np.ones(6, f32), 60)]] * n          # singular: X = 0, the pose stays, the cache is rewritten
    n_rows = np.ones(n, np.int32)
    dev = gpu_ctx.test_solve_steps(n_rows, pack_rows(steps, n_rows), poses, lisreg.default_params(1))
    assert (dev["trace"][:, 0, 55] == 1).all() and same_bits(dev["trace"][:, 0, 49:55], poses)
    worst = 0.0
    for i in range(n):
        M = dev["state"][i, 0, 36:48].reshape(3, 4)
        want = synth.pose_matrix(poses[i].astype(f64))
        worst = max(worst, np.abs(M[:, :3].astype(f64) - want[:3, :3]).max())
        assert same_bits(M[:, 3], poses[i, 3:6])
    print(f"pose cache at {n} non-level poses: worst rotation entry error {worst / 2.0 ** -24:.2f} x 2^-24 (bar 16)")
    assert worst <= 16 * 2.0 ** -24


# ---- GPU: whole registrations on the scenes the suite lacked -------------------------------------------------------------------------
def oracle_iter0_eigenvalues(tro):
    return np.linalg.eigvalsh(tro[0, 1:37].reshape(6, 6).astype(f64))


@pytest.mark.gpu
@pytest.mark.parametrize("emulate", [1, 0])
@pytest.mark.parametrize("scene", ["oblique", "oblique tilted", "no floor", "short"])
def test_corridor_production_matches_oracle(oracle, scene, emulate):
    import lisreg
    case = corridor(scene)
    p_o = oracle.default_params(1); p_o.emulate_matp_shadow = emulate
    To, so, tro = oracle.align(case["tgt_corner"], case["tgt_surf"], case["src_corner"], case["src_surf"], case["T_init"], p_o)
    ev = oracle_iter0_eigenvalues(tro)
    print(f"corridor '{scene}', emulate {emulate}: oracle eigenvalues {np.round(ev, 1)}, degenerate {so['degenerate']}, iters {so['iters']}")
    # the production AtA differs from the oracle's in the fourth digit: only scenes whose eigenvalues keep clear of the threshold
    assert not ((ev >= 0.8 * p_o.eig_thresh) & (ev <= 1.25 * p_o.eig_thresh)).any(), ev
    assert so["degenerate"] == 1
    c = lisreg.Context(0)
    c.set_target(case["tgt_corner"], case["tgt_surf"])
    Tg, sg, trg = c.align(case["src_corner"], case["src_surf"], case["T_init"], copy_params(p_o, lisreg.Params))
    c.close()
    assert (sg["status"], sg["degenerate"], sg["iters"]) == (so["status"], so["degenerate"], so["iters"]), (sg, so)
    assert max(pose_err(Tg, To)) <= 1e-3, pose_err(Tg, To)
    # the slide along the corridor is what stays unobserved: the other five directions come home
    along = np.array([np.cos(0.6 if scene != "no floor" else 1.1), np.sin(0.6 if scene != "no floor" else 1.1)])
    if not emulate:
        d = (To - case["T_true"]).astype(f64)
        across = d[3:5] - (d[3:5] @ along) * along
        assert np.abs(d[:3]).max() < 5e-3 and np.abs(across).max() < 1e-2, d


@pytest.mark.gpu
@pytest.mark.parametrize("emulate", [1, 0])
@pytest.mark.parametrize("scene", ["oblique", "oblique tilted", "no floor", "short", "hugging 95", "hugging 99", "hugging 102"])
def test_corridor_exact_build_equals_oracle(oracle, scene, emulate):
    import lisreg
    from test_exact import check_exact
    case = corridor(scene)
    p_o = oracle.default_params(1); p_o.emulate_matp_shadow = emulate
    worst, n = check_exact(oracle, lisreg, case, p_o, None)
    print(f"[exact] corridor '{scene}', emulate {emulate}: worst pose difference over all iterations {worst:.2e}, {n} accept flags equal")
    assert worst == 0.0                      # bit for bit


def tilted_case(k):
    from lisreg import synth
    tilt, seed = [((0.3, -0.25), 3000), ((-0.4, 0.35), 3001)][k]
    Tt = synth.draw_pose(np.random.default_rng(seed)); Tt[0], Tt[1] = tilt
    sc = synth.make_scan(16, 450, seed, T_true=Tt)
    tc, ts = synth.make_submap(20000)
    T0 = synth.perturb_pose(sc["T_true"], np.random.default_rng(seed + 7919))
    return dict(tgt_corner=tc, tgt_surf=ts, src_corner=sc["corner"], src_surf=sc["surf"], T_init=T0, T_true=Tt.astype(f32))


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1])
def test_tilted_scene_matches_oracle(oracle, k):
    """A sensor rolled and pitched by 0.25 .. 0.4 rad: the D F terms of the pose matrix and the second-order Jacobian factors carry weight.
    Production arithmetic within the bars of test_gpu_parity.test_pose_and_trace_match_oracle; the exact build bit for bit."""
    import lisreg
    from test_exact import check_exact
    case = tilted_case(k)
    p_o = oracle.default_params(1)
    To, so, tro = oracle.align(case["tgt_corner"], case["tgt_surf"], case["src_corner"], case["src_surf"], case["T_init"], p_o)
    assert so["status"] == 0 and so["iters"] < p_o.max_iters and so["n_corr_last"] > 3000
    c = lisreg.Context(0)
    c.set_target(case["tgt_corner"], case["tgt_surf"])
    Tg, sg, trg = c.align(case["src_corner"], case["src_surf"], case["T_init"], copy_params(p_o, lisreg.Params))
    c.close()
    assert sg["status"] == 0 and sg["iters"] == so["iters"] and sg["degenerate"] == so["degenerate"]
    assert max(pose_err(Tg, To)) <= 1e-3 and len(trg) == len(tro)
    for i in range(len(tro)):
        assert abs(trg[i, 0] - tro[i, 0]) <= max(3, 0.002 * tro[i, 0])
        assert max(pose_err(trg[i, 49:55], tro[i, 49:55])) <= 1e-3
        assert np.abs(trg[i, 1:37] - tro[i, 1:37]).max() <= 2e-3 * np.abs(tro[i, 1:37]).max()
    worst, n = check_exact(oracle, lisreg, case, p_o, None)
    assert worst == 0.0
