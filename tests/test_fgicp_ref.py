"""tests/fgicp_ref.py, the definition of lisreg_fgicp_*, against itself and against independent computations — no GPU:
the loop forms against the vector forms, the correspondences against scipy's kd-tree, b and H against central differences of the error
with the pairs and M held fixed, H against a per-pair reassembly, the reuse of a linearisation's pairs by an error evaluation on a case
built by hand, the scene's alignments and their decision margins, the structs and symbols of include/lisreg.h, the golden file."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fgicp_ref as R
from test_ndt import _header_struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "fgicp", "fgicp_cases.npz")
SYMBOLS = ("lisreg_fgicp_default_params", "lisreg_fgicp_set_target", "lisreg_fgicp_align", "lisreg_fgicp_correspondences",
           "lisreg_fgicp_linearize")


@pytest.fixture(scope="module")
def now():
    """the golden cases made afresh: once, for the tests that read them"""
    return R.golden_cases()


def test_loop_form_equals_vector_form():
    prm = R.params()
    # the searches: a planted target (identical points, NaN points) with queries on, between and far from its points, both kinds
    xyz, groups = R.planted_cloud(n_base=120)
    Tt = R.build_target(xyz, prm)
    rng = np.random.default_rng(4)
    q = np.concatenate([xyz[groups["identical"][:2]].astype(np.float64), rng.uniform(-8.0, 40.0, (60, 3)), [[np.nan, 0.0, 0.0]],
                        xyz[groups["base"][:5]].astype(np.float64) + 5.0e-4])
    for kind in (0, 1):
        a, b = R.search_loops(Tt, q, R.params(kind)["max_correspondence_distance"]), R.search(Tt, q, R.params(kind)["max_correspondence_distance"])
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True), kind          # ties included: the lower index
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), kind
        assert a[0][0] == a[0][1] == groups["identical"].min() and a[0][62] == -1 and not np.isin(a[0], groups["nan"]).any()
        assert (a[0][np.isfinite(q).all(1)] >= 0).all() if kind == 1 else (a[0] == -1).sum() > 10
    # one linearisation: 1 500 target points of the scene, 40 source points, with the whole clouds' distributions
    W = R.world()
    Tc = dict(W["T"])
    Tc["idx"] = Tc["idx"][:1500]
    S = dict(x=W["S"]["x"][:40], C=W["S"]["C"][:40], ok=W["S"]["ok"][:40])
    poses = R.lin_poses(W["guess"], W["T_true"])
    for T in poses:
        for hess in (True, False):
            u, v = R.linearize(Tc, S, T, prm, hess, loops=True), R.linearize(Tc, S, T, prm, hess)
            assert u["n_pairs"] == v["n_pairs"] and np.array_equal(u["pairs"]["idx"], v["pairs"]["idx"])
            assert np.allclose(u["pairs"]["M"], v["pairs"]["M"], rtol=1e-12, atol=0)
            assert np.all(np.abs(u["out"] - v["out"]) <= 1e-12 * np.maximum(u["abs"], 1e-300)) and np.allclose(u["abs"], v["abs"], rtol=1e-12, atol=0)
    assert v["n_pairs"] == 0 and not v["out"].any()                           # the pose 100 m away
    u, v = (R.linearize(Tc, S, poses[0], prm, True, T_eval=poses[1], loops=lp) for lp in (True, False))
    assert np.all(np.abs(u["out"] - v["out"]) <= 1e-12 * u["abs"]) and u["n_pairs"] == v["n_pairs"] > 0


def test_correspondences_equal_the_kd_trees_on_the_scene():
    from scipy.spatial import cKDTree
    W = R.world()
    tree = cKDTree(W["T"]["x"][W["T"]["idx"]])
    for T in (W["guess"].astype(np.float64), W["T_true"]):
        p = R.find_pairs(W["T"], W["S"], T, R.params())
        d, j = tree.query(R.transform_points(T, W["S"]["x"]), k=1)
        sure = p["row_nn"] >= 1e-9
        assert sure.sum() >= len(j) - 2 and np.array_equal(W["T"]["idx"][j][sure], p["idx"][sure])
        assert np.allclose(d * d, p["sq"], rtol=1e-12, atol=0) and (p["idx"] >= 0).all() and p["cut_gap"] >= 1e-9
    # the cut-off: with 0.05 m some points keep their pair and some lose it, exactly those beyond it
    p2 = R.find_pairs(W["T"], W["S"], T, R.params(max_correspondence_distance=0.05))
    assert 0 < (p2["idx"] >= 0).sum() < len(j) and np.array_equal(p2["idx"] >= 0, p["sq"] < 0.05 * 0.05)
    assert np.array_equal(p2["idx"][p2["idx"] >= 0], p["idx"][p2["idx"] >= 0])


def test_b_and_h_against_central_differences_of_the_error():
    W = R.world()
    T0 = W["guess"].astype(np.float64)
    full = R.find_pairs(W["T"], W["S"], T0, R.params())
    pairs = dict(pi=full["pi"][::5], ti=full["ti"][::5], M=full["M"][::5])
    ev = R.sums(W["T"], W["S"], pairs, T0, True, per_pair=True)
    e0, b, H = R.unpack(ev["out"])

    def err(delta, tgt=W["T"]):
        return R.sums(tgt, W["S"], pairs, R.se3_exp(delta) @ T0, False)["out"][0]
    # e over the fixed pair set with M held: its gradient at delta = 0 is 2 b
    h = 1e-5
    g = np.array([(err(h * np.eye(6)[k]) - err(-h * np.eye(6)[k])) / (2 * h) for k in range(6)])
    assert np.abs(g - 2 * b).max() <= 1e-6 * np.abs(ev["abs"][1:7]).max()
    # with every correspondent moved onto its transformed point the residuals vanish and the second differences of e are 2 H exactly
    moved = dict(W["T"])
    moved["x"] = W["T"]["x"].copy()
    assert len(np.unique(pairs["ti"])) > 100
    first = {}
    for p, t in zip(pairs["pi"], pairs["ti"]):
        first.setdefault(t, p)
    keep = np.array([first[t] == p for p, t in zip(pairs["pi"], pairs["ti"])])          # one source point per correspondent
    pairs = dict(pi=pairs["pi"][keep], ti=pairs["ti"][keep], M=pairs["M"][keep])
    moved["x"][pairs["ti"]] = R.transform_points(T0, W["S"]["x"][pairs["pi"]])
    _, _, H = R.unpack(R.sums(moved, W["S"], pairs, T0, True)["out"])
    assert err(np.zeros(6), moved) == 0.0
    h = 1e-3
    E = np.eye(6)
    H2 = np.array([[(err(h * (E[i] + E[j]), moved) - err(h * (E[i] - E[j]), moved) - err(h * (E[j] - E[i]), moved) + err(-h * (E[i] + E[j]), moved))
                    / (4 * h * h) for j in range(6)] for i in range(6)])
    assert np.abs(H2 - 2 * H).max() <= 1e-5 * np.abs(H).max()
    assert np.abs(H - H.T).max() == 0 and np.linalg.eigvalsh(H).min() > 0


def test_h_of_a_linearisation_equals_the_one_reassembled_per_pair():
    W = R.world()
    T0 = W["guess"].astype(np.float64)
    ev = R.linearize(W["T"], W["S"], T0, R.params(), True)
    _, b, H = R.unpack(ev["out"])
    Rm = T0[:3, :3]
    H2, b2 = np.zeros((6, 6)), np.zeros(6)
    for p, t in zip(ev["pairs"]["pi"], ev["pairs"]["ti"]):
        x = R.transform_points(T0, W["S"]["x"][p:p + 1])[0]
        J = np.hstack([R.skew(x), -np.eye(3)])
        M = np.linalg.inv(W["T"]["C"][t] + Rm @ W["S"]["C"][p] @ Rm.T)
        H2 += J.T @ M @ J
        b2 += J.T @ M @ (W["T"]["x"][t] - x)
    assert np.abs(H - H2).max() <= 1e-11 * np.abs(H).max() and np.abs(b - b2).max() <= 1e-11 * ev["abs"][1:7].max()


def test_an_error_evaluation_keeps_the_pairs_of_the_linearisation():
    """two target points, one source point, by hand: moved by T_eval the source point is nearer to the OTHER target point, and the error
    is still that of the old pair"""
    eye = np.eye(3)
    tgt = dict(x=np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), C=np.stack([eye, eye]), ok=np.array([True, True]), idx=np.array([0, 1]))
    src = dict(x=np.array([[0.4, 0.0, 0.0]]), C=np.stack([eye]), ok=np.array([True]))
    T_pairs, T_eval = np.eye(4), np.eye(4)
    T_eval[0, 3] = 1.2
    prm = R.params()
    lin = R.linearize(tgt, src, T_pairs, prm, True)
    assert list(lin["pairs"]["ti"]) == [0] and np.allclose(lin["pairs"]["M"][0], 0.5 * eye) and np.isclose(lin["out"][0], 0.5 * 0.4 ** 2)
    assert list(R.find_pairs(tgt, src, T_eval, prm)["ti"]) == [1]                       # a search at T_eval would change the pair
    held = R.sums(tgt, src, lin["pairs"], T_eval, False)
    fresh = R.linearize(tgt, src, T_eval, prm, False)
    assert np.isclose(held["out"][0], 0.5 * 1.6 ** 2) and np.isclose(fresh["out"][0], 0.5 * 0.4 ** 2) and held["n_pairs"] == fresh["n_pairs"] == 1
    both = R.linearize(tgt, src, T_pairs, prm, False, T_eval=T_eval)
    assert both["out"][0] == held["out"][0] and not both["out"][7:].any()
    # M is held too: a T_eval that rotates does not re-form it
    Rz = R.se3_exp(np.r_[0.0, 0.0, 0.5, 0.0, 0.0, 0.0])
    src2 = dict(src, C=np.stack([np.diag([1.0, 1e-3, 1.0])]))
    lin2 = R.linearize(tgt, src2, T_pairs, prm, True)
    assert np.array_equal(R.linearize(tgt, src2, T_pairs, prm, True, T_eval=Rz)["pairs"]["M"], lin2["pairs"]["M"])
    assert not np.allclose(R.find_pairs(tgt, src2, Rz, prm)["M"], lin2["pairs"]["M"])
    # the optimiser's closures: lm_optimise's error evaluations see the pair count of the last linearisation
    calls = []
    orig = R.sums

    def spy(tg, sr, pairs, T, hess=True, per_pair=False):
        calls.append((bool(hess), len(pairs["pi"])))
        return orig(tg, sr, pairs, T, hess, per_pair)
    W = R.world()
    R.sums = spy
    try:
        r = R.align(W["T"], W["S"], R.params(max_iters=2), W["guess"])
    finally:
        R.sums = orig
    assert [h for h, _ in calls] == [True, False, True, False] and r["n_evals"] == 4 and r["n_pairs_last"] == calls[-1][1] == calls[-2][1]


def test_scene_alignments_and_their_margins(now):
    assert len(R.ALIGN_CASES) >= 4
    for (seed, trans, rot, eps), c, f in zip(R.ALIGN_CASES, now["align_counts"], now["align_fig"]):
        print(f"[fgicp_ref] seed {seed} eps {eps}: counts {c.tolist()}, rho {f[2]:.2e} conv {f[3]:.2e} nn {f[4]:.2e} cut {f[5]:.2e}, "
              f"{1e3 * f[6]:.2f} mm from the truth (guess {1e3 * f[8]:.0f} mm)")
        assert c[0] == 1, seed
        assert f[8] >= 10.0 * f[6], (seed, f[8], f[6])                        # ends at least ten times closer in translation
        assert f[2] >= 1e-6 and f[3] >= 1e-6, (seed, "a rho-sign or convergence comparison decided by less than 1e-6")
        assert f[4] >= 1e-9 and f[5] >= 1e-9, (seed, "a nearest neighbour or a cut-off decided by less than 1e-9")
    assert [tuple(c[:5]) for c in now["align_counts"]] == [(1, 5, 10, 0, 2934), (1, 6, 12, 0, 2936), (1, 6, 12, 0, 2939), (1, 3, 6, 0, 2939)]
    assert (now["corr_gaps"][:2] >= 1e-9).all()                               # the poses of the one-linearisation cases that have pairs


def test_structs_match_the_header():
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()

    def size_from_text(name):
        """doubles first, then ints: no padding inside, the size a multiple of the widest member"""
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        total, widest = 0, 1
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            t, names = re.match(r"(long long|\w+)\s+(.*)", decl).groups()
            w = {"double": 8, "long long": 8, "int": 4, "float": 4}[t]
            widest = max(widest, w)
            for n in names.split(","):
                m = re.match(r"\s*\w+\s*(?:\[(\d+)\])?", n)
                total += w * (int(m.group(1)) if m.group(1) else 1)
        return -(-total // widest) * widest
    # five doubles and four ints; three ints and one
    assert (size_from_text("lisreg_fgicp_params"), size_from_text("lisreg_fgicp_info")) == (56, 16)
    for name, mine, size in (("lisreg_fgicp_params", lisreg.FgicpParams, size_from_text("lisreg_fgicp_params")),
                             ("lisreg_fgicp_info", lisreg.FgicpInfo, size_from_text("lisreg_fgicp_info")),
                             ("lisreg_fgicp_result", lisreg.FgicpResult, 168)):
        theirs = _header_struct(name)
        assert [(getattr(mine, n).offset, getattr(mine, n).size) for n, _ in mine._fields_] == \
               [(getattr(theirs, n).offset, getattr(theirs, n).size) for n, _ in theirs._fields_], name
        assert [n.rstrip("_") for n, _ in mine._fields_] == [n for n, _ in theirs._fields_], name       # ("lambda" is a Python keyword)
        assert C.sizeof(mine) == C.sizeof(theirs) == size, name
    v, f = _header_struct("lisreg_vgicp_result"), _header_struct("lisreg_fgicp_result")             # the fields of lisreg_vgicp_result, same order
    assert [(n, getattr(v, n).offset, getattr(v, n).size) for n, _ in v._fields_] == [(n, getattr(f, n).offset, getattr(f, n).size) for n, _ in f._fields_]


def test_library_exports_the_fgicp_symbols_and_defaults():
    import lisreg
    L = lisreg.lib()
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in lisreg.ABI_SYMBOLS, s
        assert re.search(r"^\s*int\s+%s\s*\(" % s, hdr, re.M), s
    p = lisreg.fgicp_default_params()
    assert {n: getattr(p, n) for n, _ in p._fields_ if n != "reserved"} == R.DEFAULTS == R.params(0)
    p1 = lisreg.fgicp_default_params(1)
    assert {n: getattr(p1, n) for n, _ in p1._fields_ if n != "reserved"} == R.params(1)
    assert p1.max_correspondence_distance == float(np.finfo(np.float32).max) == R.FLT_MAX and np.isfinite(R.FLT_MAX * R.FLT_MAX)
    assert lisreg.fgicp_default_params(transformation_epsilon=5e-4).transformation_epsilon == 5e-4
    with pytest.raises(AttributeError):
        lisreg.fgicp_default_params(resolution=1.0)
    assert L.lisreg_fgicp_default_params(2, C.byref(p)) == lisreg.ERR_ARG and L.lisreg_fgicp_default_params(-1, C.byref(p)) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_default_params(0, None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_set_target(None, 0, None, 0, 0, 0, C.byref(p), None, 0.0) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_align(None, 0, None, 0, 0, 0, C.byref(p), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_correspondences(None, 0, None, 0, 0, 0, C.byref(p), None, None, None) == lisreg.ERR_ARG
    assert L.lisreg_fgicp_linearize(None, 0, None, 0, 0, 0, C.byref(p), None, None, 1, None, None) == lisreg.ERR_ARG
    for text in ("registration.cpp:157-166", "subMapOptmizationNode.cpp:2771", "lisreg_nearest", "tests/fgicp_ref.py"):
        assert text in hdr[hdr.index("§7l"):hdr.index("loop-closure candidate detection: FEPSC")], text


def test_golden_file_regenerates_from_the_restatement(now):
    g = np.load(GOLDEN)
    assert os.path.getsize(GOLDEN) < 64 * 1024
    assert sorted(now) == sorted(g.files)
    for k in g.files:
        a, b = g[k], now[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind in "iu":
            assert np.array_equal(a, b), k
    # doubles: LAPACK / BLAS builds may add in another order; everything else is the same arithmetic
    assert np.array_equal(g["lin_T"], now["lin_T"])
    assert np.all(np.abs(g["lin_out"] - now["lin_out"]) <= 1e-11 * g["lin_abs"]) and np.allclose(g["lin_abs"], now["lin_abs"], rtol=1e-11, atol=0)
    assert np.allclose(g["corr_gaps"], now["corr_gaps"], rtol=1e-6, atol=0)
    assert np.allclose(g["align_T"], now["align_T"], rtol=0, atol=1e-8)
    assert np.allclose(g["align_fig"][:, [0, 1]], now["align_fig"][:, [0, 1]], rtol=1e-6, atol=0)
    assert np.allclose(g["align_fig"][:, 2:], now["align_fig"][:, 2:], rtol=1e-3, atol=1e-12)
    assert g["corr_idx"].shape == (3, 368) and (g["corr_idx"][2] == -1).all() and (g["corr_idx"][:2] >= 0).all()
    assert list(g["lin_pairs"]) == [2939, 2939, 2939, 2939, 0, 0, 2939, 2939]
    assert np.abs(g["lin_out"][6] - g["lin_out"][2]).max() > 1e-3                 # pairs of the guess, sums at the truth: not a fresh linearisation
