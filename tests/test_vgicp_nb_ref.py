"""The CPU side of the VGICP neighbourhoods: tests/vgicp_nb_ref.py, the definition of lisreg_vgicp_params.neighbor_search,
against itself and against tests/vgicp_ref.py; the golden file; the margins of every alignment case tests/test_vgicp_nb.py uses; a census
of the grid-border cases; the layout of the parameter struct.  Needs no GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import vgicp_nb_ref as N
import vgicp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def now():
    return N.golden_cases()


def test_offsets_of_the_three_modes():
    assert N.offsets(1).tolist() == [[0, 0, 0]]
    assert N.offsets(7).tolist() == [[0, 0, -1], [0, -1, 0], [-1, 0, 0], [0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
    o = N.offsets(27)
    ids = (o[:, 0] + 1) + 3 * (o[:, 1] + 1) + 9 * (o[:, 2] + 1)
    assert ids.tolist() == list(range(27))                                  # ascending cell id: dz outermost, dx innermost
    o7 = N.offsets(7)
    assert ((o7[:, 0] + 1) + 3 * (o7[:, 1] + 1) + 9 * (o7[:, 2] + 1)).tolist() == [4, 10, 12, 13, 14, 16, 22]
    for bad in (0, 2, -1, 26, 28):
        with pytest.raises(ValueError):
            N.offsets(bad)


def test_mode_1_is_the_restatement_of_direct1():
    W = R.world()
    for T in R.lin_poses(W["guess"], W["T_true"]):
        pi, vi, face = R.find_pairs(W["T"], W["S"], T)
        p1, v1, f1 = N.find_pairs(W["T"], W["S"], T, 1)
        assert np.array_equal(pi, p1) and np.array_equal(vi, v1) and face == f1
        for hess in (True, False):
            a, b = R.linearize(W["T"], W["S"], T, hess), N.linearize(W["T"], W["S"], T, 1, hess)
            assert a["out"].tobytes() == b["out"].tobytes() and a["abs"].tobytes() == b["abs"].tobytes() and a["n_pairs"] == b["n_pairs"]
    r, r1 = R.align(W["T"], W["S"], R.params(), W["guess"]), N.align(W["T"], W["S"], R.params(), 1, W["guess"])
    assert r["T"].tobytes() == r1["T"].tobytes() and r["log"] == r1["log"] and r["n_pairs_last"] == r1["n_pairs_last"]


@pytest.mark.parametrize("mode", N.MODES)
def test_loop_form_equals_vector_form(mode):
    """257 points of the source, the NaN source and the flat target; the pairs equal as lists, the sums to rounding"""
    W = R.world()
    xyz, S = N.nan_source()
    T = W["guess"].astype(np.float64)
    B = N.border_poses(W["T"], S, T)
    for tgt, P in ((W["T"], T), (W["T"], B["+x1"]), (W["T"], B["-z2"]), (N.flat_world()["T"], T), (W["T"], N.far_pose(T))):
        pi, vi, _ = N.find_pairs(tgt, S, P, mode)
        pl, vl = N.find_pairs_loops(tgt, S, P, mode)
        assert np.array_equal(pi, pl) and np.array_equal(vi, vl)
        assert not np.isin(pi, [5, 64, 130, 200]).any()                     # the NaN points pair with nothing
        for hess in (True, False):
            a, b = N.linearize(tgt, S, P, mode, hess), N.linearize_loops(tgt, S, P, mode, hess)
            assert a["n_pairs"] == b["n_pairs"] == len(pi)
            assert np.all(np.abs(a["out"] - b["out"]) <= 1e-12 * a["abs"]) and np.allclose(a["abs"], b["abs"], rtol=1e-12, atol=0)
            if not hess:
                assert not a["out"][7:].any() and not b["out"][7:].any()


def test_pairs_of_a_larger_mode_contain_the_smaller_ones():
    W = R.world()
    T = W["guess"].astype(np.float64)
    sets = {m: set(zip(*(a.tolist() for a in N.find_pairs(W["T"], W["S"], T, m)[:2]))) for m in N.MODES}
    assert sets[1] < sets[7] < sets[27]
    print(f"[vgicp_nb] pairs at the guess: {[len(sets[m]) for m in N.MODES]}")
    assert len(sets[1]) <= len(W["src"]) < len(sets[7]) < len(sets[27])     # pairs, not points


def test_alignment_cases_and_their_margins(now):
    """only cases whose rho-sign and convergence margins exceed 1e-6 in the restatement may be compared on the GPU"""
    for c, f in zip(now["align_counts"], now["align_fig"]):
        print(f"[vgicp_nb] case {c[6]} mode {c[7]}: converged {c[0]} iters {c[1]} evals {c[2]} rejected {c[3]} pairs {c[4]}; "
              f"{1e3 * f[5]:.2f} mm / {1e3 * f[6]:.3f} mrad from the truth; margins rho {f[2]:.2e} convergence {f[3]:.2e} face {f[4]:.2e} m")
        assert c[0] == 1 and f[2] > 1e-6 and f[3] > 1e-6, (c, f)
        assert f[4] >= 1e-9, (c, "a transformed point within 1e-9 m of a voxel face")
        assert c[4] > c[5]                                                  # more pairs than points
    assert [tuple(c[[6, 7]]) for c in now["align_counts"]] == list(N.ALIGN_RUNS)
    assert [tuple(c[:4]) for c in now["align_counts"][:4]] == [(1, 5, 19, 10), (1, 2, 10, 6), (1, 6, 19, 8), (1, 4, 8, 0)]
    # the coarse guess: DIRECT27 ends within 10 mm of the truth where DIRECT1 reports convergence metres away
    W, prm = N.align_case(len(R.ALIGN_CASES))
    r1 = R.align(W["T"], W["S"], prm, W["guess"])
    e1, e27 = R.pose_error(r1["T"], W["T_true"])[0], now["align_fig"][-1][5]
    print(f"[vgicp_nb] coarse guess {N.COARSE}: DIRECT1 converged {r1['converged']} {1e3 * e1:.1f} mm from the truth, DIRECT27 {1e3 * e27:.2f} mm")
    assert r1["converged"] == 1 and e1 > 1.0 and e27 < 0.010


def test_census_of_the_border_cases():
    """the events tests/test_vgicp_nb.py is after really occur: points whose own cell is outside the grid and that still pair, and
    points inside with offsets out of range"""
    W = R.world()
    T = W["guess"].astype(np.float64)
    B = N.border_poses(W["T"], W["S"], T)
    assert sorted(B) == sorted(s + a + d for s in "+-" for a in "xyz" for d in "12")
    for name, P in B.items():
        for mode in N.NB_MODES:
            c = N.census(W["T"], W["S"], P, mode)
            print(f"[vgicp_nb] border {name} mode {mode}: {c}")
            assert c["outside_pairing"] > 0 and c["inside_clipped"] > 0 and c["pairs"] > 0, (name, mode, c)
            if name.endswith("1"):
                assert c["outside_pairing"] <= c["outside"]
            else:
                assert c["outside_pairing"] < c["outside"], (name, mode, c)  # two cells out: some points beyond every voxel's reach
    F = N.flat_world()
    assert F["T"]["dims"][2] == 1 and len(F["tgt"]) >= R.PLANTED_K
    for mode in N.NB_MODES:
        c = N.census(F["T"], W["S"], T, mode)
        print(f"[vgicp_nb] flat target mode {mode}: {c}")
        assert c["outside_pairing"] > 0 and c["inside_clipped"] > 0
        own_in = len(W["src"]) - c["outside"]
        assert c["inside_clipped"] == own_in                                # every dz = +-1 offset of a point inside is out of range
        assert N.census(W["T"], W["S"], N.far_pose(T), mode) == dict(outside_pairing=0, inside_clipped=0, pairs=0, outside=len(W["src"]))
    xyz, S = N.nan_source()
    assert np.isnan(xyz).any(1).sum() == 4 and S["ok"].sum() == len(xyz) - 4


def test_golden_file_regenerates_from_the_restatement(now):
    g = np.load(N.GOLDEN)
    assert os.path.getsize(N.GOLDEN) < 64 * 1024
    assert sorted(now) == sorted(g.files)
    for k in g.files:
        a, b = g[k], now[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        if a.dtype.kind in "iu":
            assert np.array_equal(a, b), k
    # doubles: LAPACK / BLAS builds may add in another order; everything else is the same arithmetic
    assert np.array_equal(g["lin_T"], now["lin_T"]) and np.array_equal(g["lin_T"], np.load(os.path.join(os.path.dirname(N.GOLDEN), "vgicp_cases.npz"))["lin_T"])
    assert np.all(np.abs(g["lin_out"] - now["lin_out"]) <= 1e-11 * g["lin_abs"]) and np.allclose(g["lin_abs"], now["lin_abs"], rtol=1e-11, atol=0)
    assert np.allclose(g["align_T"], now["align_T"], rtol=0, atol=1e-8)
    assert np.allclose(g["align_fig"][:, [0, 1]], now["align_fig"][:, [0, 1]], rtol=1e-6, atol=0)
    assert np.allclose(g["align_fig"][:, 2:], now["align_fig"][:, 2:], rtol=1e-3, atol=1e-12)
    pairs = g["lin_pairs"].reshape(2, 3, len(R.LIN_SIZES), 2)
    assert (pairs[:, 2] == 0).all() and (pairs[:, :, :, 0] == pairs[:, :, :, 1]).all()
    assert (pairs[0, :2, -1] > 5 * 2939).all() and (pairs[1, :2, -1] > 15 * 2939).all()


def test_the_field_keeps_its_place_in_the_struct():
    """neighbor_search is the struct's last int, which keeps the member name `reserved` in the header and in the ctypes mirror (the
    member names of both are pinned by tests/test_vgicp_ref.py): the same size, the same offset, 0 by default, and the ctypes mirror
    reaches it through a property over its unchanged field list"""
    import lisreg
    hdr = open(os.path.join(ROOT, "include", "lisreg.h")).read()
    body = re.search(r"typedef struct lisreg_vgicp_params \{(.*?)\} lisreg_vgicp_params;", hdr, re.S).group(1)
    names = re.findall(r"^\s*(?:double|int)\s+(\w+);", body, re.M)
    assert names == [n for n, _ in lisreg.VgicpParams._fields_] and names[-1] == "reserved"
    assert re.search(r"int\s+reserved;\s*/\* neighbor_search:", body)
    assert C.sizeof(lisreg.VgicpParams) == 56 and lisreg.VgicpParams.reserved.offset == 52 and lisreg.VgicpParams.reserved.size == 4
    for name, value in (("LISREG_VGICP_DIRECT1", 1), ("LISREG_VGICP_DIRECT7", 7), ("LISREG_VGICP_DIRECT27", 27)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), hdr, re.M), name
    assert (lisreg.VGICP_DIRECT1, lisreg.VGICP_DIRECT7, lisreg.VGICP_DIRECT27) == (1, 7, 27)
    p = lisreg.vgicp_default_params()
    assert p.neighbor_search == 0 and p.reserved == 0 and lisreg.VgicpParams().neighbor_search == 0
    p.neighbor_search = 27
    assert p.reserved == 27 and bytes(p)[52:56] == (27).to_bytes(4, "little")
    q = lisreg.vgicp_default_params(neighbor_search=7, max_iters=3)
    assert (q.neighbor_search, q.reserved, q.max_iters) == (7, 7, 3)
    assert {n: getattr(q, n) for n, _ in q._fields_ if n != "reserved"} == dict(R.DEFAULTS, max_iters=3)
    for text in ("tests/vgicp_nb_ref.py", "neighbor_search", "ascending cell id"):
        assert text in hdr, text
