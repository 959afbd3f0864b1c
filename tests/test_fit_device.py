"""Device-level parity of the residual models (`plane5_closed`).

The production build forms surfOptimization's plane (odomEstimationNode.cpp:776-791) in closed form (`plane5_closed`,
lisreg_assoc.hip) and hands near-collinear neighbourhoods to the column-pivoted QR.  `tests/test_oracle_units.py` checks a Python
restatement of that formula; THIS file runs the DEVICE functions themselves (`lisreg_test_fit_models`: `surf_model` + `surf_eval`,
`corner_model` + `corner_eval`, one case per thread, the same code the correspondence kernel inlines) on caller-given neighbourhoods
and compares with the oracle (`orc_surf_coeff` / `orc_corner_coeff`, the reference's float QR / cv::eigen) and with the float64
least-squares plane, on patches at |p| = 10 ... 1 000 m (KITTI-00 map scale: SURVEY.md section 7 "fp32 conditioning").

What is compared is what reaches the normal equations: the point-to-plane distance at the query (coeff.intensity / |coeff.xyz|), the
unit normal (coeff.xyz / |coeff.xyz|) and the accept flag.  Bars (in the tests, per distance band): the production arithmetic against the FLOAT64 plane of the same
float32 neighbours (maximum over 2 000 patches), against the ORACLE in the median (2e-5 m up to 100 m) and — because the reference's own
float QR on uncentred coordinates is up to 0.6 mm off the float64 plane at 100 m already (condition number ~ |p| / patch size) — in the
maximum only through that float64 plane; and the device must be no farther from the float64 plane than the oracle is (the closed form
works on centred differences: it is closer).
The exact-arithmetic build must reproduce the oracle's coefficients TO THE BIT.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import copy_params

f32 = np.float32


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def make_patches(rng, n, dist, spread=(0.05, 0.5), noise=0.01, through_origin=False):
    """n planar 5-point neighbourhoods centred `dist` metres from the origin + one query 5 cm off each; float32 inputs."""
    nb = np.zeros((n, 5, 3), f32); q = np.zeros((n, 3), f32)
    for i in range(n):
        while True:
            centre = rng.normal(0, 1, 3); centre *= dist / np.linalg.norm(centre)
            nrm = rng.normal(0, 1, 3); nrm /= np.linalg.norm(nrm)
            if through_origin:
                nrm -= (nrm @ centre) / (centre @ centre) * centre; nrm /= np.linalg.norm(nrm)      # the plane contains the origin: n . p = -1 has no solution
                break
            if abs(nrm @ centre) >= 0.05 * dist:
                break
        u = np.cross(nrm, [1.0, 0, 0]); u /= np.linalg.norm(u); v = np.cross(nrm, u)
        s = rng.uniform(*spread)
        p = centre + np.outer(rng.uniform(-s, s, 5), u) + np.outer(rng.uniform(-s, s, 5), v) + np.outer(rng.normal(0, noise, 5), nrm)
        nb[i] = p.astype(f32)
        q[i] = (p.mean(0) + 0.05 * nrm + 0.1 * s * u).astype(f32)
    return nb, q


def oracle_surf(oc, nb, q, p):
    L = oc.lib()
    cf = np.zeros((len(nb), 4), f32); ok = np.zeros(len(nb), np.int32)
    for i in range(len(nb)):
        ok[i] = L.orc_surf_coeff(_fp(np.ascontiguousarray(nb[i])), _fp(np.ascontiguousarray(q[i])), 1.0, C.byref(p), _fp(cf[i]))
    return cf, ok


def oracle_corner(oc, nb, q, p):
    L = oc.lib()
    cf = np.zeros((len(nb), 4), f32); ok = np.zeros(len(nb), np.int32)
    for i in range(len(nb)):
        ok[i] = L.orc_corner_coeff(_fp(np.ascontiguousarray(nb[i])), _fp(np.ascontiguousarray(q[i])), 1.0, C.byref(p), _fp(cf[i]))
    return cf, ok


def truth_plane(nb):
    """float64 least-squares plane of the float32 neighbours: (unit normal, offset), n . p + d = 0 form of [p_j] x = -1"""
    out = np.zeros((len(nb), 4))
    for i, P in enumerate(nb.astype(np.float64)):
        x = np.linalg.lstsq(P, -np.ones(5), rcond=None)[0]
        out[i] = np.append(x, 1.0) / np.linalg.norm(x)
    return out


def dist_and_normal(cf):
    s = np.linalg.norm(cf[:, :3].astype(np.float64), axis=1)
    s = np.where(s > 0, s, 1.0)
    return cf[:, 3].astype(np.float64) / s, cf[:, :3].astype(np.float64) / s[:, None]


def compare_surf(ctx, oc, lisreg, nb, q):
    po = oc.default_params(1); pl = copy_params(po, lisreg.Params)
    dev = ctx.test_fit_models(1, nb, q, pl)
    dev_exact = ctx.test_fit_models(1, nb, q, pl, exact=True)
    cfo, oko = oracle_surf(oc, nb, q, po)
    tp = truth_plane(nb)
    d_true = np.einsum("ij,ij->i", tp[:, :3], q.astype(np.float64)) + tp[:, 3]
    d_dev, n_dev = dist_and_normal(dev[:, 5:9]); d_orc, n_orc = dist_and_normal(cfo)
    both = (dev[:, 9] == 1) & (oko == 1)
    return dict(dev=dev, dev_exact=dev_exact, cfo=cfo, oko=oko, both=both, d_true=d_true, d_dev=d_dev, d_orc=d_orc, n_dev=n_dev, n_orc=n_orc, tp=tp)


# (distance from the map origin, bar on the MEDIAN |device - oracle| of the point-to-plane distance at the query, bar on the MAXIMUM |device - float64|)
BANDS = [(10.0, 2e-5, 1e-5), (100.0, 2e-5, 4e-5), (300.0, 6e-5, 2e-4), (1000.0, 2e-4, 6e-4)]
# (distance from the map origin, bar on the MAXIMUM |device - oracle| of the point-to-line distance at the query)
LINE_BANDS = [(10.0, 2e-5), (100.0, 3e-5), (1000.0, 4e-4)]


@pytest.mark.gpu
@pytest.mark.parametrize("dist,bar_oracle,bar_truth", BANDS)
def test_device_plane_fit_matches_oracle_far_from_origin(gpu_ctx, oracle, dist, bar_oracle, bar_truth):
    import lisreg
    rng = np.random.default_rng(int(dist) + 7)
    nb, q = make_patches(rng, 2000, dist)
    r = compare_surf(gpu_ctx, oracle, lisreg, nb, q)
    both = r["both"]
    assert both.sum() >= 1800                                    # planar patches, query 5 cm off: nearly all accepted by both
    # the closed form produced these planes (not the QR fall-back)
    assert (r["dev"][:, 4] == 1).mean() >= 0.99
    # accept flags: equal except where s or a |n.p + d| sits on its threshold (none expected on these patches at <= 100 m)
    disagree = int((r["dev"][:, 9] != r["oko"]).sum())
    assert disagree <= (0 if dist <= 100 else 4), disagree
    e_do = np.abs(r["d_dev"] - r["d_orc"])[both]; e_dt = np.abs(r["d_dev"] - r["d_true"])[both]; e_ot = np.abs(r["d_orc"] - r["d_true"])[both]
    print(f"|p| = {dist:6.0f} m: point-to-plane distance at the query, max |device - oracle| {e_do.max():.2e}, |device - f64| {e_dt.max():.2e}, "
          f"|oracle - f64| {e_ot.max():.2e} (medians {np.median(e_do):.1e} / {np.median(e_dt):.1e} / {np.median(e_ot):.1e}); accept flags differ in {disagree}")
    # (1) the device against the float64 plane of the same float32 neighbours
    assert e_dt.max() <= bar_truth
    # (2) against the oracle: typically within bar_oracle; the WORST case is the oracle's own (its float QR on uncentred coordinates loses
    # cond(A) eps ~ |p| / patch size * 6e-8: 0.6 mm at 100 m on a 5 cm patch), so the maximum is bounded through the float64 plane
    assert np.median(e_do) <= bar_oracle
    assert e_do.max() <= e_ot.max() + bar_truth
    # (3) the device is no farther from the float64 plane than the reference's float QR is (it is closer: centred differences)
    assert np.quantile(e_dt, 0.99) <= np.quantile(e_ot, 0.99) + 2e-6
    # (4) unit normals likewise (a 5 cm patch with 1 cm of noise does not pin its normal better than the coordinates' ulp / 5 cm)
    en_d = np.abs(r["n_dev"] - r["tp"][:, :3])[both].max(1); en_o = np.abs(r["n_orc"] - r["tp"][:, :3])[both].max(1)
    print(f"           unit normal, |device - f64| max {en_d.max():.2e} q99 {np.quantile(en_d, 0.99):.2e}; |oracle - f64| max {en_o.max():.2e} q99 {np.quantile(en_o, 0.99):.2e}")
    assert np.quantile(en_d, 0.99) <= np.quantile(en_o, 0.99) + 1e-5 and en_d.max() <= en_o.max() + 1e-5
    # the exact-arithmetic build IS the oracle: coefficients and flags to the bit
    ex = r["dev_exact"]
    assert np.array_equal(ex[:, 9].astype(np.int32), r["oko"])
    acc = r["oko"] == 1
    assert np.array_equal(ex[acc, 5:9].view(np.uint32), r["cfo"][acc].view(np.uint32))


@pytest.mark.gpu
def test_device_plane_fit_hand_over_to_qr(gpu_ctx, oracle):
    """Near-collinear neighbourhoods around kPlaneLineRatio (second eigenvalue of the scatter matrix / first = 1e-2): at half the
    ratio the QR runs (flag 0), at twice the ratio the closed form does; either way the coefficients stay with the oracle's.  A plane
    THROUGH the map origin (n . p = -1 has no solution: the reference's QR returns a huge |n|, pd ~ 0) and five coincident points are
    handed over too or rejected consistently."""
    import lisreg
    po = oracle.default_params(1); pl = copy_params(po, lisreg.Params)
    rng = np.random.default_rng(99)

    def strip(ratio, n, dist):
        nb = np.zeros((n, 5, 3), f32); q = np.zeros((n, 3), f32)
        for i in range(n):
            centre = rng.normal(0, 1, 3); centre *= dist / np.linalg.norm(centre)
            nrm = centre / np.linalg.norm(centre) + 0.3 * rng.normal(0, 1, 3); nrm /= np.linalg.norm(nrm)
            u = np.cross(nrm, [0.0, 0, 1.0]); u /= np.linalg.norm(u); v = np.cross(nrm, u)
            t = np.array([-0.4, -0.2, 0.0, 0.2, 0.4])                     # along the line; across it with sqrt(ratio) of the spread
            w = np.sqrt(ratio) * np.array([0.4, -0.4, 0.0, -0.4, 0.4]) * (0.4 / 0.64) ** 0.5        # sum t w = 0, sum w^2 = ratio * sum t^2
            p = centre + np.outer(t, u) + np.outer(w, v)
            nb[i] = p.astype(f32); q[i] = (centre + 0.04 * nrm).astype(f32)
        return nb, q

    for ratio, want_closed in ((0.5e-2, 0.0), (2e-2, 1.0)):
        nb, q = strip(ratio, 500, 30.0)
        dev = gpu_ctx.test_fit_models(1, nb, q, pl)
        cfo, oko = oracle_surf(oracle, nb, q, po)
        assert (dev[:, 4] == want_closed).mean() >= 0.98, (ratio, dev[:, 4].mean())
        both = (dev[:, 9] == 1) & (oko == 1)
        assert both.sum() >= 450 and (dev[:, 9] != oko).sum() <= 2
        d_dev, n_dev = dist_and_normal(dev[:, 5:9]); d_orc, n_orc = dist_and_normal(cfo)
        # a strip constrains the plane's tilt about its long axis badly (that is why the QR keeps these): the distance AT the query, which
        # sits on the strip, still agrees
        assert np.abs(d_dev - d_orc)[both].max() <= (5e-5 if want_closed else 2e-5), (ratio, np.abs(d_dev - d_orc)[both].max())
    # planes through the origin: whatever the reference's QR makes of them, the production build must decide accept / reject the same way
    nb, q = make_patches(rng, 500, 40.0, through_origin=True)
    dev = gpu_ctx.test_fit_models(1, nb, q, pl)
    cfo, oko = oracle_surf(oracle, nb, q, po)
    frac = float((dev[:, 9] != oko).mean())
    print("planes through the origin: accept flags differ in", frac)
    assert frac <= 0.02
    # five coincident points: S = 0, ww = 0 -> QR (rank 1) -> whatever it returns fails or passes like the oracle
    nb = np.tile(np.array([[3.0, 4.0, 5.0]], f32), (8, 5, 1)); q = np.tile(np.array([[3.0, 4.0, 5.05]], f32), (8, 1))
    dev = gpu_ctx.test_fit_models(1, nb, q, pl)
    cfo, oko = oracle_surf(oracle, nb, q, po)
    assert (dev[:, 4] == 0).all() and np.array_equal(dev[:, 9].astype(np.int32), oko)


@pytest.mark.gpu
def test_device_line_fit_matches_oracle(gpu_ctx, oracle):
    """cornerOptimization's body on the device (production: cyclic Jacobi; exact build: cv::eigen's pivot order) against the oracle,
    at 10 ... 1 000 m from the origin: point-to-line distance at the query and the accept flag."""
    import lisreg
    po = oracle.default_params(1); pl = copy_params(po, lisreg.Params)
    rng = np.random.default_rng(5)
    for dist, bar in LINE_BANDS:
        n = 1500
        nb = np.zeros((n, 5, 3), f32); q = np.zeros((n, 3), f32)
        for i in range(n):
            centre = rng.normal(0, 1, 3); centre *= dist / np.linalg.norm(centre)
            d = rng.normal(0, 1, 3); d /= np.linalg.norm(d)
            off = np.cross(d, rng.normal(0, 1, 3)); off /= np.linalg.norm(off)
            p = centre + np.outer(rng.uniform(-0.6, 0.6, 5), d) + rng.normal(0, 0.01, (5, 3))
            nb[i] = p.astype(f32); q[i] = (centre + 0.08 * off + 0.1 * d).astype(f32)
        dev = gpu_ctx.test_fit_models(0, nb, q, pl)
        ex = gpu_ctx.test_fit_models(0, nb, q, pl, exact=True)
        cfo, oko = oracle_corner(oracle, nb, q, po)
        both = (dev[:, 9] == 1) & (oko == 1)
        assert both.sum() >= 0.9 * n and (dev[:, 9] != oko).sum() <= (0 if dist <= 100 else 6)
        d_dev, n_dev = dist_and_normal(dev[:, 5:9]); d_orc, n_orc = dist_and_normal(cfo)
        e = np.abs(d_dev - d_orc)[both]
        print(f"|p| = {dist:6.0f} m: point-to-line distance at the query, max |device - oracle| {e.max():.2e} (median {np.median(e):.1e})")
        assert e.max() <= bar
        assert np.array_equal(ex[:, 9].astype(np.int32), oko)
        acc = oko == 1
        assert np.array_equal(ex[acc, 5:9].view(np.uint32), cfo[acc].view(np.uint32))
