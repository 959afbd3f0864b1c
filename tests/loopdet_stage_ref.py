"""Glue of test_loopdet_stages: the crafted scenes, one run of the restatement per case (cached), and the stage-by-stage ("forced")
comparison of a device run with loopdet_ref (R) / loopdet_kinds_ref (K) applied to the device's own input to each stage: the stored
projections to the yaw search and ICP, the ICP's transform to the binning, the stored and the pair descriptors to the scores, the
scores to the selection.  Every integer, and every double formed from integers, is then known exactly."""
import math
import struct

import numpy as np

import loopdet_ref as R
import loopdet_kinds_ref as K
from test_loopdet_kinds import pcl, polar, _drive

DIST_KINDS = (K.ISC, K.SC, K.EPSC, K.SEPSC, K.FEPSC)
DEFAULT = (20.0, 0.01, 0.75)
GATE_ALL = (20.0, 10.0, 0.75)          # an inflation of 10: every history frame more than 20 m of travel back is gated
EDGE_CAP = 16                          # cells an atan2f ulp may decide (the cap of the end-to-end tests)
ROT_BOUND = 1e-5                       # matched rotation entries: a few ulp of pi (atan2f) + a few ulp of 1 (sinf, cosf) < 2e-6
NON_PROJ = (9, 10, 11, 12, 15, 17, 3, 25)


def bits(x):
    return struct.pack("<d", float(x))


def same_double(a, b):
    return bits(a) == bits(b) or (math.isnan(a) and math.isnan(b))


# ---- scenes: points at (r, degrees, z, label, intensity), at least 0.25 degrees from every 1 and 4.5 degree edge ------------------

def ring_r(ring):
    return R.MIN_DIS + R.RING_STEP * (ring + 0.5)


def place(r, d, z):
    """polar(); a point of the second half turn is the exact negative of the one half a turn before it."""
    if d < 180.0:
        return polar(r, math.radians(d), z)
    x, y, _ = polar(r, math.radians(d - 180.0), z)
    return [-x, -y, z]


def cloud(items):
    items = list(items)
    if not items:
        return pcl(np.zeros((0, 3)), [], [])
    return pcl([place(r, d, z) for r, d, z, _, _ in items], [it[3] for it in items], [it[4] for it in items])


def frame(sem, corner, surf, yaw, x, y=0.0):
    from lisreg import synth
    return dict(corner=cloud(corner), surf=cloud(surf), semantic=cloud(sem), odom=synth.pose_matrix([0, 0, yaw, x, y, 0])[:3].astype(np.float32))


def repeat(items, period):
    """items of the first `period` sectors, repeated round the circle."""
    step = 4.5 * period
    return [(r, d + step * b, z, lab, it) for b in range(R.SECTORS // period) for r, d, z, lab, it in items]


def periodic_scene(period):
    """the same content every `period` sectors (1 or 4), in all three clouds.  Nine projection-labelled points at 3.5 m, two per
    1-degree column (the later one is the column's), fill the block's first sector: with period 1 every column counts 2; with period 4
    the counts are 2 2 2 2 1 and thirteen zeros, every 18 columns.  z above 5.24 m and an intensity above 1 wrap SC and ISC."""
    sem = [(3.5, 0.25 + 0.5 * i, -1.0 + 0.25 * i, (13, 18)[i % 2], 0.1 * i) for i in range(9)]
    sem += [(ring_r(2), 2.25, 0.5, 9, 0.3), (ring_r(2), 2.75, 6.0, 10, 1.2), (ring_r(5), 1.25, 1.0, 15, 0.7)]
    corner = [(ring_r(2), 2.25, 0.0, 0, 0.0)]
    surf = [(ring_r(2), 1.75, 0.0, 0, 0.0)] * 3 + [(ring_r(5), 3.25, 0.0, 0, 0.0)] * 2
    if period == 4:
        sem += [(ring_r(3), 4.5 + 1.25, 0.0, 11, 0.4)]
        surf += [(ring_r(3), 4.5 + 2.25, 0.0, 0, 0.0)]
    return repeat(sem, period), repeat(corner, period), repeat(surf, period)


def scatter_scene(seed, proj_r=2.0, labels=NON_PROJ, drop=0.0, turn=0):
    """an aperiodic scene: per sector a few surf, corner and semantic points at ring centres, and the projection-labelled points of
    projected() (proj_r: their radius, below 3 m they stay out of the descriptors; None: none).  drop: the fraction of the other
    points left out; turn: sectors by which the other points are turned.  The projection points never change."""
    rng = np.random.default_rng(seed)
    sem, corner, surf = [], [], []
    for s in range(R.SECTORS):
        for dst, n in ((surf, rng.integers(0, 5)), (corner, rng.integers(0, 3)), (sem, rng.integers(0, 5))):
            for _ in range(n):
                d = 4.5 * s + 0.25 + 0.5 * rng.integers(0, 9)
                dst.append((ring_r(rng.integers(0, 9)), d, rng.uniform(-3, 9), int(rng.choice(labels)), rng.uniform(0, 1.3)))
    keep = np.random.default_rng(seed + 1000).random(len(sem) + len(corner) + len(surf)) >= drop
    it = iter(keep)
    sem, corner, surf = ([(r, (d + 4.5 * turn) % 360.0, z, lab, i) for r, d, z, lab, i in c if next(it)] for c in (sem, corner, surf))
    if proj_r is not None:
        sem += projected(proj_r)
    return sem, corner, surf


def projected(r):
    """the projection-labelled points of every scatter scene: a random half of the first 180 columns and the columns half a turn on.
    Two frames' sector clouds are then the same cloud with its mean at exactly zero (place()), the yaw search finds shift 0 or 360,
    and the ICP's first step is the identity in float32 with a translation of exactly zero: it ends there, `transformation epsilon
    reached`, on any arithmetic.  (An ICP that goes on after its correspondences have settled ends when two mean squared errors
    differ by less than 1e-12, which rounding noise decides; the drive's ICPs all move through their ten iterations.)"""
    rng = np.random.default_rng(99)
    half = [(r, c + (0.25, 0.75)[int(rng.integers(0, 2))], 0.2, int(rng.choice(R.PROJ_LABELS)), 0.5)
            for c in np.nonzero(rng.random(R.PROJ // 2) < 0.5)[0]]
    return half + [(r, d + 180.0, z, lab, i) for r, d, z, lab, i in half]


def outside_scene(seed):
    """nothing between 3 m and 60 m: every descriptor is empty; the projection points at 2 m still drive the yaw search and the ICP."""
    sem, corner, surf = scatter_scene(seed)
    far = lambda c: [((1.5, 65.0)[k % 2], d, z, lab, i) for k, (r, d, z, lab, i) in enumerate(c) if r > R.MIN_DIS]
    return [p for p in sem if p[0] < R.MIN_DIS] + far(sem), far(corner), far(surf)


def many_projected(n):
    """n projection-labelled points at 2 m, dealt over the 360 columns."""
    return [(2.0, (k % R.PROJ) + (0.25, 0.75)[(k // R.PROJ) % 2], 0.0, R.PROJ_LABELS[k % 5], 0.5) for k in range(n)]


def extended_drive():
    """_drive() and one more key frame beside history frame 23 (the frame before it is 0.1 m from there: gated), turned 0.03 rad
    below it: a slightly negative yaw difference, a wrapped yaw of 358 sectors (the modulo-360 columns)."""
    from lisreg import synth
    frames = _drive()
    th = 2 * np.pi * 23 / 24
    T = np.array([0.0, 0.0, th + np.pi / 2 - 0.03, 12.1 * np.cos(th), 12.1 * np.sin(th), synth.SENSOR_Z], np.float64)
    s = synth.make_scan(16, 361, seed=3000, labelled=True, T_true=T)
    rng = np.random.default_rng(100 + len(frames))
    sem = synth.concat_clouds([s["corner"], s["surf"]])
    sem["intensity"] = rng.uniform(0.0, 1.3, len(sem)).astype(np.float32)
    tall = rng.random(len(sem)) < 0.05
    sem["z"][tall] = rng.uniform(5.3, 9.0, int(tall.sum())).astype(np.float32)
    frames.append(dict(corner=s["corner"], surf=s["surf"], semantic=sem, odom=synth.pose_matrix(T)[:3].astype(np.float32)))
    return frames


def _case_frames(name):
    if name == "drive":
        return extended_drive()
    if name == "all_tie":
        sc = periodic_scene(1)
        return [frame(*sc, 0.0, x) for x in (0.0, 21.0, 0.0)]
    if name == "periodic":            # the revisits are turned by 18 and 36 degrees: the 18-degree-periodic scene looks the same
        sc = periodic_scene(4)
        return [frame(*sc, math.radians(a), x) for a, x in ((0.0, 0.0), (18.0, 21.0), (54.0, 0.0))]
    if name == "shifted":             # the content (not the projection) turned by +3 sectors, then back
        return [frame(*scatter_scene(7, turn=t), 0.0, x) for t, x in ((0, 0.0), (3, 21.0), (0, 0.0))]
    if name == "equal_candidates":    # frames 0 and 1 are the same frame; frame 2 gates both
        return [frame(*scatter_scene(11, proj_r=4.0, drop=d), 0.0, x) for d, x in ((0.0, 0.0), (0.0, 0.0), (0.1, 21.0))]
    if name == "strict":
        return [frame(*scatter_scene(s, proj_r=4.0, drop=d), 0.0, x) for s, d, x in ((12, 0.0, 0.0), (13, 0.0, 21.0), (13, 0.1, 42.0))]
    if name == "no_shift":
        sem, corner, surf = scatter_scene(14, proj_r=None)
        return [frame(sem + many_projected(100001), corner, surf, 0.5, 0.0), frame(*scatter_scene(15, proj_r=None), 0.2, 21.0)]
    if name == "empty_sector_clouds":
        return [frame(*scatter_scene(16 + j, proj_r=p), yaw, x) for j, (p, yaw, x) in enumerate(((2.0, 0.0, 0.0), (None, 0.3, 21.0), (2.0, 0.1, 0.0)))]
    if name == "empty_descriptors":
        return [frame(*outside_scene(20), 0.0, 0.0), frame(*outside_scene(21), 0.1, 21.0), frame(*scatter_scene(22), 0.0, 0.0),
                frame(*outside_scene(23), 0.2, 21.0)]
    if name == "ssc_order0":
        return [frame(*scatter_scene(24 + j, proj_r=None, labels=(1, 5, 8, 20, 33, 59)), 0.0, x) for j, x in enumerate((0.0, 21.0))]
    raise KeyError(name)


CASES = {"drive": (DEFAULT, 0.5),            # this drive's SSC scores are ~0.4 - 0.65: below the default 0.79 nothing would be selected
         "all_tie": (DEFAULT, K.LABEL_THRESHOLD), "periodic": (DEFAULT, K.LABEL_THRESHOLD), "shifted": (DEFAULT, K.LABEL_THRESHOLD),
         "equal_candidates": (DEFAULT, K.LABEL_THRESHOLD), "strict": (GATE_ALL, 0.5), "no_shift": (DEFAULT, K.LABEL_THRESHOLD),
         "empty_sector_clouds": (DEFAULT, K.LABEL_THRESHOLD), "empty_descriptors": (DEFAULT, K.LABEL_THRESHOLD),
         "ssc_order0": (DEFAULT, K.LABEL_THRESHOLD)}
CRAFTED = [n for n in CASES if n != "drive"]
_FRAMES, _REF = {}, {}


def case_frames(name):
    if name not in _FRAMES:
        _FRAMES[name] = _case_frames(name)
    return _FRAMES[name]


# ---- the restatement alone -------------------------------------------------------------------------------------------------------

def select(cands, thr, label_thr):
    """[(kind, history_id, score)] in push order from [(history_id, score[7])] in candidate order: per kind the first strict maximum
    above its threshold, for Pose the first strict minimum below 1000000 (compared with EPSCGenerationKinds' own matched list on
    every case by test_selection_glue_equals_the_restatement)."""
    out = []
    for kind in range(7):
        best, at = (1000000.0 if kind == K.POSE else 0.0), -1
        for h, s in cands:
            v = float(s[kind])
            if (v < best) if kind == K.POSE else (v > (label_thr if kind == K.SSC else thr) and v > best):
                best, at = v, h
        if at >= 0:
            out.append((kind, at, best))
    return out


def record(k, h, yaw_diff, g, proj_h, proj_k, stored, D, score, shift, pos_distance):
    return dict(frame=k, hist=h, yaw_diff=yaw_diff, tmp_id=R.wrap_yaw(yaw_diff)[1], icp=g, proj_h=proj_h, proj_k=proj_k, stored=stored,
                D=D, score=score, shift=shift, pos_distance=pos_distance)


def reference(name, oracle, params=None, label_thr=None):
    """the restatement's run of a case: dict(E, out, records, matches = per frame [(kind, history_id, score)]); cached per argument set."""
    key = (name, params, label_thr)
    if key in _REF:
        return _REF[key]
    p0, l0 = CASES[name]
    params, label_thr = params or p0, l0 if label_thr is None else label_thr
    frames = case_frames(name)
    E = K.EPSCGenerationKinds(oracle, K.ALL, params, label_thr)
    out = [E.loop_detection(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames]
    recs = []
    for k, (f, o) in enumerate(zip(frames, out)):
        for c in o["candidates"]:
            h = c["history_id"]
            score = dict(c["score"]); score[K.POSE] = c["pos_distance"]
            recs.append(record(k, h, np.float32(E.yaw[k] - E.yaw[h]), c["g"], E.proj[h], E.proj[k], {kk: E.db[kk][h] for kk in range(6)},
                               K.all_descriptors(f["corner"], f["surf"], f["semantic"], c["T"]), score, c["shift"], c["pos_distance"]))
    _REF[key] = dict(E=E, out=out, records=recs, params=params, label_thr=label_thr,
                     matches=[[(m[0], m[1], m[3]) for m in o["matches"]] for o in out])
    return _REF[key]


class OneUlpNumpy:
    """numpy with an arctan2 one float32 ulp off (up or down): what an atan2f of another library may return."""
    def __init__(self, up):
        self._to = np.float32(np.inf if up else -np.inf)

    def __getattr__(self, name):
        return getattr(np, name)

    def arctan2(self, y, x):
        return np.nextafter(np.arctan2(y, x), self._to)


# ---- the forced check ------------------------------------------------------------------------------------------------------------

def forced_check(ctx, oracle, name, db_id, params=None, label_thr=None):
    """run the case on the device and check every stage against the restatement applied to the device's input to that stage.  Returns
    dict(records (the reference-side values, which the device equals), matches, n_cand, selected[7], rot (largest difference of a
    matched rotation entry))."""
    import lisreg
    ref = reference(name, oracle, params, label_thr)
    E, params, label_thr = ref["E"], ref["params"], ref["label_thr"]
    frames = case_frames(name)
    ctx.loopdet_reset(db_id)
    ctx.loopdet_configure(K.ALL, db_id=db_id, label_threshold=label_thr)
    got = ctx.loopdet_detect([(f["corner"], f["surf"], f["semantic"], f["odom"]) for f in frames], db_id=db_id, params=lisreg.LoopdetParams(*params))
    proj = [ctx.loopdet_get(k, db_id=db_id)[1] for k in range(len(frames))]
    stored = [{kk: ctx.loopdet_get_descriptor(k, 1 << kk, db_id=db_id) for kk in range(6)} for k in range(len(frames))]
    recs, matches, rot, selected = [], [], 0.0, np.zeros(7, int)
    for k, (f, o, g) in enumerate(zip(frames, ref["out"], got)):
        assert np.array_equal(ctx.loopdet_get(k, db_id=db_id)[0], stored[k][K.FEPSC]), k
        cands, cs = ctx.loopdet_candidates(k, db_id=db_id), ctx.loopdet_candidate_scores(k, db_id=db_id)
        # gate
        gated = [c["history_id"] for c in o["candidates"]]
        assert [c["history_id"] for c in cands] == gated and [c["history_id"] for c in cs] == gated, (name, k)
        assert g["current_frame_id"] == k and g["n_candidates"] == len(gated), (name, k)
        by_hist = {}
        for c, s, rc in zip(cands, cs, o["candidates"]):
            h, at = c["history_id"], (name, k, c["history_id"])
            assert s["score"][K.POSE] == rc["pos_distance"], at
            # yaw search and ICP on the stored projections
            yaw_diff = np.float32(E.yaw[k] - E.yaw[h])
            gi = R.global_icp(proj[h], proj[k], yaw_diff, oracle)
            assert c["yaw_shift"] == gi["shift"], (at, c["yaw_shift"], gi["shift"])
            assert bits(c["yaw_angle"]) == bits(gi["angle"]), (at, c["yaw_angle"], gi["angle"])
            assert (c["icp_state"], c["icp_iters"], c["icp_n_corr"]) == (gi["state"], gi["iters"], gi["n_corr"]), (at, c, gi)
            T = c["transform"]
            assert np.abs(T - gi["T"]).max() <= 1e-3, (at, T, gi["T"])
            # the pair's descriptors under the device's own transform
            D = {kk: ctx.loop_descriptor_kind(1 << kk, f["corner"], f["surf"], f["semantic"], M=T) for kk in range(6)}
            refD = K.all_descriptors(f["corner"], f["surf"], f["semantic"], T)
            for kk in range(6):
                assert np.count_nonzero(D[kk] != refD[kk]) <= EDGE_CAP, (at, K.NAMES[kk], np.count_nonzero(D[kk] != refD[kk]))
            # scores
            score, shift = {K.POSE: rc["pos_distance"]}, {}
            for kk in DIST_KINDS:
                score[kk], shift[kk] = R.distance(stored[h][kk], D[kk])
                assert bits(score[kk]) == bits(s["score"][kk]) and shift[kk] == s["shift"][kk], \
                    (at, K.NAMES[kk], score[kk], shift[kk], s["score"][kk], s["shift"][kk])
            score[K.SSC], shift[K.SSC] = K.label_sim(stored[h][K.SSC], D[K.SSC]), 0
            assert same_double(score[K.SSC], s["score"][K.SSC]) and s["shift"][K.SSC] == 0, (at, score[K.SSC], s["score"][K.SSC])
            assert bits(c["score"]) == bits(score[K.FEPSC]) and c["score_shift"] == shift[K.FEPSC], at
            by_hist[h] = (T, yaw_diff, D)
            recs.append(record(k, h, yaw_diff, gi, proj[h], proj[k], stored[h], D, score, shift, rc["pos_distance"]))
        # selection, from the device's own scores
        want = select([(s["history_id"], s["score"]) for s in cs], params[2], label_thr)
        ms = ctx.loopdet_matches(k, db_id=db_id)
        assert [(m["kind"].bit_length() - 1, m["history_id"]) for m in ms] == [(w[0], w[1]) for w in want], (name, k, ms, want)
        for m, (kk, h, sc) in zip(ms, want):
            at = (name, k, K.NAMES[kk], h)
            assert m["kind"] == 1 << kk and bits(m["score"]) == bits(sc), at
            T, yaw_diff, D = by_hist[h]
            M = m["transform"]
            assert M[0, 3] == T[0, 3] and M[1, 3] == T[1, 3], at
            if kk in (K.SSC, K.POSE):
                assert np.array_equal(M, T), at
            else:
                angle = R.atan2f(T[1, 0], T[0, 0])
                if kk != K.FEPSC:
                    angle = K.distance_angle(stored[h][kk], D[kk], float(yaw_diff) if kk == K.EPSC else float(angle))[2]
                want_M = K.planar(T, angle)
                d = float(np.abs(M - want_M).max())
                rot = max(rot, d)
                assert d <= ROT_BOUND, (at, d, M, want_M)
            selected[kk] += 1
        fe = {m["kind"]: m for m in ms}.get(1 << K.FEPSC)
        assert g["matched_frame_id"] == (fe["history_id"] if fe else -1), (name, k)
        if fe:
            assert np.array_equal(g["matched_transform"], fe["transform"]) and bits(g["score"]) == bits(fe["score"]), (name, k)
        else:
            assert g["score"] == 0.0 and np.array_equal(g["matched_transform"], np.eye(4, dtype=np.float32)), (name, k)
        matches.append(want)
    return dict(records=recs, matches=matches, n_cand=len(recs), selected=selected, rot=rot)


# ---- what each case exists for: asserted on reference-side records (the restatement's own, or the forced check's) -----------------

def uniform(d):
    return bool((d == d[:, :1]).all())


def period_of(d, axis):
    """the smallest roll along axis that maps d onto itself."""
    n = d.shape[axis]
    return next(p for p in range(1, n + 1) if n % p == 0 and np.array_equal(d, np.roll(d, p, axis=axis)))


def pairs_of(run):
    return {(r["frame"], r["hist"]): r for r in run["records"]}


def check_icp_decisive(run):
    """the crafted frames' ICPs end at their first step (see projected()) or have no correspondences: nothing rounding decides."""
    for r in run["records"]:
        assert (r["icp"]["state"], r["icp"]["iters"]) in ((2, 1), (5, 0)), (r["frame"], r["hist"], r["icp"])


def check_drive(run):
    recs = run["records"]
    assert len(recs) >= 40, len(recs)
    assert any(r["yaw_diff"] < 0 and r["tmp_id"] > 331 for r in recs)                  # the modulo-360 columns
    assert any(abs(float(r["yaw_diff"])) > math.pi for r in recs)
    sel = np.bincount([m[0] for ms in run["matches"] for m in ms], minlength=7)
    assert all(sel[:6] >= 10), sel


def check_all_tie(run):
    recs = run["records"]
    assert len(recs) == 2
    for r in recs:
        assert uniform(r["proj_h"][:, :1].T) and uniform(r["proj_k"][:, :1].T) and r["proj_h"][0, 0] == 2        # 60 equal sums
        assert r["tmp_id"] == 0 and r["icp"]["shift"] == -30 and r["icp"]["n_corr"] == R.PROJ
        for kk in DIST_KINDS:
            assert uniform(r["stored"][kk]) and uniform(r["D"][kk]) and r["stored"][kk].any(), K.NAMES[kk]          # 20 equal sums
            assert (r["score"][kk], r["shift"][kk]) == (1.0, -10), K.NAMES[kk]
        assert r["score"][K.SSC] == 1.0
    assert all(sorted(m[0] for m in ms) == list(range(7)) for ms in run["matches"][1:])


def check_periodic(run):
    recs = run["records"]
    assert [(r["frame"], r["hist"]) for r in recs] == [(1, 0), (2, 1)]
    for r, first in zip(recs, (0, 18)):
        assert period_of(r["proj_h"][:, 0], 0) == 18 and np.array_equal(r["proj_h"][:, 0], r["proj_k"][:, 0])
        lo, hi = r["tmp_id"] - 30, r["tmp_id"] + 30
        ties = [i for i in range(lo, hi) if i % 18 == 0]
        assert len(ties) >= 3 and ties[0] == first == r["icp"]["shift"], (ties, r["icp"]["shift"])
        for kk in DIST_KINDS:
            assert period_of(r["stored"][kk], 1) == 4 and np.array_equal(r["stored"][kk], r["D"][kk]), K.NAMES[kk]
            assert (r["score"][kk], r["shift"][kk]) == (1.0, -8), K.NAMES[kk]                    # -8, -4, 0, 4, 8 tie: the first wins


def check_shifted(run):
    p = pairs_of(run)
    for key, want in (((1, 0), 3), ((2, 1), -3)):
        r = p[key]
        assert r["icp"]["shift"] == 0
        for kk in DIST_KINDS:
            assert np.array_equal(np.roll(r["stored"][kk], want, axis=1), r["D"][kk]) and period_of(r["D"][kk], 1) == R.SECTORS
            assert (r["score"][kk], r["shift"][kk]) == (1.0, want), (K.NAMES[kk], r["score"][kk], r["shift"][kk])
        assert r["stored"][K.EPSC][:, -3:].any() and r["stored"][K.EPSC][:, :3].any()              # both wraps carry content


def check_equal_candidates(run):
    p = pairs_of(run)
    assert sorted(p) == [(2, 0), (2, 1)]
    a, b = p[(2, 0)], p[(2, 1)]
    for kk in range(7):
        assert bits(a["score"][kk]) == bits(b["score"][kk]), K.NAMES[kk]
        assert a["score"][kk] < 1.0 or kk == K.POSE
    assert a["pos_distance"] == b["pos_distance"] == 0.0
    assert run["matches"][2] == [(kk, 0, a["score"][kk]) for kk in range(7)], run["matches"][2]


def check_no_shift(run):
    (r,) = run["records"]
    assert r["proj_h"][:, 0].sum() == 100001 and not r["proj_k"].any()
    assert r["yaw_diff"] < 0 and r["icp"]["shift"] == R.NO_SHIFT
    assert r["icp"]["angle"] == np.float32(R.wrap_yaw(r["yaw_diff"])[0] * R.STEP360)
    assert (r["icp"]["state"], r["icp"]["iters"], r["icp"]["n_corr"]) == (5, 0, 0)
    assert np.array_equal(r["icp"]["T"], R.rot_z(r["icp"]["angle"]))


def check_empty_sector_clouds(run):
    p = pairs_of(run)
    cur, hist = p[(1, 0)], p[(2, 1)]
    assert (cur["proj_h"][:, 3] > 0).any() and not (cur["proj_k"][:, 3] > 0).any()
    assert (hist["proj_k"][:, 3] > 0).any() and not (hist["proj_h"][:, 3] > 0).any()
    assert hist["yaw_diff"] < 0
    for r in (cur, hist):
        assert r["icp"]["shift"] == r["tmp_id"] - 30                    # sixty equal sums below 100000: the first shift
        assert (r["icp"]["state"], r["icp"]["iters"], r["icp"]["n_corr"]) == (5, 0, 0)
        assert np.array_equal(r["icp"]["T"], R.rot_z(r["icp"]["angle"]))


def check_empty_descriptors(run):
    p = pairs_of(run)
    both, hist, cur = p[(1, 0)], p[(2, 1)], p[(3, 2)]
    assert both["icp"]["n_corr"] > 0
    for kk in range(6):
        assert not both["stored"][kk].any() and not both["D"][kk].any() and not hist["stored"][kk].any() and not cur["D"][kk].any()
        assert hist["D"][kk].any() and cur["stored"][kk].any(), K.NAMES[kk]
    for kk in DIST_KINDS:
        assert (both["score"][kk], both["shift"][kk]) == (1.0, -10)
        assert hist["shift"][kk] == cur["shift"][kk] == -10 and hist["score"][kk] < 1.0 and cur["score"][kk] < 1.0
    assert math.isnan(both["score"][K.SSC]) and hist["score"][K.SSC] == 0.0 and cur["score"][K.SSC] == 0.0
    assert [m[0] for m in run["matches"][1]] == [K.ISC, K.SC, K.EPSC, K.SEPSC, K.FEPSC, K.POSE]
    assert K.SSC not in [m[0] for ms in run["matches"] for m in ms]


def check_ssc_order0(run):
    (r,) = run["records"]
    assert not r["stored"][K.SSC].any() and not r["D"][K.SSC].any() and math.isnan(r["score"][K.SSC])
    for kk in (K.ISC, K.SC, K.EPSC):
        assert r["stored"][kk].any() and r["D"][kk].any()
    assert K.SSC not in [m[0] for m in run["matches"][1]] and K.EPSC in [m[0] for m in run["matches"][1]]


def check_strict(run):
    p = pairs_of(run)
    assert sorted(p) == [(1, 0), (2, 0), (2, 1)]


def _crafted(check):
    def both(run):
        check_icp_decisive(run)
        check(run)
    return both


CHECKS = {"drive": check_drive, "all_tie": _crafted(check_all_tie), "periodic": _crafted(check_periodic), "shifted": _crafted(check_shifted),
          "equal_candidates": _crafted(check_equal_candidates), "strict": _crafted(check_strict), "no_shift": _crafted(check_no_shift),
          "empty_sector_clouds": _crafted(check_empty_sector_clouds), "empty_descriptors": _crafted(check_empty_descriptors),
          "ssc_order0": _crafted(check_ssc_order0)}


def best_of(run, frame_id, kind):
    """the largest score of a kind among a frame's candidates, and its history id (the first of equals)."""
    c = [(r["hist"], r["score"][kind]) for r in run["records"] if r["frame"] == frame_id]
    s = max(v for _, v in c)
    return s, next(h for h, v in c if v == s)


def strict_runs(run_with):
    """threshold strictness: run_with(params, label_thr) -> a run.  The best FEPSC and SSC scores of frame 2 become the thresholds:
    not selected at the score itself, selected one ulp below it."""
    base = run_with(None, None)
    CHECKS["strict"](base)
    (s, h), (l, hl) = best_of(base, 2, K.FEPSC), best_of(base, 2, K.SSC)
    assert 0.75 < s < 1.0 and 0.5 < l < 1.0, (s, l)
    assert (K.FEPSC, h, s) in base["matches"][2] and (K.SSC, hl, l) in base["matches"][2]
    at = run_with((GATE_ALL[0], GATE_ALL[1], s), l)
    kinds = [m[0] for m in at["matches"][2]]
    assert K.FEPSC not in kinds and K.SSC not in kinds, at["matches"][2]
    below = run_with((GATE_ALL[0], GATE_ALL[1], float(np.nextafter(s, 0))), float(np.nextafter(l, 0)))
    assert (K.FEPSC, h, s) in below["matches"][2] and (K.SSC, hl, l) in below["matches"][2], below["matches"][2]
    for r in (at, below):                                   # the thresholds change the selection, nothing before it
        assert [(x["frame"], x["hist"]) for x in r["records"]] == [(x["frame"], x["hist"]) for x in base["records"]]
        assert all(bits(a["score"][kk]) == bits(b["score"][kk]) for a, b in zip(r["records"], base["records"]) for kk in DIST_KINDS)
