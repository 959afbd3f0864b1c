"""The normal equations of the correspondence kernel per workgroup, in the PRODUCTION arithmetic (`row_and_reduce`,
csrc/lisreg_assoc.hip: Jacobian row from the coefficients, the untransformed source point and ItemState::jk; the 28 terms in float32; the
float32 halving butterfly; the four wave sums in fp64; one partial row per block descriptor).

lisreg_get_partial_rows hands back the partial rows, the block table and — with eight lanes per query — the kernel's own coefficients
and accept flags.  tests/normal_rows_ref.py forms the same rows in float64 from those coefficients with math.fsum; what is left between
the two is a few dozen float32 roundings, bounded by counting them (C_ROUND = 50, that module's docstring).  The planted batch decides by
POSITION in the segment which queries are accepted, so that single lanes, lane pairs across every butterfly level, tail wavefronts and
all-rejected blocks each stand alone in a workgroup; the CPU census shows that losing a row, adding a rejected query's row, moving a row
to the neighbouring block or swapping value index k with k + 16 each exceed the budget a hundred times over.

Two limits of the inputs, both forced: the segment sizes 1, 63, 64, 65, 255, 256, 257 and 513 for both kinds add up to 2 948 queries,
so the batch has 3 076 (it runs in milliseconds); and a batch's "trace_cap" records have no reader
(tests/test_option_state.py), so the trace leg reads the trace of every item registered ALONE (lisreg_align) and holds it against the
rows the batch left for that item, which are the same workgroups."""
import ctypes as C

import numpy as np
import pytest

import normal_rows_ref as N

f32, f64 = np.float32, np.float64
BIG = 1 << 30
SEED = 0


def _batch():
    return N.planted_batch(SEED)


_MODELS = {}


def _models(labelled=False):
    if labelled not in _MODELS:
        score = None
        if labelled:
            import lisreg
            score = np.array(list(lisreg.default_params(2).label_score), f32)
        _MODELS[labelled] = N.models(_batch(), score)
    return _MODELS[labelled]


# ---------------------------------------------------------------- CPU
def test_batch_has_the_planted_properties():
    b = _batch()
    segs = b["segments"]
    for kind in (0, 1):
        assert set(N.SIZES) <= {s["n"] for s in segs if s["kind"] == kind}
    assert {s["pattern"] for s in segs} == set(N.PATTERNS)
    assert len(b["items"]) >= 8 and b["n_elems"] == sum(s["n"] for s in segs) == 3076
    assert sum(len(t) for it in b["items"] for t in it["tgt"]) <= 4000
    names = [it["name"] for it in b["items"]]
    i = names.index("loud")
    assert b["items"][i - 1]["spec"]["where"] == "quiet" and b["items"][i + 1]["spec"]["where"] == "quiet"
    for it in b["items"]:
        top = max(float(np.abs(s[:, :3]).max()) for s in it["src"] if len(s))
        if it["spec"]["where"] == "quiet":
            assert top < 2.0, (it["name"], top)
        if it["spec"]["where"] == "loud":
            assert min(float(np.abs(s[:, :3]).min()) for s in it["src"]) > 50.0 and top < 80.0
        ang = np.abs(it["T"][:3])
        assert (ang == 0).all() if it["name"] == "level" else ((ang >= 0.2) & (ang <= 1.2)).all(), it["name"]
        assert np.abs(it["T"][3:]).max() >= 1.0
    assert len(b["items"][names.index("no_corner")]["src"][0]) == 0
    assert len(b["items"][names.index("four_point_surf_target")]["tgt"][1]) == 4
    kinds = np.concatenate([s["planted"] for s in segs])
    for k in N.KINDS_REJECTED:
        assert (kinds == k).sum() >= 50, k
    # labels 0-19, 20-31, >= 32, every payload with high bits of its own
    bits = np.concatenate([s["src"][:, 3].copy().view(np.uint32) for s in segs])
    lab = bits & 0xffff
    assert set(range(20)) <= set(lab.tolist()) and ((lab >= 20) & (lab < 32)).any() and (lab >= 32).any() and np.all(bits >> 16 != 0)
    assert np.isfinite(np.concatenate([s["src"][:, 3] for s in segs])).all()


def test_margins_hold_for_every_query():
    N.check_margins(_batch(), _models())
    N.check_margins(_batch(), _models(labelled=True))                     # (the weights scale the coefficients, no decision)
    w = np.concatenate([r["w"] for r in _models(labelled=True)])
    assert len(np.unique(w)) >= 8 and w.min() > 0


def lanes_by_block(blocks, flags):
    """per block: the (wavefront, lane) pairs of its accepted queries"""
    out = []
    for _, _, first, count in blocks:
        tid = np.flatnonzero(np.asarray(flags[first:first + count]) != 0)
        out.append([(int(t) >> 6, int(t) & 63) for t in tid])
    return out


def check_patterns(batch, blocks, flags):
    """the planted patterns land on the lanes they are named for — from a block table and accept flags (the plan's and the models' on the
    CPU, the device's on the GPU)"""
    per_block = lanes_by_block(blocks, flags)
    seen = set()
    for sg in batch["segments"]:
        mine = [(b, per_block[i]) for i, b in enumerate(blocks) if sg["base"] <= b[2] < sg["base"] + sg["n"]]
        assert sum(b[3] for b, _ in mine) == sg["n"] and all(b[0] == sg["item"] and b[1] == sg["kind"] for b, _ in mine)
        assert all((b[2] - sg["base"]) % 256 == 0 for b, _ in mine)
        pat = sg["pattern"]
        if sg["kind"] == 1 and batch["items"][sg["item"]]["spec"].get("short_surf"):
            pat = "none"
        lanes = [wl for _, l in mine for wl in l]
        only = lambda allowed: all(l in allowed for _, l in lanes)
        if pat == "all":
            assert all(len(l) == b[3] for b, l in mine)
        elif pat == "none":
            assert not lanes
        elif pat == "lane0":
            assert lanes and only((0,))
        elif pat == "lane63":
            assert lanes and only((63,))
        elif pat == "lanes31_32":
            assert {l for _, l in lanes} == {31, 32} and only((31, 32))
        elif pat == "lanes15_16":
            assert {l for _, l in lanes} == {15, 16} and only((15, 16))
        elif pat == "one_per_wave":
            waves = [[w for w, _ in l] for _, l in mine]
            assert all(sorted(w) == list(range((b[3] + 63) // 64)) for (b, _), w in zip(mine, waves))
            assert len({l for _, l in lanes}) >= min(4, len(lanes))
        elif pat == "last_of_tail":
            (b, l), = [m for m in mine if m[1]]
            assert b is mine[-1][0] and b[3] < 256 and l == [((b[3] - 1) >> 6, (b[3] - 1) & 63)]
        elif pat == "alternating":
            assert all(l == [(t >> 6, t & 63) for t in range(0, b[3], 2)] for b, l in mine)
        seen.add(pat)
    assert seen == set(N.PATTERNS)
    # blocks with nothing accepted, a single accepted lane, and a tail block of one query all occur
    assert any(not l for l in per_block) and any(len(l) == 1 for l in per_block) and any(b[3] == 1 for b in blocks)


def test_patterns_land_on_the_claimed_lanes():
    b = _batch()
    check_patterns(b, N.plan_blocks(b), N.flat(b, _models(), "ok"))


def test_mutation_census():
    assert N.C_ROUND <= 64                                                # (a larger count of roundings would be a miscount: normal_rows_ref)
    for labelled in (False, True):
        worst = N.census(_batch(), _models(labelled))
        print("census, smallest move / budget per mutation:", {k: round(v, 1) for k, v in worst.items()})
        assert all(v > 100.0 for v in worst.values())


def test_reference_rows_against_a_plain_restatement():
    """rows_from_coefficients against J^T J of the rotation's analytic derivative — another route to the same numbers: the row is the
    gradient of n . (R(T) p + t) with respect to (roll, pitch, yaw, x, y, z), by central differences of the float64 pose matrix"""
    rng = np.random.default_rng(3)
    T = np.array([0.4, -0.7, 1.1, 1.0, 2.0, -3.0], f32)
    src = rng.uniform(-5, 5, (40, 3)).astype(f32)
    cf = rng.uniform(-1, 1, (40, 4)).astype(f32)
    terms, mags = N.rows_from_coefficients(T, src, cf, np.ones(40, bool))
    h = 1e-6
    J = np.zeros((40, 6))
    for k in range(6):
        d = np.zeros(6); d[k] = h
        qp, qm = _to_map64(T.astype(f64) + d, src), _to_map64(T.astype(f64) - d, src)
        J[:, k] = ((qp - qm) / (2 * h) * cf[:, :3].astype(f64)).sum(1)
    want = J[:, [0, 1, 2, 3, 4, 5]]
    got = np.stack([terms[:, 21 + k] / -cf[:, 3].astype(f64) for k in range(6)], 1)          # row = (row * b) / b
    assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max()
    assert np.all(mags >= np.abs(terms) * (1 - 1e-12)) and np.all(terms[:, 27] == 1)
    for k in range(21):
        assert np.allclose(terms[:, k], got[:, N.TRI_R[k]] * got[:, N.TRI_C[k]], rtol=1e-9, atol=1e-12)
    none, _ = N.rows_from_coefficients(T, src, np.full((40, 4), np.nan, f32), np.zeros(40, bool))
    assert not none.any()


def _to_map64(T, src):
    import math
    A, B, Cc, D, E, F = math.cos(T[2]), math.sin(T[2]), math.cos(T[1]), math.sin(T[1]), math.cos(T[0]), math.sin(T[0])
    R = np.array([[A * Cc, A * D * F - B * E, B * F + A * D * E], [B * Cc, A * E + B * D * F, B * D * E - A * F], [-D, Cc * F, Cc * E]])
    return src.astype(f64) @ R.T + T[3:6]


# ---------------------------------------------------------------- GPU
def _params(variant=1, fixed_iters=1, min_corr=BIG):
    import lisreg
    p = lisreg.default_params(variant)
    p.knn_sq_thresh = N.TAU; p.fixed_iters = fixed_iters
    p.edge_min = -1; p.surf_min = -1                                   # the feature-count guard passes whatever the query count
    p.min_corr = min_corr                                              # 2^30: no step is ever solved, the pose stays T_init
    return p


BASE_OPTS = (("dump_neighbors", 1), ("canonical_ties", 1), ("sort_sources", 0))


class Prepared:
    """one context with the planted batch's targets in slots 0 .. and its sources as device records"""

    def __init__(self, mode=1, lanes=0, opts=()):
        import lisreg
        from lisreg import synth
        self.b = _batch()
        self.ctx = lisreg.Context(0)
        self.keep = []
        for k, v in (("search_mode", mode), ("lanes_per_query", lanes)) + BASE_OPTS + tuple(opts):
            self.ctx.set_option(k, v)
        self.items = []
        for i, it in enumerate(self.b["items"]):
            self.ctx.set_target(synth.to_pcl(it["tgt"][0]), synth.to_pcl(it["tgt"][1]), slot=i)
            a, s = lisreg.DeviceArray(it["src"][0]), lisreg.DeviceArray(it["src"][1])
            self.keep += [a, s]
            self.items.append(dict(corner_ptr=a.ptr, n_corner=len(it["src"][0]), surf_ptr=s.ptr, n_surf=len(it["src"][1]), target=i))
        self.T0 = np.array([it["T"] for it in self.b["items"]], f32)

    def run(self, variant=1, fixed_iters=1, min_corr=BIG, opts=()):
        ctx, n = self.ctx, self.b["n_elems"]
        for k, v in opts:
            ctx.set_option(k, v)
        ctx.batch_prepare_device(self.items, self.T0, _params(variant, fixed_iters, min_corr))
        ctx.batch_run()
        T, st = ctx.batch_fetch()
        if min_corr == BIG:                                            # frozen pose: nothing solved, every iteration ran
            assert np.array_equal(T, self.T0) and all(s["iters"] == fixed_iters for s in st), st
        lanes = ctx.get_option("lanes_per_query")
        out = ctx.partial_rows(n if lanes == 8 else None)
        if lanes == 8:
            # the queries of a segment whose target has fewer than five points: the kernel never writes their coefficients and the hook
            # hands back what the buffers held (include/lisreg.h: unspecified).  Such a query is accepted by nobody: masked to "rejected".
            for sg in self.b["segments"]:
                if len(self.b["items"][sg["item"]]["tgt"][sg["kind"]]) < 5:
                    out["coef"][sg["base"]:sg["base"] + sg["n"]] = 0
                    out["coef_ok"][sg["base"]:sg["base"] + sg["n"]] = 0
        out.update(nb=ctx.neighbors(n), T=T, st=st, front=ctx.front_end(), lanes=lanes)
        return out

    def close(self):
        self.ctx.close()
        for a in self.keep:
            a.free()


def _run(mode=1, lanes=0, opts=(), **kw):
    p = Prepared(mode, lanes, opts)
    try:
        return p.run(**kw)
    finally:
        p.close()


@pytest.fixture(scope="module")
def leg1():
    """eight lanes per query, fixed_iters = 1: computed once, shared, never written to"""
    out = _run()
    assert out["front"] == 1 and out["lanes"] == 8
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == f64 else np.uint32)


def check_rows(batch, out, mods, what):
    """leg 1's assertions on one dump with coefficients; returns the worst |device - fsum| / budget"""
    blocks, rows, coef, ok = out["blocks"], out["rows"], out["coef"], out["coef_ok"]
    assert np.array_equal(blocks, N.plan_blocks(batch)), what
    assert set(np.unique(ok)) <= {0, 1}
    want = N.flat(batch, mods, "ok")
    bad = np.flatnonzero((ok == 1) != want)
    assert bad.size == 0, (what, "coef_ok against the float64 models", bad[:8])
    assert np.array_equal(ok == 1, out["nb"][5] == 1), (what, "coef_ok against row 5 of lisreg_get_neighbors")
    check_patterns(batch, blocks, ok)
    # the device's five neighbours are the patch the query was planted on
    idx = np.concatenate([r["idx"] for r in mods])
    found = N.flat(batch, mods, "found")
    assert np.array_equal(np.sort(out["nb"][:5, found].T, 1), np.sort(idx[found], 1)) and np.all(out["nb"][4, ~found] == -1), what
    terms, mags = N.terms_of_batch(batch, coef, ok)
    S, A = N.block_sums(blocks, terms, mags)
    count = np.array([ok[f:f + c].sum() for _, _, f, c in blocks])
    assert np.array_equal(rows[:, 27], count.astype(f64)), (what, "counts")
    empty = count == 0
    assert empty.sum() >= 4 and not bits(rows[empty]).any(), (what, "all-rejected blocks are 28 x +0.0")
    bud = N.budget(A)
    err = np.abs(rows - S)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / bud, 0.0)
    worst = float(ratio.max())
    b_, k_ = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{what}: worst |device - fsum| / budget = {worst:.4f} (block {b_} {tuple(blocks[b_])}, entry {k_}; budget = {N.C_ROUND} * 2^-24 * A); "
          f"{int((~empty).sum())} blocks with rows, {int(empty.sum())} without")
    assert worst < 1.0, (what, worst, int(b_), int(k_), rows[b_, k_], S[b_, k_], bud[b_, k_])
    return worst


def test_check_rows_rejects_what_it_must(capsys):
    """the GPU assertion itself, on a dump made on the CPU: the reference's own rows pass (also rounded to float32 and back, a relative
    error of 2^-24 per entry); a lost row, a rejected query's row added, a row moved to the neighbouring block, two value indices
    swapped, a count off by one, a count entry right with its row missing and a -0.0 in an all-rejected block all fail"""
    b, mods = _batch(), _models()
    ok = N.flat(b, mods, "ok").astype(np.int32)
    cf = np.concatenate([r["cf"] for r in mods])
    idx = np.concatenate([r["idx"] for r in mods])
    found = N.flat(b, mods, "found")
    d5 = np.concatenate([r["d5"] for r in mods])
    nb = np.full((6, b["n_elems"]), -1, np.int32)
    nb[:5, found] = idx[found].T
    nb[5] = ok
    blocks = N.plan_blocks(b)
    terms, mags = N.terms_of_batch(b, cf, ok)
    would, _ = N.terms_of_batch(b, cf, found)
    S, _ = N.block_sums(blocks, terms, mags)
    good = dict(blocks=blocks, rows=S, coef=cf, coef_ok=ok, nb=nb)
    assert d5[found].max() <= 0.5
    assert check_rows(b, good, mods, "the reference's own rows") == 0.0
    assert check_rows(b, dict(good, rows=S.astype(f32).astype(f64)), mods, "rounded to float32") <= 1.0 / N.C_ROUND

    def rejected(rows):
        try:
            check_rows(b, dict(good, rows=rows), mods, "mutant")
        except AssertionError:
            return True
        return False
    full = int(np.argmax(blocks[:, 3] * (S[:, 27] == blocks[:, 3])))          # a block with every query accepted (the hardest to move)
    assert S[full, 27] == 256
    q = int(blocks[full, 2]) + 77
    lost = S.copy(); lost[full] -= terms[q]
    assert rejected(lost)
    kept_count = lost.copy(); kept_count[full, 27] = S[full, 27]
    assert rejected(kept_count)
    mixed = next(i for i, (_, _, f, c) in enumerate(blocks) if 0 < S[i, 27] and (found[f:f + c] & (ok[f:f + c] == 0)).any())
    f, c = blocks[mixed, 2:]
    r = int(f) + int(np.flatnonzero(found[f:f + c] & (ok[f:f + c] == 0))[0])
    added = S.copy(); added[mixed, :27] += would[r, :27]
    assert rejected(added)
    moved = S.copy(); moved[full] -= terms[q]; moved[full + 1] += terms[q]
    assert rejected(moved)
    for k in range(12):
        swapped = S.copy(); swapped[full, [k, k + 16]] = swapped[full, [k + 16, k]]
        assert rejected(swapped), k
    off = S.copy(); off[full, 27] += 1
    assert rejected(off)
    empty = int(np.flatnonzero(S[:, 27] == 0)[0])
    neg = S.copy(); neg[empty, 3] = -0.0
    assert rejected(neg)
    capsys.readouterr()


@pytest.mark.gpu
def test_hip_rows_match_fsum_of_the_kernels_own_coefficients(leg1):
    check_rows(_batch(), leg1, _models(), "eight lanes per query, fixed_iters 1")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [2, 3])
def test_hip_rows_with_label_weights(leg1, variant):
    """the labelled leg: w = 2 - LabelSorce[label] differs per query (labels 0-19, 20-31, >= 32 under high payload bits)"""
    b = _batch()
    out = _run(variant=variant)
    assert out["lanes"] == 8
    check_rows(b, out, _models(labelled=True), f"variant {variant} (label weights)")
    # coefficient = (w * s) * model against s * model in float32: the quotient is w within three roundings
    w = np.concatenate([r["w"] for r in _models(labelled=True)])
    acc = leg1["coef_ok"] == 1
    big = acc[:, None] & (np.abs(leg1["coef"]) > 1e-3)
    q = out["coef"].astype(f64)[big] / leg1["coef"].astype(f64)[big]
    assert np.abs(q / np.broadcast_to(w[:, None], big.shape)[big] - 1).max() <= 3 * N.U


@pytest.mark.gpu
def test_hip_dumped_coefficients_against_float64_models_of_the_devices_neighbours(leg1, oracle):
    """direction and distance of the dumped coefficients against the float64 models of the device's OWN five neighbours, under the bars
    tests/test_fit_device.py applies to the device functions in the distance band of every query (no new number): the plane distance
    within `bar_truth` (BANDS) of the float64 plane, the plane's unit normal no farther from it than the oracle's + 1e-5 (per segment,
    as there), the line distance within LINE_BANDS' bar of the oracle's.  The query handed to the models is the float64 transform of the
    float32 source point, the kernel's is float32 from its pose cache: the in-kernel transform is inside what the bars hold.  The
    DIRECTION of a line's coefficients is not checked: tests/test_fit_device.py has no bar for it."""
    from test_fit_device import BANDS, LINE_BANDS, dist_and_normal, oracle_corner, oracle_surf
    b = _batch()
    po = oracle.default_params(1)
    plane_bars, line_bars = {d: t for d, _, t in BANDS}, dict(LINE_BANDS)
    worst, normals = {}, []
    for sg in b["segments"]:
        it = b["items"][sg["item"]]
        sl = slice(sg["base"], sg["base"] + sg["n"])
        acc = np.flatnonzero(leg1["coef_ok"][sl] == 1)
        if not len(acc):
            continue
        tgt = it["tgt"][sg["kind"]]
        nb = tgt[leg1["nb"][:5, sl][:, acc].T]                           # [n, 5, 3] float32, nearest first
        q = N.to_map(it["T"], sg["src"][acc, :3])
        cf = leg1["coef"][sl][acc]
        d_dev, n_dev = dist_and_normal(cf)
        reach = np.linalg.norm(q, axis=1)                                # the band of every query: the first one that holds it
        table = plane_bars if sg["kind"] == 1 else line_bars
        band = np.array([min(d for d in table if d >= r) for r in reach])
        bar = np.array([table[d] for d in band])
        if sg["kind"] == 1:
            m = [N.surf_model(nb[i].astype(f64), q[i]) for i in range(len(acc))]
            d_true = np.array([x["dist"] for x in m]); n_true = np.array([x["normal"] for x in m])
            cfo, oko = oracle_surf(oracle, nb, q.astype(f32), po)
            _, n_orc = dist_and_normal(cfo)
            assert (oko == 1).all()
            e = np.abs(d_dev - d_true)
            en_d, en_o = np.abs(n_dev - n_true).max(1), np.abs(n_orc - n_true).max(1)
            normals.append((it["name"], float(en_d.max()), float(en_o.max())))
        else:
            cfo, oko = oracle_corner(oracle, nb, q.astype(f32), po)
            d_orc, _ = dist_and_normal(cfo)
            assert (oko == 1).all()
            e = np.abs(d_dev - d_orc)
        for d in np.unique(band):
            key = ("plane" if sg["kind"] == 1 else "line", float(d))
            worst[key] = max(worst.get(key, 0.0), float((e / bar)[band == d].max()))
    print("dumped coefficients, worst distance error / bar of the band:", {k: round(v, 3) for k, v in sorted(worst.items())})
    print("unit normals, worst |device - f64| against the oracle's (item, device, oracle):", max(normals, key=lambda t: t[1] - t[2]))
    assert {("plane", 10.0), ("line", 10.0)} <= set(worst) and any(k[1] > 10.0 for k in worst)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert all(dev <= orc + 1e-5 for _, dev, orc in normals), normals


def same_rows(out, ref, what):
    assert np.array_equal(out["blocks"], ref["blocks"]), (what, "block tables")
    bad = np.flatnonzero((bits(out["rows"]) != bits(ref["rows"])).any(1))
    assert bad.size == 0, (what, "rows differ in blocks", bad[:8], out["rows"][bad[:2]], ref["rows"][bad[:2]])
    print(f"{what}: {len(out['rows'])} partial rows bit-identical")


@pytest.mark.gpu
def test_hip_later_iterations_leave_the_same_rows(leg1):
    """fixed_iters = 3 at a frozen pose: iterations 1 and 2 run the other instantiations (seeded, wide); the dump holds the last one"""
    out = _run(fixed_iters=3)
    assert out["lanes"] == 8
    same_rows(out, leg1, "fixed_iters 3")
    assert np.array_equal(out["coef_ok"], leg1["coef_ok"])
    acc = leg1["coef_ok"] == 1
    assert np.array_equal(bits(out["coef"][acc]), bits(leg1["coef"][acc]))


ONE_LANE = {"walk": (1, ()), "graph": (3, ()), "rows_reach0": (5, (("row_reach", 0),)),
            "rows_reach2": (5, (("row_reach", 2), ("rebuild_targets_each_run", 1)))}


@pytest.mark.gpu
@pytest.mark.parametrize("leg", list(ONE_LANE))
def test_hip_one_lane_per_query_leaves_the_same_rows(leg1, leg):
    """k_assoc_walk<kQ = 1> reduces in its own tail (residual_and_reduce): same workgroups, same tree, same bits as k_rows_reduce"""
    mode, opts = ONE_LANE[leg]
    for iters in (1, 3):
        p = Prepared(mode, 1, opts)
        try:
            out = p.run(fixed_iters=iters)
            assert out["front"] == mode and out["lanes"] == 1 and p.ctx.get_option("search_mode") == mode
            if leg == "rows_reach2":
                assert p.ctx.get_option("row_reach_now") == 1
            assert np.array_equal(out["nb"][5] == 1, leg1["coef_ok"] == 1)
            same_rows(out, leg1, f"one lane per query, {leg}, fixed_iters {iters}")
        finally:
            p.close()


@pytest.mark.gpu
def test_hip_sorted_sources(leg1):
    """sort_sources = 1 moves the queries inside their segments, so the blocks hold other queries: per item, the total of its blocks is
    within the budget of the reference's item total and the counts are equal; the coefficients are, as a multiset per segment, those
    of the unsorted run.  "xcd_order" and "interleave" must not change a bit of their own baseline's rows."""
    b = _batch()
    terms, mags = N.terms_of_batch(b, leg1["coef"], leg1["coef_ok"])
    p = Prepared(1, 0, (("sort_sources", 1),))
    try:
        out = p.run()
        assert out["lanes"] == 8 and p.ctx.get_option("sorted_now") == 1
    finally:
        p.close()
    assert np.array_equal(out["blocks"], leg1["blocks"])
    for sg in b["segments"]:
        sl = slice(sg["base"], sg["base"] + sg["n"])
        rec = lambda o: np.sort(np.concatenate([bits(np.where((o["coef_ok"][sl] == 1)[:, None], o["coef"][sl], f32(0))),
                                                o["coef_ok"][sl, None].astype(np.uint32)], 1).view("u4,u4,u4,u4,u4").ravel())
        assert np.array_equal(rec(out), rec(leg1)), ("coefficients as a multiset", sg["item"], sg["kind"])
    worst = 0.0
    for i in range(len(b["items"])):
        mine = out["blocks"][:, 0] == i
        sl = slice(min(s["base"] for s in b["segments"] if s["item"] == i), max(s["base"] + s["n"] for s in b["segments"] if s["item"] == i))
        got, want, A = N.fsum_rows(out["rows"][mine]), N.fsum_rows(terms[sl]), N.fsum_rows(mags[sl])
        assert got[27] == want[27], (i, got[27], want[27])
        err, bud = np.abs(got - want), N.budget(A)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, err / bud, 0.0)
        worst = max(worst, float(r.max()))
    print(f"sorted sources: worst |item total - fsum| / budget = {worst:.4f}")
    assert worst < 1.0
    # bit-identical to their own baseline: the sector dispatch order (cell rows) and the free-running split (walk), on sorted sources
    for mode, opts, readout in ((5, (("xcd_order", 1),), "xcd_order_now"), (1, (("interleave", 2), ("interleave_min_blocks", 4)), "interleaved_now")):
        res = []
        for o in ((("xcd_order", 0), ("interleave", 0), ("interleave_min_blocks", 8192)), opts):
            p = Prepared(mode, 1, (("sort_sources", 1),) + o)
            try:
                res.append(p.run(fixed_iters=2))
                assert p.ctx.get_option("sorted_now") == 1 and p.ctx.get_option(readout) == (1 if o is opts else 0), (readout, o)
            finally:
                p.close()
        same_rows(res[1], res[0], f"{readout} against its own baseline")


@pytest.mark.gpu
def test_hip_trace_of_every_item_alone_against_its_rows(leg1):
    """every item registered alone (lisreg_align, min_corr = 1, one iteration): the trace's n_corr is the item's summed count and its
    AtA / AtB are float32(fsum of the item's partial rows) within one float ulp + 1e-13 * A — the solve's fixed-order fp64 sum of the
    same workgroups' rows, rounded to float."""
    import lisreg
    from lisreg import synth
    b = _batch()
    _, mags = N.terms_of_batch(b, leg1["coef"], leg1["coef_ok"])
    ctx = lisreg.Context(0)
    worst = 0.0
    try:
        for k, v in (("search_mode", 1), ("lanes_per_query", 0)) + BASE_OPTS:
            ctx.set_option(k, v)
        for i, it in enumerate(b["items"]):
            ctx.set_target(synth.to_pcl(it["tgt"][0]), synth.to_pcl(it["tgt"][1]))
            _, st, tr = ctx.align(synth.to_pcl(it["src"][0][:, :3]), synth.to_pcl(it["src"][1][:, :3]), it["T"], _params(1, 1, 1))
            mine = leg1["blocks"][:, 0] == i
            S = N.fsum_rows(leg1["rows"][mine])
            sl = slice(min(s["base"] for s in b["segments"] if s["item"] == i), max(s["base"] + s["n"] for s in b["segments"] if s["item"] == i))
            A = N.fsum_rows(mags[sl])
            assert len(tr) == 1 and tr[0, 0] == S[27] == st["n_corr_last"], (it["name"], tr[0, 0], S[27], st)
            want = np.zeros(42); amp = np.zeros(42)
            for k in range(21):
                for r, c in ((N.TRI_R[k], N.TRI_C[k]), (N.TRI_C[k], N.TRI_R[k])):
                    want[6 * r + c], amp[6 * r + c] = S[k], A[k]
            want[36:], amp[36:] = S[21:27], A[21:27]
            if S[27] < 1:
                want[:] = 0                                            # (nothing solved: the trace keeps its zeros)
            w32 = want.astype(f32)
            tol = np.spacing(np.abs(w32)).astype(f64) + 1e-13 * amp
            err = np.abs(tr[0, 1:43].astype(f64) - w32.astype(f64))
            assert np.all(err <= tol), (it["name"], np.flatnonzero(err > tol), tr[0, 1:43], w32)
            worst = max(worst, float((err / np.where(tol > 0, tol, 1)).max()))
    finally:
        ctx.close()
    print(f"trace against rows: worst |trace - float32(fsum)| / (ulp + 1e-13 A) = {worst:.3f}")


@pytest.mark.gpu
def test_hip_hook_refusals_leave_the_outputs_untouched():
    import lisreg
    L = lisreg.lib()
    n = _batch()["n_elems"]
    ip, fp, dp = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_double)

    def call(ctx, coef=True, n_elems=n, cap=64):
        nb = C.c_int(-7)
        blocks, rows = np.full((64, 4), -7, np.int32), np.full((64, 28), -7.0)
        cf, ok = np.full((n, 4), -7, f32), np.full(n, -7, np.int32)
        rc = L.lisreg_get_partial_rows(ctx._h, C.byref(nb), blocks.ctypes.data_as(ip), rows.ctypes.data_as(dp), cap,
                                       cf.ctypes.data_as(fp) if coef else None, ok.ctypes.data_as(ip) if coef else None, n_elems)
        untouched = nb.value == -7 and (blocks == -7).all() and (rows == -7).all() and (cf == -7).all() and (ok == -7).all()
        return rc, untouched, nb.value

    ctx = lisreg.Context(0)
    try:
        ctx.set_option("dump_neighbors", 1)
        assert call(ctx)[:2] == (lisreg.ERR_ARG, True) and "no prepared batch" in ctx.last_error()
    finally:
        ctx.close()
    p = Prepared(1, 0, (("dump_neighbors", 0),))                           # the dump switched off before the batch is prepared
    try:
        p.ctx.batch_prepare_device(p.items, p.T0, _params()); p.ctx.batch_run(); p.ctx.batch_fetch()
        assert call(p.ctx)[:2] == (lisreg.ERR_ARG, True) and "dump_neighbors" in p.ctx.last_error()
    finally:
        p.close()
    p = Prepared(1, 0)
    try:
        p.ctx.batch_prepare_device(p.items, p.T0, _params())
        p.ctx.batch_run(); p.ctx.batch_fetch()
        assert p.ctx.get_option("lanes_per_query") == 8
        assert call(p.ctx, n_elems=n - 1)[:2] == (lisreg.ERR_ARG, True) and "n_elems" in p.ctx.last_error()
        assert call(p.ctx, cap=3)[:2] == (lisreg.ERR_ARG, True) and "capacity" in p.ctx.last_error()
        assert L.lisreg_get_partial_rows(p.ctx._h, None, None, None, 0, None, None, 0) == lisreg.ERR_ARG
        rc, untouched, nb = call(p.ctx)
        assert rc == lisreg.OK and not untouched and nb == len(N.plan_blocks(_batch()))
    finally:
        p.close()
    p = Prepared(1, 1)
    try:
        p.ctx.batch_prepare_device(p.items, p.T0, _params())
        p.ctx.batch_run(); p.ctx.batch_fetch()
        assert p.ctx.get_option("lanes_per_query") == 1
        assert call(p.ctx)[:2] == (lisreg.ERR_ARG, True) and "one lane per query" in p.ctx.last_error()
        rc, untouched, nb = call(p.ctx, coef=False)
        assert rc == lisreg.OK and nb == len(N.plan_blocks(_batch()))
    finally:
        p.close()
