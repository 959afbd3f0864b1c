"""The device-resident map stores of csrc/lisreg_api_localmap.hip, branch by branch: lisreg_localmap_insert / _extract / _get,
lisreg_submap_insert / _extract, lisreg_keyframes_push / _target on the planted sequences of tests/map_store_ref.py.

CPU (-m "not gpu"): every case's census — the restatement's run alone proves that the case reaches the branch it exists for (a case
that lost its planted point fails here) — and lisreg_submap_crop_boxes (host arithmetic) on the cases' boxes.
GPU: after EVERY operation of a case the device state equals the restatement's: counts, feature_point_num, bounds, crop and
intersection boxes as integers / double bits, every class cloud, both targets and both sources as the bits of their 16-byte records
(label included), the installed search index point for point.  Local-map and submap cases run twice, from host PointXYZIL structs and
from LISREG_FMT_DEVICE records, against the same expected bits.  There is no tolerance anywhere in this file.

Ids kept to this file: local maps / submaps 700-715 (so map-index slots 60700-60715), key-frame ring 700, target slots 46 and 47."""
import ctypes as C
import functools

import numpy as np
import pytest

import map_store_ref as ref

MAP_ID, MAP_IDS, RING_ID, SLOTS = 700, dict(A=701, B=702, C=703, D=704, E=705, F=706, G=707, H=708, never=715), 700, (46, 47)

LOCALMAP_NAMES = ["at_threshold", "above_threshold", "band_widen", "band_off", "band_fltmax", "band_radius_fltmax", "empty_dynamic",
                  "leaf_too_small", "pad_zero", "after_reset"]
SUBMAP_NAMES = ["submap_main", "submap_empty_source", "submap_leaf_too_small"]
RING_NAMES = ["max_keep_1", "shrink", "kinds", "leaf_too_small", "shortcut"]


@functools.lru_cache(maxsize=None)
def _cases(kind):
    make = dict(localmap=ref.localmap_cases, submap=ref.submap_cases, ring=ref.ring_cases)[kind]
    return {c["name"]: c for c in make()}


@functools.lru_cache(maxsize=None)
def _expected(kind, name):
    """(case, expected states): computed once per process, shared by the census and both GPU runs, never modified."""
    if kind == "growth":
        case = dict(localmap=ref.growth_localmap_case, submap=ref.growth_submap_case)[name]()
        return case, (ref.run_localmap if name == "localmap" else ref.run_submaps)(case)
    case = _cases(kind)[name]
    return case, dict(localmap=ref.run_localmap, submap=ref.run_submaps, ring=ref.run_ring)[kind](case)


def test_the_case_lists_are_complete():
    assert [list(_cases(k)) for k in ("localmap", "submap", "ring")] == [LOCALMAP_NAMES, SUBMAP_NAMES, RING_NAMES]


# ---- CPU: the census -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LOCALMAP_NAMES)
def test_localmap_case_reaches_its_branch(oracle, name):
    assert ref.census_localmap(*_expected("localmap", name))


@pytest.mark.parametrize("name", SUBMAP_NAMES)
def test_submap_case_reaches_its_branch(oracle, name):
    assert ref.census_submaps(*_expected("submap", name))


@pytest.mark.parametrize("name", RING_NAMES)
def test_ring_case_reaches_its_branch(oracle, name):
    assert ref.census_ring(*_expected("ring", name))


def test_growth_cases_pass_the_first_allocation_on_the_fourth_insert(oracle):
    """grow_keep asks for max(1.5 * needed, 16 MB) = 16 MB for a class cloud's first allocation and DevBuf::ensure adds a quarter and
    256 bytes: 1 310 736 records of 16 bytes.  An insert asks for n + 1 records: 1 200 001 fit, 1 600 001 do not, so the fourth insert of
    400 000 reallocates with 1 200 000 records to keep.  (Three inserts stay inside the first allocation: a `keep` of half its size went
    unnoticed by them.)"""
    assert ref.FIRST_ALLOCATION_RECORDS == 1310736 and 3 * ref.GROW_N + 1 <= ref.FIRST_ALLOCATION_RECORDS < 4 * ref.GROW_N + 1
    assert ref.census_growth(_expected("growth", "localmap")[1], [2])
    assert ref.census_growth(_expected("growth", "submap")[1], range(5), "sinsert")


def test_a_case_that_lost_its_planted_point_fails_its_census(oracle):
    """The census is a condition on the input: without the point planted ON `near` / ON the crop box's face it must fail."""
    case = ref.case_above_threshold()
    frame = list(case["ops"][1][1])
    frame[0] = frame[0][frame[0]["label"] != ref.PLANT_TAG["on_near"]]
    case["ops"][1] = ("insert", frame, case["ops"][1][2])
    with pytest.raises(AssertionError):
        ref.census_localmap(case, ref.run_localmap(case))
    case = ref.case_pad_zero()
    frame = list(case["ops"][0][1])
    frame[2] = frame[2][frame[2]["label"] != 800 + list(ref.PAD0_GROUND).index("inside_crop_face")]
    case["ops"][0] = ("insert", frame, case["ops"][0][2])
    with pytest.raises(AssertionError):
        ref.census_localmap(case, ref.run_localmap(case))
    case = ref.case_band("widen")
    frame = list(case["ops"][1][1])
    frame[0] = frame[0][~np.isin(frame[0]["label"], (600, 601, 602))]
    case["ops"][1] = ("insert", frame, case["ops"][1][2])
    with pytest.raises(AssertionError):
        ref.census_localmap(case, ref.run_localmap(case))


def test_submap_crop_boxes_on_the_cases_boxes(oracle):
    """lisreg_submap_crop_boxes is host arithmetic: on every extract of the submap cases it gives submap_crop_boxes' doubles."""
    import lisreg
    import replay_oracle as ro
    L = lisreg.lib()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    boxes = ref.crop_box_inputs()
    assert len(boxes) >= 4
    for pb, Tp, cb, Tc, pad in boxes:
        pb, cb = np.ascontiguousarray(pb, np.float64), np.ascontiguousarray(cb, np.float64)
        a, b = np.zeros(6), np.zeros(6)
        L.lisreg_submap_crop_boxes(pb.ctypes.data_as(dp), Tp.ctypes.data_as(fp), cb.ctypes.data_as(dp), Tc.ctypes.data_as(fp), pad,
                                   a.ctypes.data_as(dp), b.ctypes.data_as(dp))
        ia, ib = ro.submap_crop_boxes(pb, Tp, cb, Tc, pad)
        assert np.array_equal(a, ia) and np.array_equal(b, ib)


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _bits(records):
    return np.ascontiguousarray(records, np.float32).view(np.uint32)


def _want(cloud):
    import lisreg
    return _bits(lisreg.pack_device_records(cloud))


def _xyz(cloud):
    from lisreg import synth
    return synth.pcl_xyz(cloud).view(np.uint32)


def _installed(ctx, slot):
    """The corner and surf clouds a target slot's search index was built over, in their own order, as bits."""
    out = []
    for kind in (0, 1):
        idx = ctx.target_index(slot, kind)
        got = np.zeros((idx["n"], 3), np.float32)
        got[idx["sorted"][:, 3].view(np.int32)] = idx["sorted"][:, :3]
        out.append(got.view(np.uint32))
    return out


def _class_clouds(ctx, mid, upto=5):
    return [_bits(ctx.localmap_get(mid, k)) for k in range(upto)]


def _insert(ctx, submap, mid, clouds, pose, P, device_records, sub_pose=None):
    """One insert from host structs or from device records (freed after the call: the insert is complete on return)."""
    import lisreg
    if not device_records:
        return ctx.submap_insert(mid, clouds, pose, sub_pose, P) if submap else ctx.localmap_insert(mid, clouds, pose, P)
    devs = [lisreg.DeviceArray(lisreg.pack_device_records(c)) if len(c) else None for c in clouds]
    ptrs, counts = [d.ptr if d else 0 for d in devs], [len(c) for c in clouds]
    try:
        return ctx.submap_insert_device(mid, ptrs, counts, pose, sub_pose, P) if submap else ctx.localmap_insert_device(mid, ptrs, counts, pose, P)
    finally:
        for d in devs:
            if d:
                d.free()


def _release(ctx, map_ids=(), ring=False):
    from lisreg import synth
    none = np.zeros(0, synth.PCL_DTYPE)
    for s in SLOTS:
        ctx.set_target(none, none, slot=s)                # (a slot installed from a store points into that store's buffers)
    for m in map_ids:
        ctx.localmap_reset(m)
    if ring:
        ctx.keyframes_reset(RING_ID)


def _drive_localmap(ctx, case, states, device_records):
    P = ref.device_params(case["prm"])
    slot = SLOTS[0]
    ctx.localmap_reset(MAP_ID)
    installed = None
    try:
        for i, (op, st) in enumerate(zip(case["ops"], states)):
            if op[0] == "reset":
                ctx.localmap_reset(MAP_ID)
                continue
            if op[0] == "insert":
                info = _insert(ctx, False, MAP_ID, op[1], np.asarray(op[2], np.float32), P, device_records)
            else:
                info = ctx.localmap_extract(MAP_ID, np.asarray(op[1], np.float32), P, target_slot=slot if st["slot"] >= 0 else -1)
                assert np.array_equal(info["crop"], st["crop"]), (i, info["crop"], st["crop"])
                assert (info["n_target_corner"], info["n_target_surf"]) == (len(st["tc"]), len(st["ts"])), i
                assert np.array_equal(_bits(ctx.localmap_get(MAP_ID, 5)), _want(st["tc"])), (i, "corner target")
                assert np.array_equal(_bits(ctx.localmap_get(MAP_ID, 6)), _want(st["ts"])), (i, "surf target")
                if st["slot"] >= 0:
                    installed = [_xyz(st["tc"]), _xyz(st["ts"])]
                if installed is not None:                  # target_slot = -1 installs nothing: the slot keeps what it held
                    assert all(np.array_equal(g, w) for g, w in zip(_installed(ctx, slot), installed)), (i, "installed index")
            assert info["n"] == st["n"] and info["feature_point_num"] == st["fpn"], (i, info, st["n"], st["fpn"])
            assert np.array_equal(info["bound"], st["bound"]), (i, info["bound"], st["bound"])
            for k, got in enumerate(_class_clouds(ctx, MAP_ID)):
                assert np.array_equal(got, _want(st["cls"][k])), (i, op[0], "class", k)
    finally:
        _release(ctx, [MAP_ID])


@pytest.mark.gpu
@pytest.mark.parametrize("device_records", [False, True], ids=["host_structs", "device_records"])
@pytest.mark.parametrize("name", LOCALMAP_NAMES)
def test_localmap_equals_restatement_after_every_operation(oracle, gpu_ctx, name, device_records):
    case, states = _expected("localmap", name)
    ref.census_localmap(case, states)
    _drive_localmap(gpu_ctx, case, states, device_records)


def _refuse(ctx, pre, cur):
    """lisreg_submap_extract on a pair it must refuse: LISREG_ERR_NO_TARGET, `out` not written."""
    import lisreg
    out = lisreg.SubmapExtractOut()
    C.memset(C.byref(out), 0xAB, C.sizeof(out))
    before = bytes(out)
    T = np.zeros(6, np.float32)
    fp = C.POINTER(C.c_float)
    rc = ctx._L.lisreg_submap_extract(ctx._h, pre, cur, T.ctypes.data_as(fp), T.ctypes.data_as(fp), 10.0, 0.2, 0.5, SLOTS[1], C.byref(out))
    assert rc == lisreg.ERR_NO_TARGET and bytes(out) == before


def _drive_submaps(ctx, case, states, device_records):
    import lisreg
    P = ref.device_params(case["prm"])
    slot = SLOTS[0]
    used = sorted({MAP_IDS[op[1]] for op in case["ops"] if op[0] == "sinsert"})
    for m in used:
        ctx.localmap_reset(m)
    installed = None
    try:
        for i, (op, st) in enumerate(zip(case["ops"], states)):
            if op[0] == "sinsert":
                _, key, clouds, rel, sub_pose = op
                mid = MAP_IDS[key]
                info = _insert(ctx, True, mid, clouds, None if rel is None else np.asarray(rel, np.float32), P, device_records,
                               np.asarray(sub_pose, np.float32))
                assert info["n"] == st["n"] and info["feature_point_num"] == st["fpn"], (i, info["n"], st["n"])
                assert np.array_equal(info["local_bound"], st["local_bound"]) and np.array_equal(info["bound"], st["bound"]), i
                for k, got in enumerate(_class_clouds(ctx, mid)):
                    assert np.array_equal(got, _want(st["cls"][k])), (i, key, "class", k)
            elif op[0] == "sextract":
                _, pk, ck, pp, cp, pad, cl, sl, _ = op
                pre, cur = MAP_IDS[pk], MAP_IDS[ck]
                before = [_class_clouds(ctx, m) for m in (pre, cur)]
                out = ctx.submap_extract(pre, cur, np.asarray(pp, np.float32), np.asarray(cp, np.float32), pad=pad, corner_leaf=cl, surf_leaf=sl,
                                         target_slot=slot if st["slot"] >= 0 else -1)
                assert np.array_equal(out["isect"], st["isect"]) and np.array_equal(out["isect_local"], st["isect_local"]), i
                assert (out["n_target_corner"], out["n_target_surf"], out["n_src_corner"], out["n_src_surf"]) == \
                       (len(st["tc"]), len(st["ts"]), len(st["sc"]), len(st["ss"])), i
                for m, c, want in ((pre, 5, st["tc"]), (pre, 6, st["ts"]), (cur, 5, st["sc"]), (cur, 6, st["ss"])):
                    assert np.array_equal(_bits(ctx.localmap_get(m, c)), _want(want)), (i, m, c)
                for ptr, want in ((out["src_corner_ptr"], st["sc"]), (out["src_surf_ptr"], st["ss"])):      # the sources as handed out
                    if len(want):
                        assert np.array_equal(_bits(lisreg.device_to_host(ptr, (len(want), 4))), _want(want)), i
                if st["slot"] >= 0:
                    installed = [_xyz(st["tc"]), _xyz(st["ts"])]
                if installed is not None:
                    assert all(np.array_equal(g, w) for g, w in zip(_installed(ctx, slot), installed)), (i, "installed index")
                after = [_class_clouds(ctx, m) for m in (pre, cur)]                                       # an extract leaves the classes alone
                assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y)), i
            else:
                pre, cur = MAP_IDS[op[1]], MAP_IDS[op[2]]
                live = [m for m in {pre, cur} if m != MAP_IDS["never"]]
                before = [_class_clouds(ctx, m, 7) for m in live]
                _refuse(ctx, pre, cur)
                after = [_class_clouds(ctx, m, 7) for m in live]
                assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y)), i
                if installed is not None:
                    assert all(np.array_equal(g, w) for g, w in zip(_installed(ctx, slot), installed)), (i, "installed index")
    finally:
        _release(ctx, used)


@pytest.mark.gpu
@pytest.mark.parametrize("device_records", [False, True], ids=["host_structs", "device_records"])
@pytest.mark.parametrize("name", SUBMAP_NAMES)
def test_submaps_equal_restatement_after_every_operation(oracle, gpu_ctx, name, device_records):
    case, states = _expected("submap", name)
    ref.census_submaps(case, states)
    _drive_submaps(gpu_ctx, case, states, device_records)


@pytest.mark.gpu
def test_localmap_class_cloud_grows_past_its_first_allocation(oracle, gpu_ctx):
    """grow_keep with contents to keep: the ground class passes 1 310 736 records (the first allocation: 16 MB and DevBuf's quarter of
    head-room) on its fourth insert of 400 000; after every insert the WHOLE class equals the restatement, then through the in-place grid
    and crop and one more insert."""
    case, states = _expected("growth", "localmap")
    ref.census_growth(states, [2])
    _drive_localmap(gpu_ctx, case, states, device_records=False)


@pytest.mark.gpu
def test_submap_class_clouds_grow_past_their_first_allocation(oracle, gpu_ctx):
    """All five class clouds of a submap, the outlier class among them, pass 1 310 736 records in the same insert, the fourth; the dynamic class
    through the filtered path's append.  Then an extract over the grown clouds and one more insert."""
    case, states = _expected("growth", "submap")
    ref.census_growth(states, range(5), "sinsert")
    _drive_submaps(gpu_ctx, case, states, device_records=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", RING_NAMES)
def test_keyframe_ring_equals_restatement_after_every_operation(oracle, gpu_ctx, name):
    """Push and target along a case; after every operation each target slot holds exactly what the restatement says it must: the
    ring's target where one was installed or re-installed, the caller's own where lisreg_keyframes_target had no business with it.
    The shortcut ("no key frame since the last call") shows only in that: a call that wrongly takes it leaves a stale index behind."""
    case, states = _expected("ring", name)
    ref.census_ring(case, states)
    hand = [ref.mk(ref.lattice(40, 99, z=2.0), 0), ref.mk(ref.lattice(90, 98, z=-2.0), 0)]
    holds = {}
    gpu_ctx.keyframes_reset(RING_ID)
    try:
        for i, (op, st) in enumerate(zip(case["ops"], states)):
            if op[0] == "push":
                info = gpu_ctx.keyframes_push(RING_ID, op[1], op[2], np.asarray(op[3], np.float32), max_keep=op[4])
                assert info["n_keyframes"] == st["n_keyframes"], i
            elif op[0] == "hand":
                gpu_ctx.set_target(hand[0], hand[1], slot=SLOTS[op[1]])
                holds[op[1]] = [_xyz(hand[0]), _xyz(hand[1])]
            else:
                slot = SLOTS[st["slot"]] if st["slot"] >= 0 else -1
                info = gpu_ctx.keyframes_target(RING_ID, op[1], op[2], target_slot=slot)
                assert info == dict(n_keyframes=st["n_keyframes"], n_target_corner=len(st["tc"]), n_target_surf=len(st["ts"])), (i, info)
                if st["slot"] >= 0:
                    holds[st["slot"]] = [_xyz(st["tc"]), _xyz(st["ts"])]
            for s, want in holds.items():
                assert all(np.array_equal(g, w) for g, w in zip(_installed(gpu_ctx, SLOTS[s]), want)), (i, op[0], "slot", s)
    finally:
        _release(gpu_ctx, ring=True)
