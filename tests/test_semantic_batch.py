"""lisreg_semantic_split_batch: the class clouds of up to 256 key frames in three launches and one host synchronisation, and
lisreg_concat_device_batch, the other per-frame step of the semantic chain, in one launch.

The contract is per frame: out.cloud[0..4][0 .. n[k]), n[] and status are, byte for byte, what lisreg_semantic_split gives for that frame
alone.  Two yardsticks: `np_split`, the stable five-way partition in six lines of numpy (independent of the library), and the single
call's bytes for the same frame.  Records are uint32 words throughout, so NaN coordinates and payloads compare by bits.  Every output
buffer is prefilled with a sentinel word and lies back to back with its neighbours in one arena: a record written past n[k], into a
failed frame or into a neighbour shows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
u32 = np.uint32
SENT = u32(0xA5C3F00D)
DEFAULT_MAP = [0, 10, 10, 10, 10, 10, 10, 10, 10, 40, 40, 40, 70, 50, 50, 70, 81, 70, 81, 81] + [0] * 12      # config/label.yaml:177-196


def np_split(rec, using_label=None):
    """yardstick 1: records (n, 4) uint32 -> the five class clouds, in input order"""
    u = np.asarray(using_label if using_label is not None else DEFAULT_MAP, u32)[rec[:, 3] & 31]
    cls = np.select([u == 10, u == 40, u == 50, u == 81], [0, 1, 2, 3], 4)
    return [rec[cls == k] for k in range(5)]


def frame(n, seed, labels=None):
    """n records as uint32 words: finite coordinates, the label (0 .. 19 unless given) in the payload"""
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 4), u32)
    rec[:, :3] = rng.uniform(-50, 50, (n, 3)).astype(np.float32).view(u32)
    rec[:, 3] = rng.integers(0, 20, n) if labels is None else np.asarray(labels, u32)
    return rec


class Arena:
    """inputs back to back in one device buffer; the outputs (caps[f][k] records, sentinel words; absent where (f, k) is in `nulls`)
    back to back in another, in (frame, class) order"""

    def __init__(self, recs, caps=None, nulls=(), shared_in=False):
        import lisreg
        self.recs = [np.ascontiguousarray(r, u32).reshape(-1, 4) for r in recs]
        self.ns = [len(r) for r in self.recs]
        self.caps = [list(c) for c in caps] if caps is not None else [[n] * 5 for n in self.ns]
        self.nulls = set(nulls)
        live = [r for r in self.recs if len(r)]
        self.d_in = lisreg.DeviceArray(np.concatenate(live) if live and not shared_in else (self.recs[0] if live else np.zeros((1, 4), u32)))
        off = np.concatenate([[0], np.cumsum(self.ns)]) if not shared_in else np.zeros(len(recs) + 1, np.int64)
        self.in_ptrs = [self.d_in.ptr + 16 * int(o) for o in off[:-1]]
        flat = [0 if (f, k) in self.nulls else self.caps[f][k] for f in range(len(recs)) for k in range(5)]
        self.out_off = np.concatenate([[0], np.cumsum(flat)]).astype(np.int64)
        self.total = max(int(self.out_off[-1]), 1)
        self.d_out = lisreg.DeviceArray(np.full((self.total, 4), SENT, u32))
        self.out_ptrs = [[0 if (f, k) in self.nulls else self.d_out.ptr + 16 * int(self.out_off[5 * f + k]) for k in range(5)] for f in range(len(recs))]

    def raw(self):
        return self.d_out.download(self.total).view(u32)

    def outputs(self):
        got = self.raw()
        return [[got[int(self.out_off[5 * f + k]):int(self.out_off[5 * f + k + 1])] for k in range(5)] for f in range(len(self.ns))]

    def free(self):
        self.d_in.free(); self.d_out.free()


def single(ctx, in_ptr, n, out_ptrs, caps, using_label=None):
    """yardstick 2: lisreg_semantic_split on one frame -> (counts, status); a refused frame keeps the counts the call wrote back"""
    import lisreg
    so = lisreg.SemanticOut()
    for k in range(5):
        so.cloud[k] = int(out_ptrs[k]) or None
        so.cap[k] = int(caps[k])
    m = (C.c_uint32 * 32)(*using_label) if using_label is not None else None
    rc = ctx._L.lisreg_semantic_split(ctx._h, C.c_void_p(in_ptr) if in_ptr else None, n, 16, lisreg.FMT_DEVICE, m, C.byref(so))
    assert rc in (lisreg.OK, lisreg.ERR_ARG), rc
    return [int(so.n[k]) for k in range(5)], rc


def run_batch(ctx, recs, caps=None, nulls=(), using_label=None, shared_in=False):
    A = Arena(recs, caps, nulls, shared_in)
    counts, status = ctx.semantic_split_batch_device(A.in_ptrs, A.ns, A.out_ptrs, A.caps, using_label)
    outs = A.outputs()
    A.free()
    return counts, status, outs


def run_singles(ctx, recs, caps=None, nulls=(), using_label=None):
    A = Arena(recs, caps, nulls)
    counts, status = [], []
    for f in range(len(recs)):
        n, rc = single(ctx, A.in_ptrs[f], A.ns[f], A.out_ptrs[f], A.caps[f], using_label)
        counts.append(n); status.append(rc)
    outs = A.outputs()
    A.free()
    return counts, status, outs


def check(ctx, recs, caps=None, nulls=(), using_label=None):
    """batch == single calls == numpy: statuses, counts, every word of every output buffer, the sentinels past n[k] included"""
    import lisreg
    recs = [np.ascontiguousarray(r, u32).reshape(-1, 4) for r in recs]
    b_n, b_st, b_out = run_batch(ctx, recs, caps, nulls, using_label)
    s_n, s_st, s_out = run_singles(ctx, recs, caps, nulls, using_label)
    assert b_st == s_st, (b_st, s_st)
    assert b_n == s_n, (b_n, s_n)
    for f, rec in enumerate(recs):
        want = np_split(rec, using_label)
        assert b_n[f] == [len(w) for w in want], (f, b_n[f])
        fits = all((f, k) in nulls or len(want[k]) <= (caps[f][k] if caps is not None else len(rec)) for k in range(5))
        assert b_st[f] == (lisreg.OK if fits else lisreg.ERR_ARG), (f, b_st[f])
        for k in range(5):
            got = b_out[f][k]
            assert got.tobytes() == s_out[f][k].tobytes(), ("frame", f, "class", k, "differs from the single call")
            m = len(want[k]) if fits and (f, k) not in nulls else 0                  # a failed frame and a NULL class: nothing written
            assert np.array_equal(got[:m], want[k][:m]), ("frame", f, "class", k, "differs from the numpy partition")
            assert (got[m:] == SENT).all(), ("frame", f, "class", k, "written past n[k]")
    return b_n, b_st, b_out


def T():
    import lisreg
    return lisreg.SEMANTIC_BATCH_TILE


# ---- sizes --------------------------------------------------------------------------------------------------------------------------
def test_sizes_around_wavefront_workgroup_and_tile(gpu_ctx):
    t = T()
    sizes = [0, 1, 2, 63, 64, 65, 255, 256, 257, t - 1, t, t + 1, 2 * t, 3 * t + 5]
    n, st, _ = check(gpu_ctx, [frame(m, 100 + i) for i, m in enumerate(sizes)])
    assert [sum(c) for c in n] == sizes and st == [0] * len(sizes)


# ---- class patterns: a frame of 3T + 5 points between two ordinary ones -----------------------------------------------------------------
def pattern_labels(name, n):
    i = np.arange(n)
    rng = np.random.default_rng(7)
    if name.startswith("all_"):                                    # one label of the class: 1 dynamic, 9 ground, 13 building, 16 pole, 0 outlier
        return np.full(n, {"all_dynamic": 1, "all_ground": 9, "all_building": 13, "all_pole": 16, "all_outlier": 0}[name])
    if name == "no_ground":
        return rng.choice([1, 5, 13, 14, 16, 18, 19, 0, 12, 15, 17], n)
    if name == "labels_20_259":                                    # & 31 matters; 20 .. 31 fall to outlier
        return 20 + (rng.integers(0, 240, n))
    if name == "i_mod_5":                                          # every lane differs from its neighbour
        return np.array([1, 9, 13, 16, 0])[i % 5]
    if name == "runs_of_64":                                       # a wavefront is one class
        return np.array([1, 9, 13, 16, 0])[(i // 64) % 5]
    if name == "runs_of_64_shifted":
        return np.array([1, 9, 13, 16, 0])[((i + 1) // 64) % 5]
    raise KeyError(name)


@pytest.mark.parametrize("name", ["all_dynamic", "all_ground", "all_building", "all_pole", "all_outlier", "no_ground", "labels_20_259", "i_mod_5",
                                  "runs_of_64", "runs_of_64_shifted"])
def test_class_patterns(gpu_ctx, name):
    n = 3 * T() + 5
    recs = [frame(700, 1), frame(n, 2, pattern_labels(name, n)), frame(1300, 3)]
    counts, st, _ = check(gpu_ctx, recs)
    assert st == [0, 0, 0]
    if name.startswith("all_"):
        k = ["all_dynamic", "all_ground", "all_building", "all_pole", "all_outlier"].index(name)
        assert counts[1] == [n if q == k else 0 for q in range(5)]
    if name == "no_ground":
        assert counts[1][1] == 0 and min(counts[1][0], counts[1][2], counts[1][3], counts[1][4]) > 0


def test_custom_using_label(gpu_ctx):
    rng = np.random.default_rng(11)
    m = [int(x) for x in rng.choice([10, 40, 50, 81, 70, 0, 11], 32)]
    n = 3 * T() + 5
    recs = [frame(500, 4, rng.integers(0, 32, 500)), frame(n, 5, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(u32)), frame(64, 6)]
    counts, st, _ = check(gpu_ctx, recs, using_label=m)
    assert st == [0, 0, 0] and sum(c > 0 for c in counts[1]) == 5
    assert counts != run_batch(gpu_ctx, recs)[0]                   # the map was read


def test_all_sixteen_bytes_arrive(gpu_ctx):
    """NaN, +-inf, denormal coordinates and payloads with high bits: records are copied whole, bit for bit"""
    n = 2 * T() + 77
    rng = np.random.default_rng(12)
    rec = rng.integers(0, 2 ** 32, (n, 4), dtype=np.uint64).astype(u32)                   # any bits at all: many NaNs among them
    odd = np.array([0x7FC00001, 0xFFC00000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x7FFFFFFF, 0x80000000], u32)
    rec[::3, 0] = odd[np.arange(len(rec[::3])) % 8]; rec[1::3, 1] = odd[::-1][np.arange(len(rec[1::3])) % 8]; rec[2::3, 2] = odd[np.arange(len(rec[2::3])) % 8]
    rec[::2, 3] = np.array([0x7FC00001, 0xFFFFFFF2, 0x80000010, 0x7F80000D], u32)[np.arange(len(rec[::2])) % 4]
    counts, st, outs = check(gpu_ctx, [frame(300, 13), rec, frame(10, 14)])
    assert st == [0, 0, 0]
    back = np.concatenate([outs[1][k][:counts[1][k]] for k in range(5)])
    assert sorted(map(bytes, back)) == sorted(map(bytes, rec))      # every record arrived once, whole


# ---- batch shapes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 256])
def test_frame_counts(gpu_ctx, k):
    rng = np.random.default_rng(k)
    sizes = rng.integers(0, 301, k) if k == 256 else [2 * T() + 3, 999][:k]
    check(gpu_ctx, [frame(int(m), 20 + i) for i, m in enumerate(sizes)])


def test_one_big_frame_among_small_ones(gpu_ctx):
    counts, st, _ = check(gpu_ctx, [frame(100, 30), frame(100, 31), frame(120000, 32), frame(100, 33)])
    assert st == [0] * 4 and sum(counts[2]) == 120000


def test_no_frames_and_too_many(gpu_ctx):
    import lisreg
    assert gpu_ctx.semantic_split_batch_device([], [], [], []) == ([], [])
    assert gpu_ctx._L.lisreg_semantic_split_batch(gpu_ctx._h, 0, None, None) == lisreg.OK
    A = Arena([frame(3, 40 + i) for i in range(257)])
    with pytest.raises(lisreg.LisregError) as ex:
        gpu_ctx.semantic_split_batch_device(A.in_ptrs, A.ns, A.out_ptrs, A.caps)
    assert ex.value.code == lisreg.ERR_ARG and "n_frames" in str(ex.value) and (A.raw() == SENT).all()
    counts, st = gpu_ctx.semantic_split_batch_device(A.in_ptrs[:256], A.ns[:256], A.out_ptrs[:256], A.caps[:256])
    assert st == [0] * 256 and all(sum(c) == 3 for c in counts)
    A.free()


# ---- capacity, NULL classes, shared input -----------------------------------------------------------------------------------------------
def test_a_short_capacity_fails_its_frame_alone(gpu_ctx):
    import lisreg
    recs = [frame(1500, 50), frame(2 * T() + 9, 51), frame(800, 52)]
    want = [[len(w) for w in np_split(r)] for r in recs]
    for k in (0, 4):
        caps = [list(w) for w in want]                             # cap == count everywhere: every frame passes
        counts, st, _ = check(gpu_ctx, recs, caps)
        assert st == [0, 0, 0] and counts == want
        caps[1][k] -= 1
        counts, st, outs = check(gpu_ctx, recs, caps)
        assert st == [lisreg.OK, lisreg.ERR_ARG, lisreg.OK] and counts == want
        assert all((outs[1][q] == SENT).all() for q in range(5))


def test_null_classes_are_counted_not_written(gpu_ctx):
    recs = [frame(T() + 50, 60), frame(2000, 61), frame(3 * T(), 62)]
    want = [[len(w) for w in np_split(r)] for r in recs]
    counts, st, _ = check(gpu_ctx, recs, nulls={(0, 1), (0, 3), (2, 0)})
    assert counts == want and st == [0, 0, 0]
    counts, st, _ = check(gpu_ctx, recs, nulls={(f, k) for f in range(3) for k in range(5)})                 # counts only
    assert counts == want and st == [0, 0, 0]
    caps = [[0] * 5, [2000] * 5, [0] * 5]                           # a NULL class never fails a frame, a non-NULL one of cap 0 does
    counts, st, _ = check(gpu_ctx, recs, caps, nulls={(0, k) for k in range(5)})
    assert counts == want and st == [0, 0, -1]


def test_two_jobs_may_split_the_same_input(gpu_ctx):
    rec = frame(2 * T() + 31, 70)
    counts, st, outs = run_batch(gpu_ctx, [rec, rec], shared_in=True)
    want = np_split(rec)
    assert st == [0, 0] and counts[0] == counts[1] == [len(w) for w in want]
    for f in range(2):
        for k in range(5):
            assert np.array_equal(outs[f][k][:len(want[k])], want[k]) and (outs[f][k][len(want[k]):] == SENT).all()


# ---- refusals: ERR_ARG, nothing written, the job named ------------------------------------------------------------------------------------
def refused(ctx, A, in_ptrs, ns, out_ptrs, caps, word):
    import lisreg
    with pytest.raises(lisreg.LisregError) as ex:
        ctx.semantic_split_batch_device(in_ptrs, ns, out_ptrs, caps)
    assert ex.value.code == lisreg.ERR_ARG and word in str(ex.value), str(ex.value)
    assert (A.raw() == SENT).all(), "a refused call wrote"


def test_refusals(gpu_ctx):
    import copy
    import lisreg
    A = Arena([frame(400, 80), frame(500, 81), frame(600, 82)])
    I, N, O, Cp = A.in_ptrs, A.ns, A.out_ptrs, A.caps

    def mod(x, f, v, k=None):
        y = copy.deepcopy(x)
        if k is None:
            y[f] = v
        else:
            y[f][k] = v
        return y
    refused(gpu_ctx, A, I, mod(N, 1, -1), O, Cp, "job 1")                                       # n < 0
    refused(gpu_ctx, A, mod(I, 2, 0), N, O, Cp, "job 2")                                        # in == NULL with n > 0
    refused(gpu_ctx, A, I, N, O, mod(Cp, 0, -1, 3), "job 0")                                    # cap < 0 on a non-NULL cloud
    refused(gpu_ctx, A, I, mod(mod(mod(N, 0, 700000000), 1, 700000000), 2, 700000000), O, Cp, "2e9")
    refused(gpu_ctx, A, I, N, mod(O, 1, I[1] + 16 * 10, 2), Cp, "job 1")                        # an output inside its own input
    refused(gpu_ctx, A, I, N, mod(O, 0, I[2], 4), Cp, "job 0")                                  # ... on another job's input
    refused(gpu_ctx, A, I, N, mod(O, 2, O[2][0] + 16, 1), Cp, "job 2")                          # two classes of one job
    refused(gpu_ctx, A, I, N, mod(O, 2, O[0][0] + 16 * 399, 3), Cp, "job")                      # outputs of two jobs
    assert gpu_ctx._L.lisreg_semantic_split_batch(gpu_ctx._h, 2, None, None) == lisreg.ERR_ARG  # jobs == NULL
    assert b"jobs is NULL" in gpu_ctx._L.lisreg_last_error(gpu_ctx._h)
    assert gpu_ctx._L.lisreg_semantic_split_batch(gpu_ctx._h, -1, None, None) == lisreg.ERR_ARG
    assert (A.raw() == SENT).all()
    counts, st = gpu_ctx.semantic_split_batch_device(I, N, O, Cp)                                # and the batch as it is passes
    assert st == [0, 0, 0] and [sum(c) for c in counts] == N
    A.free()


# ---- reuse, determinism, the caller's stream ----------------------------------------------------------------------------------------------
def test_large_small_large_on_one_context(gpu_ctx):
    big = [frame(int(m), 90 + i) for i, m in enumerate([3 * T() + 5, 0, 17, 2 * T(), 5000, 1, T() - 1, 9000])]
    small = [frame(40, 99)]
    a = run_batch(gpu_ctx, big)
    s1 = run_batch(gpu_ctx, small)
    b = run_batch(gpu_ctx, big)
    s2 = run_batch(gpu_ctx, small)
    for x, y in ((a, b), (s1, s2)):
        assert x[0] == y[0] and x[1] == y[1]
        assert all(p.tobytes() == q.tobytes() for fx, fy in zip(x[2], y[2]) for p, q in zip(fx, fy))
    check(gpu_ctx, big)


def test_on_a_callers_busy_stream():
    """the input arrives late on the caller's stream, behind a stall; a context set to that stream must split the real input"""
    import lisreg
    from stream_gate import Gate
    gate = Gate()
    ctx = lisreg.Context(0)
    S = gate.stream_create()
    try:
        ns = [2 * T() + 3, 1500, 700]
        real = np.concatenate([frame(n, 200 + i) for i, n in enumerate(ns)])
        decoy = np.concatenate([frame(n, 300 + i) for i, n in enumerate(ns)])
        d_real, d_decoy, dst = lisreg.DeviceArray(real), lisreg.DeviceArray(decoy), lisreg.DeviceArray(decoy)
        d_out = lisreg.DeviceArray(np.full((5 * sum(ns), 4), SENT, u32))
        off = np.concatenate([[0], np.cumsum(ns)])
        in_ptrs = [dst.ptr + 16 * int(o) for o in off[:-1]]
        out_ptrs = [[d_out.ptr + 16 * (5 * int(off[f]) + k * ns[f]) for k in range(5)] for f in range(3)]
        caps = [[n] * 5 for n in ns]

        def run(src):
            gate.hip.hipDeviceSynchronize()
            d_out.upload(np.full((5 * sum(ns), 4), SENT, u32))
            if src is not None:
                dst.copy_from_device(src.ptr, src.nbytes)
            gate.hip.hipDeviceSynchronize()
            r, t = gate.wall(lambda: ctx.semantic_split_batch_device(in_ptrs, ns, out_ptrs, caps))
            gate.stream_sync(ctx.stream); gate.hip.hipDeviceSynchronize()
            return (r, d_out.download(5 * sum(ns)).view(u32).tobytes()), t
        out_decoy, _ = run(d_decoy)
        out_real, _ = run(d_real)
        again, t_call = run(d_real)
        assert again == out_real and out_real != out_decoy
        assert out_real[0][0] == [[len(w) for w in np_split(real[int(a):int(b)])] for a, b in zip(off[:-1], off[1:])]
        run(d_decoy)                                               # whatever the context keeps now holds the decoy's
        gate.hip.hipDeviceSynchronize()
        d_out.upload(np.full((5 * sum(ns), 4), SENT, u32))
        gate.hip.hipDeviceSynchronize()
        ctx.set_stream(S)
        try:
            assert ctx.stream == S
            gate.late_input(S, dst, d_real, d_decoy, gate.stall_ms_for(t_call))
            ev = gate.mark(S)
            pending_before = gate.event_pending(ev)
            r = ctx.semantic_split_batch_device(in_ptrs, ns, out_ptrs, caps)
            gate.stream_sync(S)
        finally:
            ctx.set_stream(None)
        gate.hip.hipDeviceSynchronize()
        gate.event_destroy(ev)
        got = (r, d_out.download(5 * sum(ns)).view(u32).tobytes())
        assert pending_before, "stall too short: the producer had finished before the call was made"
        assert got == out_real, "on the busy caller's stream the call " + ("split the DECOY" if got == out_decoy else "gave neither result")
        for a in (d_real, d_decoy, dst, d_out):
            a.free()
    finally:
        gate.hip.hipDeviceSynchronize()
        gate.stream_destroy(S)
        ctx.close()
        gate.close()


# ---- lisreg_concat_device_batch ---------------------------------------------------------------------------------------------------------
class ConcatArena:
    """jobs[j] = list of clouds ((n, 4) uint32; an empty one has a NULL pointer); outputs (caps[j] records, sentinel) back to back"""

    def __init__(self, jobs, caps=None):
        import lisreg
        self.jobs = jobs
        self.ns = [[len(c) for c in j] for j in jobs]
        self.sums = [sum(n) for n in self.ns]
        self.caps = list(caps) if caps is not None else [s + 2 for s in self.sums]
        flat = [c for j in jobs for c in j if len(c)]
        self.d_in = lisreg.DeviceArray(np.concatenate(flat) if flat else np.zeros((1, 4), u32))
        self.in_ptrs, at = [], 0
        for j in jobs:
            self.in_ptrs.append([])
            for c in j:
                self.in_ptrs[-1].append(self.d_in.ptr + 16 * at if len(c) else 0)
                at += len(c)
        self.out_off = np.concatenate([[0], np.cumsum(self.caps)]).astype(np.int64)
        self.total = max(int(self.out_off[-1]), 1)
        self.d_out = lisreg.DeviceArray(np.full((self.total, 4), SENT, u32))
        self.out_ptrs = [self.d_out.ptr + 16 * int(o) for o in self.out_off[:-1]]

    def raw(self):
        import lisreg
        lisreg.hip_runtime().hipDeviceSynchronize()                # lisreg_concat_device does not wait
        return self.d_out.download(self.total).view(u32)

    def free(self):
        self.d_in.free(); self.d_out.free()


def check_concat(ctx, jobs):
    A, B = ConcatArena(jobs), ConcatArena(jobs)
    totals = ctx.concat_device_batch(A.in_ptrs, A.ns, A.out_ptrs, A.caps)
    single_totals = [ctx.concat_device(B.in_ptrs[j], B.ns[j], B.out_ptrs[j]) for j in range(len(jobs))]
    got, ref = A.raw(), B.raw()
    assert totals == single_totals == A.sums
    assert got.tobytes() == ref.tobytes(), "differs from lisreg_concat_device"
    for j, clouds in enumerate(jobs):
        want = np.concatenate([c.reshape(-1, 4) for c in clouds] + [np.zeros((0, 4), u32)])
        o = got[int(A.out_off[j]):int(A.out_off[j + 1])]
        assert np.array_equal(o[:len(want)], want) and (o[len(want):] == SENT).all(), j
    A.free(); B.free()


def test_concat_batch_equals_the_single_calls(gpu_ctx):
    e = np.zeros((0, 4), u32)
    jobs = [[],                                                                        # k = 0
            [frame(777, 400)],                                                         # k = 1
            [frame(10 + 300 * i, 410 + i) for i in range(8)],                          # k = 8
            [frame(500, 420), e, e, frame(3, 421), e, frame(20000, 422)],              # empty clouds in the middle; more than one stride
            [e, e, e]]
    check_concat(gpu_ctx, jobs)
    check_concat(gpu_ctx, [[frame(1234, 430), frame(1, 431)]])                          # n_jobs = 1
    assert gpu_ctx.concat_device_batch([], [], [], []) == []
    rng = np.random.default_rng(5)
    check_concat(gpu_ctx, [[frame(int(rng.integers(0, 4)), 1000 + 3 * j + i) for i in range(int(rng.integers(0, 4)))] for j in range(1024)])


def test_concat_batch_refusals(gpu_ctx):
    import lisreg
    jobs = [[frame(100, 440), frame(50, 441)], [frame(70, 442)], [frame(30, 443), frame(30, 444), frame(30, 445)]]
    A = ConcatArena(jobs)

    def refused_c(in_ptrs, ns, out_ptrs, caps, word):
        with pytest.raises(lisreg.LisregError) as ex:
            gpu_ctx.concat_device_batch(in_ptrs, ns, out_ptrs, caps)
        assert ex.value.code == lisreg.ERR_ARG and word in str(ex.value), str(ex.value)
        assert (A.raw() == SENT).all(), "a refused call wrote"
    I, N, O, Cp = A.in_ptrs, A.ns, A.out_ptrs, A.caps
    refused_c([I[0], I[1] * 9, I[2]], [N[0], N[1] * 9, N[2]], O, Cp, "job 1")                   # k = 9
    refused_c(I, [N[0], [-1], N[2]], O, Cp, "job 1")
    refused_c([I[0], I[1], [I[2][0], 0, I[2][2]]], N, O, Cp, "job 2")                           # NULL input with n > 0
    refused_c(I, N, O, [Cp[0], Cp[1], 89], "job 2")                                             # capacity below the sum
    refused_c(I, N, [I[0][1], O[1], O[2]], Cp, "job 0")                                         # out on its own input
    refused_c(I, N, [O[0], O[0] + 16 * 151, O[2]], Cp, "job")                                   # out on another job's out (cap 152)
    refused_c(I, N, [O[0], I[2][1] + 16 * 29, O[2]], Cp, "job 1")                               # out on another job's input
    A2 = ConcatArena([[frame(1, 450)]] * 1025)
    with pytest.raises(lisreg.LisregError) as ex:
        gpu_ctx.concat_device_batch(A2.in_ptrs, A2.ns, A2.out_ptrs, A2.caps)
    assert "n_jobs" in str(ex.value) and (A2.raw() == SENT).all()
    assert gpu_ctx.concat_device_batch(I, N, O, Cp) == A.sums
    A.free(); A2.free()


# ---- the chain: split -> class grids -> concat, batch calls against single calls ------------------------------------------------------------
def test_chain_split_grids_concat(gpu_ctx):
    """three labelled frames through semantic_split_batch -> voxel_downsample_batch (keyframeInit's class leaves in split order:
    0.2 dynamic, 0.6 ground, 0.4 building, 0.05 pole, 0.6 outlier) -> concat_device_batch of (dynamic_down, building_down, ground_down)
    equal, byte for byte, the single split, the single grids and lisreg_concat_device"""
    import lisreg
    ctx = gpu_ctx
    D = lisreg.DeviceArray
    LEAF = [0.2, 0.6, 0.4, 0.05, 0.6]
    rng = np.random.default_rng(77)
    ns = [4000, 2 * T() + 100, 3000]
    recs = []
    for n in ns:
        r = np.zeros((n, 4), u32)
        r[:, :3] = (rng.uniform(-0.5, 0.5, (n, 3)) * np.array([40.0, 40.0, 6.0])).astype(np.float32).view(u32)
        r[:, 3] = rng.integers(0, 20, n)
        recs.append(r)

    def buffers():
        return dict(split=[[D(np.full((n, 4), SENT, u32)) for _ in range(5)] for n in ns],
                    down=[[D(np.full((n, 4), SENT, u32)) for _ in range(5)] for n in ns],
                    cat=[D(np.full((3 * n, 4), SENT, u32)) for n in ns])
    ins = [D(r) for r in recs]
    P, Q = buffers(), buffers()
    # batch calls
    cnt, st = ctx.semantic_split_batch_device([b.ptr for b in ins], ns, [[b.ptr for b in f] for f in P["split"]], [[n] * 5 for n in ns])
    assert st == [0, 0, 0]
    flat = [(f, k) for f in range(3) for k in range(5)]
    n_down, vst = ctx.voxel_downsample_batch_device([P["split"][f][k].ptr for f, k in flat], [cnt[f][k] for f, k in flat], [LEAF[k] for f, k in flat],
                                                    [P["down"][f][k].ptr for f, k in flat], [ns[f] for f, k in flat])
    assert vst == [0] * 15
    nd = [[n_down[5 * f + k] for k in range(5)] for f in range(3)]
    order = (0, 2, 1)                                              # dynamic_down + building_down + ground_down (currentCloudInit :866-889)
    tot = ctx.concat_device_batch([[P["down"][f][k].ptr for k in order] for f in range(3)], [[nd[f][k] for k in order] for f in range(3)],
                                  [b.ptr for b in P["cat"]], [3 * n for n in ns])
    # single calls
    for f in range(3):
        c1 = ctx.semantic_split_device(ins[f].ptr, ns[f], [b.ptr for b in Q["split"][f]], ns[f])
        assert c1 == cnt[f]
        d1 = [ctx.voxel_downsample_device(Q["split"][f][k].ptr, c1[k], LEAF[k], Q["down"][f][k].ptr, ns[f])[1] if c1[k] else 0 for k in range(5)]
        assert d1 == nd[f]
        assert ctx.concat_device([Q["down"][f][k].ptr for k in order], [d1[k] for k in order], Q["cat"][f].ptr) == tot[f] == sum(d1[k] for k in order)
    lisreg.hip_runtime().hipDeviceSynchronize()
    for f in range(3):
        assert 0 < tot[f] < ns[f]
        for k in range(5):
            assert P["split"][f][k].download(ns[f]).tobytes() == Q["split"][f][k].download(ns[f]).tobytes(), ("split", f, k)
            assert P["down"][f][k].download(ns[f]).tobytes() == Q["down"][f][k].download(ns[f]).tobytes(), ("grid", f, k)
        got = P["cat"][f].download(3 * ns[f])
        assert got.tobytes() == Q["cat"][f].download(3 * ns[f]).tobytes(), ("concat", f)
        assert (got.view(u32)[tot[f]:] == SENT).all()
    for b in ins + [x for S in (P, Q) for f in S["split"] + S["down"] for x in f] + P["cat"] + Q["cat"]:
        b.free()
