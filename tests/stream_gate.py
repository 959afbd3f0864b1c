"""A caller's busy HIP stream for the tests: plain ctypes on lisreg.hip_runtime(), no torch, no kernel of its own.

`Gate.stall(stream, ms)` occupies a stream with a chain of large device-to-device copies between two scratch buffers: it ends by itself,
its length is bounded (STALL_CAP_MS), and the host goes on while it runs.  `Gate.late_input(stream, dst, real, decoy)` queues the stall
and, behind it, the copy real -> dst: whoever reads `dst` in the order of `stream` sees the real input, whoever reads it from another
stream (or from the null stream, which orders nothing against a hipStreamNonBlocking stream) still sees the decoy.

How long a stall has to be: a reader on a wrong stream starts, at the latest, one host-side call time after the producer was queued, so
the stall is 3 x t_call (t_call = the wall time of the same call on an idle stream, measured by the test after a warm-up), never below
MIN_COPIES calibrated copies and never above STALL_CAP_MS; a test whose 3 x t_call exceeds the cap has to shrink its shapes.

The two scratch buffers are COPY_BYTES (256 MiB) each, held for the module's life time: a copy has to be long enough (0.1 ms on an
MI355X) for the 8-copy floor to outlast the host's enqueue of the call under test, and short enough to calibrate well."""
import ctypes as C
import math
import time

import numpy as np

COPY_BYTES = 256 << 20
MIN_COPIES = 8
STALL_CAP_MS = 200.0
STREAM_NON_BLOCKING = 1
D2D, H2D = 3, 1
HIP_SUCCESS, HIP_NOT_READY = 0, 600


class HipError(RuntimeError):
    pass


class Gate:
    def __init__(self):
        import lisreg
        self.hip = lisreg.hip_runtime()
        self.hip.hipEventQuery.restype = C.c_int
        self._scratch = []
        for _ in range(2):
            p = C.c_void_p()
            self._ok(self.hip.hipMalloc(C.byref(p), C.c_size_t(COPY_BYTES)), "hipMalloc")
            self._ok(self.hip.hipMemset(p, 0, C.c_size_t(COPY_BYTES)), "hipMemset")
            self._scratch.append(p.value)
        self.ms_per_copy = None
        self.log = dict(copy_bytes=COPY_BYTES, ms_per_copy=None, max_copies=0, max_t_call_ms=0.0, max_stall_ms=0.0, stalls=0)
        self.calibrate()

    def _ok(self, rc, what):
        if rc != HIP_SUCCESS:
            raise HipError(f"{what} failed with HIP error {rc}")

    # ---- streams and events ----
    def stream_create(self) -> int:
        s = C.c_void_p()
        self._ok(self.hip.hipStreamCreateWithFlags(C.byref(s), C.c_uint(STREAM_NON_BLOCKING)), "hipStreamCreateWithFlags")
        return s.value

    def stream_destroy(self, stream: int):
        self._ok(self.hip.hipStreamDestroy(C.c_void_p(stream)), "hipStreamDestroy")

    def stream_sync(self, stream: int):
        self._ok(self.hip.hipStreamSynchronize(C.c_void_p(stream)), "hipStreamSynchronize")

    def copy_async(self, dst: int, src: int, nbytes: int, stream: int, kind: int = D2D):
        """hipMemcpyAsync: device to device, or (kind = H2D) from a lisreg.PinnedArray's ptr"""
        if nbytes:
            self._ok(self.hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), kind, C.c_void_p(stream)), "hipMemcpyAsync")

    def event_create(self) -> int:
        e = C.c_void_p()
        self._ok(self.hip.hipEventCreate(C.byref(e)), "hipEventCreate")
        return e.value

    def event_destroy(self, ev: int):
        self._ok(self.hip.hipEventDestroy(C.c_void_p(ev)), "hipEventDestroy")

    def event_record(self, ev: int, stream: int):
        self._ok(self.hip.hipEventRecord(C.c_void_p(ev), C.c_void_p(stream)), "hipEventRecord")

    def event_pending(self, ev: int) -> bool:
        rc = self.hip.hipEventQuery(C.c_void_p(ev))
        if rc not in (HIP_SUCCESS, HIP_NOT_READY):
            raise HipError(f"hipEventQuery failed with HIP error {rc}")
        return rc == HIP_NOT_READY

    def event_elapsed_ms(self, start: int, stop: int) -> float:
        ms = C.c_float(0)
        self._ok(self.hip.hipEventElapsedTime(C.byref(ms), C.c_void_p(start), C.c_void_p(stop)), "hipEventElapsedTime")
        return float(ms.value)

    def mark(self, stream: int) -> int:
        """a fresh event recorded on `stream` (the caller destroys it)"""
        ev = self.event_create()
        self.event_record(ev, stream)
        return ev

    # ---- the stall ----
    def _chain(self, stream: int, copies: int):
        a, b = self._scratch
        for k in range(copies):
            self.copy_async(b if k % 2 == 0 else a, a if k % 2 == 0 else b, COPY_BYTES, stream)

    def calibrate(self):
        """once per session, with events on an idle stream: the time of one copy of the chain"""
        s = self.stream_create()
        try:
            self._chain(s, 4)                     # first touches
            self.stream_sync(s)
            e0, e1 = self.event_create(), self.event_create()
            self.event_record(e0, s)
            self._chain(s, 16)
            self.event_record(e1, s)
            self.stream_sync(s)
            self.ms_per_copy = self.event_elapsed_ms(e0, e1) / 16
            self.event_destroy(e0); self.event_destroy(e1)
        finally:
            self.stream_destroy(s)
        if not self.ms_per_copy > 0:
            raise HipError(f"stall calibration gave {self.ms_per_copy} ms per copy")
        self.log["ms_per_copy"] = self.ms_per_copy

    def stall_ms_for(self, t_call_s: float) -> float:
        """3 x t_call, at least MIN_COPIES copies; more than the cap is the test's mistake (its shapes are too large)"""
        want = 3.0e3 * t_call_s
        self.log["max_t_call_ms"] = max(self.log["max_t_call_ms"], 1e3 * t_call_s)
        if want > STALL_CAP_MS:
            raise AssertionError(f"3 x t_call = {want:.1f} ms exceeds the {STALL_CAP_MS:.0f} ms cap of a stall: shrink the shapes of this test")
        return max(want, MIN_COPIES * self.ms_per_copy)

    def stall(self, stream: int, ms: float) -> int:
        """queue about `ms` milliseconds (capped) of copies on `stream`; returns the number of copies"""
        ms = min(float(ms), STALL_CAP_MS)
        copies = max(MIN_COPIES, int(math.ceil(ms / self.ms_per_copy)))
        self._chain(stream, copies)
        self.log["max_copies"] = max(self.log["max_copies"], copies)
        self.log["max_stall_ms"] = max(self.log["max_stall_ms"], copies * self.ms_per_copy)
        self.log["stalls"] += 1
        return copies

    def late_input(self, stream: int, dst, real, decoy, ms: float):
        """`dst` holds the decoy (a different valid input of the same size); behind a stall of `ms` on `stream` it receives the real one.
        dst / real / decoy: lisreg.DeviceArray of one size."""
        assert dst.nbytes == real.nbytes == decoy.nbytes and dst.ptr not in (real.ptr, decoy.ptr)
        self.stall(stream, ms)
        self.copy_async(dst.ptr, real.ptr, real.nbytes, stream)

    def wall(self, fn):
        """(result, seconds) of one host-side call"""
        t0 = time.perf_counter()
        r = fn()
        return r, time.perf_counter() - t0

    def report(self) -> str:
        g = self.log
        return (f"[stream_gate] copy {g['copy_bytes'] >> 20} MiB device to device, {g['ms_per_copy']:.4f} ms per copy; {g['stalls']} stalls, "
                f"longest {g['max_copies']} copies = {g['max_stall_ms']:.2f} ms; largest t_call {g['max_t_call_ms']:.3f} ms")

    def close(self):
        for p in self._scratch:
            self.hip.hipFree(C.c_void_p(p))
        self._scratch = []


def to_host(ptr: int, shape, dtype=np.float32) -> np.ndarray:
    """blocking D2H of a finished buffer (the caller has synchronised the stream that wrote it)"""
    import lisreg
    out = np.zeros(shape, dtype)
    if out.nbytes and lisreg.hip_runtime().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) != 0:
        raise HipError("hipMemcpy D2H failed")
    return out
