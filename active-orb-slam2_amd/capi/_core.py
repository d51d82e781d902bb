"""Loading of lib/libaos2.so (built by csrc/Makefile) and the bench harness around it: recording of call lists, graph replay, the
HIP runtime's copies and the native step runner.  The library and the open recording are globals of this file alone."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._abi import AOS2_OK, PROTOTYPES, _Call

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB = None


class LibraryMissing(RuntimeError):
    pass


class AosError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"aos2 error {code}: {msg}")
        self.code = code


def _declare(L, prototypes, path):
    """restype and argtypes of every function of `prototypes` (name -> (restype, argtypes)) set on the loaded library L; a symbol the
    library does not export is an error that names it"""
    for name, (restype, argtypes) in prototypes.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise LibraryMissing(f"{path} does not export {name}: rebuild it") from None
        fn.restype, fn.argtypes = restype, argtypes
    return L


def lib_path():
    return os.environ.get("AOS2_LIB") or os.path.join(_PKG, "lib", "libaos2.so")


def lib():
    global _LIB
    if _LIB is None:
        p = lib_path()
        if not os.path.exists(p):
            raise LibraryMissing(f"{p} not found: build it with `make -C {_PKG}/csrc` "
                                 "(__graft_entry__.build()); there is no fallback path")
        _LIB = _RecLib(_declare(C.CDLL(p), PROTOTYPES, p))
    return _LIB


# ---- recording (bench harness): the calls of a job captured instead of executed, for the native step runner (csrc/host_runner.cpp)
# the functions a recorded job may consist of: work that is enqueued / solved / waited for.  Everything else (getters, stream handles,
# setters) executes at once even while a recording is open
_RECORDABLE = {
    "aos2_frames_set_pose", "aos2_extractor_extract_batch_device_async", "aos2_frames_build", "aos2_frames_build_stereo",
    "aos2_compute_stereo_matches_device_async", "aos2_frames_search_by_projection_last", "aos2_frames_pose_optimization",
    "aos2_frames_discard_outliers", "aos2_frames_search_local_points", "aos2_frames_wait", "aos2_extractor_wait",
    "aos2_extractor_stream_wait", "aos2_extractor_wait_for_stream", "aos2_vocabulary_transform_device", "aos2_matcher_search_by_bow_frames",
    "aos2_frames_search_for_triangulation", "aos2_frames_fuse", "aos2_lba_solve_batch", "aos2_extractor_pack_slots",
    "hipMemcpyAsync", "hipStreamSynchronize", "hipStreamWaitEvent", "hipEventRecord", "hipMemcpy",
}
_REC = None   # the open recording (a list), or None


class recording:
    """with capi.recording() as calls: ...   -- the recordable C calls made inside are appended to `calls` (not executed; they
    "return" AOS2_OK); calls.keep holds every argument object alive; calls.array() is the aos2_call_t array for the runner"""

    class _List(list):
        def __init__(self):
            super().__init__()
            self.keep = []
            self.names = []   # function name per call (diagnostics)

        def array(self):
            a = (_Call * max(1, len(self)))()
            for i, c in enumerate(self):
                a[i] = c
            return a

    def __enter__(self):
        global _REC
        assert _REC is None, "recordings do not nest"
        _REC = recording._List()
        return _REC

    def __exit__(self, *exc):
        global _REC
        _REC = None
        return False


def _record(fn, name, args):
    import struct
    at = fn.argtypes
    if at is None or len(at) != len(args):
        raise TypeError(f"recording {name}: the function needs argtypes for every argument")
    c = _Call()
    c.fn = C.cast(fn, C.c_void_p).value
    ni = nf = 0
    for a, t in zip(args, at):
        if t is C.c_float or t is C.c_double:
            v = float(a.value if isinstance(a, C._SimpleCData) else a)
            bits = struct.unpack("<I", struct.pack("<f", v))[0] if t is C.c_float else struct.unpack("<Q", struct.pack("<d", v))[0]
            if nf >= 8:
                raise TypeError(f"recording {name}: more than 8 floating-point arguments")
            c.fargs[nf] = bits
            nf += 1
            continue
        if a is None:
            v = 0
        elif isinstance(a, (int, np.integer)):
            v = int(a)
        elif isinstance(a, C._SimpleCData):
            v = a.value or 0
        else:
            v = C.cast(a, C.c_void_p).value or 0   # pointers, arrays, byref()
        if ni >= 24:
            raise TypeError(f"recording {name}: more than 24 integer arguments")
        if v >= 1 << 63:
            v -= 1 << 64
        c.iargs[ni] = v
        ni += 1
    c.n_int, c.n_fp = ni, nf
    _REC.append(c)
    _REC.keep.append(args)
    _REC.names.append(name)
    return AOS2_OK


class _RecLib:
    """the loaded library; a recordable function called while a recording is open is captured instead of executed"""

    def __init__(self, L):
        object.__setattr__(self, "_L", L)
        object.__setattr__(self, "_w", {})
        object.__setattr__(self, "_names", frozenset(_RECORDABLE))   # (kept here: module globals are gone when handles close at exit)

    def __getattr__(self, name):
        w = self._w.get(name)
        if w is None:
            fn = getattr(self._L, name)
            if name in self._names:
                def w(*args, _fn=fn, _name=name):
                    if _REC is None:
                        return _fn(*args)
                    return _record(_fn, _name, args)
                w.argtypes_of = fn
            else:
                w = fn
            self._w[name] = w
        return w


class Graph:
    """include/aos2.h "Replay of a fixed call sequence": the calls made inside `with Graph.capture(stream) as g:` are recorded
    (nothing runs); g.launch() enqueues them all with one call"""

    def __init__(self, stream):
        self.L, self.stream, self.h = lib(), stream, None

    @classmethod
    def capture(cls, stream):
        return cls(stream)

    def __enter__(self):
        _check(self.L.aos2_capture_begin(self.stream))
        return self

    def __exit__(self, et, ev, tb):
        h = C.c_void_p()
        st = self.L.aos2_capture_end(self.stream, C.byref(h))
        if et is None:
            _check(st)
            self.h = h
        elif st == AOS2_OK and h:
            self.L.aos2_graph_destroy(h)   # (the body failed: what was recorded until then is dropped)
        return False

    def nodes(self):
        return int(self.L.aos2_graph_nodes(self.h))

    def launch(self, stream=None):
        _check(self.L.aos2_graph_launch(self.h, self.stream if stream is None else stream))

    def close(self):
        if self.h:
            self.L.aos2_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_HIP = None


def hip_runtime():
    """libamdhip64 (the runtime the library itself links) for the harness's own copies: hipMemcpyAsync & co, recordable"""
    global _HIP
    if _HIP is None:
        vp, ci, pvp = C.c_void_p, C.c_int, C.POINTER(C.c_void_p)
        _HIP = _RecLib(_declare(C.CDLL("libamdhip64.so"), {
            "hipMemcpyAsync": (ci, [vp, vp, C.c_size_t, ci, vp]), "hipMemcpy": (ci, [vp, vp, C.c_size_t, ci]),
            "hipStreamSynchronize": (ci, [vp]), "hipStreamWaitEvent": (ci, [vp, vp, C.c_uint]), "hipEventRecord": (ci, [vp, vp]),
            "hipStreamCreateWithFlags": (ci, [pvp, C.c_uint]), "hipEventCreateWithFlags": (ci, [pvp, C.c_uint]),
            "hipHostMalloc": (ci, [pvp, C.c_size_t, C.c_uint])}, "libamdhip64.so"))
    return _HIP


class Runner:
    """csrc/host_runner.cpp: the step schedule of bench.py on native threads over recorded call lists"""
    PIPE_WAIT, PIPE_STEP, KF_JOB, LBA_JOB = 0, 1, 2, 3

    def __init__(self, n_pipes, n_lba):
        p = os.path.join(os.path.dirname(lib_path()), "libaos2_runner.so")
        if not os.path.exists(p):
            raise LibraryMissing(f"{p} not found: build it with `make -C {_PKG}/csrc`")
        vp, ci = C.c_void_p, C.c_int
        R = _declare(C.CDLL(p), {
            "aos2_runner_create": (vp, [ci, ci]), "aos2_runner_destroy": (ci, [vp]), "aos2_runner_set_list": (ci, [vp, ci, ci, vp, ci]),
            "aos2_runner_step": (ci, [vp, ci]), "aos2_runner_run": (ci, [vp, ci, ci]), "aos2_runner_sync": (ci, [vp]),
            "aos2_runner_error": (C.c_char_p, [vp]), "aos2_runner_reset_stats": (ci, [vp]), "aos2_runner_stats": (ci, [vp, ci, vp, ci]),
            "aos2_runner_set_lba_every": (ci, [vp, ci]), "aos2_runner_last_lba": (ci, [vp])}, p)
        self.R = R
        self.h = R.aos2_runner_create(int(n_pipes), int(n_lba))
        if not self.h:
            raise ValueError("aos2_runner_create")
        self._keep = {}

    def __del__(self):
        if getattr(self, "h", None):
            self.R.aos2_runner_destroy(self.h)
            self.h = None

    def set_list(self, kind, index, calls):
        """calls: a recording (or None / empty: the job is skipped)"""
        n = len(calls) if calls else 0
        arr = calls.array() if n else None
        if self.R.aos2_runner_set_list(self.h, kind, index, C.cast(arr, C.c_void_p) if n else None, n) != 0:
            raise ValueError("aos2_runner_set_list")
        self._keep[(kind, index)] = (calls, arr)

    def _st(self, st):
        if st != 0:
            raise AosError(st, self.R.aos2_runner_error(self.h).decode() + ": " + lib().aos2_last_error().decode(errors="replace"))

    def set_lba_every(self, n):
        """a LocalBA job every n steps (its list then solves the windows of n steps in one call)"""
        if self.R.aos2_runner_set_lba_every(self.h, int(n)) != 0:
            raise ValueError("aos2_runner_set_lba_every")

    def last_lba(self):
        return int(self.R.aos2_runner_last_lba(self.h))

    def step(self, s):
        self._st(self.R.aos2_runner_step(self.h, int(s)))

    def run(self, s0, n):
        self._st(self.R.aos2_runner_run(self.h, int(s0), int(n)))

    def sync(self):
        self._st(self.R.aos2_runner_sync(self.h))

    def reset_stats(self):
        self.R.aos2_runner_reset_stats(self.h)

    def stats(self, which):
        n = self.R.aos2_runner_stats(self.h, which, None, 0)
        a = np.zeros(max(n, 1), np.float64)
        self.R.aos2_runner_stats(self.h, which, _p(a), n)
        return a[:n]


def _check(st, ok=(AOS2_OK,)):
    if st not in ok:
        raise AosError(st, lib().aos2_last_error().decode(errors="replace"))
    return st


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class _Handle:
    """a handle of the library: aos2_<KIND>_create(..., &h) makes it; close(), or the last reference, destroys it"""
    KIND = None

    def _create(self, *args):
        self.L = lib()
        h = C.c_void_p()
        _check(getattr(self.L, "aos2_%s_create" % self.KIND)(*args, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            getattr(self.L, "aos2_%s_destroy" % self.KIND)(self.h)
            self.h = None

    def __del__(self):
        self.close()


class _HostBlock:
    """page-locked host allocation (aos2_host_alloc), released with the last array that views it"""

    def __init__(self, nbytes):
        self.L = lib()
        p = C.c_void_p()
        _check(self.L.aos2_host_alloc(C.byref(p), max(int(nbytes), 1)))
        self.p = p.value

    def __del__(self):
        if getattr(self, "p", None) and C is not None:   # (at interpreter shutdown the module globals may already be gone)
            self.L.aos2_host_free(C.c_void_p(self.p))
            self.p = None


def host_empty(shape, dtype=np.uint8):
    """uninitialised numpy array in page-locked host memory (for Extractor.extract_batch inputs / outputs)"""
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) * dt.itemsize
    blk = _HostBlock(n)
    buf = (C.c_uint8 * max(n, 1)).from_address(blk.p)
    buf._block = blk   # the ctypes view keeps the allocation alive; numpy keeps the view alive (.base)
    return np.frombuffer(buf, dtype=dt, count=int(np.prod(shape))).reshape(shape)


def device_count():
    return lib().aos2_device_count()


def device_local_cpus(device=0):
    """set of host CPUs on the device's NUMA node (aos2_device_local_cpus; empty when the platform does not say)"""
    buf = C.create_string_buffer(8192)
    _check(lib().aos2_device_local_cpus(int(device), buf, len(buf)))
    cpus = set()
    for part in buf.value.decode().split(","):
        part = part.strip()
        if not part:
            continue
        a, _, b = part.partition("-")
        cpus.update(range(int(a), int(b or a) + 1))
    return cpus


def bind_to_device_node(device=0):
    """sched_setaffinity of the calling thread (and the threads it creates from now on) to the device's local CPUs, intersected with
    the CPUs the process may use; returns the CPU count bound to, 0 when nothing was changed"""
    try:
        cpus = device_local_cpus(device) & os.sched_getaffinity(0)
    except (AosError, OSError):
        return 0
    if not cpus:
        return 0
    os.sched_setaffinity(0, cpus)
    return len(cpus)
