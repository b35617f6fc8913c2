"""What every family of the binding shares: status codes, the error, the library's loading and its signature tables, the
pointer / call helpers, and a Context's lifetime, error check, pinned pool and test aids."""

from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .. import build as _build

ABI_VERSION = 4

ERR_READ_NO_SEQ, ERR_READ_NO_NM, ERR_READ_ZERO_ALIGN, ERR_READ_NO_QUAL, ERR_READ_CIGAR_OVERRUN, \
    ERR_READ_BAD_CIGAR_OP = range(1, 7)
ERR_INVALID_ARG, ERR_NO_DEVICE, ERR_HIP, ERR_OUT_OF_MEMORY, ERR_UNSUPPORTED, ERR_BAD_LAYOUT = \
    -1, -2, -3, -4, -5, -6

vp, i32, i64, f64, cstr = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.c_char_p
P = C.POINTER


class MidasSnpsError(RuntimeError):
    def __init__(self, status: int, message: str, read_index: int = -1):
        super().__init__("midas_snps status %d: %s" % (status, message))
        self.status = status
        self.message = message
        self.read_index = read_index


_lib = None
_signatures = {}     # family tag -> {symbol: (restype, argtypes)}, in the order the modules registered them


def register(family: str, table: dict):
    """A module's entry points under a family tag: load_library() gives each its restype and argtypes, symbols(family) lists
    them.  A name is declared once in the whole package."""
    twice = [name for name in table for known in _signatures.values() if name in known]
    assert not twice, "declared twice: %s" % twice
    _signatures.setdefault(family, {}).update(table)


def symbols(family: str) -> list:
    """The names registered under a family tag."""
    return list(_signatures[family])


def library_path() -> str:
    return _build.LIB_PATH


def load_library(build_if_missing: bool = True):
    """dlopen the in-tree libmidas_snps_hip.so; raises if it cannot be found or built."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("MIDAS_SNPS_LIBRARY") or _build.LIB_PATH     # override: developer builds (tools/)
    if not os.path.exists(path):
        if not build_if_missing:
            raise MidasSnpsError(ERR_NO_DEVICE, "native library %s is missing (run `python -m midas_amd.build`)" % path)
        _build.build_native()
    lib = C.CDLL(path)
    for table in _signatures.values():
        for name, (res, args) in table.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is missing: fail loudly
            fn.restype = res
            fn.argtypes = args
    if lib.midas_snps_abi_version() != ABI_VERSION:
        raise MidasSnpsError(ERR_INVALID_ARG, "ABI version mismatch: library %d, binding %d"
                             % (lib.midas_snps_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


register('exported', {
    'midas_snps_abi_version': (i32, []),
    'midas_snps_cpu_budget': (i32, []),
    'midas_snps_status_string': (cstr, [i32]),
    'midas_snps_create': (i32, [i32, P(vp)]),
    'midas_snps_destroy': (None, [vp]),
    'midas_snps_last_error': (cstr, [vp]),
    'midas_snps_last_error_read': (i64, [vp]),
    'midas_snps_set_stream': (i32, [vp, vp]),
    'midas_snps_device_info': (i32, [vp, cstr, P(i32), P(i64)]),
    'midas_snps_host_alloc': (vp, [i64]),
    'midas_snps_host_free': (None, [vp]),
    'midas_snps_stream_rates': (i32, [vp, i64, i32, P(f64)]),
    'midas_snps_calibration_pass': (i32, [vp, i64]),
    'midas_snps_copy_rate': (i32, [vp, i64, i32, P(f64)]),
    'midas_snps_scan_u32': (i32, [vp, i64, vp, i32, vp, P(i32), P(i32)]),
    'midas_snps_sort_pairs': (i32, [vp, i64, i32, i32, vp, vp, vp, vp, P(i32), P(i32)]),
    'midas_snps_mt19937_stream': (i32, [vp, vp, i32, i64, i64, i64, vp, vp, vp, vp, vp]),
})


def ptr(a):
    """The array's address for the library; None or an empty array -> NULL."""
    return a.ctypes.data_as(vp) if a is not None and a.size else None


def addr(a):
    """ptr() for the sites where an empty array must keep its (valid) address: the entry point reads NULL as "this argument
    is not given", or refuses it, whatever the count beside it says.  None -> NULL."""
    return a.ctypes.data_as(vp) if a is not None else None


def text_buffer(wide: bool = False):
    """A buffer the library writes text into: the header's err256 / name256, or err1024 where it says so."""
    return C.create_string_buffer(1024) if wide else C.create_string_buffer(256)


def host_call(fn, *args, wide: bool = False, what: str = None):
    """fn(*args, err) for an entry point that reports through a message buffer: a status other than 0 raises MidasSnpsError
    with the buffer's text (or "<what> failed" when it is empty and `what` is given)."""
    err = text_buffer(wide)
    st = fn(*args, err)
    if st != 0:
        raise MidasSnpsError(st, err.value.decode(errors='replace') or (what + " failed" if what else ""))


def walk_stats(stats, rows: str = 'n_sites', side: bool = True) -> dict:
    """The slots every row-walking command fills, under the names the wrappers return: [0] rows read (as `rows`), [2] / [3]
    side cells, [7] groups, [9] group_rows, [10] chunk_bytes."""
    out = {rows: int(stats[0]), 'groups': int(stats[7]), 'group_rows': int(stats[9]), 'chunk_bytes': int(stats[10])}
    if side:
        out.update(side_freq=int(stats[2]), side_depth=int(stats[3]))
    return out


def mt_states(py_state=None, np_state=None):
    """(624 words, position) of Python's and numpy's global generators, or of the given random.getstate() /
    np.random.get_state() values."""
    import random
    ps = py_state if py_state is not None else random.getstate()
    ns = np_state if np_state is not None else np.random.get_state()
    return (np.array(ps[1][:624], np.uint32), int(ps[1][624])), (np.ascontiguousarray(ns[1], np.uint32), int(ns[2]))


class _Column:
    def __init__(self, owner, ptr, n, dtype):
        self._owner = owner
        dt = np.dtype(dtype)
        self.__array_interface__ = {'shape': (int(n),), 'typestr': dt.str, 'data': (int(ptr) if n else 0, True), 'version': 3} \
            if n else np.empty(0, dt).__array_interface__


def columns(owner, ptrs):
    """col(k, n, dtype): entry k of a native handle's pointer table as a read-only view that keeps `owner` alive."""
    return lambda k, n, dt: np.asarray(_Column(owner, ptrs[k] or 0, n, dt))


class _GenesOwner:
    def __init__(self, lib, h, close):
        self._lib, self._h, self._close = lib, h, close

    def __del__(self):
        if self._h:
            getattr(self._lib, self._close)(self._h)
            self._h = None


class PinnedPool:
    """Page-locked result buffers of a Context (midas_snps_host_alloc): grown on demand and REUSED across calls -- pinning
    a quarter of a gigabyte costs more than the copy it speeds up.  An array handed out under a key is overwritten by the
    next request for that key."""

    def __init__(self, lib):
        self._lib = lib
        self._bufs = {}

    def array(self, key, shape, dtype):
        dtype = np.dtype(dtype)
        nbytes = max(1, int(np.prod(shape)) * dtype.itemsize)
        ptr, cap = self._bufs.get(key, (None, 0))
        if cap < nbytes:
            if ptr:
                self._lib.midas_snps_host_free(C.c_void_p(ptr))
            ptr = self._lib.midas_snps_host_alloc(nbytes)
            if not ptr:
                self._bufs.pop(key, None)
                return np.empty(shape, dtype)          # no pinned memory: an ordinary array (staged copy)
            self._bufs[key] = (ptr, nbytes)
        return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype, count=int(np.prod(shape))).reshape(shape)

    def close(self):
        for ptr, _ in self._bufs.values():
            self._lib.midas_snps_host_free(C.c_void_p(ptr))
        self._bufs = {}


class _ContextCore:
    """A Context's handle, its error check and call helper, its pinned pool and the test aids; the commands come from the
    families' mixins (context.py)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        self._pool = None
        h = C.c_void_p()
        st = self._lib.midas_snps_create(int(device), C.byref(h))
        if st != 0:
            raise MidasSnpsError(st, "midas_snps_create(device=%d): %s"
                                 % (device, self._lib.midas_snps_status_string(st).decode()))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, '_pool', None):
            self._pool.close()
            self._pool = None
        if getattr(self, '_h', None):
            self._lib.midas_snps_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def pinned(self, key, shape, dtype):
        """A page-locked array owned by the context (see PinnedPool): valid until the same key is asked for again."""
        if self._pool is None:
            self._pool = PinnedPool(self._lib)
        return self._pool.array(key, shape, dtype)

    def _check(self, st: int, read_index: int = None):
        """read_index: the error's, where the call reported one itself (else the context's last)."""
        if st != 0:
            msg = self._lib.midas_snps_last_error(self._h).decode() or \
                self._lib.midas_snps_status_string(st).decode()
            raise MidasSnpsError(st, msg, int(self._lib.midas_snps_last_error_read(self._h) if read_index is None else read_index))

    def _check_bad(self, st: int, stats, n: int = 3):
        """_check() for a call that reports the place of a bad row: the error carries .bad = stats[4..4 + n), None where [4] is 0."""
        try:
            self._check(st)
        except MidasSnpsError as e:
            e.bad = tuple(int(x) for x in stats[4:4 + n]) if stats[4] else None
            raise

    def _device_call(self, fn, *args, tail=(), bad: int = 3, extra=None):
        """fn(handle, *args, stats[16], ms[8], *tail) -> (stats, ms).  A failure raises MidasSnpsError with .bad from `bad`
        slots of stats (_check_bad; 0: the call reports no row, plain _check).  extra = (name, slot, predicate): the error
        also carries .name = stats[slot] when the status is ERR_OUT_OF_MEMORY and predicate(stats[slot]) holds, else None."""
        stats, ms = np.zeros(16, np.int64), np.zeros(8, np.float32)
        st = fn(self._h, *args, ptr(stats), ptr(ms), *tail)
        try:
            if bad:
                self._check_bad(st, stats, bad)
            else:
                self._check(st)
        except MidasSnpsError as e:
            if extra is not None:
                name, slot, holds = extra
                setattr(e, name, int(stats[slot]) if st == ERR_OUT_OF_MEMORY and holds(stats[slot]) else None)
            raise
        return stats, ms

    def set_stream(self, hip_stream: Optional[int]):
        self._check(self._lib.midas_snps_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def scan_u32(self, v, in_place: bool = False, n=None):
        """The library's exclusive scan of 32-bit counters on v, between guard words (midas_snps_scan_u32; test aid).
        in_place: one device buffer is input and output.  n: the count handed over, len(v) unless given.
        -> (out uint32 [n], guards_ok, in_kept)."""
        v = np.ascontiguousarray(v, np.uint32).reshape(-1)
        out = np.zeros(v.size, np.uint32)
        ok, kept = C.c_int32(-1), C.c_int32(-1)
        # (addr: an empty v still goes up as a pointer with the count beside it)
        self._check(self._lib.midas_snps_scan_u32(self._h, v.size if n is None else int(n), addr(v), int(bool(in_place)), addr(out),
                                                  C.byref(ok), C.byref(kept)))
        return out, ok.value == 1, kept.value == 1

    def sort_pairs(self, key, val, bits: int, n=None):
        """The library's stable radix sort of (key, val) pairs by the keys' low `bits` bits, between guard words
        (midas_snps_sort_pairs; test aid).  key uint32 [n] below 2^bits; val uint32 [n] or float64 [n] (moved as bit patterns).
        n: the count handed over, len(key) unless given.
        -> (keys, values, which, guards_ok); which: 0 the result lay in the buffer pair the input went up to, 1 in the other."""
        key = np.ascontiguousarray(key, np.uint32).reshape(-1)
        val = np.ascontiguousarray(val).reshape(-1)
        if val.dtype not in (np.uint32, np.float64) or val.size != key.size:
            raise ValueError("sort_pairs: val must be uint32 or float64 and as long as key")
        out_key, out_val = np.zeros(key.size, np.uint32), np.zeros(val.size, val.dtype)
        which, ok = C.c_int32(-1), C.c_int32(-1)
        self._check(self._lib.midas_snps_sort_pairs(self._h, key.size if n is None else int(n), int(bits), int(val.dtype == np.float64),
                                                    addr(key), addr(val), addr(out_key), addr(out_val), C.byref(which), C.byref(ok)))
        return out_key, out_val, which.value, ok.value == 1

    def mt19937_stream(self, key, pos: int, n_words: int, per_launch: int = 0, bound: int = 0xFFFFFFFF):
        """The device's MT19937 generator from numpy's legacy state (key uint32 [624], pos), n_words words, per_launch a launch
        (midas_snps_mt19937_stream; test aid).  -> (raw uint32 [n], accepted uint8 [n], masked uint32 [n], key uint32 [624], pos)."""
        key = np.ascontiguousarray(key, np.uint32).reshape(-1)
        assert key.size == 624
        n = int(n_words)
        raw, flag, masked = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint32)
        key_out, pos_out = np.zeros(624, np.uint32), C.c_int32(-1)
        self._check(self._lib.midas_snps_mt19937_stream(self._h, ptr(key), int(pos), n, int(per_launch), int(bound), ptr(raw), ptr(flag),
                                                        ptr(masked), ptr(key_out), C.byref(pos_out)))
        return raw[:n], flag[:n], masked[:n], key_out, pos_out.value

    def copy_rate(self, nbytes: int = 1 << 30, reps: int = 10) -> float:
        """GB/s (read + written) of a device-to-device copy with the library's 16-bytes-per-lane copy kernel."""
        out = C.c_double(0.0)
        self._check(self._lib.midas_snps_copy_rate(self._h, int(nbytes), int(reps), C.byref(out)))
        return out.value

    def stream_rates(self, nbytes: int = 1 << 32, reps: int = 5):
        """GB/s of a saturating read stream, write stream and copy (read + written) over nbytes per buffer."""
        out = (C.c_double * 3)()
        self._check(self._lib.midas_snps_stream_rates(self._h, int(nbytes), int(reps), out))
        return {"read_GBps": out[0], "write_GBps": out[1], "copy_GBps": out[2]}

    def calibration_pass(self, nbytes: int = 1 << 30):
        """The known-byte-count kernels that calibrate FETCH_SIZE / WRITE_SIZE (run it under rocprofv3 --pmc)."""
        self._check(self._lib.midas_snps_calibration_pass(self._h, int(nbytes)))

    def device_info(self):
        name = text_buffer()
        ncu = C.c_int32(0)
        mem = C.c_int64(0)
        self._check(self._lib.midas_snps_device_info(self._h, name, C.byref(ncu), C.byref(mem)))
        return {'name': name.value.decode(), 'compute_units': ncu.value, 'hbm_bytes': mem.value}
