"""The RCCL communicator of the ranks' contexts."""

from __future__ import annotations

import ctypes as C

import numpy as np

from .core import P, addr, cstr, host_call, i32, i64, load_library, register, vp

register('exported', {
    'midas_comm_device_key': (i32, [vp, cstr]),
    'midas_comm_unique_id': (i32, [vp, cstr]),
    'midas_comm_probe': (i32, [P(i32), cstr]),
    'midas_comm_create': (i32, [vp, vp, i32, i32, P(vp), cstr]),
    'midas_comm_destroy': (None, [vp]),
    'midas_comm_all_gather': (i32, [vp, vp, vp, i64, cstr]),
    'midas_comm_all_to_all_v': (i32, [vp, vp, vp, vp, vp, cstr]),
})


class Comm:
    """An RCCL communicator of the ranks' contexts (comm.cpp): the all-gather of the summary rows over xGMI and the genes
    path's all-to-all, with no process group behind them.  midas_amd/dist.py makes one per job (the id travels through a file)."""

    def __init__(self, ctx: "Context", id128: bytes, rank: int, world: int):
        self._lib = ctx._lib
        self.rank, self.world = int(rank), int(world)
        h = C.c_void_p()
        buf = C.create_string_buffer(bytes(id128), 128)
        host_call(self._lib.midas_comm_create, ctx._h, C.cast(buf, C.c_void_p), self.rank, self.world, C.byref(h), what="midas_comm_create")
        self._h = h
        self._ctx = ctx          # (the communicator runs on the context's stream: keep it alive)

    @staticmethod
    def unique_id() -> bytes:
        lib = load_library()
        out = C.create_string_buffer(128)
        host_call(lib.midas_comm_unique_id, C.cast(out, C.c_void_p), what="midas_comm_unique_id")
        return out.raw

    @staticmethod
    def probe() -> int:
        """RCCL's version when this process can use it at all (midas_comm_probe); raises MidasSnpsError when it cannot."""
        lib = load_library()
        v = C.c_int32(0)
        host_call(lib.midas_comm_probe, C.byref(v), what="midas_comm_probe")
        return int(v.value)

    @staticmethod
    def device_key(ctx: "Context") -> str:
        out = C.create_string_buffer(64)
        ctx._check(ctx._lib.midas_comm_device_key(ctx._h, out))
        return out.value.decode()

    def close(self):
        if getattr(self, '_h', None):
            self._lib.midas_comm_destroy(self._h)
            self._h = None

    __del__ = close

    def all_gather(self, data: bytes):
        """every rank's `data` (the same length everywhere), by rank"""
        n = len(data)
        out = C.create_string_buffer(max(1, n * self.world))
        src = C.create_string_buffer(bytes(data), max(1, n))
        host_call(self._lib.midas_comm_all_gather, self._h, C.cast(src, C.c_void_p), C.cast(out, C.c_void_p), n, what="midas_comm_all_gather")
        raw = out.raw
        return [raw[r * n:(r + 1) * n] for r in range(self.world)]

    def all_to_all_v(self, parts, recv_bytes):
        """parts[r]: the bytes for rank r; recv_bytes[r]: how many come from rank r -> the bytes received, by source rank"""
        send = b"".join(bytes(p) for p in parts)
        sb = np.array([len(p) for p in parts], np.int64)
        rb = np.array([int(x) for x in recv_bytes], np.int64)
        out = C.create_string_buffer(max(1, int(rb.sum())))
        src = C.create_string_buffer(send, max(1, len(send)))
        host_call(self._lib.midas_comm_all_to_all_v, self._h, C.cast(src, C.c_void_p), addr(sb), C.cast(out, C.c_void_p), addr(rb),
                  what="midas_comm_all_to_all_v")
        raw, got, at = out.raw, [], 0
        for n in rb:
            got.append(raw[at:at + int(n)])
            at += int(n)
        return got
