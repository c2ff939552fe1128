"""Test helper: the CPU-emulated twin of libenerf_hip.so (same kernel sources, g++ + tests/emu/hip_emu.h)."""
import contextlib
import functools

from enerf_amd.lib import EnerfLib
from emu.build_emu import build

EMU_DEFAULT_CUS = 256


@functools.lru_cache(maxsize=1)
def emu_lib() -> EnerfLib:
    return EnerfLib(build())


@contextlib.contextmanager
def emu_cu_count(lib: EnerfLib, n: int):
    """The emulated library sizes its launch geometry for ``n`` CUs inside the block (256 again after it), so that persistent
    kernels — a grid capped by the CU count, each wave or block looping over tiles — run their second and later passes on CPU.

    Limits: workspace sizes depend on the CU count too, so a ``Network`` whose frame workspace was sized under one count must not
    be reused under another; and the count must not change between ``wgrad_reduce_begin`` and the flush of a ``wgrad_reduce_batch``
    (the deferred second stages are sized when they are recorded)."""
    lib.dll.emu_set_cu_count(int(n))
    try:
        yield
    finally:
        lib.dll.emu_set_cu_count(EMU_DEFAULT_CUS)


@contextlib.contextmanager
def emu_trace(lib: EnerfLib, main_stream: int = 0):
    """Record what the calling thread enqueues inside the block (tests/emu/hip_emu.h); yields a list that is filled when the block
    ends, in enqueue order, with
        ("launch", kernel, (gx, gy, gz), stream)      every ENERF_LAUNCH / ENERF_LAUNCH_SIMPLE; kernel as written at the call site
        ("record", event, stream)                     the frame's side lane (csrc/side_lane.h): event recorded on stream
        ("wait", event, stream)                       stream waits for event
    Streams are "main" (the handle ``main_stream``: the caller's), "side" and "render" (the lane's), or the handle in hex."""
    import ctypes as C
    dll = lib.dll
    dll.emu_trace_read.restype = C.c_longlong
    dll.emu_trace_read.argtypes = [C.c_char_p, C.c_longlong]
    out = []
    dll.emu_trace_reset(1)
    try:
        yield out
    finally:
        n = dll.emu_trace_read(None, 0)
        buf = C.create_string_buffer(max(int(n), 1))
        dll.emu_trace_read(buf, n)
        dll.emu_trace_reset(0)
        rows = [ln.split("\t") for ln in buf.raw[:n].decode().splitlines()]
        names = {"%x" % main_stream: "main"}
        names.update({r[3]: r[2] for r in rows if r[0] != "launch"})
        for r in rows:
            if r[0] == "launch":
                out.append(("launch", r[1], (int(r[2]), int(r[3]), int(r[4])), names.get(r[5], r[5])))
            else:
                out.append((r[0], r[1], r[2]))
