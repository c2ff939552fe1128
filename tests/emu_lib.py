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
