"""Source-view cache of the composite network: what its two FeatureNets make of a source image, computed once per time frame.

A viewer draws many target cameras from one fixed rig of V source views per time frame.  Both FeatureNets of
``network_composite`` read ``src_inps`` and neither depends on the target camera, so a :class:`CompositeSourceCache` holds, per
net, exactly what a composite frame reads — the channels-last feature map of every cascade level (the cost volumes' inputs) and the
texel image of every rendered level, the foreground's coloured by ``inps``, the background's by ``bg_inps`` — plus the V cameras
(``enerf_composite_cache_build``).  A feature map no cost volume reads is not kept: with ``actor1``'s two levels that is level_2,
the largest, which reaches the frame only through the full-resolution texels.  ``Network.forward_cached`` then gathers the selected
views by a device-resident index instead of running the FeatureNets (``enerf_forward_composite_cached``) — bit-identical to
``Network.forward`` on the same views.

    cache = net.cache_sources(inps, bg_inps, exts, ixts)      # once per time frame: (V,3,H,W) x 2, (V,4,4), (V,3,3)
    cache.rebuild(next_inps)                                   # the next time frame, in place; the background images stay
    idx = lib.select_views(cam_points, c2w, S)                 # per camera, on the device
    out = net.forward_cached(cache, idx, {"tar_ext": ..., "tar_ixt": ..., "near_far": ..., "bbox": ...})
"""
from __future__ import annotations

import torch

from .lib import COMPOSITE_CACHE_BUFFERS, MAX_LEVELS, CompositeCacheStruct, cascade_struct

BUFFER_NAMES = tuple(f"{net}_{kind}{i}" for net in ("fg", "bg") for kind in ("feat", "tex") for i in range(MAX_LEVELS)) + ("exts", "ixts")


class CompositeSourceCache:
    """The tensors of one cache (owned here, one per buffer) + the ``enerf_composite_cache_t`` that points into them.

    ``packed_gen`` is the generation of the network's packed weight images the maps were computed with: ``load_state_dict`` /
    ``.to()`` move it on, and ``Network.forward_cached`` refuses the cache from then on (:meth:`rebuild` it, or build a new one).

    ``inps`` / ``bg_inps`` are either float images, (V,3,H,W) float32 in [-1,1], or what a camera / decoder delivers, (V,H,W,3)
    uint8: those go through ``enerf_ingest_views_u8`` (no mask) first.  The reference's ``read_data_bg`` reads one static
    background image per camera, so a :meth:`rebuild` without ``bg_inps`` keeps the images of the last build.  With ``raw`` (a
    :class:`enerf_amd.raw_ingest.RawIngest`) uint8 images, the background's too, are RAW frames (V,Hraw,Wraw,3): they go through
    ``enerf_ingest_raw_u8`` (read_data / read_data_bg of enerf_outdoor/enerf.py:107-152), the cache's H and W are the rig's and
    ``ixts`` are ``raw.ixts``."""

    def __init__(self, net, inps: torch.Tensor, bg_inps: torch.Tensor, exts: torch.Tensor, ixts: torch.Tensor, chunk: int = 0, raw=None):
        self._raw = raw
        V, H, W = self._image_shape(inps)
        self._allocate(net, V, H, W, exts, ixts, chunk)
        self.rebuild(inps, bg_inps)

    @classmethod
    def empty(cls, net, V: int, H: int, W: int, exts: torch.Tensor, ixts: torch.Tensor, chunk: int = 0) -> "CompositeSourceCache":
        """The buffers of a cache for V views of HxW with nothing in them yet: :meth:`rebuild` (with ``bg_inps``) fills them
        (``packed_gen`` is -1 until then, so ``forward_cached`` refuses the empty cache)."""
        self = cls.__new__(cls)
        self._raw = None
        self._allocate(net, V, H, W, exts, ixts, chunk)
        return self

    def _image_shape(self, inps):
        if self._raw is not None and inps.dtype == torch.uint8:
            self._raw.check_frame(inps, what="cache_sources (raw)")
            return inps.shape[0], self._raw.H, self._raw.W
        if inps.dim() == 4 and inps.dtype == torch.uint8 and inps.shape[3] == 3:
            return inps.shape[0], inps.shape[1], inps.shape[2]
        if inps.dim() != 4 or inps.shape[1] != 3 or inps.dtype == torch.uint8:
            raise ValueError(f"cache_sources: images must be (V,3,H,W) float32 or (V,H,W,3) uint8, got {inps.dtype} {tuple(inps.shape)}")
        return inps.shape[0], inps.shape[2], inps.shape[3]

    def _check_cameras(self, exts, ixts):
        V = self.V
        if tuple(exts.shape) != (V, 4, 4) or tuple(ixts.shape) != (V, 3, 3):
            raise ValueError(f"cache_sources: exts / ixts must be ({V},4,4) / ({V},3,3), got {tuple(exts.shape)} / {tuple(ixts.shape)}")

    def _allocate(self, net, V, H, W, exts, ixts, chunk):
        if net.training:
            raise RuntimeError("cache_sources: call net.eval() first (the cache holds the inference FeatureNets' maps)")
        self.V, self.H, self.W = int(V), int(H), int(W)
        self._check_cameras(exts, ixts)
        lib, dev = net.lib, exts.device
        cas = cascade_struct(net.cfg)
        floats = lib.composite_cache_sizes(cas, self.V, self.H, self.W)
        # one allocation per buffer (each 16-byte aligned by the allocator); slots the frame does not read stay None
        self.buffers = [None if n == 0 else torch.empty((n,), dtype=torch.float32, device=dev) for n in floats]
        st = CompositeCacheStruct(V=self.V, H=self.H, W=self.W)
        for k, field in enumerate(("fg_feat", "fg_tex", "bg_feat", "bg_tex")):
            for i in range(MAX_LEVELS):
                b = self.buffers[k * MAX_LEVELS + i]
                getattr(st, field)[i] = None if b is None else b.data_ptr()
        st.exts, st.ixts = self.buffers[-2].data_ptr(), self.buffers[-1].data_ptr()
        assert len(self.buffers) == COMPOSITE_CACHE_BUFFERS
        self.struct = st
        self.device = dev
        self._net, self._cas, self._chunk = net, cas, chunk
        self._cams = (exts.contiguous(), ixts.contiguous())     # what a rebuild without cameras builds with again
        self._bg = None                                          # the background images of the last build, (V,3,H,W) float32
        self.packed_gen = -1
        self._packed = None

    def _image(self, lib, inps, what):
        if self._image_shape(inps) != (self.V, self.H, self.W):
            raise ValueError(f"CompositeSourceCache.rebuild: the cache holds V={self.V} views of {self.H}x{self.W}, got {what} "
                             f"{tuple(inps.shape)}; build a new cache for another V, H or W")
        if inps.device != self.device:
            raise ValueError("CompositeSourceCache.rebuild: the images must live on the cache's device")
        if inps.dtype == torch.uint8 and self._raw is not None:
            return self._raw(inps, lib=lib)
        if inps.dtype == torch.uint8:
            return lib.ingest_views_u8(inps.contiguous())
        return inps.contiguous()

    def rebuild(self, inps: torch.Tensor, bg_inps=None, exts=None, ixts=None, *, workspace=None):
        """Build again IN PLACE, for the next time frame, on the current stream: the same buffers and the same
        ``enerf_composite_cache_t`` (a frame that still reads them must have finished, or be ordered in front by the stream).
        ``inps`` / ``bg_inps`` as in the constructor, of the cache's own V, H and W; ``bg_inps`` None = the background images of the
        last build; ``exts`` / ``ixts`` None = the cameras the cache already holds.  Refreshes ``packed_gen`` to the network's current
        weights.  ``workspace`` (``EnerfLib.composite_cache_build_workspace``) is optional preallocated scratch."""
        net = self._net
        if net.training:
            raise RuntimeError("cache_sources: call net.eval() first (the cache holds the inference FeatureNets' maps)")
        if (exts is None) != (ixts is None):
            raise ValueError("CompositeSourceCache.rebuild: pass exts and ixts together")
        if bg_inps is None and self._bg is None:
            raise ValueError("CompositeSourceCache.rebuild: an empty cache has no background images yet: pass bg_inps")
        lib = net.lib
        with torch.no_grad():
            img = self._image(lib, inps, "inps")
            bg = self._bg if bg_inps is None else self._image(lib, bg_inps, "bg_inps")
            if exts is not None:
                self._check_cameras(exts, ixts)
                self._cams = (exts.contiguous(), ixts.contiguous())
            packed = (net._packed_weights("feature_net"), net._packed_weights("feature_net_bg"))
            lib.composite_cache_build(self.struct, img, bg, self._cams[0], self._cams[1], packed[0], packed[1], self._cas, self._chunk,
                                      net.options, workspace=workspace)
        self._bg = bg
        self.packed_gen = net._packed_gen
        self._packed = packed                       # the weight images the maps came from (kept alive with the cache)
        return self

    def named_buffers(self):
        """``{name: flat tensor}`` of the buffers the cache holds: ``fg_feat0``, ``fg_tex1``, ``bg_feat0``, ..., ``exts``, ``ixts``."""
        return {n: b for n, b in zip(BUFFER_NAMES, self.buffers) if b is not None}

    def nbytes(self) -> int:
        return sum(b.numel() * 4 for b in self.buffers if b is not None)
