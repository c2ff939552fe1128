"""Source-view cache: what a frame derives from a source image alone, computed once per scene / time frame.

The reference's interactive dataset preloads the V views of a time frame (zjumocap/enerf_interactive.py:102-105,138-153) and
only selects and gathers per target camera (:205-217); static scenes draw every frame's S views from one fixed set too.  A
:class:`SourceCache` holds the HIP FeatureNet's three channels-last maps, the render texels and the cameras of those V views
(``enerf_source_cache_build``); ``Network.forward_cached`` then gathers the selected views by a device-resident index instead of
re-running the FeatureNet (``enerf_forward_cached``) — bit-identical to ``Network.forward`` on the same views.

    cache = net.cache_sources(inps, exts, ixts)              # once per time frame: (V,3,H,W), (V,4,4), (V,3,3)
    cache = net.cache_sources(u8, exts, ixts, masks, dilate=5)  # ... or (V,H,W,3) uint8 + (V,H,W) masks, ingested on the device
    cache.rebuild(next_u8, masks=next_masks, dilate=5)       # the next time frame, in place (enerf_amd/sequence.py overlaps it)
    cache = net.cache_sources(raw_u8, exts, rig.ixts, raw_masks, dilate=5, raw=rig)   # raw camera frames: enerf_amd/raw_ingest.py
    idx = lib.select_views(cam_points, c2w, S)               # per camera, on the device
    out = net.forward_cached(cache, idx, {"tar_ext": ..., "tar_ixt": ..., "near_far": ...})
"""
from __future__ import annotations

import torch

from .lib import MAX_LEVELS, SourceCacheStruct, cascade_struct


class SourceCache:
    """The tensors of one cache (owned here) + the ``enerf_source_cache_t`` that points into them.

    ``packed_gen`` is the generation of the network's packed weight images the maps were computed with: ``load_state_dict`` /
    ``.to()`` move it on, and ``Network.forward_cached`` refuses the cache from then on (:meth:`rebuild` it, or build a new one).

    ``inps`` is either the float image the reference's dataset keeps, (V,3,H,W) float32 in [-1,1], or what a camera / decoder
    delivers, (V,H,W,3) uint8 with optional foreground ``masks`` (V,H,W) uint8 / bool: that one goes through
    ``enerf_ingest_views_u8`` first (``dilate``: the box size of the mask dilation, 0 or odd 3..9).  With ``raw`` (a
    :class:`enerf_amd.raw_ingest.RawIngest`) uint8 input is the RAW frame, (V,Hraw,Wraw,3) with masks (V,Hraw,Wraw): it is
    undistorted, resized and cropped by ``enerf_ingest_raw_u8``, the cache's H and W are the rig's, and ``ixts`` are the rig's
    adjusted intrinsics (``raw.ixts``)."""

    def __init__(self, net, inps: torch.Tensor, exts: torch.Tensor, ixts: torch.Tensor, chunk: int = 0, masks=None, dilate: int = 0,
                 raw=None):
        self._raw = raw
        V, H, W = self._image_shape(inps)
        self._allocate(net, V, H, W, exts, ixts, chunk)
        self.rebuild(inps, masks=masks, dilate=dilate)

    @classmethod
    def empty(cls, net, V: int, H: int, W: int, exts: torch.Tensor, ixts: torch.Tensor, chunk: int = 0) -> "SourceCache":
        """The buffers of a cache for V views of HxW with nothing in them yet: :meth:`rebuild` fills them (``packed_gen`` is -1
        until then, so ``forward_cached`` refuses the empty cache)."""
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
            raise ValueError(f"cache_sources: inps must be (V,3,H,W) float32 or (V,H,W,3) uint8, got {inps.dtype} {tuple(inps.shape)}")
        return inps.shape[0], inps.shape[2], inps.shape[3]

    def _check_cameras(self, exts, ixts):
        V = self.V
        if tuple(exts.shape) != (V, 4, 4) or tuple(ixts.shape) != (V, 3, 3):
            raise ValueError(f"cache_sources: exts / ixts must be ({V},4,4) / ({V},3,3), got {tuple(exts.shape)} / {tuple(ixts.shape)}")

    def _allocate(self, net, V, H, W, exts, ixts, chunk):
        if net.training:
            raise RuntimeError("cache_sources: call net.eval() first (the cache holds the inference FeatureNet's maps)")
        if net.feature_backend != "hip":
            raise ValueError("cache_sources needs feature_backend='hip' (the cache holds the HIP FeatureNet's channels-last maps)")
        self.V, self.H, self.W = V, H, W
        self._check_cameras(exts, ixts)
        lib, dev = net.lib, exts.device
        cas = cascade_struct(net.cfg)
        l2s, floats = lib.source_cache_sizes(cas, V, H, W)
        # one allocation per buffer (each 16-byte aligned by the allocator); unused texel slots stay None
        self.buffers = [None if n == 0 else torch.empty((n,), dtype=torch.float32, device=dev) for n in floats]
        st = SourceCacheStruct(V=V, H=H, W=W, l2_stride=l2s)
        st.feat_l0, st.feat_l1, st.feat_l2 = (self.buffers[l].data_ptr() for l in range(3))
        for i in range(MAX_LEVELS):
            st.tex[i] = None if self.buffers[3 + i] is None else self.buffers[3 + i].data_ptr()
        st.exts, st.ixts = self.buffers[3 + MAX_LEVELS].data_ptr(), self.buffers[4 + MAX_LEVELS].data_ptr()
        self.struct = st
        self.l2_stride, self.device = l2s, dev
        self._net, self._cas, self._chunk = net, cas, chunk
        self._cams = (exts.contiguous(), ixts.contiguous())     # what a rebuild without cameras builds with again
        self.packed_gen = -1
        self._packed = None

    def rebuild(self, inps: torch.Tensor, exts=None, ixts=None, masks=None, dilate: int = 0, *, image=None, workspace=None):
        """Build again IN PLACE, for the next time frame: the same buffers and the same ``enerf_source_cache_t`` (a frame that still
        reads them must have finished — or be ordered in front by the stream / an event: :class:`enerf_amd.sequence.SequencePlayer`
        does that), on the current stream.  ``inps`` as in the constructor, of the cache's own V, H and W; ``exts`` / ``ixts`` None
        = the cameras the cache already holds.  Refreshes ``packed_gen`` to the network's current weights.  ``image`` (V,3,H,W)
        float32 and ``workspace`` (``EnerfLib.source_cache_build_workspace``) are optional preallocated scratch for the uint8 ingest
        and the FeatureNet; without them the call allocates its own."""
        net = self._net
        if net.training:
            raise RuntimeError("cache_sources: call net.eval() first (the cache holds the inference FeatureNet's maps)")
        if self._image_shape(inps) != (self.V, self.H, self.W):
            raise ValueError(f"SourceCache.rebuild: the cache holds V={self.V} views of {self.H}x{self.W}, got {tuple(inps.shape)}; "
                             "build a new cache for another V, H or W")
        if inps.device != self.device:
            raise ValueError("SourceCache.rebuild: the images must live on the cache's device")
        if (exts is None) != (ixts is None):
            raise ValueError("SourceCache.rebuild: pass exts and ixts together")
        if exts is not None:
            self._check_cameras(exts, ixts)
            self._cams = (exts.contiguous(), ixts.contiguous())
        lib = net.lib
        with torch.no_grad():
            if inps.dtype == torch.uint8 and self._raw is not None:
                inps = self._raw(inps, masks, dilate, out=image, lib=lib)
            elif inps.dtype == torch.uint8:
                inps = lib.ingest_views_u8(inps.contiguous(), masks, dilate, out=image)
            elif masks is not None or dilate:
                raise ValueError("cache_sources: masks / dilate belong to uint8 (V,H,W,3) images; a float image is taken as it is")
            packed = net._packed_weights("feature_net")
            lib.source_cache_build(self.struct, inps.contiguous(), self._cams[0], self._cams[1], packed, self._cas, self._chunk,
                                   net.options, workspace=workspace)
        self.packed_gen = net._packed_gen
        self._packed = packed                       # the weight image the maps came from (kept alive with the cache)
        return self

    @property
    def feats(self):
        """The three channels-last maps as views: (V,H/4,W/4,32), (V,H/2,W/2,16), (V,H,W,l2_stride)."""
        V, H, W = self.V, self.H, self.W
        return (self.buffers[0].view(V, H // 4, W // 4, 32), self.buffers[1].view(V, H // 2, W // 2, 16),
                self.buffers[2].view(V, H, W, self.l2_stride))

    def nbytes(self) -> int:
        return sum(b.numel() * 4 for b in self.buffers if b is not None)
