"""Source-view cache: what a frame derives from a source image alone, computed once per scene / time frame.

The reference's interactive dataset preloads the V views of a time frame (zjumocap/enerf_interactive.py:102-105,138-153) and
only selects and gathers per target camera (:205-217); static scenes draw every frame's S views from one fixed set too.  A
:class:`SourceCache` holds the HIP FeatureNet's three channels-last maps, the render texels and the cameras of those V views
(``enerf_source_cache_build``); ``Network.forward_cached`` then gathers the selected views by a device-resident index instead of
re-running the FeatureNet (``enerf_forward_cached``) — bit-identical to ``Network.forward`` on the same views.

    cache = net.cache_sources(inps, exts, ixts)              # once per time frame: (V,3,H,W), (V,4,4), (V,3,3)
    idx = lib.select_views(cam_points, c2w, S)               # per camera, on the device
    out = net.forward_cached(cache, idx, {"tar_ext": ..., "tar_ixt": ..., "near_far": ...})
"""
from __future__ import annotations

import torch

from .lib import MAX_LEVELS, SourceCacheStruct, cascade_struct


class SourceCache:
    """The tensors of one cache (owned here) + the ``enerf_source_cache_t`` that points into them.

    ``packed_gen`` is the generation of the network's packed weight images the maps were computed with: ``load_state_dict`` /
    ``.to()`` move it on, and ``Network.forward_cached`` refuses the cache from then on (rebuild it)."""

    def __init__(self, net, inps: torch.Tensor, exts: torch.Tensor, ixts: torch.Tensor, chunk: int = 0):
        if net.training:
            raise RuntimeError("cache_sources: call net.eval() first (the cache holds the inference FeatureNet's maps)")
        if net.feature_backend != "hip":
            raise ValueError("cache_sources needs feature_backend='hip' (the cache holds the HIP FeatureNet's channels-last maps)")
        if inps.dim() != 4 or inps.shape[1] != 3:
            raise ValueError(f"cache_sources: inps must be (V,3,H,W), got {tuple(inps.shape)}")
        V, _, H, W = inps.shape
        if tuple(exts.shape) != (V, 4, 4) or tuple(ixts.shape) != (V, 3, 3):
            raise ValueError(f"cache_sources: exts / ixts must be ({V},4,4) / ({V},3,3), got {tuple(exts.shape)} / {tuple(ixts.shape)}")
        lib, dev = net.lib, inps.device
        cas = cascade_struct(net.cfg)
        with torch.no_grad():
            packed = net._packed_weights("feature_net")
            l2s, floats = lib.source_cache_sizes(cas, V, H, W)
            # one allocation per buffer (each 16-byte aligned by the allocator); unused texel slots stay None
            self.buffers = [None if n == 0 else torch.empty((n,), dtype=torch.float32, device=dev) for n in floats]
            st = SourceCacheStruct(V=V, H=H, W=W, l2_stride=l2s)
            st.feat_l0, st.feat_l1, st.feat_l2 = (self.buffers[l].data_ptr() for l in range(3))
            for i in range(MAX_LEVELS):
                st.tex[i] = None if self.buffers[3 + i] is None else self.buffers[3 + i].data_ptr()
            st.exts, st.ixts = self.buffers[3 + MAX_LEVELS].data_ptr(), self.buffers[4 + MAX_LEVELS].data_ptr()
            lib.source_cache_build(st, inps.contiguous(), exts.contiguous(), ixts.contiguous(), packed, cas, chunk, net.options)
        self.struct = st
        self.V, self.H, self.W, self.l2_stride, self.device = V, H, W, l2s, dev
        self.packed_gen = net._packed_gen
        self._packed = packed                       # the weight image the maps came from (kept alive with the cache)

    @property
    def feats(self):
        """The three channels-last maps as views: (V,H/4,W/4,32), (V,H/2,W/2,16), (V,H,W,l2_stride)."""
        V, H, W = self.V, self.H, self.W
        return (self.buffers[0].view(V, H // 4, W // 4, 32), self.buffers[1].view(V, H // 2, W // 2, 16),
                self.buffers[2].view(V, H, W, self.l2_stride))

    def nbytes(self) -> int:
        return sum(b.numel() * 4 for b in self.buffers if b is not None)
