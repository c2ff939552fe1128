"""Raw camera frames in front of the source-view caches: undistort, area resize, crop — one device call per time frame.

The reference's datasets do this on the host for every view of every time frame (zjumocap/enerf_interactive.py:116-135,
zjumocap/enerf.py:141-149, enerf_outdoor/enerf.py:129-152): ``cv2.undistort`` of image and mask, a resize by ``input_ratio``
(``INTER_AREA`` for the image, ``INTER_NEAREST`` for the mask), the mask dilated in front and zeroed behind, and — outdoor — an
asymmetric crop to ``input_h_w`` with the intrinsics moved along.  A :class:`RawIngest` holds what is fixed for a rig (raw size,
intrinsics, distortion, ratio, crop) and turns a raw uint8 frame into the (V,3,H,W) float image with ``enerf_ingest_raw_u8``:

    rig = RawIngest(K, D, 1024, 1366, input_ratio=0.75, crop=RawIngest.outdoor_crop(768, 1024, 704, 1024) + (704, 1024))
    cache = net.cache_sources(raw_u8, exts, rig.ixts, raw=rig)           # (V,1024,1366,3) uint8 in, a cache of rig.H x rig.W
    cache.rebuild(next_raw_u8)
    player = SequencePlayer(net, exts, rig.ixts, rig.H, rig.W, dilate=5, raw=rig)

The arithmetic is specified in include/enerf_hip.h; it is pinned to a float64 evaluation of that model, NOT to OpenCV's bits
(OpenCV rounds its remap coordinates to 1/32 pixel, drops area overlaps under 1e-3 pixel and sums in another order).
"""
from __future__ import annotations

import torch


class RawIngest:
    """``ixts`` (V,3,3) raw intrinsics, ``dist`` (V,5) = (k1,k2,p1,p2,k3) or None (no undistortion: the bilinear step is skipped
    altogether), raw frames of ``Hraw`` x ``Wraw``, ``input_ratio`` in [0.25, 1], ``crop`` = (y0, x0, H, W) in the resized image or
    None (all of it).  ``.H`` / ``.W``: the output size; ``.ixts``: the intrinsics of the output image (``K[:2] *= input_ratio``,
    ``cx -= x0``, ``cy -= y0``), float32 on the device of ``ixts``, computed once in float64.  ``lib``: the
    :class:`enerf_amd.lib.EnerfLib` a call runs on when it names none (None: libenerf_hip.so); the caches and the player pass their
    network's."""

    def __init__(self, ixts: torch.Tensor, dist, Hraw: int, Wraw: int, input_ratio: float = 1.0, crop=None, lib=None):
        if ixts.dim() != 3 or tuple(ixts.shape[1:]) != (3, 3):
            raise ValueError(f"RawIngest: ixts must be (V,3,3), got {tuple(ixts.shape)}")
        V = ixts.shape[0]
        if dist is not None and (tuple(dist.shape) != (V, 5) or dist.device != ixts.device):
            raise ValueError(f"RawIngest: dist must be ({V},5) = (k1,k2,p1,p2,k3) on the device of ixts, got {tuple(dist.shape)}")
        if not 0.25 <= float(input_ratio) <= 1.0:
            raise ValueError(f"RawIngest: input_ratio={input_ratio} (0.25..1)")
        self.V, self.Hraw, self.Wraw, self.input_ratio = V, int(Hraw), int(Wraw), float(input_ratio)
        self.Hs, self.Ws = self.resized(self.Hraw, self.Wraw, self.input_ratio, lib)
        y0, x0, H, W = (0, 0, self.Hs, self.Ws) if crop is None else (int(c) for c in crop)
        if H < 1 or W < 1 or y0 < 0 or x0 < 0 or y0 + H > self.Hs or x0 + W > self.Ws:
            raise ValueError(f"RawIngest: crop (y0={y0}, x0={x0}, {H}x{W}) leaves the resized image {self.Hs}x{self.Ws}")
        self.crop, self.H, self.W = (y0, x0, H, W), H, W
        self.device = ixts.device
        self.raw_ixts = ixts.detach().to(torch.float32).contiguous()
        self.dist = None if dist is None else dist.detach().to(torch.float32).contiguous()
        k = ixts.detach().double().clone()
        k[:, :2] *= self.input_ratio
        k[:, 0, 2] -= x0
        k[:, 1, 2] -= y0
        self.ixts = k.to(torch.float32).contiguous()
        self.lib = lib
        self._scratch = {}

    @staticmethod
    def resized(Hraw: int, Wraw: int, input_ratio: float, lib=None):
        """(Hs, Ws): the raw size times ``input_ratio``, rounded half-to-even (``enerf_ingest_raw_geometry`` when ``lib`` is given;
        Python's ``round`` is the same rule)."""
        if lib is not None:
            return lib.ingest_raw_geometry(Hraw, Wraw, input_ratio)
        return int(round(Hraw * float(input_ratio))), int(round(Wraw * float(input_ratio)))

    @staticmethod
    def outdoor_crop(Hs: int, Ws: int, h: int, w: int):
        """(y0, x0) of the outdoor dataset's crop of a resized Hs x Ws image to ``input_h_w`` = (h, w) (enerf_outdoor/enerf.py:118-123:
        65 % of the rows cut go off the top)."""
        return int((Hs - h) * 0.65), int((Ws - w) * 0.5)

    def scratch(self, V: int, device):
        """The (V,Hraw,Wraw) uint8 buffer of the dilated raw mask, one per (V, device), kept."""
        key = (int(V), str(device))
        if key not in self._scratch:
            self._scratch[key] = torch.empty((V, self.Hraw, self.Wraw), dtype=torch.uint8, device=device)
        return self._scratch[key]

    def check_frame(self, img_u8, masks=None, what="RawIngest"):
        V, Hr, Wr = self.V, self.Hraw, self.Wraw
        if img_u8.dtype != torch.uint8 or tuple(img_u8.shape) != (V, Hr, Wr, 3):
            raise ValueError(f"{what}: a raw frame must be uint8 ({V},{Hr},{Wr},3), got {img_u8.dtype} {tuple(img_u8.shape)}")
        if masks is not None and (masks.dtype not in (torch.uint8, torch.bool) or tuple(masks.shape) != (V, Hr, Wr)):
            raise ValueError(f"{what}: raw masks must be uint8 / bool ({V},{Hr},{Wr}), got {masks.dtype} {tuple(masks.shape)}")

    def __call__(self, img_u8, masks=None, dilate: int = 0, out=None, mask_out=None, lib=None, scratch=None):
        """The (V,3,H,W) float32 image of a raw frame (``out`` when given); ``mask_out`` (V,H,W) uint8 receives the final mask.
        ``scratch``: the caller's own (V,Hraw,Wraw) uint8 buffer for the dilated mask — a caller on a stream of its own passes one
        (the rig's :meth:`scratch` is one buffer per device, for calls that the stream orders)."""
        self.check_frame(img_u8, masks)
        lib = lib or self.lib
        if lib is None:
            from .lib import get_lib
            lib = get_lib()
        if img_u8.device != self.device:
            raise ValueError("RawIngest: the frame must live on the device of the rig's intrinsics")
        if scratch is None and masks is not None and dilate:
            scratch = self.scratch(self.V, img_u8.device)
        if masks is not None:
            masks = masks.contiguous()
        return lib.ingest_raw_u8(img_u8.contiguous(), self.raw_ixts, self.dist, masks, dilate, self.input_ratio, self.crop, scratch,
                                 out, mask_out)
