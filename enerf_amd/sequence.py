"""Playing a dynamic scene: the time frames of a sequence streamed as uint8 into double-buffered source-view caches.

The reference's interactive dataset (zjumocap/enerf_interactive.py) holds, for every time frame, the V camera images of that
instant and renders any number of target cameras from them.  A :class:`SourceCache` makes the per-camera half of that loop cheap;
a :class:`SequencePlayer` does the other half — what happens when the time frame changes — beside the rendering instead of in
front of it: the next frame's images go up as uint8 (4 bytes per pixel with the mask, not 12), ``enerf_ingest_views_u8`` converts
and masks them on the device, and the cache of a slot nobody renders from is rebuilt in place, all on the player's own stream.

    player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=5)
    player.submit(frames[0], masks[0]); player.flip()
    for t in range(1, T):
        player.submit(frames[t], masks[t])                   # upload + ingest + rebuild of the back slot: build stream
        for cam in cameras_of(t - 1):                        # meanwhile, on the caller's stream
            idx = lib.select_views(cam_points, cam["c2w"], S)
            out = player.render(idx, {"tar_ext": ..., "tar_ixt": ..., "near_far": lib.bounds_near_far(vertices, tar_ext)})
        player.flip()                                        # the next render waits (on the device) for the build

Ordering is by events between the two streams, never by the host:
  * a build into a slot waits for the event recorded after the last ``render`` that read that slot;
  * the first ``render`` after a ``flip`` makes the caller's stream wait for that slot's build event (with ``hull=``, below, so does
    reading ``bounds`` / ``corners``, and a build into a slot waits for what the streams that read them had enqueued by then).
The one place the host can wait is the player's own pinned staging buffer: a host frame is copied into the slot's staging buffer
by the CPU, so if the upload that used that buffer ``slots`` submissions ago is still in flight (the host has run that far ahead
of the device) ``submit`` waits for that upload — never for a kernel.  Device tensors are never staged through the host.

With ``raw=`` (a :class:`enerf_amd.raw_ingest.RawIngest`) the frames submitted are RAW camera frames, (V,Hraw,Wraw,3) uint8 with masks
(V,Hraw,Wraw): the staging and the device uint8 buffers take the raw size, ``enerf_ingest_raw_u8`` undistorts, resizes and crops them into
the float image, and ``ixts`` are the rig's adjusted intrinsics (``raw.ixts``); H and W stay the cache's.

With ``hull=`` (a :class:`HullSpec`) every build also carves the foreground's world-space box of its time frame from the masks
(``enerf_vhull_bounds``), on the build stream after the ingest and before the rebuild, into the slot's own output tensors:
``player.bounds`` (L,2,3), ``player.corners`` (L,8,3) and ``player.hull_flags`` (L) are the front slot's, ordered for the caller's
stream by the build event like the cache — what ``lib.layer_boxes`` (the composite network's ``bbox_xy`` and ``near_far``) and
``lib.bounds_near_far`` (``corners`` as its vertices) take, never read on the host.  The masks are the submitted ones; with ``raw=``
the ingest's final mask (undistorted, resized, cropped), carved against ``raw.ixts``.  With ``dilate > 0`` on the raw path that mask
is the DILATED one, so the hull is the dilated silhouettes': larger, never smaller — conservative for a box.  (Without ``raw=`` the
submitted masks are carved as they are; the dilation there happens inside the ingest kernel.)

Every buffer — pinned staging, device uint8 image and mask, the float image, the build workspace, the hull's outputs and the caches
— is allocated in the constructor, so nothing is allocated on one stream and freed under another while a sequence plays.
"""
from __future__ import annotations

import torch

from .source_cache import SourceCache


class HullSpec:
    """What ``SequencePlayer(hull=...)`` carves with: the arguments of ``EnerfLib.vhull_bounds`` that are not tensors.
    ``scene_bounds`` ((x0,y0,z0),(x1,y1,z1)) and ``grid`` (Gx,Gy,Gz) are host values."""

    def __init__(self, scene_bounds, grid=(128, 128, 128), n_layers=1, labels=False, min_views=2, max_miss=0, pad=0.0):
        self.scene_bounds = torch.as_tensor(scene_bounds, dtype=torch.float32).reshape(2, 3).tolist()
        self.grid = tuple(int(g) for g in grid)
        self.n_layers, self.labels, self.min_views, self.max_miss, self.pad = int(n_layers), bool(labels), int(min_views), int(max_miss), float(pad)

    def kwargs(self):
        return dict(grid=self.grid, n_layers=self.n_layers, labels=self.labels, min_views=self.min_views, max_miss=self.max_miss,
                    pad=self.pad)


class _Slot:
    def __init__(self, cache, pin_img, pin_mask, hull=None):
        self.cache = cache
        self.hull = hull                                    # (bounds, counts, flags, corners) of the time frame the slot holds, or None
        self.pin_img, self.pin_mask = pin_img, pin_mask     # host staging (None on a CPU device)
        self.uploaded = None                                # event: the last H2D copy out of the staging buffers
        self.built = None                                   # event: the last rebuild (build stream)
        self.read = {}                                      # caller stream handle -> (stream, event after its last render of this slot)
        self.hull_readers = {}                              # caller stream handle -> stream that was handed this slot's hull tensors
        self.seq = -1                                       # submission number of what the slot holds (-1: nothing)
        self.pending = False                                # submitted, not flipped to yet


class SequencePlayer:
    """``slots`` source-view caches for V = ``exts.shape[0]`` cameras of H x W, one of them the *front* that ``render`` draws from.

    ``submit(frame_u8, masks=None)``  (V,H,W,3) uint8 and optionally (V,H,W) uint8 / bool, host (pinned or not) or device tensors:
        enqueues upload, ingest and the in-place rebuild of the oldest slot that is neither the front nor holds a submitted frame
        that was not flipped to yet, on the build stream.  Raises when there is no such slot.
    ``flip()``  the most recently submitted slot becomes the front (older unflipped submissions are dropped).
    ``render(view_idx, tar)``  ``Network.forward_cached`` on the front slot, on the caller's current stream.
    ``hull=HullSpec(...)``  every build also carves the time frame's world-space box from the masks (``submit`` then needs masks);
        ``bounds``, ``corners``, ``hull_flags`` and ``hull_counts`` are the front slot's device tensors.
    """

    def __init__(self, net, exts: torch.Tensor, ixts: torch.Tensor, H: int, W: int, slots: int = 2, dilate: int = 0, raw=None,
                 hull=None):
        if slots < 2:
            raise ValueError("SequencePlayer: slots must be at least 2 (one to render from, one to build into)")
        if exts.dim() != 3 or exts.device != ixts.device:
            raise ValueError("SequencePlayer: exts (V,4,4) and ixts (V,3,3) on one device")
        self.net, self.H, self.W, self.V, self.dilate = net, int(H), int(W), exts.shape[0], int(dilate)
        self.device = dev = exts.device
        self.raw = raw
        if raw is not None and (raw.H, raw.W, raw.V) != (self.H, self.W, self.V):
            raise ValueError(f"SequencePlayer: raw= gives {raw.V} views of {raw.H}x{raw.W}, the player was opened for {self.V} of {H}x{W}")
        Hin, Win = (self.H, self.W) if raw is None else (raw.Hraw, raw.Wraw)    # what submit takes and the staging holds
        V, cuda = self.V, exts.is_cuda
        net.prepare()                                       # weight images packed before the two streams start sharing them
        self.build_stream = torch.cuda.Stream(dev) if cuda else None
        exts, ixts = exts.contiguous(), ixts.contiguous()
        pin = (lambda *shape: torch.empty(shape, dtype=torch.uint8, pin_memory=True)) if cuda else (lambda *shape: None)
        self.hull = hull
        L = 0 if hull is None else hull.n_layers
        hull_out = (lambda: None) if hull is None else (lambda: (
            torch.zeros((L, 2, 3), dtype=torch.float32, device=dev), torch.zeros((L,), dtype=torch.int32, device=dev),
            torch.zeros((L,), dtype=torch.int32, device=dev), torch.zeros((L, 8, 3), dtype=torch.float32, device=dev)))
        self.slots = [_Slot(SourceCache.empty(net, V, H, W, exts, ixts), pin(V, Hin, Win, 3), pin(V, Hin, Win), hull_out())
                      for _ in range(slots)]
        # the build stream serialises every build, so one device copy of the uint8 frame, one float image and one workspace serve all slots
        self._img_u8 = torch.empty((V, Hin, Win, 3), dtype=torch.uint8, device=dev)
        self._mask_u8 = torch.empty((V, Hin, Win), dtype=torch.uint8, device=dev)
        self._mask_scratch = None if raw is None or not self.dilate else torch.empty((V, Hin, Win), dtype=torch.uint8, device=dev)
        self._image = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        self._workspace = net.lib.source_cache_build_workspace(H, W, dev)
        # the hull: the cameras at the masks' resolution, the raw ingest's final mask, the accumulators
        self._hull_exts, self._hull_ixts = (exts, ixts) if hull is not None else (None, None)
        self._hull_mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev) if hull is not None and raw is not None else None
        self._hull_workspace = net.lib.vhull_workspace(L, dev) if hull is not None else None
        self._front = None
        self._latest = None
        self._seq = 0
        self._front_waited = set()                          # caller streams that already wait for the front's build event

    # -- bookkeeping -------------------------------------------------------------------------------
    @property
    def front(self):
        """The cache ``render`` draws from (None before the first ``flip``)."""
        return None if self._front is None else self._front.cache

    def nbytes(self) -> int:
        """Device bytes the player holds (caches, uint8 frame + mask, float image, build workspace); ``pinned_nbytes`` is the host's."""
        own = sum(t.numel() * t.element_size() for t in (self._img_u8, self._mask_u8, self._image, self._workspace, self._mask_scratch,
                                                         self._hull_mask, self._hull_workspace) if t is not None)
        own += sum(t.numel() * t.element_size() for s in self.slots if s.hull is not None for t in s.hull)
        return own + sum(s.cache.nbytes() for s in self.slots)

    def pinned_nbytes(self) -> int:
        return sum(t.numel() for s in self.slots for t in (s.pin_img, s.pin_mask) if t is not None)

    def _check_frame(self, frame, masks):
        V, H, W = (self.V, self.H, self.W) if self.raw is None else (self.V, self.raw.Hraw, self.raw.Wraw)
        if frame.dtype != torch.uint8 or tuple(frame.shape) != (V, H, W, 3):
            raise ValueError(f"SequencePlayer.submit: frame must be uint8 ({V},{H},{W},3), got {frame.dtype} {tuple(frame.shape)}")
        if masks is not None and (masks.dtype not in (torch.uint8, torch.bool) or tuple(masks.shape) != (V, H, W)):
            raise ValueError(f"SequencePlayer.submit: masks must be uint8 / bool ({V},{H},{W}), got {masks.dtype} {tuple(masks.shape)}")
        for t in (frame, masks):
            if t is not None and t.device != self.device and t.device.type != "cpu":
                raise ValueError("SequencePlayer.submit: tensors must live on the host or on the player's device")

    def _stage(self, slot, src, pin, dst, caller):
        """One tensor of a frame into its device buffer, on the build stream (the current one)."""
        if src.dtype == torch.bool:
            src = src.view(torch.uint8)
        if src.device.type == "cpu" and pin is not None:
            pin.copy_(src)                                  # host memcpy into the player's pinned buffer
            dst.copy_(pin, non_blocking=True)
        else:                                               # device tensor (or a CPU-device player): ordered after its producer
            if caller is not None:
                self.build_stream.wait_stream(caller)
                src.record_stream(self.build_stream)        # the caller may drop its tensor before the copy has run
            dst.copy_(src, non_blocking=True)

    # -- the three verbs ---------------------------------------------------------------------------
    def submit(self, frame_u8: torch.Tensor, masks=None):
        self._check_frame(frame_u8, masks)
        if self.hull is not None and masks is None:
            raise ValueError("SequencePlayer.submit: the player was opened with hull=, which carves the bounds from the masks: pass masks")
        free = [s for s in self.slots if s is not self._front and not s.pending]
        if not free:
            raise RuntimeError("SequencePlayer.submit: no free slot — every slot but the front holds a submitted frame that was "
                               "not flipped to yet (call flip(), or open the player with more slots)")
        slot = min(free, key=lambda s: s.seq)
        lib = self.net.lib
        if self.build_stream is None:                       # CPU device (the emulator): everything is synchronous
            self._stage(slot, frame_u8, None, self._img_u8, None)
            if masks is not None:
                self._stage(slot, masks, None, self._mask_u8, None)
            self._build(slot, masks is not None)
        else:
            on_host = any(t is not None and t.device.type == "cpu" for t in (frame_u8, masks))
            if on_host and slot.uploaded is not None and not slot.uploaded.query():
                slot.uploaded.synchronize()                 # the staging buffer is still being read: the host is `slots` frames ahead
            caller = torch.cuda.current_stream(self.device)
            bs = self.build_stream
            with torch.cuda.stream(bs):
                self._stage(slot, frame_u8, slot.pin_img, self._img_u8, caller)
                if masks is not None:
                    self._stage(slot, masks, slot.pin_mask, self._mask_u8, caller)
                if slot.uploaded is None:
                    slot.uploaded = torch.cuda.Event()
                slot.uploaded.record(bs)
                for st, ev in slot.read.values():           # the renders that still read this slot's buffers
                    bs.wait_event(ev)
                for st in slot.hull_readers.values():       # ... and whatever read its bounds (handed out while it was the front,
                    ev = torch.cuda.Event()                 # so those reads are enqueued by now; a caller need not render after them)
                    ev.record(st)
                    bs.wait_event(ev)
                slot.hull_readers = {}
                self._build(slot, masks is not None)
                if slot.built is None:
                    slot.built = torch.cuda.Event()
                slot.built.record(bs)
        slot.seq, slot.pending = self._seq, True
        self._seq += 1
        self._latest = slot

    def _build(self, slot, masked):
        with torch.no_grad():
            if self.raw is not None:
                self.raw(self._img_u8, self._mask_u8 if masked else None, self.dilate if masked else 0, out=self._image, lib=self.net.lib,
                         scratch=self._mask_scratch, mask_out=self._hull_mask)
            else:
                self.net.lib.ingest_views_u8(self._img_u8, self._mask_u8 if masked else None, self.dilate if masked else 0, out=self._image)
            if self.hull is not None:
                self.net.lib.vhull_bounds(self._mask_u8 if self.raw is None else self._hull_mask, self._hull_exts, self._hull_ixts,
                                          self.hull.scene_bounds, out=slot.hull, workspace=self._hull_workspace, **self.hull.kwargs())
            slot.cache.rebuild(self._image, workspace=self._workspace)

    def flip(self):
        if self._latest is None or not self._latest.pending:
            raise RuntimeError("SequencePlayer.flip: nothing was submitted since the last flip")
        self._front = self._latest
        for s in self.slots:
            s.pending = False
        self._front_waited = set()

    def _wait_front(self, slot):
        """The caller's current stream waits (on the device, once per flip) for the front slot's build; returns that stream."""
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream not in self._front_waited:
            cur.wait_event(slot.built)
            self._front_waited.add(cur.cuda_stream)
        return cur

    def _front_hull(self, what):
        slot = self._front
        if self.hull is None:
            raise RuntimeError(f"SequencePlayer.{what}: the player was opened without hull=")
        if slot is None:
            raise RuntimeError(f"SequencePlayer.{what}: no front slot yet (submit a frame and flip)")
        if self.build_stream is not None:
            cur = self._wait_front(slot)
            slot.hull_readers[cur.cuda_stream] = cur        # the next build into this slot waits for what this stream enqueues
        return slot.hull

    @property
    def bounds(self):
        """(L,2,3) float32: the front time frame's world-space box per layer, on the device (``hull=``)."""
        return self._front_hull("bounds")[0]

    @property
    def hull_counts(self):
        return self._front_hull("hull_counts")[1]

    @property
    def hull_flags(self):
        """(L) int32: bit 0 = nothing occupied (bounds = scene_bounds), bit 1 = the hull touches a face of the grid."""
        return self._front_hull("hull_flags")[2]

    @property
    def corners(self):
        """(L,8,3) float32: the box's corners, the ``vertices`` of ``lib.bounds_near_far``."""
        return self._front_hull("corners")[3]

    def render(self, view_idx, tar):
        slot = self._front
        if slot is None:
            raise RuntimeError("SequencePlayer.render: no front slot yet (submit a frame and flip)")
        if self.build_stream is None:
            return self.net.forward_cached(slot.cache, view_idx, tar)
        cur = self._wait_front(slot)
        sid = cur.cuda_stream
        out = self.net.forward_cached(slot.cache, view_idx, tar)
        ent = slot.read.get(sid)
        if ent is None:
            ent = slot.read[sid] = (cur, torch.cuda.Event())
        ent[1].record(cur)
        return out
