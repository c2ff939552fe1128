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
  * the first ``render`` after a ``flip`` makes the caller's stream wait for that slot's build event.
The one place the host can wait is the player's own pinned staging buffer: a host frame is copied into the slot's staging buffer
by the CPU, so if the upload that used that buffer ``slots`` submissions ago is still in flight (the host has run that far ahead
of the device) ``submit`` waits for that upload — never for a kernel.  Device tensors are never staged through the host.

With ``raw=`` (a :class:`enerf_amd.raw_ingest.RawIngest`) the frames submitted are RAW camera frames, (V,Hraw,Wraw,3) uint8 with masks
(V,Hraw,Wraw): the staging and the device uint8 buffers take the raw size, ``enerf_ingest_raw_u8`` undistorts, resizes and crops them into
the float image, and ``ixts`` are the rig's adjusted intrinsics (``raw.ixts``); H and W stay the cache's.

Every buffer — pinned staging, device uint8 image and mask, the float image, the build workspace and the caches — is allocated in
the constructor, so nothing is allocated on one stream and freed under another while a sequence plays.
"""
from __future__ import annotations

import torch

from .source_cache import SourceCache


class _Slot:
    def __init__(self, cache, pin_img, pin_mask):
        self.cache = cache
        self.pin_img, self.pin_mask = pin_img, pin_mask     # host staging (None on a CPU device)
        self.uploaded = None                                # event: the last H2D copy out of the staging buffers
        self.built = None                                   # event: the last rebuild (build stream)
        self.read = {}                                      # caller stream handle -> (stream, event after its last render of this slot)
        self.seq = -1                                       # submission number of what the slot holds (-1: nothing)
        self.pending = False                                # submitted, not flipped to yet


class SequencePlayer:
    """``slots`` source-view caches for V = ``exts.shape[0]`` cameras of H x W, one of them the *front* that ``render`` draws from.

    ``submit(frame_u8, masks=None)``  (V,H,W,3) uint8 and optionally (V,H,W) uint8 / bool, host (pinned or not) or device tensors:
        enqueues upload, ingest and the in-place rebuild of the oldest slot that is neither the front nor holds a submitted frame
        that was not flipped to yet, on the build stream.  Raises when there is no such slot.
    ``flip()``  the most recently submitted slot becomes the front (older unflipped submissions are dropped).
    ``render(view_idx, tar)``  ``Network.forward_cached`` on the front slot, on the caller's current stream.
    """

    def __init__(self, net, exts: torch.Tensor, ixts: torch.Tensor, H: int, W: int, slots: int = 2, dilate: int = 0, raw=None):
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
        self.slots = [_Slot(SourceCache.empty(net, V, H, W, exts, ixts), pin(V, Hin, Win, 3), pin(V, Hin, Win)) for _ in range(slots)]
        # the build stream serialises every build, so one device copy of the uint8 frame, one float image and one workspace serve all slots
        self._img_u8 = torch.empty((V, Hin, Win, 3), dtype=torch.uint8, device=dev)
        self._mask_u8 = torch.empty((V, Hin, Win), dtype=torch.uint8, device=dev)
        self._mask_scratch = None if raw is None or not self.dilate else torch.empty((V, Hin, Win), dtype=torch.uint8, device=dev)
        self._image = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        self._workspace = net.lib.source_cache_build_workspace(H, W, dev)
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
        own = sum(t.numel() * t.element_size() for t in (self._img_u8, self._mask_u8, self._image, self._workspace, self._mask_scratch)
                  if t is not None)
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
                         scratch=self._mask_scratch)
            else:
                self.net.lib.ingest_views_u8(self._img_u8, self._mask_u8 if masked else None, self.dilate if masked else 0, out=self._image)
            slot.cache.rebuild(self._image, workspace=self._workspace)

    def flip(self):
        if self._latest is None or not self._latest.pending:
            raise RuntimeError("SequencePlayer.flip: nothing was submitted since the last flip")
        self._front = self._latest
        for s in self.slots:
            s.pending = False
        self._front_waited = set()

    def render(self, view_idx, tar):
        slot = self._front
        if slot is None:
            raise RuntimeError("SequencePlayer.render: no front slot yet (submit a frame and flip)")
        if self.build_stream is None:
            return self.net.forward_cached(slot.cache, view_idx, tar)
        cur = torch.cuda.current_stream(self.device)
        sid = cur.cuda_stream
        if sid not in self._front_waited:
            cur.wait_event(slot.built)
            self._front_waited.add(sid)
        out = self.net.forward_cached(slot.cache, view_idx, tar)
        ent = slot.read.get(sid)
        if ent is None:
            ent = slot.read[sid] = (cur, torch.cuda.Event())
        ent[1].record(cur)
        return out
