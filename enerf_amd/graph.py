"""Whole-frame HIP graph: capture one ``Network.forward`` — ~38 kernel launches and their
ctypes/torch bookkeeping (0.26 ms of host time per 1.09 ms frame) — once, replay it per frame.

    frame = GraphedFrame(net, example_batch)      # captures on a side stream; static input/output buffers
    out = frame(batch)                            # copies the batch into the static inputs, one hipGraphLaunch

``fn`` (optional) is what gets captured instead of ``net`` itself: a callable ``fn(static_batch) -> dict`` around the network, e.g.
the interactive loop ``select_views -> net.forward_cached -> pack_rgb8`` (nothing in it may synchronise).  Tensors of the batch may
then also be changed in place between replays (a device-resident view index, the target camera).  The graph holds the addresses
of whatever ``fn`` closed over: a SourceCache rebuilt at new addresses (a new time frame) is NOT noticed — the replay keeps reading
the old one, which stays alive here — so either refill the same cache's buffers in place or capture again.

The graph holds the shapes and the weights' packed images of the capture; re-capture after load_state_dict /
a shape change.  Works because the HIP path never synchronises, allocates only through torch's (graph-aware)
caching allocator and takes every pointer from tensors that stay alive inside the graph's private pool."""
from __future__ import annotations

from typing import Dict

import torch


class GraphedFrame:
    def __init__(self, net, batch: Dict[str, torch.Tensor], warmup: int = 2, fn=None):
        if net.training:
            raise RuntimeError("GraphedFrame: call net.eval() first")
        if getattr(net, "human", False) and not net.static_shapes:
            raise RuntimeError("GraphedFrame: the human variant needs static_shapes=True (no count readback inside a graph)")
        # the composite network (network_composite.py) reads its boxes on the host: a device tensor would be a readback inside the
        # capture, and the boxes' windows are baked into the captured launches
        # With batch['bbox_size'] (+ batch['bbox_xy'], a device tensor, or positions ``fn`` computes itself, e.g. EnerfLib.layer_boxes)
        # only the sizes are baked in: the positions are read by the kernels, and a replay with moved boxes is legal.
        self.composite = hasattr(net, "num_fg_layers")
        self.moving = self.composite and net._is_moving(batch)
        if self.moving:
            xy = batch.get("bbox_xy")
            if xy is not None and not (torch.is_tensor(xy) and xy.is_cuda):
                raise RuntimeError("GraphedFrame: batch['bbox_xy'] must be a device tensor (an upload inside the capture is not replayed)")
            self._sizes = net._sizes(batch)
        elif self.composite:
            if torch.is_tensor(batch.get("bbox")) and batch["bbox"].is_cuda:
                raise RuntimeError("GraphedFrame: the composite network needs batch['bbox'] on the host (a CPU tensor or a sequence); "
                                   "a device tensor is a readback inside the capture")
            self._boxes = net._boxes(batch)
        self.net = net
        # kept for the life of the graph: the closure owns what the captured kernels read besides the network's own buffers
        # (a SourceCache's maps live outside the graph's private pool)
        self.fn = fn
        run = net if fn is None else fn
        self.static_in = {k: v.clone() if torch.is_tensor(v) else v for k, v in batch.items()}
        with torch.no_grad():
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(max(1, warmup)):          # packs weights, sizes workspaces, warms the allocator
                    run(self.static_in)
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            # capture on the warm-up stream: the library's per-stream side lane (frame.hip) then exists before the capture
            # starts, and the lane's fork/join (event waits) is captured as a two-branch graph
            with torch.cuda.graph(self.graph, stream=s):
                self.static_out = run(self.static_in)
        # the graph holds raw addresses of the packed weight images and the FeatureNet scratch, which live OUTSIDE the
        # graph's private pool: keep them alive here and refuse to replay once the network has replaced them
        if self.composite:               # its packed images are plain tensors, its per-shape buffers hold the frame's workspace
            self._held = dict(net._packed)
            self._held_ws = {k: dict(v) for k, v in net._shapes.items()}
        else:
            self._held = {k: v[0] for k, v in net._packed.items()}
            self._held_ws = {k: v["ws"] for k, v in net._frames.items()}     # the frame workspaces

    def __call__(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        for k, t in self._held.items():
            ent = self.net._packed.get(k)
            if ent is None or (ent if self.composite else ent[0]) is not t:
                raise RuntimeError("GraphedFrame: the network's weights changed (load_state_dict / .to()) after capture; "
                                   "re-capture the frame")
        if self.moving:
            if not self.net._is_moving(batch) or self.net._sizes(batch) != self._sizes:
                raise RuntimeError("GraphedFrame: batch['bbox_size'] changed; the boxes' sizes are part of the captured launches: re-capture "
                                   "(the positions, batch['bbox_xy'], may move freely)")
        elif self.composite and (self.net._is_moving(batch) or self.net._boxes(batch) != self._boxes):
            raise RuntimeError("GraphedFrame: batch['bbox'] changed; the boxes' windows are part of the captured launches: re-capture")
        for k, v in batch.items():
            if torch.is_tensor(v):
                dst = self.static_in[k]
                if dst.shape != v.shape:
                    raise RuntimeError(f"GraphedFrame: '{k}' changed shape {tuple(dst.shape)} -> {tuple(v.shape)}; re-capture")
                if dst.data_ptr() != v.data_ptr():
                    dst.copy_(v, non_blocking=True)
        self.graph.replay()
        return self.static_out                      # static buffers: valid until the next call
