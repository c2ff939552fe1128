"""``Network`` for the reference's ``lib/networks/enerf/network_composite.py`` (ENeRF-Outdoor, ``enerf_outdoor/actor1.yaml``):
``num_fg_layers`` foreground cascades, each restricted to its layer's 2-D box and depth range, one background cascade over the
whole image, and one alpha-compositing pass over the depth-sorted union of their samples.

Same sub-module names and shapes as the reference (``feature_net``, ``feature_net_bg``, ``cost_reg_{i}_layer{l}``,
``nerf_{i}_layer{l}``, ``cost_reg_{i}_bg``, ``nerf_{i}_bg``), so ``load_state_dict(strict=True)`` takes its checkpoints.  The
modules only own parameters; everything runs in the library's HIP kernels (include/enerf_hip.h, "the composite network"):

  * a foreground layer's cost volume, MinCostRegNet and its depth regression see only the layer's window; the reference's two
    zero-padded full-size volumes are never built (``enerf_build_feature_volume_window``, ``enerf_depth_regression_window``);
  * a layer renders only its window's rays, picked on the device (``enerf_window_ray_index`` + the render kernel's selection),
    and the kernel stops at the MLP (``enerf_render_rays_raw``);
  * ``enerf_composite_layers`` is parse_layer + raw2outputs_composite, one thread per pixel.

A frame is ONE C call, ``enerf_forward_composite`` (csrc/frame.hip): the driver runs the stages above itself, the foreground layers
forked onto the library's side lane (``options.single_stream`` keeps the frame on the caller's stream).  ``Network(...,
driver="staged")`` keeps the earlier path — one ctypes call per stage, the same kernels, the same bits — and a ``stage_hook`` selects
it for that frame too (per-stage timing, tools/time_composite.py).

A viewer that draws many target cameras from one rig of V source views per time frame runs the two FeatureNets once per time frame:
``cache = net.cache_sources(inps, bg_inps, exts, ixts)`` (enerf_amd/composite_cache.py), then ``net.forward_cached(cache, view_idx,
batch)`` per camera — ``enerf_forward_composite_cached``, the same frame with both nets' maps, the texels and the source cameras
gathered by a device-resident view index, bit for bit ``forward`` on those views.

Training is opt-in: ``Network(..., trainable=True)`` in ``.train()`` mode runs the differentiable path of
``train_path_composite.py`` (every stage on the library in both directions; ``enerf_amd.loss.EnerfLoss`` takes its output dict), and
the packed weight images — and any source cache — are rebuilt after it.  Without the argument ``forward`` raises in training mode, as
``forward_cached`` and ``cache_sources`` do on every network.

Restrictions, all stated in DESIGN.md §8: ``B == 1`` (the reference reads
``batch['bbox'][0]`` for every batch element); ``feature_backend="hip"``; no ``SequencePlayer`` or multi-GPU driver; the cached
frame has no staged form (``forward_cached`` with a ``stage_hook`` raises); at most four foreground layers with
``num_fg_layers * num_samples <= 16`` per level.

The output dict has the reference's keys per rendered level — ``rgb``, ``depth``, ``weights``, ``net_output``, ``z_vals``, each
suffixed ``_level{i}`` — except ``idx``: that is ``torch.sort``'s permutation, which is unspecified among samples of equal depth
(two layers' zero samples outside their boxes, for one).  Here such samples keep layer-then-sample order, always.

Buffers: every tensor a frame touches — stage outputs, workspaces, the returned outputs and ``intermediates`` — is allocated on the
first frame of a shape (image size, views, boxes) and reused by every later frame of that shape, so the NEXT frame of the shape
overwrites what this one returned; clone what must outlive it.  The last ``MAX_SHAPES`` shapes are kept.

Host synchronisation: the boxes are read on the host.  ``batch['bbox']`` as a CPU tensor or a sequence costs nothing; as a device
tensor that read is the frame's ONE synchronisation.  Nothing after it waits for the device.

Boxes that move (a moving actor, a moving camera): ``batch['bbox_size']`` — a host sequence of ``(w, h)`` per layer — together with
``batch['bbox_xy']`` — a float32 DEVICE tensor (L,2) or (1,L,2) of ``(x, y)`` — instead of ``batch['bbox']``.  The sizes are part
of the frame's shape, the positions are read by the kernels (``enerf_forward_composite_moving``): a moved box is the same shape —
no new buffers, no new plan — the position is never read on the host, and a ``GraphedFrame`` replays with moved boxes.  A position
is resolved on the device: non-finite -> 0, truncated, clamped into the image; ``intermediates['bbox_flags']`` (L) int32 on the
device has bit 0 set for every layer whose position that changed.  For positions ``bbox`` accepts the outputs are its bits.
``EnerfLib.layer_boxes`` computes the positions of a target camera on the device.  One C call per frame only: ``driver="staged"``,
a ``stage_hook`` and the training path refuse such a batch.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Optional

import ctypes as C

import torch
import torch.nn as nn

from .config import EnerfConfig
from .lib import MAX_FG_LAYERS, CompositeFrameArgs, EnerfLib, NerfRaw, Options, cascade_struct, get_lib
from .network import AggParams, CostRegParams, FeatureNet, _fc, _kaiming, _require_f32c

BG_PLANES = (16, 4)          # network_composite.py:122: the background's depth planes per level
MAX_SHAPES = 4               # frame shapes (image size, views, boxes) whose buffers a network keeps


class NerfCompositeParams(nn.Module):
    """nerf_.py:6-44: the NeRF head that ignores the voxel feature — ``lr0`` is 16 -> 64, ``color.0`` takes 64 + 16 + F + 4."""

    def __init__(self, feat_ch: int, viewdir_agg: bool, hid_n: int = 64):
        super().__init__()
        self.feat_ch, self.viewdir_agg = feat_ch, viewdir_agg
        self.agg = AggParams(feat_ch, viewdir_agg)
        self.lr0 = _fc(16, hid_n, nn.ReLU())
        self.lrs = nn.ModuleList()
        self.sigma = _fc(hid_n, 1, nn.Softplus())
        self.color = nn.Sequential(nn.Linear(64 + 16 + feat_ch + 4, hid_n), nn.ReLU(), nn.Linear(hid_n, 1), nn.ReLU())
        for m in (self.lr0, self.sigma, self.color):
            m.apply(_kaiming)

    def raw(self):
        """(enerf_nerf_raw_t, tensors it points into): the layouts enerf_nerf_pack reads (nerf.py's, with the eight voxel inputs),
        zero columns standing in for the voxel inputs of ``lr0`` and ``color.0``.  Exact: the raw render kernel feeds zeros there."""
        r = NerfRaw()
        lr0, col0 = self.lr0[0].weight, self.color[0].weight
        lr0_p = torch.cat([lr0.new_zeros(lr0.shape[0], 8), lr0.detach()], 1).contiguous()
        col0_p = torch.cat([col0.detach()[:, :64], col0.new_zeros(col0.shape[0], 8), col0.detach()[:, 64:]], 1).contiguous()
        pairs = [("glob", self.agg.global_fc[0]), ("aggw", self.agg.agg_w_fc[0]), ("fc", self.agg.fc[0]), ("sigma", self.sigma[0]),
                 ("col2", self.color[2])]
        if self.viewdir_agg:
            pairs.append(("view", self.agg.view_fc[0]))
        for name, lin in pairs:
            _require_f32c(lin.weight), _require_f32c(lin.bias)
            setattr(r, name + "_w", lin.weight.data_ptr())
            setattr(r, name + "_b", lin.bias.data_ptr())
        for name, w, lin in (("lr0", lr0_p, self.lr0[0]), ("col0", col0_p, self.color[0])):
            _require_f32c(w), _require_f32c(lin.bias)
            setattr(r, name + "_w", w.data_ptr())
            setattr(r, name + "_b", lin.bias.data_ptr())
        return r, (lr0_p, col0_p)


def _scaled_box(box, scale):
    """``(bbox * scale).int()`` of the reference (network_composite.py:88, utils.py:879): float32 product, truncation."""
    return tuple(int(v) for v in (torch.tensor([float(b) for b in box], dtype=torch.float32) * scale).int())


class Network(nn.Module):
    """ENeRF-Outdoor's layered renderer with the reference's call surface (network_composite.py:11-146)."""

    def __init__(self, cfg: Optional[EnerfConfig] = None, num_fg_layers: int = 1, lib: Optional[EnerfLib] = None,
                 feature_backend: str = "hip", driver: str = "call", trainable: bool = False):
        super().__init__()
        self.trainable = bool(trainable)               # opt-in: forward() in .train() mode runs train_path_composite.py
        if feature_backend != "hip":
            raise ValueError("network_composite: feature_backend must be 'hip'")
        if driver not in ("call", "staged"):
            raise ValueError("network_composite: driver must be 'call' (enerf_forward_composite) or 'staged' (one C call per stage)")
        self.driver = driver
        if not 1 <= int(num_fg_layers) <= MAX_FG_LAYERS:
            raise ValueError(f"network_composite: num_fg_layers must be in 1..{MAX_FG_LAYERS}")
        self.cfg = cfg or EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1))      # actor1.yaml
        self.cfg.cas.validate()
        cas = self.cfg.cas
        if cas.num > len(BG_PLANES):
            raise ValueError(f"network_composite: the background has depth planes for {len(BG_PLANES)} levels")
        self.feature_backend = feature_backend
        self.num_fg_layers = int(num_fg_layers)
        self._lib = lib
        self.options: Optional[Options] = None
        self.feature_net = FeatureNet()
        self.feature_net_bg = FeatureNet()
        for i in range(cas.num):
            for l in range(self.num_fg_layers):
                setattr(self, f"cost_reg_{i}_layer{l}", CostRegParams(int(32 * (2 ** (-i))), full=False))
                setattr(self, f"nerf_{i}_layer{l}", NerfCompositeParams(cas.nerf_model_feat_ch[i] + 3, self.cfg.viewdir_agg))
            setattr(self, f"cost_reg_{i}_bg", CostRegParams(int(32 * (2 ** (-i))), full=False))
            setattr(self, f"nerf_{i}_bg", NerfCompositeParams(cas.nerf_model_feat_ch[i] + 3, self.cfg.viewdir_agg))
        self._packed: Dict[str, torch.Tensor] = {}
        self._packed_gen = 0                           # moves on whenever the packed images are dropped: a source cache built before is stale
        self._shapes: "OrderedDict[tuple, dict]" = OrderedDict()     # frame shape -> its buffers (_shape_buffers)
        self.intermediates: Dict[str, torch.Tensor] = {}
        self.stage_hook = None                         # optional callable(stage name), called between the stages of forward()

    # -- weight images ---------------------------------------------------------------------------
    @property
    def lib(self) -> EnerfLib:
        if self._lib is None:
            self._lib = get_lib()
        return self._lib

    def invalidate_packed(self):
        self._packed = {}
        self._packed_gen = getattr(self, "_packed_gen", 0) + 1
        self._shapes = OrderedDict()

    def _apply(self, fn, *a, **k):
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self.invalidate_packed()
        return super().load_state_dict(*a, **k)

    def _packed_weights(self, name: str) -> torch.Tensor:
        t = self._packed.get(name)
        if t is None:
            m = getattr(self, name)
            dev = next(m.parameters()).device
            if isinstance(m, CostRegParams):
                t = self.lib.cost_reg_pack(m.raw(), dev)
            elif isinstance(m, FeatureNet):
                t = self.lib.feature_net_pack(m.raw(), dev)
            else:
                raw, keep = m.raw()                    # (the padded copies are read by a kernel enqueued on this stream: stream-ordered)
                t = self.lib.nerf_pack(raw, m.feat_ch, m.viewdir_agg, dev)
                del keep
            self._packed[name] = t
        return t

    def prepare(self):
        """Pack every weight image now, on the current stream."""
        for name, _ in self.named_children():
            self._packed_weights(name)
        return self

    # -- the frame -------------------------------------------------------------------------------
    def _boxes(self, batch):
        bbox = batch["bbox"]
        if torch.is_tensor(bbox):
            bbox = bbox.detach().cpu()                 # a device tensor: the frame's one synchronisation
            if bbox.dim() == 3:
                if bbox.shape[0] != 1:
                    raise ValueError("network_composite: B must be 1 (the reference reads batch['bbox'][0] for every batch element)")
                bbox = bbox[0]
            bbox = bbox.tolist()
        elif len(bbox) == 1 and len(bbox[0]) and hasattr(bbox[0][0], "__len__"):
            bbox = bbox[0]
        if len(bbox) < self.num_fg_layers or any(len(b) != 4 for b in bbox):
            raise ValueError(f"network_composite: batch['bbox'] must hold (x, y, w, h) for {self.num_fg_layers} layers")
        return [tuple(b) for b in bbox[:self.num_fg_layers]]

    @staticmethod
    def _is_moving(batch):
        return batch.get("bbox_size") is not None or batch.get("bbox_xy") is not None

    def _sizes(self, batch):
        """``batch['bbox_size']``: the layers' (w, h), read on the host — a sequence or a CPU tensor, never a device tensor."""
        if batch.get("bbox") is not None:
            raise ValueError("network_composite: pass either batch['bbox'] or batch['bbox_size'] with batch['bbox_xy'], not both")
        size = batch.get("bbox_size")
        if size is None:
            raise ValueError("network_composite: batch['bbox_xy'] needs batch['bbox_size'], the (w, h) of every layer on the host")
        if torch.is_tensor(size):
            if size.is_cuda:
                raise ValueError("network_composite: batch['bbox_size'] must be on the host (a sequence or a CPU tensor): the sizes are "
                                 "part of the frame's shape")
            size = size.reshape(-1, 2).tolist()
        elif len(size) == 1 and len(size[0]) and hasattr(size[0][0], "__len__"):
            size = size[0]
        if len(size) != self.num_fg_layers or any(len(b) != 2 for b in size):
            raise ValueError(f"network_composite: batch['bbox_size'] must hold (w, h) for {self.num_fg_layers} layers")
        return tuple((float(w), float(h)) for w, h in size)

    def _positions(self, batch, held):
        """``batch['bbox_xy']`` as the (L,2) float32 device tensor the kernels read: used in place if it is one, otherwise converted
        and uploaded into the shape's buffer first (as ``view_idx`` is).  Never read on the host."""
        xy = batch.get("bbox_xy")
        if xy is None:
            raise ValueError("network_composite: batch['bbox_size'] needs batch['bbox_xy'], the (x, y) of every layer")
        if not torch.is_tensor(xy):
            xy = torch.tensor(xy, dtype=torch.float32)
        L = self.num_fg_layers
        if xy.numel() != 2 * L or tuple(xy.shape) not in ((L, 2), (1, L, 2)):
            raise ValueError(f"network_composite: batch['bbox_xy'] must be ({L}, 2) or (1, {L}, 2)")
        return held("bbox_xy", xy, (L, 2))

    def _shape_buffers(self, key):
        """The buffers of one frame shape — (H, W, S, boxes, which levels bring their own rays, device) — allocated on the first frame of that shape and reused by every
        later one; the few most recent shapes are kept (moving boxes change the windowed buffers' sizes)."""
        st = self._shapes.get(key)
        if st is None:
            st = {}
            while len(self._shapes) >= MAX_SHAPES:
                self._shapes.popitem(last=False)
            self._shapes[key] = st
        else:
            self._shapes.move_to_end(key)
        dev = key[-1]

        def buf(name, shape, dtype=torch.float32):
            t = st.get(name)
            if t is None:
                t = st[name] = torch.empty(tuple(int(v) for v in shape), dtype=dtype, device=dev)
            return t
        return st, buf

    @staticmethod
    def _holder(buf, dev):
        def held(name, t, shape):
            """``t`` if the kernels can read it in place, else its copy in the shape's buffer (no allocation either way)."""
            t = t.reshape(shape)
            if t.dtype == torch.float32 and t.is_contiguous() and t.device == dev:
                return t
            b_ = buf(name, shape)
            b_.copy_(t)
            return b_
        return held

    def _texels(self, lib, buf, name, feats, src, level, H, W):
        cas = self.cfg.cas
        Hr, Wr = int(H * cas.render_scale[level]), int(W * cas.render_scale[level])
        f = feats[cas.render_im_feat_level[level]]
        n, hf, wf, Cf = f.shape
        if (hf, wf) != (Hr, Wr) or Cf != cas.nerf_model_feat_ch[level]:
            raise RuntimeError("network_composite: render_im_feat_level must name the feature map at the render resolution")
        tex = lib.pack_texels_cl(f, src, Hr, Wr, out=buf(name, (n, Hr, Wr, 4 * ((Cf + 3 + 3) // 4))))
        return tex.view(1, n, Hr, Wr, tex.shape[-1])

    def forward(self, batch):
        """network_composite.py:77-146.  ``batch``: the reference's — ``src_inps`` (1,S,3,H,W), ``bg_src_inps`` (same shape),
        cameras, ``bbox`` (1,L,4) = (x, y, w, h) per foreground layer in pixels of the input image, ``near_far`` (1,L+1,2) with
        the background's range last, and optionally ``rays_{i}`` (1,Hr*Wr,8), the full raster of each rendered level."""
        if self.training:
            if not getattr(self, "trainable", False):
                raise RuntimeError("network_composite: inference only — forward() has no training path unless the network was built "
                                   "with trainable=True; call net.eval()")
            if self._is_moving(batch):
                raise ValueError("network_composite: the training path takes batch['bbox'] only; batch['bbox_size'] / batch['bbox_xy'] "
                                 "(positions on the device) are for inference")
            from .train_path_composite import forward_train_composite
            self.invalidate_packed()                   # the optimizer is about to change what the packed images (and a source cache) hold
            return forward_train_composite(self, batch)
        cas, lib, L = self.cfg.cas, self.lib, self.num_fg_layers
        src = batch["src_inps"]
        B, S, _, H, W = src.shape
        if B != 1:
            raise ValueError("network_composite: B must be 1 (the reference reads batch['bbox'][0] for every batch element)")
        moving = self._is_moving(batch)
        if moving and (self.driver != "call" or self.stage_hook is not None):
            raise RuntimeError("network_composite: batch['bbox_size'] / batch['bbox_xy'] (positions on the device) have no staged form: "
                               "use driver='call' and clear stage_hook")
        boxes = [(0.0, 0.0, w, h) for w, h in self._sizes(batch)] if moving else self._boxes(batch)
        dev = src.device
        near_far = batch["near_far"]
        if tuple(near_far.shape) != (1, L + 1, 2):
            raise ValueError(f"network_composite: near_far must be (1, {L + 1}, 2): one range per foreground layer, the background's last")
        # (generated rays live in the frame's workspace: a batch with and one without rays_{i} are two shapes)
        own_rays = tuple(batch.get(f"rays_{i}") is not None for i in range(cas.num))
        st, buf = self._shape_buffers(("moving", H, W, S, tuple(b[2:] for b in boxes), own_rays, dev) if moving
                                      else (H, W, S, tuple(boxes), own_rays, dev))
        hook = self.stage_hook if self.stage_hook is not None else (lambda name: None)
        held = self._holder(buf, dev)
        exts, ixts = held("src_exts", batch["src_exts"], (1, S, 4, 4)), held("src_ixts", batch["src_ixts"], (1, S, 3, 3))
        tar_ext, tar_ixt = held("tar_ext", batch["tar_ext"], (1, 4, 4)), held("tar_ixt", batch["tar_ixt"], (1, 3, 3))
        src4 = held("src_inps", src, (S, 3, H, W))
        bg4 = held("bg_src_inps", batch["bg_src_inps"], (S, 3, H, W))
        nfs = buf("near_far", (L + 1, 1, 2))                        # one contiguous (1, 2) range per cascade
        nfs.copy_(near_far.reshape(L + 1, 1, 2))
        if self.driver == "call" and self.stage_hook is None:
            return self._forward_call(batch, st, buf, held, boxes, (src4, bg4, exts, ixts, tar_ext, tar_ixt, nfs), S, H, W,
                                      bbox_xy=self._positions(batch, held) if moving else None)
        hook("begin")
        feats, feats_bg = [], []
        for name, into in (("feature_net", feats), ("feature_net_bg", feats_bg)):           # both read src_inps (network_composite.py:78-79)
            bufs = (buf(name + ".f0", (S, H // 4, W // 4, 32)), buf(name + ".f1", (S, H // 2, W // 2, 16)), buf(name + ".f2", (S, H, W, 8)),
                    buf("feature_net.ws", ((lib.dll.enerf_feature_net_workspace_bytes(S, H, W) + 3) // 4,)))
            lib.feature_net_stage(self._packed_weights(name), src4, bufs, lib.FEAT_ALL, options=self.options)
            into.extend(bufs[:3])
        hook("feature_nets")
        ret, inter = {}, {}
        prev = [None] * L
        prev_bg = None
        for i in range(cas.num):
            h, w = int(H * cas.volume_scale[i]), int(W * cas.volume_scale[i])
            Hr, Wr = int(H * cas.render_scale[i]), int(W * cas.render_scale[i])
            C, inv, Ns, F = int(32 * (2 ** (-i))), cas.depth_inv[i], cas.num_samples[i], cas.nerf_model_feat_ch[i] + 3
            f_i, fbg_i = feats[i], feats_bg[i]
            f_i, fbg_i = f_i.view(1, *f_i.shape), fbg_i.view(1, *fbg_i.shape)
            proj = lib.get_proj_mats(ixts, exts, tar_ixt, tar_ext, cas.im_feat_scale[i], cas.volume_scale[i], out=buf(f"proj{i}", (1, S, 3, 4)))
            render = bool(cas.render_if[i])
            if render:
                rays = batch.get(f"rays_{i}")
                if rays is None:
                    rays = lib.gen_rays(tar_ext, tar_ixt, Hr, Wr, cas.render_scale[i], out=buf(f"rays{i}", (1, Hr * Wr, 8)))
                elif tuple(rays.shape) != (1, Hr * Wr, 8):
                    raise ValueError(f"network_composite: rays_{i} must be the full (1, {Hr * Wr}, 8) raster of the level")
                else:
                    rays = held(f"rays{i}", rays, (1, Hr * Wr, 8))
                tex = self._texels(lib, buf, f"tex{i}", feats, src4, i, H, W)
                tex_bg = self._texels(lib, buf, f"tex{i}.bg", feats_bg, bg4, i, H, W)

            def cascade(who, nf_in, prev_maps, D, feat, win):
                """One cascade level up to its depth / std maps: ``win`` = the layer's window of the (h, w) grid, or None."""
                n = f"{who}.{i}."
                wh, ww = (win[3], win[2]) if win is not None else (h, w)
                dv, nf = lib.get_depth_values(nf_in, prev_maps, 1, D, h, w, inv, out=(buf(n + "dv", (1, D, h, w)), buf(n + "nf", (1, 2, h, w))))
                vol = buf(n + "vol", (1, D, wh, ww, C))
                if win is not None:
                    lib.build_feature_volume_window(feat, proj, dv, C, win, out=vol)
                else:
                    lib.build_feature_volume(feat, proj, dv, C, out=vol)
                ws = buf(n + "ws", ((lib.dll.enerf_cost_reg_workspace_bytes(0, 1, D, wh, ww) + 3) // 4,))
                _, prob = lib.cost_reg(self._packed_weights(f"cost_reg_{i}_{who}"), C, False, vol, workspace=ws, options=self.options,
                                       out=(buf(n + "feat", (1, D, wh, ww, 8)), buf(n + "prob", (1, D, wh, ww))))     # (feat: dead work)
                maps = (buf(n + "depth", (1, h, w)), buf(n + "std", (1, h, w)))
                if win is not None:
                    lib.depth_regression_window(prob, dv, inv, win, out=maps)
                else:
                    lib.depth_regression(prob, dv, inv, out=maps)
                inter[f"depth_{i}_{who}"], inter[f"std_{i}_{who}"] = maps
                return maps[0], maps[1], nf

            def raw_samples(who, tex_, maps, win):
                n = f"{who}.{i}."
                rows = win[2] * win[3] if win is not None else Hr * Wr
                sel = {}
                if win is not None:
                    index, count = buf(n + "index", (rows,), torch.int32), buf(n + "count", (1,), torch.int32)
                    if not st.get(n + "index_ready"):           # the shape's key holds the boxes: filled once
                        lib.window_ray_index(win, Hr, Wr, dev, out=(index, count))
                        st[n + "index_ready"] = True
                    sel = dict(ray_index=index, ray_count=count, n_out=rows)
                return lib.render_rays_raw(rays, tex_, None, exts, ixts, tar_ext, self._packed_weights(f"nerf_{i}_{who}"), n_samples=Ns,
                                           depth_inv=inv, F=F, render_scale=cas.render_scale[i], maps=maps,
                                           out=(buf(n + "raw", (1, rows, Ns, 4)), buf(n + "z", (1, rows, Ns))), **sel)
            fg, wins = [], []
            for l in range(L):
                prev[l] = cascade(f"layer{l}", nfs[l], prev[l], cas.volume_planes[i], f_i, _scaled_box(boxes[l], cas.volume_scale[i]))
                if render:
                    wins.append(_scaled_box(boxes[l], cas.render_scale[i]))
                    fg.append(raw_samples(f"layer{l}", tex, prev[l], wins[-1]))
            hook(f"level{i}_foreground")
            prev_bg = cascade("bg", nfs[L], prev_bg, BG_PLANES[i], fbg_i, None)
            if render:
                bg = raw_samples("bg", tex_bg, prev_bg, None)
                N, T = Hr * Wr, (L + 1) * Ns
                out = {"rgb": buf(f"out{i}.rgb", (N, 3)), "depth": buf(f"out{i}.depth", (N,)), "weights": buf(f"out{i}.weights", (N, T)),
                       "net_output": buf(f"out{i}.net_output", (N, T, 4)), "z_vals": buf(f"out{i}.z_vals", (N, L * Ns))}
                lib.composite_layers([(r[0], z[0]) for r, z in fg], wins, (bg[0][0], bg[1][0]), Hr, Wr, white_bkgd=False, out=out)
                ret.update({f"{k}_level{i}": v.unsqueeze(0) for k, v in out.items()})
            hook(f"level{i}_background" + ("+composite" if render else ""))
        self.intermediates = inter
        return ret

    # -- source-view cache (enerf_amd/composite_cache.py) -------------------------------------------
    def cache_sources(self, inps, bg_inps, exts, ixts, chunk: int = 0, raw=None):
        """What both FeatureNets make of the V views a time frame draws its source views from, the render texels (the
        foreground's coloured by ``inps``, the background's by ``bg_inps``) and the cameras, computed once: ``inps`` / ``bg_inps``
        (V,3,H,W) float32 in [-1,1] or (V,H,W,3) uint8, ``exts`` (V,4,4), ``ixts`` (V,3,3).  Eval mode only.
        ``CompositeSourceCache.rebuild`` takes the next time frame in place.  ``raw`` (a :class:`enerf_amd.raw_ingest.RawIngest`):
        uint8 images are RAW camera frames (V,Hraw,Wraw,3), undistorted, resized and cropped on the device; ``ixts`` = ``raw.ixts``."""
        from .composite_cache import CompositeSourceCache
        return CompositeSourceCache(self, inps, bg_inps, exts, ixts, chunk, raw)

    def forward_cached(self, cache, view_idx, batch):
        """``forward`` with the source views named by ``view_idx`` — an int32 DEVICE tensor (S,) or (1,S), e.g. the output of
        ``EnerfLib.select_views`` — taken from ``cache``; ``batch`` carries ``tar_ext``, ``tar_ixt``, ``near_far`` (1,L+1,2), ``bbox``
        and optionally ``rays_{i}``.  The index is never read on the host; anything else that holds integer indices is converted
        and uploaded first.  Same output dict, ``intermediates``, per-shape buffers and ``options`` as ``forward``, bit for bit its
        frame on those views; always ONE C call (``enerf_forward_composite_cached``), whatever ``driver`` is."""
        if self.training:
            raise RuntimeError("network_composite: inference only — forward_cached() has no training path; call net.eval()")
        if self.stage_hook is not None:
            raise RuntimeError("network_composite: forward_cached is one C call and has no staged form: clear stage_hook "
                               "(per-stage timing runs forward on hand-gathered views)")
        if cache.packed_gen != self._packed_gen:
            raise RuntimeError("forward_cached: the cache is empty or the network's weights changed (load_state_dict / .to()) after "
                               "it was built; rebuild it (cache.rebuild(...)) or call cache_sources again")
        if not torch.is_tensor(view_idx):
            import numpy as np
            view_idx = torch.from_numpy(np.ascontiguousarray(view_idx))
        if view_idx.is_floating_point() or view_idx.dtype == torch.bool or view_idx.dim() not in (1, 2) or \
                (view_idx.dim() == 2 and view_idx.shape[0] != 1):
            raise ValueError("forward_cached: view_idx must hold integer view indices, (S,) or (1,S)")
        if view_idx.dtype != torch.int32 or view_idx.device != cache.device or not view_idx.is_contiguous():
            view_idx = view_idx.to(device=cache.device, dtype=torch.int32).contiguous()
        dev, L = cache.device, self.num_fg_layers
        if batch["tar_ext"].device != dev:
            raise ValueError("forward_cached: cache and batch must live on one device")
        S, H, W = int(view_idx.numel()), cache.H, cache.W
        moving = self._is_moving(batch)
        boxes = [(0.0, 0.0, w, h) for w, h in self._sizes(batch)] if moving else self._boxes(batch)
        near_far = batch["near_far"]
        if tuple(near_far.shape) != (1, L + 1, 2):
            raise ValueError(f"network_composite: near_far must be (1, {L + 1}, 2): one range per foreground layer, the background's last")
        own_rays = tuple(batch.get(f"rays_{i}") is not None for i in range(self.cfg.cas.num))
        st, buf = self._shape_buffers(("cached-moving", H, W, S, tuple(b[2:] for b in boxes), own_rays, dev) if moving
                                      else ("cached", H, W, S, tuple(boxes), own_rays, dev))
        held = self._holder(buf, dev)
        tar_ext, tar_ixt = held("tar_ext", batch["tar_ext"], (1, 4, 4)), held("tar_ixt", batch["tar_ixt"], (1, 3, 3))
        nfs = buf("near_far", (L + 1, 1, 2))
        nfs.copy_(near_far.reshape(L + 1, 1, 2))
        return self._forward_call(batch, st, buf, held, boxes, (None, None, None, None, tar_ext, tar_ixt, nfs), S, H, W, cache, view_idx,
                                  bbox_xy=self._positions(batch, held) if moving else None)

    def _forward_call(self, batch, st, buf, held, boxes, inputs, S, H, W, cache=None, view_idx=None, bbox_xy=None):
        """The frame as ONE C call (enerf_forward_composite): the shape's outputs, depth / std maps and one workspace tensor are handed
        to the driver, which runs the stages of the staged path below ``forward`` itself — same kernels, same bits — with the
        foreground layers forked onto the library's side lane unless ``options.single_stream``.  With ``cache`` and ``view_idx`` it is
        the cached frame (enerf_forward_composite_cached): no images, source cameras or FeatureNet weights in the argument block.
        With ``bbox_xy`` (the (L,2) float32 device tensor of a batch with ``bbox_size``) ``boxes`` are (0, 0, w, h), the shape is keyed
        by the sizes and the entry is enerf_forward_composite_moving / _cached_moving, which reads the positions on the device."""
        cas, lib, L = self.cfg.cas, self.lib, self.num_fg_layers
        whos = [f"layer{l}" for l in range(L)] + ["bg"]
        a = st.get("call.args")
        if a is None:                                   # everything that belongs to the shape: filled once
            a = CompositeFrameArgs(L=L, S=S, H=H, W=W, cas=cascade_struct(self.cfg))
            for l, box in enumerate(boxes):
                for k in range(4):
                    a.bbox[l][k] = float(box[k])
            if cache is None:
                a.feature_net_packed = self._packed_weights("feature_net").data_ptr()
                a.feature_net_bg_packed = self._packed_weights("feature_net_bg").data_ptr()
            outs, inter = {}, {}
            for i in range(cas.num):
                a.bg_volume_planes[i] = BG_PLANES[i]
                h, w = int(H * cas.volume_scale[i]), int(W * cas.volume_scale[i])
                Hr, Wr = int(H * cas.render_scale[i]), int(W * cas.render_scale[i])
                for c, who in enumerate(whos):
                    a.cost_reg_packed[i][c] = self._packed_weights(f"cost_reg_{i}_{who}").data_ptr()
                    maps = (buf(f"{who}.{i}.depth", (1, h, w)), buf(f"{who}.{i}.std", (1, h, w)))
                    a.depth_map[i][c], a.std_map[i][c] = maps[0].data_ptr(), maps[1].data_ptr()
                    inter[f"depth_{i}_{who}"], inter[f"std_{i}_{who}"] = maps
                    if cas.render_if[i]:
                        a.nerf_packed[i][c] = self._packed_weights(f"nerf_{i}_{who}").data_ptr()
                if cas.render_if[i]:
                    N, Ns = Hr * Wr, cas.num_samples[i]
                    T = (L + 1) * Ns
                    out = {"rgb": buf(f"out{i}.rgb", (N, 3)), "depth": buf(f"out{i}.depth", (N,)), "weights": buf(f"out{i}.weights", (N, T)),
                           "net_output": buf(f"out{i}.net_output", (N, T, 4)), "z_vals": buf(f"out{i}.z_vals", (N, L * Ns))}
                    for k, v in out.items():
                        getattr(a, k)[i] = v.data_ptr()
                    outs.update({f"{k}_level{i}": v.unsqueeze(0) for k, v in out.items()})
            st["call.outs"], st["call.inter"] = outs, inter
        src4, bg4, exts, ixts, tar_ext, tar_ixt, nfs = inputs
        if cache is None:
            a.src_inps, a.bg_src_inps, a.src_exts, a.src_ixts = src4.data_ptr(), bg4.data_ptr(), exts.data_ptr(), ixts.data_ptr()
        a.tar_ext, a.tar_ixt, a.near_far = tar_ext.data_ptr(), tar_ixt.data_ptr(), nfs.data_ptr()
        for i in range(cas.num):
            rays = batch.get(f"rays_{i}") if cas.render_if[i] else None
            if rays is not None:
                n = int(H * cas.render_scale[i]) * int(W * cas.render_scale[i])
                if tuple(rays.shape) != (1, n, 8):
                    raise ValueError(f"network_composite: rays_{i} must be the full (1, {n}, 8) raster of the level")
                rays = held(f"rays{i}", rays, (1, n, 8))
            a.rays[i] = None if rays is None else rays.data_ptr()
        opts = self.options                              # (kept alive by self for the length of the call)
        a.options = None if opts is None else C.pointer(opts)
        if "call.args" not in st:                        # one workspace per shape, sized by the plan (which refuses a bad frame here)
            if bbox_xy is not None:
                nbytes = lib.forward_composite_moving_workspace_bytes(a, None if cache is None else cache.struct)
            else:
                nbytes = lib.forward_composite_workspace_bytes(a) if cache is None else lib.forward_composite_cached_workspace_bytes(a, cache.struct)
            ws = buf("call.ws", ((nbytes + 3) // 4,))
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel() * 4
            st["call.args"] = a
        if bbox_xy is not None:
            flags = buf("bbox_flags", (L,), torch.int32)
            lib.forward_composite_moving(a, bbox_xy.data_ptr(), flags.data_ptr(), lib.stream_of(tar_ext),
                                         None if cache is None else cache.struct, None if cache is None else view_idx.data_ptr())
            self.intermediates = dict(st["call.inter"], bbox_flags=flags)
            return dict(st["call.outs"])
        if cache is None:
            lib.forward_composite(a, lib.stream_of(src4))
        else:
            lib.forward_composite_cached(a, cache.struct, view_idx.data_ptr(), lib.stream_of(tar_ext))
        self.intermediates = dict(st["call.inter"])
        return dict(st["call.outs"])
