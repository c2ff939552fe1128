"""Training-mode forward of the composite network (``network_composite.Network(..., trainable=True)`` in ``.train()`` mode): the
reference's ``network_composite.py:77-146`` with autograd, on the network's own parameter modules.

It is the plain training path (``train_path.py``, ``autograd.py``) run once per cascade — ``num_fg_layers`` boxed foreground layers
and the background — plus the three stages only this network has, each a ``torch.autograd.Function`` over a forward entry the
inference path already uses and a backward kernel of its own:

  * ``WindowFeatureVolumeFn``    the cost volume of a layer's window (``enerf_build_feature_volume_window`` / ``_window_bwd``);
  * ``WindowDepthRegressionFn``  F.pad + depth_regression without the padded prob (``enerf_depth_regression_window`` / ``_window_bwd``):
                                 depth / std over the full grid, so the next level's align-corners upsampling and the ray builder read
                                 past the window's edge exactly as in the reference;
  * ``CompositeLayersFn``        parse_layer + raw2outputs_composite (``enerf_composite_layers`` / ``_bwd``).

Per cascade and level: ``get_depth_values`` with the cascade's own row of ``batch['near_far']`` (``DepthValuesFn`` after level 0: the
masked in-place clamps pass the gradient through the un-clamped branch only, ``near_far`` detached; a level after a depth-space level
raises, as in ``forward_train``), the (windowed) volume, the MinCostRegNet through ``cost_reg_train`` — batch statistics over the
window's voxels, running statistics updated as the reference's modules update them (a window whose ``D``, ``wh`` or ``ww`` is not
divisible by 4 is refused by layer and window before its volume is built); with frozen BatchNorm (``bn.eval()``) through the
modules —, the (windowed) regression, and on a rendered level ``RaySamplesFn`` + ``TexelsFn`` + ``GatherFn`` + the fused MLP on the
cascade's rays.  Both FeatureNets run through ``feature_net_forward``.

The ``nerf_.py`` head ignores the voxel feature: it runs on ``enerf_nerf_mlp_fwd`` / ``_bwd`` with zero voxel inputs and zero weight
columns in their place (``_PaddedHead``: the padding ``NerfCompositeParams.raw()`` does for inference, as two differentiable
``torch.cat`` per head whose backward slices the ``lr0`` / ``color.0`` gradients back).  A cost-reg net's ``feat_conv`` is on no
path to the loss: it receives a zero gradient (the reference leaves it ``None``).

Still torch glue, none of it on a hot path: the two ``torch.cat`` per head, cropping the batch's ray raster to a layer's window
(input preparation, one index), a zero volume per rendered level for the gather's voxel fetch (the inference kernel takes a NULL
volume instead), ``1 / z`` of the returned sample depths at a disparity-space level (one library launch, ``enerf_reciprocal``).

``B == 1``, as everywhere in this network.  ``batch`` is not mutated (the reference leaves ``batch['near_far']`` two-dimensional behind
it).  Out of scope: ``idx_level{i}``, ``GraphedTrainStep`` capture, DDP runs.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Dict

import torch

from .lib import NerfRaw


class _PaddedHead:
    """A ``NerfCompositeParams`` as the ``NerfParams`` that ``autograd.NerfMlpFn`` drives: ``lr0`` (64, 8 + 16) and ``color.0``
    (64, 64 + 8 + 16 + F + 4) with zero columns where nerf.py's head reads the eight voxel inputs.  The padded weights are
    differentiable functions of the module's parameters; every other entry is the module's own."""

    def __init__(self, m):
        self._m = m
        lr0, col0 = m.lr0[0].weight, m.color[0].weight
        self.lr0_w = torch.cat([lr0.new_zeros(lr0.shape[0], 8), lr0], 1)
        self.col0_w = torch.cat([col0[:, :64], col0.new_zeros(col0.shape[0], 8), col0[:, 64:]], 1)
        self.feat_ch, self.viewdir_agg, self.agg, self.sigma = m.feat_ch, m.viewdir_agg, m.agg, m.sigma
        self.lr0 = [SimpleNamespace(weight=self.lr0_w, bias=m.lr0[0].bias)]
        self.color = [SimpleNamespace(weight=self.col0_w, bias=m.color[0].bias), None, m.color[2]]
        swap = {"lr0.0.weight": self.lr0_w, "color.0.weight": self.col0_w}
        self._params = [(n, swap.get(n, p)) for n, p in m.named_parameters()]

    def named_parameters(self):
        return list(self._params)

    def raw(self) -> NerfRaw:
        """The layouts enerf_nerf_pack reads: the module's own padded copies, alive as long as this object (NerfMlpFn keeps it)."""
        r, self._held = self._m.raw()
        return r


def forward_train_composite(net, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The reference's output dict per rendered level: ``rgb``, ``depth``, ``weights`` (differentiable), ``net_output`` and
    ``z_vals`` — both returned DETACHED: they are the sorted samples and the concatenated sample depths, data movement the loss
    does not read — each suffixed ``_level{i}``; no ``idx`` (see the module docstring of network_composite.py)."""
    from .autograd import (CompositeLayersFn, DepthRegressionFn, DepthValuesFn, FeatureVolumeFn, GatherFn, RaySamplesFn, TexelsFn,
                           WindowDepthRegressionFn, WindowFeatureVolumeFn, check_cost_reg_train_shape, cost_reg_train, nerf_mlp)
    from .network_composite import BG_PLANES, _scaled_box
    from .train_path import _hip_lib, _need, camera_tables, cost_reg_forward, feature_net_forward
    cas, L = net.cfg.cas, net.num_fg_layers
    src = batch["src_inps"]
    lib = _need(_hip_lib(net, src), "composite training step")
    B, S, _, H, W = src.shape
    if B != 1:
        raise ValueError("network_composite: B must be 1 (the reference reads batch['bbox'][0] for every batch element)")
    boxes = net._boxes(batch)
    near_far = batch["near_far"].detach()
    if tuple(near_far.shape) != (1, L + 1, 2):
        raise ValueError(f"network_composite: near_far must be (1, {L + 1}, 2): one range per foreground layer, the background's last")
    nf_rows = [near_far[:, c].contiguous() for c in range(L + 1)]          # (1, 2) per cascade, the background's last

    def level_maps(m):
        f2, f1, f0 = feature_net_forward(m, src.view(S, 3, H, W), lib)
        return {2: f0.reshape(1, S, f0.shape[1], H, W), 1: f1.reshape(1, S, f1.shape[1], H // 2, W // 2),
                0: f2.reshape(1, S, f2.shape[1], H // 4, W // 4)}
    feats, feats_bg = level_maps(net.feature_net), level_maps(net.feature_net_bg)       # both read src_inps (network_composite.py:78-79)
    tables = camera_tables(cas, batch, lib)
    ret: Dict[str, torch.Tensor] = {}
    inter: Dict[str, torch.Tensor] = {}
    prev = [None] * (L + 1)
    for i in range(cas.num):
        hv, wv = int(H * cas.volume_scale[i]), int(W * cas.volume_scale[i])
        Hr, Wr = int(H * cas.render_scale[i]), int(W * cas.render_scale[i])
        inv, Ns, P = bool(cas.depth_inv[i]), cas.num_samples[i], tables[f"proj_{i}"]
        render = bool(cas.render_if[i])
        if render:
            k = cas.render_im_feat_level[i]
            if tuple(feats[k].shape[-2:]) != (Hr, Wr) or feats[k].shape[2] != cas.nerf_model_feat_ch[i]:
                raise RuntimeError("network_composite: render_im_feat_level must name the feature map at the render resolution")
            rays = batch.get(f"rays_{i}")
            if rays is None:
                rays = lib.gen_rays(batch["tar_ext"].contiguous(), batch["tar_ixt"].contiguous(), Hr, Wr, cas.render_scale[i])
            elif tuple(rays.shape) != (1, Hr * Wr, 8):
                raise ValueError(f"network_composite: rays_{i} must be the full (1, {Hr * Wr}, 8) raster of the level")
            tex = TexelsFn.apply(lib, feats[k], src, Hr, Wr)
            tex_bg = TexelsFn.apply(lib, feats_bg[k], batch["bg_src_inps"], Hr, Wr)
            no_vol = src.new_zeros(1, BG_PLANES[i], hv, wv, 8)              # the head ignores the voxel feature: zeros are fetched
            cam, tcen = tables[f"cam_{i}"], tables["tcen"]

        def cascade(c, who, D, feat, win):
            """One cascade level up to its depth / std maps over the full (hv, wv) grid; ``win``: the layer's window of it, or None."""
            if prev[c] is None:
                dv, nf = lib.get_depth_values(nf_rows[c], None, 1, D, hv, wv, inv)
            else:
                if not cas.depth_inv[i - 1]:
                    raise RuntimeError("cascade levels after a depth-space level are undefined in the reference (utils.py:130)")
                dv, nf = DepthValuesFn.apply(lib, *prev[c], nf_rows[c], D, hv, wv, inv)
            reg = getattr(net, f"cost_reg_{i}_{who}")
            bn_batch = all(m.training for m in reg.modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm))
            if bn_batch:                    # a window is int(bbox * scale): any size.  Refused here, by name, before its volume is built
                try:
                    check_cost_reg_train_shape(bool(reg.full), 1, D, *((hv, wv) if win is None else (win[3], win[2])))
                except ValueError as e:
                    where = "the full grid" if win is None else f"window (x0, y0, ww, wh) = {tuple(win)}"
                    raise ValueError(f"network_composite: cost_reg_{i}_{who}, {where} of the {hv} x {wv} level-{i} grid: {e}") from None
            vol = FeatureVolumeFn.apply(lib, feat, P, dv) if win is None else WindowFeatureVolumeFn.apply(lib, feat, P, dv, win)
            # batch statistics on the HIP training blocks; frozen BatchNorm (bn.eval()) through the modules, as in forward_train
            if bn_batch:
                _, prob = cost_reg_train(lib, reg, vol)
            else:
                _, prob = cost_reg_forward(reg, vol, lib)
            if win is None:
                depth, std = DepthRegressionFn.apply(lib, prob, dv, inv)
            else:
                depth, std = WindowDepthRegressionFn.apply(lib, prob, dv, inv, win)
            inter[f"depth_{i}_{who}"], inter[f"std_{i}_{who}"] = depth.detach(), std.detach()
            prev[c] = (depth, std, nf)

        def raw_samples(c, who, tex_, win):
            """(raw (n, Ns, 4), z (n, Ns)) of the cascade's rays: the window's, raster order, or the whole raster's."""
            r = rays
            if win is not None:
                x0, y0, ww, wh = win
                r = rays.reshape(1, Hr, Wr, 8)[:, y0:y0 + wh, x0:x0 + ww].reshape(1, ww * wh, 8)
            n = r.shape[1]
            z, xyz, dn, uv = RaySamplesFn.apply(lib, *prev[c], r, Ns, Hr, Wr, inv)
            x, vox = GatherFn.apply(lib, xyz.reshape(1, n * Ns, 3), dn.reshape(1, n * Ns), uv.reshape(1, n * Ns, 2), tex_, no_vol, cam, tcen,
                                    Ns, Wr if n == Hr * Wr else 0)
            raw = nerf_mlp(lib, _PaddedHead(getattr(net, f"nerf_{i}_{who}")), None, vox, x).reshape(n, Ns, 4)
            z = z.detach().reshape(n, Ns).contiguous()
            return raw, (lib.reciprocal(z) if inv else z)                   # network_composite.py:48-51

        layers, wins = [], []
        for l in range(L):
            cascade(l, f"layer{l}", cas.volume_planes[i], feats[i], _scaled_box(boxes[l], cas.volume_scale[i]))
            if render:
                wins.append(_scaled_box(boxes[l], cas.render_scale[i]))
                layers.extend(raw_samples(l, f"layer{l}", tex, wins[-1]))
        cascade(L, "bg", BG_PLANES[i], feats_bg[i], None)
        if render:
            bg_raw, bg_z = raw_samples(L, "bg", tex_bg, None)
            out = CompositeLayersFn.apply(lib, wins, Hr, Wr, False, bg_raw, bg_z, *layers)
            ret.update({f"{k}_level{i}": v.unsqueeze(0) for k, v in zip(("rgb", "depth", "weights", "net_output", "z_vals"), out)})
    net.intermediates = inter
    return ret
