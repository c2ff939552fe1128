"""The trainer's loss on the device (lib/train/losses/enerf.py:16-56): MSE per level plus ``0.01 x VGGPerceptualLoss``
(lib/train/losses/vgg_perceptual_loss.py:21-37, resize=False, feature_layers=[0,1,2,3]), the perceptual term forward AND backward on
the library's kernels (csrc/perceptual_vgg.h) — the trainer-side counterpart of ``DeviceEvaluator``.

    weights = PerceptualWeights.from_state_dict(torchvision_vgg16.state_dict(), device)      # the user's: none ship
    loss_fn = EnerfLoss.from_yacs(cfg, weights)                                            # (outputs, batch) -> loss
    step = GraphedTrainStep(net, optimizer, loss_fn, example_batch)

``perceptual_loss`` only enqueues (the float64 loss is converted on the device, the upstream gradient is read on the device), so a
step with it is captured in one hipGraph like a step without; its value and gradient are bit-identical from call to call.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

from .lib import PERCEPTUAL_CONVS, EnerfError, EnerfLib, get_lib
from .lpips import VGG_FEATURE_INDEX, LpipsWeights
from .train_graph import mse_loss

PERCEPTUAL_FEATURE_INDEX = VGG_FEATURE_INDEX[:10]          # torchvision VGG16 ``features`` index of the ten convolutions


class PerceptualWeights:
    """The ten (w, b) pairs of VGG16 ``features[:23]`` on one device, plus the packed image the kernels read (built on first use)."""

    def __init__(self, convs: Sequence[Tuple[torch.Tensor, torch.Tensor]]):
        if len(convs) != 10:
            raise ValueError("PerceptualWeights needs 10 (w, b) pairs")
        for i, ((w, b), (cin, cout)) in enumerate(zip(convs, PERCEPTUAL_CONVS)):
            if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
                raise ValueError(f"conv {i} (features.{PERCEPTUAL_FEATURE_INDEX[i]}): expected ({cout},{cin},3,3) + ({cout},), "
                                 f"got {tuple(w.shape)} + {tuple(b.shape)}")
        self.convs = [(w.detach().to(torch.float32).contiguous(), b.detach().to(torch.float32).contiguous()) for w, b in convs]
        self._packed: Optional[torch.Tensor] = None
        self._packed_by = None

    @property
    def device(self):
        return self.convs[0][0].device

    def packed(self, lib: Optional[EnerfLib] = None) -> torch.Tensor:
        lib = lib or get_lib()
        if self._packed is None or self._packed_by is not lib:
            self._packed, self._packed_by = lib.perceptual_pack(self.convs), lib
        return self._packed

    def state_dict(self) -> Dict[str, torch.Tensor]:
        sd = {}
        for idx, (w, b) in zip(PERCEPTUAL_FEATURE_INDEX, self.convs):
            sd[f"features.{idx}.weight"], sd[f"features.{idx}.bias"] = w, b
        return sd

    @classmethod
    def from_state_dict(cls, sd: Dict[str, torch.Tensor], device) -> "PerceptualWeights":
        """A torchvision VGG16 state dict: ``features.{0,2,5,7,10,12,14,17,19,21}.{weight,bias}`` are taken; the network's other
        entries (the later convolutions, the classifier) belong to layers the term never runs.  A missing key or a wrong shape
        raises."""
        want = [f"features.{idx}.{p}" for idx in PERCEPTUAL_FEATURE_INDEX for p in ("weight", "bias")]
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"PerceptualWeights.from_state_dict: missing {missing}")
        return cls([(sd[f"features.{idx}.weight"].to(device), sd[f"features.{idx}.bias"].to(device)) for idx in PERCEPTUAL_FEATURE_INDEX])

    @classmethod
    def from_lpips_weights(cls, w: LpipsWeights) -> "PerceptualWeights":
        """The trunk is the same network: the first ten convolutions of the evaluator's LPIPS weights."""
        return cls(w.convs[:10])

    @classmethod
    def random(cls, seed: int, device="cpu") -> "PerceptualWeights":
        """Seeded random weights — TEST AND TIMING MATERIAL, not a perceptual term: ``LpipsWeights.random``'s rule (He-normal
        convolutions, biases 0.05 * N(0,1)) and, for the same seed, its first ten layers."""
        g = torch.Generator().manual_seed(int(seed))
        convs = []
        for cin, cout in PERCEPTUAL_CONVS:
            w = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (9 * cin)) ** 0.5
            convs.append((w.to(device), (0.05 * torch.randn((cout,), generator=g)).to(device)))
        return cls(convs)


class _PerceptualLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, packed, hw, lib):
        N = pred.shape[0]
        out, ws = lib.perceptual_fwd(packed, pred, gt, hw)
        ctx.saved = (lib, packed, N, hw, ws)
        ctx.shape = pred.shape
        return lib.cast_f32(out[:1]).reshape(())

    @staticmethod
    def backward(ctx, grad_output):
        lib, packed, N, hw, ws = ctx.saved
        scale = grad_output.detach().to(torch.float32).reshape(1).contiguous()
        return lib.perceptual_bwd(packed, N, hw, ws, scale).reshape(ctx.shape), None, None, None, None


def perceptual_loss(pred: torch.Tensor, gt: torch.Tensor, weights: PerceptualWeights, image_hw: Optional[Tuple[int, int]] = None,
                    lib: Optional[EnerfLib] = None) -> torch.Tensor:
    """``VGGPerceptualLoss()(pred, gt)`` of the reference's trainer for images in [0,1]: ``pred`` / ``gt`` (N, h, w, 3), or
    (N, h*w, 3) with ``image_hw`` = (h, w) — the renderer's own layout, channels-last already: nothing is permuted.  Returns a
    float32 scalar tensor; differentiable with respect to ``pred`` only (``gt`` is a target, the weights are frozen)."""
    lib = lib or get_lib()
    if pred.dim() == 4 and image_hw is None:
        image_hw = (int(pred.shape[1]), int(pred.shape[2]))
    if image_hw is None or pred.shape[-1] != 3 or pred.dim() not in (3, 4) or pred.shape != gt.shape:
        raise EnerfError(f"perceptual_loss: pred / gt must both be (N,h,w,3), or (N,h*w,3) with image_hw; got {tuple(pred.shape)}, {tuple(gt.shape)}")
    h, w = int(image_hw[0]), int(image_hw[1])
    if pred[0].numel() != h * w * 3:
        raise EnerfError(f"perceptual_loss: images of {tuple(pred.shape[1:])} are not {h}x{w}x3")
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise EnerfError("perceptual_loss: float32 images")
    return _PerceptualLoss.apply(pred.contiguous(), gt.detach().contiguous(), weights.packed(lib), (h, w), lib)


class EnerfLoss:
    """``NetworkWrapper.forward``'s loss (lib/train/losses/enerf.py:21-51) as a callable ``(outputs, batch) -> loss`` for
    ``train_graph.train_step`` / ``GraphedTrainStep``.  Per level i: ``loss_weight[i] * MSE``; with ``train_img[i]`` the perceptual
    term on the whole ``int(H*render_scale[i]) x int(W*render_scale[i])`` image, else with ``num_patchs[i] > 0`` on the
    ``num_patchs[i]`` patches of ``patch_size[i]``^2 rays that follow the first ``num_rays[i]`` rays; the term is weighted
    ``0.01 * loss_weight[i]``.  ``scalar_stats`` (``color_mse_i``, ``psnr_i``, ``perceptual_loss_i``, ``loss``: device tensors, no
    host read) is kept on the object after every call.  ``perceptual=None`` leaves the term out.  ``render_scale``: the cascade's
    (``from_yacs`` passes it); without it a level's image size is taken from its ray count and the source images' aspect."""

    def __init__(self, loss_weight: Sequence[float], train_img: Sequence[bool], num_patchs: Sequence[int], patch_size: Sequence[int],
                 num_rays: Sequence[int], perceptual: Optional[PerceptualWeights] = None, render_scale: Optional[Sequence[float]] = None,
                 lib: Optional[EnerfLib] = None):
        self.num = len(loss_weight)
        if not all(len(v) >= self.num for v in (train_img, num_patchs, patch_size, num_rays)):
            raise ValueError("EnerfLoss: every per-level list needs one entry per loss_weight")
        self.loss_weight, self.train_img = [float(v) for v in loss_weight], [bool(v) for v in train_img]
        self.num_patchs, self.patch_size, self.num_rays = [int(v) for v in num_patchs], [int(v) for v in patch_size], [int(v) for v in num_rays]
        self.render_scale = None if render_scale is None else [float(v) for v in render_scale]
        self.perceptual, self.lib = perceptual, lib
        self.scalar_stats: Dict[str, torch.Tensor] = {}

    @classmethod
    def from_yacs(cls, cfg, perceptual: Optional[PerceptualWeights] = None, lib: Optional[EnerfLib] = None) -> "EnerfLoss":
        """From the reference's global ``cfg`` (``cfg.enerf.cas_config``)."""
        cas = cfg.enerf.cas_config
        n = int(cas.num)
        return cls(list(cas.loss_weight)[:n], list(cas.train_img)[:n], list(cas.num_patchs)[:n], list(cas.patch_size)[:n],
                   list(cas.num_rays)[:n], perceptual, list(cas.render_scale)[:n], lib)

    def __call__(self, output: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]) -> torch.Tensor:
        stats: Dict[str, torch.Tensor] = {}
        loss = 0
        for i in range(self.num):
            pred, gt = output[f"rgb_level{i}"], batch[f"rgb_{i}"]
            color = mse_loss(gt, pred)
            stats[f"color_mse_{i}"] = color
            loss = loss + self.loss_weight[i] * color
            stats[f"psnr_{i}"] = -10.0 * torch.log(color.detach()) / 2.302585092994046
            if self.perceptual is None:
                continue
            term = None
            if self.train_img[i]:
                _, _, _, H, W = batch["src_inps"].shape
                if self.render_scale is not None:
                    h, w = int(H * self.render_scale[i]), int(W * self.render_scale[i])
                else:                                   # no render_scale given: the level's scale from its ray count
                    s = (pred.shape[1] / float(H * W)) ** 0.5
                    h, w = int(round(H * s)), int(round(W * s))
                if h * w != pred.shape[1]:
                    raise EnerfError(f"EnerfLoss: level {i} holds {pred.shape[1]} rays, not a {h}x{w} image (train_img needs whole images)")
                term = perceptual_loss(pred.reshape(-1, h * w, 3), gt.reshape(-1, h * w, 3), self.perceptual, (h, w), self.lib)
            elif self.num_patchs[i] > 0:
                ps, n0 = self.patch_size[i], self.num_rays[i]
                cut = lambda t: torch.cat([t[:, n0 + j * ps * ps:n0 + (j + 1) * ps * ps, :] for j in range(self.num_patchs[i])], 0)
                term = perceptual_loss(cut(pred), cut(gt), self.perceptual, (ps, ps), self.lib)
            if term is not None:
                loss = loss + 0.01 * term * self.loss_weight[i]
                stats[f"perceptual_loss_{i}"] = term.detach()
        stats["loss"] = loss
        self.scalar_stats = stats
        return loss
