"""Evaluator-shaped consumer of the rendered frame that keeps the images on the device.

Mirrors the part of ``lib/evaluators/enerf.py`` the hot path can serve: masked / centre-cropped PSNR per rendered level
(:45-71) and the NeRF / MVS depth statistics (:88-103), same ``evaluate(output, batch)`` / ``summarize()`` surface, so
``run.py:69-70`` can call it in place of the skimage/numpy evaluator.  The reductions run in ``enerf_eval_stats`` (io.hip):
one 48-byte D2H copy per (frame, level) instead of the fp32 images.  With ``eval_ssim=True`` the evaluators' second number, SSIM
(:76: skimage's ``structural_similarity(gt, pred, multichannel=True)`` on the mask-zeroed, centre-cropped images), comes from
``enerf_eval_ssim`` in the same way and the copy grows to 64 bytes.  ``DeviceEvaluatorHuman`` is the counterpart of
``lib/evaluators/enerf_human.py`` (``mask_at_box`` at the last level, SSIM on the mask's bounding rectangle).  With
``eval_lpips=LpipsWeights`` the third number, LPIPS (:81-87: ``lpips.LPIPS(net='vgg')`` on the same mask-zeroed, cropped images), comes
from ``enerf_eval_lpips`` (the VGG16 trunk as fp32-MFMA HIP kernels) and the same copy grows by 48 bytes.  The package ships the
code, not the network's weights: those are the user's (``enerf_amd.lpips.LpipsWeights.from_state_dict``).
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .config import EnerfConfig
from .lib import EnerfLib, get_lib, stats_from_acc
from .lpips import LpipsWeights

LPIPS_MIN_EXTENT = 16      # under 16 pixels the fourth pool leaves nothing for relu5_3: such a level's lpips is NaN


def nearest_resize_index(src: int, dst: int, device) -> torch.Tensor:
    """Source index of every destination pixel along one axis under cv2.resize(..., interpolation=cv2.INTER_NEAREST):
    ``min(floor(d * (1 / (dst / src))), src - 1)`` in double precision (OpenCV resizeNN)."""
    inv = 1.0 / (float(dst) / float(src))
    idx = torch.floor(torch.arange(dst, dtype=torch.float64) * inv).to(torch.int64).clamp_(max=src - 1)
    return idx.to(device)


class DeviceEvaluator:
    def __init__(self, cfg: EnerfConfig, eval_center: bool = False, eval_depth: bool = False,
                 lib: Optional[EnerfLib] = None, eval_ssim: bool = False, eval_lpips: Optional[LpipsWeights] = None):
        self.cfg, self.eval_center, self.eval_depth, self.eval_ssim = cfg, eval_center, eval_depth, eval_ssim
        self.eval_lpips = eval_lpips
        self._lib = lib
        self.reset()

    def reset(self):
        self.psnrs: List[float] = []
        self.level_psnrs: Dict[int, List[float]] = {}
        self.ssims: List[float] = []
        self.level_ssims: Dict[int, List[float]] = {}
        self.lpips: List[float] = []
        self.level_lpips: Dict[int, List[float]] = {}
        self.abs, self.acc_2, self.acc_10 = [], [], []
        self.mvs_abs, self.mvs_acc_2, self.mvs_acc_10 = [], [], []

    @property
    def lib(self) -> EnerfLib:
        if self._lib is None:
            self._lib = get_lib()
        return self._lib

    def evaluate(self, output: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]):
        """evaluators/enerf.py:38-103 (PSNR and depth parts)."""
        cas = self.cfg.cas
        B, S, _, H, W = batch["src_inps"].shape
        for i in range(cas.num):
            if not cas.render_if[i]:
                continue
            h, w = int(H * cas.render_scale[i]), int(W * cas.render_scale[i])
            crop = (int(h * 0.1), int(w * 0.1)) if self.eval_center else (0, 0)
            for b in range(B):
                pred = output[f"rgb_level{i}"][b].contiguous()
                gt = batch[f"rgb_{i}"][b].reshape(h * w, 3).contiguous()
                mask = batch[f"msk_{i}"][b].reshape(h * w).contiguous()
                depth_args = {}
                last = i == cas.num - 1
                if self.eval_depth and last and "tar_dpt" in batch:
                    depth_args = dict(pred_depth=output[f"depth_level{i}"][b].contiguous(),
                                      gt_depth=batch["tar_dpt"][b].reshape(-1).contiguous())
                if self.eval_ssim or self.eval_lpips is not None:
                    st = self._stats_and_ssim(i, last, pred, gt, mask, (h, w), crop, depth_args)
                else:
                    st = self.lib.eval_stats(pred, gt, mask, image_hw=(h, w), crop=crop, **depth_args)
                self.level_psnrs.setdefault(i, []).append(st["psnr"])
                if last:
                    self.psnrs.append(st["psnr"])
                    if "abs" in st:
                        self.abs.append(st["abs"]); self.acc_2.append(st["acc_2"]); self.acc_10.append(st["acc_10"])
                    mvs_key = f"depth_mvs_level{i}"
                    if depth_args and mvs_key in output:
                        # :91-103 — the cost-volume depth map against the ground truth resized to ITS resolution with
                        # cv2.INTER_NEAREST (src index = min(floor(dst * src/dst), src-1)), gathered on the device
                        mvs = output[mvs_key][b]
                        gt_map = batch["tar_dpt"][b].reshape(h, w)
                        ys = nearest_resize_index(h, mvs.shape[0], mvs.device)
                        xs = nearest_resize_index(w, mvs.shape[1], mvs.device)
                        mvs_gt = gt_map.index_select(0, ys).index_select(1, xs).contiguous()
                        ms = self.lib.depth_stats(mvs.contiguous(), mvs_gt)
                        if ms:
                            self.mvs_abs.append(ms["abs"]); self.mvs_acc_2.append(ms["acc_2"]); self.mvs_acc_10.append(ms["acc_10"])

    def _stats_and_ssim(self, level, last, pred, gt, mask, hw, crop, depth_args, bbox=False, mask_is_one=False) -> dict:
        """psnr / depth accumulator, SSIM and LPIPS of one image: up to three enqueued calls, ONE blocking D2H copy for all of them
        (48 bytes, + 16 with SSIM, + 48 with LPIPS).  LPIPS needs its rectangle on the host (it fixes the launch geometry of
        thirteen layers): with ``bbox`` that is one more small blocking copy per image, the 16 bytes of ``mask_bbox``."""
        parts = [self.lib.eval_stats(pred, gt, mask, image_hw=hw, crop=crop, sync=False, **depth_args)]
        if self.eval_ssim:
            parts.append(self.lib.eval_ssim(pred, gt, mask, image_hw=hw, crop=crop, bbox=bbox, mask_is_one=mask_is_one,
                                            sync=False).reshape(-1))
        too_small = False
        if self.eval_lpips is not None:
            rect = self.lib.mask_bbox(mask, hw, mask_is_one=mask_is_one)[0] if bbox else None
            rh, rw = (rect[3], rect[2]) if bbox else (hw[0] - 2 * crop[0], hw[1] - 2 * crop[1])
            too_small = rh < LPIPS_MIN_EXTENT or rw < LPIPS_MIN_EXTENT
            if not too_small:
                parts.append(self.lib.eval_lpips(self.eval_lpips.packed(self.lib), pred, gt, mask, image_hw=hw, crop=crop, rect=rect,
                                                 mask_is_one=mask_is_one, sync=False).reshape(-1))
        both = torch.cat(parts).cpu().tolist()
        if self.eval_ssim:
            self.level_ssims.setdefault(level, []).append(both[6])
            if last:
                self.ssims.append(both[6])
        if self.eval_lpips is not None:
            lp = float("nan") if too_small else both[-6]
            self.level_lpips.setdefault(level, []).append(lp)
            if last:
                self.lpips.append(lp)
        return stats_from_acc(both[:6])

    def summarize(self) -> dict:
        mean = lambda v: sum(v) / len(v) if v else float("nan")
        ret = {"psnr": mean(self.psnrs)}
        ret.update({f"psnr_level{i}": mean(v) for i, v in self.level_psnrs.items()})
        if self.eval_ssim:
            ret["ssim"] = mean(self.ssims)
            ret.update({f"ssim_level{i}": mean(v) for i, v in self.level_ssims.items()})
        if self.eval_lpips is not None:
            ret["lpips"] = mean(self.lpips)
            ret.update({f"lpips_level{i}": mean(v) for i, v in self.level_lpips.items()})
        if self.abs:
            ret.update(abs=mean(self.abs), acc_2=mean(self.acc_2), acc_10=mean(self.acc_10))
        if self.mvs_abs:                 # the reference accumulates these (:101-103) but never prints them; reported here
            ret.update(mvs_abs=mean(self.mvs_abs), mvs_acc_2=mean(self.mvs_acc_2), mvs_acc_10=mean(self.mvs_acc_10))
        self.reset()
        return ret


class DeviceEvaluatorHuman(DeviceEvaluator):
    """``lib/evaluators/enerf_human.py:29-84`` on the device: the mask is ``mask_at_box`` at the last cascade level and all ones
    at the others (:39-42), selected by ``== 1`` (:54); psnr over the selected pixels (:58); SSIM on the selected pixels'
    bounding rectangle with everything else zeroed (:55-56,64-66).  The rectangle is found on the device.  ``summarize()``
    returns ``psnr``, ``ssim`` (last level) and both per rendered level; no depth statistics, as in the reference.  With
    ``eval_lpips=LpipsWeights`` also ``lpips`` (:71-77) on the same rectangle: the device-found rectangle fixes every later launch
    geometry, so it is read back first — one more small blocking copy (16 bytes) per masked image."""

    def __init__(self, cfg: EnerfConfig, lib: Optional[EnerfLib] = None, eval_lpips: Optional[LpipsWeights] = None):
        super().__init__(cfg, eval_center=False, eval_depth=False, lib=lib, eval_ssim=True, eval_lpips=eval_lpips)

    def evaluate(self, output: Dict[str, torch.Tensor], batch: Dict[str, torch.Tensor]):
        cas = self.cfg.cas
        B, S, _, H, W = batch["src_inps"].shape
        for i in range(cas.num):
            if not cas.render_if[i]:
                continue
            h, w = int(H * cas.render_scale[i]), int(W * cas.render_scale[i])
            last = i == cas.num - 1
            for b in range(B):
                pred = output[f"rgb_level{i}"][b].reshape(h * w, 3).contiguous()
                gt = batch[f"rgb_{i}"][b].reshape(h * w, 3).contiguous()
                mask = None
                if last:                                                # any dtype the dataset hands over; == 1 decided here
                    mask = (batch["mask_at_box"][b].reshape(h * w) == 1).to(torch.uint8)
                st = self._stats_and_ssim(i, last, pred, gt, mask, (h, w), (0, 0), {}, bbox=mask is not None, mask_is_one=True)
                self.level_psnrs.setdefault(i, []).append(st["psnr"])
                if last:
                    self.psnrs.append(st["psnr"])
