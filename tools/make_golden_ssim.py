#!/usr/bin/env python
"""Generate tests/golden/ssim_cases.npz: what the reference's evaluators get from skimage for the cases of tests/ssim_cases.py.

Needs numpy and scikit-image 0.18.x (the line on which the reference's ``ssim(gt, pred, multichannel=True)`` runs); no torch,
nothing from the reference tree.  The preprocessing in front of the call is restated from lib/evaluators/enerf.py:48-54,67-69,76
and lib/evaluators/enerf_human.py:39-42,54-56,64-66, line by line, on copies of the arrays.

    python tools/make_golden_ssim.py            # writes the fixture
    python tools/make_golden_ssim.py --time     # also times one skimage call at 512x640 and 1024x1024 (printed as JSON)

The fixture holds, per case: ``expected/<case>`` (B,) float64, ``windows/<case>`` (B,) int64 = (h-6)(w-6) of the image handed to
skimage, ``sha1/<case>/<array>`` of the inputs, and ``meta/*`` (library versions, how the values were produced)."""
from __future__ import annotations

import inspect
import json
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ssim_cases  # noqa: E402

from skimage.metrics import structural_similarity as ssim  # noqa: E402

if "multichannel" not in inspect.signature(ssim).parameters:
    sys.exit("this scikit-image's structural_similarity has no `multichannel` argument: the reference's call does not run on "
             "it; use scikit-image 0.18.x")


def bounding_rect(mask_u8: np.ndarray):
    """cv2.boundingRect of a uint8 mask: (x, y, w, h) of the non-zero pixels, (0,0,0,0) when there are none."""
    try:
        import cv2
        return cv2.boundingRect(mask_u8)
    except ImportError:
        ys, xs = np.nonzero(mask_u8)
        if ys.size == 0:
            return 0, 0, 0, 0
        return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


def evaluator_images(case: dict, b: int):
    """The two (h,w,3) float32 arrays the evaluator hands to ssim() for image b."""
    pred_rgb, gt_rgb = case["pred"].copy(), case["gt"].copy()
    B, h, w, _ = pred_rgb.shape
    if case["evaluator"] == "enerf":
        msk = case["mask"] if case["mask"] is not None else np.ones((B, h, w), np.uint8)
        masks = (msk.reshape(B, h, w) >= 1).astype(np.uint8)                                   # enerf.py:48
        if case["center"]:                                                                     # :50-54
            H_crop, W_crop = int(h * 0.1), int(w * 0.1)
            pred_rgb = pred_rgb[:, H_crop:-H_crop, W_crop:-W_crop]
            gt_rgb = gt_rgb[:, H_crop:-H_crop, W_crop:-W_crop]
            masks = masks[:, H_crop:-H_crop, W_crop:-W_crop]
        mask = masks[b] == 1                                                                   # :67-69
        gt_rgb[b][mask == False] = 0.                                                          # noqa: E712
        pred_rgb[b][mask == False] = 0.                                                        # noqa: E712
        return gt_rgb[b], pred_rgb[b]                                                          # :76
    masks = case["mask"] if case["mask"] is not None else np.ones_like(pred_rgb[..., 0])       # enerf_human.py:39-42
    mask = masks[b] == 1                                                                       # :54-56
    gt_rgb[b][mask == False] = 0.                                                              # noqa: E712
    pred_rgb[b][mask == False] = 0.                                                            # noqa: E712
    x, y, w, h = bounding_rect(mask.astype(np.uint8))                                          # :64
    return gt_rgb[b][y:y + h, x:x + w], pred_rgb[b][y:y + h, x:x + w]                          # :66


def main():
    import scipy
    import skimage
    out = {}
    for name in ssim_cases.CASE_NAMES:
        case = ssim_cases.build(name)
        vals, wins = [], []
        for b in range(case["pred"].shape[0]):
            gt, pred = evaluator_images(case, b)
            assert gt.dtype == np.float32 and pred.dtype == np.float32
            vals.append(float(ssim(gt, pred, multichannel=True)))                              # the reference's call
            wins.append((gt.shape[0] - 6) * (gt.shape[1] - 6))
        out[f"expected/{name}"] = np.asarray(vals, np.float64)
        out[f"windows/{name}"] = np.asarray(wins, np.int64)
        for k, v in ssim_cases.sha1s(case).items():
            out[f"sha1/{name}/{k}"] = np.asarray(v)
        print(f"{name:10s} {case['pred'].shape} -> {vals}")
    out["meta/skimage"] = np.asarray(skimage.__version__)
    out["meta/scipy"] = np.asarray(scipy.__version__)
    out["meta/numpy"] = np.asarray(np.__version__)
    out["meta/produced_by"] = np.asarray("skimage.metrics.structural_similarity(gt, pred, multichannel=True)")
    path = os.path.join(ROOT, "tests", "golden", "ssim_cases.npz")
    np.savez(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    if "--time" in sys.argv:
        res = {"cpu": platform.processor() or platform.machine(), "threads": 1, "skimage": skimage.__version__}
        try:
            with open("/proc/cpuinfo") as f:
                res["cpu"] = next(l.split(":", 1)[1].strip() for l in f if l.startswith("model name"))
        except (OSError, StopIteration):
            pass
        for name in ("full_dtu", "full_zju"):
            case = ssim_cases.build(name)
            h, w = case["pred"].shape[1:3]
            gt, pred = case["gt"][0], case["pred"][0]                                            # the whole image, no mask
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                ssim(gt, pred, multichannel=True)
                ts.append(time.perf_counter() - t0)
            res[f"skimage_ms_{h}x{w}"] = round(1e3 * sorted(ts)[len(ts) // 2], 2)
        print("TIMING " + json.dumps(res))


if __name__ == "__main__":
    main()
