#!/usr/bin/env python
"""Time the device-side LPIPS (enerf_eval_lpips: the VGG16 trunk as fp32-MFMA kernels + taps) on the GPU, and the same restatement
through torch-ROCm ``F.conv2d`` in fp32 on the same GPU, in the same process and alternating.

    python tools/time_eval_lpips.py --out profiles/eval_lpips_timing.json

Cases: 512x640 centre-cropped (dtu: msk >= 1, eval_center -> 410x512) and 1024x1024 with a bounding rectangle (zju: mask == 1,
603x751 box given as x, y, w, h).  Weights: ``LpipsWeights.random(0)`` (the time does not depend on the values).  All figures are
device-event medians over --samples samples, warm:
  whole_call_ms     one enerf_eval_lpips call (13 conv launches, 5 taps, 1 finish), B = 1: a (pred, gt) pair
  layers            every conv layer ALONE through enerf_vgg_conv3x3 at the layer's own size, N = 2, with its GFLOP (2*9*cin*cout*H*W*N),
                    achieved TF/s and the fraction of the 157.3 TF/s fp32-MFMA peak.  A layer behind a pool is timed here on an already
                    pooled input; inside the call it takes the 2x2 max while staging (four loads per staged value instead of one)
  front_ms          conv 0 through the evaluator front (enerf_lpips_front: mask, rectangle, scaling layer on load)
  taps_and_rest_ms  whole call - (front + layers 1..12): the five tap kernels, the finish and the pool-on-load excess together (the
                    taps have no entry of their own)
  torch_ms          the torch-ROCm restatement on images cropped and scaled beforehand (its preprocessing is not timed)
  ratio             whole_call_ms / torch_ms
The floor of the trunk at the fp32-MFMA peak is recorded per case (2.55 ms per 512x640 pair, uncropped)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TFLOPS = 157.3
POOL_BEFORE = (2, 4, 7, 10)
TAP_AFTER = (1, 3, 6, 9, 12)


def median_ms(fn, samples: int, warmup: int, calls: int = 1) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return statistics.median(out)


def torch_lpips(w, in0, in1):
    """The restatement of tests/lpips_cases.py on the device: (1,3,h,w) in [-1,1] -> lpips (fp32, channels-first, F.conv2d)."""
    shift = torch.tensor([-.030, -.088, -.188], device=in0.device).view(1, 3, 1, 1)
    scale = torch.tensor([.458, .448, .450], device=in0.device).view(1, 3, 1, 1)
    x = (torch.cat([in0, in1]) - shift) / scale
    total = 0.0
    for i, (cw, cb) in enumerate(w.convs):
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = torch.relu(F.conv2d(x, cw, cb, padding=1))
        if i in TAP_AFTER:
            n = x / (torch.sqrt((x ** 2).sum(1, keepdim=True)) + 1e-10)
            lin = w.lins[TAP_AFTER.index(i)].view(1, -1, 1, 1)
            total = total + (lin * (n[:1] - n[1:]) ** 2).sum(1).mean()
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-ROCm comparison")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_eval_lpips: no GPU; timings are taken on the device only")
    from enerf_amd.lib import VGG_CONVS, get_lib
    from enerf_amd.lpips import LpipsWeights
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    lib = get_lib()
    dev = torch.device("cuda:0")
    w = LpipsWeights.random(0, dev)
    packed = w.packed(lib)
    layer_packed = [lib.vgg_conv3x3_pack(cw, cb) for cw, cb in w.convs]
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "samples": a.samples, "peak_fp32_mfma_tflops": PEAK_TFLOPS,
           "how": "device-event medians, warm; see tools/time_eval_lpips.py"}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for tag, (h, wd), human in (("dtu_512x640_center", (512, 640), False), ("zju_1024x1024_bbox", (1024, 1024), True)):
        gt = torch.rand((1, h * wd, 3), generator=g).to(dev)
        pred = (gt + 0.05 * torch.randn((1, h * wd, 3), generator=g).to(dev)).clamp_(0, 1).contiguous()
        if human:
            m = torch.zeros((h, wd), dtype=torch.uint8)
            m[150:901, 200:803] = 1
            mask = m.reshape(1, h * wd).to(dev)
            rect = lib.mask_bbox(mask, (h, wd), mask_is_one=True)[0]
            kw = dict(rect=rect, mask_is_one=True)
            x0, y0, rw, rh = rect
        else:
            mask = (torch.rand((1, h * wd), generator=g) > 0.3).to(torch.uint8).to(dev)
            kw = dict(crop=(int(h * 0.1), int(wd * 0.1)))
            y0, x0 = kw["crop"]
            rh, rw = h - 2 * y0, wd - 2 * x0
        ours = lambda: lib.eval_lpips(packed, pred, gt, mask, image_hw=(h, wd), sync=False, **kw)
        value = ours().cpu()[0].tolist()
        row = {"rect_hw": [rh, rw], "lpips": value[0], "d": value[1:]}
        row["whole_call_ms"] = round(median_ms(ours, a.samples, a.warmup), 4)
        row["front_ms"] = round(median_ms(lambda: lib.lpips_front(packed, pred, gt, mask, image_hw=(h, wd), **kw), a.samples, a.warmup), 4)
        layers, H, W, gflop_total, layer_sum = [], rh, rw, 0.0, row["front_ms"]
        for i, (cin, cout) in enumerate(VGG_CONVS):
            if i in POOL_BEFORE:
                H, W = H // 2, W // 2
            gflop = 2.0 * 9 * cin * cout * H * W * 2 / 1e9
            gflop_total += gflop
            x = torch.rand((2, H, W, cin), generator=g).to(dev)
            ms = median_ms(lambda: lib.vgg_conv3x3(layer_packed[i], cin, cout, x), a.samples, a.warmup)
            if i > 0:
                layer_sum += ms
            tf = gflop / ms                                                  # GFLOP / ms = TFLOP / s
            layers.append({"conv": i, "cin": cin, "cout": cout, "hw": [H, W], "pooled_input": i in POOL_BEFORE, "gflop": round(gflop, 3),
                           "ms": round(ms, 4), "tflops": round(tf, 2), "of_peak": round(tf / PEAK_TFLOPS, 3)})
            del x
        row["layers"] = layers
        row["trunk_gflop"] = round(gflop_total, 2)
        row["floor_ms_at_peak"] = round(gflop_total / PEAK_TFLOPS, 3)
        row["trunk_tflops_in_call"] = round(gflop_total / row["whole_call_ms"], 2)
        row["taps_and_rest_ms"] = round(row["whole_call_ms"] - layer_sum, 4)
        res[tag] = row
        print(tag, json.dumps({k: v for k, v in row.items() if k != "layers"}), flush=True)
        for L_ in layers:
            print("   ", json.dumps(L_), flush=True)
        save()
        if a.no_torch:
            continue
        # the same restatement through torch-ROCm, alternating with ours sample by sample
        img = lambda t: ((torch.where(mask.reshape(h, wd, 1) == 1 if human else mask.reshape(h, wd, 1) >= 1, t.reshape(h, wd, 3),
                                      torch.zeros((), device=dev))[y0:y0 + rh, x0:x0 + rw] - 0.5) * 2).permute(2, 0, 1)[None].contiguous()
        in0, in1 = img(pred), img(gt)
        with torch.no_grad():
            tv = float(torch_lpips(w, in0, in1))                            # first call: MIOpen picks its kernels
            print(tag, "torch value", tv, "ours", value[0], flush=True)
            t_ours, t_torch = [], []
            for _ in range(a.samples):
                t_ours.append(median_ms(ours, 1, 0))
                t_torch.append(median_ms(lambda: torch_lpips(w, in0, in1), 1, 0))
        row["torch_lpips"] = tv
        row["alternating_ours_ms"] = round(statistics.median(t_ours), 4)
        row["torch_ms"] = round(statistics.median(t_torch), 4)
        row["ratio_ours_over_torch"] = round(row["alternating_ours_ms"] / row["torch_ms"], 3)
        print(tag, json.dumps({k: row[k] for k in ("alternating_ours_ms", "torch_ms", "ratio_ours_over_torch")}), flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
