#!/usr/bin/env python
"""Time the device evaluator's calls on the GPU: enerf_eval_stats alone (what evaluate() cost before SSIM), enerf_eval_ssim alone,
and both on the same buffers, at 512x640 (dtu: msk >= 1, whole image) and 1024x1024 (zju: mask_at_box == 1, bounding box).

    python tools/time_eval_ssim.py --out profiles/eval_ssim_timing.json [--extra context.json]

Two figures per configuration, both from device events, warm, median over --samples samples of --calls back-to-back calls:
  device_us  the calls queued behind a short busy-wait kernel, so that the host has enqueued all of them before the first one
             starts: the GPU time of one call (its 2-4 launches back to back);
  eager_us   no busy-wait: what a Python loop that calls the wrapper gets, host enqueue cost included.
--extra merges a JSON object (the bench line's frame time, a skimage timing taken elsewhere) into the output under "context"."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(fn, calls: int, samples: int, warmup: int, blocker_cycles: int) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per_call = []
    for _ in range(samples):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if blocker_cycles:
            torch.cuda._sleep(blocker_cycles)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        per_call.append(1e3 * e0.elapsed_time(e1) / calls)
    return statistics.median(per_call)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--extra", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_eval_ssim: no GPU; timings are taken on the device only")
    from enerf_amd.lib import get_lib
    lib = get_lib()
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "calls_per_sample": a.calls, "samples": a.samples, "unit": "us per call (median)"}
    for tag, (h, w), human in (("dtu_512x640", (512, 640), False), ("zju_1024x1024", (1024, 1024), True)):
        gt = torch.rand((1, h * w, 3), generator=g).to(dev)
        pred = (gt + 0.05 * torch.randn((1, h * w, 3), generator=g).to(dev)).clamp_(0, 1).contiguous()
        if human:
            m = torch.zeros((h, w), dtype=torch.uint8)
            m[150:901, 200:803] = 1
            mask = m.reshape(1, h * w).to(dev)
            kw = dict(bbox=True, mask_is_one=True)
        else:
            mask = (torch.rand((1, h * w), generator=g) > 0.3).to(torch.uint8).to(dev)
            kw = {}
        stats = lambda: lib.eval_stats(pred[0], gt[0], mask[0], image_hw=(h, w), sync=False)
        ssim = lambda: lib.eval_ssim(pred, gt, mask, image_hw=(h, w), sync=False, **kw)
        both = lambda: (stats(), ssim())
        value = lib.eval_ssim(pred, gt, mask, image_hw=(h, w), **kw)[0]
        row = {"ssim_value": value, "launches_ssim": 4 if human else 2}
        # busy-wait long enough for the host to enqueue one sample's calls (about 50 us each) before the first one runs
        blocker = int(a.calls * 2 * 100e-6 * 2.4e9)
        for name, fn in (("eval_stats", stats), ("eval_ssim", ssim), ("eval_stats+eval_ssim", both)):
            row[name] = {"device_us": round(measure(fn, a.calls, a.samples, a.warmup, blocker), 2),
                         "eager_us": round(measure(fn, a.calls, a.samples, a.warmup, 0), 2)}
        res[tag] = row
        print(tag, json.dumps(row))
    if a.extra:
        with open(a.extra) as f:
            res["context"] = json.load(f)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
