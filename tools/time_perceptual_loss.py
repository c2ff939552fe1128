#!/usr/bin/env python
"""Time the device-side perceptual term of the trainer's loss (enerf_amd.loss.perceptual_loss: enerf_perceptual_fwd + _bwd) on the
GPU against the same restatement through torch-ROCm autograd (bench.py's module shape: F.conv2d / max_pool2d, the gt branch under
no_grad), in the same process and alternating, with random weights (the time does not depend on the values).

    python tools/time_perceptual_loss.py --out profiles/perceptual_loss_timing.json

All figures are device-event medians over --samples alternating batches, warm:
  term            forward + backward of the term alone (loss -> gradient of the rendered image): ours_ms, torch_ms, their ratio, our
                  forward and backward separately, the workspace size.  Shapes: the dtu levels 128x160 and 512x640 (B = 1), the zju
                  patch shape 4 x 64x64
  layers          (512x640 only) every layer ALONE: our forward (enerf_vgg_conv3x3, N = 2) and data gradient (enerf_vgg_conv3x3_dgrad,
                  N = 1, plain: no mask / seed / pool routing) against F.conv2d and F.conv_transpose2d at the same shapes
  train_step      one graphed dtu_pretrain step at 512x640 (GraphedTrainStep replay) with EnerfLoss, and the same step with the torch
                  term in the loss (--no-step skips it)"""
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

POOL_BEFORE = (2, 4, 7)
TAP_AFTER = (1, 3, 6, 9)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def event_ms(fn, calls: int = 1) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / calls


def alternating(fns, samples: int, warmup: int, calls: int = 1):
    """Medians of ``samples`` batches of ``calls`` calls per function, the functions taking turns batch by batch."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(samples):
        for k, fn in enumerate(fns):
            out[k].append(event_ms(fn, calls))
    return [statistics.median(v) for v in out]


class TorchTerm:
    """VGGPerceptualLoss (vgg_perceptual_loss.py:21-37, resize=False) on torch ops, as bench.py's module runs it."""

    def __init__(self, weights, reduce=torch.sum):
        dev = weights.device
        self.convs, self.reduce = weights.convs, reduce
        self.mean, self.std = torch.tensor(MEAN, device=dev).view(1, 3, 1, 1), torch.tensor(STD, device=dev).view(1, 3, 1, 1)

    def features(self, x):
        for i, (w, b) in enumerate(self.convs):
            if i in POOL_BEFORE:
                x = F.max_pool2d(x, 2, 2)
            x = torch.relu(F.conv2d(x, w, b, padding=1))
            if i in TAP_AFTER:
                yield x

    def __call__(self, inp, tar):                                          # (N,3,h,w) each
        with torch.no_grad():
            ys = list(self.features((tar - self.mean) / self.std))
        loss = 0.0
        for x, y in zip(self.features((inp - self.mean) / self.std), ys):
            loss = loss + self.reduce((x - y).abs()) / x.numel()
        return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_perceptual_loss: no GPU; timings are taken on the device only")
    from enerf_amd.lib import PERCEPTUAL_CONVS, get_lib
    from enerf_amd.loss import EnerfLoss, PerceptualWeights, perceptual_loss
    torch.backends.cudnn.allow_tf32 = False
    torch.backends.cuda.matmul.allow_tf32 = False
    lib = get_lib()
    dev = torch.device("cuda:0")
    w = PerceptualWeights.random(0, dev)
    packed = w.packed(lib)
    term = TorchTerm(w)
    g = torch.Generator(device="cpu").manual_seed(0)
    res = {"device": torch.cuda.get_device_name(0), "samples": a.samples,
           "how": "device-event medians of alternating batches, warm; see tools/time_perceptual_loss.py", "term": {}}

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    for tag, N, h, wd in (("dtu_128x160", 1, 128, 160), ("dtu_512x640", 1, 512, 640), ("zju_4x64x64", 4, 64, 64)):
        gt = torch.rand((N, h * wd, 3), generator=g).to(dev)
        pred = (gt + 0.05 * torch.randn((N, h * wd, 3), generator=g).to(dev)).clamp_(0, 1).contiguous().requires_grad_(True)
        img = lambda t: t.reshape(N, h, wd, 3).permute(0, 3, 1, 2)

        def ours():
            pred.grad = None
            perceptual_loss(pred, gt, w, (h, wd), lib=lib).backward()

        def theirs():
            pred.grad = None
            term(img(pred), img(gt)).backward()

        ours()
        g_ours, v_ours = pred.grad.clone(), float(perceptual_loss(pred, gt, w, (h, wd), lib=lib))
        theirs()                                                            # first call: MIOpen picks its kernels
        g_torch, v_torch = pred.grad.clone(), float(term(img(pred), img(gt)))
        t_ours, t_torch = alternating([ours, theirs], a.samples, a.warmup)
        ws = lib.perceptual_workspace(N, h, wd, dev)
        fwd = lambda: lib.perceptual_fwd(packed, pred.detach(), gt, (h, wd), workspace=ws)
        bwd = lambda: lib.perceptual_bwd(packed, N, (h, wd), ws)
        fwd()
        t_fwd, t_bwd = alternating([fwd, bwd], a.samples, a.warmup)
        row = {"N": N, "hw": [h, wd], "ours_ms": round(t_ours, 4), "torch_ms": round(t_torch, 4), "ratio_ours_over_torch": round(t_ours / t_torch, 3),
               "ours_fwd_ms": round(t_fwd, 4), "ours_bwd_ms": round(t_bwd, 4), "workspace_mb": round(ws.numel() * 4 / 2 ** 20, 1),
               "loss_ours": v_ours, "loss_torch": v_torch,
               "grad_maxrel_ours_vs_torch": float((g_ours - g_torch).abs().max() / g_torch.abs().max())}
        res["term"][tag] = row
        print(tag, json.dumps(row), flush=True)
        save()
        del ws
        if tag != "dtu_512x640" or a.no_layers:
            continue
        layers, H, W = [], h, wd
        for i, (cin, cout) in enumerate(PERCEPTUAL_CONVS):
            if i in POOL_BEFORE:
                H, W = H // 2, W // 2
            cw, cb = w.convs[i]
            pk_f, pk_d = lib.vgg_conv3x3_pack(cw, cb), lib.vgg_conv3x3_dgrad_pack(cw)
            x_cl, go_cl = torch.rand((2, H, W, cin), generator=g).to(dev), torch.randn((1, H, W, cout), generator=g).to(dev)
            x, go = x_cl.permute(0, 3, 1, 2).contiguous(), go_cl.permute(0, 3, 1, 2).contiguous()
            fns = [lambda: lib.vgg_conv3x3(pk_f, cin, cout, x_cl), lambda: F.conv2d(x, cw, cb, padding=1),
                   lambda: lib.vgg_conv3x3_dgrad(pk_d, cin, cout, go_cl), lambda: F.conv_transpose2d(go, cw, padding=1)]
            with torch.no_grad():
                t = alternating(fns, a.samples, a.warmup)
            layers.append({"conv": i, "cin": cin, "cout": cout, "hw": [H, W], "fwd_ours_ms": round(t[0], 4), "fwd_torch_ms": round(t[1], 4),
                           "dgrad_ours_ms": round(t[2], 4), "dgrad_torch_ms": round(t[3], 4),
                           "fwd_ratio": round(t[0] / t[1], 3), "dgrad_ratio": round(t[2] / t[3], 3)})
            print("   ", json.dumps(layers[-1]), flush=True)
            del x_cl, go_cl, x, go
        res["layers_512x640"] = layers
        save()

    if not a.no_step:
        import numpy as np
        from __graft_entry__ import _seeded_network
        from enerf_amd.config import EnerfConfig
        from enerf_amd.synth import make_batch
        from enerf_amd.train_graph import GraphedTrainStep, mse_loss, tree_sum
        H, W = 512, 640
        cfg = EnerfConfig()                                                 # dtu_pretrain.yaml: planes 64,8, render_if True,True
        b = make_batch(H, W, 3, cfg, seed=0, textured=True)
        rng = np.random.default_rng(0)
        for i in range(2):
            b[f"rgb_{i}"] = rng.uniform(0, 1, size=(1, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
        batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
        graph_term = TorchTerm(w, tree_sum)

        def torch_loss(out, bt):                                            # bench.py's loss_fn with the term on
            loss = 0.0
            for i, lw in enumerate((0.1, 1.0)):
                loss = loss + lw * mse_loss(bt[f"rgb_{i}"], out[f"rgb_level{i}"])
                hi, wi = int(H * cfg.cas.render_scale[i]), int(W * cfg.cas.render_scale[i])
                im = lambda t: t.reshape(-1, hi, wi, 3).permute(0, 3, 1, 2)
                loss = loss + 0.01 * lw * graph_term(im(out[f"rgb_level{i}"]), im(bt[f"rgb_{i}"]))
            return loss

        steps = {}
        for tag, fn in (("enerf_loss", EnerfLoss((0.1, 1.0), (True, True), (0, 0), (0, 0), (0, 0), w, render_scale=cfg.cas.render_scale, lib=lib)),
                        ("torch_term", torch_loss)):
            net = _seeded_network(cfg, dev).train()
            opt = torch.optim.Adam(net.parameters(), lr=5e-4, capturable=True, fused=True)
            gs = GraphedTrainStep(net, opt, fn, batch, clip_value=40.0, fallback="raise")
            steps[tag] = (gs, float(gs(batch)))
            print("train_step", tag, gs.step_launch, "first loss", steps[tag][1], flush=True)
        t = alternating([lambda: steps["enerf_loss"][0](batch), lambda: steps["torch_term"][0](batch)], a.samples, a.warmup, calls=3)
        res["train_step_512x640"] = {"enerf_loss_ms": round(t[0], 3), "torch_term_ms": round(t[1], 3), "ratio_ours_over_torch": round(t[0] / t[1], 3),
                                     "first_loss": {k: v[1] for k, v in steps.items()},
                                     "launch": {k: v[0].step_launch for k, v in steps.items()}}
        print("train_step", json.dumps(res["train_step_512x640"]), flush=True)
        save()
    print("wrote", a.out)


if __name__ == "__main__":
    main()
