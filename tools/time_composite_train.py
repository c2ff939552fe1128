#!/usr/bin/env python
"""Time one eager training step of the composite network (``Network(..., trainable=True)``, enerf_amd/train_path_composite.py) on the
GPU at the shape of tools/time_composite.py: 576x768, 3 views, the last level rendered, one and two foreground layers whose boxes
cover a quarter of the image each.  Beside it, as a SCALE only, the plain ``Network``'s training step at that size (one cascade over
the whole image against 1 + L: no ratio between them means anything).

    python tools/time_composite_train.py --out profiles/composite_train_timing.json

A step is forward, MSE loss on the rendered level, backward, ``clip_grad_value_`` and Adam (trainer.py:56-63 through
``train_graph.train_step``), with a device synchronise after it and the host clock around both.  One process, one device; the three
networks alternate inside every one of --samples repetitions after --warmup untimed rounds; reported: the median over the
repetitions with min and max beside it.  There is no earlier composite step to compare with: the numbers are a record, not a claim."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, S = 576, 768, 3
BOXES = [(96, 64, 384, 288), (288, 224, 384, 288)]         # (x, y, w, h): a quarter of the image each, overlapping


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_train_timing.json"))
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from __graft_entry__ import _seeded_network
    from enerf_amd.config import EnerfConfig
    from enerf_amd.network_composite import Network
    from enerf_amd.synth import make_batch
    from enerf_amd.train_graph import mse_loss, train_step
    dev = torch.device("cuda:0")
    cfg = EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=(False, True))
    base = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(H, W, S, cfg, seed=0, textured=True).items()}
    base["rgb_1"] = torch.rand((1, H * W, 3), generator=torch.Generator().manual_seed(1)).to(dev)
    n, f = (float(v) for v in base["near_far"][0])
    loss_fn = lambda out, batch: mse_loss(batch["rgb_1"], out["rgb_level1"])
    rows = {}
    for L in (1, 2):
        torch.manual_seed(0)
        net = Network(cfg, L, trainable=True).to(dev).train()
        b = dict(base)
        b["bbox"] = [BOXES[:L]]
        b["near_far"] = torch.tensor([[(n + 0.1 * (f - n), n + 0.5 * (f - n)), (n + 0.4 * (f - n), n + 0.8 * (f - n))][:L] + [(n, f)]],
                                     dtype=torch.float32, device=dev)
        b["bg_src_inps"] = base["src_inps"].flip(-1).contiguous()
        rows[f"composite_L{L}"] = (net, torch.optim.Adam(net.parameters(), lr=5e-4), b)
    plain = _seeded_network(cfg, dev).train()
    rows["plain_network"] = (plain, torch.optim.Adam(plain.parameters(), lr=5e-4), base)
    times = {k: [] for k in rows}
    losses = {}
    for rep in range(args.warmup + args.samples):
        for k, (net, opt, batch) in rows.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = train_step(net, opt, loss_fn, batch)
            torch.cuda.synchronize()
            if rep >= args.warmup:
                times[k].append((time.perf_counter() - t0) * 1e3)
            losses.setdefault(k, []).append(float(loss.detach()))
    for k, v in losses.items():
        assert all(x == x for x in v), (k, v)          # (no NaN)
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"H": H, "W": W, "S": S, "render_if": [False, True], "boxes": BOXES},
           "protocol": {"samples": args.samples, "warmup": args.warmup, "step": "forward + MSE + backward + clip_grad_value_ + Adam, "
                        "eager, a device synchronise per step"},
           "step_ms": {k: spread(v) for k, v in times.items()},
           "loss_first_last": {k: [v[0], v[-1]] for k, v in losses.items()},
           "note": "plain_network is a scale only: it trains one cascade over the whole image, the composite networks 1 + L; recorded, "
                   "not compared: there is no earlier composite training step"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["step_ms"]))
    print(json.dumps(out["loss_first_last"]))


if __name__ == "__main__":
    main()
