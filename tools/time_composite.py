#!/usr/bin/env python
"""Time the composite network (enerf_amd/network_composite.py) on the GPU at 576x768 (enerf_outdoor/actor1.yaml's 768x1024 at
input_ratio 0.75), 3 views, render_if False,True, with one and with two foreground layers whose boxes cover a quarter of the image
each; beside it, as a SCALE only, the plain ``Network.forward`` at the same size and cascade values (the two compute different
things: no ratio between them means anything).

    python tools/time_composite.py --out profiles/composite_timing.json

Protocol: one process, one device; the three networks alternate inside every one of --samples repetitions after --warmup untimed
rounds; a repetition of a network is --frames frames enqueued back to back with ONE device synchronise at the end, host clock
around it, divided by the number of frames; reported: the median over the repetitions with min and max beside it.  Per stage:
device events between the stages of single frames (median over the repetitions; the staged path — a stage hook selects it); their
sum is below the frame time by what the host spends between the ctypes calls, which that path does not hide.

Drivers ("driver_ms"): for L = 1 and L = 2 three rows over the same weights and batch — ``staged`` (Network(driver="staged"): one C
call per stage, the path before enerf_forward_composite existed, the baseline), ``call_single_stream`` (one
enerf_forward_composite per frame, options.single_stream) and ``call_forked`` (the same with the foreground layers on the side
lane) — under two protocols: ``back_to_back`` as above, and ``sync_per_frame`` (the reference's run.py protocol: a device
synchronise after every frame, so the host time of a frame's calls lands on the frame).  The rows alternate inside every
repetition."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, S = 576, 768, 3
BOXES = [(96, 64, 384, 288), (288, 224, 384, 288)]         # (x, y, w, h): a quarter of the image each, overlapping


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_timing.json"))
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from __graft_entry__ import _seeded_network
    from enerf_amd.config import EnerfConfig
    from enerf_amd.network_composite import Network
    from enerf_amd.synth import make_batch
    dev = torch.device("cuda:0")
    cfg = EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=(False, True))
    base = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(H, W, S, cfg, seed=0, textured=True).items()}
    n, f = (float(v) for v in base["near_far"][0])
    nets, batches = {}, {}
    for L in (1, 2):
        torch.manual_seed(0)
        nets[f"composite_L{L}"] = Network(cfg, L).to(dev).eval().prepare()
        b = dict(base)
        b["bbox"] = [BOXES[:L]]                                                     # host-side boxes: no synchronisation in the frame
        b["near_far"] = torch.tensor([[(n + 0.1 * (f - n), n + 0.5 * (f - n)), (n + 0.4 * (f - n), n + 0.8 * (f - n))][:L] + [(n, f)]],
                                     dtype=torch.float32, device=dev)
        b["bg_src_inps"] = base["src_inps"].flip(-1).contiguous()
        batches[f"composite_L{L}"] = b
    from enerf_amd.lib import Options
    drivers = {}                                     # (L, row) -> (network, options): same weights as composite_L{L}
    for L in (1, 2):
        staged = Network(cfg, L, driver="staged")
        staged.load_state_dict(nets[f"composite_L{L}"].state_dict())
        staged = staged.to(dev).eval().prepare()
        call = Network(cfg, L)
        call.load_state_dict(nets[f"composite_L{L}"].state_dict())
        call = call.to(dev).eval().prepare()
        drivers[L, "staged"] = (staged, None)
        drivers[L, "call_single_stream"] = (call, Options(single_stream=1))
        drivers[L, "call_forked"] = (call, None)
    driver_times = {proto: {k: [] for k in drivers} for proto in ("back_to_back", "sync_per_frame")}
    nets["plain_network"] = _seeded_network(cfg, dev)
    batches["plain_network"] = base
    times = {k: [] for k in nets}
    stages = {k: {} for k in nets if k != "plain_network"}
    with torch.no_grad():
        for rep in range(args.warmup + args.samples):
            for k, net in nets.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    net(batches[k])
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    times[k].append((time.perf_counter() - t0) * 1e3 / args.frames)
                if k in stages:
                    marks = []

                    def mark(name):
                        ev = torch.cuda.Event(enable_timing=True)
                        ev.record()
                        marks.append((name, ev))
                    net.stage_hook = mark
                    net(batches[k])
                    torch.cuda.synchronize()
                    net.stage_hook = None
                    if rep >= args.warmup:
                        for (_, a), (name, b) in zip(marks, marks[1:]):
                            stages[k].setdefault(name, []).append(a.elapsed_time(b))
            for proto in driver_times:               # the driver rows, alternating inside the repetition
                for (L, row), (net, options) in drivers.items():
                    net.options = options
                    b = batches[f"composite_L{L}"]
                    net(b)                           # (the two call rows share their buffers: settle the switch outside the clock)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        net(b)
                        if proto == "sync_per_frame":
                            torch.cuda.synchronize()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        driver_times[proto][L, row].append((time.perf_counter() - t0) * 1e3 / args.frames)
    out = {"device": torch.cuda.get_device_name(dev), "shape": {"H": H, "W": W, "S": S, "render_if": [False, True], "boxes": BOXES},
           "protocol": {"frames_per_window": args.frames, "samples": args.samples, "warmup": args.warmup},
           "frame_ms": {k: spread(v) for k, v in times.items()},
           "stage_ms": {k: {name: spread(v) for name, v in st.items()} for k, st in stages.items()},
           "driver_ms": {proto: {f"L{L}": {row: spread(rows[L, row]) for row in ("staged", "call_single_stream", "call_forked")} for L in (1, 2)}
                         for proto, rows in driver_times.items()},
           "note": "plain_network is a scale only: it renders one cascade over the whole image, the composite networks 1 + L; "
                   "composite_L* frame_ms is the default driver (one enerf_forward_composite per frame), stage_ms the staged path"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["frame_ms"]))
    print(json.dumps(out["stage_ms"]))
    print(json.dumps(out["driver_ms"]))


if __name__ == "__main__":
    main()
