#!/usr/bin/env python
"""Time the composite network's cached frame (Network.forward_cached, enerf_forward_composite_cached) against ``forward`` on the same
views gathered by hand, on the GPU, at tools/time_composite.py's size: 576x768, 3 of 8 cached views, last level rendered, boxes of a
quarter of the image each, L = 1 and 2 foreground layers.

    timeout -k 10 600 python tools/time_composite_cached.py --out profiles/composite_cached_timing.json

(run it under a time limit of its own, and chain it to other GPU steps with ``&&``: nothing else should start on the card after
a step that failed).

Protocol: one process, one device.  Per L the two rows — ``forward`` (both FeatureNets per frame: the frame as it was) and
``forward_cached`` (two gathers instead) — alternate inside every one of --samples repetitions after --warmup untimed rounds, over
the same weights, views, boxes and target camera (their outputs are compared bit for bit once, before the clock starts).  A
repetition of a row is --frames frames, host clock around them, divided by the number of frames, under two protocols:
``back_to_back`` (ONE device synchronise at the end) and ``sync_per_frame`` (one after every frame, the reference's run.py protocol:
the host time of a frame's calls lands on the frame).  Reported: the median over the repetitions with min and max beside it.  Also
the cost of ``cache_sources`` — once per time frame, not per camera — as milliseconds per cached view, and the cache's size."""
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
H, W, S, V = 576, 768, 3, 8
BOXES = [(96, 64, 384, 288), (288, 224, 384, 288)]         # (x, y, w, h): a quarter of the image each, overlapping
VIEWS = [5, 1, 6]                                          # the index row of every timed frame


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_cached_timing.json"))
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    from enerf_amd.config import EnerfConfig
    from enerf_amd.network_composite import Network
    from enerf_amd.synth import make_batch
    dev = torch.device("cuda:0")
    cfg = EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=(False, True))
    base = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(H, W, V, cfg, seed=0, textured=True).items()}
    inps, exts, ixts = (base[k][0].contiguous() for k in ("src_inps", "src_exts", "src_ixts"))
    bg_inps = inps.flip(-1).contiguous()
    n, f = (float(v) for v in base["near_far"][0])
    rows = {}                                                # (L, row) -> callable running one frame
    caches, build_ms = {}, {}
    idx = torch.tensor(VIEWS, dtype=torch.int32, device=dev)
    pick = torch.tensor(VIEWS, dtype=torch.long, device=dev)
    with torch.no_grad():
        for L in (1, 2):
            torch.manual_seed(0)
            net = Network(cfg, L).to(dev).eval().prepare()
            tar = {k: v for k, v in base.items() if not k.startswith("src_")}
            tar["bbox"] = [BOXES[:L]]                        # host-side boxes: no synchronisation in the frame
            tar["near_far"] = torch.tensor([[(n + 0.1 * (f - n), n + 0.5 * (f - n)), (n + 0.4 * (f - n), n + 0.8 * (f - n))][:L] + [(n, f)]],
                                           dtype=torch.float32, device=dev)
            hand = dict(tar, src_inps=inps[pick][None].contiguous(), bg_src_inps=bg_inps[pick][None].contiguous(),
                        src_exts=exts[pick][None].contiguous(), src_ixts=ixts[pick][None].contiguous())
            cache = net.cache_sources(inps, bg_inps, exts, ixts)
            ref = {k: v.clone() for k, v in net(hand).items()}
            got = net.forward_cached(cache, idx, tar)
            torch.cuda.synchronize()
            for k in ref:
                assert torch.equal(got[k], ref[k]), (L, k)
            caches[L] = cache
            build_ms[L] = []
            rows[L, "forward"] = (lambda net=net, hand=hand: net(hand))
            rows[L, "forward_cached"] = (lambda net=net, cache=cache, tar=tar: net.forward_cached(cache, idx, tar))
        times = {proto: {k: [] for k in rows} for proto in ("back_to_back", "sync_per_frame")}
        for rep in range(args.warmup + args.samples):
            for proto in times:
                for key, run in rows.items():                # the rows alternate inside the repetition
                    run()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.frames):
                        run()
                        if proto == "sync_per_frame":
                            torch.cuda.synchronize()
                    torch.cuda.synchronize()
                    if rep >= args.warmup:
                        times[proto][key].append((time.perf_counter() - t0) * 1e3 / args.frames)
            for L, cache in caches.items():                  # the build, once per time frame: in place, as a viewer would
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                cache.rebuild(inps)
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    build_ms[L].append((time.perf_counter() - t0) * 1e3 / V)
    out = {"device": torch.cuda.get_device_name(dev),
           "shape": {"H": H, "W": W, "S": S, "V": V, "views": VIEWS, "render_if": [False, True], "boxes": BOXES},
           "protocol": {"frames_per_window": args.frames, "samples": args.samples, "warmup": args.warmup},
           "frame_ms": {proto: {f"L{L}": {row: spread(t[L, row]) for row in ("forward", "forward_cached")} for L in (1, 2)}
                        for proto, t in times.items()},
           "cache_sources_ms_per_view": {f"L{L}": spread(v) for L, v in build_ms.items()},
           "cache_nbytes": {f"L{L}": c.nbytes() for L, c in caches.items()},
           "note": "forward = enerf_forward_composite on the three views gathered by hand (both FeatureNets per frame); forward_cached = "
                   "enerf_forward_composite_cached on a cache of 8 views; outputs compared bit for bit before timing; "
                   "cache_sources_ms_per_view is CompositeSourceCache.rebuild of all 8 views (both nets), divided by 8"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["frame_ms"]))
    print(json.dumps(out["cache_sources_ms_per_view"]), json.dumps(out["cache_nbytes"]))


if __name__ == "__main__":
    main()
