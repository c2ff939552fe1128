#!/usr/bin/env python
"""Time the source-view cache on the GPU against the plain frame, in one process on one device, at the three bench shapes
(dtu 512x640 / 3 views, lego 800x800 / 4 views / both levels, zju 1024x1024 / 4 views / masked), V = 8 cached views each.

    python tools/time_source_cache.py --out profiles/source_cache_timing.json

Per workload:
  forward / forward_cached   one frame of ``Network.forward`` on hand-gathered views (the path without the cache) and of
             ``Network.forward_cached`` on the same views, under the bench's protocol: network(batch), device sync, per frame.
             ``wall_ms`` is the host clock around call + sync, ``device_ms`` two device events around the call; both the median
             over --samples batches of the median over --frames frames, the two paths' batches alternating.
  gather     the gather alone, from the frame's own stage events (begin -> feature_net slot) with everything on one stream
             (``single_stream``: one launch carries every segment), and the bytes it moves (read + written) per second; and the
             share that stays on the caller's stream in the default two-stream frame.  (The masked workload's mask compaction
             is not inside that interval: ``Network`` runs it before the C call and passes ``ray_index_ready``.)
  build      ``Network.cache_sources`` over the V views, device events, per view."""
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
V = 8


class StageEvents:
    """The network's optional stage timer (Network._timer): keeps the last frame's named events."""

    def __init__(self):
        self.last = {}

    def new_events(self, n):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(n)]
        for e in evs:
            e.record()                                 # creates the underlying hipEvent_t; the C call re-records it
        return evs

    def frame(self, named):
        self.last = dict(named)


def workload(name):
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch, make_lego_batch, make_zju_batch
    if name == "dtu":
        cfg = EnerfConfig.dtu_eval()
        return cfg, [make_batch(512, 640, V, cfg, seed=0, textured=True)], 3, False
    if name == "lego":
        cfg = EnerfConfig()
        return cfg, [make_lego_batch(800, 800, 4, cfg, seed=s) for s in (0, 1)], 4, False
    cfg = EnerfConfig().with_cas(volume_planes=(32, 8), render_if=(False, True))
    return cfg, [make_zju_batch(1024, 1024, 4, cfg, seed=s) for s in (0, 1)], 4, True


def frames(fn, n):
    """n frames, each: call, device sync -> (median wall ms, median device ms)."""
    wall, devt = [], []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        devt.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(devt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--samples", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--workloads", default="dtu,lego,zju")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_source_cache: no GPU; timings are taken on the device only")
    import __graft_entry__ as G
    from enerf_amd.lib import Options, cascade_struct
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "views_cached": V, "frames_per_batch": a.frames, "batches": a.samples,
           "protocol": "network(batch) + device sync per frame; median over batches of the per-batch median"}
    for name in a.workloads.split(","):
        cfg, rigs, S, human = workload(name)
        net = G._seeded_network(cfg, dev, human=human)
        cat = lambda k: torch.from_numpy(np.concatenate([r[k][0] for r in rigs])).to(dev).contiguous()
        inps, exts, ixts = cat("src_inps"), cat("src_exts"), cat("src_ixts")
        tar = {k: torch.from_numpy(v).to(dev) for k, v in rigs[0].items() if not k.startswith("src_")}
        rows = [5, 2, 7, 0][:S]
        idx = torch.tensor(rows, dtype=torch.int32, device=dev)
        hand = dict(tar, src_inps=inps[rows][None].contiguous(), src_exts=exts[rows][None].contiguous(),
                    src_ixts=ixts[rows][None].contiguous())
        net.prepare()
        build = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cache = net.cache_sources(inps, exts, ixts)
            e1.record()
            torch.cuda.synchronize()
            build.append(e0.elapsed_time(e1))
        plain = lambda: net(hand)
        cached = lambda: net.forward_cached(cache, idx, tar)
        a_out, b_out = plain(), cached()
        torch.cuda.synchronize()
        same = sorted(a_out) == sorted(b_out) and all(torch.equal(a_out[k], b_out[k]) for k in a_out)
        for _ in range(a.warmup):
            plain(); cached()
            torch.cuda.synchronize()
        rec = {"forward": [], "forward_cached": []}
        for _ in range(a.samples):
            rec["forward"].append(frames(plain, a.frames))
            rec["forward_cached"].append(frames(cached, a.frames))
        row = {"shape": f"{cache.H}x{cache.W}, {S} of {V} views", "bit_identical": bool(same)}
        for k, v in rec.items():
            row[k] = {"wall_ms": round(statistics.median(x[0] for x in v), 4), "device_ms": round(statistics.median(x[1] for x in v), 4)}
        row["cached_over_forward_wall"] = round(row["forward_cached"]["wall_ms"] / row["forward"]["wall_ms"], 4)
        # the gather alone
        _, floats = net.lib.source_cache_sizes(cascade_struct(cfg), V, cache.H, cache.W)
        moved = 2 * 4 * S * (sum(floats) // V)                          # bytes read + written per frame (cameras included)
        timer = StageEvents()
        net._timer = timer
        g = {}
        for tag, opt in (("single_stream_us", Options(single_stream=1)), ("caller_stream_share_us", None)):
            us = []
            for _ in range(a.frames + 10):
                net._forward(tar, opt, cache, idx)
                torch.cuda.synchronize()
                us.append(1e3 * timer.last["begin"].elapsed_time(timer.last["feature_net"]))
            g[tag] = round(statistics.median(us[10:]), 2)
        net._timer = None
        g["bytes_moved"] = int(moved)
        g["gbytes_per_s_single_stream"] = round(moved / (g["single_stream_us"] * 1e-6) / 1e9, 1)
        row["gather"] = g
        row["build"] = {"ms_per_view": round(statistics.median(build[1:]) / V, 4), "ms_total": round(statistics.median(build[1:]), 3),
                        "cache_mbytes": round(cache.nbytes() / 1e6, 1)}
        res[name] = row
        print(name, json.dumps(row), flush=True)
        del cache, net
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
