#!/usr/bin/env python
"""Time a dynamic scene on the GPU: milliseconds per TIME FRAME (upload of the V camera images, source-cache build, K = 4 target
cameras rendered from it), in one process on one device, three ways on the same uint8 frames:

  a_float_serial    what a caller does without the uint8 entries: the float32 (V,3,H,W) image (converted on the host beforehand,
                    not timed) uploaded from pinned memory, ``Network.cache_sources``, K x ``forward_cached``; one stream.
  b_uint8_serial    uint8 (V,H,W,3) + mask uploaded from pinned memory, ``SourceCache.rebuild`` (ingest + build, in place),
                    K x ``forward_cached``; one stream.
  c_player          ``SequencePlayer``: submit t+1 (host memcpy into the player's pinned staging, upload, ingest, rebuild on the
                    build stream), K x render of t on the caller's stream, flip.

    python tools/time_sequence.py --out profiles/sequence_timing.json

Protocol: a window is --frames time frames enqueued back to back with ONE device synchronise at its end, host clock around it,
divided by the number of time frames; the three paths alternate inside every one of --samples repetitions after --warmup untimed
windows; reported: the median over the repetitions, with min and max beside it.  Also: the ingest kernel alone (device events
around 20 back-to-back calls; its bytes are 4 read + 12 written per pixel), the host-to-device copy of both formats from pinned
memory, and the host memcpy into the player's staging buffer.  The outputs of the three paths are compared bit for bit."""
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
K = 4
DILATE = 5


def workload(name):
    """(cfg, one synthetic rig of 4 views with its target batch, S, human, V)."""
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch, make_zju_batch
    if name == "dtu":
        cfg = EnerfConfig.dtu_eval()
        return cfg, make_batch(512, 640, 4, cfg, seed=0, textured=True), 3, False, 8
    cfg = EnerfConfig().with_cas(volume_planes=(32, 8), render_if=(False, True))
    return cfg, make_zju_batch(1024, 1024, 4, cfg, seed=0), 4, True, 21 if name == "zju21" else 8


def restate(u8, mask, dilate):
    import torch.nn.functional as F
    x = u8.float() / 255
    keep = F.max_pool2d((mask != 0).float()[:, None], dilate, 1, dilate // 2)
    x[keep[:, 0] == 0] = 0
    return (x * 2 - 1).permute(0, 3, 1, 2).contiguous()


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def device_ms(fn, reps, inner=1):
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(inner):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / inner)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=8, help="time frames per timed window")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="dtu,zju,zju21")
    ap.add_argument("--single-stream", action="store_true", help="frames with enerf_options_t.single_stream (no side lanes), all paths")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_sequence: no GPU; timings are taken on the device only")
    import __graft_entry__ as G
    from enerf_amd.sequence import SequencePlayer
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "cameras_per_time_frame": K, "time_frames_per_window": a.frames,
           "repetitions": a.samples, "dilate": DILATE, "single_stream_frames": bool(a.single_stream),
           "protocol": "host clock around a window of time frames with one device sync at its end, / time frames; paths alternate "
                       "inside every repetition; median (min, max) over the repetitions"}
    for name in a.workloads.split(","):
        cfg, rig, S, human, V = workload(name)
        H, W = rig["src_inps"].shape[-2:]
        net = G._seeded_network(cfg, dev, human=human)
        net.static_shapes = human
        if a.single_stream:
            from enerf_amd.lib import Options
            net.options = Options(single_stream=1)
        net.prepare()
        rep = lambda k: torch.from_numpy(np.concatenate([rig[k][0]] * ((V + 3) // 4))[:V]).to(dev).contiguous()
        exts, ixts = rep("src_exts"), rep("src_ixts")
        tar = {k: torch.from_numpy(v).to(dev) for k, v in rig.items() if not k.startswith("src_")}
        idx = [torch.tensor([(c + s * 2) % V for s in range(S)], dtype=torch.int32, device=dev) for c in range(K)]
        g = torch.Generator().manual_seed(1)
        n_frames = 2                                                   # distinct time frames, played round and round
        u8 = [torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(n_frames)]
        masks = []
        for t in range(n_frames):
            m = torch.zeros((V, H, W), dtype=torch.uint8)
            m[:, H // 5 + 8 * t: H - H // 6, W // 4: W - W // 4 - 8 * t] = 255
            masks.append(m.pin_memory())
        f32 = [restate(u8[t], masks[t], DILATE).pin_memory() for t in range(n_frames)]
        dev_f = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        dev_u8 = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
        dev_m = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
        image = torch.empty_like(dev_f)
        ws = net.lib.source_cache_build_workspace(H, W, dev)
        cache_b = net.cache_sources(f32[0].to(dev), exts, ixts)
        player = SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE)

        def path_a(T, t0=0):
            out = None
            for t in range(t0, t0 + T):
                dev_f.copy_(f32[t % n_frames], non_blocking=True)
                cache = net.cache_sources(dev_f, exts, ixts)
                for k in range(K):
                    out = net.forward_cached(cache, idx[k], tar)
            return out

        def path_b(T, t0=0):
            out = None
            for t in range(t0, t0 + T):
                dev_u8.copy_(u8[t % n_frames], non_blocking=True)
                dev_m.copy_(masks[t % n_frames], non_blocking=True)
                cache_b.rebuild(dev_u8, masks=dev_m, dilate=DILATE, image=image, workspace=ws)
                for k in range(K):
                    out = net.forward_cached(cache_b, idx[k], tar)
            return out

        def path_c(T, t0=0):
            """Primed: time frame t0 is the front.  Submits t0+1 .. t0+T, renders t0 .. t0+T-1."""
            out = None
            for t in range(t0, t0 + T):
                player.submit(u8[(t + 1) % n_frames], masks[(t + 1) % n_frames])
                for k in range(K):
                    out = player.render(idx[k], tar)
                player.flip()
            return out

        player.submit(u8[0], masks[0])
        player.flip()
        torch.cuda.synchronize()
        # the same last time frame (index T-1) and camera on all three paths
        outs = [{k: v.clone() for k, v in p(n_frames).items()} for p in (path_a, path_b, path_c)]
        torch.cuda.synchronize()
        keys = [k for k in outs[0] if k.startswith(("rgb", "depth_mvs", "std"))]     # (static_shapes leaves rows past the ray count unwritten)
        same = all(sorted(o) == sorted(outs[0]) and all(torch.equal(o[k], outs[0][k]) for k in keys) for o in outs[1:])
        player.submit(u8[0], masks[0])                                 # front = time frame 0 again for every later window
        player.flip()
        paths = {"a_float_serial": path_a, "b_uint8_serial": path_b, "c_player": path_c}
        assert a.frames % n_frames == 0
        rec = {k: [] for k in paths}
        for r in range(a.warmup + a.samples):
            for k, p in paths.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                p(a.frames)
                torch.cuda.synchronize()
                if r >= a.warmup:
                    rec[k].append(1e3 * (time.perf_counter() - t0) / a.frames)
        row = {"shape": f"{H}x{W}, V = {V}, {S} views per camera, {K} cameras per time frame" + (", masked (human)" if human else ""),
               "bit_identical": bool(same), "ms_per_time_frame": {k: spread(v) for k, v in rec.items()}}
        mt = row["ms_per_time_frame"]
        row["b_over_a"] = round(mt["b_uint8_serial"]["median"] / mt["a_float_serial"]["median"], 4)
        row["c_over_b"] = round(mt["c_player"]["median"] / mt["b_uint8_serial"]["median"], 4)
        # the pieces
        px = V * H * W
        ing = device_ms(lambda: net.lib.ingest_views_u8(dev_u8, dev_m, DILATE, out=image), 7, inner=20)
        ing0 = device_ms(lambda: net.lib.ingest_views_u8(dev_u8, None, 0, out=image), 7, inner=20)
        row["ingest_kernel"] = {"bytes": 16 * px, "dilate5_us": spread([1e3 * x for x in ing]), "no_mask_us": spread([1e3 * x for x in ing0])}
        row["ingest_kernel"]["dilate5_gbytes_per_s"] = round(16 * px / (statistics.median(ing) * 1e-3) / 1e9, 1)
        row["ingest_kernel"]["no_mask_gbytes_per_s"] = round(15 * px / (statistics.median(ing0) * 1e-3) / 1e9, 1)
        h2d_f = device_ms(lambda: dev_f.copy_(f32[0], non_blocking=True), 9)
        h2d_u = device_ms(lambda: (dev_u8.copy_(u8[0], non_blocking=True), dev_m.copy_(masks[0], non_blocking=True)), 9)
        row["h2d_ms"] = {"float32": spread(h2d_f), "uint8_and_mask": spread(h2d_u), "float32_mbytes": round(12 * px / 1e6, 1),
                         "uint8_and_mask_mbytes": round(4 * px / 1e6, 1)}
        stage = []
        for _ in range(7):
            t0 = time.perf_counter()
            player.slots[0].pin_img.copy_(u8[0])
            player.slots[0].pin_mask.copy_(masks[0])
            stage.append(1e3 * (time.perf_counter() - t0))
        row["player_host_staging_memcpy_ms"] = spread(stage)
        build = device_ms(lambda: cache_b.rebuild(dev_u8, masks=dev_m, dilate=DILATE, image=image, workspace=ws), 7)
        row["rebuild_uint8_ms"] = spread(build)
        row["player_device_mbytes"] = round(player.nbytes() / 1e6, 1)
        row["player_pinned_mbytes"] = round(player.pinned_nbytes() / 1e6, 1)
        res[name] = row
        print(name, json.dumps(row), flush=True)
        del player, cache_b, net, u8, masks, f32
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
