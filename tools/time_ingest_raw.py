#!/usr/bin/env python
"""Time the raw-camera ingest on the GPU (``enerf_ingest_raw_u8``: undistort, area resize, crop; enerf_amd/raw_ingest.py).

    python tools/time_ingest_raw.py --out profiles/ingest_raw_timing.json

Per case — ZJU raw 1024x1024 -> 512x512 (input_ratio 0.5, masked, dilate 5) at V = 8 and 21; outdoor raw 1024x1366 -> 768x1024
(input_ratio 0.75, 1366 * 0.75 = 1024.5 rounds to 1024, so actor1's crop to input_h_w = (768, 1024) has the offsets (0, 0)), V = 8,
image only:

  kernel alone       device events around --inner back-to-back calls of ``enerf_ingest_raw_u8`` (with its dilation launch), and
                     beside it, as a scale, ``enerf_ingest_views_u8`` at the same OUTPUT size (same mask, same dilate) — the
                     memory-bound conversion a caller with finished images runs.  The two alternate inside every repetition.
  per time frame     a_raw_u8: raw uint8 (+ mask) uploaded from pinned memory, raw ingest, ``SourceCache.rebuild`` of the float image;
                     b_float32: the finished float32 image uploaded from pinned memory, ``SourceCache.rebuild``.  Host clock around a
                     window of --frames time frames with one device synchronise at its end; the two alternate inside every repetition.

Reported: the median over --samples repetitions with (min, max).  There is no earlier device path to compare with and nothing here
is a threshold: what b_float32 leaves out is the host's undistort + resize per view, which is not timed (OpenCV is not a dependency of this project)."""
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
DILATE = 5
DCOEF = (-0.25, 0.12, 0.003, -0.002, -0.03)
CASES = {
    #            Hraw  Wraw  ratio out (H, W)   V   masked
    "zju_v8": (1024, 1024, 0.5, (512, 512), 8, True),
    "zju_v21": (1024, 1024, 0.5, (512, 512), 21, True),
    "outdoor_v8": (1024, 1366, 0.75, (768, 1024), 8, False),
}


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def event_ms(fn, inner):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=4, help="time frames per timed window")
    ap.add_argument("--inner", type=int, default=20, help="back-to-back kernel calls per device-event sample")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-frames", action="store_true", help="kernel timings only (no network, no cache build)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_ingest_raw: no GPU; timings are taken on the device only")
    import __graft_entry__ as G
    from enerf_amd.config import EnerfConfig
    from enerf_amd.lib import get_lib
    from enerf_amd.raw_ingest import RawIngest
    from enerf_amd.synth import make_batch
    dev = torch.device("cuda:0")
    lib = get_lib()
    res = {"device": torch.cuda.get_device_name(0), "dilate": DILATE, "repetitions": a.samples, "kernel_calls_per_sample": a.inner,
           "time_frames_per_window": a.frames,
           "protocol": "kernel: device events around back-to-back calls, / calls; per time frame: host clock around a window with one "
                       "device sync at its end, / time frames; the compared paths alternate inside every repetition; median (min, max)"}
    for name in a.cases.split(","):
        Hraw, Wraw, ratio, (H, W), V, masked = CASES[name]
        Hs, Ws = lib.ingest_raw_geometry(Hraw, Wraw, ratio)
        crop = RawIngest.outdoor_crop(Hs, Ws, H, W) + (H, W)
        K = torch.tensor([[[0.9 * Wraw, 0.0, Wraw / 2 + 3.5 - v], [0.0, 0.92 * Wraw, Hraw / 2 - 2.25 + v], [0.0, 0.0, 1.0]] for v in range(V)])
        D = torch.tensor([[c * (1.0 + 0.02 * v) for c in DCOEF] for v in range(V)])
        rig = RawIngest(K.to(dev), D.to(dev), Hraw, Wraw, ratio, crop, lib=lib)
        g = torch.Generator().manual_seed(1)
        n_frames = 2
        raw = [torch.randint(0, 256, (V, Hraw, Wraw, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(n_frames)]
        masks = None
        if masked:
            masks = []
            for t in range(n_frames):
                m = torch.zeros((V, Hraw, Wraw), dtype=torch.uint8)
                m[:, Hraw // 5 + 16 * t: Hraw - Hraw // 6, Wraw // 4: Wraw - Wraw // 4 - 16 * t] = 255
                masks.append(m.pin_memory())
        dev_raw = raw[0].to(dev)
        dev_mask = masks[0].to(dev) if masked else None
        image = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        small_u8 = torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
        small_mask = dev_mask[:, ::2, ::2].contiguous() if masked else None
        dil = DILATE if masked else 0
        kernels = {"ingest_raw_u8": lambda: rig(dev_raw, dev_mask, dil, out=image),
                   "ingest_views_u8_at_output_size": lambda: lib.ingest_views_u8(small_u8, small_mask, dil, out=image)}
        if masked:
            kernels["ingest_raw_u8_mask_no_dilate"] = lambda: rig(dev_raw, dev_mask, 0, out=image)
            kernels["ingest_raw_u8_no_mask"] = lambda: rig(dev_raw, out=image)
        rec = {k: [] for k in kernels}
        for r in range(a.warmup + a.samples):
            for k, fn in kernels.items():
                ms = event_ms(fn, a.inner)
                if r >= a.warmup:
                    rec[k].append(1e3 * ms)
        px_raw, px = V * Hraw * Wraw, V * H * W
        row = {"shape": f"raw {Hraw}x{Wraw} -> {H}x{W} (input_ratio {ratio}, crop offsets {crop[:2]}), V = {V}"
                        + (f", masked, dilate {DILATE}" if masked else ", image only"),
               "kernel_us": {k: spread(v) for k, v in rec.items()},
               "bytes": {"raw_in": (4 if masked else 3) * px_raw, "float_out": 12 * px}}
        ku = row["kernel_us"]
        row["raw_over_views"] = round(ku["ingest_raw_u8"]["median"] / ku["ingest_views_u8_at_output_size"]["median"], 3)
        if not a.no_frames:
            zju = name.startswith("zju")
            cfg = EnerfConfig().with_cas(volume_planes=(32, 8), render_if=(False, True)) if zju else EnerfConfig.dtu_eval()
            net = G._seeded_network(cfg, dev, human=zju)
            net.prepare()
            b = make_batch(64, 96, 4, cfg, seed=0)
            exts = torch.from_numpy(np.concatenate([b["src_exts"][0]] * ((V + 3) // 4))[:V]).to(dev).contiguous()
            f32 = [rig(raw[t].to(dev), masks[t].to(dev) if masked else None, dil).cpu().pin_memory() for t in range(n_frames)]
            dev_f = torch.empty_like(image)
            ws = lib.source_cache_build_workspace(H, W, dev)
            cache = net.cache_sources(f32[0].to(dev), exts, rig.ixts, raw=rig)
            want = [t.clone() for t in net.cache_sources(f32[1].to(dev), exts, rig.ixts).buffers if t is not None]

            def path_raw(T):
                for t in range(T):
                    dev_raw.copy_(raw[t % n_frames], non_blocking=True)
                    if masked:
                        dev_mask.copy_(masks[t % n_frames], non_blocking=True)
                    cache.rebuild(dev_raw, masks=dev_mask, dilate=dil, image=image, workspace=ws)

            def path_float(T):
                for t in range(T):
                    dev_f.copy_(f32[t % n_frames], non_blocking=True)
                    cache.rebuild(dev_f, workspace=ws)

            same = []
            for p in (path_raw, path_float):                               # both end on time frame 1
                p(n_frames)
                torch.cuda.synchronize()
                same.append(all(torch.equal(x, y) for x, y in zip([t for t in cache.buffers if t is not None], want)))
            paths = {"a_raw_u8": path_raw, "b_float32": path_float}
            rec = {k: [] for k in paths}
            for r in range(a.warmup + a.samples):
                for k, p in paths.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    p(a.frames)
                    torch.cuda.synchronize()
                    if r >= a.warmup:
                        rec[k].append(1e3 * (time.perf_counter() - t0) / a.frames)
            row["ms_per_time_frame"] = {k: spread(v) for k, v in rec.items()}
            row["bit_identical_caches"] = bool(all(same))
            row["upload_mbytes"] = {"a_raw_u8": round((4 if masked else 3) * px_raw / 1e6, 1), "b_float32": round(12 * px / 1e6, 1)}
            mt = row["ms_per_time_frame"]
            row["a_over_b"] = round(mt["a_raw_u8"]["median"] / mt["b_float32"]["median"], 4)
            del net, cache, f32
        res[name] = row
        print(name, json.dumps(row), flush=True)
        del raw, masks, dev_raw, dev_mask, image
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
