#!/usr/bin/env python
"""Time the visual-hull bounds on the GPU (``enerf_vhull_bounds``: the foreground's world-space box carved from the masks).

    python tools/time_vhull.py --out profiles/vhull_timing.json

Per case, all at a 128^3 grid — V = 8 with 512x512 masks, V = 21 with 1024x1024 masks, V = 8 with 512x512 masks and two labelled
layers; the masks are analytic ellipsoids seen by a ring of cameras:

  kernel alone       device events around --inner back-to-back calls of ``enerf_vhull_bounds`` (its three launches: the fill of the
                     accumulators, the carving, the finish); beside it the same model as a vectorised float64 restatement in torch on the
                     same device, and, as a scale, ``enerf_ingest_views_u8`` of V images of the masks' size.  The three alternate inside
                     every repetition.
  per time frame     ``SequencePlayer`` with and without ``hull=`` (512x640, V = 8, four cameras rendered per time frame), the protocol
                     of tools/time_sequence.py: host clock around a window of --frames time frames with one device synchronise at its
                     end; the two players alternate inside every repetition.

Reported: the median over --samples repetitions with (min, max).  Nothing here is a threshold."""
from __future__ import annotations

import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID = (128, 128, 128)
SCENE = ((-1.2, -1.1, -1.0), (1.3, 1.0, 1.1))
CASES = {
    #             V   H     W     layers
    "v8_512": (8, 512, 512, 1),
    "v21_1024": (21, 1024, 1024, 1),
    "v8_512_two_layers": (8, 512, 512, 2),
}
OBJECTS = (((0.45, 0.05, 0.0), (0.32, 0.36, 0.55)), ((-0.35, -0.1, 0.05), (0.36, 0.30, 0.50)))


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


def ring(V, H, W):
    """V cameras on a tilted ring of radius 3.4 looking at the origin: exts (V,4,4), ixts (V,3,3) float64."""
    exts, ixts = [], []
    for v in range(V):
        a = 0.137 + 2 * math.pi * v / V
        pos = np.array([3.4 * math.cos(a), 3.4 * math.sin(a), 0.9 + 0.35 * math.sin(3 * a)])
        f = -pos / np.linalg.norm(pos)
        r = np.cross(f, [0.0, 0.0, 1.0])
        r /= np.linalg.norm(r)
        E = np.eye(4)
        E[:3, :3] = np.stack([r, np.cross(f, r), f])
        E[:3, 3] = -E[:3, :3] @ pos
        exts.append(E)
        ixts.append(np.array([[1.1 * W, 0.0, W / 2 + 0.237 - 0.11 * v], [0.0, 1.1 * W, H / 2 - 0.311 + 0.07 * v], [0.0, 0.0, 1.0]]))
    return np.stack(exts), np.stack(ixts)


def raster(exts, ixts, H, W, objects, dev):
    """(V,H,W) uint8 on the device: the 1-based label of the nearest ellipsoid the ray through each pixel centre hits."""
    V = exts.shape[0]
    out = torch.zeros((V, H, W), dtype=torch.uint8, device=dev)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    for v in range(V):
        E, K = torch.from_numpy(exts[v]).to(dev), torch.from_numpy(ixts[v]).to(dev)
        R, t = E[:3, :3], E[:3, 3]
        o = -R.T @ t
        d = torch.stack([(xx - K[0, 2]) / K[0, 0], (yy - K[1, 2]) / K[1, 1], torch.ones_like(xx)], -1) @ R
        best = torch.full((H, W), float("inf"), dtype=torch.float64, device=dev)
        for label, (c, r) in enumerate(objects, 1):
            c, r = torch.tensor(c, dtype=torch.float64, device=dev), torch.tensor(r, dtype=torch.float64, device=dev)
            oc, ds = (o - c) / r, d / r
            A, B, C = (ds * ds).sum(-1), 2 * (ds * oc).sum(-1), (oc * oc).sum() - 1.0
            disc = B * B - 4 * A * C
            s = torch.where(disc >= 0, (-B - disc.clamp_min(0).sqrt()) / (2 * A), torch.full_like(A, float("inf")))
            hit = (disc >= 0) & (s > 0) & (s < best)
            out[v][hit] = label
            best = torch.where(hit, s, best)
    return out


def torch_model(masks, exts, ixts, scene, grid, L, labels, min_views, max_miss):
    """The model of include/enerf_hip.h, vectorised in float64 on the masks' device: (bounds (L,2,3) float32, counts (L))."""
    dev = masks.device
    V, H, W = masks.shape
    lo, hi = (torch.tensor(s, dtype=torch.float32, device=dev).double() for s in scene)
    ax = [lo[a] + (torch.arange(grid[a], dtype=torch.float64, device=dev) + 0.5) * (hi[a] - lo[a]) / grid[a] for a in range(3)]
    z, y, x = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    P = torch.stack([x, y, z], -1)
    inside = torch.zeros((L,) + tuple(P.shape[:3]), dtype=torch.int32, device=dev)
    votes = torch.zeros(tuple(P.shape[:3]), dtype=torch.int32, device=dev)
    for v in range(V):
        E, K = exts[v].double(), ixts[v].double().reshape(9)
        c = P @ E[:3, :3].T + E[:3, 3]
        cz = c[..., 2]
        fu, fv = torch.floor(K[0] * c[..., 0] / cz + K[2] + 0.5), torch.floor(K[4] * c[..., 1] / cz + K[5] + 0.5)
        seen = (cz > 0) & (fu >= 0) & (fu < W) & (fv >= 0) & (fv < H)
        iu, iv = torch.where(seen, fu, torch.zeros_like(fu)).long(), torch.where(seen, fv, torch.zeros_like(fv)).long()
        m = masks[v][iv, iu]
        votes += seen
        for l in range(L):
            inside[l] += seen & ((m == l + 1) if labels else (m != 0))
    occ = (inside >= min_views) & ((votes[None] - inside) <= max_miss)
    bounds = torch.zeros((L, 2, 3), dtype=torch.float32, device=dev)
    for l in range(L):
        for a in range(3):
            idx = torch.nonzero(occ[l].any(dim=tuple(d for d in range(3) if d != 2 - a)))
            cell = (hi[a] - lo[a]) / grid[a]
            bounds[l, 0, a] = (lo[a] + idx[0, 0] * cell).float()
            bounds[l, 1, a] = (lo[a] + (idx[-1, 0] + 1) * cell).float()
    return bounds, occ.sum(dim=(1, 2, 3)).int()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--frames", type=int, default=8, help="time frames per timed window")
    ap.add_argument("--inner", type=int, default=10, help="back-to-back kernel calls per device-event sample")
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--no-frames", action="store_true", help="kernel timings only (no network, no player)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_vhull: no GPU; timings are taken on the device only")
    from enerf_amd.lib import get_lib
    dev = torch.device("cuda:0")
    lib = get_lib()
    res = {"device": torch.cuda.get_device_name(0), "grid": list(GRID), "repetitions": a.samples, "kernel_calls_per_sample": a.inner,
           "time_frames_per_window": a.frames,
           "protocol": "kernel: device events around back-to-back calls, / calls; per time frame: host clock around a window with one "
                       "device sync at its end, / time frames; the compared paths alternate inside every repetition; median (min, max)"}
    for name in a.cases.split(","):
        V, H, W, L = CASES[name]
        e64, k64 = ring(V, H, W)
        masks = raster(e64, k64, H, W, OBJECTS[:L], dev)
        exts, ixts = torch.from_numpy(e64).float().to(dev), torch.from_numpy(k64).float().to(dev)
        kw = dict(n_layers=L, labels=L > 1, min_views=V if L == 1 else V - 2, max_miss=0 if L == 1 else 2)   # (a layer is hidden from some views)
        out = lib.vhull_bounds(masks, exts, ixts, SCENE, grid=GRID, **kw)
        ws = lib.vhull_workspace(L, dev)
        img = torch.randint(0, 256, (V, H, W, 3), dtype=torch.uint8, device=dev)
        image = torch.empty((V, 3, H, W), dtype=torch.float32, device=dev)
        want = torch_model(masks, exts, ixts, SCENE, GRID, L, L > 1, kw["min_views"], kw["max_miss"])
        torch.cuda.synchronize()
        kernels = {"vhull_bounds": (lambda: lib.vhull_bounds(masks, exts, ixts, SCENE, grid=GRID, out=out, workspace=ws, **kw), a.inner),
                   "torch_float64_restatement": (lambda: torch_model(masks, exts, ixts, SCENE, GRID, L, L > 1, kw["min_views"],
                                                                     kw["max_miss"]), 1),
                   "ingest_views_u8_same_size": (lambda: lib.ingest_views_u8(img, masks, 0, out=image), a.inner)}
        rec = {k: [] for k in kernels}
        for r in range(a.warmup + a.samples):
            for k, (fn, inner) in kernels.items():
                ms = event_ms(fn, inner)
                if r >= a.warmup:
                    rec[k].append(1e3 * ms)
        row = {"shape": f"V = {V}, masks {H}x{W}, {L} layer{'s, labelled' if L > 1 else ''}, min_views {kw['min_views']}, max_miss {kw['max_miss']}",
               "kernel_us": {k: spread(v) for k, v in rec.items()},
               "occupied_voxels": out[1].tolist(), "flags": out[2].tolist(),
               "counts_equal_restatement": bool(torch.equal(out[1], want[1])), "bounds_equal_restatement": bool(torch.equal(out[0], want[0])),
               "mask_bytes": V * H * W, "voxel_views": GRID[0] * GRID[1] * GRID[2] * V}
        ku = row["kernel_us"]
        row["us_per_million_voxel_views"] = round(ku["vhull_bounds"]["median"] / (row["voxel_views"] / 1e6), 4)
        row["restatement_over_kernel"] = round(ku["torch_float64_restatement"]["median"] / ku["vhull_bounds"]["median"], 1)
        res[name] = row
        print(name, json.dumps(row), flush=True)
        del masks, img, image
        torch.cuda.empty_cache()
    if not a.no_frames:
        import __graft_entry__ as G
        from enerf_amd.config import EnerfConfig
        from enerf_amd.sequence import HullSpec, SequencePlayer
        from enerf_amd.synth import make_batch
        cfg = EnerfConfig.dtu_eval()
        rig = make_batch(512, 640, 4, cfg, seed=0, textured=True)
        V, S, K, DILATE = 8, 3, 4, 5
        H, W = rig["src_inps"].shape[-2:]
        net = G._seeded_network(cfg, dev)
        net.prepare()
        rep = lambda k: torch.from_numpy(np.concatenate([rig[k][0]] * ((V + 3) // 4))[:V]).to(dev).contiguous()      # noqa: E731
        exts, ixts = rep("src_exts"), rep("src_ixts")
        tar = {k: torch.from_numpy(v).to(dev) for k, v in rig.items() if not k.startswith("src_")}
        idx = [torch.tensor([(c + s * 2) % V for s in range(S)], dtype=torch.int32, device=dev) for c in range(K)]
        g = torch.Generator().manual_seed(1)
        u8 = [torch.randint(0, 256, (V, H, W, 3), generator=g, dtype=torch.uint8).pin_memory() for _ in range(2)]
        masks = []
        for t in range(2):
            m = torch.zeros((V, H, W), dtype=torch.uint8)
            m[:, H // 5 + 8 * t: H - H // 6, W // 4: W - W // 4 - 8 * t] = 255
            masks.append(m.pin_memory())
        near, far = (float(x) for x in tar["near_far"].reshape(-1)[:2])
        spec = HullSpec(((-300.0, -300.0, near), (300.0, 300.0, far)), grid=GRID, min_views=2, max_miss=V)
        players = {"player": SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE),
                   "player_hull": SequencePlayer(net, exts, ixts, H, W, slots=2, dilate=DILATE, hull=spec)}

        def window(p, T):
            for t in range(T):
                p.submit(u8[(t + 1) % 2], masks[(t + 1) % 2])
                for k in range(K):
                    p.render(idx[k], tar)
                p.flip()

        for p in players.values():
            p.submit(u8[0], masks[0])
            p.flip()
        rec = {k: [] for k in players}
        for r in range(a.warmup + a.samples):
            for k, p in players.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                window(p, a.frames)
                torch.cuda.synchronize()
                if r >= a.warmup:
                    rec[k].append(1e3 * (time.perf_counter() - t0) / a.frames)
        row = {"shape": f"{H}x{W}, V = {V}, {S} views per camera, {K} cameras per time frame, hull grid {GRID[0]}^3",
               "ms_per_time_frame": {k: spread(v) for k, v in rec.items()},
               "occupied_voxels": players["player_hull"].hull_counts.tolist()}
        mt = row["ms_per_time_frame"]
        row["hull_over_plain"] = round(mt["player_hull"]["median"] / mt["player"]["median"], 4)
        res["sequence_player"] = row
        print("sequence_player", json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
