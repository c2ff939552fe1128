#!/usr/bin/env python
"""Time the composite network's cached frame when the foreground boxes MOVE, on the GPU, at tools/time_composite_cached.py's size:
576x768, 3 of 8 cached views, last level rendered, boxes of a quarter of the image, L = 1 and 2 foreground layers.

    timeout -k 10 900 python tools/time_composite_moving.py --parent /path/to/a/built/checkout/of/the/parent/commit \
        --out profiles/composite_moving_timing.json

(run it under a time limit of its own, and chain it to other GPU steps with ``&&``: nothing else should start on the card after a
step that failed).

Rows, per L:
    a  fixed_box        the parent commit's ``forward_cached`` with ``bbox`` that never moves: the floor (every published composite
                        timing was taken like this)
    b  moving_bbox      the parent's ``forward_cached`` with ``bbox`` cycling through 8 positions of one size: what a moving actor
                        costs on the host path — every position is a new shape (new buffers, a new plan), and 8 shapes thrash the
                        4 a network keeps
    c  moving_xy        this tree's ``forward_cached`` with ``bbox_size`` + a device ``bbox_xy`` over the same 8 positions, eager
    d  moving_xy_graph  the same through ONE ``GraphedFrame``: the positions are copied into its static input, one graph launch
                        (every other tensor of a replay's batch is the graph's own static input, so nothing else is copied)
``--parent`` names a checkout of the parent commit with its library built; its package is loaded beside this tree's under another
module name, so rows a and b run the parent's code in the same process and alternate with c and d.  Without ``--parent`` rows a and
b run this tree's ``bbox`` path (whose kernels are the parent's, instruction for instruction) and the output says so.

Protocol: one process, one device.  The four rows of an L alternate inside every one of --samples repetitions after --warmup untimed
rounds, over the same weights, cache, view index and target camera; rows b, c and d walk the same position list, one position per
frame (c's and d's outputs are compared with b's bit for bit at every position once, before the clock starts).  A repetition of a
row is --frames frames, host clock around them, divided by the number of frames, under two protocols: ``back_to_back`` (ONE device
synchronise at the end) and ``sync_per_frame`` (one after every frame).  Reported: the median over the repetitions with min and max
beside it, the ratios b / c and d / c of the medians, and whether c lies within row a's own min-max width of a.

``graph_probe_ms`` (a pass of its own after the rows, back to back, fixed positions): where a replay's time goes — the parent's
``bbox`` frame through the parent's ``GraphedFrame``, the ``bbox_xy`` frame through this tree's, and both the eager frame and the
graph of a network with ``options.single_stream`` (no fork: the captured graph is one chain)."""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
H, W, S, V = 576, 768, 3, 8
SIZES = [(384, 288), (384, 288)]                           # (w, h): a quarter of the image each
FIXED = [(96, 64), (288, 224)]                             # time_composite_cached.py's boxes
# 8 positions of each layer, odd ones among them (x * 0.25 and x * 0.5 truncate), the image's corners included
TRACK = [[(96, 64), (288, 224)], [(101, 67), (283, 221)], [(133, 90), (250, 199)], [(0, 0), (384, 288)],
         [(171, 121), (213, 170)], [(384, 0), (0, 288)], [(239, 155), (155, 111)], [(311, 203), (77, 59)]]
VIEWS = [5, 1, 6]


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def load_package(root, name):
    """The ``enerf_amd`` package of another checkout under the module name ``name`` (its relative imports stay inside it)."""
    pkg = os.path.join(root, "enerf_amd")
    spec = importlib.util.spec_from_file_location(name, os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "composite_moving_timing.json"))
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built (rows a and b)")
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--samples", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import importlib
    from enerf_amd.config import EnerfConfig
    from enerf_amd.graph import GraphedFrame
    from enerf_amd.lib import Options
    from enerf_amd.network_composite import Network
    from enerf_amd.synth import make_batch
    old = load_package(args.parent, "enerf_amd_parent") if args.parent else "enerf_amd"
    OldNetwork = importlib.import_module(old + ".network_composite").Network
    OldGraphedFrame = importlib.import_module(old + ".graph").GraphedFrame
    old_cfg = importlib.import_module(old + ".config").EnerfConfig(viewdir_agg=False).with_cas(
        volume_planes=(32, 8), num_samples=(2, 1), render_if=(False, True))
    dev = torch.device("cuda:0")
    cfg = EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=(False, True))
    base = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(H, W, V, cfg, seed=0, textured=True).items()}
    inps, exts, ixts = (base[k][0].contiguous() for k in ("src_inps", "src_exts", "src_ixts"))
    bg_inps = inps.flip(-1).contiguous()
    n, f = (float(v) for v in base["near_far"][0])
    idx = torch.tensor(VIEWS, dtype=torch.int32, device=dev)
    rows, shapes_kept, probe = {}, {}, {}
    with torch.no_grad():
        for L in (1, 2):
            torch.manual_seed(0)
            net = Network(cfg, L).to(dev).eval().prepare()
            torch.manual_seed(0)
            parent = OldNetwork(old_cfg, L)
            parent.load_state_dict(net.state_dict())
            parent = parent.to(dev).eval().prepare()
            tar = {k: v for k, v in base.items() if not k.startswith("src_")}
            tar["near_far"] = torch.tensor([[(n + 0.1 * (f - n), n + 0.5 * (f - n)), (n + 0.4 * (f - n), n + 0.8 * (f - n))][:L] + [(n, f)]],
                                           dtype=torch.float32, device=dev)
            cache, pcache = net.cache_sources(inps, bg_inps, exts, ixts), parent.cache_sources(inps, bg_inps, exts, ixts)
            boxed = [dict(tar, bbox=[[p + s for p, s in zip(pos[:L], SIZES[:L])]]) for pos in TRACK]       # host-side boxes: no sync
            fixed = dict(tar, bbox=[[p + s for p, s in zip(FIXED[:L], SIZES[:L])]])
            moving = [dict(tar, bbox_size=SIZES[:L], bbox_xy=torch.tensor(pos[:L], dtype=torch.float32, device=dev)) for pos in TRACK]
            graph = GraphedFrame(net, moving[0], fn=lambda b, net=net, cache=cache: net.forward_cached(cache, idx, b))
            for k, (bb, mb) in enumerate(zip(boxed, moving)):            # b == c == d at every position, before the clock starts
                ref = {key: v.clone() for key, v in parent.forward_cached(pcache, idx, bb).items()}
                got = {key: v.clone() for key, v in net.forward_cached(cache, idx, mb).items()}
                rep = graph(mb)
                torch.cuda.synchronize()
                for key in ref:
                    assert torch.equal(got[key], ref[key]) and torch.equal(rep[key], ref[key]), (L, k, key)
            assert len(net._shapes) == 1

            def cycle(run, batches):
                state = {"k": 0}

                def one():
                    b = batches[state["k"] % len(batches)]
                    state["k"] += 1
                    return run(b)
                return one
            rows[L, "a_fixed_box"] = cycle(lambda b, p=parent, c=pcache: p.forward_cached(c, idx, b), [fixed])
            rows[L, "b_moving_bbox"] = cycle(lambda b, p=parent, c=pcache: p.forward_cached(c, idx, b), boxed)
            rows[L, "c_moving_xy"] = cycle(lambda b, net=net, c=cache: net.forward_cached(c, idx, b), moving)
            # (a replay copies every tensor of its batch that is not the graph's own static input: the viewer hands the static
            # inputs back and changes the positions alone — 8 bytes per layer instead of the level's 14 MB of rays)
            rows[L, "d_moving_xy_graph"] = cycle(graph, [dict(graph.static_in, bbox_xy=mb["bbox_xy"]) for mb in moving])
            shapes_kept[L] = (parent, net)
            one = Network(cfg, L)
            one.load_state_dict(net.state_dict())
            one = one.to(dev).eval().prepare()
            one.options = Options(single_stream=1)
            ocache = one.cache_sources(inps, bg_inps, exts, ixts)
            pgraph = OldGraphedFrame(parent, fixed, fn=lambda b, p=parent, c=pcache: p.forward_cached(c, idx, b))
            ograph = GraphedFrame(one, moving[0], fn=lambda b, one=one, c=ocache: one.forward_cached(c, idx, b))
            probe[L, "bbox_graph_parent"] = lambda g=pgraph: g(g.static_in)
            probe[L, "bbox_xy_graph"] = lambda g=graph: g(g.static_in)
            probe[L, "bbox_xy_eager_single_stream"] = lambda one=one, c=ocache, b=moving[0]: one.forward_cached(c, idx, b)
            probe[L, "bbox_xy_graph_single_stream"] = lambda g=ograph: g(g.static_in)
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
        probe_ms = {k: [] for k in probe}
        for rep in range(args.warmup + args.samples):
            for key, run in probe.items():
                run()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.frames):
                    run()
                torch.cuda.synchronize()
                if rep >= args.warmup:
                    probe_ms[key].append((time.perf_counter() - t0) * 1e3 / args.frames)
    names = ("a_fixed_box", "b_moving_bbox", "c_moving_xy", "d_moving_xy_graph")
    frame_ms = {proto: {f"L{L}": {row: spread(t[L, row]) for row in names} for L in (1, 2)} for proto, t in times.items()}
    summary = {}
    for proto, per_l in frame_ms.items():
        summary[proto] = {}
        for L, r in per_l.items():
            a, b, c, d = (r[k] for k in names)
            width = a["max"] - a["min"]
            summary[proto][L] = {"b_over_c": round(b["median"] / c["median"], 3), "d_over_c": round(d["median"] / c["median"], 3),
                                 "c_minus_a_ms": round(c["median"] - a["median"], 4), "a_min_max_width_ms": round(width, 4),
                                 "c_within_a_width_of_a": bool(abs(c["median"] - a["median"]) <= width)}
    out = {"device": torch.cuda.get_device_name(dev),
           "shape": {"H": H, "W": W, "S": S, "V": V, "views": VIEWS, "render_if": [False, True], "sizes": SIZES, "fixed": FIXED, "track": TRACK},
           "protocol": {"frames_per_window": args.frames, "samples": args.samples, "warmup": args.warmup},
           "rows_a_b_from": "a checkout of the parent commit, loaded beside this tree" if args.parent else "this tree's bbox path",
           "frame_ms": frame_ms, "summary": summary,
           "graph_probe_ms": {f"L{L}": {row: spread(probe_ms[L, row]) for row in ("bbox_graph_parent", "bbox_xy_graph",
                                                                                   "bbox_xy_eager_single_stream", "bbox_xy_graph_single_stream")}
                              for L in (1, 2)},
           "shapes_after": {f"L{L}": {"b_moving_bbox": len(p._shapes), "c_moving_xy": len(m._shapes)} for L, (p, m) in shapes_kept.items()},
           "note": "a = forward_cached, bbox fixed; b = forward_cached, bbox cycling through the 8 positions of `track` (a new shape per "
                   "position); c = forward_cached with bbox_size + device bbox_xy over the same positions; d = c through one GraphedFrame; "
                   "b, c and d compared bit for bit at every position before timing"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out["frame_ms"]))
    print(json.dumps(out["summary"]))
    print(json.dumps(out["graph_probe_ms"]))


if __name__ == "__main__":
    main()
