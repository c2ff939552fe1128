"""Fixtures of the composite network's training step (enerf_amd/train_path_composite.py) from the UNMODIFIED reference on CPU: usable
only where the reference tree is present (oracle/ref_loader.py).  From the repository root:

    python tools/make_golden_composite_train.py             # both cases, one subprocess each (the reference's cfg is an import-time global)
    python tools/make_golden_composite_train.py --case t

Per case of tests/composite_train_cases.py::TRAIN_CASES, from the stored weights (tests/golden/composite_weights_*.npz), the network in
``.train()`` mode and loss = sum over the rendered levels of MSE(rgb_level{i}, rgb_{i}) with seeded float32 targets:

    composite_train_<case>_fp32_{out,grad}.npz   the reference's fp32 step: loss, every output (``out/``), BatchNorm's running statistics
                                                 after the step (``stat/``); every parameter gradient (``grad/``, see below)
    composite_train_<case>_fp64_{out,grad}.npz   the same step with the reference's modules in float64 (net.double(), float64 default dtype,
                                                 create_meshgrid in float64), stored rounded to float32
    composite_train_<case>_spread.npz            8 re-runs of the fp32 step with src_inps moved by one ulp (x (1 +- 6e-8), seeded signs):
                                                 per output and running statistic the worst max|draw - fp64| / max|fp64| (``spread/``),
                                                 per parameter the worst distance of its gradient to float64 (``ulp/grad/``); per draw
                                                 the median and 75th percentile of those distances (``meta/draw_median``, ``_p75``)

``--case t --seed N --dry`` prints the figures of another batch seed and writes nothing: a case marked ``seed_chosen_here`` must keep
the bulk (median, 75th percentile) of every one-ulp draw within 3 x its single fp32 draw's, or the tool refuses the seed.

A gradient of at most GRAD_FULL_BELOW elements is stored whole, a larger one as every GRAD_STRIDE-th element (both numbers are in the
file); ``gradmax/`` holds max|.| and ``gradnorm/`` the float64 norm of the whole tensor.  Distances are taken on the stored elements
and scaled by the float64 run's ``gradmax``.  No file passes 1 MiB."""
import argparse
import functools
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden")


def run_case(name, seed=None, dry=False):
    """``seed``: try another batch seed for the case (with ``dry``: print the figures, write nothing)."""
    import composite_train_cases as TC
    from oracle.ref_loader import load_reference
    if seed is not None:
        TC.TRAIN_CASES[name] = dict(TC.TRAIN_CASES[name], seed=int(seed))
    c = TC.TRAIN_CASES[name]
    ecfg = TC.train_config(name)
    lst = lambda v: ",".join(map(str, v))
    cfg, _ = load_reference("configs/enerf/enerf_outdoor/actor1.yaml",
                            ["num_fg_layers", str(c["L"]), "enerf.cas_config.render_if", lst(c["render_if"])])
    from lib.networks.enerf import network_composite as ref_network
    from lib.networks.enerf import utils as ref_utils
    from enerf_amd.config import EnerfConfig
    assert EnerfConfig.from_yacs(cfg) == ecfg, (EnerfConfig.from_yacs(cfg), ecfg)
    torch.set_num_threads(1)                       # fixed summation order
    sd = TC.train_weights(name)
    base = {k: torch.from_numpy(v) for k, v in TC.train_batch(name).items()}
    levels = [i for i, on in enumerate(c["render_if"]) if on]
    sample = lambda flat: flat if flat.numel() <= TC.GRAD_FULL_BELOW else flat[::TC.GRAD_STRIDE]

    def step(batch, fp64=False):
        torch.manual_seed(0)
        net = ref_network.Network()
        missing = net.load_state_dict(sd, strict=False)
        assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
        net.train()
        batch = dict(batch)                        # (the reference re-binds batch['near_far'])
        plain_grid = ref_utils.create_meshgrid
        if fp64:                                   # oracle/make_golden.py:369-375
            net = net.double()
            torch.set_default_dtype(torch.float64)
            batch = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
            ref_utils.create_meshgrid = functools.partial(plain_grid, dtype=torch.float64)
        try:
            out = net(batch)
            loss = sum(torch.nn.functional.mse_loss(out[f"rgb_level{i}"], batch[f"rgb_{i}"]) for i in levels)
            loss.backward()
        finally:
            torch.set_default_dtype(torch.float32)
            ref_utils.create_meshgrid = plain_grid
        res = {"loss": float(loss.detach())}
        res["out"] = {k: v.detach().double() for k, v in out.items() if v is not None and not k.startswith("idx")}
        res["stat"] = {k: v.detach().double().clone() for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var"))}
        res["grad"] = {k: (None if p.grad is None else p.grad.detach().double().reshape(-1)) for k, p in net.named_parameters()}
        return res

    def save(run, tag):
        if dry:
            return
        o = {"loss": np.array(run["loss"], np.float64)}
        o.update({f"out/{k}": v.float().numpy() for k, v in run["out"].items()})
        o.update({f"stat/{k}": v.float().numpy() for k, v in run["stat"].items()})
        g = {"meta/full_below": np.array(TC.GRAD_FULL_BELOW), "meta/stride": np.array(TC.GRAD_STRIDE)}
        for k, v in run["grad"].items():
            if v is None:
                continue
            g[f"grad/{k}"] = sample(v).float().numpy().copy()
            g[f"gradmax/{k}"], g[f"gradnorm/{k}"] = np.array(float(v.abs().max())), np.array(float(v.norm()))
        for part, d in (("out", o), ("grad", g)):
            path = os.path.join(GOLDEN, TC.TRAIN_FILES.format(name, f"{tag}_{part}"))
            np.savez_compressed(path, **d)
            print(f"case {name}: wrote {path} ({os.path.getsize(path)} bytes)")
            assert os.path.getsize(path) < (1 << 20), path

    rel = lambda a, b: float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)
    r64 = step(base, fp64=True)
    r32 = step(base)
    print(f"case {name}: loss fp32 {r32['loss']:.10g} fp64 {r64['loss']:.10g}")
    none = sorted(k for k, v in r64["grad"].items() if v is None)
    print(f"case {name}: {len(r64['grad'])} parameters, without a gradient: {none}")
    assert none == sorted(k for k, v in r32["grad"].items() if v is None)
    save(r32, "fp32")
    save(r64, "fp64")
    scale = {k: float(v.abs().max()) for k, v in r64["grad"].items() if v is not None}
    gdist = lambda run, k: float((sample(run["grad"][k]) - sample(r64["grad"][k])).abs().max()) / scale[k]
    names = [k for k in scale if scale[k] >= TC.GRAD_TINY]
    single = {k: gdist(r32, k) for k in names}
    print(f"case {name}: {len(names)} compared parameters; fp32-to-fp64 distance median {np.median(list(single.values())):.2e}, "
          f"{sum(v > 1e-3 for v in single.values())} beyond 1e-3, worst {max(single.values()):.2e}")
    spread = {f"spread/{kind}/{k}": rel(r32[kind][k], v) for kind in ("out", "stat") for k, v in r64[kind].items()}
    ulp = {k: 0.0 for k in names}
    bulk = lambda d: (float(np.median(list(d.values()))), float(np.percentile(list(d.values()), 75)))
    draw_bulk = []
    for d in range(1, TC.ONE_ULP_DRAWS + 1):
        gen = torch.Generator().manual_seed(d)
        batch = dict(base)
        sign = torch.randint(0, 2, base["src_inps"].shape, generator=gen).float() * 2 - 1
        batch["src_inps"] = base["src_inps"] * (1 + 6e-8 * sign)
        run = step(batch)
        for kind in ("out", "stat"):
            for k, v in r64[kind].items():
                spread[f"spread/{kind}/{k}"] = max(spread[f"spread/{kind}/{k}"], rel(run[kind][k], v))
        dd = {k: gdist(run, k) for k in names}
        for k in names:
            ulp[k] = max(ulp[k], dd[k])
        draw_bulk.append(bulk(dd))
        print(f"case {name} draw {d}: gradients median {np.median(list(dd.values())):.2e} max {max(dd.values()):.2e}; outputs worst "
              f"{max(rel(run['out'][k], v) for k, v in r64['out'].items()):.2e}", flush=True)
    # The step is discontinuous in its inputs (ReLU masks under batch statistics, floor() of sample positions).  The tests hold the
    # median and the 75th percentile of a port's distances to 3 x those of the reference's SINGLE fp32 draw, so a case is only usable
    # where the reference's own one-ulp draws satisfy that: a batch seed on which the reference itself is bimodal in bulk is refused
    # here, on the reference alone (a case whose seed the tests fix elsewhere is reported, not refused).
    worst_bulk = tuple(max(b[j] for b in draw_bulk) / bulk(single)[j] for j in (0, 1))
    print(f"case {name} seed {c['seed']}: single draw median {bulk(single)[0]:.2e} p75 {bulk(single)[1]:.2e}; worst one-ulp draw / single: "
          f"median x{worst_bulk[0]:.1f}, p75 x{worst_bulk[1]:.1f}")
    if "seed_chosen_here" in c:
        assert max(worst_bulk) <= 3.0, f"case {name}: the reference is bimodal in bulk on seed {c['seed']}; choose another seed"
    if dry:
        return
    out = {k: np.array(v) for k, v in spread.items()}
    out.update({"meta/draw_median": np.array([b[0] for b in draw_bulk]), "meta/draw_p75": np.array([b[1] for b in draw_bulk])})
    out.update({f"ulp/grad/{k}": np.array(v) for k, v in ulp.items()})
    out.update({"meta/draws": np.array(TC.ONE_ULP_DRAWS), "meta/torch_version": np.array(torch.__version__),
                "meta/perturbation": np.array("src_inps * (1 +- 6e-8), seeded signs (torch.Generator seeds 1..draws)")})
    path = os.path.join(GOLDEN, TC.TRAIN_FILES.format(name, "spread"))
    np.savez_compressed(path, **out)
    print(f"case {name}: wrote {path} ({os.path.getsize(path)} bytes); worst output spread "
          f"{max(v for k, v in spread.items() if k.startswith('spread/out/')):.2e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    ap.add_argument("--seed", type=int, default=None, help="try this batch seed for --case")
    ap.add_argument("--dry", action="store_true", help="print the figures, write no fixture")
    args = ap.parse_args()
    if args.case:
        run_case(args.case, args.seed, args.dry)
    else:
        for name in ("t", "a"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], check=True, cwd=ROOT)
