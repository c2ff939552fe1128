"""Fixtures of the composite network (enerf_amd/network_composite.py) from the UNMODIFIED reference on CPU: usable only where the
reference tree is present (oracle/ref_loader.py).  From the repository root:

    python tools/make_golden_composite.py             # both cases, one subprocess each (the reference's cfg is an import-time global)
    python tools/make_golden_composite.py --case a

Case "a" (two foreground layers) also writes the network's state dict, tests/golden/composite_weights_*.npz: seeded default
init with randomised BatchNorm statistics / affine and MLP biases (oracle/make_golden.py::seeded_state_dict), split so that no file
passes 1 MiB.  Case "b" (one layer) loads it minus the ``*_layer1.*`` keys (tests/composite_cases.py::NETWORK_CASES).  Per case,
tests/golden/composite_<case>.npz holds every output of the rendered levels except ``idx`` and, per level, each layer's and the
background's regressed depth / std maps (``mid/...``).  Inputs are regenerated from tests/composite_cases.py::network_batch."""
import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
GOLDEN = os.path.join(ROOT, "tests", "golden")
MAX_FILE = 900 * 1024          # bytes of arrays per weight file (they barely compress)


def run_case(name):
    import composite_cases as CC
    from oracle.make_golden import seeded_state_dict
    from oracle.ref_loader import load_reference
    c = CC.NETWORK_CASES[name]
    ecfg = CC.network_config(name)
    lst = lambda v: ",".join(map(str, v))
    cfg, _ = load_reference("configs/enerf/enerf_outdoor/actor1.yaml",
                            ["num_fg_layers", str(c["L"]), "enerf.cas_config.render_if", lst(c["render_if"])])
    from lib.networks.enerf import network_composite as ref_network
    from lib.networks.enerf import utils as ref_utils
    from enerf_amd.config import EnerfConfig
    assert cfg.network_module == "lib.networks.enerf.network_composite" and int(cfg.num_fg_layers) == c["L"]
    assert EnerfConfig.from_yacs(cfg) == ecfg, (EnerfConfig.from_yacs(cfg), ecfg)

    torch.manual_seed(0)
    torch.set_num_threads(1)                       # fixed summation order
    net = ref_network.Network().eval()
    keys = {k for k in net.state_dict() if not k.endswith("num_batches_tracked")}
    wfiles = sorted(f for f in os.listdir(GOLDEN) if f.startswith("composite_weights_"))
    if c["L"] == 2:
        sd = {k: v for k, v in seeded_state_dict(net).items() if k in keys}
        net.load_state_dict(sd, strict=False)
        for f in wfiles:
            os.remove(os.path.join(GOLDEN, f))
        part, size, n = {}, 0, 0
        for k in sorted(sd):
            a = sd[k].numpy()
            if part and size + a.nbytes > MAX_FILE:
                np.savez_compressed(os.path.join(GOLDEN, CC.WEIGHT_FILES.format(n)), **part)
                part, size, n = {}, 0, n + 1
            part[k] = a
            size += a.nbytes
        np.savez_compressed(os.path.join(GOLDEN, CC.WEIGHT_FILES.format(n)), **part)
    else:
        assert wfiles, "run case a first: it writes the weights"
    sd = CC.network_weights(name)
    assert set(sd) == keys, sorted(set(sd) ^ keys)[:8]                   # exactly the reference network's key set
    n_par = sum(v.numel() for k, v in sd.items() if not k.endswith(("running_mean", "running_var")))
    print(f"case {name}: {len(sd)} tensors, {n_par} parameters")
    # the reference network's own counts (state dict with BatchNorm's batch counters, parameters)
    assert (len(net.state_dict()), sum(p.numel() for p in net.parameters()), n_par) == {2: (440, 599330, 599330), 1: (324, 424460, 424460)}[c["L"]]
    net.load_state_dict(sd, strict=False)

    batch = {k: torch.from_numpy(v) for k, v in CC.network_batch(name).items()}
    mids = []
    plain = ref_utils.depth_regression

    def recording(*a, **k):
        out = plain(*a, **k)
        mids.append(out)
        return out
    ref_utils.depth_regression = recording
    with torch.no_grad():
        ret = net(batch)
    ref_utils.depth_regression = plain
    L, cas = c["L"], ecfg.cas
    assert len(mids) == cas.num * (L + 1)
    out = {}
    for i in range(cas.num):
        for j in range(L + 1):
            who = f"layer{j}" if j < L else "bg"
            d, s = mids[i * (L + 1) + j]
            out[f"mid/depth_{i}_{who}"], out[f"mid/std_{i}_{who}"] = d.numpy(), s.numpy()
    for k, v in ret.items():
        if not k.startswith("idx"):
            out[k] = v.numpy()
    for i in range(cas.num):
        if not cas.render_if[i]:
            assert f"rgb_level{i}" not in ret
            continue
        Ns, rs = cas.num_samples[i], cas.render_scale[i]
        if L > 1:
            z = ret[f"z_vals_level{i}"][0]                               # (N, L*Ns), concatenation order
            Hr, Wr = int(c["H"] * rs), int(c["W"] * rs)
            cover = torch.zeros(L, Hr, Wr, dtype=torch.bool)
            for l, box in enumerate(c["boxes"]):
                x, y, w, h = (int(v * rs) for v in box)
                cover[l, y:y + h, x:x + w] = True
            both = (cover.sum(0) == L).reshape(-1)
            assert int(both.sum()) > 0
            zb = z[both]
            order = torch.sort(zb, -1).indices
            assert bool((order != torch.arange(L * Ns)[None]).any(-1).all()), "sorted order equals the concatenation order somewhere"
            gap = min(float(((zb[:, a * Ns:(a + 1) * Ns, None] - zb[:, None, b * Ns:(b + 1) * Ns]).abs() /
                             zb[:, a * Ns:(a + 1) * Ns, None].abs()).min()) for a in range(L) for b in range(a + 1, L))
            print(f"case {name} level {i}: {int(both.sum())} doubly covered pixels, smallest cross-layer |dz| / z = {gap:.3g}")
            assert gap >= 1e-3, gap
    path = os.path.join(GOLDEN, f"composite_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"case {name}: wrote {path} ({os.path.getsize(path)} bytes), keys {sorted(out)}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    args = ap.parse_args()
    if args.case:
        run_case(args.case)
    else:
        for name in ("a", "b"):
            subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], check=True, cwd=ROOT)
