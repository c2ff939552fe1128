"""Golden vectors for tests/test_integration_reference_loader.py, so that the binding modules under ``integration/`` are
checked on machines without the reference tree.

TEST INFRASTRUCTURE (build container only).  Per case (``dtu``: dtu_pretrain.yaml with the binding module selected and
volume_planes 8,8; ``human``: zjumocap_eval.yaml) it records, from the UNMODIFIED reference:

  * the ``cfg.enerf`` values ``EnerfConfig.from_yacs`` reads and the ``network_path`` the reference's config derives,
  * the names, shapes and dtypes of the reference network's state_dict (the values are ``seeded_state_dict`` of them: the
    test rebuilds the same weights instead of storing them),
  * the reference network's own forward with those weights on the seeded synthetic batch (``make_batch`` /
    ``make_zju_batch``, seed 1, rebuilt by the test as well),

into ``tests/golden/integration_<case>.npz``.  One process per case: the reference's cfg is an import-time global.

    python oracle/make_golden_integration.py
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
ENERF_KEYS = ("viewdir_agg", "white_bkgd", "chunk_size")
CAS_KEYS = ("num", "depth_inv", "volume_scale", "volume_planes", "im_feat_scale", "im_ibr_scale", "render_scale",
            "render_im_feat_level", "nerf_model_feat_ch", "render_if", "num_samples")


def seeded_state_dict(spec):
    """State_dict values from ``spec`` = [(name, shape, dtype)]: fan-in-scaled uniform weights, BatchNorm affine and running
    statistics near their usual values, integer counters zero — one numpy generator, seed 0, in spec order."""
    rng = np.random.default_rng(0)
    sd = {}
    for name, shape, dtype in spec:
        if not dtype.startswith("float"):
            v = np.zeros(shape, dtype=dtype)
        elif name.endswith("running_var"):
            v = rng.uniform(0.5, 1.5, shape)
        elif len(shape) == 1 and name.endswith("weight"):
            v = rng.uniform(0.5, 1.5, shape)
        elif len(shape) == 1:                                            # biases, BatchNorm bias, running_mean
            v = rng.normal(0.0, 0.1, shape)
        else:
            bound = 1.0 / np.sqrt(np.prod(shape[1:]))
            v = rng.uniform(-bound, bound, shape)
        sd[name] = torch.from_numpy(np.asarray(v, dtype=dtype))
    return sd


def one(case):
    from oracle.ref_loader import load_reference
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch, make_zju_batch
    human = case == "human"
    module = "lib.networks.enerf.network_human_amd" if human else "lib.networks.enerf.network_amd"
    cfg_file = "configs/enerf/zjumocap_eval.yaml" if human else "configs/enerf/dtu_pretrain.yaml"
    opts = ["network_module", module] + ([] if human else ["enerf.cas_config.volume_planes", "8,8"])
    cfg, ref_network = load_reference(cfg_file, opts)
    if human:
        from lib.networks.enerf import network_human as ref_network
    plain = lambda v: [plain(x) for x in v] if isinstance(v, (list, tuple)) else v
    yacs = {"network_module": cfg.network_module, "network_path": cfg.network_path,
            "enerf": {**{k: plain(cfg.enerf[k]) for k in ENERF_KEYS},
                      "cas_config": {k: plain(cfg.enerf.cas_config[k]) for k in CAS_KEYS}}}
    ecfg = EnerfConfig.from_yacs(cfg)
    ref = ref_network.Network().eval()
    spec = [(k, list(v.shape), str(v.dtype).replace("torch.", "")) for k, v in ref.state_dict().items()]
    ref.load_state_dict(seeded_state_dict(spec), strict=True)
    b = make_zju_batch(32, 32, 2, ecfg, seed=1) if human else make_batch(32, 64, 3, ecfg, seed=1, textured=True)
    torch.set_num_threads(1)
    with torch.no_grad():
        want = ref({k: torch.from_numpy(v) for k, v in b.items()})
    save = {"cfg_json": np.array(json.dumps(yacs)), "state_dict_spec": np.array(json.dumps(spec))}
    save.update({f"out/{k}": v.numpy() for k, v in want.items()})
    np.savez_compressed(os.path.join(OUT, f"integration_{case}.npz"), **save)
    print(case, len(spec), "tensors in the state_dict,", sorted(want))


if __name__ == "__main__":
    if len(sys.argv) > 1:
        one(sys.argv[1])
    else:
        for case in ("dtu", "human"):
            subprocess.run([sys.executable, os.path.abspath(__file__), case], check=True)
