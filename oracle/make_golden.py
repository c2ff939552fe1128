"""Generate golden vectors by running the UNMODIFIED reference on CPU (build container only).

TEST INFRASTRUCTURE.  Usage (from the repo root):

    python oracle/make_golden.py            # regenerates every case (one subprocess per case,
                                            # because the reference's cfg is an import-time global)
    python oracle/make_golden.py --case tiny_s3

Writes ``tests/golden/weights_seed0.npz`` (the reference state_dict: seeded default init with
randomised BN statistics/affine and MLP biases) and ``tests/golden/<case>.npz``
(reference outputs + stage-boundary intermediates).  Inputs are NOT stored: they are regenerated
from ``enerf_amd.synth.make_batch`` with the seed recorded in CASES (numpy PCG64, platform-stable).
"""
from __future__ import annotations

import argparse
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

# case -> dict(H, W, S, planes, render_if, seed, textured, human, full_intermediates)
CASES = {
    "tiny_s3": dict(H=32, W=64, S=3, planes=(8, 8), render_if=(True, True), seed=1, textured=False,
                    human=False, inter="all"),
    "tiny_s2": dict(H=32, W=64, S=2, planes=(8, 8), render_if=(True, True), seed=2, textured=True,
                    human=False, inter="none"),
    "tiny_s4_mask": dict(H=32, W=64, S=4, planes=(8, 8), render_if=(False, True), seed=3, textured=True,
                         human=True, inter="none"),
    "small_s3_eval": dict(H=64, W=96, S=3, planes=(16, 8), render_if=(False, True), seed=4, textured=True,
                          human=False, inter="maps"),
    # BASELINE config 3 at reduced size: the reference's own lego.yaml (S=4, render_if True,True, planes 64,8), lego
    # pinhole intrinsics and near_far [2.5, 5.5] (enerf_amd.synth.make_lego_batch)
    "lego_small": dict(H=64, W=64, S=4, planes=(64, 8), render_if=(True, True), seed=5, human=False, inter="maps",
                       rig="lego", cfg_file="configs/enerf/nerf/lego.yaml"),
    # BASELINE config 4 at reduced size: zjumocap_eval.yaml (network_human, planes 32,8, render_if False,True) with
    # 4 source views and the projected-bbox mask_at_box (enerf_amd.synth.make_zju_batch)
    "zju_small": dict(H=64, W=64, S=4, planes=(32, 8), render_if=(False, True), seed=6, human=True, inter="maps",
                      rig="zju", cfg_file="configs/enerf/zjumocap_eval.yaml"),
    # the reference's fourth eval config on this path (configs/enerf/llff_eval.yaml: planes 32,8, render_if False,True, 640x960)
    # at 1/5 of its size (the reference's U-Nets need H, W divisible by 32): the 2:3 aspect, level-0 volume 32 x 16 x 24
    "llff_small": dict(H=128, W=192, S=3, planes=(32, 8), render_if=(False, True), seed=7, textured=True, human=False,
                       inter="maps", cfg_file="configs/enerf/llff_eval.yaml"),
    # configs/enerf/dtu_pretrain_nocascade.yaml as shipped (one level: volume_scale 0.25, render_scale 1.0, feature level 2,
    # nerf_model_feat_ch 8, num_samples 2) with volume_planes 8; its network takes weights_seed0 by the rule "nocascade"
    # (tests/golden_cases.py::WEIGHT_RULES).  inter: what oracle.forward reports back (no per-sample tensors: size)
    "nocascade_tiny": dict(H=32, W=64, S=3, planes=(8,), render_if=(True,), seed=8, textured=True, human=False, inter="oracle",
                           base_cfg="configs/enerf/dtu_pretrain_nocascade.yaml", weights="nocascade"),
    # configs/enerf/enerf_outdoor/actor1.yaml's enerf block (viewdir_agg False, volume_planes 32,8, num_samples 2,1) on top of its
    # parent dtu_pretrain.yaml, both levels rendered, through the plain lib.networks.enerf.network: that yaml's network_composite
    # and its layered foreground are out of scope here
    "outdoor_tiny": dict(H=32, W=64, S=3, planes=(32, 8), render_if=(True, True), seed=9, textured=True, human=False, inter="oracle",
                         cas=dict(num_samples=(2, 1)), viewdir_agg=False, weights="outdoor"),
}


sys.path.insert(0, os.path.join(ROOT, "tests"))
from adversarial import ADV_CASES, regime_stats, tweak_batch, tweak_weights  # noqa: E402  (tests/adversarial.py: shared case table)

# adversarial-regime cases: the base batch / weights plus the edits of tests/adversarial.py
for _n, _c in ADV_CASES.items():
    CASES[_n] = dict(H=_c["H"], W=_c["W"], S=_c["S"], planes=_c["planes"], render_if=_c["render_if"], seed=_c["seed"],
                     textured=_c["textured"], human=False, inter="maps", adv=True, white_bkgd=bool(_c.get("white_bkgd")))


def seeded_state_dict(net) -> dict:
    """Default init under seed 0 is done by the caller; here: non-trivial BN + biases (seed 1)."""
    g = torch.Generator().manual_seed(1)
    sd = net.state_dict()
    for k, v in sd.items():
        if k.endswith("running_mean"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
        elif k.endswith("running_var"):
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif (".bn." in k or k.split(".")[-2] == "1") and k.endswith("weight") and v.dim() == 1:
            v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        elif k.endswith("bias") and v.dim() == 1 and ("nerf_" in k or ".bn." in k or k.split(".")[-2] == "1"):
            v.copy_(torch.randn(v.shape, generator=g) * 0.1)
    return sd


def run_case(name: str) -> None:
    from oracle.ref_loader import load_reference
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch, make_lego_batch, make_zju_batch

    c = CASES[name]
    if "cfg_file" in c:                            # the reference's own yaml for that dataset, no overrides
        cfg, ref_network = load_reference(c["cfg_file"], [])
        assert tuple(cfg.enerf.cas_config.volume_planes) == c["planes"]
        assert tuple(cfg.enerf.cas_config.render_if) == c["render_if"]
        assert cfg.network_module.endswith("network_human") == c["human"]
    else:
        lst = lambda v: ",".join(map(str, v)) + ("," if len(v) == 1 else "")       # ("8," parses as a one-element list)
        opts = ["enerf.cas_config.volume_planes", lst(c["planes"]), "enerf.cas_config.render_if", lst(c["render_if"])]
        for k, v in c.get("cas", {}).items():
            opts += [f"enerf.cas_config.{k}", lst(v)]
        if "viewdir_agg" in c:
            opts += ["enerf.viewdir_agg", str(c["viewdir_agg"])]
        if c.get("white_bkgd"):
            opts += ["enerf.white_bkgd", "True"]
        cfg, ref_network = load_reference(c.get("base_cfg", "configs/enerf/dtu_pretrain.yaml"), opts)
        assert bool(cfg.enerf.white_bkgd) == bool(c.get("white_bkgd"))
        assert tuple(cfg.enerf.cas_config.volume_planes) == c["planes"] and tuple(cfg.enerf.cas_config.render_if) == c["render_if"]
        assert bool(cfg.enerf.viewdir_agg) == c.get("viewdir_agg", True) and cfg.network_module == "lib.networks.enerf.network"
    if c["human"]:
        from lib.networks.enerf import network_human as ref_network  # noqa: F811
    from lib.networks.enerf import utils as ref_utils

    torch.manual_seed(0)
    torch.set_num_threads(1)                       # fixed summation order
    net = ref_network.Network().eval()
    wpath = os.path.join(GOLDEN, "weights_seed0.npz")
    if c.get("weights"):                           # a network weights_seed0 does not fit as it is: the case's rule derives its state dict
        from golden_cases import derive_weights
        wz = np.load(wpath)
        sd = derive_weights({k: torch.from_numpy(wz[k]) for k in wz.files}, c["weights"])
        assert set(sd) == {k for k in net.state_dict() if not k.endswith("num_batches_tracked")}
        net.load_state_dict(sd, strict=False)
    else:
        sd = seeded_state_dict(net)
        net.load_state_dict(sd)
        wnp = {k: v.numpy() for k, v in sd.items() if not k.endswith("num_batches_tracked")}
        if os.path.exists(wpath):
            old = np.load(wpath)
            assert all(np.array_equal(old[k], wnp[k]) for k in wnp), "weights changed between cases"
        else:
            np.savez_compressed(wpath, **wnp)

    ecfg = EnerfConfig.from_yacs(cfg)
    if c.get("rig") == "lego":
        batch_np = make_lego_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"])
    elif c.get("rig") == "zju":
        batch_np = make_zju_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"])
    else:
        batch_np = make_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"], textured=c["textured"],
                              mask_box=c["human"])
    if c.get("adv"):                               # edits on top of the pinned seeded weights / batch (tests/adversarial.py)
        net.load_state_dict(tweak_weights({k: v.clone() for k, v in sd.items()}, name))
        batch_np = tweak_batch(batch_np, name)
    batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}

    # record stage boundaries by wrapping the reference's own functions (no reference code is edited)
    rec = {}
    level = {"i": -1}

    def tap(fn_name, handler):
        orig = getattr(ref_utils, fn_name)

        def wrapped(*a, **k):
            out = orig(*a, **k)
            handler(out, a, k)
            return out
        setattr(ref_utils, fn_name, wrapped)

    def on_volume(out, a, k):
        level["i"] = k["level"]
        i = level["i"]
        rec[f"vol_{i}"], rec[f"dv_{i}"], rec[f"nf_{i}"] = out

    def on_reg(out, a, k):
        i = level["i"]
        rec[f"depth_{i}"], rec[f"std_{i}"] = out
        rec[f"prob_{i}"] = a[0]

    tap("build_feature_volume", on_volume)
    tap("depth_regression", on_reg)
    tap("build_rays", lambda out, a, k: rec.__setitem__(f"rays12_{level['i']}", out))
    tap("get_vox_feat", lambda out, a, k: (rec.__setitem__(f"vox_{level['i']}", out),
                                           rec.__setitem__(f"feat3d_{level['i']}", a[1])))
    tap("get_img_feat", lambda out, a, k: rec.__setitem__(f"img_{level['i']}", out))
    tap("get_proj_mats", lambda out, a, k: rec.__setitem__(f"proj_{level['i'] + 1}", out))
    for i in range(int(cfg.enerf.cas_config.num)):
        m = getattr(net, f"nerf_{i}")
        m.register_forward_hook(lambda mod, inp, out, i=i: rec.__setitem__(f"raw_{i}", out))
        r = getattr(net, f"cost_reg_{i}")
        r.register_forward_hook(lambda mod, inp, out, i=i: rec.__setitem__(f"feat3d_{i}", out[0]))
    feats = {}
    net.feature_net.register_forward_hook(
        lambda mod, inp, out: feats.update(feat_l0=out[0], feat_l1=out[1], feat_l2=out[2]))

    with torch.no_grad():
        out = net(batch)

    save = {f"out/{k}": v.numpy() for k, v in out.items()}
    inter = c["inter"]
    if inter == "all":
        save.update({f"mid/{k}": v.detach().numpy() for k, v in rec.items()})
        save.update({f"mid/{k}": v.detach().numpy() for k, v in feats.items()})
    elif inter == "oracle":                        # the stage boundaries oracle.forward(intermediates=) hands back
        for k, v in rec.items():
            if k.split("_")[0] in ("vol", "dv", "nf", "feat3d", "prob", "depth", "std", "rays12", "proj"):
                save[f"mid/{k}"] = v.detach().numpy()
    elif inter == "maps":
        for k, v in rec.items():
            if k.split("_")[0] in ("depth", "std", "nf", "proj", "rays12"):
                save[f"mid/{k}"] = v.detach().numpy()
    save["meta/torch_version"] = np.array(torch.__version__)
    if c.get("adv"):                               # how deep into its regime the case is (asserted again by the tests)
        import json
        st = regime_stats(ecfg, {k: v.detach() for k, v in net.state_dict().items()}, batch)
        save["meta/regime"] = np.array(json.dumps(st))
        print(f"[golden] {name} regime: {st}")
    np.savez_compressed(os.path.join(GOLDEN, f"{name}.npz"), **save)
    rgb = out[[k for k in out if k.startswith("rgb")][-1]]
    print(f"[golden] {name}: {len(save)} arrays; rgb mean {rgb.mean():.4f} min {rgb.min():.4f} "
          f"max {rgb.max():.4f}; keys {sorted(out)}")


# BASELINE configs 2, 3, 4 at their REAL shapes (the frames tests/test_gpu_parity.py::test_full_size_* and bench.py render).
# The outputs are too large to commit whole, so each tensor is stored as: every STRIDE-th row (ray / pixel), its float64
# L2 norm, sum and max|.|, and a 64-bit checksum of the reference's raw bytes (regeneration check).  < 1 MB per case.
FULL_STRIDE = 97
FULL_CASES = {
    "dtu_full": dict(H=512, W=640, S=3, planes=(48, 8), render_if=(False, True), seed=0, textured=True, human=False),
    # BASELINE configs[0] (configs/enerf/dtu/scan114.yaml shape): 512x640, 3 views, planes 48,8, BOTH levels rendered
    "dtu_full_tt": dict(H=512, W=640, S=3, planes=(48, 8), render_if=(True, True), seed=0, textured=True, human=False),
    "lego_full": dict(H=800, W=800, S=4, planes=(64, 8), render_if=(True, True), seed=5, human=False, rig="lego",
                      cfg_file="configs/enerf/nerf/lego.yaml"),
    "zju_full": dict(H=1024, W=1024, S=4, planes=(32, 8), render_if=(False, True), seed=6, human=True, rig="zju",
                     cfg_file="configs/enerf/zjumocap_eval.yaml"),
    # configs/enerf/llff_eval.yaml at its own size (input_h_w 640, 960; the reference's fourth eval config; not a BASELINE config)
    "llff_full": dict(H=640, W=960, S=3, planes=(32, 8), render_if=(False, True), seed=7, textured=True, human=False,
                      cfg_file="configs/enerf/llff_eval.yaml"),
}


def sparse_digest(prefix: str, t, save: dict) -> None:
    """rows[::FULL_STRIDE] of the tensor viewed as (rows, last_dim) + whole-tensor statistics."""
    import zlib
    a = np.ascontiguousarray(t.detach().numpy() if hasattr(t, "detach") else t)
    rows = a.reshape(-1, a.shape[-1]) if a.ndim >= 2 and a.shape[-1] <= 16 else a.reshape(-1, 1)
    save[f"{prefix}/rows"] = rows[::FULL_STRIDE].copy()
    save[f"{prefix}/shape"] = np.array(a.shape, np.int64)
    f = a.astype(np.float64).reshape(-1)
    save[f"{prefix}/norm"] = np.array(np.sqrt((f * f).sum()))
    save[f"{prefix}/sum"] = np.array(f.sum())
    save[f"{prefix}/absmax"] = np.array(np.abs(f).max() if f.size else 0.0)
    raw = a.tobytes()
    save[f"{prefix}/crc64"] = np.array([zlib.crc32(raw), zlib.adler32(raw)], np.uint32)   # two 32-bit halves


def run_full_case(name: str) -> None:
    """One full-size frame through the UNMODIFIED reference (network.py:76-113 / network_human.py:69-119) on CPU."""
    import time
    from oracle.ref_loader import load_reference
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch, make_lego_batch, make_zju_batch

    c = FULL_CASES[name]
    if "cfg_file" in c:
        cfg, ref_network = load_reference(c["cfg_file"], [])
        assert tuple(cfg.enerf.cas_config.volume_planes) == c["planes"]
        assert tuple(cfg.enerf.cas_config.render_if) == c["render_if"]
    else:
        opts = ["enerf.cas_config.volume_planes", ",".join(map(str, c["planes"])),
                "enerf.cas_config.render_if", ",".join(map(str, c["render_if"]))]
        cfg, ref_network = load_reference("configs/enerf/dtu_pretrain.yaml", opts)
    if c["human"]:
        from lib.networks.enerf import network_human as ref_network  # noqa: F811
    from lib.networks.enerf import utils as ref_utils
    torch.manual_seed(0)
    torch.set_num_threads(1)                       # fixed summation order
    net = ref_network.Network().eval()
    sd = seeded_state_dict(net)
    net.load_state_dict(sd)
    wnp = np.load(os.path.join(GOLDEN, "weights_seed0.npz"))
    assert all(np.array_equal(wnp[k], v.numpy()) for k, v in sd.items() if k in wnp.files), "weights differ from weights_seed0"
    ecfg = EnerfConfig.from_yacs(cfg)
    if c.get("rig") == "lego":
        batch_np = make_lego_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"])
    elif c.get("rig") == "zju":
        batch_np = make_zju_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"])
    else:
        batch_np = make_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"], textured=c["textured"])
    batch = {k: torch.from_numpy(v) for k, v in batch_np.items()}
    rec, level = {}, {"i": -1}
    orig_vol, orig_reg = ref_utils.build_feature_volume, ref_utils.depth_regression

    def vol(*a, **k):
        level["i"] = k["level"]
        out = orig_vol(*a, **k)
        rec[f"nf_{level['i']}"] = out[2]
        return out

    def reg(*a, **k):
        out = orig_reg(*a, **k)
        rec[f"depth_{level['i']}"], rec[f"std_{level['i']}"] = out
        return out
    ref_utils.build_feature_volume, ref_utils.depth_regression = vol, reg
    t0 = time.perf_counter()
    with torch.no_grad():
        out = net(batch)
    dt = time.perf_counter() - t0
    save = {}
    for k, v in out.items():
        sparse_digest(f"out/{k}", v, save)
    for k, v in rec.items():
        sparse_digest(f"mid/{k}", v.reshape(-1, 1), save)
    save["meta/torch_version"] = np.array(torch.__version__)
    save["meta/stride"] = np.array(FULL_STRIDE)
    save["meta/reference_cpu_seconds_1thread"] = np.array(dt)
    np.savez_compressed(os.path.join(GOLDEN, f"{name}.npz"), **save)
    print(f"[golden] {name}: {len(save)} arrays, reference forward {dt:.1f} s on 1 thread; keys {sorted(out)}")


TRAIN_CASE = dict(H=32, W=64, S=3, planes=(8, 8), render_if=(True, True), seed=7, loss_weight=(0.1, 1.0))
TRAIN_CASES = {"train_tiny": TRAIN_CASE,
               # a mid-size step: 128x160, 16 + 8 planes, 20,480 + 1,280 rays
               "train_small": dict(H=128, W=160, S=3, planes=(16, 8), render_if=(True, True), seed=8, loss_weight=(0.1, 1.0)),
               # the same two steps with the reference's modules in float64 (net.double(), float64 batch): the arbiter between two
               # fp32 implementations of an ill-conditioned step (VERDICT r03 next #1b) — full gradients
               "train_tiny_fp64": dict(H=32, W=64, S=3, planes=(8, 8), render_if=(True, True), seed=7, loss_weight=(0.1, 1.0), fp64=True),
               "train_small_fp64": dict(H=128, W=160, S=3, planes=(16, 8), render_if=(True, True), seed=8, loss_weight=(0.1, 1.0), fp64=True),
               # BASELINE config 5 at its REAL shape (dtu_pretrain.yaml: 512x640, planes 64,8, both levels, full-image rays):
               # sparse digests (every 97th element of every gradient + float64 norm), fp32 and fp64
               "train_full": dict(H=512, W=640, S=3, planes=(64, 8), render_if=(True, True), seed=9, loss_weight=(0.1, 1.0), sparse=True),
               "train_full_fp64": dict(H=512, W=640, S=3, planes=(64, 8), render_if=(True, True), seed=9, loss_weight=(0.1, 1.0), sparse=True,
                                       fp64=True, threads=8)}


def grad_digest(g: torch.Tensor, sparse: bool = False) -> dict:
    """The FULL gradient of every parameter (436,012 floats per case) + its float64 norm; sparse: every FULL_STRIDE-th element
    and max|.| instead of the full tensor (the full-size cases)."""
    f = g.detach().reshape(-1)
    d = {"norm": np.array(float(f.double().norm()))}
    if sparse:
        d["rows"] = f[::FULL_STRIDE].float().numpy().copy()
        d["absmax"] = np.array(float(f.abs().max()))
    else:
        d["full"] = f.float().numpy()          # (a float64 run is stored rounded to float32: 6e-8, far below what it arbitrates)
    return d


def run_train_case(case: str = "train_tiny") -> None:
    """One training step of the UNMODIFIED reference network (``.train()``: BN batch statistics, autograd) under the MSE
    part of lib/train/losses/enerf.py:21-24 (loss_weight from dtu_pretrain.yaml:43; the VGG perceptual term needs
    downloaded torchvision weights and is left out).  Writes tests/golden/train_tiny.npz: loss, outputs, parameter
    gradients (digests) and the updated BN running statistics."""
    from oracle.ref_loader import load_reference
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch

    c = TRAIN_CASES[case]
    opts = ["enerf.cas_config.volume_planes", ",".join(map(str, c["planes"])),
            "enerf.cas_config.render_if", ",".join(map(str, c["render_if"]))]
    cfg, ref_network = load_reference("configs/enerf/dtu_pretrain.yaml", opts)
    assert tuple(cfg.enerf.cas_config.loss_weight) == c["loss_weight"]
    import time
    torch.manual_seed(0)
    torch.set_num_threads(c.get("threads", 1))
    net = ref_network.Network()
    net.load_state_dict(seeded_state_dict(net))
    wnp = np.load(os.path.join(GOLDEN, "weights_seed0.npz"))
    assert all(np.array_equal(wnp[k], v.numpy()) for k, v in net.state_dict().items() if k in wnp.files)
    net.train()
    ecfg = EnerfConfig.from_yacs(cfg)
    b = make_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"], textured=True)
    rng = np.random.default_rng(c["seed"])
    for i in range(2):
        b[f"rgb_{i}"] = rng.uniform(0, 1, size=(1, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
    batch = {k: torch.from_numpy(v) for k, v in b.items()}
    if c.get("fp64"):                               # the SAME fp32 weights and inputs, every module and tensor in float64;
        net = net.double()                          # (the reference builds its sampling grids with the default dtype:
        torch.set_default_dtype(torch.float64)      #  linspace / create_meshgrid / ones — make that float64 too)
        batch = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
        import functools
        from lib.networks.enerf import utils as ref_utils
        ref_utils.create_meshgrid = functools.partial(ref_utils.create_meshgrid, dtype=torch.float64)   # (kornia's default is float32)
    t0 = time.perf_counter()
    out = net(batch)
    loss = sum(c["loss_weight"][i] * torch.nn.functional.mse_loss(batch[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
    loss.backward()
    dt = time.perf_counter() - t0
    sparse = bool(c.get("sparse"))
    save = {"loss": np.array(float(loss)), "meta/reference_cpu_seconds": np.array(dt), "meta/threads": np.array(c.get("threads", 1)),
            "meta/dtype": np.array("float64" if c.get("fp64") else "float32")}
    if sparse:
        for k, v in out.items():
            sparse_digest(f"out/{k}", v, save)
        save["meta/stride"] = np.array(FULL_STRIDE)
    else:
        save.update({f"out/{k}": v.detach().float().numpy() for k, v in out.items()})
        for i in range(2):
            save[f"in/rgb_{i}"] = b[f"rgb_{i}"]
    n_grad = 0
    for name, p_ in net.named_parameters():
        if p_.grad is None:
            save[f"nograd/{name}"] = np.array(1)
            continue
        n_grad += 1
        for k, v in grad_digest(p_.grad, sparse).items():
            save[f"grad/{name}/{k}"] = v
    for name, buf in net.named_buffers():
        if name.endswith("running_mean") or name.endswith("running_var"):
            save[f"buf/{name}"] = buf.numpy()
    save["meta/torch_version"] = np.array(torch.__version__)
    np.savez_compressed(os.path.join(GOLDEN, f"{case}.npz"), **save)
    print(f"[golden] {case}: loss {float(loss):.6f}; {n_grad} parameter gradients; {len(save)} arrays; forward+backward {dt:.1f} s "
          f"on {c.get('threads', 1)} thread(s), {'float64' if c.get('fp64') else 'float32'}")


# Multi-step training trajectories: N optimizer steps of the reference's trainer loop on a fixed SEQUENCE of
# batches (a different sample per step, like the data loader's), at two sizes.
TRAJ_CASES = {"train_traj_tiny": dict(H=32, W=64, S=3, planes=(8, 8), render_if=(True, True), seed=50, steps=10, loss_weight=(0.1, 1.0)),
              "train_traj_small": dict(H=64, W=96, S=3, planes=(16, 8), render_if=(True, True), seed=70, steps=10, loss_weight=(0.1, 1.0))}


def traj_batch(c: dict, ecfg, step: int) -> dict:
    """Batch `step` of a trajectory case (numpy): seed = case seed + step; target colours for both levels."""
    from enerf_amd.synth import make_batch
    b = make_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"] + step, textured=True)
    rng = np.random.default_rng(c["seed"] + step)
    for i in range(2):
        b[f"rgb_{i}"] = rng.uniform(0, 1, size=(1, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
    return b


def run_traj_case(case: str) -> None:
    """`steps` iterations of the UNMODIFIED reference's training loop (lib/train/trainers/trainer.py:44-63: forward in .train(),
    loss, optimizer.zero_grad(), backward, clip_grad_value_(40), optimizer.step()) with the optimizer the reference builds
    (lib/train/optimizer.py make_optimizer: Adam, lr 5e-4, eps 1e-8, weight_decay 0 from dtu_pretrain.yaml) and the MSE part of
    lib/train/losses/enerf.py:21-24.  Records the loss of every step, the final BatchNorm running statistics, the float64
    norm of every final parameter, and the eval-mode frame of the FINAL network on a held-out batch."""
    from oracle.ref_loader import load_reference
    from enerf_amd.config import EnerfConfig

    c = TRAJ_CASES[case]
    opts = ["enerf.cas_config.volume_planes", ",".join(map(str, c["planes"])),
            "enerf.cas_config.render_if", ",".join(map(str, c["render_if"]))]
    cfg, ref_network = load_reference("configs/enerf/dtu_pretrain.yaml", opts)
    # the reference's own optimizer factory, loaded from its FILE: `import lib.train` pulls the trainer, whose data utilities need
    # imgaug / cv2 (absent here); optimizer.py itself only needs torch and the reference's RAdam
    import importlib.util
    spec = importlib.util.spec_from_file_location("ref_train_optimizer", "/root/reference/lib/train/optimizer.py")
    ref_opt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_opt)
    make_optimizer = ref_opt.make_optimizer
    import time
    torch.set_num_threads(1)
    ecfg = EnerfConfig.from_yacs(cfg)

    def trajectory(draw: int):
        """draw 0: the trajectory itself; draw k > 0: the SAME loop with every batch's source images perturbed by one ulp
        (x (1 +- 6e-8), seeded) — how far the REFERENCE's trajectory moves under a perturbation below its input precision."""
        torch.manual_seed(0)
        net = ref_network.Network()
        net.load_state_dict(seeded_state_dict(net))
        net.train()
        optimizer = make_optimizer(cfg, net)
        assert type(optimizer).__name__ == "Adam" and float(cfg.train.lr) == 5e-4
        gen = torch.Generator().manual_seed(draw)
        losses = []
        for step in range(c["steps"]):
            batch = {k: torch.from_numpy(v) for k, v in traj_batch(c, ecfg, step).items()}
            if draw:
                sign = torch.randint(0, 2, batch["src_inps"].shape, generator=gen).float() * 2 - 1
                batch["src_inps"] = batch["src_inps"] * (1 + 6e-8 * sign)
            out = net(batch)
            loss = sum(c["loss_weight"][i] * torch.nn.functional.mse_loss(batch[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
            optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_value_(net.parameters(), 40)
            optimizer.step()
            losses.append(float(loss.detach()))
        pn = {name: float(p_.detach().double().norm()) for name, p_ in net.named_parameters()}
        bufs = {name: buf.numpy().copy() for name, buf in net.named_buffers()
                if name.endswith("running_mean") or name.endswith("running_var") or name.endswith("num_batches_tracked")}
        net.eval()
        with torch.no_grad():
            held = {k: torch.from_numpy(v) for k, v in traj_batch(c, ecfg, 1000).items()}
            ev = {k: v.float().numpy() for k, v in net(held).items()}
        return losses, pn, bufs, ev, optimizer

    t0 = time.perf_counter()
    losses, pn, bufs, ev, optimizer = trajectory(0)
    dt = time.perf_counter() - t0
    save = {"loss": np.array(losses), "meta/steps": np.array(c["steps"]), "meta/reference_cpu_seconds": np.array(dt),
            "meta/optimizer": np.array(f"{type(optimizer).__name__}(lr={cfg.train.lr}, eps={cfg.train.eps}, weight_decay={cfg.train.weight_decay})"),
            "meta/torch_version": np.array(torch.__version__)}
    save.update({f"pnorm/{k}": np.array(v) for k, v in pn.items()})
    save.update({f"buf/{k}": v for k, v in bufs.items()})
    save.update({f"eval/{k}": v for k, v in ev.items()})
    # the reference against ITSELF: per-step loss deviation, final parameter-norm / BatchNorm-statistics / eval-frame deviation of
    # NOISE_DRAWS one-ulp draws (the yardstick of tests/test_training.py's trajectory criterion)
    NOISE_DRAWS = 6
    nl, npn, nbuf, nev = [], [], [], []
    for k in range(1, NOISE_DRAWS + 1):
        l2, pn2, b2, ev2, _ = trajectory(k)
        nl.append([abs(a - b) / b for a, b in zip(l2, losses)])
        npn.append(max(abs(pn2[n] - pn[n]) / max(pn[n], 1e-6) for n in pn))
        nbuf.append(max(float(np.abs(b2[n] - bufs[n]).max() / max(np.abs(bufs[n]).max(), 1e-12)) for n in bufs if bufs[n].dtype.kind == "f"))
        nev.append({kk: float(np.abs(ev2[kk] - ev[kk]).max() / max(np.abs(ev[kk]).max(), 1e-12)) for kk in ev})
    save["noise/loss_rel"] = np.array(nl)                                  # (draws, steps)
    save["noise/pnorm_rel"] = np.array(npn)
    save["noise/buf_rel"] = np.array(nbuf)
    for kk in ev:
        save[f"noise/eval/{kk}"] = np.array([d[kk] for d in nev])
    print(f"[golden] {case}: reference vs itself under 1-ulp inputs: worst loss deviation per step {np.array(nl).max(0).round(6).tolist()}; "
          f"pnorm {max(npn):.2e}; BN statistics {max(nbuf):.2e}; eval frame {({kk: round(max(d[kk] for d in nev), 5) for kk in ev})}")
    np.savez_compressed(os.path.join(GOLDEN, f"{case}.npz"), **save)
    print(f"[golden] {case}: {c['steps']} steps in {dt:.1f} s; loss {losses[0]:.6f} -> {losses[-1]:.6f}: {[round(l, 6) for l in losses]}")


NOISE_CASES = {"train_small_noise": dict(base="train_small", draws=8, threads=1), "train_full_noise": dict(base="train_full", draws=6, threads=8)}


def run_noise_case(case: str) -> None:
    """The reference's OWN fp32 noise level on a training fixture: ``draws`` more steps of the unmodified reference network with
    the source images perturbed by ONE ULP (x (1 +- 6e-8), seeded signs) — each an equally valid fp32 evaluation of the same
    problem — and, per parameter, the largest distance of those gradients to the float64 step (``<base>_fp64.npz``).  The step's
    gradients are discontinuous in its inputs (ReLU masks under BatchNorm batch statistics, floor() of sample positions): single
    draws jump by 10-70x on dozens of parameters, which is what the arbitration tests calibrate their outlier bounds on."""
    from oracle.ref_loader import load_reference
    from enerf_amd.config import EnerfConfig
    from enerf_amd.synth import make_batch
    nc = NOISE_CASES[case]
    c = TRAIN_CASES[nc["base"]]
    sparse = bool(c.get("sparse"))
    opts = ["enerf.cas_config.volume_planes", ",".join(map(str, c["planes"])), "enerf.cas_config.render_if", ",".join(map(str, c["render_if"]))]
    cfg, ref_network = load_reference("configs/enerf/dtu_pretrain.yaml", opts)
    g32 = np.load(os.path.join(GOLDEN, nc["base"] + ".npz"))
    g64 = np.load(os.path.join(GOLDEN, nc["base"] + "_fp64.npz"))
    key = "rows" if sparse else "full"
    torch.set_num_threads(nc["threads"])
    ecfg = EnerfConfig.from_yacs(cfg)
    b = make_batch(c["H"], c["W"], c["S"], ecfg, seed=c["seed"], textured=True)
    rng = np.random.default_rng(c["seed"])
    for i in range(2):
        b[f"rgb_{i}"] = rng.uniform(0, 1, size=(1, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
    base = {k: torch.from_numpy(v) for k, v in b.items()}
    names = [k[5:-(len(key) + 1)] for k in g64.files if k.startswith("grad/") and k.endswith("/" + key)]
    scale = {n: (float(g64[f"grad/{n}/absmax"]) if sparse else float(np.abs(g64[f"grad/{n}/{key}"]).max())) for n in names}
    names = [n for n in names if scale[n] >= 1e-9]
    single = {n: float(np.abs(g32[f"grad/{n}/{key}"].astype(np.float64) - g64[f"grad/{n}/{key}"]).max() / scale[n]) for n in names}
    floor = float(np.median(list(single.values())))
    noise = {n: 0.0 for n in names}
    counts, worst = [], []
    for k in range(1, nc["draws"] + 1):
        gen = torch.Generator().manual_seed(k)
        batch = dict(base)
        sign = torch.randint(0, 2, base["src_inps"].shape, generator=gen).float() * 2 - 1
        batch["src_inps"] = base["src_inps"] * (1 + 6e-8 * sign)
        torch.manual_seed(0)
        net = ref_network.Network()
        net.load_state_dict(seeded_state_dict(net))
        net.train()
        out = net(batch)
        loss = sum(c["loss_weight"][i] * torch.nn.functional.mse_loss(batch[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
        loss.backward()
        grads = dict(net.named_parameters())
        d = {}
        for n in names:
            f = grads[n].grad.detach().reshape(-1).double().numpy()
            f = f[::FULL_STRIDE] if sparse else f
            d[n] = float(np.abs(f - g64[f"grad/{n}/{key}"]).max() / scale[n])
            noise[n] = max(noise[n], d[n])
        viol = [d[n] / max(single[n], floor) for n in names if d[n] > 3 * max(single[n], floor)]
        counts.append(len(viol))
        worst.append(max(viol) if viol else 0.0)
        print(f"[golden] {case} draw {k}: median {np.median(list(d.values())):.2e} max {max(d.values()):.2e}; parameters beyond 3x their "
              f"single-draw distance: {len(viol)} (worst {worst[-1]:.1f}x)", flush=True)
    save = {f"noise/{n}": np.array(v) for n, v in noise.items()}
    save.update({"meta/draw_outliers": np.array(counts), "meta/draw_worst_ratio": np.array(worst), "meta/draws": np.array(nc["draws"]),
                 "meta/perturbation": np.array("src_inps * (1 +- 6e-8), seeded signs (torch.Generator seeds 1..draws)"),
                 "meta/threads": np.array(nc["threads"]), "meta/torch_version": np.array(torch.__version__)})
    np.savez_compressed(os.path.join(GOLDEN, f"{case}.npz"), **save)
    print(f"[golden] {case}: outliers per draw {counts}; noise max {max(noise.values()):.2e}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default=None)
    a = ap.parse_args()
    os.makedirs(GOLDEN, exist_ok=True)
    if a.case in NOISE_CASES:
        run_noise_case(a.case)
        return
    if a.case in TRAIN_CASES:
        run_train_case(a.case)
        return
    if a.case in TRAJ_CASES:
        run_traj_case(a.case)
        return
    if a.case in FULL_CASES:
        run_full_case(a.case)
        return
    if a.case:
        run_case(a.case)
        return
    wpath = os.path.join(GOLDEN, "weights_seed0.npz")
    if os.path.exists(wpath):
        os.remove(wpath)
    for name in list(CASES) + list(TRAIN_CASES) + list(TRAJ_CASES) + list(FULL_CASES) + list(NOISE_CASES):
        subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], check=True, cwd=ROOT)


if __name__ == "__main__":
    main()
