"""Shared helpers: golden-case registry, batch/config/weights loading (tests only)."""
from __future__ import annotations

import os

import numpy as np
import torch

from enerf_amd.config import EnerfConfig
from enerf_amd.synth import make_batch, make_lego_batch, make_zju_batch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# cas_config of configs/enerf/dtu_pretrain_nocascade.yaml (volume_planes / render_if come from the case)
NOCASCADE_CAS = dict(num=1, depth_inv=(True,), volume_scale=(0.25,), im_feat_scale=(0.25,), im_ibr_scale=(1.0,), render_scale=(1.0,),
                     render_im_feat_level=(2,), nerf_model_feat_ch=(8,), num_samples=(2,))

# must mirror oracle/make_golden.py::CASES (the generator is the source of truth)
CASES = {
    "tiny_s3": dict(H=32, W=64, S=3, planes=(8, 8), render_if=(True, True), seed=1, textured=False, human=False),
    "tiny_s2": dict(H=32, W=64, S=2, planes=(8, 8), render_if=(True, True), seed=2, textured=True, human=False),
    "tiny_s4_mask": dict(H=32, W=64, S=4, planes=(8, 8), render_if=(False, True), seed=3, textured=True, human=True),
    "small_s3_eval": dict(H=64, W=96, S=3, planes=(16, 8), render_if=(False, True), seed=4, textured=True, human=False),
    "lego_small": dict(H=64, W=64, S=4, planes=(64, 8), render_if=(True, True), seed=5, human=False, rig="lego"),
    "zju_small": dict(H=64, W=64, S=4, planes=(32, 8), render_if=(False, True), seed=6, human=True, rig="zju"),
    # configs/enerf/llff_eval.yaml (planes 32,8; 640x960) at 1/5 size (2:3 aspect, level-0 volume 32 x 16 x 24)
    "llff_small": dict(H=128, W=192, S=3, planes=(32, 8), render_if=(False, True), seed=7, textured=True, human=False),
    # configs/enerf/dtu_pretrain_nocascade.yaml: its one-level cas_config as shipped, volume_planes 8 instead of 48
    "nocascade_tiny": dict(H=32, W=64, S=3, planes=(8,), render_if=(True,), seed=8, textured=True, human=False,
                           cas=NOCASCADE_CAS, weights="nocascade"),
    # configs/enerf/enerf_outdoor/actor1.yaml: viewdir_agg False, num_samples (2, 1), volume_planes (32, 8), both levels rendered
    # (through the plain network: network_composite and its layered foreground are out of scope)
    "outdoor_tiny": dict(H=32, W=64, S=3, planes=(32, 8), render_if=(True, True), seed=9, textured=True, human=False,
                         cas=dict(num_samples=(2, 1)), viewdir_agg=False, weights="outdoor"),
}


def case_config(name: str) -> EnerfConfig:
    c = CASES[name]
    cfg = EnerfConfig(viewdir_agg=c.get("viewdir_agg", True))
    return cfg.with_cas(**c.get("cas", {})).with_cas(volume_planes=c["planes"], render_if=c["render_if"])


def case_batch(name: str, as_torch: bool = True) -> dict:
    c = CASES[name]
    if c.get("rig") == "lego":
        b = make_lego_batch(c["H"], c["W"], c["S"], case_config(name), seed=c["seed"])
    elif c.get("rig") == "zju":
        b = make_zju_batch(c["H"], c["W"], c["S"], case_config(name), seed=c["seed"])
    else:
        b = make_batch(c["H"], c["W"], c["S"], case_config(name), seed=c["seed"], textured=c["textured"],
                       mask_box=c["human"])
    return {k: torch.from_numpy(v) for k, v in b.items()} if as_torch else b


# The networks of two cases do not take weights_seed0 as it is.  Their state dicts are subsets of it, so instead of storing
# the same arrays twice more (about 1.5 MB each) a case names how its state dict derives from weights_seed0; the generator
# asserts that the derived keys are exactly the reference network's (BatchNorm's batch counters aside) before it loads them.
#   nocascade: one level whose NeRF has 8 feature channels -> that level takes the stored nerf_1 (8 channels); level 1 goes
#   outdoor:   viewdir_agg False -> Agg has no view_fc
WEIGHT_RULES = {"nocascade": dict(drop=("nerf_0.", "cost_reg_1."), rename={"nerf_1.": "nerf_0."}),
                "outdoor": dict(drop=("nerf_0.agg.view_fc.", "nerf_1.agg.view_fc."), rename={})}


def derive_weights(sd: dict, rule: str) -> dict:
    r = WEIGHT_RULES[rule]
    out = {}
    for k, v in sd.items():
        if k.startswith(r["drop"]):
            continue
        for a, b in r["rename"].items():
            if k.startswith(a):
                k = b + k[len(a):]
        out[k] = v
    return out


def load_weights(name: str | None = None) -> dict:
    """The reference state dict of golden case ``name`` (None, or a case of the default networks: weights_seed0)."""
    z = np.load(os.path.join(GOLDEN, "weights_seed0.npz"))
    sd = {k: torch.from_numpy(z[k]) for k in z.files}
    rule = CASES[name].get("weights") if name is not None else None
    return derive_weights(sd, rule) if rule else sd


def load_golden(name: str) -> dict:
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return {k: z[k] for k in z.files}


# ---- full-size frames pinned to the reference itself (oracle/make_golden.py::FULL_CASES; sparse digests, < 1 MB each) ----
FULL_CASES = {
    "dtu_full": dict(H=512, W=640, S=3, planes=(48, 8), render_if=(False, True), seed=0, textured=True, human=False),
    # BASELINE configs[0] (configs/enerf/dtu/scan114.yaml shape): 512x640, 3 views, planes 48,8, BOTH levels rendered
    "dtu_full_tt": dict(H=512, W=640, S=3, planes=(48, 8), render_if=(True, True), seed=0, textured=True, human=False),
    "lego_full": dict(H=800, W=800, S=4, planes=(64, 8), render_if=(True, True), seed=5, human=False, rig="lego"),
    "zju_full": dict(H=1024, W=1024, S=4, planes=(32, 8), render_if=(False, True), seed=6, human=True, rig="zju"),
    # configs/enerf/llff_eval.yaml at its own size (the reference's fourth eval config; not a BASELINE config)
    "llff_full": dict(H=640, W=960, S=3, planes=(32, 8), render_if=(False, True), seed=7, textured=True, human=False),
}


def full_case_config(name: str) -> EnerfConfig:
    c = FULL_CASES[name]
    return EnerfConfig().with_cas(volume_planes=c["planes"], render_if=c["render_if"])


def full_case_batch(name: str) -> dict:
    c = FULL_CASES[name]
    cfg = full_case_config(name)
    if c.get("rig") == "lego":
        return make_lego_batch(c["H"], c["W"], c["S"], cfg, seed=c["seed"])
    if c.get("rig") == "zju":
        return make_zju_batch(c["H"], c["W"], c["S"], cfg, seed=c["seed"])
    return make_batch(c["H"], c["W"], c["S"], cfg, seed=c["seed"], textured=c["textured"])


def check_sparse_golden(name: str, out: dict, rel_tol: float, mids: dict | None = None) -> dict:
    """Compare full-size outputs (torch tensors or arrays) with the reference's sparse digest: the stored rows
    (every ``meta/stride``-th ray / pixel) within rel_tol of max|ref|, and the whole-tensor L2 norm and sum.
    Returns {key: worst relative error} for reporting."""
    g = load_golden(name)
    stride = int(g["meta/stride"])
    keys = sorted({k.split("/")[1] for k in g if k.startswith("out/")})
    assert sorted(out) == keys, (sorted(out), keys)
    worst = {}
    groups = [("out", out)] + ([("mid", mids)] if mids else [])
    for grp, tensors in groups:
        for k in sorted({k.split("/")[1] for k in g if k.startswith(grp + "/")}):
            if k not in tensors:
                continue
            a = tensors[k]
            a = np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)
            pre = f"{grp}/{k}"
            if grp == "out":
                assert tuple(a.shape) == tuple(g[pre + "/shape"]), (k, a.shape, g[pre + "/shape"])
            ref_rows = g[pre + "/rows"]
            rows = a.reshape(-1, ref_rows.shape[1])[::stride]
            scale = max(float(g[pre + "/absmax"]), 1e-12)
            err = float(np.abs(rows.astype(np.float64) - ref_rows).max()) / scale
            f = a.astype(np.float64).reshape(-1)
            nerr = abs(float(np.sqrt((f * f).sum())) - float(g[pre + "/norm"])) / max(float(g[pre + "/norm"]), 1e-12)
            assert err < rel_tol, (name, k, "rows", err)
            assert nerr < rel_tol, (name, k, "norm", nerr)
            worst[k] = max(err, nerr)
    return worst
