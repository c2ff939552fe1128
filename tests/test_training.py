"""Training path (BASELINE config 5): ``Network.train()`` + autograd + DDP.

PINNED to the reference: tests/golden/train_tiny.npz holds one training step of the unmodified reference network
(``.train()``: BatchNorm batch statistics) under the MSE part of lib/train/losses/enerf.py:21-24 — loss, outputs, the
gradient of every parameter (digests) and the updated BN running statistics (oracle/make_golden.py --case train_tiny)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from enerf_amd.config import EnerfConfig
from enerf_amd.network import Network
from enerf_amd.synth import make_batch
from golden_cases import GOLDEN, load_weights

HERE = os.path.dirname(os.path.abspath(__file__))
LOSS_W = (0.1, 1.0)                                   # configs/enerf/dtu_pretrain.yaml:43
# reference-generated training fixtures (oracle/make_golden.py::TRAIN_CASES): FULL gradients of all 115 parameters
TRAIN_CASES = {"train_tiny": dict(seed=7, H=32, W=64, planes=(8, 8)), "train_small": dict(seed=8, H=128, W=160, planes=(16, 8))}
FULL_TRAIN_CASE = dict(seed=9, H=512, W=640, planes=(64, 8))        # train_full / train_full_fp64: sparse digests (every 97th element)


def _grad_errors(named_grads, g):
    """{name: max|grad - ref| / max|ref|} against the FULL reference gradients of a training fixture (no digests)."""
    errs = {}
    for name, grad in named_grads:
        key = f"grad/{name}/full"
        assert key in g.files or f"nograd/{name}" in g.files, f"{name}: the fixture must hold every parameter's full gradient"
        if key in g.files:
            ref = g[key]
            f = grad.detach().reshape(-1).cpu().numpy()
            # 1e-8 absolute floor: nerf_*.agg.agg_w_fc.0.bias feeds a softmax over views (shift invariant), its true gradient
            # is zero and the reference value is rounding noise of the order 1e-10
            errs[name] = float(max(np.abs(f - ref).max() - 1e-8, 0.0) / max(np.abs(ref).max(), 1e-30))
    return errs


def _distance_to_fp64(named_grads, g32, g64, sparse=False):
    """Per parameter: (d_ours, d_ref) = max|. - fp64| / max|fp64| of OUR fp32 gradient and of the REFERENCE's fp32 gradient, against
    the reference's own modules run in float64 on the same weights and inputs (oracle/make_golden.py --case *_fp64).  ``sparse``:
    the full-size fixtures hold every 97th element (+ max|.|).  Parameters whose float64 gradient is numerically zero (the
    shift-invariant agg_w_fc bias) are skipped."""
    key, out = ("rows" if sparse else "full"), {}
    for name, grad in named_grads:
        k = f"grad/{name}/{key}"
        if k not in g64.files:
            continue
        r64 = g64[k].astype(np.float64)
        scale = float(g64[f"grad/{name}/absmax"]) if sparse else float(np.abs(r64).max())
        if scale < 1e-9:
            continue
        f = grad.detach().reshape(-1).cpu().numpy().astype(np.float64)
        f = f[::97] if sparse else f
        out[name] = (float(np.abs(f - r64).max() / scale), float(np.abs(g32[k].astype(np.float64) - r64).max() / scale))
    return out


def _assert_as_close_to_fp64_as_the_reference(dist, noise=None, slack=3.0, what=""):
    """VERDICT r03 next #1b.  The step is ill-conditioned — worse, DISCONTINUOUS in its inputs (ReLU masks under BatchNorm batch
    statistics, floor() of bilinear sample positions): two fp32 evaluations differ by far more than fp32 epsilon, so 'equal to
    the reference's fp32 gradients' is the wrong bar.  The right one: our fp32 result is (within ``slack``) as close to the
    float64 result as the reference's fp32 result is.  ``noise`` (tests/golden/train_*_noise.npz, oracle/make_golden.py
    run_noise_case) calibrates what 'the reference's fp32 result' means per parameter: the UNMODIFIED reference re-run with its
    input images perturbed by ONE ULP lands, in 2 of 8 draws at 128x160, 10-70x further from float64 on 37-56 of its 114
    parameters (one flipped mask / floor moves a BatchNorm-bias-like gradient by a whole term).  Hence:
      * bulk: median and 75th percentile of our distances <= slack x the reference's (robust to such jumps);
      * per parameter, NO exceptions (round 5, ADVICE r04: the round-4 form let up to `max draw_outliers` parameters — 56 of 114 at
        128x160 — go anywhere below a global ceiling): ours <= slack x max(reference single draw, the worst of the reference's
        own 1-ulp draws FOR THAT PARAMETER, median reference distance), and a hard cap of 1.5e-1 on every parameter;
      * how many parameters leave the reference's SINGLE draw by more than slack is bounded by what the reference's MEDIAN 1-ulp
        draw does to itself (not its worst draw), with a small allowance for the draws whose median is zero."""
    names = list(dist)
    ours = np.array([dist[n][0] for n in names])
    ref = np.array([dist[n][1] for n in names])
    floor = float(np.median(ref))
    if noise is None:
        per_param, allowed, ceiling = ref, 0, float(ref.max())
    else:
        per_param = np.maximum(ref, np.array([float(noise[f"noise/{n}"]) if f"noise/{n}" in noise.files else 0.0 for n in names]))
        allowed, ceiling = int(noise["meta/draw_outliers"].max()), float(per_param.max())
    outliers = {n: dist[n] for i, n in enumerate(names) if ours[i] > slack * max(per_param[i], floor)}
    assert len(dist) >= 105 and not outliers, (what, floor, outliers)                       # per parameter, its OWN noise: no exceptions
    assert float(ours.max()) <= 1.5e-1, (what, float(ours.max()))                            # hard cap (the old element-wise bound)
    beyond_single = [n for i, n in enumerate(names) if ours[i] > slack * max(ref[i], floor)]
    if noise is not None:
        allowed = int(np.median(noise["meta/draw_outliers"])) + 5
    assert len(beyond_single) <= allowed, (what, allowed, {n: dist[n] for n in beyond_single})
    stats = dict(median=(float(np.median(ours)), floor), p75=(float(np.percentile(ours, 75)), float(np.percentile(ref, 75))),
                 max=(float(ours.max()), ceiling), outliers=(len(outliers), 0), beyond_single_draw=(len(beyond_single), allowed))
    assert stats["median"][0] <= slack * stats["median"][1] and stats["p75"][0] <= slack * stats["p75"][1], (what, stats)
    assert stats["max"][0] <= slack * ceiling, (what, stats, outliers)
    return stats


def _assert_stable_parameters_elementwise(named_grads, g32, g64, noise, sparse, tol=3e-4, what=""):
    """VERDICT r05 #6c.  The fp64 arbitration above is a STATISTICAL bar; where the reference is demonstrably stable it is not
    needed.  A parameter is 'stable' when the unmodified reference, re-run with its inputs moved by one ulp, stays within 1e-4 of
    float64 in EVERY draw (tests/golden/train_*_noise.npz) and its pinned fp32 gradient does too.  For those — 30 of 114 at
    512x640: every MLP layer of level 1, most of level 0's, the FeatureNet's lateral / smooth0 layers, the level-1 heads — our
    gradient is compared ELEMENT-WISE with the reference's fp32 gradient: max|ours - ref| <= tol x max|ref| (3e-4: both sit within
    1e-4 of float64, plus fp32 summation order).  Returns the names it covered."""
    key, covered = ("rows" if sparse else "full"), []
    for name, grad in named_grads:
        k, nk = f"grad/{name}/{key}", f"noise/{name}"
        if k not in g32.files or k not in g64.files or nk not in noise.files:
            continue
        r64, r32 = g64[k].astype(np.float64), g32[k].astype(np.float64)
        scale = float(g64[f"grad/{name}/absmax"]) if sparse else float(np.abs(r64).max())
        if scale < 1e-9 or float(noise[nk]) >= 1e-4 or float(np.abs(r32 - r64).max() / scale) >= 1e-4:
            continue
        f = grad.detach().reshape(-1).cpu().numpy().astype(np.float64)
        f = f[::97] if sparse else f
        err = float(np.abs(f - r32).max() / scale)
        assert err <= tol, (what, name, err)
        covered.append(name)
    return covered


def _train_batch(seed=7, H=32, W=64, S=3, planes=(8, 8)):
    cfg = EnerfConfig().with_cas(volume_planes=planes, render_if=(True, True))
    b = make_batch(H, W, S, cfg, seed=seed, textured=True)
    rng = np.random.default_rng(seed)
    for i in range(2):
        b[f"rgb_{i}"] = rng.uniform(0, 1, size=(1, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
    return cfg, {k: torch.from_numpy(v) for k, v in b.items()}


def _loss(out, batch):                                # losses/enerf.py:21-24
    return sum(LOSS_W[i] * F.mse_loss(batch[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))


def _net(cfg, twins=False):
    """twins=True: every stage of the training forward through its torch-op twin (tests/torch_twins.py) — the reference's own
    ops on CPU tensors; the product path has no eager fallback and raises without the library."""
    net = Network(cfg)
    net.load_state_dict(load_weights(), strict=False)
    if twins:
        import torch_twins
        torch_twins.install(net)
    return net.train()


def test_training_forward_without_the_library_raises():
    """no eager fallback in the product — CPU tensors and no injected emulator library = an error naming the
    first stage, not a silent PyTorch forward; the torch twins are test infrastructure (tests/torch_twins.py)."""
    cfg, batch = _train_batch()
    net = _net(cfg)
    with pytest.raises(RuntimeError, match="HIP library is required"):
        net(batch)
    import enerf_amd.train_path as TP
    for name in ("depth_values", "proj_mats", "feature_volume", "depth_regression", "build_rays", "sample_along_depth", "img_feat",
                 "raw2outputs", "agg_forward", "nerf_forward"):
        assert not hasattr(TP, name), f"torch twin {name} is back in the product package"


@pytest.mark.parametrize("case", list(TRAIN_CASES))
def test_training_step_matches_reference_gradients(case):
    g = np.load(os.path.join(GOLDEN, f"{case}.npz"))
    assert not [k for k in g.files if k.endswith("/head") or k.endswith("/tail")], "norm-only / digest gradients are gone"
    cfg, batch = _train_batch(**TRAIN_CASES[case])
    for i in range(2):
        assert np.array_equal(batch[f"rgb_{i}"].numpy(), g[f"in/rgb_{i}"])
    torch.set_num_threads(1)
    net = _net(cfg, twins=True)
    out = net(batch)
    loss = _loss(out, batch)
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-5)
    for k in [k[4:] for k in g.files if k.startswith("out/")]:
        np.testing.assert_allclose(out[k].detach().numpy(), g["out/" + k], rtol=2e-4, atol=2e-5, err_msg=k)
    loss.backward()
    checked = 0
    for name, p in net.named_parameters():
        if f"nograd/{name}" in g.files:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        f = p.grad.reshape(-1)
        scale = max(float(f.abs().max()), 1e-12)
        ref = g[f"grad/{name}/full"]                                       # every element of every parameter gradient
        assert np.abs(f.numpy() - ref).max() <= 2e-4 * max(scale, np.abs(ref).max()) + 1e-9, name
        checked += 1
    assert checked == 115 - len([k for k in g.files if k.startswith("nograd/")])
    # BatchNorm running statistics were updated like the reference's (momentum 0.1, unbiased variance)
    for name, buf in net.named_buffers():
        if f"buf/{name}" in g.files:
            np.testing.assert_allclose(buf.numpy(), g[f"buf/{name}"], rtol=1e-4, atol=1e-6, err_msg=name)


def test_hip_training_step_is_as_close_to_fp64_as_the_reference_emulated():
    """The fp64 arbitration on the lane emulator at 32x64 (the 128x160 and 512x640 steps run on the GPU: -m gpu)."""
    from emu_lib import emu_lib
    g32, g64 = np.load(os.path.join(GOLDEN, "train_tiny.npz")), np.load(os.path.join(GOLDEN, "train_tiny_fp64.npz"))
    cfg, batch = _train_batch(**TRAIN_CASES["train_tiny"])
    net = Network(cfg, lib=emu_lib())
    net.load_state_dict(load_weights(), strict=False)
    net.train()
    _loss(net(batch), batch).backward()
    dist = _distance_to_fp64([(n, p.grad) for n, p in net.named_parameters() if p.grad is not None], g32, g64)
    st = _assert_as_close_to_fp64_as_the_reference(dist, what="32x64 emulator")     # (no noise fixture needed at this size: every
    assert st["median"][0] < 1e-4                                       #  parameter within 3x; measured median 2.1e-5 vs 2.9e-5)


def test_reference_gradients_jump_under_one_ulp_input_perturbations():
    """The calibration behind the arbitration bounds, read from the fixtures (generated by the UNMODIFIED reference,
    oracle/make_golden.py run_noise_case): with the source images perturbed by one ulp, some draws put dozens of parameters
    10x-70x further from the float64 step than the unperturbed fp32 draw — the gradients are discontinuous in the inputs."""
    for name in ("train_small_noise", "train_full_noise"):
        nz = np.load(os.path.join(GOLDEN, name + ".npz"))
        counts, worst = nz["meta/draw_outliers"], nz["meta/draw_worst_ratio"]
        assert len(counts) == int(nz["meta/draws"]) >= 6
        assert counts.max() >= 5 and worst.max() >= 4.0, (name, counts, worst)
    nz = np.load(os.path.join(GOLDEN, "train_small_noise.npz"))
    assert nz["meta/draw_outliers"].max() >= 30 and (nz["meta/draw_outliers"] == 0).sum() >= 4      # all-or-nothing jumps at 128x160


def test_mid_size_step_is_ill_conditioned_in_the_reference():
    """Why the 128x160 fixture cannot carry the 5e-4 bound of the 32x64 one: the reference's OWN gradients (torch-op path = the
    reference's ops; bit-identical forward) are not reproducible beyond ~1e-3 at this size.  A 1e-6 relative perturbation of the
    cost volume — smaller than the difference between two fp32 summation orders of the warp — moves some parameter gradients
    by more than 1e-3 of their largest element."""
    import torch_twins as T
    g = np.load(os.path.join(GOLDEN, "train_small.npz"))
    cfg, batch = _train_batch(**TRAIN_CASES["train_small"])
    gen = torch.Generator().manual_seed(0)
    net = _net(cfg, twins=True)
    T.install(net, feature_volume=lambda f, P, dv: (lambda v: v * (1 + 1e-6 * (torch.rand(v.shape, generator=gen) * 2 - 1)))(T.feature_volume(f, P, dv)))
    _loss(net(batch), batch).backward()
    errs = _grad_errors([(n, p.grad) for n, p in net.named_parameters() if p.grad is not None], g)
    assert max(errs.values()) > 1e-3, max(errs.values())          # (measured 7e-3; with 1 vs 8 CPU threads alone: 1.8e-3)
    assert max(errs.values()) < 1.5e-1                             # (the element-wise bound round 3 needed at this size)
    # the same with the FeatureNet's three output maps perturbed by 1e-5 relative (two fp32 summation orders of its convolutions
    # differ by that much): the reference's own gradients move by > 1e-2 somewhere (measured: worst 1.0e-1, median 4.4e-3)
    gen2 = torch.Generator().manual_seed(0)
    net = _net(cfg, twins=True)
    T.install(net, feature_net=lambda m, x: tuple(v * (1 + 1e-5 * (torch.rand(v.shape, generator=gen2) * 2 - 1)) for v in T.feature_net_forward(m, x)))
    _loss(net(batch), batch).backward()
    errs = _grad_errors([(n, p.grad) for n, p in net.named_parameters() if p.grad is not None], g)
    assert max(errs.values()) > 1e-2, max(errs.values())


def _check_hip_backward_stages(lib, dev):
    """Every autograd.Function of enerf_amd/autograd.py (HIP forward + HIP backward through the C ABI) against the same
    stage in torch ops (tests/torch_twins.py), values and gradients."""
    # (One shape per stage against a float32 twin, hence the loose bounds: the tight check of these kernels — float64 reference, every
    # launcher branch, partial waves — is tests/test_backward_regimes.py.)
    import torch_twins as T
    from enerf_amd.autograd import CompositeFn, DepthRegressionFn, FeatureVolumeFn
    cfg, batch = _train_batch()
    batch = {k: v.to(dev) for k, v in batch.items()}
    cas = cfg.cas
    g = torch.Generator().manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    # --- warp + variance, both levels (C = 32 at 8x16 / C = 16 at 16x32 source maps) ---
    for level, (C, Hs, Ws, D) in enumerate(((32, 8, 16, 8), (16, 16, 32, 8))):
        feats = rnd(1, 3, C, Hs, Ws).requires_grad_(True)
        h, w = int(32 * cas.volume_scale[level]), int(64 * cas.volume_scale[level])
        dv0 = (torch.linspace(500.0, 800.0, D).view(1, D, 1, 1).expand(1, D, h, w) + 3.0 * torch.randn(1, D, h, w, generator=g)).to(dev)
        dv = dv0.clone().requires_grad_(True)
        P = T.proj_mats(batch, cas.im_feat_scale[level], cas.volume_scale[level])
        gout = rnd(1, C, D, h, w)
        ref = T.feature_volume(feats, P, dv)
        ref.backward(gout)
        gf_ref, gd_ref = feats.grad.clone(), dv.grad.clone()
        feats.grad = dv.grad = None
        out = FeatureVolumeFn.apply(lib, feats, P, dv)
        out.backward(gout)
        assert float((out - ref).abs().max()) <= 2e-5 * float(ref.abs().max())
        assert float((feats.grad - gf_ref).abs().max()) <= 1e-4 * float(gf_ref.abs().max()), level
        assert float((dv.grad - gd_ref).abs().max()) <= 2e-3 * float(gd_ref.abs().max()), level      # sums of +- terms
    # --- depth regression, disparity- and depth-space ---
    for level, inv in enumerate((True, False)):
        prob = rnd(1, 8, 6, 10).requires_grad_(True)
        dv = (500 + 300 * torch.rand(1, 8, 6, 10, generator=g)).to(dev).requires_grad_(True)
        gd, gs = rnd(1, 6, 10), rnd(1, 6, 10)
        c2 = cfg.with_cas(depth_inv=(inv, inv)).cas
        d_ref, s_ref = T.depth_regression(c2, prob, dv, 0)
        (d_ref * gd + s_ref * gs).sum().backward()
        gp_ref, gv_ref = prob.grad.clone(), dv.grad.clone()
        prob.grad = dv.grad = None
        d, s_ = DepthRegressionFn.apply(lib, prob, dv, inv)
        (d * gd + s_ * gs).sum().backward()
        assert float((d - d_ref).abs().max()) <= 1e-5 * float(d_ref.abs().max())
        assert float((prob.grad - gp_ref).abs().max()) <= 1e-4 * float(gp_ref.abs().max()), inv
        assert float((dv.grad - gv_ref).abs().max()) <= 1e-4 * float(gv_ref.abs().max()), inv
    # --- compositing ---
    for Ns in (2, 8):
        raw = torch.cat([torch.rand(2, 37, Ns, 3, generator=g), 2 * torch.rand(2, 37, Ns, 1, generator=g)], -1).to(dev).requires_grad_(True)
        z = (400 + 500 * torch.rand(2, 37, Ns, generator=g)).to(dev).requires_grad_(True)
        gr, gdp, gw = rnd(2, 37, 3), rnd(2, 37) * 1e-2, rnd(2, 37, Ns)
        # the reference's own expression (utils.py:584-603) under autograd, depth term included: z_vals is DETACHED in
        # depth_map = sum(weights * z_vals.detach()) (utils.py:595), so a loss on the composited depth reaches raw only
        alpha = 1.0 - torch.exp(-raw[..., 3])
        Tm = torch.cumprod(torch.cat([torch.ones_like(alpha[..., :1]), 1.0 - alpha + 1e-10], -1), -1)[..., :-1]
        w0 = alpha * Tm
        rgb_r = torch.sum(w0[..., None] * raw[..., :3], -2)
        w_r = torch.softmax(w0, -1)
        dep_r = torch.sum(w_r * z.detach(), -1)
        ((rgb_r * gr).sum() + (dep_r * gdp).sum() + (w_r * gw).sum()).backward()
        gr_ref = raw.grad.clone()
        assert z.grad is None
        raw.grad = None
        ref = T.raw2outputs(raw, z)                                    # the torch twin of the training path
        (ref["rgb"] * gr).sum().add((ref["depth"] * gdp).sum()).add((ref["weights"] * gw).sum()).backward()
        assert z.grad is None                                          # no gradient into the sample depths
        assert float((raw.grad - gr_ref).abs().max()) <= 1e-5 * float(gr_ref.abs().max()), Ns
        raw.grad = None
        rgb, depth, wts = CompositeFn.apply(lib, raw, z, False)
        ((rgb * gr).sum() + (depth * gdp).sum() + (wts * gw).sum()).backward()
        assert float((rgb - ref["rgb"]).abs().max()) < 1e-5 and float((wts - ref["weights"]).abs().max()) < 1e-5
        assert float((depth - dep_r).abs().max()) <= 1e-5 * float(dep_r.abs().max())
        assert float((raw.grad - gr_ref).abs().max()) <= 1e-4 * float(gr_ref.abs().max()), Ns
        assert z.grad is None

    # --- render-side fetches: get_img_feat + get_vox_feat (points in front of the cameras, some outside the images);
    #     two batch elements with different camera rigs ---
    from enerf_amd.autograd import GatherFn
    gather_cameras = T.gather_cameras
    _, batch_b = _train_batch(seed=11)
    batch1 = batch
    batch = {k: torch.cat([v, batch_b[k].to(dev)], 0) for k, v in batch1.items()}
    Bg = 2
    for level, (Fc, Ns) in enumerate(((35, 4), (11, 2))):
        rs = cas.render_scale[level]
        Hr, Wr = int(32 * rs), int(64 * rs)
        rays = batch[f"rays_{level}"][:, :200]
        N = rays.shape[1]
        o, d = rays[..., :3], rays[..., 3:6]
        t = (batch["near_far"].min() + (batch["near_far"].max() - batch["near_far"].min()) * torch.rand(Bg, N, Ns, generator=g).to(dev))
        side = (0.0 + 120.0 * torch.randn(Bg, N, Ns, 3, generator=g)).to(dev) * (torch.rand(Bg, N, Ns, 1, generator=g).to(dev) < 0.3)
        xyz = (o[:, :, None] + d[:, :, None] * t[..., None] + side).reshape(Bg, N * Ns, 3).requires_grad_(True)
        dn = (torch.rand(Bg, N * Ns, generator=g) * 1.3 - 0.15).to(dev).requires_grad_(True)
        uv = (torch.rand(Bg, N * Ns, 2, generator=g) * torch.tensor([Wr - 1.0, Hr - 1.0])).to(dev)
        tex = rnd(Bg, 3, Fc, Hr, Wr).requires_grad_(True)
        vol = rnd(Bg, 8, 8, int(32 * cas.volume_scale[level]), int(64 * cas.volume_scale[level])).requires_grad_(True)
        gx, gv = rnd(Bg, N * Ns, 3, Fc + 4), rnd(Bg, N * Ns, 8)

        def torch_twin():
            nd = torch.stack([uv[..., 0] / (Wr - 1), uv[..., 1] / (Hr - 1), dn], -1)
            gg = nd.reshape(Bg, 1, 1, N * Ns, 3) * 2.0 - 1.0
            vox = F.grid_sample(vol, gg, align_corners=True)[:, :, 0, 0].permute(0, 2, 1)
            return T.img_feat(cas, xyz.reshape(Bg, N, Ns, 3), tex, batch, level), vox
        x_ref, v_ref = torch_twin()
        ((x_ref * gx).sum() + (v_ref * gv).sum()).backward()
        ref = [t_.grad.clone() for t_ in (xyz, dn, tex, vol)]
        for t_ in (xyz, dn, tex, vol):
            t_.grad = None
        cam, tcen = gather_cameras(batch, rs)
        x, vox = GatherFn.apply(lib, xyz, dn, uv, tex.permute(0, 1, 3, 4, 2), vol.permute(0, 2, 3, 4, 1), cam, tcen)   # channels-last
        ((x * gx).sum() + (vox * gv).sum()).backward()
        assert float((x - x_ref).abs().max()) <= 2e-4 * float(x_ref.abs().max()), level
        assert float((vox - v_ref).abs().max()) <= 1e-5 * float(v_ref.abs().max()), level
        for name, t_, r in zip(("xyz", "dn", "tex", "vol"), (xyz, dn, tex, vol), ref):
            err, scale = float((t_.grad - r).abs().max()), float(r.abs().max())
            assert err <= (2e-3 if name == "xyz" else 2e-4) * scale, (level, name, err, scale)


def _check_conv_wgrad(lib, dev):
    """enerf_conv_wgrad against torch's own weight gradients for every convolution shape of the path (FeatureNet 2-D
    layers incl. the 5x5 stride-2 ones, the 3-D stride-1 / stride-2 / transposed layers, the width-1 depth head)."""
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g).to(dev)
    cases2d = [(3, 8, 3, 1, 1), (8, 16, 5, 2, 2), (16, 32, 5, 2, 2), (32, 32, 1, 1, 0), (32, 8, 3, 1, 1), (16, 16, 3, 1, 1)]
    for cin, cout, k, st, pad in cases2d:
        x = rnd(2, cin, 12, 20)
        w = rnd(cout, cin, k, k).requires_grad_(True)
        y = F.conv2d(x, w, None, st, pad)
        gy = rnd(*y.shape)
        (ref,) = torch.autograd.grad(y, w, gy)
        got = lib.conv_wgrad(gy, x, (k, k), st, (pad, pad))
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), (cin, cout, k, st)
    # the LDS-tiled 3x3 kernel of the <= 8-channel layers (k_wgrad2d_3x3_c8: >= 2048 positions): image edges inside a tile, a
    # partial last tile row / column, the row above the image, 16-byte and scalar staging (channel counts 8, 4, 5, 3), two and
    # four blocks of 8 input channels (smooth0: 32 -> 8)
    for cin, cout, H, W in [(8, 8, 40, 70), (3, 8, 33, 64), (8, 4, 47, 45), (5, 8, 9, 250), (8, 8, 64, 32), (32, 8, 40, 70), (16, 8, 17, 66),
                            (32, 5, 33, 40), (8, 8, 300, 7),                           # (an image narrower than a tile)
                            (16, 16, 40, 70), (32, 16, 33, 45), (32, 32, 17, 66)]:      # (the plain 16 / 32-channel tiles: conv1.1, smooth1, conv2.1)
        x = rnd(2, cin, H, W)
        w = rnd(cout, cin, 3, 3).requires_grad_(True)
        y = F.conv2d(x, w, None, 1, 1)
        gy = rnd(*y.shape)
        (ref,) = torch.autograd.grad(y, w, gy)
        got = lib.conv_wgrad(gy, x, (3, 3), 1, (1, 1))
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), (cin, cout, H, W, float((got - ref).abs().max() / ref.abs().max()))
        assert torch.equal(got, lib.conv_wgrad(gy, x, (3, 3), 1, (1, 1)))                       # deterministic
    # ... and its 3-D form (k_wgrad3d_c8: >= 32768 positions): conv0 (32 / 16 -> 8, two columns of 16 channels for 32), 8 -> 8, and the
    # fused heads 8 -> 16 (roles swapped, taps mirrored); volume borders in d, h and w inside tiles
    for cin, cout, D, H, W, nb in [(16, 8, 5, 81, 83, 1), (32, 8, 3, 100, 112, 1), (8, 16, 6, 70, 80, 1), (8, 8, 4, 96, 96, 1), (32, 5, 5, 81, 83, 1),
                                   (16, 8, 3, 80, 72, 2)]:                              # (the last: two volumes — planes of different volumes never mix)
        x = rnd(nb, cin, D, H, W)
        w = rnd(cout, cin, 3, 3, 3).requires_grad_(True)
        y = F.conv3d(x, w, None, 1, 1)
        gy = rnd(*y.shape)
        (ref,) = torch.autograd.grad(y, w, gy)
        got = lib.conv_wgrad(gy, x, (3, 3, 3), 1, (1, 1, 1))
        assert got.shape == ref.shape
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), (cin, cout, D, H, W, float((got - ref).abs().max() / ref.abs().max()))
        assert torch.equal(got, lib.conv_wgrad(gy, x, (3, 3, 3), 1, (1, 1, 1)))
    for cin, cout, st in [(32, 8, 1), (8, 16, 2), (16, 32, 2), (64, 64, 1), (8, 1, 1), (8, 8, 1)]:
        x = rnd(1, cin, 4, 6, 10)
        w = rnd(cout, cin, 3, 3, 3).requires_grad_(True)
        y = F.conv3d(x, w, None, st, 1)
        gy = rnd(*y.shape)
        (ref,) = torch.autograd.grad(y, w, gy)
        got = lib.conv_wgrad(gy, x, (3, 3, 3), st, (1, 1, 1))
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), (cin, cout, st)
    for cin, cout in [(64, 32), (16, 8)]:                                   # ConvTranspose3d(k3, s2, p1, op1)
        x = rnd(1, cin, 2, 3, 5)
        w = rnd(cin, cout, 3, 3, 3).requires_grad_(True)
        y = F.conv_transpose3d(x, w, None, stride=2, padding=1, output_padding=1)
        gy = rnd(*y.shape)
        (ref,) = torch.autograd.grad(y, w, gy)
        got = lib.conv_wgrad(x, gy, (3, 3, 3), 2, (1, 1, 1))
        assert float((got - ref).abs().max()) <= 2e-5 * float(ref.abs().max()), (cin, cout)
    # the two-stage commit (workspace given: what the wrappers do) is deterministic; without a workspace the entry falls back to
    # fp32 atomics onto a zeroed grad_w and must agree
    a_cl, b_cl = rnd(1, 4, 6, 10, 16), rnd(1, 4, 6, 10, 32)
    two = [lib.conv_wgrad_cl(a_cl, b_cl, 1) for _ in range(2)]
    assert torch.equal(two[0], two[1])
    gw = torch.full((16, 32, 3, 3, 3), 7.0, device=dev)
    lib._check(lib.dll.enerf_conv_wgrad(a_cl.data_ptr(), b_cl.data_ptr(), 1, 4, 6, 10, 16, 4, 6, 10, 32, 3, 3, 3, 1, 1, 1, 1,
                                        gw.data_ptr(), None, 0, lib.stream_of(a_cl)), "conv_wgrad")
    assert float((gw - two[0]).abs().max()) <= 1e-5 * float(two[0].abs().max())
    am, bm = rnd(1000, 40), rnd(1000, 24)
    g1, gb1 = lib.gemm_wgrad(am, bm, bias=True)
    assert torch.equal(g1, lib.gemm_wgrad(am, bm, bias=True)[0])
    assert float((g1 - am.t() @ bm).abs().max()) <= 2e-5 * float((am.t() @ bm).abs().max())
    assert float((gb1 - am.sum(0)).abs().max()) <= 2e-5 * float(am.sum(0).abs().max())
    g2 = torch.full((40, 24), 7.0, device=dev)
    lib._check(lib.dll.enerf_gemm_wgrad(am.data_ptr(), 40, 40, bm.data_ptr(), 24, 24, 1000, g2.data_ptr(), None, None, 0,
                                        lib.stream_of(am)), "gemm_wgrad")
    assert float((g2 - g1).abs().max()) <= 1e-5 * float(g1.abs().max())
    # ABI v11: the grouped call (what NerfMlpFn's backward issues: all of one MLP's weight gradients in two to four launches) gives
    # every member the bits of its single call — shapes of all three register classes, column slices, a gradient written as a
    # column block of a wider matrix, with and without the bias column, ragged row counts
    P = 1003
    hv, d64, d1, d32, xs = rnd(P, 88), rnd(P, 64), rnd(P, 1), rnd(P, 32), rnd(P, 15)
    wide = torch.full((64, 88 + 15), 7.0, device=dev)
    members = [dict(a=d1, b=d64, bias=True), dict(a=d64, b=hv, bias=True, into=(wide, 0)), dict(a=d64, b=xs, into=(wide, 88)),
               dict(a=d1, b=hv, Cb=64, bias=True), dict(a=d64, b=hv[:, 64:], bias=True), dict(a=d32[:, :16], b=d32, bias=True),
               dict(a=d32, b=xs[:, :11]), dict(a=d32, b=hv[:, :71], bias=True), dict(a=xs[:, :11], b=xs[:, 11:], bias=True)]
    got = lib.gemm_wgrad_group(members)
    for m, (gw_, gb_) in zip(members, got):
        single = lib.gemm_wgrad(m["a"], m["b"], Cb=m.get("Cb"), bias=bool(m.get("bias")))
        sw, sb = single if m.get("bias") else (single, None)
        if m.get("into") is not None:
            c0 = m["into"][1]
            assert gw_ is wide and torch.equal(wide[:, c0:c0 + sw.shape[1]], sw)
        else:
            assert torch.equal(gw_, sw)
        assert (gb_ is None) == (sb is None) and (sb is None or torch.equal(gb_, sb))
    # ABI v11: deferred second stages — the reductions of a whole backward pass recorded and run as ONE kernel on leaving the block:
    # every gradient (the k_wgrad_reduce and the k_colsum kinds, 3-D, 2-D, GEMM, with a bias column) gets the bits of its immediate call
    i1, i2, i3, i4 = (rnd(1, 8, 32, 40, 8), rnd(1, 8, 32, 40, 16)), (rnd(1, 4, 8, 10, 32), rnd(1, 8, 16, 20, 16)), \
        (rnd(2, 16, 20, 8), rnd(2, 16, 20, 8)), (rnd(2, 8, 10, 16), rnd(2, 16, 20, 8))
    calls = [lambda: lib.conv_wgrad_cl(a_cl, b_cl, 1), lambda: lib.conv_wgrad_cl(i1[0], i1[1], 1), lambda: lib.conv_wgrad_cl(i2[0], i2[1], 2),
             lambda: lib.conv_wgrad_cl2d(i3[0], i3[1], 3, 1), lambda: lib.conv_wgrad_cl2d(i4[0], i4[1], 5, 2), lambda: lib.gemm_wgrad(am, bm),
             lambda: lib.gemm_wgrad(am, bm, bias=True)]          # (every output of a recorded call must stay alive until the flush)
    now = [c() for c in calls]
    with lib.wgrad_reduce_batch(a_cl):
        later = [c() for c in calls]
        with pytest.raises(Exception, match="already deferring"):
            with lib.wgrad_reduce_batch(a_cl):
                pass
    for k, (x0, x1) in enumerate(zip(now[:6], later[:6])):
        assert torch.equal(x0, x1), k
    assert torch.equal(now[6][0], later[6][0]) and torch.equal(now[6][1], later[6][1])
    assert lib._deferred_scratch is None
    assert torch.equal(lib.conv_wgrad_cl(a_cl, b_cl, 1), two[0])          # and the library is back to immediate second stages
    with pytest.raises(Exception, match="4 x 6 tiles"):
        lib.gemm_wgrad_group([dict(a=rnd(10, 80), b=rnd(10, 8))])
    with pytest.raises(Exception, match="1..16 members"):
        lib.gemm_wgrad_group([dict(a=d1, b=d64)] * 17)


def _check_feature_net_train(lib, dev, H=32, W=64, n=3, tol=2e-4):
    """autograd.FeatureNetTrainFn (conv forward / input gradients / BatchNorm2d / weight gradients / upsampling adjoint on the
    HIP kernels, channels-last throughout) against the same FeatureNet through its torch modules in fp32 AND in fp64: the
    three output maps, every parameter gradient and the BatchNorm running statistics.  A parameter gradient must be within
    ``tol`` of the fp32 module path, or — the gradients of the upstream layers amplify 1e-5-level differences between two
    fp32 implementations of one op ~200x through the BatchNorm backward (batch statistics) — at least as close to the fp64
    result as the fp32 module path is (3x slack)."""
    from enerf_amd.autograd import feature_net_train
    from enerf_amd.network import FeatureNet
    from torch_twins import feature_net_forward
    torch.manual_seed(5)
    # the upsampling adjoint on its own: enerf_up2_adjoint vs autograd through F.interpolate(2x, bilinear, align_corners)
    c = torch.randn(2, 16, H // 4, W // 4, device=dev, requires_grad=True)
    gf = torch.randn(2, 16, H // 2, W // 2, device=dev)
    extra = torch.randn(2, H // 4, W // 4, 16, device=dev)
    F.interpolate(c, scale_factor=2, mode="bilinear", align_corners=True).backward(gf)
    got = lib.up2_adjoint(gf.permute(0, 2, 3, 1).contiguous(), add=extra)
    ref = c.grad.permute(0, 2, 3, 1) + extra
    assert float((got - ref).abs().max()) <= 5e-5 * float(ref.abs().max())
    nets = [FeatureNet().to(dev).train() for _ in range(3)]
    with torch.no_grad():
        for k, v in nets[0].state_dict().items():
            if k.endswith("bn.weight"):
                v.uniform_(0.5, 1.5)
            elif k.endswith("bn.bias"):
                v.normal_(0.0, 0.1)
    nets[1].load_state_dict(nets[0].state_dict())
    nets[2].load_state_dict(nets[0].state_dict())
    nets[2].double()
    x = torch.randn(n, 3, H, W, device=dev)
    gen = torch.Generator().manual_seed(6)
    outs = []
    for i, net in enumerate(nets):                       # 0: HIP fp32, 1: modules fp32, 2: modules fp64
        o = feature_net_train(lib, net, x) if i == 0 else feature_net_forward(net, x.double() if i == 2 else x)
        if not outs:
            wts = [torch.randn(t.shape, generator=gen).to(dev) for t in o]
        sum((t * w_.to(t.dtype)).sum() for t, w_ in zip(o, wts)).backward()
        outs.append(o)
    for a, b in zip(outs[0], outs[1]):
        assert a.shape == b.shape
        assert float((a - b).abs().max()) <= 2e-5 * float(b.abs().max()), float((a - b).abs().max() / b.abs().max())
    named = [dict(net.named_parameters()) for net in nets]
    for k, p0 in named[0].items():
        g0, g1, g64 = p0.grad.double(), named[1][k].grad.double(), named[2][k].grad
        scale = max(float(g64.abs().max()), 1e-12)
        err_vs32 = float((g0 - g1).abs().max()) / scale
        err_hip, err_mod = float((g0 - g64).abs().max()) / scale, float((g1 - g64).abs().max()) / scale
        assert err_vs32 <= tol or err_hip <= max(tol, 3.0 * err_mod), (k, err_vs32, err_hip, err_mod)
    for (k, b0), (_, b1) in zip(nets[0].named_buffers(), nets[1].named_buffers()):
        if b1.dtype.is_floating_point:
            assert float((b0 - b1).abs().max()) <= 1e-5 + 1e-4 * float(b1.abs().max()), k


def test_batchnorm_train_kernels_match_torch_modules_emulated():
    """autograd._BatchNormTrain (statistics + coefficient + affine kernels) against nn.BatchNorm in training mode: output,
    input / gamma / beta gradients and the running statistics, with momentum 0.1 and with momentum=None (cumulative average),
    with and without ReLU + skip."""
    from emu_lib import emu_lib
    from enerf_amd.autograd import _BatchNormTrain
    lib = emu_lib()
    torch.manual_seed(3)
    for mom in (0.1, None):
        for relu in (False, True):
            bn, ref = torch.nn.BatchNorm1d(8, momentum=mom).train(), torch.nn.BatchNorm1d(8, momentum=mom).train()
            with torch.no_grad():
                bn.weight.uniform_(0.5, 1.5); bn.bias.normal_()
            ref.load_state_dict(bn.state_dict())
            for it in range(2):
                z = (torch.randn(60, 8) * 2 + 1).requires_grad_(True)
                res = torch.randn(60, 8)
                g = torch.randn(60, 8)
                blk = _BatchNormTrain(lib, bn, relu)
                out = blk.forward(z.detach(), residual=res if relu else None)
                r = ref(z)
                r = (torch.relu(r) + res) if relu else r
                assert float((out - r).abs().max()) <= 2e-6 * float(r.abs().max())
                r.backward(g)
                dz, dgamma, dbeta = blk.backward(g)
                assert float((dz - z.grad).abs().max()) <= 2e-5 * float(z.grad.abs().max())
                assert float((dgamma - ref.weight.grad).abs().max()) <= 2e-5 * float(ref.weight.grad.abs().max())
                assert float((dbeta - ref.bias.grad).abs().max()) <= 2e-5 * float(ref.bias.grad.abs().max())
                ref.zero_grad()
                for name in ("running_mean", "running_var"):
                    a, b = getattr(bn, name), getattr(ref, name)
                    assert float((a - b).abs().max()) <= 1e-6 + 1e-5 * float(b.abs().max()), (mom, relu, it, name)
                assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == it + 1


def _check_bn_two_launch_form(lib, dev):
    """enerf_bn_train_apply / enerf_bn_train_bwd_apply (ABI v11: the coefficient launch folded into the affine kernel's prologue for
    small / mid layers) against the three-launch entries they replace — outputs, coefficients, running statistics and gradients
    bit for bit, on layers on both sides of the fold's size limit (partial rows x C <= 2048) and with ragged tails."""
    import copy
    torch.manual_seed(11)
    for C_, n, relu, res in ((64, 1280, True, True), (32, 10240, True, False), (16, 81920, False, True), (8, 60, True, True),
                             (8, 300000, True, False), (32, 61440, False, False), (16, 777, True, True)):
        bn = torch.nn.BatchNorm1d(C_, momentum=0.1).train().to(dev)
        with torch.no_grad():
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_()
        bn2 = copy.deepcopy(bn)
        z, g = (torch.randn(n, C_) * 2 + 1).to(dev), torch.randn(n, C_).to(dev)
        r = torch.randn(n, C_).to(dev) if res else None
        y, mi, ss, cnt = lib.bn_train_apply(z, bn, r, relu)
        mi2, ss2, cnt2 = lib.bn_train_stats(z, bn2)
        y2 = lib.channel_affine(z, ss2[0], ss2[1], residual=r, relu=relu)
        what = (C_, n, relu, res)
        assert cnt == cnt2 and torch.equal(mi, mi2) and torch.equal(ss, ss2) and torch.equal(y, y2), what
        assert torch.equal(bn.running_mean, bn2.running_mean) and torch.equal(bn.running_var, bn2.running_var), what
        assert int(bn.num_batches_tracked) == int(bn2.num_batches_tracked) == 1
        dz, dgb = lib.bn_train_bwd_apply(g, z, mi, ss, relu)
        mask = dict(z_mask=z, mask_scale=ss2[0], mask_shift=ss2[1]) if relu else {}
        dgb2, k23 = lib.bn_train_bwd_stats(g, z, mi2, ss2[0], **mask)
        dz2 = lib.channel_affine(g, ss2[0], k23[1], b=z, q=k23[0], **mask)
        assert torch.equal(dgb, dgb2) and torch.equal(dz, dz2), what


def test_batchnorm_two_launch_form_equals_the_three_launch_form_emulated():
    from emu_lib import emu_lib
    _check_bn_two_launch_form(emu_lib(), "cpu")


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_batchnorm_two_launch_form_equals_the_three_launch_form_on_gpu():
    from enerf_amd.lib import get_lib
    _check_bn_two_launch_form(get_lib(), "cuda:0")


def test_up2_adjoint_emulated_sizes():
    """enerf_up2_adjoint against autograd through F.interpolate at even, odd and non-square coarse sizes, with and without the
    summed-in second gradient; and the guards of the entry."""
    from emu_lib import emu_lib
    from enerf_amd.lib import EnerfError
    lib = emu_lib()
    g = torch.Generator().manual_seed(11)
    for (N, C_, Hc, Wc) in ((1, 8, 8, 16), (2, 16, 15, 20), (1, 32, 5, 33), (1, 4, 2, 2)):
        c = torch.randn(N, C_, Hc, Wc, generator=g, requires_grad=True)
        gf = torch.randn(N, C_, 2 * Hc, 2 * Wc, generator=g)
        F.interpolate(c, scale_factor=2, mode="bilinear", align_corners=True).backward(gf)
        ref = c.grad.permute(0, 2, 3, 1)
        got = lib.up2_adjoint(gf.permute(0, 2, 3, 1).contiguous())
        assert float((got - ref).abs().max()) <= 2e-6 * float(ref.abs().max()), (N, C_, Hc, Wc)
        extra = torch.randn(N, Hc, Wc, C_, generator=g)
        got2 = lib.up2_adjoint(gf.permute(0, 2, 3, 1).contiguous(), add=extra)
        assert float((got2 - (ref + extra)).abs().max()) <= 2e-6 * float((ref + extra).abs().max())
    with pytest.raises(EnerfError, match="bad arguments"):           # channel count must be a multiple of 4
        lib.up2_adjoint(torch.zeros(1, 4, 4, 6))


def test_graphed_step_shape_key_and_flat_sync_guards():
    """Host logic of train_graph that needs no device: the per-shape key of GraphedTrainSteps distinguishes what a captured
    graph depends on (tensor shapes and dtypes, not values or non-tensor entries), and FlatGradSync refuses to exist without
    a process group."""
    from enerf_amd.train_graph import FlatGradSync, GraphedTrainSteps
    _, b3 = _train_batch(seed=1, S=3)
    _, b3b = _train_batch(seed=2, S=3)
    _, b2 = _train_batch(seed=1, S=2)
    k = GraphedTrainSteps.key
    assert k(b3) == k(b3b) and k(b3) != k(b2)
    assert k(dict(b3, meta={"scene": "x"})) == k(b3)
    assert k(dict(b3, near_far=b3["near_far"].double())) != k(b3)
    with pytest.raises(RuntimeError, match="process group"):
        FlatGradSync(torch.nn.Linear(2, 2))


def _check_pack_plan_images(lib, dev):
    """enerf_amd/pack_plan.py: the one-launch gather of a network's packed weight images is, element for element, what the
    per-layer pack entries (enerf_conv3d_layer_pack / enerf_conv2d_layer_pack / enerf_weights_flip_transpose /
    enerf_conv2d_s2k5_dgrad_pack) produce from the same parameters — after a parameter update too (the plan holds getters)."""
    from enerf_amd import pack_plan as PP
    from enerf_amd.network import CostRegParams, FeatureNet
    torch.manual_seed(11)
    S1, S2, T2 = 0, 1, 2
    for full in (True, False):
        m = CostRegParams(32 if full else 8, full).to(dev)
        plan = PP.plan_of(lib, m, PP.cost_reg_plan, dev)
        assert PP.plan_of(lib, m, PP.cost_reg_plan, dev) is plan                  # cached per module
        import copy
        copy.deepcopy(m)                                                          # (the cache must not ride on the module)
        for rnd in range(2):
            if rnd == 1:
                with torch.no_grad():
                    for p_ in m.parameters():
                        p_.add_(torch.randn_like(p_) * 0.1)
            img = plan.run()
            kinds = {0: S1, 1: S2, 2: S1, 3: S2, 4: S1, 5: S2, 6: S1, 7: T2, 9: T2, 11: T2}
            for i in [0, 1, 2, 3, 4] + ([5, 6, 7] if full else []) + [9, 11]:
                mod = getattr(m, f"conv{i}")
                w = (mod[0] if i in (7, 9, 11) else mod.conv).weight.detach().contiguous()
                k = kinds[i]
                cin, cout = (w.shape[0], w.shape[1]) if k == T2 else (w.shape[1], w.shape[0])
                assert torch.equal(img[i, "fwd"], lib.conv3d_layer_pack(w, cin, cout, k)), (i, "fwd")
                if k == S1:
                    ref = lib.conv3d_layer_pack(lib.weights_flip_transpose(w), cout, cin, S1)
                else:
                    ref = lib.conv3d_layer_pack(w, cout, cin, T2 if k == S2 else S2)
                assert torch.equal(img[i, "bwd"], ref), (i, "bwd")
            wf, wd = m.feat_conv[0].weight.detach().contiguous(), m.depth_conv[0].weight.detach().contiguous()
            w16 = lib.concat2_pad(wf, wd, 16 * 8 * 27).view(16, 8, 3, 3, 3)
            assert torch.equal(img["heads", "fwd"], lib.conv3d_layer_pack(w16, 8, 16, S1))
            assert torch.equal(img["heads", "bwd"], lib.conv3d_layer_pack(lib.weights_flip_transpose(w16), 16, 8, S1))
    f = FeatureNet().to(dev)
    with torch.no_grad():
        for p_ in f.parameters():
            p_.add_(torch.randn_like(p_) * 0.1)
    img = PP.plan_of(lib, f, PP.feature_net_plan, dev).run()
    for name in PP.FEAT_LAYERS:
        conv = getattr(f, name[:5])[int(name[6])].conv if name.startswith("conv") else getattr(f, name)
        w = conv.weight.detach().contiguous()
        b = None if conv.bias is None else conv.bias.detach()
        cout, cin, k, _ = w.shape
        assert torch.equal(img[name, "fwd"], lib.conv2d_layer_pack(w, b, cin, cout, k)), name
        if name == "conv0.0":
            continue
        if int(conv.stride[0]) == 1:
            assert torch.equal(img[name, "bwd"], lib.conv2d_layer_pack(lib.weights_flip_transpose(w), None, cout, cin, k)), name
        else:
            assert torch.equal(img[name, "s2k5"], lib.conv2d_s2k5_dgrad_pack(w)[0]), name


def test_pack_plan_images_emulated():
    from emu_lib import emu_lib
    _check_pack_plan_images(emu_lib(), torch.device("cpu"))


@pytest.mark.gpu
def test_pack_plan_images_on_gpu():
    from enerf_amd.lib import get_lib
    _check_pack_plan_images(get_lib(), torch.device("cuda:0"))


def test_feature_net_train_emulated():
    from emu_lib import emu_lib
    _check_feature_net_train(emu_lib(), torch.device("cpu"))


def test_conv_wgrad_emulated():
    from emu_lib import emu_lib
    _check_conv_wgrad(emu_lib(), torch.device("cpu"))


def test_conv_wgrad_with_few_cus_emulated():
    """The same weight-gradient checks with the emulated library sized for three CUs: the wgrad kernels' persistent tile loops
    take several passes, chunk counts drop to 1, and the deferred second stages (k_wgrad_reduce_batch) add more partial rows each."""
    from emu_lib import emu_cu_count, emu_lib
    lib = emu_lib()
    with emu_cu_count(lib, 3):
        _check_conv_wgrad(lib, torch.device("cpu"))


def test_hip_backward_stages_emulated():
    from emu_lib import emu_lib
    _check_hip_backward_stages(emu_lib(), torch.device("cpu"))


def test_training_step_with_hip_stages_matches_reference_gradients():
    """The reference-pinned training step again, now with the three HIP forward+backward stages switched on (CPU lane
    emulator here, the real kernels in the gpu test below)."""
    from emu_lib import emu_lib
    g = np.load(os.path.join(GOLDEN, "train_tiny.npz"))
    cfg, batch = _train_batch()
    torch.set_num_threads(1)
    net = Network(cfg, lib=emu_lib())
    net.load_state_dict(load_weights(), strict=False)
    net.train()
    from enerf_amd import train_path as T
    from enerf_amd import autograd as AG
    assert T._hip_lib(net, batch["src_inps"]) is not None and not getattr(net, "_stage_twins", None)
    calls = {"cost_reg": 0, "conv": 0, "feature_net": 0}
    orig_cr, orig_conv, orig_fn = AG.cost_reg_train, AG.conv_module, AG.feature_net_train
    AG.cost_reg_train = lambda *a: (calls.__setitem__("cost_reg", calls["cost_reg"] + 1), orig_cr(*a))[1]
    AG.conv_module = lambda *a: (calls.__setitem__("conv", calls["conv"] + 1), orig_conv(*a))[1]
    AG.feature_net_train = lambda *a: (calls.__setitem__("feature_net", calls["feature_net"] + 1), orig_fn(*a))[1]
    try:
        loss = _loss(net(batch), batch)
    finally:
        AG.cost_reg_train, AG.conv_module, AG.feature_net_train = orig_cr, orig_conv, orig_fn
    # both cost-reg nets and the FeatureNet whole on HIP (conv forward + input gradients + BatchNorm): no per-layer ConvFn left
    assert calls == {"cost_reg": 2, "conv": 0, "feature_net": 1}
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-5)
    loss.backward()
    for name, p in net.named_parameters():
        assert p.grad is not None or f"nograd/{name}" in g.files, name
        if f"grad/{name}/full" in g.files:
            ref = g[f"grad/{name}/full"]
            assert np.abs(p.grad.reshape(-1).numpy() - ref).max() <= 5e-4 * np.abs(ref).max() + 1e-9, name
    for name, buf in net.named_buffers():                # BatchNorm running statistics updated by the HIP path as well
        if f"buf/{name}" in g.files:
            np.testing.assert_allclose(buf.numpy(), g[f"buf/{name}"], rtol=2e-4, atol=2e-6, err_msg=name)
    # the same step with the whole-net HIP functions off (per-layer ConvFn: library conv forward / input gradient + torch
    # BatchNorm, HIP weight gradients only) gives the same gradients
    net2 = Network(cfg, lib=emu_lib())
    net2.load_state_dict(load_weights(), strict=False)
    net2.train()
    net2.hip_cost_reg_train = False
    net2.hip_feature_net_train = False
    _loss(net2(batch), batch).backward()
    for (n1, p1), (_, p2) in zip(net.named_parameters(), net2.named_parameters()):
        if p1.grad is not None:
            assert float((p1.grad - p2.grad).abs().max()) <= 5e-4 * float(p2.grad.abs().max()) + 1e-9, n1


def test_train_then_eval_repacks_weights():
    """An optimizer step changes the parameters; the eval-mode HIP path must see the new ones (packed images rebuilt)."""
    from emu_lib import emu_lib
    cfg, batch = _train_batch()
    net = Network(cfg, lib=emu_lib())
    net.load_state_dict(load_weights(), strict=False)
    net.eval()
    with torch.no_grad():
        before = net(batch)["rgb_level1"].clone()
    net.train()
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    loss = _loss(net(batch), batch)
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_value_(net.parameters(), 40)            # trainer.py:62
    opt.step()
    net.eval()
    with torch.no_grad():
        after = net(batch)["rgb_level1"]
    from oracle import enerf_oracle as O
    with torch.no_grad():
        ref = O.forward(cfg, {k: v.detach() for k, v in net.state_dict().items()}, batch)["rgb_level1"]
    assert float((after - before).abs().max()) > 1e-5                 # the step changed the image ...
    assert float((after - ref).abs().max()) < 1e-4                    # ... and the HIP path renders the NEW weights


def _ddp_worker(rank, world, port, q):
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from torch.nn.parallel import DistributedDataParallel as DDP
    cfg, batch = _train_batch(seed=20 + rank)                          # DistributedSampler: a different sample per rank
    net = DDP(_net(cfg, twins=True), find_unused_parameters=True)      # trainer.py:17-22
    loss = _loss(net(batch), batch)
    loss.backward()                                                    # gradient all-reduce (RCCL on GPUs, gloo here)
    grads = {n: p.grad.clone() for n, p in net.module.named_parameters() if p.grad is not None}
    q.put((rank, float(loss), {n: v.numpy() for n, v in grads.items()}))
    dist.destroy_process_group()


def _batch2():
    """A two-sample batch (B = 2) and its per-sample slices."""
    cfg = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(True, True))
    b = make_batch(32, 64, 3, cfg, seed=31, B=2, textured=True)
    rng = np.random.default_rng(31)
    for i in range(2):
        b[f"rgb_{i}"] = rng.uniform(0, 1, size=(2, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
    full = {k: torch.from_numpy(v) for k, v in b.items()}
    return cfg, full, [{k: v[r:r + 1].contiguous() for k, v in full.items()} for r in range(2)]


def _syncbn_worker(rank, world, port, q):
    try:
        sys.path.insert(0, HERE)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), ENERF_EMU_THREADS="2")
        torch.set_num_threads(1)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from emu_lib import emu_lib
        cfg, _, parts = _batch2()
        net = Network(cfg, lib=emu_lib())                                  # HIP training stages on (lane emulator)
        net.load_state_dict(load_weights(), strict=False)
        net.train()
        # trainer.py:16 on the WHOLE network: every BatchNorm (FeatureNet 2-D, cost-reg 3-D) runs inside the HIP training
        # functions, whose statistics exchange (autograd._BatchNormTrain) works on any backend (torch's own SyncBatchNorm forward,
        # which refuses CPU tensors, is never called on this path)
        net = torch.nn.SyncBatchNorm.convert_sync_batchnorm(net)
        assert isinstance(net.feature_net.conv0[0].bn, torch.nn.SyncBatchNorm)
        loss = _loss(net(parts[rank]), parts[rank])
        loss.backward()
        grads = {}
        for n, p in net.named_parameters():                                # what DDP does: average over ranks
            if p.grad is not None:
                dist.all_reduce(p.grad)
                grads[n] = (p.grad / world).numpy()
        q.put((rank, grads, {n: b.numpy().copy() for n, b in net.named_buffers() if n.endswith("running_var")}))
        dist.destroy_process_group()
    except Exception as e:                                                 # never leave the parent waiting
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc(), None))


def test_two_rank_syncbn_on_hip_training_path_equals_one_process_with_batch_two():
    """trainer.py:15-22 on the HIP training path: SyncBatchNorm statistics of EVERY BatchNorm of the network (FeatureNet and
    both cost-volume networks) all-reduced inside the HIP training functions (one small all-reduce per BN layer and
    direction) + gradient averaging == one process with both samples in one batch."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_syncbn_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=300) for _ in procs], key=lambda r: r[0])
    [p.join(60) for p in procs]
    for r in res:
        assert not isinstance(r[1], str), r[1]
    torch.set_num_threads(1)
    cfg, full, _ = _batch2()
    net = _net(cfg, twins=True)                                        # torch-op twins, plain BatchNorm, B = 2
    _loss(net(full), full).backward()
    ref = {n: p.grad for n, p in net.named_parameters() if p.grad is not None}
    checked = 0
    for n, v in res[0][1].items():
        assert np.allclose(v, res[1][1][n], rtol=1e-5, atol=1e-9), n   # both ranks hold the averaged gradients
        r = ref[n].numpy()
        tol = 1.5e-2      # two different summation orders of the same ill-conditioned step (see GPU_GRAD_TOL's note)
        assert np.abs(v - r).max() <= tol * max(np.abs(r).max(), 1e-12) + 1e-9, (n, float(np.abs(v - r).max() / max(np.abs(r).max(), 1e-12)))
        checked += 1
    assert checked > 80
    for n, v in res[0][2].items():                                     # running_var from the global statistics
        assert np.allclose(v, dict(net.named_buffers())[n].numpy(), rtol=1e-3, atol=1e-6), n


def test_two_rank_ddp_gradients_equal_mean_of_single_process_gradients():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29700 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    [p.join(60) for p in procs]
    # both ranks hold the same (averaged) gradients
    for n in res[0][2]:
        np.testing.assert_allclose(res[0][2][n], res[1][2][n], rtol=1e-6, atol=1e-9, err_msg=n)
    # = the mean of the two single-process gradients
    torch.set_num_threads(1)
    single = []
    for rank in range(2):
        cfg, batch = _train_batch(seed=20 + rank)
        net = _net(cfg, twins=True)
        loss = _loss(net(batch), batch)
        loss.backward()
        assert float(loss) == pytest.approx(res[rank][1], rel=1e-5)
        single.append({n: p.grad for n, p in net.named_parameters() if p.grad is not None})
    for n, v in res[0][2].items():
        mean = 0.5 * (single[0][n] + single[1][n]).numpy()
        assert np.abs(v - mean).max() <= 2e-5 * max(np.abs(mean).max(), 1e-12) + 1e-10, n


def _flat_sync_worker(rank, world, port, q):
    try:
        sys.path.insert(0, HERE)
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        torch.set_num_threads(1)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from torch.nn.parallel import DistributedDataParallel as DDP
        from enerf_amd.train_graph import FlatGradSync, train_step
        cfg, batch = _train_batch(seed=40 + rank)                          # a different sample per rank
        nets = [_net(cfg, twins=True), _net(cfg, twins=True)]
        with torch.no_grad():                                              # rank 1 starts from DIFFERENT weights: both schemes
            if rank == 1:                                                  # must begin by adopting rank 0's
                for net in nets:
                    for p in net.parameters():
                        p.mul_(1.01)
        opts = [torch.optim.SGD(n.parameters(), lr=1e-2, momentum=0.9) for n in nets]
        ddp = DDP(nets[0], find_unused_parameters=True)                    # trainer.py:17-22 (broadcasts rank 0's state)
        sync = FlatGradSync(nets[1])
        sync.broadcast()
        for _ in range(2):
            loss_a = train_step(ddp, opts[0], _loss, batch, 40.0, None, params=list(nets[0].parameters()))
            loss_b = train_step(nets[1], opts[1], _loss, batch, 40.0, sync)
        sd = [{k: v.numpy().copy() for k, v in n.state_dict().items()} for n in nets]
        q.put((rank, float(loss_a.detach()), float(loss_b.detach()), sd[0], sd[1]))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "ERROR: " + traceback.format_exc(), None, None, None))


def test_flat_gradient_sync_step_equals_distributed_data_parallel_step():
    """train_graph.FlatGradSync (ONE all-reduce of one flat buffer after backward — the data-parallel step the hipGraph
    captures) leaves exactly the parameters DistributedDataParallel's step leaves: two ranks, two optimizer steps each,
    different samples per rank, rank 1 starting from different weights."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 30100 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_flat_sync_worker, args=(r, 2, port, q)) for r in range(2)]
    [p.start() for p in procs]
    res = sorted([q.get(timeout=900) for _ in procs], key=lambda r: r[0])
    [p.join(60) for p in procs]
    for r in res:
        assert not isinstance(r[1], str), r[1]
    for rank, loss_a, loss_b, sd_ddp, sd_flat in res:
        assert loss_a == pytest.approx(loss_b, rel=1e-6)
        for k, v in sd_ddp.items():
            # (running statistics: with PLAIN BatchNorm they are per-rank quantities that DDP overwrites with rank 0's before
            # every forward; under the trainer's SyncBatchNorm they are identical on all ranks by construction)
            if v.dtype.kind == "f" and "running" not in k:
                assert np.abs(v - sd_flat[k]).max() <= 1e-6 * max(np.abs(v).max(), 1e-12) + 1e-9, (rank, k)
    for k, v in res[0][4].items():                                         # and both ranks hold the same model
        if v.dtype.kind == "f" and "running" not in k:
            np.testing.assert_allclose(v, res[1][4][k], rtol=1e-6, atol=1e-9, err_msg=k)


GPU_GRAD_TOL = 5e-4            # max|grad - reference| / max|reference| per parameter, every element (fp32 atomics reorder sums)
# The 128x160 and 512x640 steps are ILL-CONDITIONED IN THE REFERENCE ITSELF: its own parameter gradients move by ~2e-3 between 1
# and 8 CPU threads, by ~7e-3 when the cost volume is perturbed by 1e-6 relative, and by up to 1e-1 when the FeatureNet's output
# maps are perturbed by 1e-5 relative (test_mid_size_step_is_ill_conditioned_in_the_reference: BatchNorm batch statistics over as
# few as 80 positions + the floor() of every bilinear sample position).  An element-wise bound against the reference's fp32
# gradients would have to be that loose (round 3 used 1.5e-1), so those sizes are judged by ARBITRATION instead: the
# reference's own modules run in float64 (tests/golden/train_*_fp64.npz) are the truth, and our fp32 gradients must be as close
# to it (x3) as the reference's fp32 gradients are (_assert_as_close_to_fp64_as_the_reference).  The 5e-4 bound holds at 32x64.


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_training_step_on_gpu_matches_reference_gradients():
    """The same reference-pinned step on the MI355X (PyTorch-ROCm autograd: MIOpen convolutions, atomics in the
    grid_sample backward -> a looser tolerance than the CPU run), then an optimizer step and an eval-mode HIP frame."""
    g = np.load(os.path.join(GOLDEN, "train_tiny.npz"))
    dev = torch.device("cuda:0")
    from enerf_amd.lib import get_lib
    _check_hip_backward_stages(get_lib(), dev)           # each HIP forward+backward stage vs its torch-op twin
    _check_conv_wgrad(get_lib(), dev)                    # MFMA weight gradients vs torch's
    _check_mlp_backward(get_lib(), dev)                  # fused MLP backward vs torch autograd
    _check_feature_net_train(get_lib(), dev)             # whole FeatureNet forward + backward vs its torch modules
    _check_feature_net_train(get_lib(), dev, H=128, W=160)
    _check_feature_net_train(get_lib(), dev, H=512, W=640, tol=3e-3)   # 983k-position fp32 reductions
    cfg, batch = _train_batch()
    batch = {k: v.to(dev) for k, v in batch.items()}
    net = _net(cfg).to(dev)
    from enerf_amd import train_path as T
    assert T._hip_lib(net, batch["src_inps"]) is get_lib()   # the HIP stages are on
    out = net(batch)
    loss = _loss(out, batch)
    assert float(loss) == pytest.approx(float(g["loss"]), rel=1e-4)
    loss.backward()
    errs = _grad_errors([(n, p.grad) for n, p in net.named_parameters() if p.grad is not None], g)
    bad = {n: e for n, e in errs.items() if e > GPU_GRAD_TOL}
    assert len(errs) >= 110 and not bad, bad
    # ... and the mid-size fixture (128x160, 16 + 8 planes, 20,480 + 1,280 rays), every element of every gradient.  This step
    # is ill-conditioned in the reference itself (test_mid_size_step_is_ill_conditioned_in_the_reference), so the bar is the
    # fp64 ARBITRATION: our fp32 gradients must be as close (x3) to the reference's float64 step as the reference's own fp32
    # gradients are — with the whole FeatureNet on the HIP kernels, and with it on the library convolutions
    g2, g2_64 = np.load(os.path.join(GOLDEN, "train_small.npz")), np.load(os.path.join(GOLDEN, "train_small_fp64.npz"))
    cfg2, batch2 = _train_batch(**TRAIN_CASES["train_small"])
    batch2 = {k: v.to(dev) for k, v in batch2.items()}
    for hip_fnet in (True, False):
        net2 = _net(cfg2).to(dev)
        net2.hip_feature_net_train = hip_fnet
        loss2 = _loss(net2(batch2), batch2)
        assert float(loss2) == pytest.approx(float(g2["loss"]), rel=1e-4)
        loss2.backward()
        named2 = [(n, p.grad) for n, p in net2.named_parameters() if p.grad is not None]
        dist = _distance_to_fp64(named2, g2, g2_64)
        noise2 = np.load(os.path.join(GOLDEN, "train_small_noise.npz"))
        stable2 = _assert_stable_parameters_elementwise(named2, g2, g2_64, noise2, sparse=False, what=f"128x160 hip_fnet={hip_fnet}")
        print(f"128x160: {len(stable2)} stable parameters element-wise within 3e-4 of the reference's fp32 gradients")
        print("128x160 fp64 arbitration (ours, reference), FeatureNet on HIP =", hip_fnet,
              _assert_as_close_to_fp64_as_the_reference(dist, noise2, what=f"128x160 hip_fnet={hip_fnet}"))
    opt = torch.optim.Adam(net.parameters(), lr=5e-4)
    opt.step()
    net.eval()
    with torch.no_grad():
        img = net(batch)["rgb_level1"]                                   # the HIP path, re-packed weights
    from oracle import enerf_oracle as O
    with torch.no_grad():
        ref = O.forward(cfg, {k: v.detach().cpu() for k, v in net.state_dict().items()},
                        {k: v.cpu() for k, v in batch.items()})["rgb_level1"]
    assert float((img.cpu() - ref).abs().max()) < 1e-4


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_cost_reg_training_stage_equals_its_float64_twin_on_the_steps_own_tensors():
    """Stage-wise arbitration (what the end-to-end numbers cannot show, because a 1e-6 change of a stage's INPUT can flip a mask):
    the cost volume entering cost_reg_i and the gradients arriving at its outputs are captured during one 128x160 step on the
    GPU, the stage is replayed in float64 on the CPU with the network's own modules, and every parameter gradient of the HIP
    stage (MFMA convolutions / dgrad / wgrad, BatchNorm-train kernels) must match it to 2e-5 of its largest element — measured
    6e-7 median / 2e-6 worst, the same as the stage's torch fp32 twin on the CPU (tools/diag_cost_reg_fp64.py)."""
    import copy
    import torch_twins
    from enerf_amd import autograd as A
    dev = torch.device("cuda:0")
    cfg, batch = _train_batch(**TRAIN_CASES["train_small"])
    batch = {k: v.to(dev) for k, v in batch.items()}
    net = _net(cfg).to(dev)
    cap, orig = {}, A.cost_reg_train

    def spy(lib, m, vol):
        i = 1 if m.full else 0
        feat, prob = orig(lib, m, vol)
        cap[i] = {"vol": vol.detach().clone()}
        feat.register_hook(lambda g, i=i: cap[i].__setitem__("g_feat", g.detach().clone()))
        prob.register_hook(lambda g, i=i: cap[i].__setitem__("g_prob", g.detach().clone()))
        return feat, prob
    A.cost_reg_train = spy
    try:
        _loss(net(batch), batch).backward()
    finally:
        A.cost_reg_train = orig
    torch.cuda.synchronize()
    for i in (0, 1):
        m = getattr(net, f"cost_reg_{i}")
        m64 = copy.deepcopy(m).cpu().double().train()
        for p in m64.parameters():
            p.grad = None
        feat, prob = torch_twins.cost_reg_forward(m64, cap[i]["vol"].cpu().double())
        torch.autograd.backward([feat, prob], [cap[i]["g_feat"].cpu().double(), cap[i]["g_prob"].cpu().double()])
        worst = 0.0
        for (n, p), (_, p64) in zip(m.named_parameters(), m64.named_parameters()):
            err = float((p.grad.cpu().double() - p64.grad).abs().max()) / max(float(p64.grad.abs().max()), 1e-30)
            worst = max(worst, err)
            assert err < 2e-5, (i, n, err)
        print(f"cost_reg_{i}: HIP stage vs float64 twin on the step's own tensors, worst parameter {worst:.1e}")


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_full_size_training_step_is_as_close_to_fp64_as_the_reference():
    """BASELINE config 5 at its real shape (dtu_pretrain.yaml: 512x640, 3 views, planes 64,8, full-image rays at both levels:
    327,680 + 20,480 rays) pinned to the REFERENCE: one training step of the unmodified reference network in fp32
    (train_full.npz) and in float64 (train_full_fp64.npz), sparse digests.  Loss and outputs against the fp32 reference; every
    parameter gradient by fp64 arbitration (see _assert_as_close_to_fp64_as_the_reference)."""
    from golden_cases import check_sparse_golden
    dev = torch.device("cuda:0")
    g32, g64 = np.load(os.path.join(GOLDEN, "train_full.npz")), np.load(os.path.join(GOLDEN, "train_full_fp64.npz"))
    cfg, batch = _train_batch(**FULL_TRAIN_CASE)
    batch = {k: v.to(dev) for k, v in batch.items()}
    net = _net(cfg).to(dev)
    out = net(batch)
    loss = _loss(out, batch)
    assert float(loss) == pytest.approx(float(g32["loss"]), rel=1e-4)
    assert float(g64["loss"]) == pytest.approx(float(g32["loss"]), rel=1e-4)
    # 1e-4 like every eval-mode test (round 4 had widened it to 2e-4; measured 9.3e-5 on rgb_level1, 2.6e-5 and below elsewhere —
    # train-mode BatchNorm divides by batch statistics over as few as 80 positions, which is where the forward's fp32 noise grows)
    worst = check_sparse_golden("train_full", {k: v.detach() for k, v in out.items()}, 1e-4)
    loss.backward()
    named = [(n, p.grad) for n, p in net.named_parameters() if p.grad is not None]
    for n, gr in named:                                                # whole-tensor norms against the fp64 run
        n64 = float(g64[f"grad/{n}/norm"])
        if n64 > 1e-9:
            assert abs(float(gr.double().norm()) - n64) <= 0.1 * n64, (n, float(gr.double().norm()), n64)
    dist = _distance_to_fp64(named, g32, g64, sparse=True)
    noise = np.load(os.path.join(GOLDEN, "train_full_noise.npz"))
    stable = _assert_stable_parameters_elementwise(named, g32, g64, noise, sparse=True, what="512x640")
    assert len(stable) >= 28, stable                    # the parameters the reference's own 1-ulp draws leave within 1e-4 of float64
    print("512x640 outputs vs reference fp32:", {k: f"{v:.1e}" for k, v in worst.items()})
    print(f"512x640: {len(stable)} stable parameters element-wise within 3e-4 of the reference's fp32 gradients")
    print("512x640 fp64 arbitration (ours, reference):",
          _assert_as_close_to_fp64_as_the_reference(dist, noise, what="512x640"))


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_graphed_training_step_equals_eager_steps():
    """enerf_amd/train_graph.py: three optimizer steps as hipGraph replays (a different batch each step) leave the same
    parameters, BatchNorm statistics and losses as three eager steps (differences: fp32 atomics order only)."""
    from enerf_amd.train_graph import GraphedTrainStep
    dev = torch.device("cuda:0")
    batches = []
    for seed in (7, 8, 9):
        cfg, b = _train_batch(seed=seed)
        batches.append({k: v.to(dev) for k, v in b.items()})
    nets = [_net(cfg).to(dev) for _ in range(2)]
    opts = [torch.optim.SGD(n.parameters(), lr=1e-3, momentum=0.9) for n in nets]   # (Adam's sign-like first steps amplify atomics-order noise)
    from enerf_amd.train_graph import mse_loss
    tree_loss = lambda out, b: sum(LOSS_W[i] * mse_loss(b[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
    gstep = GraphedTrainStep(nets[0], opts[0], tree_loss, batches[0], clip_value=40.0, warmup=1)   # verify=True: replays vs eager
    # warm-up, capture and verification ran real optimizer steps on batches[0]; the constructor must have undone them:
    # parameters, BatchNorm running statistics and num_batches_tracked equal the untouched twin, optimizer state is zero
    for k, v in nets[1].state_dict().items():
        assert torch.equal(nets[0].state_dict()[k], v), f"GraphedTrainStep construction changed {k}"
    for st in opts[0].state.values():
        for v in st.values():
            if torch.is_tensor(v):
                assert float(v.abs().max()) == 0.0
    losses = [[], []]
    for b in batches:
        losses[0].append(float(gstep(b)))
        out = nets[1](b)
        loss = _loss(out, b)
        opts[1].zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(nets[1].parameters(), 40.0)
        opts[1].step()
        losses[1].append(float(loss))
    assert losses[0] == pytest.approx(losses[1], rel=1e-4), losses
    assert len(set(round(x, 6) for x in losses[0])) == 3              # three different batches really went through
    sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
    for k in sd1:
        if sd1[k].dtype.is_floating_point:
            assert float((sd0[k] - sd1[k]).abs().max()) <= 1e-5 + 1e-4 * float(sd1[k].abs().max()), k
    nets[0].eval()
    with torch.no_grad():
        img = nets[0](batches[0])["rgb_level1"]                         # eval after graphed training: re-packed weights
    assert torch.isfinite(img).all()


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_graphed_steps_per_source_view_count_equal_eager_steps():
    """train_graph.GraphedTrainSteps: the trainer draws S in {2,3,4} per sample (dtu_pretrain.yaml:71-72) — one captured graph
    per shape, all on the same parameters and optimizer state.  Five steps alternating S = 3, 2, 3, 4, 2 as replays leave the
    parameters, BatchNorm statistics and losses of five eager steps."""
    from enerf_amd.train_graph import GraphedTrainSteps, mse_loss
    dev = torch.device("cuda:0")
    by_s = {}
    for S_ in (2, 3, 4):
        cfg, b = _train_batch(seed=30 + S_, S=S_)
        by_s[S_] = {k: v.to(dev) for k, v in b.items()}
    nets = [_net(cfg).to(dev) for _ in range(2)]
    opts = [torch.optim.SGD(n.parameters(), lr=1e-3, momentum=0.9) for n in nets]
    tree_loss = lambda out, b: sum(LOSS_W[i] * mse_loss(b[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
    gsteps = GraphedTrainSteps(nets[0], opts[0], tree_loss, [by_s[3], by_s[2], by_s[4]], clip_value=40.0, warmup=1)
    assert len(gsteps.steps) == 3
    for k, v in nets[1].state_dict().items():                           # three constructions, no net change
        assert torch.equal(nets[0].state_dict()[k], v), k
    losses = [[], []]
    for S_ in (3, 2, 3, 4, 2):
        b = by_s[S_]
        losses[0].append(float(gsteps(b)))
        loss = _loss(nets[1](b), b)
        opts[1].zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_(nets[1].parameters(), 40.0)
        opts[1].step()
        losses[1].append(float(loss))
    assert losses[0] == pytest.approx(losses[1], rel=1e-4), losses
    sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
    for k in sd1:
        if sd1[k].dtype.is_floating_point:
            assert float((sd0[k] - sd1[k]).abs().max()) <= 1e-5 + 1e-4 * float(sd1[k].abs().max()), k
    with pytest.raises(KeyError, match="no graph was captured"):
        gsteps({k: (v[:, :1] if k.startswith("rays_") or k.startswith("rgb_") else v) for k, v in by_s[3].items()})


def _graphed_data_parallel_body():
    """(runs in a child process: see test_graphed_data_parallel_step_captures_its_collectives)
    train_graph.GraphedTrainStep(distributed=True) on a 1-rank RCCL group (a 1-GPU box cannot hold two ranks): the flat
    gradient all-reduce and the cost-volume networks' SyncBatchNorm statistics exchanges (forced on for the 1-rank group) are
    RCCL kernels INSIDE the captured graph; the replays must equal eager steps (the constructor verifies that, and three
    further steps are compared with an eager twin here)."""
    import torch.distributed as tdist
    from enerf_amd import autograd as A
    from enerf_amd.train_graph import GraphedTrainStep, mse_loss
    dev = torch.device("cuda:0")
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(30300 + os.getpid() % 2000))
    tdist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    A.SYNC_SINGLE_RANK = True
    try:
        batches = []
        for seed in (7, 8, 9):
            cfg, b = _train_batch(seed=seed)
            batches.append({k: v.to(dev) for k, v in b.items()})
        nets = [torch.nn.SyncBatchNorm.convert_sync_batchnorm(_net(cfg)).to(dev) for _ in range(2)]     # trainer.py:16
        assert isinstance(nets[0].cost_reg_0.conv0.bn, torch.nn.SyncBatchNorm)
        opts = [torch.optim.SGD(n.parameters(), lr=1e-3, momentum=0.9) for n in nets]
        tree_loss = lambda out, b: sum(LOSS_W[i] * mse_loss(b[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
        calls = {"n": 0}
        real = tdist.all_reduce

        def counting(*a, **k):
            calls["n"] += 1
            return real(*a, **k)
        tdist.all_reduce = counting
        try:
            gstep = GraphedTrainStep(nets[0], opts[0], tree_loss, batches[0], clip_value=40.0, warmup=1, distributed=True)
        finally:
            tdist.all_reduce = real
        # per ENQUEUED step (1 warm-up + the capture + 4 eager verification steps; replays issue none from Python): one flat
        # gradient all-reduce + two exchanges per BatchNorm3d layer of the two cost-volume networks (7 + 10 layers)
        assert calls["n"] >= 6 * (1 + 2 * 17), calls
        losses = [[], []]
        for b in batches:
            losses[0].append(float(gstep(b)))
            loss = _loss(nets[1](b), b)
            opts[1].zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_value_(nets[1].parameters(), 40.0)
            opts[1].step()
            losses[1].append(float(loss))
        assert losses[0] == pytest.approx(losses[1], rel=1e-4), losses
        sd0, sd1 = nets[0].state_dict(), nets[1].state_dict()
        for k in sd1:
            if sd1[k].dtype.is_floating_point:
                assert float((sd0[k] - sd1[k]).abs().max()) <= 1e-5 + 1e-4 * float(sd1[k].abs().max()), k
    finally:
        A.SYNC_SINGLE_RANK = False
        tdist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_graphed_data_parallel_step_captures_its_collectives():
    """The graphed data-parallel step with its RCCL collectives inside the capture (_graphed_data_parallel_body), in a CHILD
    process: a process group's helper threads and a stream capture in one process are a known hazard (an illegal call from
    another thread during a capture aborts the process; train_graph.py guards against the case seen here) — an abort there
    must fail this one test, not take the whole pytest session down.  One retry for the same reason."""
    import subprocess
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_training as T; T._graphed_data_parallel_body(); print('DP_GRAPH_OK')" % (
        os.path.dirname(HERE) if os.path.basename(HERE) == "tests" else HERE, os.path.join(os.path.dirname(os.path.abspath(__file__))))
    last = None
    for attempt in range(2):
        last = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), text=True,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
        if last.returncode == 0 and "DP_GRAPH_OK" in last.stdout:
            return
    raise AssertionError(f"child rc={last.returncode}\n{last.stdout[-3000:]}")


def _check_mlp_backward(lib, dev):
    """enerf_nerf_mlp_bwd + enerf_gemm_wgrad (NerfMlpFn) against torch autograd through the module's own layers, for both
    MLP widths (F = 11: level 1, F = 35: level 0) and S = 2, 3, 4 views; ragged point counts."""
    import torch_twins as T
    from enerf_amd.autograd import nerf_mlp
    from enerf_amd.network import NerfParams
    g = torch.Generator().manual_seed(11)
    torch.manual_seed(11)                                   # NerfParams draws its kaiming init from the global generator
    # (F = 11: the per-view layers' weight gradients come from inside the kernel — S <= 3: colour + aggregation branch, S = 4: colour branch)
    for F, S, P, vda in ((11, 3, 37, True), (11, 4, 16, True), (11, 2, 70, True), (11, 3, 21, False), (35, 2, 21, True), (35, 4, 33, True)):
        m = NerfParams(F, vda).to(dev)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 1:
                    p.copy_(torch.randn(p.shape, generator=g).to(dev) * 0.1)
        vox = torch.randn(1, P, 8, generator=g).to(dev).requires_grad_(True)
        x = torch.randn(1, P, S, F + 4, generator=g).to(dev).requires_grad_(True)
        gout = torch.randn(1, P, 4, generator=g).to(dev)
        ref = T.nerf_forward(m, vox, x)
        ref.backward(gout)
        want = {n: p.grad.clone() for n, p in m.named_parameters()}
        gv, gx = vox.grad.clone(), x.grad.clone()
        for p in m.parameters():
            p.grad = None
        vox.grad = x.grad = None
        out = nerf_mlp(lib, m, None, vox, x)
        assert float((out - ref.detach()).abs().max()) <= 2e-5 * float(ref.abs().max())       # HIP forward (enerf_nerf_mlp_fwd)
        out.backward(gout)
        tol = lambda r: 5e-4 * float(r.abs().max()) + 1e-6
        assert float((vox.grad - gv).abs().max()) <= tol(gv), (F, S, "vox")
        assert float((x.grad - gx).abs().max()) <= tol(gx), (F, S, "x")
        for n, p in m.named_parameters():
            assert p.grad is not None, n
            assert float((p.grad - want[n]).abs().max()) <= tol(want[n]), (F, S, n)


def test_mlp_backward_emulated():
    from emu_lib import emu_lib
    _check_mlp_backward(emu_lib(), torch.device("cpu"))


def test_tree_reductions_match_torch():
    """train_graph.tree_sum / mse_loss (the single-block reductions a captured training step uses) equal torch's, values and
    gradients, for sizes that are not multiples of 256."""
    from enerf_amd.train_graph import mse_loss, tree_sum
    g = torch.Generator().manual_seed(3)
    for n in (1, 255, 256, 257, 70001):
        x = torch.randn(n, generator=g, dtype=torch.float64).requires_grad_(True)
        s = tree_sum(x)
        assert float(s) == pytest.approx(float(x.sum()), rel=1e-12, abs=1e-12)
        (gx,) = torch.autograd.grad(s, x)
        assert torch.equal(gx, torch.ones_like(x))
    a = torch.randn(1000, 77, generator=g, requires_grad=True)
    b = torch.randn(1000, 77, generator=g)
    l1, l2 = mse_loss(a, b), F.mse_loss(a, b)
    assert float(l1) == pytest.approx(float(l2), rel=1e-6)
    (g1,), (g2,) = torch.autograd.grad(l1, a), torch.autograd.grad(l2, a)
    assert float((g1 - g2).abs().max()) < 1e-9


# ---- multi-step trajectories of the reference's trainer loop (tests/golden/train_traj_*.npz) --------------------
TRAJ_CASES = {"train_traj_tiny": dict(H=32, W=64, planes=(8, 8), seed=50), "train_traj_small": dict(H=64, W=96, planes=(16, 8), seed=70)}


def _traj_batch(case, step, dev=None):
    """Batch `step` of a trajectory case: the generator's (oracle/make_golden.py::traj_batch) — seed = case seed + step."""
    c = TRAJ_CASES[case]
    cfg, b = _train_batch(seed=c["seed"] + step, H=c["H"], W=c["W"], planes=c["planes"])
    return cfg, ({k: v.to(dev) for k, v in b.items()} if dev is not None else b)


def _reference_optimizer(net, **kw):
    """lib/train/optimizer.py make_optimizer under dtu_pretrain.yaml: Adam, lr 5e-4, eps 1e-8, weight_decay 0."""
    return torch.optim.Adam(net.parameters(), lr=5e-4, eps=1e-8, weight_decay=0.0, **kw)


def _trainer_step(net, opt, batch):
    """trainer.py:56-63."""
    loss = _loss(net(batch), batch)
    opt.zero_grad()
    loss.backward()
    torch.nn.utils.clip_grad_value_(net.parameters(), 40)
    opt.step()
    return float(loss)


def _assert_tracks_reference_trajectory(losses, g, what, slack=3.0, floor=1e-4):
    """The trajectory criterion, calibrated on the reference ITSELF (as the fp64 arbitration is): ten Adam steps from a random
    initialisation are chaotic at fp32 resolution — the unmodified reference, re-run with its source images perturbed by ONE ULP,
    leaves its own loss curve by up to 8e-3 (32x64) / 2.6e-3 (64x96) within ten steps (`noise/loss_rel`: 6 draws; Adam's first
    updates are +-lr whatever the gradient's size, so a sign flip of a near-zero gradient moves a weight by 5e-4).  The literal
    "within 1e-3 per step" of VERDICT r04 #6 is therefore violated by the reference against itself; asserted instead: at every
    step our loss is no further from the reference's than `slack` x its worst own draw (+ a floor for the first steps, where the
    draws agree to the last digit)."""
    noise = g["noise/loss_rel"].max(0)
    dev_ = np.array([abs(a - r) / r for a, r in zip(losses, g["loss"])])
    allowed = slack * noise[: len(dev_)] + floor
    assert (dev_ <= allowed).all(), (what, dev_.round(6).tolist(), allowed.round(6).tolist())
    return float((dev_ / allowed).max())


def _check_final_state(net, g, case, dev=None, slack=3.0):
    """Final parameter norms, BatchNorm running statistics and the trained network's eval-mode frame against the reference's,
    each within `slack` x what the reference's own one-ulp draws move them (+ a floor)."""
    pn_allowed = slack * float(g["noise/pnorm_rel"].max()) + 1e-4
    for name, p in net.named_parameters():
        ref = float(g[f"pnorm/{name}"])
        assert abs(float(p.detach().double().norm()) - ref) <= pn_allowed * max(ref, 1e-6), (case, name)
    buf_allowed = slack * float(g["noise/buf_rel"].max()) + 1e-4
    for name, buf in net.named_buffers():
        if f"buf/{name}" in g.files and buf.dtype.is_floating_point:
            ref = g[f"buf/{name}"]
            assert float(np.abs(buf.cpu().numpy() - ref).max()) <= buf_allowed * float(np.abs(ref).max()), (case, name)
        elif f"buf/{name}" in g.files:
            assert int(buf) == int(g[f"buf/{name}"]), (case, name)                     # num_batches_tracked: exact
    net.eval()
    with torch.no_grad():
        _, held = _traj_batch(case, 1000, dev)
        if dev is None and net._lib is None:                    # CPU tensors, no emulator injected (the twins test): the eval-mode
            from oracle import enerf_oracle as O                # frame of these weights through the oracle (pinned to the reference)
            out = O.forward(net.cfg, {k: v.detach() for k, v in net.state_dict().items()}, held)
        else:
            out = net(held)
    worst = {}
    for k in [k[5:] for k in g.files if k.startswith("eval/")]:
        ref = g["eval/" + k]
        err = float(np.abs(out[k].cpu().numpy() - ref).max()) / max(float(np.abs(ref).max()), 1e-12)
        allowed = slack * float(g[f"noise/eval/{k}"].max()) + 1e-4
        assert err <= allowed, (case, k, err, allowed)              # the frame of OUR trained network vs the reference's trained network
        worst[k] = round(err / allowed, 3)
    net.train()
    return worst


def test_reference_trajectories_are_chaotic_at_fp32_resolution():
    """Why the trajectory tests are not a plain 1e-3 bound: the fixtures' own noise records (the unmodified reference re-run under
    one-ulp input perturbations) exceed it."""
    for case in TRAJ_CASES:
        g = np.load(os.path.join(GOLDEN, case + ".npz"))
        assert g["noise/loss_rel"].shape == (6, 10)
        assert g["noise/loss_rel"].max() > 1e-3 and g["noise/loss_rel"][:, 0].max() < 1e-6


@pytest.mark.parametrize("case", list(TRAJ_CASES))
def test_trainer_loop_of_the_torch_twins_tracks_the_reference_trajectory(case):
    """Ten iterations of the reference's trainer loop (zero_grad, backward, clip_grad_value_ 40, its Adam) on ten different
    batches through the torch twins + torch.optim.Adam as this repository configures it: identical to the unmodified reference for
    the first steps (same ops, same order: 1e-6) and inside the reference's own spread afterwards; pins the STEP SEQUENCE —
    running statistics, momentum, clipping, parameter updates — next to the per-stage pins of the HIP kernels."""
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    torch.set_num_threads(1)
    cfg, _ = _traj_batch(case, 0)
    net = _net(cfg, twins=True)
    opt = _reference_optimizer(net)
    losses = [_trainer_step(net, opt, _traj_batch(case, s)[1]) for s in range(int(g["meta/steps"]))]
    assert losses[:2] == pytest.approx(list(g["loss"][:2]), rel=2e-6)
    _assert_tracks_reference_trajectory(losses, g, case)
    _check_final_state(net, g, case)


def test_hip_training_trajectory_tracks_the_reference_emulated():
    """The same loop on the HIP training path (CPU lane emulator; the full ten steps at both sizes run on the GPU): the first
    three steps of the 32x64 trajectory — weight re-packing, BatchNorm running statistics and the optimizer state carried from
    step to step."""
    from emu_lib import emu_lib
    case = "train_traj_tiny"
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    torch.set_num_threads(1)
    cfg, _ = _traj_batch(case, 0)
    net = Network(cfg, lib=emu_lib())
    net.load_state_dict(load_weights(), strict=False)
    net.train()
    opt = _reference_optimizer(net)
    losses = [_trainer_step(net, opt, _traj_batch(case, s)[1]) for s in range(3)]
    assert losses[0] == pytest.approx(float(g["loss"][0]), rel=1e-5)
    _assert_tracks_reference_trajectory(losses, g, case + " (emulator)")


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("graphed", [False, True])
@pytest.mark.parametrize("case", list(TRAJ_CASES))
def test_training_trajectory_on_gpu_tracks_the_reference(case, graphed):
    """ten Adam steps of the reference's trainer loop on the MI355X path — eager steps and ONE hipGraph replay
    per step (GraphedTrainStep, batches copied into the captured buffers) — track the unmodified reference's loss curve inside
    3 x the reference's OWN one-ulp spread at every step (_assert_tracks_reference_trajectory), and the final network (BatchNorm
    statistics, parameter norms, eval-mode frame through the re-packed HIP inference path) stays as close to the reference's final
    network."""
    dev = torch.device("cuda:0")
    g = np.load(os.path.join(GOLDEN, case + ".npz"))
    n = int(g["meta/steps"])
    cfg, b0 = _traj_batch(case, 0, dev)
    net = _net(cfg).to(dev)
    if graphed:
        from enerf_amd.train_graph import GraphedTrainStep, mse_loss
        opt = _reference_optimizer(net, capturable=True)
        tree_loss = lambda out, b: sum(LOSS_W[i] * mse_loss(b[f"rgb_{i}"], out[f"rgb_level{i}"]) for i in range(2))
        gstep = GraphedTrainStep(net, opt, tree_loss, b0, clip_value=40.0, warmup=1)
        losses = [float(gstep(_traj_batch(case, s, dev)[1])) for s in range(n)]
    else:
        opt = _reference_optimizer(net)
        losses = [_trainer_step(net, opt, _traj_batch(case, s, dev)[1]) for s in range(n)]
    worst = max(abs(a - r) / r for a, r in zip(losses, g["loss"]))
    frac = _assert_tracks_reference_trajectory(losses, g, f"{case} graphed={graphed}")
    fin = _check_final_state(net, g, case, dev)
    print(f"{case} graphed={graphed}: worst relative loss deviation over {n} steps {worst:.2e} ({frac:.2f} of the allowed envelope = 3 x the "
          f"reference's own one-ulp spread); final eval frame / allowed: {fin}")
