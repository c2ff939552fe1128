"""Cases of the composite network's backward kernels (k_feature_volume_bwd<CQ, true>, k_depth_regression_bwd<MK, true>,
k_composite_layers_bwd), shared by the emulator tests (test_composite_train.py) and the MI355X tests (test_composite_train_gpu.py):
every function takes the library and the device and asserts.

    window_warp_bwd_case         grad_depth_values is the full-grid backward's on a zero-padded grad_vol inside the window, bit for
                                 bit, and 0 outside; volume, grad_feat and grad_depth_values against float64 autograd of
                                 torch_twins.feature_volume sliced to the window, by the rule of backward_cases.py
    window_regression_bwd_case   grad_prob / grad_depth_values are those of the plain backward on the zero-padded prob, bit for bit
    layers_bwd_case              the layer merge's gradients against float64 autograd of composite_cases.composite_reference,
                                 bound 4 d32 + 16 * 2^-24 (backward_cases' rule); every row written; the same bits twice
    bwd_refusals                 every new entry validates before it launches
    train_step_case              one training step (forward, EnerfLoss, backward) against the unmodified reference's fixtures
    surface cases                the opt-in constructor argument, the packed images and the source cache after an optimizer step
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import backward_cases as BC          # noqa: E402
import composite_cases as CC         # noqa: E402
import torch_twins as T              # noqa: E402

WINDOWS = CC.WINDOWS
GRID_H, GRID_W = CC.GRID_H, CC.GRID_W
SHIFTABLE = (3, 2, 4, 4)             # the window the sensitivity check moves by one pixel


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(a, b), (what, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. windowed warp + variance backward
class WindowWarpCase(BC.WarpCase):
    """WarpCase "unit" (one texel per voxel step: the neighbour merge is on) on the 8 x 12 grid with D = 4, S = 2, B = 1 and per-pixel
    random planes; volume and upstream gradient exist only inside ``win``."""

    def __init__(self, C, win):
        self.kind, self.C, self.B, self.S, self.src, self.vol, self.win = "unit", C, 1, 2, (9, 13), (4, GRID_H, GRID_W), tuple(win)
        self.proj = BC._rigid(self.B, self.S, BC._unit_step)
        self.key, self.label = ("window_warp", C, self.win), f"window {self.win} C={C}"
        self.seed0 = 4100 + C + 17 * WINDOWS.index(self.win)

    def inputs(self, seed, dev):
        g = torch.Generator().manual_seed(seed)
        B, S, C, (Hs, Ws), (D, h, w) = self.B, self.S, self.C, self.src, self.vol
        x0, y0, ww, wh = self.win
        feats = torch.randn(B, S, C, Hs, Ws, generator=g)
        dv = torch.linspace(500.0, 800.0, D).view(1, D, 1, 1).expand(B, D, h, w) + 3.0 * torch.randn(B, D, h, w, generator=g)
        gout = torch.randn(B, C, D, wh, ww, generator=g)
        inp = dict(feats=feats.to(dev), dv=dv.contiguous().to(dev), proj=self.proj.to(dev), count=B * D * wh * ww)
        _, _, pz, u, v = BC.warp_coords(inp["proj"], inp["dv"])
        near = ((BC.near_integer(u, -1, Ws) | BC.near_integer(v, -1, Hs)) & (u >= -2) & (u <= Ws + 1) & (v >= -2) & (v <= Hs + 1)) | \
            ((pz - 1e-6).abs() <= BC.NEAR * pz.abs().clamp_min(1.0))
        near = near.any(1)[:, :, y0:y0 + wh, x0:x0 + ww]                            # (B,D,wh,ww): the window's voxels
        inp["masked"] = int(near.sum())
        inp["gout"] = gout.to(dev) * (~near)[:, None]
        return inp

    def twin(self, inp, dtype, gout=None, win=None):
        """``win``: the window the twin slices (the sensitivity defect: another one of the same size)."""
        x0, y0, ww, wh = self.win if win is None else win
        feats, dv = BC.leaf(inp["feats"], dtype), BC.leaf(inp["dv"], dtype)
        vol = T.feature_volume(feats, inp["proj"].to(dtype), dv)[:, :, :, y0:y0 + wh, x0:x0 + ww]
        vol.backward((inp["gout"] if gout is None else gout).to(dtype))
        return {"volume": vol.detach(), "g_feats": feats.grad, "g_dv": dv.grad}

    def hip(self, lib, inp, gout=None):
        from enerf_amd.autograd import WindowFeatureVolumeFn
        feats, dv = BC.leaf(inp["feats"]), BC.leaf(inp["dv"])
        vol = WindowFeatureVolumeFn.apply(lib, feats, inp["proj"].contiguous(), dv, self.win)
        vol.backward(inp["gout"] if gout is None else gout)
        return {"volume": vol.detach(), "g_feats": feats.grad, "g_dv": dv.grad}


def window_warp_bwd_case(lib, dev, C, win, worst=None):
    case = WindowWarpCase(C, win)
    x0, y0, ww, wh = win
    inp, r64, sc, d32 = BC.yardstick(case, dev)                 # (asserts ``capped`` on this draw)
    D, h, w = case.vol
    nvw = 64 // (C // 4)
    sparse = torch.zeros_like(inp["gout"])                      # an upstream gradient that fills no wave: three voxels
    for (d, y, x) in ((0, 0, 0), (1, wh - 1, ww - 1), (D - 1, wh // 2, 1)):
        sparse[:, :, d, y, x] = inp["gout"][:, :, d, y, x]
    assert int((sparse.abs().sum(1) > 0).sum()) <= 3 < nvw
    for what, gout in (("dense", inp["gout"]), ("sparse", sparse)):
        hip = case.hip(lib, inp, gout)
        # (a) inside the window: the full-grid backward on the zero-padded upstream gradient, bit for bit; (b) outside: 0
        padded = torch.zeros(1, C, D, h, w, device=dev)
        padded[:, :, :, y0:y0 + wh, x0:x0 + ww] = gout
        feat_cl = inp["feats"].permute(0, 1, 3, 4, 2).contiguous()
        _, full_gdv = lib.build_feature_volume_bwd(feat_cl, inp["proj"].contiguous(), inp["dv"], padded.permute(0, 2, 3, 4, 1).contiguous())
        inside = torch.zeros(h, w, dtype=torch.bool, device=dev)
        inside[y0:y0 + wh, x0:x0 + ww] = True
        _same(hip["g_dv"][..., inside], full_gdv[..., inside], ("g_dv inside", C, win, what))
        assert float(full_gdv.abs().max()) > 0 and bool((hip["g_dv"][..., ~inside] == 0).all()), (C, win, what)
        # (c) against float64
        if what == "dense":
            ratio = BC.compare(case, hip, dev)
            if worst is not None:
                worst["warp"] = max(worst.get("warp", 0.0), ratio)
        else:
            ref, bd = case.twin(inp, torch.float64, gout=sparse), BC.bounds(d32)
            for k in ref:
                err = BC.distance(hip[k], ref[k], sc[k])
                assert err <= bd[k], (C, win, what, k, err, bd[k])
    if tuple(win) == SHIFTABLE:         # sensitivity, on the reference alone: the window one pixel to the right, one pixel down
        for moved_win in ((x0 + 1, y0, ww, wh), (x0, y0 + 1, ww, wh)):
            mv = BC.moved(case, dev, case.twin(inp, torch.float64, win=moved_win), keys=("g_feats", "g_dv"))
            assert mv > 10, (moved_win, mv)
            print(f"[window warp] C={C} sensitivity: the window at {moved_win[:2]} moves a gradient by {mv:.0f} bounds")


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. windowed depth regression backward
def regression_kernel(D):
    return "k_depth_regression_bwd<4, true>" if D <= 16 else "k_depth_regression_bwd<16, true>"


def window_regression_bwd_case(lib, dev, D, depth_inv):
    from enerf_amd.autograd import WindowDepthRegressionFn
    h, w = GRID_H, GRID_W
    g = torch.Generator().manual_seed(4200 + D + int(depth_inv))
    dv = (0.3 + 2.0 * torch.rand(1, D, h, w, generator=g)).to(dev)
    for win in WINDOWS:
        x0, y0, ww, wh = win
        prob = (3.0 * torch.randn(1, D, wh, ww, generator=g)).to(dev)
        g_depth, g_std = torch.randn(1, h, w, generator=g).to(dev), torch.randn(1, h, w, generator=g).to(dev)     # the whole image
        padded = torch.zeros(1, D, h, w, device=dev)
        padded[:, :, y0:y0 + wh, x0:x0 + ww] = prob
        want_p, want_dv = lib.depth_regression_bwd(padded, dv, g_depth, g_std, depth_inv)
        pl, dl = BC.leaf(prob), BC.leaf(dv)
        depth, std = WindowDepthRegressionFn.apply(lib, pl, dl, depth_inv, win)
        ((depth * g_depth).sum() + (std * g_std).sum()).backward()
        assert float(want_p.abs().max()) > 0 and float(want_dv.abs().max()) > 0
        _same(pl.grad, want_p[:, :, y0:y0 + wh, x0:x0 + ww].contiguous(), ("g_prob", D, depth_inv, win))
        _same(dl.grad, want_dv, ("g_dv", D, depth_inv, win))
        if (ww, wh) != (w, h):           # outside the window the upstream gradient arrives: the uniform softmax passes it to dv
            outside = torch.ones(h, w, dtype=torch.bool, device=dev)
            outside[y0:y0 + wh, x0:x0 + ww] = False
            assert float(dl.grad[..., outside].abs().min()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. layer merge + composite backward
IMG_H, IMG_W = CC.IMG_H, CC.IMG_W
LAYER_SEEDS = BC.SEEDS


def _upstream(L, ns, seed):
    g = torch.Generator().manual_seed(4300 + seed)
    N, Tt = IMG_H * IMG_W, (L + 1) * ns
    return torch.randn(N, 3, generator=g), 0.1 * torch.randn(N, generator=g), torch.randn(N, Tt, generator=g)


def _layers_reference(fg, windows, bg, ups, white, dtype):
    """Autograd of composite_reference in ``dtype``: the gradients of every layer's and the background's raw; ups entries may be None."""
    raws = [BC.leaf(r, dtype) for r, _ in fg] + [BC.leaf(bg[0], dtype)]
    out = CC.composite_reference([(r, z.to(dtype)) for r, (_, z) in zip(raws[:-1], fg)], windows, (raws[-1], bg[1].to(dtype)), IMG_H, IMG_W,
                                 white)
    loss = sum((out[k] * u.to(dtype)).sum() for k, u in zip(("rgb", "depth", "weights"), ups) if u is not None)
    grads = torch.autograd.grad(loss, raws, allow_unused=True)
    res = {f"g_fg{l}": gr if gr is not None else torch.zeros_like(raws[l]) for l, gr in enumerate(grads[:-1])}
    res["g_bg"] = grads[-1]
    return res


_LAYER_YARD = {}


def _layers_yardstick(L, name, ns, white):
    """(inputs and upstream gradients of seed 0, float64 reference, scales, d32 per tensor over LAYER_SEEDS seeds); CPU, computed once."""
    key = (L, name, ns, white)
    if key not in _LAYER_YARD:
        d32, first = {}, None
        for seed in range(LAYER_SEEDS):
            fg, windows, bg = CC.composite_inputs(L, name, ns, seed=seed)
            ups = _upstream(L, ns, seed)
            r64 = _layers_reference(fg, windows, bg, ups, white, torch.float64)
            r32 = _layers_reference(fg, windows, bg, ups, white, torch.float32)
            zmax = max(float(z.abs().max()) for _, z in list(fg) + [bg])
            nat = float(ups[0].abs().max()) + float(ups[2].abs().max()) + float(ups[1].abs().max()) * zmax          # CompositeCase.natural
            sc = BC.scales(r64, {k: nat for k in r64})
            for k in r64:
                d32[k] = max(d32.get(k, 0.0), BC.distance(r32[k], r64[k], sc[k]))
            if seed == 0:
                first = (fg, windows, bg, ups, r64, sc)
        _LAYER_YARD[key] = first + (d32,)
    return _LAYER_YARD[key]


def layers_bwd_case(lib, dev, L, name, ns, worst=None):
    to = lambda pair: tuple(t.to(dev).contiguous() for t in pair)
    for white in (False, True):
        fg, windows, bg, ups, r64, sc, d32 = _layers_yardstick(L, name, ns, white)
        bd = BC.bounds(d32)
        dfg, dbg, dups = [to(f) for f in fg], to(bg), [u.to(dev) for u in ups]

        def run(u):
            out = ([torch.full_like(r, float("nan")) for r, _ in dfg], torch.full_like(dbg[0], float("nan")))     # every row is written
            g_fg, g_bg = lib.composite_layers_bwd(dfg, windows, dbg, IMG_H, IMG_W, *u, white_bkgd=white, out=out)
            res = {f"g_fg{l}": t for l, t in enumerate(g_fg)}
            res["g_bg"] = g_bg
            for k, t in res.items():
                assert bool(torch.isfinite(t).all()), (L, name, ns, white, k)
            return res

        def check(got, ref, what):
            for k in ref:
                err = BC.distance(got[k].cpu(), ref[k], sc[k])
                if worst is not None:
                    worst["layers"] = max(worst.get("layers", 0.0), err / bd[k])
                assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
                assert err <= bd[k], f"L={L} {name} Ns={ns} white={int(white)} {what}: {k} rel err {err:.3e} > {bd[k]:.3e} (d32 {d32[k]:.3e})"
            return max(BC.distance(got[k].cpu(), ref[k], sc[k]) / bd[k] for k in ref)

        got = run(dups)
        ratio = check(got, r64, "all three")
        print(f"[layers bwd] L={L} {name} Ns={ns} white={int(white)}: worst hip/bound {ratio:.2f}; d32 " +
              ", ".join(f"{k} {v:.1e}" for k, v in d32.items()))
        again = run(dups)
        for k in got:
            _same(got[k], again[k], ("layers bwd twice", L, name, ns, white, k))
        for absent in range(3):             # each upstream gradient absent once: NULL is zeros bit for bit, and the reference agrees
            with_none = run([None if i == absent else u for i, u in enumerate(dups)])
            with_zero = run([torch.zeros_like(u) if i == absent else u for i, u in enumerate(dups)])
            for k in got:
                _same(with_none[k], with_zero[k], ("layers bwd absent", absent, L, name, ns, white, k))
            ref = _layers_reference(fg, windows, bg, [None if i == absent else u for i, u in enumerate(ups)], white, torch.float64)
            check(with_none, ref, f"upstream {absent} absent")
        # through the autograd Function: the same bits, no gradient to any depth, net_output / z_vals detached
        from enerf_amd.autograd import CompositeLayersFn
        leaves = [BC.leaf(t) for pair in dfg for t in pair]
        bgl = [BC.leaf(dbg[0]), BC.leaf(dbg[1])]
        rgb, depth, wts, net, zv = CompositeLayersFn.apply(lib, windows, IMG_H, IMG_W, white, *bgl, *leaves)
        assert not net.requires_grad and not zv.requires_grad
        ((rgb * dups[0]).sum() + (depth * dups[1]).sum() + (wts * dups[2]).sum()).backward()
        assert bgl[1].grad is None and all(leaves[2 * l + 1].grad is None for l in range(L))
        _same(bgl[0].grad, got["g_bg"], ("Fn g_bg", L, name, ns, white))
        for l in range(L):
            _same(leaves[2 * l].grad, got[f"g_fg{l}"], ("Fn g_fg", l, L, name, ns, white))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. the training step against the unmodified reference (tools/make_golden_composite_train.py writes tests/golden/composite_train_*.npz)
# Case "t": one foreground layer, both levels rendered, windows (4, 0, 8, 8) / (8, 0, 16, 16) of the 8 x 16 / 16 x 32 volume grids; the
# two-layer weights minus the second layer's.  Case "a": composite_cases.NETWORK_CASES["a"] as it is — two overlapping layers, both
# levels rendered, the far range in front: the sort decides the composited order.
# The seed of "t" is chosen on the REFERENCE alone (tools/make_golden_composite_train.py asserts it): the first one from 23 upwards on
# which each of the reference's eight one-ulp draws keeps the median and the 75th percentile of its distances to float64 within 3 x those
# of its single fp32 draw — the bulk rule train_step_case applies to a port.  On 23, 25 and 26 the reference is bimodal there (a
# flipped ReLU mask / floor() moves the median by 150 x in 2 of 8 draws on 23): such a batch cannot pin a bulk figure to one draw.
TRAIN_CASES = {
    "t": dict(H=32, W=64, S=3, L=1, render_if=(True, True), boxes=[(16, 0, 32, 32)], ranges=[(0.2, 0.7), (0.0, 1.0)], seed=24,
              seed_chosen_here=True, drop=("_layer1.",)),
    "a": CC.NETWORK_CASES["a"],
}
TRAIN_FILES = "composite_train_{}_{}.npz"          # case, part: "fp32_out", "fp32_grad", "fp64_out", "fp64_grad" (rounded to float32), "spread"
GRAD_TINY = 1e-12                                  # a parameter whose float64 gradient is below this has no gradient to compare
GRAD_FULL_BELOW, GRAD_STRIDE = 2048, 13            # a gradient of more elements is stored as every 13th (no fixture passes 1 MiB)
ONE_ULP_DRAWS = 8


def train_config(name):
    from enerf_amd.config import EnerfConfig
    return EnerfConfig(viewdir_agg=False).with_cas(volume_planes=(32, 8), num_samples=(2, 1), render_if=TRAIN_CASES[name]["render_if"])


def train_batch(name):
    """composite_cases.network_batch for a TRAIN_CASES entry, plus the targets ``rgb_{i}`` (1, Hr*Wr, 3): seeded, drawn as float32."""
    import numpy as np
    from enerf_amd.synth import make_batch
    c, cfg = TRAIN_CASES[name], train_config(name)
    b = make_batch(c["H"], c["W"], c["S"], cfg, seed=c["seed"], textured=True)
    n, f = float(b["near_far"][0, 0]), float(b["near_far"][0, 1])
    b["near_far"] = np.array([[(n + lo * (f - n), n + hi * (f - n)) for lo, hi in c["ranges"]]], np.float32)
    b["bbox"] = np.array([c["boxes"]], np.float32)
    b["bg_src_inps"] = np.random.default_rng(c["seed"] + 100).uniform(-1, 1, size=b["src_inps"].shape).astype(np.float32)
    rng = np.random.default_rng(c["seed"] + 200)
    for i, on in enumerate(c["render_if"]):
        if on:
            rs = cfg.cas.render_scale[i]
            b[f"rgb_{i}"] = rng.random((1, int(c["H"] * rs) * int(c["W"] * rs), 3), dtype=np.float32)
    return b


def train_weights(name):
    import glob
    import numpy as np
    sd = {}
    for p in sorted(glob.glob(os.path.join(CC.GOLDEN, CC.WEIGHT_FILES.format("*")))):
        z = np.load(p)
        sd.update({k: torch.from_numpy(z[k]) for k in z.files})
    drop = TRAIN_CASES[name].get("drop", ())
    return {k: v for k, v in sd.items() if not any(d in k for d in drop)}


def train_network(lib, dev, name, **kw):
    """A trainable network holding the case's reference weights, in training mode."""
    from enerf_amd.network_composite import Network
    net = Network(train_config(name), TRAIN_CASES[name]["L"], lib=lib, trainable=True, **kw)
    full = dict(net.state_dict())
    full.update(train_weights(name))
    net.load_state_dict(full, strict=True)
    return net.to(dev).train()


def train_loss_fn(name):
    """Σ over rendered levels of MSE(rgb_level{i}, rgb_{i}) as the trainer's loss object (unit weights, no perceptual term)."""
    from enerf_amd.loss import EnerfLoss
    n = train_config(name).cas.num
    return EnerfLoss([1.0] * n, [False] * n, [0] * n, [0] * n, [0] * n)


def train_step_results(lib, dev, name):
    """One forward + loss + backward from the case's weights: (loss, outputs, running statistics after the step, gradients)."""
    net = train_network(lib, dev, name)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in train_batch(name).items()}
    batch["bbox"] = batch["bbox"].cpu()
    before = {k: v.clone() for k, v in batch.items()}
    out = net(batch)
    loss = train_loss_fn(name)(out, batch)
    loss.backward()
    assert set(batch) == set(before) and all(torch.equal(batch[k], before[k]) for k in before), "the batch was mutated"
    stats = {k: v.detach().cpu() for k, v in net.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    grads = {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in net.named_parameters()}
    return float(loss.detach()), {k: v.detach().cpu() for k, v in out.items()}, stats, grads


def load_train_golden(name):
    import numpy as np
    parts = {"fp32": {}, "fp64": {}, "spread": {}}
    for part, files in (("fp32", ("fp32_out", "fp32_grad")), ("fp64", ("fp64_out", "fp64_grad")), ("spread", ("spread",))):
        for f in files:
            z = np.load(os.path.join(CC.GOLDEN, TRAIN_FILES.format(name, f)))
            parts[part].update({k: z[k] for k in z.files})
    return parts


def _rel(a, b):
    """max|a - b| / max|b| (the yardstick of tests/test_training.py::_distance_to_fp64)."""
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-30)


def train_step_case(lib, dev, name, worst=None):
    """The assertions of the issue, on the fixtures' own numbers; prints every figure before it asserts."""
    import numpy as np
    gold = load_train_golden(name)
    g32, g64, spread = gold["fp32"], gold["fp64"], gold["spread"]
    loss, out, stats, grads = train_step_results(lib, dev, name)
    t = lambda a: torch.from_numpy(np.asarray(a))
    # -- loss
    ref_loss = float(g32["loss"])
    e = abs(loss - ref_loss) / abs(ref_loss)
    print(f"[composite train] case {name} loss {loss:.9g} ref32 {ref_loss:.9g} rel {e:.2e}")
    assert e <= 1e-5, (loss, ref_loss)
    # -- outputs and running statistics: max|ours - ref32| <= tol * max|ref|, tol = max(REL_TOL, 3 x the stored one-ulp spread)
    want_out = sorted(k[4:] for k in g32 if k.startswith("out/"))
    assert sorted(out) == want_out, (sorted(out), want_out)
    for kind, ours in (("out", out), ("stat", stats)):
        keys = sorted(k for k in g32 if k.startswith(kind + "/"))
        assert keys and len(keys) == len(ours), (kind, len(keys), len(ours))
        top = 0.0
        for k in keys:
            ref = t(g32[k])
            got = ours[k[len(kind) + 1:]]
            assert got.shape == ref.shape, (k, got.shape, ref.shape)
            tol = max(CC.REL_TOL, 3.0 * float(spread["spread/" + k]))
            err = _rel(got, ref)
            top = max(top, err / tol)
            if kind == "out":
                print(f"[composite train] case {name} {k}: e {err:.2e} tol {tol:.2e}")
            assert err <= tol, (name, k, err, tol)
        print(f"[composite train] case {name}: worst {kind} error / tolerance {top:.2f}")
        if worst is not None:
            worst[f"{name}/{kind}"] = top
    # -- gradients: tests/test_training.py::_assert_as_close_to_fp64_as_the_reference, for this parameter set
    names = sorted(k[5:] for k in g64 if k.startswith("grad/"))
    no_grad = sorted(k for k, g in grads.items() if k not in names)
    assert all(".feat_conv." in k for k in no_grad), no_grad           # the reference leaves exactly these without a gradient
    for k in no_grad:
        assert grads[k] is None or float(grads[k].abs().max()) == 0.0, k
    assert (int(g64["meta/full_below"]), int(g64["meta/stride"])) == (GRAD_FULL_BELOW, GRAD_STRIDE)
    sample = lambda g: g.reshape(-1) if g.numel() <= GRAD_FULL_BELOW else g.reshape(-1)[::GRAD_STRIDE]       # the stored elements
    dist = lambda a, b, scale: float((a.double() - b.double()).abs().max()) / scale
    d_ours, d_ref, d_ulp, mine = {}, {}, {}, {}
    for k in names:
        r64, scale = t(g64["grad/" + k]), float(g64["gradmax/" + k])
        if scale < GRAD_TINY:
            continue
        assert grads[k] is not None and sample(grads[k]).shape == r64.shape, k
        mine[k] = sample(grads[k])
        d_ours[k], d_ref[k] = dist(mine[k], r64, scale), dist(t(g32["grad/" + k]), r64, scale)
        d_ulp[k] = float(spread["ulp/grad/" + k])
    assert len(d_ours) >= len(names) - 8, (len(d_ours), len(names))
    med = lambda v: float(np.median(list(v)))
    q75 = lambda v: float(np.percentile(list(v), 75))
    m_ref = med(d_ref.values())
    ratios = {k: d_ours[k] / (3.0 * max(d_ref[k], d_ulp[k], m_ref)) for k in d_ours}
    kw = max(ratios, key=ratios.get)
    print(f"[composite train] case {name}: {len(d_ours)} parameters; distance to float64: ours median {med(d_ours.values()):.2e} "
          f"p75 {q75(d_ours.values()):.2e} max {max(d_ours.values()):.2e}; reference median {m_ref:.2e} p75 {q75(d_ref.values()):.2e} "
          f"max {max(d_ref.values()):.2e}; worst ours / bound {ratios[kw]:.2f} ({kw}: ours {d_ours[kw]:.2e}, ref {d_ref[kw]:.2e}, "
          f"one-ulp {d_ulp[kw]:.2e})")
    if worst is not None:
        worst[f"{name}/grad"] = ratios[kw]
    for k in d_ours:
        assert ratios[k] <= 1.0, f"{name} {k}: ours {d_ours[k]:.3e} > 3 x max(ref {d_ref[k]:.3e}, one-ulp {d_ulp[k]:.3e}, median {m_ref:.3e})"
        assert d_ours[k] <= 1.5e-1, (name, k, d_ours[k])
    assert med(d_ours.values()) <= 3.0 * m_ref and q75(d_ours.values()) <= 3.0 * q75(d_ref.values())
    # -- parameters the reference holds within 1e-4 of float64 in every draw: element-wise against the fp32 fixture at 3e-4
    stable = [k for k in d_ours if max(d_ref[k], d_ulp[k]) < 1e-4]
    print(f"[composite train] case {name}: {len(stable)} of {len(d_ours)} parameters are stable (compared element-wise)")
    assert stable
    for k in stable:
        err = dist(mine[k], t(g32["grad/" + k]), float(g64["gradmax/" + k]))
        assert err <= 3e-4, (name, k, err)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. refusals
def bwd_refusals(lib, dev):
    """Every new entry validates before it launches (the outputs keep their sentinel)."""
    import pytest
    from enerf_amd.lib import EnerfError
    feat, proj = torch.zeros(1, 2, 8, 12, 16, device=dev), torch.zeros(1, 2, 3, 4, device=dev)
    dv = torch.ones(1, 4, 8, 12, device=dev)
    gv = lambda D, wh, ww, C=16: torch.zeros(1, D, wh, ww, C, device=dev)
    with pytest.raises(EnerfError, match="outside"):
        lib.build_feature_volume_window_bwd(feat, proj, dv, gv(4, 8, 8), (8, 0, 8, 8))
    with pytest.raises(EnerfError, match="divisible by 4"):
        lib.build_feature_volume_window_bwd(feat, proj, dv, gv(4, 8, 6), (0, 0, 6, 8))
    with pytest.raises(EnerfError, match="divisible by 4"):
        lib.build_feature_volume_window_bwd(feat, proj, torch.ones(1, 6, 8, 12, device=dev), gv(6, 8, 8), (0, 0, 8, 8))
    with pytest.raises(EnerfError, match="unsupported"):
        lib.build_feature_volume_window_bwd(torch.zeros(1, 2, 8, 12, 8, device=dev), proj, dv, gv(4, 8, 8, 8), (0, 0, 8, 8))
    with pytest.raises(EnerfError, match="null pointer"):
        lib._check(lib.dll.enerf_build_feature_volume_window_bwd(None, None, None, None, 1, 2, 16, 8, 12, 4, 8, 12, 0, 0, 8, 8, None, None,
                                                                 None), "build_feature_volume_window_bwd")
    with pytest.raises(EnerfError, match="limit 2\\^31"):         # scatter offsets past 32 bits; nothing is read before the refusal
        lib._check(lib.dll.enerf_build_feature_volume_window_bwd(feat.data_ptr(), proj.data_ptr(), dv.data_ptr(), dv.data_ptr(), 1, 2, 16,
                                                                 1 << 13, 1 << 13, 4, 8, 12, 0, 0, 8, 8, feat.data_ptr(), dv.data_ptr(), None),
                   "build_feature_volume_window_bwd")
    gi = torch.zeros(1, 8, 12, device=dev)
    with pytest.raises(EnerfError, match="outside"):
        lib.depth_regression_window_bwd(torch.zeros(1, 4, 4, 4, device=dev), dv, gi, gi, False, (0, 6, 4, 4))
    with pytest.raises(EnerfError, match="divisible by 4"):
        lib.depth_regression_window_bwd(torch.zeros(1, 4, 4, 2, device=dev), dv, gi, gi, False, (0, 0, 2, 4))
    with pytest.raises(EnerfError, match="null pointer"):
        lib._check(lib.dll.enerf_depth_regression_window_bwd(None, None, None, None, 1, 4, 8, 12, 0, 0, 4, 4, 0, None, None, None),
                   "depth_regression_window_bwd")
    z4 = lambda n, ns: (torch.zeros(n, ns, 4, device=dev), torch.zeros(n, ns, device=dev))
    N = IMG_H * IMG_W
    with pytest.raises(EnerfError, match="L\\*n_samples <= 16"):          # L * Ns = 20
        lib.composite_layers_bwd([z4(4, 5)] * 4, [(0, 0, 2, 2)] * 4, z4(N, 5), IMG_H, IMG_W, None, None, None)
    with pytest.raises(EnerfError, match="outside"):
        lib.composite_layers_bwd([z4(6, 1)], [(8, 4, 3, 2)], z4(N, 1), IMG_H, IMG_W, None, None, None)
    with pytest.raises(EnerfError, match="null args"):
        lib._check(lib.dll.enerf_composite_layers_bwd(None, None), "composite_layers_bwd")
    sent = ([torch.full((6, 1, 4), 7.0, device=dev)], torch.full((N, 1, 4), 7.0, device=dev))
    with pytest.raises(EnerfError, match="outside"):
        lib.composite_layers_bwd([z4(6, 1)], [(8, 4, 3, 2)], z4(N, 1), IMG_H, IMG_W, None, None, None, out=sent)
    assert bool((sent[0][0] == 7.0).all()) and bool((sent[1] == 7.0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the public surface
def surface_optin_case(lib, dev):
    """A default-constructed network still refuses training mode; a trainable one returns the reference's keys; the cached entries refuse
    training mode on both."""
    import pytest
    from enerf_amd.network_composite import Network
    name = "t"
    batch = {k: torch.from_numpy(v).to(dev) for k, v in train_batch(name).items()}
    batch["bbox"] = batch["bbox"].cpu()
    plain = Network(train_config(name), TRAIN_CASES[name]["L"], lib=lib).to(dev)
    with pytest.raises(RuntimeError, match="inference only"):
        plain.train()(batch)
    net = train_network(lib, dev, name)
    out = net(batch)
    want = {f"{k}_level{i}" for i in (0, 1) for k in ("rgb", "depth", "weights", "net_output", "z_vals")}      # the reference's, minus idx
    assert set(out) == want, sorted(set(out) ^ want)
    for k, v in out.items():
        assert v.requires_grad == k.startswith(("rgb", "depth", "weights")), k
    views = (batch["src_inps"][0], batch["bg_src_inps"][0], batch["src_exts"][0], batch["src_ixts"][0])
    for n in (plain.train(), net.train()):
        with pytest.raises(RuntimeError, match="inference only|eval"):
            n.cache_sources(*views)
    cache = net.eval().cache_sources(*views)
    with pytest.raises(RuntimeError, match="inference only"):
        net.train().forward_cached(cache, torch.arange(3, dtype=torch.int32, device=dev), batch)


def surface_step_case(lib, dev):
    """EnerfLoss + Adam: two eager steps from the same state give the same loss; after the step and ``.eval()`` the frame has the bits
    of a fresh network loaded with the stepped state dict; a source cache built before the step is refused."""
    import pytest
    from enerf_amd.network_composite import Network
    from enerf_amd.train_graph import train_step
    name = "t"
    batch = {k: torch.from_numpy(v).to(dev) for k, v in train_batch(name).items()}
    batch["bbox"] = batch["bbox"].cpu()
    views = (batch["src_inps"][0], batch["bg_src_inps"][0], batch["src_exts"][0], batch["src_ixts"][0])
    idx = torch.arange(3, dtype=torch.int32, device=dev)
    losses, nets = [], []
    for _ in range(2):
        net = train_network(lib, dev, name)
        if not nets:
            with torch.no_grad():
                cache = net.eval().cache_sources(*views)
                before = {k: v.clone() for k, v in net.forward_cached(cache, idx, batch).items()}
            net.train()
        opt = torch.optim.Adam(net.parameters(), lr=5e-4)
        losses.append(float(train_step(net, opt, train_loss_fn(name), batch).detach()))
        nets.append(net)
    assert losses[0] == losses[1], losses
    net = nets[0].eval()
    with pytest.raises(RuntimeError, match="rebuild"):
        net.forward_cached(cache, idx, batch)
    fresh = Network(train_config(name), TRAIN_CASES[name]["L"], lib=lib)
    fresh.load_state_dict(net.state_dict(), strict=True)
    fresh = fresh.to(dev).eval()
    with torch.no_grad():
        a, b = net(batch), fresh(batch)
    assert set(a) == set(b)
    moved = 0.0
    for k in a:
        assert torch.equal(a[k], b[k]), k
        moved = max(moved, float((a[k] - before[k]).abs().max()))
    assert moved > 0, "the step changed nothing the frame shows"
