"""The trainer's perceptual term on the device (enerf_perceptual_fwd / _bwd, csrc/perceptual_vgg.h; enerf_amd/loss.py): the first ten
VGG16 layers forward with every activation kept, L1 taps, ten data-gradient layers back into the rendered image — with seeded random
weights (``PerceptualWeights.random``: nothing large is committed, no pretrained network is needed).

Reference: the float64 torch-CPU restatement in tests/perceptual_cases.py.  Yardstick: the SAME restatement in float32 on the CPU,
never our own output: ``err(ours) <= max(tau, 3 * e_ref32)``, ``e_ref32`` the float32 restatement's own distance from
float64 on that tensor, ``tau`` five times the worst ``e_ref32`` of the group, err = max|a - ref64| / max|ref64|; both are computed
here and printed.

The gradient is discontinuous in three decisions (sign of x - y, act > 0, pool arg-max): one flipped decision between a float32 and a
float64 forward moves the end-to-end gradient by 1e-4 .. 1e-3, far above rounding noise.  So the backward check PINS the decisions:
the float32-rounded float64 reference activations are written into the workspace through ``enerf_perceptual_layout``,
``enerf_perceptual_bwd`` runs on them and is compared with the float64 linear chain on exactly those tensors (the case builder
asserts, from the reference alone, that this chain equals float64 autograd to 1e-12 and that no tap collision x == y exists).

1. single data-gradient layers against float64 conv_transpose2d;  2. forward: out[0..4], the ten saved pred activations, the gt half
at the taps, the pooled sizes, the fixed-order sum;  3. backward with pinned decisions, and planted 2x2 ties;  4. through
``perceptual_loss`` and autograd: bit-identical to the entries called by hand, within the bound of the chain on the library's own
activations, every decision that differs from float64's has a float64 margin under the forward bound;  5. exact properties;
6. discrimination (CPU, no kernel): every (variant, case) pair of the issue separates at 10x the bound of 3, none had to be changed;
7. ``EnerfLoss`` against losses/enerf.py:21-51 restated;  8. (GPU only) three ``GraphedTrainStep`` steps;  9. argument errors.
Every check runs on the CPU lane emulator and again on the gfx950 library (-m gpu).  On the emulator, where a 16x16 forward takes
a quarter of a minute, 4. runs on the two smallest cases; on the GPU on all five.
"""
import numpy as np
import pytest
import torch

import perceptual_cases as P

_needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
_FWD, _BWD, _HAND = {}, {}, {}


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


def _bound(tau, e32):
    return max(tau, 3.0 * e32)


# ---- 1. single data-gradient layers --------------------------------------------------------------------------------------------
def _layer_tau():
    return 5.0 * max(P.rel_err(P.layer_case(*cs)["ref32"], P.layer_case(*cs)["ref64"]) for cs in P.LAYER_CASES)


def _check_layer(lib, dev, cs):
    cin, cout, H, W = cs
    c = P.layer_case(*cs)
    packed = lib.vgg_conv3x3_dgrad_pack(c["w"].to(dev))
    got = lib.vgg_conv3x3_dgrad(packed, cin, cout, c["g_cl"].to(dev)).cpu()
    tau, e32, err = _layer_tau(), P.rel_err(c["ref32"], c["ref64"]), P.rel_err(got, c["ref64"])
    print(f"{dev.type} data gradient of conv {cin}->{cout} at {H}x{W}: err {err:.3e}; e_ref32 {e32:.3e}, tau {tau:.3e}")
    assert got.shape == c["ref64"].shape and err <= _bound(tau, e32)


@pytest.mark.parametrize("cs", P.LAYER_CASES, ids=lambda cs: "%dto%d_%dx%d" % cs)
def test_dgrad_layer_emulated(cs):
    _check_layer(*_emu(), cs)


# ---- 2. forward ------------------------------------------------------------------------------------------------------------------
def _forward(lib, dev, name):
    """(out (5,) float64, the ten saved activations, workspace) of a case, computed once per device."""
    key = (dev.type, name)
    if key not in _FWD:
        c = P.build(name)
        pred, gt = P.images_on(c, dev)
        out, ws = lib.perceptual_fwd(P.weights_on(c["weights"], dev).packed(lib), pred, gt, (c["h"], c["w"]))
        _FWD[key] = (out.cpu(), P.read_acts(lib, ws, c), ws)
    return _FWD[key]


def _act_tau():
    worst = 0.0
    for name in P.FORWARD_CASES:
        c = P.build(name)
        worst = max([worst] + [P.rel_err(a32, a64) for a32, a64 in zip(c["acts32"], c["acts64"])])
    return 5.0 * worst


def _out_tau():
    return 5.0 * max(float(((P.build(n)["out32"] - P.build(n)["out64"]).abs() / P.build(n)["out64"].abs()).max()) for n in P.FORWARD_CASES)


def _check_forward(lib, dev, name):
    c = P.build(name)                                                       # asserts the case's pooled sizes
    N = c["N"]
    out, acts, _ = _forward(lib, dev, name)
    assert out.shape == (5,) and out.dtype == torch.float64
    e32 = (c["out32"] - c["out64"]).abs() / c["out64"].abs()
    err = (out - c["out64"]).abs() / c["out64"].abs()
    bound = torch.maximum(torch.full_like(e32, _out_tau()), 3.0 * e32)
    print(f"{dev.type} {name}: ours {out.tolist()}\n    ref64 {c['out64'].tolist()}\n    err {err.tolist()}\n    e_ref32 {e32.tolist()}\n"
          f"    bound {bound.tolist()}")
    assert bool((err <= bound).all())
    l = out[1:].tolist()
    assert out[0].item() == ((l[0] + l[1]) + l[2]) + l[3]                   # the fixed-order sum
    tau = _act_tau()
    for i, (a, a64, a32) in enumerate(zip(acts, c["acts64"], c["acts32"])):
        assert a.shape == a64.shape
        if i in P.TAP_AFTER:
            assert tuple(a.shape[1:3]) == c["pooled"][P.TAP_AFTER.index(i)]
        halves = [("pred", slice(0, N))] + ([("gt", slice(N, 2 * N))] if i in P.TAP_AFTER else [])
        for tag, s in halves:
            e, r = P.rel_err(a[s], a64[s]), P.rel_err(a32[s], a64[s])
            print(f"{dev.type} {name} act {i} {tag} {tuple(a[s].shape)}: err {e:.3e}; e_ref32 {r:.3e}, tau {tau:.3e}")
            assert e <= _bound(tau, r)


@pytest.mark.parametrize("name", P.FORWARD_CASES)
def test_forward_emulated(name):
    _check_forward(*_emu(), name)


# ---- 3. backward with pinned decisions -----------------------------------------------------------------------------------------------
def _grad_tau():
    return 5.0 * max(P.rel_err(P.build(n)["grad32"], P.build(n)["grad64"]) for n in P.BACKWARD_CASES)


def _pinned_grad(lib, dev, name):
    key = (dev.type, name)
    if key not in _BWD:
        c = P.build(name)
        ws = P.workspace_with(lib, dev, c)
        g = lib.perceptual_bwd(P.weights_on(c["weights"], dev).packed(lib), c["N"], (c["h"], c["w"]), ws)
        _BWD[key] = g.cpu().reshape(c["N"], c["h"], c["w"], 3)
    return _BWD[key]


def _check_backward(lib, dev, name):
    c = P.build(name)               # asserts chain == float64 autograd to 1e-12 and no tap collision (ties16: planted, chain only)
    g = _pinned_grad(lib, dev, name)
    tau, e32, err = _grad_tau(), P.rel_err(c["grad32"], c["grad64"]), P.rel_err(g, c["grad64"])
    print(f"{dev.type} {name} gradient, decisions pinned: err {err:.3e}; e_ref32 {e32:.3e}, tau {tau:.3e}")
    assert err <= _bound(tau, e32)


@pytest.mark.parametrize("name", P.BACKWARD_CASES)
def test_backward_pinned_emulated(name):
    _check_backward(*_emu(), name)


def test_planted_ties_go_to_the_first_element():
    """What the ties16 case pins, from torch alone: in a window of four equal values max_pool2d's index is the first (row-major)."""
    c = P.build("ties16")
    for layer, n, y0, x0 in P.TIES:
        a = c["pinned_x"][layer]
        assert bool((a[n, ::3, y0:y0 + 2, x0:x0 + 2] == a[n, ::3, y0:y0 + 1, x0:x0 + 1]).all()) and float(a[n, 0, y0, x0]) > 0
        _, idx = torch.nn.functional.max_pool2d(a.to(torch.float64), 2, 2, return_indices=True)
        assert bool((idx[n, ::3, y0 // 2, x0 // 2] == y0 * a.shape[3] + x0).all())
    assert P.rel_err(c["grad64"], P.build("plain16")["grad64"]) > 1e-3      # the planted windows do move the gradient


# ---- 4. through perceptual_loss and autograd -------------------------------------------------------------------------------------
def _flipped(lib_acts, c, fwd_bound):
    """Decisions of the library's activations that differ from float64's: count, and the worst float64 margin / (bound * max|act|)."""
    N, count, worst = c["N"], 0, 0.0
    for i in range(10):
        a = lib_acts[i][:N].permute(0, 3, 1, 2).to(torch.float64)
        r = c["ax64"][i]
        scale = fwd_bound * float(r.abs().max())
        checks = [((a > 0) != (r > 0), r.abs())]
        if i in P.TAP_AFTER:
            y, ry = lib_acts[i][N:].permute(0, 3, 1, 2).to(torch.float64), c["ay64"][i]
            checks.append((torch.sign(a - y) != torch.sign(r - ry), (r - ry).abs()))
        if i + 1 in P.POOL_BEFORE:
            F = torch.nn.functional
            _, ia = F.max_pool2d(a, 2, 2, return_indices=True)
            _, ir = F.max_pool2d(r, 2, 2, return_indices=True)
            H2, W2 = 2 * ir.shape[2], 2 * ir.shape[3]
            win = r[:, :, :H2, :W2].unfold(2, 2, 2).unfold(3, 2, 2).reshape(*ir.shape, 4)
            top = win.topk(2, dim=-1).values
            checks.append((ia != ir, top[..., 0] - top[..., 1]))
        for differ, margin in checks:
            if bool(differ.any()):
                count += int(differ.sum())
                worst = max(worst, float(margin[differ].max()) / scale)
    return count, worst


def _by_hand_grad(lib, dev, name):
    """enerf_perceptual_bwd called by hand on the workspace enerf_perceptual_fwd left (_forward), once per device and case."""
    key = (dev.type, name)
    if key not in _HAND:
        c = P.build(name)
        _HAND[key] = lib.perceptual_bwd(P.weights_on(c["weights"], dev).packed(lib), c["N"], (c["h"], c["w"]), _forward(lib, dev, name)[2]).cpu()
    return _HAND[key]


def _check_autograd(lib, dev, name):
    from enerf_amd.loss import perceptual_loss
    c = P.build(name)
    N, h, w = c["N"], c["h"], c["w"]
    W = P.weights_on(c["weights"], dev)
    out, acts, ws = _forward(lib, dev, name)
    by_hand = _by_hand_grad(lib, dev, name)
    pred, gt = P.images_on(c, dev)
    if name == "min8":                                                      # (N,h,w,3) in and out; the others (N,h*w,3) + image_hw
        pred, gt = pred.reshape(N, h, w, 3), gt.reshape(N, h, w, 3)
    pred.requires_grad_(True)
    loss = perceptual_loss(pred, gt, W, None if name == "min8" else (h, w), lib=lib)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and float(loss.detach()) == float(out[0].to(torch.float32))
    loss.backward()
    grad = pred.grad.cpu()
    assert grad.shape == pred.shape and grad.numpy().tobytes() == by_hand.numpy().tobytes()
    # the chain on the library's OWN activations (verified against float64 in 2.)
    ax = [a[:N].permute(0, 3, 1, 2).to(torch.float64) for a in acts]
    ay = {i: acts[i][N:].permute(0, 3, 1, 2).to(torch.float64) for i in P.TAP_AFTER}
    g64, g32 = P.chain(c["weights"], ax, ay, torch.float64), P.chain(c["weights"], ax, ay, torch.float32).to(torch.float64)
    tau, e32, err = _grad_tau(), P.rel_err(g32, g64), P.rel_err(grad.reshape(g64.shape), g64)
    print(f"{dev.type} {name} gradient through autograd vs the chain on the library's activations: err {err:.3e}; e_ref32 {e32:.3e}, tau {tau:.3e}")
    assert err <= _bound(tau, e32)
    fwd_bound = _act_tau()
    count, worst = _flipped(acts, c, fwd_bound)
    end_to_end = P.rel_err(grad.reshape(g64.shape), c["auto64"])
    print(f"{dev.type} {name}: {count} decisions differ from float64's; worst margin / (forward bound {fwd_bound:.3e} * max|act|) = {worst:.3f}; "
          f"end to end against float64 autograd: {end_to_end:.3e}")
    assert worst <= 1.0


@pytest.mark.parametrize("name", ("min8", "plain16"))
def test_autograd_emulated(name):
    _check_autograd(*_emu(), name)


# ---- 5. exact properties -------------------------------------------------------------------------------------------------------------
def _check_exact(lib, dev, name):
    c = P.build(name)
    N, hw = c["N"], (c["h"], c["w"])
    pk = P.weights_on(c["weights"], dev).packed(lib)
    out, _, ws = _forward(lib, dev, name)
    g1 = _by_hand_grad(lib, dev, name)
    pred, gt = P.images_on(c, dev)
    out2, ws2 = lib.perceptual_fwd(pk, pred, gt, hw)
    g2 = lib.perceptual_bwd(pk, N, hw, ws2).cpu()
    assert out.numpy().tobytes() == out2.cpu().numpy().tobytes() and g1.numpy().tobytes() == g2.numpy().tobytes()
    assert float(g1.abs().max()) > 0
    half = lib.perceptual_bwd(pk, N, hw, ws2, torch.full((1,), 0.5, device=dev)).cpu()
    assert torch.equal(half, g1 * 0.5)
    same, _ = P.images_on(c, dev, same=True)
    out0, ws0 = lib.perceptual_fwd(pk, same, gt, hw)
    assert out0.cpu().numpy().tobytes() == np.zeros(5).tobytes()            # pred == gt: exactly +0.0, every l
    g0 = lib.perceptual_bwd(pk, N, hw, ws0).cpu()
    assert g0.shape == g1.shape and bool((g0 == 0).all())


def test_exact_properties_emulated():
    _check_exact(*_emu(), "min8")


# ---- 6. discrimination (CPU, no kernel) ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.FORWARD_CASES)
@pytest.mark.parametrize("variant", ("nomask", "allfour", "nosign", "pixmean"))
def test_wrong_variants_are_told_apart(variant, name):
    c = P.build(name)
    rx = [a.to(torch.float64) for a in c["pinned_x"]]
    ry = {i: v.to(torch.float64) for i, v in c["pinned_y"].items()}
    gap = P.rel_err(P.chain(c["weights"], rx, ry, torch.float64, variant=variant), c["grad64"])
    bound = _bound(_grad_tau(), P.rel_err(c["grad32"], c["grad64"]))
    print(f"{variant} on {name}: max|wrong - true| / max|true| = {gap:.3e}, bound of the kernel check {bound:.3e}")
    assert gap > 10.0 * bound


# ---- 7. EnerfLoss ------------------------------------------------------------------------------------------------------------------------
def _check_enerf_loss(lib, dev, mode):
    from enerf_amd.loss import EnerfLoss
    c = P.loss_case(mode)
    T = lambda d: {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
    output, batch = T(c["output"]), T(c["batch"])
    kw = {k: c[k] for k in ("loss_weight", "train_img", "num_patchs", "patch_size", "num_rays")}
    fn = EnerfLoss(perceptual=P.weights_on(P.weights(), dev), render_scale=c["render_scale"], lib=lib, **kw)
    for v in output.values():
        v.requires_grad_(True)
    loss = fn(output, batch)
    stats = {k: float(v) for k, v in fn.scalar_stats.items()}
    assert sorted(stats) == sorted(c["ref64"]) and float(loss) == stats["loss"]
    assert ("perceptual_loss_0" in stats) == (mode == "image") and "perceptual_loss_1" in stats
    tau = max(_out_tau(), 5.0 * max(abs(c["ref32"][k] - c["ref64"][k]) / abs(c["ref64"][k]) for k in stats))
    for k in sorted(stats):
        r64, r32 = c["ref64"][k], c["ref32"][k]
        err, e32 = abs(stats[k] - r64) / abs(r64), abs(r32 - r64) / abs(r64)
        print(f"{dev.type} EnerfLoss[{mode}] {k}: ours {stats[k]!r}, ref64 {r64!r}: err {err:.3e}; e_ref32 {e32:.3e}, tau {tau:.3e}")
        assert err <= _bound(tau, e32)
    loss.backward()                                                         # both levels receive a gradient, the patches' rays too
    assert all(v.grad is not None and float(v.grad.abs().max()) > 0 for v in output.values())
    plain = EnerfLoss(perceptual=None, lib=lib, **kw)
    mse_only = P.loss_restated(c, torch.float64, perceptual=False)
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in output.items()}
    plain_loss = plain(leaves, batch)
    got = float(plain_loss)
    if mode == "patch":                                                     # the term reaches the patches' rays and no others
        plain_loss.backward()
        g, g_mse = output["rgb_level1"].grad, leaves["rgb_level1"].grad
        assert torch.equal(g[:, :40], g_mse[:, :40]) and torch.equal(output["rgb_level0"].grad, leaves["rgb_level0"].grad)
        assert bool((g[:, 40:] != g_mse[:, 40:]).any(-1).float().mean() > 0.9)
    assert sorted(plain.scalar_stats) == sorted(mse_only) and abs(got - mse_only["loss"]) <= 1e-6 * mse_only["loss"]
    assert got == float(0.5 * fn.scalar_stats["color_mse_0"] + 1.0 * fn.scalar_stats["color_mse_1"])


@pytest.mark.parametrize("mode", ("image", "patch"))
def test_enerf_loss_emulated(mode):
    _check_enerf_loss(*_emu(), mode)


def test_enerf_loss_from_yacs():
    from types import SimpleNamespace as NS
    from enerf_amd.loss import EnerfLoss
    cas = NS(num=2, loss_weight=[0.5, 1.0], train_img=[False, False], num_patchs=[0, 4], patch_size=[64, 64], num_rays=[4096, 32768],
             render_scale=[0.25, 0.5])
    fn = EnerfLoss.from_yacs(NS(enerf=NS(cas_config=cas)), None)
    assert (fn.num, fn.num_patchs, fn.patch_size, fn.num_rays, fn.render_scale) == (2, [0, 4], [64, 64], [4096, 32768], [0.25, 0.5])
    assert fn.perceptual is None and fn.scalar_stats == {}


# ---- 9. argument errors and the weight loader --------------------------------------------------------------------------------------
def _check_errors(lib, dev):
    from enerf_amd.lib import EnerfError
    from enerf_amd.loss import perceptual_loss
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    W = P.weights_on(P.weights(), dev)
    pk = W.packed(lib)
    with pytest.raises(EnerfError, match="unsupported image 7x16"):
        perceptual_loss(z(1, 7 * 16, 3), z(1, 7 * 16, 3), W, (7, 16), lib=lib)
    with pytest.raises(EnerfError, match="unsupported image 16x7"):
        lib.perceptual_fwd(pk, z(1, 16 * 7, 3), z(1, 16 * 7, 3), (16, 7))
    with pytest.raises(EnerfError, match="unsupported layer"):
        lib.vgg_conv3x3_dgrad_pack(z(256, 64, 3, 3))
    with pytest.raises(EnerfError, match="image_hw"):
        perceptual_loss(z(1, 64, 3), z(1, 64, 3), W, lib=lib)
    # the C ABI itself; nothing is launched: the outputs keep their fill
    d = lib.dll
    st = lib.stream_of(pk)
    assert d.enerf_perceptual_workspace_bytes(1, 7, 16) == 0 and b"7x16" in d.enerf_last_error()
    assert d.enerf_perceptual_workspace_bytes(0, 8, 8) == 0 and d.enerf_perceptual_workspace_bytes(1 << 15, 8, 8) == 0
    assert d.enerf_perceptual_workspace_bytes(2, 46341, 46341) == 0 and b"too large" in d.enerf_last_error()    # past the element limit
    need = d.enerf_perceptual_workspace_bytes(1, 8, 16)
    floats = 4 * 1024 * 2 + 2 * (128 * 128 + 32 * 256 + 8 * 768 + 2 * 1536)
    assert need % 16 == 0 and need >= 4 * floats
    ws = torch.zeros((need // 4,), dtype=torch.float32, device=dev)
    a, b = z(1, 128, 3), z(1, 128, 3)
    out = torch.full((5,), 7.0, dtype=torch.float64, device=dev)
    grad = torch.full((1, 128, 3), 7.0, device=dev)
    fwd = lambda pkp=pk.data_ptr(), ap=a.data_ptr(), wsp=ws.data_ptr(), nbytes=need, op=out.data_ptr(), h=8: \
        d.enerf_perceptual_fwd(pkp, ap, b.data_ptr(), 1, h, 16, wsp, nbytes, op, st)
    bwd = lambda pkp=pk.data_ptr(), wsp=ws.data_ptr(), nbytes=need, gp=grad.data_ptr(), h=8: \
        d.enerf_perceptual_bwd(pkp, 1, h, 16, wsp, nbytes, None, gp, st)
    for call in (lambda: fwd(pkp=None), lambda: fwd(ap=None), lambda: fwd(wsp=None), lambda: fwd(op=None), lambda: bwd(pkp=None),
                 lambda: bwd(wsp=None), lambda: bwd(gp=None)):
        assert call() == -1 and b"null" in d.enerf_last_error()
    assert fwd(nbytes=need - 1) == -3 and b"workspace" in d.enerf_last_error()
    assert bwd(nbytes=need - 1) == -3 and b"workspace" in d.enerf_last_error()
    assert fwd(h=7) == -1 and b"unsupported image 7x16" in d.enerf_last_error() and bwd(h=7) == -1
    offs = (__import__("ctypes").c_longlong * 10)()
    assert d.enerf_perceptual_layout(1, 7, 16, offs) == -1 and d.enerf_perceptual_layout(1, 8, 16, None) == -1
    assert d.enerf_perceptual_layout(1, 8, 16, offs) == 0 and list(offs)[:3] == [8192, 8192 + 2 * 128 * 64, 8192 + 4 * 128 * 64]
    assert d.enerf_vgg_conv3x3_dgrad_packed_floats(64, 256) == 0 and d.enerf_vgg_conv3x3_dgrad_packed_floats(64, 128) == 9 * 64 * 128
    x, y = z(1, 4, 4, 128), torch.full((1, 4, 4, 64), 7.0, device=dev)
    assert d.enerf_vgg_conv3x3_dgrad(pk.data_ptr(), 64, 256, x.data_ptr(), y.data_ptr(), 1, 4, 4, st) == -1
    assert d.enerf_vgg_conv3x3_dgrad(None, 64, 128, x.data_ptr(), y.data_ptr(), 1, 4, 4, st) == -1
    assert out.cpu().tolist() == [7.0] * 5 and float(grad.min()) == 7.0 and float(y.min()) == 7.0 and float(ws.abs().max()) == 0.0


def test_errors_emulated():
    _check_errors(*_emu())


def test_weight_loader():
    from enerf_amd.loss import PERCEPTUAL_FEATURE_INDEX, PerceptualWeights
    from enerf_amd.lpips import LpipsWeights
    w = P.weights()
    sd = w.state_dict()
    assert sorted(sd) == sorted(f"features.{i}.{p}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21) for p in ("weight", "bias"))
    assert PERCEPTUAL_FEATURE_INDEX == (0, 2, 5, 7, 10, 12, 14, 17, 19, 21)
    full = dict(LpipsWeights.random(0).state_dict("torchvision"))          # a whole VGG16 + lin: the later layers are not the term's
    back = PerceptualWeights.from_state_dict(full, "cpu")
    for (a, b), (c, d), (e, f) in zip(back.convs, w.convs, PerceptualWeights.from_lpips_weights(LpipsWeights.random(0)).convs):
        assert torch.equal(a, c) and torch.equal(b, d) and torch.equal(e, c) and torch.equal(f, d)
    with pytest.raises(KeyError, match="missing.*features.17.weight"):
        PerceptualWeights.from_state_dict({k: v for k, v in sd.items() if k != "features.17.weight"}, "cpu")
    with pytest.raises(ValueError, match="expected"):
        PerceptualWeights.from_state_dict(dict(sd, **{"features.5.weight": sd["features.5.weight"][:, :-1]}), "cpu")
    with pytest.raises(ValueError, match="10"):
        PerceptualWeights(w.convs[:9])
    assert "test" in PerceptualWeights.random.__doc__.lower()


# ---- the gfx950 library --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("cs", P.LAYER_CASES, ids=lambda cs: "%dto%d_%dx%d" % cs)
def test_dgrad_layer_gpu(cs):
    _check_layer(*_gpu(), cs)


@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("name", P.FORWARD_CASES)
def test_forward_gpu(name):
    _check_forward(*_gpu(), name)


@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("name", P.BACKWARD_CASES)
def test_backward_pinned_gpu(name):
    _check_backward(*_gpu(), name)


@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("name", P.FORWARD_CASES)
def test_autograd_gpu(name):
    _check_autograd(*_gpu(), name)


@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("name", ("min8", "plain16", "wide40x72"))
def test_exact_properties_gpu(name):
    _check_exact(*_gpu(), name)


@pytest.mark.gpu
@_needs_gpu
@pytest.mark.parametrize("mode", ("image", "patch"))
def test_enerf_loss_gpu(mode):
    _check_enerf_loss(*_gpu(), mode)


@pytest.mark.gpu
@_needs_gpu
def test_errors_gpu():
    _check_errors(*_gpu())


@pytest.mark.gpu
@_needs_gpu
def test_perceptual_loss_has_no_implicit_host_sync():
    """Forward and backward only enqueue: under ``torch.cuda.set_sync_debug_mode("error")`` any synchronisation raises."""
    from enerf_amd.loss import perceptual_loss
    lib, dev = _gpu()
    c = P.build("min8")
    W = P.weights_on(c["weights"], dev)
    W.packed(lib)
    pred, gt = P.images_on(c, dev)
    pred.requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        perceptual_loss(pred, gt, W, (8, 8), lib=lib).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert float(pred.grad.abs().max()) > 0


@pytest.mark.gpu
@_needs_gpu
def test_graphed_train_step_with_enerf_loss():
    """8. Three GraphedTrainStep steps of a 32x64 / S = 3 frame with EnerfLoss and random perceptual weights (level 0 renders 8x16,
    the smallest legal image): the capture is kept (fallback='raise': no eager fallback) and the class's own replay-against-eager
    verification passes."""
    from enerf_amd.config import EnerfConfig
    from enerf_amd.loss import EnerfLoss, PerceptualWeights
    from enerf_amd.network import Network
    from enerf_amd.synth import make_batch
    from enerf_amd.train_graph import GraphedTrainStep
    from golden_cases import load_weights
    lib, dev = _gpu()
    cfg = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(True, True))
    net = Network(cfg)
    net.load_state_dict(load_weights(), strict=False)
    net = net.to(dev).train()
    b = make_batch(32, 64, 3, cfg, seed=3, textured=True)
    rng = np.random.default_rng(3)
    for i in range(2):
        b[f"rgb_{i}"] = rng.uniform(0, 1, size=(1, b[f"rays_{i}"].shape[1], 3)).astype(np.float32)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in b.items()}
    assert batch["rgb_0"].shape[1] == 8 * 16 and batch["rgb_1"].shape[1] == 32 * 64
    fn = EnerfLoss((0.5, 1.0), (True, True), (0, 0), (0, 0), (0, 0), PerceptualWeights.random(0, dev),
                   render_scale=cfg.cas.render_scale, lib=lib)
    opt = torch.optim.SGD(net.parameters(), lr=1e-3, momentum=0.9)
    step = GraphedTrainStep(net, opt, fn, batch, clip_value=40.0, warmup=1, fallback="raise", verify=True)
    assert step.graph is not None and "verified against eager steps" in step.step_launch
    losses = [float(step(batch)) for _ in range(3)]
    assert all(np.isfinite(losses)) and sorted(fn.scalar_stats) == sorted(
        ["color_mse_0", "color_mse_1", "psnr_0", "psnr_1", "perceptual_loss_0", "perceptual_loss_1", "loss"])
    assert float(fn.scalar_stats["perceptual_loss_1"]) > 0
    assert losses[0] != losses[1]                                            # the optimizer did step
