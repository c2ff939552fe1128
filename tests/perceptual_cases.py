"""Helper of tests/test_perceptual_loss.py: the restatement of the trainer's perceptual term (lib/train/losses/vgg_perceptual_loss.py:
21-37 as losses/enerf.py:30-51 calls it) as torch-CPU functions parameterised by dtype, the LINEAR backward chain with its three
decisions (sign of x - y, act > 0, pool arg-max) taken from given activations, and the recipes of the cases.  The float64 run is the
reference of every check; the float32 run of the SAME function is the yardstick, never the library's own output.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from enerf_amd.lib import PERCEPTUAL_CONVS
from enerf_amd.loss import PerceptualWeights

MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
POOL_BEFORE = (2, 4, 7)              # conv numbers (0..9) with a max pool in front: features.4, .9, .16
TAP_AFTER = (1, 3, 6, 9)             # relu1_2, relu2_2, relu3_3, relu4_3


@functools.lru_cache(maxsize=None)
def weights():
    return PerceptualWeights.random(0)


_ON_DEVICE = {}


def weights_on(w, dev):
    if dev.type == "cpu":
        return w
    key = (id(w), str(dev))
    if key not in _ON_DEVICE:
        _ON_DEVICE[key] = PerceptualWeights([(a.to(dev), b.to(dev)) for a, b in w.convs])
    return _ON_DEVICE[key]


def rel_err(got, ref64):
    return float((got.to(torch.float64) - ref64).abs().max() / ref64.abs().max())


def normalise(img_nchw):
    dt = img_nchw.dtype
    return (img_nchw - torch.tensor(MEAN, dtype=dt).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=dt).view(1, 3, 1, 1)


def trunk(w, img_nchw):
    """(N,3,h,w) images in [0,1] -> the ten post-ReLU activations (N,C_i,H_i,W_i), in the images' dtype."""
    dt = img_nchw.dtype
    x, acts = normalise(img_nchw), []
    for i, (cw, cb) in enumerate(w.convs):
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2)
        x = torch.relu(F.conv2d(x, cw.to(dt), cb.to(dt), padding=1))
        acts.append(x)
    return acts


def loss_of(acts_x, acts_y):
    """{loss, l_0 .. l_3} (5,), loss = ((l_0 + l_1) + l_2) + l_3, l = F.l1_loss (mean over all elements)."""
    ls = [(acts_x[i] - acts_y[i]).abs().mean() for i in TAP_AFTER]
    return torch.stack([((ls[0] + ls[1]) + ls[2]) + ls[3]] + ls)


def nchw(img_nhwc, dtype):
    return torch.from_numpy(np.ascontiguousarray(img_nhwc)).to(dtype).permute(0, 3, 1, 2).contiguous()


def chain(w, acts_x, taps_y, dtype=torch.float64, variant=None):
    """d loss / d pred (N,h,w,3) as the LINEAR chain on given activations: ``acts_x`` the ten pred activations (N,C,H,W), ``taps_y``
    {layer: gt activation} at the four taps.  Every decision is read from these tensors: seeds sign(x - y) / numel, ReLU masks
    x > 0, pool arg-max of x (torch's max_pool2d(return_indices=True)); the arithmetic (transposed convolutions, / std) runs in
    ``dtype``.  variant (wrong on purpose, for the discrimination test): 'nomask' the ReLU mask left out, 'allfour' the pool
    gradient sent to all four positions, 'nosign' x - y instead of its sign, 'pixmean' the mean over pixels instead of elements."""
    g = None
    for i in range(9, -1, -1):
        a = acts_x[i]
        g = torch.zeros(a.shape, dtype=dtype) if g is None else g
        if i in TAP_AFTER:
            d = a - taps_y[i]
            seed = (d if variant == "nosign" else torch.sign(d)).to(dtype)
            g = g + seed / (a.numel() // a.shape[1] if variant == "pixmean" else a.numel())
        if variant != "nomask":
            g = g * (a > 0).to(dtype)
        g = F.conv_transpose2d(g, w.convs[i][0].to(dtype), padding=1)
        if i in POOL_BEFORE:
            below = acts_x[i - 1]
            if variant == "allfour":
                up = torch.zeros(below.shape, dtype=dtype)
                H2, W2 = 2 * g.shape[2], 2 * g.shape[3]
                up[:, :, :H2, :W2] = g.repeat_interleave(2, 2).repeat_interleave(2, 3)
                g = up
            else:
                _, idx = F.max_pool2d(below, 2, 2, return_indices=True)
                g = F.max_unpool2d(g, idx, 2, 2, output_size=below.shape[-2:])
    g = g / torch.tensor(STD, dtype=dtype).view(1, 3, 1, 1)
    return g.permute(0, 2, 3, 1).contiguous()


def cl(t):
    """(N,C,H,W) -> channels-last (N,H,W,C), contiguous."""
    return t.permute(0, 2, 3, 1).contiguous()


def sizes(h, w):
    out = []
    for i in range(10):
        if i in POOL_BEFORE:
            h, w = h // 2, w // 2
        out.append((h, w))
    return out


# ---- whole-term cases: name -> recipe ------------------------------------------------------------------------------------------
CASES = {
    "plain16": dict(N=1, h=16, w=16, pooled=[(16, 16), (8, 8), (4, 4), (2, 2)]),
    "odd22x37": dict(N=1, h=22, w=37, pooled=[(22, 37), (11, 18), (5, 9), (2, 4)]),              # every floor cuts a row or a column
    "min8": dict(N=2, h=8, w=8, pooled=[(8, 8), (4, 4), (2, 2), (1, 1)]),                        # a 1x1 map at conv 7 - 9
    "patches": dict(N=4, h=16, w=16, pooled=[(16, 16), (8, 8), (4, 4), (2, 2)]),
    "wide40x72": dict(N=1, h=40, w=72, pooled=[(40, 72), (20, 36), (10, 18), (5, 9)]),           # more than one 8x32 tile both ways
    # plain16 with 2x2 windows of EQUAL positive values planted in the activations written for conv 1, 3 and 6
    "ties16": dict(N=1, h=16, w=16, pooled=[(16, 16), (8, 8), (4, 4), (2, 2)], images="plain16", ties=True),
}
FORWARD_CASES = ("plain16", "odd22x37", "min8", "patches", "wide40x72")
BACKWARD_CASES = FORWARD_CASES + ("ties16",)
# (layer, n, y0, x0) of the planted windows: one per pooled layer at least, inside the map, also in the last full window
TIES = ((1, 0, 0, 0), (1, 0, 6, 10), (1, 0, 14, 14), (3, 0, 2, 4), (3, 0, 6, 6), (6, 0, 0, 2), (6, 0, 2, 0))


@functools.lru_cache(maxsize=None)
def build(name):
    c = dict(CASES[name])
    rng = np.random.default_rng(sum(c.get("images", name).encode()))
    N, h, w = c["N"], c["h"], c["w"]
    yy, xx = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 4, w), indexing="ij")
    base = 0.5 + 0.3 * np.sin(yy[None, :, :, None] * rng.uniform(1, 3, (N, 1, 1, 3)) + xx[None, :, :, None] * rng.uniform(1, 3, (N, 1, 1, 3)))
    gt = np.clip(base + rng.normal(0, 0.08, (N, h, w, 3)), 0, 1).astype(np.float32)
    pred = np.clip(gt + rng.normal(0, 0.06, (N, h, w, 3)), 0, 1).astype(np.float32)
    W = weights()
    assert [sizes(h, w)[i] for i in TAP_AFTER] == c["pooled"], (name, sizes(h, w))
    c.update(pred=pred, gt=gt, weights=W)
    # forward: float64 reference, float32 yardstick
    p64 = nchw(pred, torch.float64).requires_grad_(True)
    ax64 = trunk(W, p64)
    ay64 = trunk(W, nchw(gt, torch.float64))
    out64 = loss_of(ax64, ay64)
    (auto64,) = torch.autograd.grad(out64[0], p64)
    ax64 = [a.detach() for a in ax64]
    ax32, ay32 = trunk(W, nchw(pred, torch.float32)), trunk(W, nchw(gt, torch.float32))
    c.update(acts64=[cl(torch.cat([x, y])) for x, y in zip(ax64, ay64)],
             acts32=[cl(torch.cat([x, y])).to(torch.float64) for x, y in zip(ax32, ay32)],
             out64=out64.detach(), out32=loss_of(ax32, ay32).to(torch.float64), ax64=ax64, ay64=ay64)
    # backward with pinned decisions: the float64 activations rounded to float32 are what the test writes into the workspace
    rx = [a.to(torch.float32) for a in ax64]
    ry = {i: ay64[i].to(torch.float32) for i in TAP_AFTER}
    if c.get("ties"):
        for k, (layer, n, y0, x0) in enumerate(TIES):
            rx[layer][n, ::3, y0:y0 + 2, x0:x0 + 2] = 0.625 + 0.125 * k      # every third channel; positive, so the ReLU mask is on
    for i in TAP_AFTER:                                                     # a collision x == y at a positive activation has no defined sign
        assert not bool(((rx[i] == ry[i]) & (rx[i] > 0)).any()), (name, i)
    rx64, ry64 = [a.to(torch.float64) for a in rx], {i: v.to(torch.float64) for i, v in ry.items()}
    c["pinned_x"], c["pinned_y"] = rx, ry
    c["grad64"] = chain(W, rx64, ry64, torch.float64)
    c["grad32"] = chain(W, rx64, ry64, torch.float32).to(torch.float64)
    if not c.get("ties"):
        # from the reference alone: rounding the activations changed no decision, so the chain IS float64 autograd
        gap = rel_err(c["grad64"], cl(auto64))
        assert gap <= 1e-12, (name, gap)
    c["auto64"] = cl(auto64)
    return c


def workspace_with(lib, dev, c):
    """A workspace holding the case's pinned activations, written through enerf_perceptual_layout: pred images first, then gt (only
    the taps' gt halves are read by the backward pass; the others stay zero)."""
    N, h, w = c["N"], c["h"], c["w"]
    ws = lib.perceptual_workspace(N, h, w, dev).zero_()
    for i, (off, shape) in enumerate(lib.perceptual_layout(N, h, w)):
        x = cl(c["pinned_x"][i])
        y = cl(c["pinned_y"][i]) if i in TAP_AFTER else torch.zeros_like(x)
        t = torch.cat([x, y])
        assert tuple(t.shape) == shape and shape[3] == PERCEPTUAL_CONVS[i][1]
        ws[off:off + t.numel()] = t.reshape(-1).to(dev)
    return ws


def read_acts(lib, ws, c):
    """The ten saved activations (2N,H,W,C) of a workspace, on the CPU."""
    return [ws[off:off + int(np.prod(shape))].reshape(shape).cpu() for off, shape in lib.perceptual_layout(c["N"], c["h"], c["w"])]


def images_on(c, dev, same=False):
    N, h, w = c["N"], c["h"], c["w"]
    T = lambda a: torch.from_numpy(a).to(dev).reshape(N, h * w, 3)
    return T(c["gt"] if same else c["pred"]), T(c["gt"])


# ---- single data-gradient layers: forward (cin, cout), H, W ----------------------------------------------------------------------
LAYER_CASES = ((3, 64, 9, 21), (64, 64, 9, 21), (64, 128, 9, 21), (128, 256, 5, 9), (256, 512, 3, 5), (512, 512, 3, 5), (512, 512, 1, 1))


@functools.lru_cache(maxsize=None)
def layer_case(cin, cout, H, W):
    """N = 2 gradients (N,cout,H,W); w of the first trunk layer with this pair; ref64 / ref32 = conv_transpose2d as (N,H,W,cin)."""
    w = weights().convs[PERCEPTUAL_CONVS.index((cin, cout))][0]
    g = torch.randn((2, cout, H, W), generator=torch.Generator().manual_seed(1000 * cout + 10 * H + W))
    ref = lambda dt: cl(F.conv_transpose2d(g.to(dt), w.to(dt), padding=1))
    return dict(w=w, g_cl=cl(g), ref64=ref(torch.float64), ref32=ref(torch.float32).to(torch.float64))


# ---- EnerfLoss: losses/enerf.py:21-51 restated -----------------------------------------------------------------------------------
LOSS_MODES = {
    # 32x64 source images, render_scale (0.25, 1): an 8x16 and a 32x64 level, both whole images
    "image": dict(loss_weight=(0.5, 1.0), train_img=(True, True), num_patchs=(0, 0), patch_size=(8, 8), num_rays=(128, 2048),
                  render_scale=(0.25, 1.0), rays=(128, 2048)),
    # level 1: 40 random rays, then two 8x8 patches; level 0 has no patches and no term
    "patch": dict(loss_weight=(0.5, 1.0), train_img=(False, False), num_patchs=(0, 2), patch_size=(8, 8), num_rays=(128, 40),
                  render_scale=(0.25, 1.0), rays=(128, 168)),
}


@functools.lru_cache(maxsize=None)
def loss_case(mode):
    c = dict(LOSS_MODES[mode])
    rng = np.random.default_rng(11 + len(mode))
    out, batch = {}, {"src_inps": np.zeros((1, 2, 3, 32, 64), np.float32)}
    for i, n in enumerate(c["rays"]):
        gt = rng.uniform(0, 1, (1, n, 3)).astype(np.float32)
        out[f"rgb_level{i}"] = np.clip(gt + rng.normal(0, 0.1, gt.shape), 0, 1).astype(np.float32)
        batch[f"rgb_{i}"] = gt
    c.update(output=out, batch=batch)
    c["ref64"], c["ref32"] = loss_restated(c, torch.float64), loss_restated(c, torch.float32)
    return c


def loss_restated(c, dtype, perceptual=True):
    """scalar_stats of NetworkWrapper.forward (losses/enerf.py:19-53) in ``dtype``, as python floats."""
    W = weights()
    stats, loss = {}, 0
    B, S, C, H0, W0 = c["batch"]["src_inps"].shape

    def term(inp, tar):                                                     # (n,3,h,w) each
        return loss_of(trunk(W, inp), trunk(W, tar))[0]

    for i in range(2):
        pred, gt = torch.from_numpy(c["output"][f"rgb_level{i}"]).to(dtype), torch.from_numpy(c["batch"][f"rgb_{i}"]).to(dtype)
        color = F.mse_loss(gt, pred)
        stats[f"color_mse_{i}"] = color
        loss = loss + c["loss_weight"][i] * color
        stats[f"psnr_{i}"] = -10.0 * torch.log(color) / torch.log(torch.tensor([10.0], dtype=dtype))
        if not perceptual:
            continue
        if c["train_img"][i]:
            H, Wd = int(H0 * c["render_scale"][i]), int(W0 * c["render_scale"][i])
            p = term(pred.reshape(B, H, Wd, 3).permute(0, 3, 1, 2), gt.reshape(B, H, Wd, 3).permute(0, 3, 1, 2))
        elif c["num_patchs"][i] > 0:
            ps, n0 = c["patch_size"][i], c["num_rays"][i]
            cut = lambda t: torch.cat([t[:, n0 + j * ps * ps:n0 + (j + 1) * ps * ps, :].reshape(-1, ps, ps, 3).permute(0, 3, 1, 2)
                                       for j in range(c["num_patchs"][i])])
            p = term(cut(pred), cut(gt))
        else:
            continue
        loss = loss + 0.01 * p * c["loss_weight"][i]
        stats[f"perceptual_loss_{i}"] = p
    stats["loss"] = loss
    return {k: float(v) for k, v in stats.items()}
