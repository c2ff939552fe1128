"""Helper of tests/test_eval_lpips.py: the restatement of ``lpips.LPIPS(net='vgg')`` (lpips 0.1.x: lpips=True, spatial=False, eval
mode) as ONE torch-CPU function parameterised by dtype, the evaluators' preprocessing in front of it, and the recipes of the
cases.  The float64 run of the restatement is the reference of every check; its float32 run is the yardstick: a
kernel may be as far from float64 as an honest float32 evaluation of the same formula, never compared to its own output.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from enerf_amd.lib import VGG_CONVS
from enerf_amd.lpips import LpipsWeights

SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
POOL_BEFORE = (2, 4, 7, 10)          # conv numbers (0..12) with a max pool in front: features.5, .10, .17, .24
TAP_AFTER = (1, 3, 6, 9, 12)         # relu1_2, relu2_2, relu3_3, relu4_3, relu5_3


@functools.lru_cache(maxsize=None)
def weights(kind="std"):
    """'std': LpipsWeights.random(0).  'tiny_tap': the same with the last convolution (weights and bias) scaled by 1e-6, so the
    relu5_3 features have a norm near 1e-6 and the placement of the 1e-10 (outside the square root: it compares with the norm;
    inside: with its square) changes d_4 by an order of magnitude; with 'std' weights no norm comes near either."""
    w = LpipsWeights.random(0)
    if kind == "tiny_tap":
        convs = list(w.convs)
        convs[12] = (convs[12][0] * 1e-6, convs[12][1] * 1e-6)
        w = LpipsWeights(convs, w.lins)
    return w


def scaling_layer(x):
    dt = x.dtype
    return (x - torch.tensor(SHIFT, dtype=dt).view(1, 3, 1, 1)) / torch.tensor(SCALE, dtype=dt).view(1, 3, 1, 1)


def trunk_taps(w, x, variant=None):
    """x (N,3,h,w) in [-1,1] -> the five tap tensors (N,C,h_l,w_l).  variant (wrong on purpose, for the discrimination test):
    'fold' the scaling layer folded into conv 0's bias (zero padding then pads the UNSCALED image), 'ceil' ceil-mode pooling."""
    dt = x.dtype
    taps = []
    for i, (cw, cb) in enumerate(w.convs):
        cw, cb = cw.to(dt), cb.to(dt)
        if i in POOL_BEFORE:
            x = F.max_pool2d(x, 2, 2, ceil_mode=variant == "ceil")
        if i == 0 and variant == "fold":
            sh, sc = torch.tensor(SHIFT, dtype=dt), torch.tensor(SCALE, dtype=dt)
            cw2 = cw / sc.view(1, 3, 1, 1)
            cb2 = cb - (cw * (sh / sc).view(1, 3, 1, 1)).sum((1, 2, 3))
            x = F.conv2d(x, cw2, cb2, padding=1)
        else:
            if i == 0:
                x = scaling_layer(x)
            x = F.conv2d(x, cw, cb, padding=1)
        x = torch.relu(x)
        if i in TAP_AFTER:
            taps.append(x)
    return taps


def lpips_restated(w, in0, in1, dtype=torch.float64, variant=None):
    """(B,3,h,w) in0 / in1 in [-1,1] -> (B,6) {lpips, d_0 .. d_4} in ``dtype``; lpips = (((d_0 + d_1) + d_2) + d_3) + d_4."""
    t0, t1 = trunk_taps(w, in0.to(dtype), variant), trunk_taps(w, in1.to(dtype), variant)
    ds = []
    for l, (f0, f1) in enumerate(zip(t0, t1)):
        if variant == "eps_inside":
            n0 = f0 / torch.sqrt((f0 ** 2).sum(1, keepdim=True) + 1e-10)
            n1 = f1 / torch.sqrt((f1 ** 2).sum(1, keepdim=True) + 1e-10)
        else:
            n0 = f0 / (torch.sqrt((f0 ** 2).sum(1, keepdim=True)) + 1e-10)
            n1 = f1 / (torch.sqrt((f1 ** 2).sum(1, keepdim=True)) + 1e-10)
        lin = w.lins[l].to(dtype).view(1, -1, 1, 1)
        ds.append((lin * (n0 - n1) ** 2).sum(1).mean((1, 2)))
    total = ds[0]
    for d in ds[1:]:
        total = total + d
    return torch.stack([total] + ds, 1)


def tap_sizes(rh, rw):
    out, h, w = [], rh, rw
    for i in range(13):
        if i in POOL_BEFORE:
            h, w = h // 2, w // 2
        if i in TAP_AFTER:
            out.append((h, w))
    return out


def evaluator_inputs(pred, gt, mask, evaluator, center=False, rect=None):
    """What the reference's evaluator hands to loss_fn_vgg for a batch: pred / gt (B,h,w,3) float32 in [0,1], mask (B,h,w) or None
    -> in0, in1 (B,3,rh,rw) float32 in [-1,1] (enerf.py:48-54,67-69,82-83; enerf_human.py:54-56,64,72-73).  rect (x, y, w, h): the
    human evaluator's bounding rectangle, shared by the batch."""
    pred, gt = pred.copy(), gt.copy()
    B, h, w, _ = pred.shape
    on = np.ones((B, h, w), bool) if mask is None else (mask == 1 if evaluator == "human" else mask >= 1)
    pred[~on] = 0
    gt[~on] = 0
    if center:
        ch, cw = int(h * 0.1), int(w * 0.1)
        pred, gt = pred[:, ch:h - ch, cw:w - cw], gt[:, ch:h - ch, cw:w - cw]
    if rect is not None:
        x, y, rw, rh = rect
        pred, gt = pred[:, y:y + rh, x:x + rw], gt[:, y:y + rh, x:x + rw]
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()
    return (T(pred) - 0.5) * 2, (T(gt) - 0.5) * 2


# ---- whole-metric cases: name -> recipe -------------------------------------------------------------------------------------
CASES = {
    # 16x16: every pool ends at 1x1
    "plain16": dict(B=1, h=16, w=16, mask=False, center=False, rect=None, pooled=[(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]),
    # 40x72 with eval_center leaves 32x58: pooled widths 29 and 7 are odd, so floor pooling matters
    "center40x72": dict(B=1, h=40, w=72, mask=False, center=True, rect=None, pooled=[(32, 58), (16, 29), (8, 14), (4, 7), (2, 3)]),
    # >= 1 mask and an (x, y, w, h) rectangle with odd offsets and odd sizes
    "rect48x64": dict(B=1, h=48, w=64, mask=True, center=False, rect=(5, 3, 37, 22), pooled=[(22, 37), (11, 18), (5, 9), (2, 4), (1, 2)]),
    # two different images per batch element
    "batch2": dict(B=2, h=20, w=24, mask=True, center=False, rect=None, pooled=[(20, 24), (10, 12), (5, 6), (2, 3), (1, 1)]),
    # the 16x16 images with the 'tiny_tap' weights: the placement of eps decides d_4
    "tiny16": dict(B=1, h=16, w=16, mask=False, center=False, rect=None, pooled=[(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)],
                   weights="tiny_tap", images="plain16"),
    "tiny40x72": dict(B=1, h=40, w=72, mask=False, center=True, rect=None, pooled=[(32, 58), (16, 29), (8, 14), (4, 7), (2, 3)],
                      weights="tiny_tap", images="center40x72"),
    # GPU only
    "gpu128x160": dict(B=2, h=128, w=160, mask=True, center=True, rect=None, pooled=[(104, 128), (52, 64), (26, 32), (13, 16), (6, 8)]),
}


@functools.lru_cache(maxsize=None)
def build(name):
    c = dict(CASES[name])
    rng = np.random.default_rng(sum(c.get("images", name).encode()))
    B, h, w = c["B"], c["h"], c["w"]
    # smooth structure + noise, and a prediction near the ground truth: the regime the metric is used in
    yy, xx = np.meshgrid(np.linspace(0, 3, h), np.linspace(0, 4, w), indexing="ij")
    base = 0.5 + 0.3 * np.sin(yy[None, :, :, None] * rng.uniform(1, 3, (B, 1, 1, 3)) + xx[None, :, :, None] * rng.uniform(1, 3, (B, 1, 1, 3)))
    gt = np.clip(base + rng.normal(0, 0.08, (B, h, w, 3)), 0, 1).astype(np.float32)
    pred = np.clip(gt + rng.normal(0, 0.06, (B, h, w, 3)), 0, 1).astype(np.float32)
    mask = None
    if c["mask"]:
        mask = (rng.uniform(size=(B, h, w)) > 0.15).astype(np.uint8) * rng.integers(1, 3, (B, h, w)).astype(np.uint8)   # 0, 1, 2
    c.update(pred=pred, gt=gt, mask_arr=mask)
    in0, in1 = evaluator_inputs(pred, gt, mask, "enerf", c["center"], c["rect"])
    assert tap_sizes(in0.shape[2], in0.shape[3]) == c["pooled"], (name, tap_sizes(in0.shape[2], in0.shape[3]))
    c.update(in0=in0, in1=in1)
    c["weights"] = weights(c.get("weights", "std"))
    c["ref64"] = lpips_restated(c["weights"], in0, in1, torch.float64)
    c["ref32"] = lpips_restated(c["weights"], in0, in1, torch.float32).to(torch.float64)
    return c


def case_tensors(lib, dev, c, pred=None):
    """Positional and keyword arguments of EnerfLib.eval_lpips for a case, already on ``dev``; ``pred`` replaces the case's."""
    B, h, w = c["B"], c["h"], c["w"]
    T = lambda a: torch.from_numpy(a).to(dev)
    p = T(c["pred"] if pred is None else pred).reshape(B, h * w, 3)
    g = T(c["gt"]).reshape(B, h * w, 3)
    m = None if c["mask_arr"] is None else T(c["mask_arr"]).reshape(B, h * w)
    crop = (int(h * 0.1), int(w * 0.1)) if c["center"] else (0, 0)
    return (weights_on(c["weights"], dev).packed(lib), p, g, m), dict(image_hw=(h, w), crop=crop, rect=c["rect"], sync=False)


def run_case(lib, dev, c, pred=None):
    """(B,6) float64 device tensor of a case through EnerfLib.eval_lpips, as the evaluators call it."""
    args, kw = case_tensors(lib, dev, c, pred)
    return lib.eval_lpips(*args, **kw)


def bounding_rect(on):
    """cv2.boundingRect of a boolean mask -> (x, y, w, h); all zero when nothing is on."""
    ys, xs = np.nonzero(on)
    if ys.size == 0:
        return 0, 0, 0, 0
    return int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)


_ON_DEVICE = {}


def weights_on(w, dev):
    """``w`` itself on the CPU, one shared copy per device otherwise (so the packed image is built once)."""
    if dev.type == "cpu":
        return w
    key = (id(w), str(dev))
    if key not in _ON_DEVICE:
        _ON_DEVICE[key] = LpipsWeights([(a.to(dev), b.to(dev)) for a, b in w.convs], [v.to(dev) for v in w.lins])
    return _ON_DEVICE[key]


@functools.lru_cache(maxsize=None)
def front_case():
    """Conv 0 through the evaluator front: 16x16, B = 1, a 0/1/2 mask -> ref64 / ref32 (2,16,16,64): pred image, then gt."""
    rng = np.random.default_rng(7)
    gt = rng.uniform(0, 1, (1, 16, 16, 3)).astype(np.float32)
    pred = np.clip(gt + rng.normal(0, 0.1, gt.shape), 0, 1).astype(np.float32)
    mask = (rng.uniform(size=(1, 16, 16)) > 0.2).astype(np.uint8) * rng.integers(1, 3, (1, 16, 16)).astype(np.uint8)
    mask[0, 0, :5] = 0                                                     # off pixels on the border too
    in0, in1 = evaluator_inputs(pred, gt, mask, "enerf")
    w, b = weights().convs[0]
    x = torch.cat([in0, in1])
    ref = lambda dt: torch.relu(F.conv2d(scaling_layer(x.to(dt)), w.to(dt), b.to(dt), padding=1)).permute(0, 2, 3, 1).contiguous()
    return dict(pred=pred, gt=gt, mask=mask, ref64=ref(torch.float64), ref32=ref(torch.float32).to(torch.float64))


# ---- single layers: (cin, cout, H, W) ---------------------------------------------------------------------------------------
LAYER_CASES = ((64, 64, 9, 21), (64, 64, 17, 33), (128, 256, 5, 9), (512, 512, 1, 1), (512, 512, 2, 3), (512, 512, 5, 9), (256, 512, 4, 7))


@functools.lru_cache(maxsize=None)
def layer_case(cin, cout, H, W):
    """N = 2 distinct images; w, b of the first trunk layer with this (cin, cout); ref64 / ref32 of conv + ReLU as (N,H,W,cout)."""
    w, b = weights().convs[VGG_CONVS.index((cin, cout))]
    g = torch.Generator().manual_seed(1000 * cin + 10 * H + W)
    x = torch.relu(torch.randn((2, cin, H, W), generator=g))                # post-ReLU statistics, as inside the trunk
    ref = lambda dt: torch.relu(F.conv2d(x.to(dt), w.to(dt), b.to(dt), padding=1)).permute(0, 2, 3, 1).contiguous()
    return dict(w=w, b=b, x_cl=x.permute(0, 2, 3, 1).contiguous(), ref64=ref(torch.float64), ref32=ref(torch.float32).to(torch.float64))


def rel_err(got, ref64):
    return float((got.to(torch.float64) - ref64).abs().max() / ref64.abs().max())
