"""The FeatureNet forward (enerf_feature_net, enerf_feature_net_stage) and the training path's single layers (enerf_conv2d_layer,
forward and data-gradient images) at image sizes the cascade never produces: partial 8 x 32 tiles in either direction, images
smaller than one tile, grids of fewer than 8 blocks, odd sizes under the stride-2 layers.  Whole frames are multiples of 32, so no
other test leaves the full-tile case of k_conv0_fused_cb, k_smooth0_cb and k_smooth1_fused.

Reference: the network's FeatureNet module (or F.conv2d / F.conv_transpose2d / F.interpolate) in float64.  Yardstick: the same in
fp32.  Per output tensor, e = max|x - f64| / max|f64|, and  e_hip <= max(TAU, 3 e_ref)  (the 3x is what
test_training.py::_check_feature_net_train gives two fp32 implementations of one op).  Both references run on the CPU.

Where the fused kernels' LDS-DMA patch of the coarser map starts: at py0 = floor((Hc - 1) / (H - 1) * (8 ty - 1)) for tile row ty
(align-corners scaling), which reaches the last coarse row only when the coarse map has one row (H = 4 for smooth1: sizes (1,4,4),
(2,4,132), (1,4,36)); otherwise the latest origin is the second-last row, at H = 16 k + 4 for smooth1 (20, 36, 100: the seven-row
patch is clamped for five rows) and the third-last at H = 8 k + 4 for smooth0 (12, 20, 36, 44, 100); the same holds for columns
with 32-wide tiles (W = 64 m + 4: 68, 132 for smooth1; W = 32 m + 4: 36, 68, 100, 132 for smooth0).

TAU: five times the worst e_ref over this file's cases, rounded up to one digit (the rule of MLP_TAU in test_kernel_regimes.py).
Measured: worst e_ref 1.22e-6 (level_2 at (1, 8, 32)), so TAU = 7e-6; worst e_hip 1.5e-6 on the emulator.
Run time: about 100 s for the CPU entries.
"""
import functools
import os
import sys

import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from enerf_amd.config import EnerfConfig
from enerf_amd.lib import EnerfError, Options

TAU = 7e-6
# (n, H, W)
FEAT_SIZES = [(1, 4, 4), (1, 8, 32), (2, 12, 20), (3, 36, 68), (1, 44, 100), (2, 4, 132), (1, 100, 4), (5, 20, 36), (1, 72, 40),
              (1, 4, 36), (1, 36, 4), (2, 8, 8)]
WAYS = {"default": None, "unfused": dict(featnet_unfused=1), "smooth0_plain": dict(featnet_smooth0_plain=1)}
# the eleven layers (feature_net.py:7-22): name, cin, cout, k, stride
LAYERS = [("conv0.0", 3, 8, 3, 1), ("conv0.1", 8, 8, 3, 1), ("conv1.0", 8, 16, 5, 2), ("conv1.1", 16, 16, 3, 1), ("conv2.0", 16, 32, 5, 2),
          ("conv2.1", 32, 32, 3, 1), ("toplayer", 32, 32, 1, 1), ("lat1", 16, 32, 1, 1), ("lat0", 8, 32, 1, 1), ("smooth1", 32, 16, 3, 1),
          ("smooth0", 32, 8, 3, 1)]
LAYER_SIZES = [(1, 1, 1), (2, 13, 37), (1, 9, 33), (1, 8, 32), (2, 3, 70), (1, 17, 31), (1, 40, 6)]
WORST = {"e_ref": 0.0, "e_hip": 0.0}


def _emu():
    from emu_lib import emu_lib
    return emu_lib(), torch.device("cpu")


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _net(gpu):
    from __graft_entry__ import _seeded_network
    lib, dev = _gpu() if gpu else _emu()
    return _seeded_network(EnerfConfig(), dev, lib=lib)


@functools.lru_cache(maxsize=None)
def _modules():
    """The FeatureNet module on the CPU in fp32 and float64 (the same seeded weights as _net's, whichever library that has)."""
    import copy
    from __graft_entry__ import _seeded_network
    m = _seeded_network(EnerfConfig(), torch.device("cpu")).feature_net
    return m, copy.deepcopy(m).double()


@functools.lru_cache(maxsize=None)
def _feat_reference(n, H, W):
    """Input images and the module's three maps in float64 and fp32 (CPU), computed once per size."""
    g = torch.Generator().manual_seed(1000 * n + 10 * H + W)
    x = torch.rand(n, 3, H, W, generator=g)
    m32, m64 = _modules()
    with torch.no_grad():
        return x, m64(x.double()), m32(x)


def _compare(tag, got, r64, r32):
    """got channels-last, references NCHW."""
    ref = r64.permute(0, 2, 3, 1)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    scale = float(ref.abs().max())
    e_hip = float((got.cpu().double() - ref).abs().max()) / scale
    e_ref = float((r32.permute(0, 2, 3, 1).double() - ref).abs().max()) / scale
    WORST["e_ref"], WORST["e_hip"] = max(WORST["e_ref"], e_ref), max(WORST["e_hip"], e_hip)
    print(f"[featnet] {tag}: e_hip {e_hip:.2e} e_ref {e_ref:.2e}")
    assert e_hip <= max(TAU, 3.0 * e_ref), f"{tag}: e_hip {e_hip:.3e} > max({TAU:.0e}, 3 x e_ref {e_ref:.3e})"


def _feature_net_case(gpu, n, H, W):
    lib, dev = _gpu() if gpu else _emu()
    packed = _net(gpu)._packed_weights("feature_net")
    x, r64, r32 = _feat_reference(n, H, W)
    src = x.to(dev)
    for way, kw in WAYS.items():
        opt = Options(**kw) if kw else None
        maps = lib.feature_net(packed, src, 8, options=opt)[:3]
        for i, got in enumerate(maps):
            _compare(f"{(n, H, W)} {way} level_{i}", got, r64[i], r32[i])
        # texel mode: the same features bit for bit, the unpreprocessed image beside them, a zero pad channel
        t2 = lib.feature_net(packed, src, 12, options=opt)[2]
        assert torch.equal(t2[..., :8], maps[2]), (n, H, W, way)
        assert float((t2[..., 8:11].permute(0, 3, 1, 2) - (src * 0.5 + 0.5)).abs().max()) <= 1e-7, (n, H, W, way)
        assert float(t2[..., 11].abs().max()) == 0.0, (n, H, W, way)
        # the three-stage form of the two-stream host path
        for stride, want in ((8, maps[2]), (12, t2)):
            bufs = lib.feature_net_alloc(src, stride)
            for stage in (lib.FEAT_TRUNK, lib.FEAT_LEVEL1, lib.FEAT_LEVEL2):
                lib.feature_net_stage(packed, src, bufs, stage, stride, opt)
            assert torch.equal(bufs[0], maps[0]) and torch.equal(bufs[1], maps[1]) and torch.equal(bufs[2], want), (n, H, W, way, stride)
    print(f"[featnet] worst so far: e_ref {WORST['e_ref']:.2e} e_hip {WORST['e_hip']:.2e}")


def _not_divisible_case(gpu):
    lib, dev = _gpu() if gpu else _emu()
    packed = _net(gpu)._packed_weights("feature_net")
    for H, W in ((6, 8), (8, 10), (5, 7), (33, 64)):
        with pytest.raises(EnerfError, match="divisible by 4"):
            lib.feature_net(packed, torch.rand(1, 3, H, W, device=dev), 8)


def _cl(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _layer_case(gpu, name, cin, cout, k, stride):
    """One layer shape at every size: forward (with bias), forward with the 2x-upsampled coarser map added where the output is
    even, and — the stride-1 layers — the data gradient as the same kernel on the flipped, channel-transposed weights."""
    lib, dev = _gpu() if gpu else _emu()
    g = torch.Generator().manual_seed(100 * cin + 10 * cout + k)
    w = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    fwd = lib.conv2d_layer_pack(w.to(dev), b.to(dev), cin, cout, k)
    bwd = lib.conv2d_layer_pack(lib.weights_flip_transpose(w.to(dev)), None, cout, cin, k) if stride == 1 and cin != 3 else None
    pad = (k - 1) // 2
    for N, H, W in LAYER_SIZES:
        x = torch.randn(N, cin, H, W, generator=g)
        xin = (x if cin == 3 else _cl(x)).to(dev)                # (the image layer reads NCHW)
        r64 = F.conv2d(x.double(), w.double(), b.double(), stride, pad)
        r32 = F.conv2d(x, w, b, stride, pad)
        _compare(f"{name} {(N, H, W)}", lib.conv2d_layer(fwd, cin, cout, k, stride, xin), r64, r32)
        Ho, Wo = r64.shape[-2:]
        if Ho % 2 == 0 and Wo % 2 == 0:
            c = torch.randn(N, cout, Ho // 2, Wo // 2, generator=g)
            up = lambda t: F.interpolate(t, scale_factor=2, mode="bilinear", align_corners=True)
            _compare(f"{name} {(N, H, W)} + up", lib.conv2d_layer(fwd, cin, cout, k, stride, xin, up=_cl(c).to(dev)), r64 + up(c.double()), r32 + up(c))
        if bwd is not None:
            dz = torch.randn(N, cout, Ho, Wo, generator=g)
            _compare(f"{name} {(N, H, W)} dgrad", lib.conv2d_layer(bwd, cout, cin, k, 1, _cl(dz).to(dev)),
                     F.conv_transpose2d(dz.double(), w.double(), None, 1, pad), F.conv_transpose2d(dz, w, None, 1, pad))
    print(f"[featnet] worst so far: e_ref {WORST['e_ref']:.2e} e_hip {WORST['e_hip']:.2e}")


def _no_kernel_case(gpu):
    lib, dev = _gpu() if gpu else _emu()
    packed = lib.conv2d_layer_pack(torch.randn(8, 16, 3, 3, device=dev), None, 16, 8, 3)
    with pytest.raises(EnerfError, match="no kernel"):
        lib.conv2d_layer(packed, 16, 8, 3, 1, torch.randn(1, 8, 32, 16, device=dev))


# ---------------------------------------------------------------------------------------------------------------------------------
# emulator
@pytest.mark.parametrize("n,H,W", FEAT_SIZES)
def test_feature_net_sizes_emulated(n, H, W):
    _feature_net_case(False, n, H, W)


def test_feature_net_rejects_sizes_not_divisible_by_4_emulated():
    _not_divisible_case(False)


@pytest.mark.parametrize("name,cin,cout,k,stride", LAYERS)
def test_conv2d_layer_sizes_emulated(name, cin, cout, k, stride):
    _layer_case(False, name, cin, cout, k, stride)


def test_conv2d_layer_without_a_kernel_raises_emulated():
    _no_kernel_case(False)


# ---------------------------------------------------------------------------------------------------------------------------------
# MI355X
@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("n,H,W", FEAT_SIZES)
def test_feature_net_sizes_on_gpu(n, H, W):
    _feature_net_case(True, n, H, W)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_feature_net_rejects_sizes_not_divisible_by_4_on_gpu():
    _not_divisible_case(True)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("name,cin,cout,k,stride", LAYERS)
def test_conv2d_layer_sizes_on_gpu(name, cin, cout, k, stride):
    _layer_case(True, name, cin, cout, k, stride)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
def test_conv2d_layer_without_a_kernel_raises_on_gpu():
    _no_kernel_case(True)
