"""Kernels past one tile per wave: the fused NeRF MLP forward + backward (k_mlp_fwd / k_mlp_bwd and the weight-gradient reductions
behind NerfMlpFn) against a float64 twin, at P = 1, with idle waves, and with three or more tiles per wave (the next-tile prefetch
and the in-kernel weight-gradient accumulators across tiles).

The emulated library sizes its grids for 256 CUs, so at CPU-sized inputs every wave there does one tile at most; the CPU entries
run under ``emu_cu_count`` (tests/emu_lib.py) to reach the later passes.  The GPU entries size P from the device's CU count."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

EPS32 = 2.0 ** -24
# max|hip - fp64| / max|fp64| per tensor (output, g_vox, g_x, every parameter gradient).  Measured worst case over the 12 cases and
# their regimes: 4.0e-6 on the emulator, 6.5e-6 on an MI355X (sigma.0.bias, F = 35, S = 4, three passes); five times that, rounded.
MLP_TAU = 3e-5
MLP_CASES = [(F, S, vda) for F in (11, 35) for S in (2, 3, 4) for vda in (True, False)]


def _mlp_module(F, vda, dev, g):
    from enerf_amd.network import NerfParams
    torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))    # NerfParams draws its kaiming init from the global generator
    m = NerfParams(F, vda)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return m.to(dev)


def _mlp_inputs(P, S, F, g, dev):
    vox = torch.randn(1, P, 8, generator=g).to(dev)
    x = torch.randn(1, P, S, F + 4, generator=g).to(dev)
    g_raw = torch.randn(1, P, 4, generator=g).to(dev)
    return vox, x, g_raw


def _hip_mlp(lib, m, vox, x, g_raw):
    """raw, g_vox, g_x and the parameter gradients through NerfMlpFn (level 2 for F = 11 / S <= 3, level 1 for S = 4, 0 for F = 35)."""
    from enerf_amd.autograd import nerf_mlp
    for p in m.parameters():
        p.grad = None
    vox, x = vox.clone().requires_grad_(True), x.clone().requires_grad_(True)
    raw = nerf_mlp(lib, m, None, vox, x)
    raw.backward(g_raw)
    return {"raw": raw.detach(), "g_vox": vox.grad, "g_x": x.grad, **{n: p.grad for n, p in m.named_parameters()}}


# biases in front of a softmax over the views: per point their gradient terms cancel across the views (exactly, where no ReLU gates
# them: at P = 1 the sum is zero), so they are measured against the sum of the terms' magnitudes (index into the twin's list)
SOFTMAX_BIASES = {"agg.agg_w_fc.0.bias": -5, "color.2.bias": -1}


def _twin_mlp(m, vox, x, g_raw, dtype=torch.float64):
    """The torch twin's raw, input and parameter gradients in ``dtype`` (float64: the reference; float32: the conditioning
    yardstick), and the magnitude each tensor is compared relative to."""
    import torch_twins as T
    m2 = copy.deepcopy(m).to(dtype)
    vox, x = vox.detach().to(dtype).clone().requires_grad_(True), x.detach().to(dtype).clone().requires_grad_(True)
    pre = []
    raw = T.nerf_forward(m2, vox, x, pre)
    for z, _ in pre:
        z.retain_grad()
    raw.backward(g_raw.to(dtype))
    out = {"raw": raw.detach(), "g_vox": vox.grad, "g_x": x.grad, **{n: p.grad for n, p in m2.named_parameters()}}
    scale = {k: float(v.abs().max()) for k, v in out.items()}
    for k, i in SOFTMAX_BIASES.items():
        scale[k] = max(scale[k], float(pre[i][0].grad.abs().sum()))
    return out, scale


def _branch_points(pre, P, slack=4.0):
    """Points where some ReLU pre-activation of the float64 twin lies within rounding of zero (|z| <= slack * eps32 * (|W| |in| + |b|)):
    fp32 may take the other branch there, and a flipped gate moves the point's gradients by O(1).  (Measured with the torch fp32
    twin over 12 x 40,000 points: its error reaches ~15 eps32 (|W| |in| + |b|) at the extreme, but the 5 gates it flipped all lie
    within 2 of that; slack 4 masks 2.5e-4 .. 5e-4 of the points.)"""
    near = torch.zeros(P, dtype=torch.bool, device=pre[0][0].device)
    for z, mag in pre:
        hit = (z.abs() <= slack * EPS32 * mag).reshape(P, -1).any(1)
        near |= hit
    return near


def _tiles_per_wave(lib, P):
    waves = int(lib.dll.enerf_nerf_mlp_bwd_chunks(P))
    return -(-(-(-P // 16)) // waves), waves


def _check_mlp_case(lib, dev, F, S, vda, P, seed, regime, sensitivity=False):
    """One case and one point count: HIP against float64, branch points masked; returns (tiles per wave, waves)."""
    g = torch.Generator().manual_seed(seed)
    m = _mlp_module(F, vda, dev, g)
    vox, x, g_raw = _mlp_inputs(P, S, F, g, dev)
    pre = []
    with torch.no_grad():
        import torch_twins as T
        T.nerf_forward(copy.deepcopy(m).double(), vox.double(), x.double(), pre)
    near = _branch_points(pre, P)
    frac = float(near.double().mean())
    assert int(near.sum()) <= max(1e-3 * P, 2), (F, S, vda, P, int(near.sum()))     # (at P ~ 1000, one point is already 1e-3)
    g_raw[0, near] = 0.0
    hip = _hip_mlp(lib, m, vox, x, g_raw)
    ref, scales = _twin_mlp(m, vox, x, g_raw)
    t32, _ = _twin_mlp(m, vox, x, g_raw, torch.float32)
    worst, worst_k, worst_e = 0.0, "", (0.0, 0.0)
    for k, r in ref.items():
        h = hip[k]
        assert h is not None and h.shape == r.shape, k
        scale = scales[k]
        if scale == 0.0:
            assert float(h.abs().max()) == 0.0, (F, S, vda, P, k)
            continue
        err = float((h.double() - r).abs().max()) / scale
        # (+ four times torch fp32's own distance: where a tensor is a cancelled difference — agg_w_fc's weight gradient at P = 1,
        # 1.6e-5 in torch fp32 too — no fp32 evaluation gets within tau; elsewhere that term is ~1e-7)
        bound = MLP_TAU + 4.0 * float((t32[k].double() - r).abs().max()) / scale
        if err / bound > worst:
            worst, worst_k, worst_e = err / bound, k, (err, bound)
        assert err <= bound, f"F={F} S={S} vda={vda} P={P}: {k} rel err {err:.3e} > {bound:.3e}"
    tpw, waves = _tiles_per_wave(lib, P)
    msg = (f"[mlp] F={F} S={S} vda={int(vda)} {regime}: P={P} waves={waves} tiles/wave={tpw} masked={int(near.sum())}/{P} "
           f"({frac:.1e}) tau={MLP_TAU:.0e}; closest to its bound: {worst_k} err {worst_e[0]:.2e} of {worst_e[1]:.2e}")
    if sensitivity:
        # the bound catches one dropped 16-point tile (a wave's second or later pass): the fp64 reference without it moves some
        # parameter gradient by more than 10 tau
        t = waves + 1 if -(-P // 16) > waves + 1 else 0
        g2 = g_raw.clone()
        g2[0, t * 16:(t + 1) * 16] = 0.0
        ref2, _ = _twin_mlp(m, vox, x, g2)
        moved = max(float((ref2[n] - ref[n]).abs().max()) / scales[n] for n, _ in m.named_parameters() if scales[n] > 0)
        assert moved > 10 * MLP_TAU, (F, S, vda, moved)
        msg += f" sensitivity: tile {t} dropped moves a parameter gradient by {moved:.2e} = {moved / MLP_TAU:.0f} tau"
    print(msg)
    return tpw, waves


def _check_tile_position_invariance(lib, dev, F, S, vda, P0, prefix, suffix, seed):
    """The same P0 points alone (first pass) and after ``prefix`` other points (later passes of their waves): raw, g_vox and g_x
    rows bit-identical.  Both counts are multiples of 16, so every point keeps its lane."""
    assert P0 % 16 == 0 and prefix % 16 == 0
    g = torch.Generator().manual_seed(seed)
    m = _mlp_module(F, vda, dev, g)
    vox, x, g_raw = _mlp_inputs(P0 + prefix + suffix, S, F, g, dev)
    alone = _hip_mlp(lib, m, vox[:, prefix:prefix + P0], x[:, prefix:prefix + P0], g_raw[:, prefix:prefix + P0])
    full = _hip_mlp(lib, m, vox, x, g_raw)
    for k in ("raw", "g_vox", "g_x"):
        assert torch.equal(alone[k], full[k][:, prefix:prefix + P0]), (F, S, vda, k)
    _, waves = _tiles_per_wave(lib, P0 + prefix + suffix)
    first, last = prefix // 16 // waves, (prefix + P0 - 1) // 16 // waves
    assert last >= 1, (first, last)
    return first, last


# ---------------------------------------------------------------------------------------------------------------------------------
# emulator: three CUs (6 blocks, 24 waves)
EMU_CUS = 3


@pytest.mark.parametrize("F,S,vda", MLP_CASES)
def test_mlp_kernels_match_float64_in_every_regime_emulated(F, S, vda):
    from emu_lib import emu_cu_count, emu_lib
    lib = emu_lib()
    dev = torch.device("cpu")
    torch.set_num_threads(4)
    seed = 100 + 10 * F + 2 * S + int(vda)
    with emu_cu_count(lib, EMU_CUS):
        waves = int(lib.dll.enerf_nerf_mlp_bwd_chunks(1 << 20))
        assert waves == 4 * 2 * EMU_CUS
        tpw, _ = _check_mlp_case(lib, dev, F, S, vda, 1, seed, "P=1")
        assert tpw == 1
        P = 16 * (waves // 2 + 1) + 7                # 14 tiles on 16 waves: two idle
        tpw, w = _check_mlp_case(lib, dev, F, S, vda, P, seed + 1, "idle waves")
        assert tpw == 1 and -(-P // 16) < w
        P = 3 * waves * 16 - 3                       # three tiles per wave, the last one ragged
        tpw, _ = _check_mlp_case(lib, dev, F, S, vda, P, seed + 2, "3 passes", sensitivity=True)
        assert tpw == 3
        # 8 tiles that fall in the second and third passes of their waves (tiles 44..51 of 57)
        first, last = _check_tile_position_invariance(lib, dev, F, S, vda, 8 * 16, (2 * waves - 4) * 16, 16 * 5 + 3, seed + 3)
        assert (first, last) == (1, 2)


@pytest.mark.gpu
@pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")
@pytest.mark.parametrize("F,S,vda", MLP_CASES)
def test_mlp_kernels_match_float64_in_every_regime_on_gpu(F, S, vda):
    """The same on the MI355X, the float64 twin on the device: P from the CU count (2 blocks of 4 waves per CU)."""
    from enerf_amd.lib import get_lib
    lib = get_lib()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    waves = int(lib.dll.enerf_nerf_mlp_bwd_chunks(1 << 30))
    assert waves == 4 * 2 * cus
    seed = 200 + 10 * F + 2 * S + int(vda)
    tpw, _ = _check_mlp_case(lib, dev, F, S, vda, 1, seed, "P=1")
    assert tpw == 1
    P = 16 * (waves // 2 + 1) + 7
    tpw, w = _check_mlp_case(lib, dev, F, S, vda, P, seed + 1, "idle waves")
    assert tpw == 1 and -(-P // 16) < w
    P = 3 * waves * 16 - 3
    tpw, _ = _check_mlp_case(lib, dev, F, S, vda, P, seed + 2, "3 passes", sensitivity=True)
    assert tpw == 3
    first, last = _check_tile_position_invariance(lib, dev, F, S, vda, 64 * 16, (2 * waves - 32) * 16, 16 * 5 + 3, seed + 3)
    assert (first, last) == (1, 2)
