"""The hand-written backward kernels of the geometric stages (csrc/backward.hip and the any-order and tiled paths of
csrc/gather.hip, with their forwards) against float64 autograd of the torch twins, at every launcher branch and at the shapes where
such kernels break: voxel / pixel / ray / point counts that fill no wave and no block, waves that straddle batch elements, every
channel width of the warp kernel with its neighbour merge shown on and shown off, the clamps (p.z, var, 1 / d, saturated sigma)
forced, absent upstream gradients.  The bound is four times the float32 twin's own distance from float64 plus 16 roundings
(tests/backward_cases.py), with the points whose texel cell is decided by rounding masked — 100 to 1000 times tighter than the
float32-referenced bounds of _check_hip_backward_stages (tests/test_training.py).

Measured worst hip / bound per family (the assertion is hip / bound <= 1; bound = 4 d32 + 16 * 2^-24), emulator | MI355X:
    warp              0.30 (oblique C = 16, volume: hip 3.5e-6, d32 2.7e-6)   | 0.35 (exact C = 16, volume: hip 5.6e-7, d32 1.6e-7)
    depth_regression  0.21 (D = 8, depth space, g_prob: hip 1.4e-6, d32 1.4e-6) | 0.76 (D = 96, disparity space, g_prob: hip 3.5e-6, d32 9.1e-7)
    composite         0.12 (Ns = 8, weights: hip 2.3e-7, d32 2.6e-7)          | 0.17 (Ns = 8, weights: hip 2.7e-7, d32 1.4e-7)
    gather            0.39 (S = 3, F = 4, x: hip 4.0e-6, d32 2.9e-6)          | 0.37 (raster 12x40, x: hip 8.9e-6, d32 5.8e-6)
Over all cases hip lies between 0 and 2.1e-5 of float64 (the largest: g_dv of the oblique warp case, d32 1.9e-5 .. 2.3e-5).
Every case prints its own line (hip and d32 per tensor) under ``pytest -s``."""
import functools
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import backward_cases as BC                                                           # noqa: E402
from backward_cases import CompositeCase, DepthCase, GatherCase, WarpCase            # noqa: E402


def _first(case, dev):
    return BC.yardstick(case, dev)[0]


# ---- 1. cost-volume warp + variance ---------------------------------------------------------------------------------------------
def _in_voxel_order(t):
    """(S, nvox) in the kernel's voxel order -> (B,S,D,h,w) given a (B,S,D,h,w) shape holder."""
    return lambda like: t.reshape(like.shape[1], like.shape[0], *like.shape[2:]).transpose(0, 1)


def _check_warp(lib, dev, C):
    """FeatureVolumeFn (k_build_feature_volume*, k_feature_volume_bwd<C/4>): volume, g_feats, g_dv."""
    nvw = 64 // (C // 4)                                              # voxels per wave; four waves per block
    # -- unit-step: 462 voxels, the last wave partially live (dead lanes shadow voxel nvox-1 through every shuffle); the merge is ON --
    case = WarpCase("unit", C)
    inp, r64, sc, d32 = BC.yardstick(case, dev)
    Hs, Ws = case.src
    nvox = inp["count"]
    assert nvox == 462 and nvox % nvw != 0 and nvox % (4 * nvw) != 0 and nvox > 4 * nvw
    m0, m1, outside = BC.warp_regime(inp["u"], inp["v"], Hs, Ws, C)
    share = float((m0 | m1).double().mean())
    assert share >= 0.5, share
    BC.compare(case, case.hip(lib, inp), dev, note=f" (merge share {share:.2f})")
    # sensitivity, on the reference alone: (a) the last, partially live wave's voxels dropped
    first = nvox // nvw * nvw
    g2 = inp["gout"].permute(0, 2, 3, 4, 1).reshape(nvox, C).clone()
    g2[first:] = 0
    ref = case.twin(inp, torch.float64, gout=g2.view(case.B, *case.vol, C).permute(0, 4, 1, 2, 3))
    mv_a = BC.moved(case, dev, ref, keys=("g_feats", "g_dv"))
    assert mv_a > 10, mv_a
    # (b) the merged neighbour contributions dropped: the restatement with explicit taps is the twin, then loses those taps' gradients
    ref = case.twin(inp, torch.float64, fn=BC.warp_taps_volume)
    for k in r64:
        assert BC.distance(ref[k], r64[k], sc[k]) < 1e-12, k
    keep = [_in_voxel_order(~torch.roll(m, 1, 1))(inp["u"]) for m in (m0, m1)]          # voxel j + 1's left tap rides on voxel j
    ref = case.twin(inp, torch.float64, fn=functools.partial(BC.warp_taps_volume, keep0=keep[0], keep1=keep[1]))
    assert BC.distance(ref["volume"], r64["volume"], sc["volume"]) < 1e-12
    mv_b = BC.moved(case, dev, ref, keys=("g_feats",))
    assert mv_b > 10, mv_b
    print(f"[warp] C={C} sensitivity: last wave's {nvox - first} voxels dropped moves a gradient by {mv_a:.0f} bounds, "
          f"merged contributions dropped by {mv_b:.0f} bounds")
    # -- exact-integer: the coordinates are the same exact numbers in float32 and float64 (integers; halves in v on the d = 1024 plane):
    #    the one-sided derivative at weight-0 taps, and g_dv through it; nothing masked --
    case = WarpCase("exact", C)
    inp = _first(case, dev)
    _, _, _, u32, v32 = BC.warp_coords(inp["proj"], inp["dv"], torch.float32)
    assert torch.equal(u32.double(), inp["u"]) and torch.equal(v32.double(), inp["v"])
    assert bool((inp["u"] == inp["u"].round()).all()) and bool((2 * inp["v"] == (2 * inp["v"]).round()).all())
    assert bool((inp["v"][:, :, :2] == inp["v"][:, :, :2].round()).all()) and inp["masked"] == 0
    # The reference here is the explicit-tap restatement (WarpCase.twin): the twin's own values and g_feats — continuous across a
    # texel edge — agree with it to rounding, its g_dv does not (see there).  At an exact integer the restatement differentiates in
    # the cell [x, x + 1] as ATen does when the coordinate reaches it exactly (W = 3: the grid's 0 un-normalises to exactly 1):
    r64, sc = BC.yardstick(case, dev)[1:3]
    tw = case.twin(inp, torch.float64, fn=BC.T.feature_volume)
    assert BC.distance(tw["volume"], r64["volume"], sc["volume"]) < 1e-12 and BC.distance(tw["g_feats"], r64["g_feats"], sc["g_feats"]) < 1e-12
    img = torch.tensor([[[[0.0, 1.0, 4.0]] * 3]], dtype=torch.float64)
    at = torch.zeros(1, 1, 1, 2, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.grid_sample(img, at, align_corners=True).sum().backward()
    assert float(at.grad[0, 0, 0, 0]) == 4.0 - 1.0                    # (d ix / d grid = (W - 1) / 2 = 1)
    BC.compare(case, case.hip(lib, inp), dev)
    # -- oblique: the merge is OFF, most taps outside, one view behind its 1e-6 clamp for part of the depths, one non-finite --
    case = WarpCase("oblique", C)
    inp = _first(case, dev)
    Hs, Ws = case.src
    m0, m1, outside = BC.warp_regime(inp["u"], inp["v"], Hs, Ws, C)
    share, out_share = float((m0 | m1).double().mean()), float(outside.double().mean())
    behind = float((inp["pz"][:, BC.BEHIND_VIEW] < 1e-6).double().mean())
    front_inside = int((~outside[BC.BEHIND_VIEW] & (inp["pz"][:, BC.BEHIND_VIEW] >= 1e-6).reshape(-1)).sum())
    assert share <= 0.05 and 0.1 <= out_share <= 0.9 and 0.1 <= behind < 1.0, (share, out_share, behind)
    assert front_inside > 0                                           # (the clamped view also samples the image: g_dv through d p.z)
    assert not bool((inp["u"][:, BC.NONFINITE_VIEW].abs() < 1e8).any())
    hip = case.hip(lib, inp)
    assert float(hip["g_feats"][:, BC.NONFINITE_VIEW].abs().max()) == 0.0
    BC.compare(case, hip, dev, note=f" (merge share {share:.2f}, outside {out_share:.2f}, behind {behind:.2f})")
    if C != 32:
        return
    # -- S = 2, B = 2: each batch element alone as a B = 1 launch gives the same bits (the b * S + s indexing) --
    case = WarpCase("unit_s2", C)
    inp, r64, sc, d32 = BC.yardstick(case, dev)
    full = case.hip(lib, inp)
    BC.compare(case, full, dev)
    for b in range(case.B):
        one = case.hip(lib, inp, b)
        assert torch.equal(one["volume"][0], full["volume"][b]) and torch.equal(one["g_dv"][0], full["g_dv"][b]), b
        err = BC.distance(one["g_feats"][0], r64["g_feats"][b], sc["g_feats"])        # (atomics: any order of the sums)
        assert err <= BC.bounds(d32)["g_feats"], (b, err)


# ---- 2. depth regression --------------------------------------------------------------------------------------------------------
def _depth_kernel(D):
    return "k_depth_regression_bwd<4>" if D <= 16 else "k_depth_regression_bwd<16>" if D <= 64 else "k_depth_regression_bwd_serial"


def _check_depth(lib, dev, D):
    """DepthRegressionFn (k_depth_regression, k_depth_regression_bwd<4> / <16> / _serial): depth, std, g_prob, g_dv."""
    for inv in (True, False):
        case = DepthCase(D, inv)
        inp = _first(case, dev)
        assert inp["count"] == 42 and case.h * case.w % 16 != 0           # a partial third wave, the second straddles the batch elements
        BC.compare(case, case.hip(lib, inp), dev)
    if D == 17:             # sensitivity: plane D - 1 (the only plane of the <16> kernel's second round at D = 17) dropped
        ref = case.twin(inp, torch.float64, planes=D - 1)
        for k in ("g_prob", "g_dv"):
            ref[k] = torch.cat([ref[k], torch.zeros_like(ref[k][:, :1])], 1)
        mv = BC.moved(case, dev, ref)
        assert mv > 10, mv
        print(f"[depth_regression] D={D} sensitivity: plane {D - 1} dropped moves an output by {mv:.0f} bounds")


def _check_depth_extremes(lib, dev):
    """The var < 1e-10 clamp (an exactly one-hot softmax) and the d < 1e-6 clamp of 1 / max(d, 1e-6), on both register kernels."""
    floor_std = float(torch.tensor(1e-10, dtype=torch.float32).sqrt())
    for D in (8, 48):
        for inv in (True, False):
            case = DepthCase(D, inv, "onehot")
            inp = _first(case, dev)
            hip = case.hip(lib, inp)
            assert bool((hip["std"].cpu() == floor_std).all())
            still = case.hip(lib, inp, g_std=torch.zeros_like(inp["g_std"]))      # the std path contributes exactly nothing
            assert torch.equal(still["g_prob"], hip["g_prob"]) and torch.equal(still["g_dv"], hip["g_dv"])
            BC.compare(case, hip, dev)
        case = DepthCase(D, True, "clamped")
        inp = _first(case, dev)
        share = float(inp["clamped"].double().mean())
        assert 0.05 <= share <= 0.2, share
        hip = case.hip(lib, inp)
        assert float(hip["g_dv"][inp["clamped"]].abs().max()) == 0.0
        BC.compare(case, hip, dev, note=f" ({share:.2f} of the depths clamped)")


# ---- 3. compositing -------------------------------------------------------------------------------------------------------------
def _check_composite(lib, dev, Ns):
    """CompositeFn / lib.composite_bwd (k_composite_fwd, k_composite_bwd): rgb, depth, weights, g_raw, g_z at n = 300 rays."""
    case = CompositeCase(Ns)
    inp = _first(case, dev)
    assert inp["count"] == 300 and 256 < inp["count"] < 512                # two blocks, the second ragged
    BC.compare(case, case.hip(lib, inp), dev)
    if Ns == 5:              # sensitivity: the last ray dropped
        mv = BC.moved(case, dev, case.twin(inp, torch.float64, rays=inp["count"] - 1), keys=("g_raw", "g_z"))
        assert mv > 10, mv
        print(f"[composite] Ns={Ns} sensitivity: the last ray dropped moves a gradient by {mv:.0f} bounds")


def _check_composite_edges(lib, dev):
    """n = 1; absent upstream gradients (NULL pointers) equal zeros bit for bit; n = 0 touches nothing."""
    from enerf_amd.lib import _ptr
    case = CompositeCase(3, n=1)
    BC.compare(case, case.hip(lib, _first(case, dev)), dev)
    case = CompositeCase(5)
    raw, z, gr, gd, gw = case.flat(_first(case, dev))
    grads = (gr, gd, gw)
    for absent in range(1, 8):
        with_none = lib.composite_bwd(raw, z, *[None if absent >> i & 1 else g for i, g in enumerate(grads)])
        with_zero = lib.composite_bwd(raw, z, *[torch.zeros_like(g) if absent >> i & 1 else g for i, g in enumerate(grads)])
        assert torch.equal(with_none[0], with_zero[0]) and torch.equal(with_none[1], with_zero[1]), absent
    assert float(lib.composite_bwd(raw, z, None, None, None)[0].abs().max()) == 0.0
    outs = [torch.full(s, 7.0, device=dev) for s in ((4, 3), (4,), (4, 5), (4, 5, 4), (4, 5))]      # rgb, depth, weights, g_raw, g_z
    st = lib.stream_of(raw)
    lib._check(lib.dll.enerf_composite(_ptr(raw), _ptr(z), 0, 5, 0, _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), st), "composite")
    lib._check(lib.dll.enerf_composite_bwd(_ptr(raw), _ptr(z), _ptr(gr), _ptr(gd), _ptr(gw), 0, 5, _ptr(outs[3]), _ptr(outs[4]), st),
               "composite_bwd")
    assert all(bool((o == 7.0).all()) for o in outs)


# ---- 4. render-side gather ------------------------------------------------------------------------------------------------------
def _check_gather_any(lib, dev, S, Fc):
    """GatherFn without raster hints (k_gather_fwd_w<1> / <3> / k_gather_fwd, k_gather_bwd): x, vox, g_xyz, g_dn, g_tex, g_vol."""
    case = GatherCase(S, Fc)
    inp = _first(case, dev)
    assert inp["count"] * S % 16 != 0                                  # the last block's trailing 16-lane groups are dead
    BC.compare(case, case.hip(lib, inp), dev)
    if (S, Fc) == (3, 17):   # sensitivity: the last 16-lane group — the last point's last view — dropped
        gx = inp["g_x"].clone()
        assert float(gx[-1, -1, S - 1].abs().max()) > 0
        gx[-1, -1, S - 1] = 0
        mv = BC.moved(case, dev, case.twin(inp, torch.float64, g_x=gx), keys=("g_tex", "g_xyz"))
        assert mv > 10, mv
        print(f"[gather] S={S} F={Fc} sensitivity: the last 16-lane group dropped moves a gradient by {mv:.0f} bounds")


def _check_gather_raster(lib, dev, which):
    """Row-major full-image rays: enerf_gather_bwd without the raster hints (k_gather_bwd) and with them (k_gather_bwd_tiled<1, true>
    at F = 11, <3, false> at F = 35), each against float64."""
    Hr, Wr, Ns, Fc, S = BC.GATHER_RASTER[which]
    case = GatherCase(S, Fc, raster=(Hr, Wr, Ns))
    inp = _first(case, dev)
    BC.compare(case, case.hip(lib, inp), dev, note=" without hints")
    BC.compare(case, case.hip(lib, inp, hints=True), dev, note=" with n_samples / ray_w")


# ---------------------------------------------------------------------------------------------------------------------------------
CPU = torch.device("cpu")


def _emu():
    from emu_lib import emu_lib
    torch.set_num_threads(4)
    return emu_lib()


def _launches(lib, fn):
    from emu_lib import emu_trace
    with emu_trace(lib) as tr:
        fn()
    return [e[1] for e in tr if e[0] == "launch"]


@pytest.mark.parametrize("C", (8, 16, 32))
def test_warp_kernels_match_float64_emulated(C):
    _check_warp(_emu(), CPU, C)


@pytest.mark.parametrize("D", BC.DEPTH_PLANES)
def test_depth_regression_kernels_match_float64_emulated(D):
    lib = _emu()
    _check_depth(lib, CPU, D)
    case = DepthCase(D, True)
    names = _launches(lib, lambda: case.hip(lib, _first(case, CPU)))
    assert any(_depth_kernel(D) in n for n in names), (D, names)          # the launcher branch this D is listed for


def test_depth_regression_clamps_emulated():
    _check_depth_extremes(_emu(), CPU)


@pytest.mark.parametrize("Ns", range(1, 9))
def test_composite_kernels_match_float64_emulated(Ns):
    _check_composite(_emu(), CPU, Ns)


def test_composite_edges_emulated():
    _check_composite_edges(_emu(), CPU)


@pytest.mark.parametrize("S,Fc", BC.GATHER_ANY)
def test_gather_any_order_matches_float64_emulated(S, Fc):
    lib = _emu()
    _check_gather_any(lib, CPU, S, Fc)
    case = GatherCase(S, Fc)
    names = _launches(lib, lambda: case.hip(lib, _first(case, CPU)))
    fwd = "k_gather_fwd_w<1>" if Fc <= 16 else "k_gather_fwd_w<3>" if Fc <= 48 else "k_gather_fwd"
    assert any(n.strip("()") == fwd for n in names) and any(n.strip("()") == "k_gather_bwd" for n in names), names


@pytest.mark.parametrize("which", range(len(BC.GATHER_RASTER)))
def test_gather_raster_form_matches_float64_emulated(which):
    lib = _emu()
    _check_gather_raster(lib, CPU, which)
    Hr, Wr, Ns, Fc, S = BC.GATHER_RASTER[which]
    case = GatherCase(S, Fc, raster=(Hr, Wr, Ns))
    tiled = "k_gather_bwd_tiled<1, true>" if Fc <= 16 else "k_gather_bwd_tiled<3, false>"
    assert any(tiled in n for n in _launches(lib, lambda: case.hip(lib, _first(case, CPU), hints=True)))
    assert not any("tiled" in n for n in _launches(lib, lambda: case.hip(lib, _first(case, CPU))))


def _gpu():
    from enerf_amd.lib import get_lib
    return get_lib(), torch.device("cuda:0")


gpu = lambda f: pytest.mark.gpu(pytest.mark.skipif(not torch.cuda.is_available(), reason="needs a GPU")(f))


@gpu
@pytest.mark.parametrize("C", (8, 16, 32))
def test_warp_kernels_match_float64_on_gpu(C):
    _check_warp(*_gpu(), C)


@gpu
@pytest.mark.parametrize("D", BC.DEPTH_PLANES)
def test_depth_regression_kernels_match_float64_on_gpu(D):
    _check_depth(*_gpu(), D)


@gpu
def test_depth_regression_clamps_on_gpu():
    _check_depth_extremes(*_gpu())


@gpu
@pytest.mark.parametrize("Ns", range(1, 9))
def test_composite_kernels_match_float64_on_gpu(Ns):
    _check_composite(*_gpu(), Ns)


@gpu
def test_composite_edges_on_gpu():
    _check_composite_edges(*_gpu())


@gpu
@pytest.mark.parametrize("S,Fc", BC.GATHER_ANY)
def test_gather_any_order_matches_float64_on_gpu(S, Fc):
    _check_gather_any(*_gpu(), S, Fc)


@gpu
@pytest.mark.parametrize("which", range(len(BC.GATHER_RASTER)))
def test_gather_raster_form_matches_float64_on_gpu(which):
    _check_gather_raster(*_gpu(), which)
