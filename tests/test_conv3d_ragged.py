"""The box-decomposed 3-D convolution kernels (k_conv3d_s1_b4g / b4c / b4 / pk8 / s1_lds, s2_lds, t2_all, t2_lds) where a box is
cut by the volume: in-plane extents that are whole boxes plus a part, two batch elements (element 1's d = -1 halo lies next to
element 0's last plane in memory), depths that are no multiple of the box, and the channel-quad-planar hand-offs, whose batch and
quad strides differ from channels-last.

1. whole cost-regularisation networks at ragged shapes against the same network in float64 (oracle.cost_reg), every element of
   `feat` and `prob`, max|out - ref| <= 2e-5 max|ref| (the single-layer bound of test_conv3d_small_layers.py); every case first
   asserts the routes it was written for;
2. the same float64 reference, wrong in the two ways such kernels go wrong (a batch element seeing its neighbour's plane; a
   non-zero halo past the volume), differs from the true one by over 100 bounds: the check of (1) can fail;
3. single layers with a depth that is no multiple of the box, which the networks (D a multiple of 4) cannot make;
4. a B = 2 frame whose level-0 volume is 1.5 x 1.25 boxes, the warp writing quad planes for b4g at both levels.

Worst max|err| / max|ref| (the bound is 2e-5; printed by every case, `-s` shows them), emulator | MI355X:
    b4g 7.1e-7 | 7.1e-7    b4c 7.1e-7 (one CU) | 7.7e-7 (784 boxes)    b4 + t2_lds 8.1e-7 | 7.6e-7    pk8 4.4e-7 | 3.7e-7
    s1_lds as conv0 / heads 8.3e-7 | 8.3e-7    global-load kernels (default) 6.8e-7 | not run
    single layers: s1_lds 8.9e-7 | 8.9e-7, s2_lds 4.3e-7 | 4.3e-7
    frame (bound 5e-5 | 1e-4): planar 1.1e-6 | 1.0e-6, channels-last 9.5e-7 | 1.0e-6
The mutated references of (2) are 0.45 .. 0.68 of max|ref| away: 2e4 bounds.  No kernel had to change.
CPU: the kernel sources under the lane emulator, at 256 and at one CU.  GPU (`-m gpu`): the same bodies on the gfx950 build."""
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from enerf_amd.lib import Options
from emu_lib import emu_cu_count, emu_lib, emu_trace
from test_conv3d_routes import OPTION_SETS, _check_cost_reg, _cost_reg_case, kernel_of, plan

BOUND = 2e-5                                    # test_conv3d_small_layers.py, test_cost_reg_routes_gpu

# (in_channels, full, B, D, h, w).  conv0 / the heads in boxes of 4 x 8 x 16: 2 x 1.5 x 2.5 (min nets), 2 x 2 x 2.5 (the full net, whose
# h is a multiple of 8 by its own rule).  Inside: conv1 writes 4 x 6 x 20 (1.5 x 1.25 boxes of s2_lds), conv2 runs there, conv4 at
# 2 x 3 x 10, conv9 reads 2 x 3 x 10, conv11 reads 4 x 6 x 20 (4 x 8 x 20 in the full net).
RAGGED = {"min32_b2": (32, False, 2, 8, 12, 40),        # two Cin passes of 16
          "full16_b2": (16, True, 2, 8, 16, 40),
          "min8_b1": (8, False, 1, 8, 12, 40)}          # the CIN = 8 instantiation of conv0
LDS_SETS = ["lds", "lds_round2", "lds_pk8_all", "lds_v2"]

# conv0 / heads of every set: (route of conv0 over {cin}, route of the heads, output box (d, h, w), both hand-offs planar)
ENDS = {"b4g": ("s1_b4g<{cin},4,false>", "s1_b4g<8,4,true>", (4, 8, 16), 1),
        "b4c": ("s1_b4c<{cin},4,false>", "s1_b4c<8,4,true>", (4, 8, 16), 1),
        "lds_round2": ("s1_b4<{cin},4,false>", "s1_b4<8,4,true>", (4, 8, 16), 0),
        "lds_pk8_all": ("s1_pk8<{cin},4>", "s1_pk8<8,4>", (4, 8, 14), 0),
        "lds_v2": ("s1_lds<{cin},1,2,4>", "s1_lds<8,1,2,4>", (2, 4, 16), 0)}
DOWN = ["s2_lds<8>", "s1_lds<16,1,2,4>", "conv3d<16,1,1,1,3>", "s1_lds<32,2,2,8>"]                 # conv1 .. conv4
DEEP = ["wl<32,1,1>", "wl<64,0,1>", "conv3d<64,1,2,1,1>"]                                         # conv5 .. conv7 of the full net
UP = {"lds_round2": ["conv3d<32,1,2,1,1>", "t2_lds<16>"]}                                          # conv9, conv11
UP_ALL = ["t2_all<32,16,1,4>", "t2_all<16,8,1,4>"]
DEFAULT = {   # the global-load kernels volumes this small take without conv3d_lds_min_voxels
    "min32_b2": ["conv3d<32,1,0,1,3>", "conv3d<8,1,1,1,1>", "conv3d<16,1,0,1,3>", "conv3d<16,1,1,1,3>", "wl<32,0,1>", "conv3d<32,1,2,1,1>",
                 "conv3d<16,1,2,1,1>", "conv3d<8,1,0,1,1>"],
    "full16_b2": ["conv3d<16,1,0,1,3>", "conv3d<8,1,1,1,1>", "conv3d<16,1,0,1,3>", "conv3d<16,1,1,1,3>", "wl<32,0,1>", "wl<32,1,1>",
                  "wl<64,0,1>", "conv3d<64,1,2,1,1>", "conv3d<32,1,2,1,1>", "conv3d<16,1,2,1,1>", "conv3d<8,1,0,1,1>"],
    "min8_b1": ["conv3d<8,1,0,1,1>", "conv3d<8,1,1,1,1>", "conv3d<16,1,0,1,3>", "conv3d<16,1,1,1,3>", "wl<32,0,1>", "conv3d<32,1,2,1,1>",
                "conv3d<16,1,2,1,1>", "conv3d<8,1,0,1,1>"]}


def family_of(tag, cus):
    """`lds` is the asynchronously staged pair: these few boxes fill no round of four blocks per CU on 256 CUs (b4g), on one CU they
    do (b4c): test_slot_round_rule_at_its_edges."""
    return tag if tag != "lds" else ("b4c" if cus == 1 else "b4g")


def pinned_routes(case, tag, cus):
    """-> (routes in launch order, planar hand-offs, output box of conv0 / the heads or None)"""
    cin, full = RAGGED[case][:2]
    if tag == "default":
        return DEFAULT[case], 0, None
    conv0, heads, box, planar = ENDS[family_of(tag, cus)]
    return [conv0.format(cin=cin)] + DOWN + (DEEP if full else []) + UP.get(tag, UP_ALL) + [heads], planar, box


def _assert_regime(case, tag, cus):
    """The plan is the pinned one, and the dimensions themselves make conv0's and the heads' grid ragged."""
    shape = RAGGED[case]
    want, planar, box = pinned_routes(case, tag, cus)
    got, hand = plan(*shape, OPTION_SETS[tag], cus)
    assert got == want, (case, tag, cus, got)
    assert hand == {"vol_planar": planar, "heads_planar": planar}, (case, tag, cus, hand)
    if box is not None:
        h, w = shape[4:]
        ragged = [(n, b) for n, b in ((h, box[1]), (w, box[2])) if n % b]
        assert ragged and all(n > b for n, b in ragged), (case, tag, box)     # a partial box BEHIND at least one whole box
        assert (h % 8 or w % (14 if "pk8" in tag else 16)), (case, tag)
    return want


def _check_ragged(lib, dev, case, tag, cus):
    want = _assert_regime(case, tag, cus)
    if dev != "cpu":
        return _check_cost_reg(lib, dev, RAGGED[case], OPTION_SETS[tag], f"{case}/{tag}")
    with emu_cu_count(lib, cus), emu_trace(lib) as rows:
        _check_cost_reg(lib, dev, RAGGED[case], OPTION_SETS[tag], f"{case}/{tag}/{cus}")
    got = [re.search(r"k_conv3d\w*", r[1]).group(0) for r in rows if r[0] == "launch" and "pack" not in r[1]]
    assert got == [kernel_of(r).split("<")[0] for r in want], (case, tag, cus, got)


@pytest.mark.parametrize("cus", [256, 1])
@pytest.mark.parametrize("tag", LDS_SETS + ["default"])
@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_cost_reg_emulated(case, tag, cus):
    _check_ragged(emu_lib(), "cpu", case, tag, cus)


def _device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("tag", LDS_SETS)
@pytest.mark.parametrize("case", list(RAGGED))
def test_ragged_cost_reg_gpu(case, tag):
    """Planned with the device's own CU count: a device on which `lds` does not mean b4g here fails the route assertion, it does not
    run another kernel under this name."""
    from enerf_amd.lib import get_lib
    _check_ragged(get_lib(), "cuda:0", case, tag, _device_cus())


# ---- b4c where a 256-CU device takes it: 769 .. 1024 boxes are one round of four blocks per CU against two of three.  7 x 7.5 x 13.5 ->
# 7 * 8 * 14 = 784 boxes, the last box row and the last box column partial.  (The emulator reaches b4c through the one-CU count above.)
B4C_SHAPES = [(8, False, 1, 28, 60, 216), (32, False, 1, 28, 60, 216)]


@pytest.mark.parametrize("shape", B4C_SHAPES, ids=["cin8", "cin32"])
def test_b4c_ragged_case_takes_b4c_on_256_cus(shape):
    routes, hand = plan(*shape)
    assert routes[0] == f"s1_b4c<{shape[0]},4,false>" and routes[-1] == "s1_b4c<8,4,true>", routes
    assert hand == {"vol_planar": 1, "heads_planar": 1}
    D, h, w = shape[3:]
    assert D % 4 == 0 and h % 8 and w % 16 and h > 8 and w > 16
    assert 768 < (D // 4) * -(-h // 8) * -(-w // 16) <= 1024


@pytest.mark.gpu
@pytest.mark.parametrize("shape", B4C_SHAPES, ids=["cin8", "cin32"])
def test_b4c_ragged_gpu(shape):
    from enerf_amd.lib import get_lib
    cus = _device_cus()
    routes, hand = plan(*shape, None, cus)
    if not (routes[0].startswith("s1_b4c<") and routes[-1].startswith("s1_b4c<")):
        pytest.skip(f"{cus} CUs route 784 boxes to {routes[0]} / {routes[-1]}: the slot-round rule takes b4c here only at 256 CUs")
    assert hand == {"vol_planar": 1, "heads_planar": 1}
    _check_cost_reg(get_lib(), "cuda:0", shape, None, "b4c")


# ---- 2. the check can fail: float64 references that are wrong the way a box kernel goes wrong ------------------------------------
def _oracle64(m, x_cl):
    from oracle import enerf_oracle as O
    with torch.no_grad():
        feat, prob = O.cost_reg({"m." + k: v.double() for k, v in m.state_dict().items()}, "m", x_cl.permute(0, 4, 1, 2, 3).double())
    return feat.permute(0, 2, 3, 4, 1).contiguous(), prob


def _worst(a, b, ref):
    return float((a - b).abs().max() / ref.abs().max())


@pytest.mark.parametrize("case", ["min32_b2", "full16_b2"])
def test_mutated_references_are_far_from_the_true_one(case):
    """No kernel involved.  With the input draw of _cost_reg_case (unit normal) both mutations clear the margin as drawn."""
    m, x, ref_feat, ref_prob = _cost_reg_case(RAGGED[case])
    _, full, B, D, h, w = RAGGED[case]
    feat, prob = _oracle64(m, x)
    assert torch.equal(feat, ref_feat) and torch.equal(prob, ref_prob)          # the unmutated restatement is the reference itself
    # batch-halo leak: the two elements as ONE volume of depth 2 D, so that element 1's d = -1 halo is element 0's last plane
    lf, lp = _oracle64(m, x.reshape(1, B * D, h, w, -1))
    leak = max(_worst(lf.reshape(ref_feat.shape), ref_feat, ref_feat), _worst(lp.reshape(ref_prob.shape), ref_prob, ref_prob))
    # edge padding: one replicated voxel past the high h and w sides, where a partial box's halo must read zeros.  The skip
    # connections admit only extents that are multiples of 4 (8: full net), so zeros fill up to the next one; the output is cropped.
    q = 8 if full else 4
    hp, wp = -(-(h + 1) // q) * q, -(-(w + 1) // q) * q
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (0, 1, 0, 1, 0, 0), mode="replicate")
    xp = F.pad(xp, (0, wp - w - 1, 0, hp - h - 1)).permute(0, 2, 3, 4, 1)
    assert xp.shape[2:4] == (hp, wp) and torch.equal(xp[:, :, :h, :w], x) and torch.equal(xp[:, :, h, :w], x[:, :, h - 1])
    pf, pp = _oracle64(m, xp)
    pad = max(_worst(pf[:, :, :h, :w], ref_feat, ref_feat), _worst(pp[:, :, :h, :w], ref_prob, ref_prob))
    print(case, f"leak {leak:.3e} pad {pad:.3e} (margin {100 * BOUND:.1e})")
    assert leak >= 100 * BOUND and pad >= 100 * BOUND, (case, leak, pad)


# ---- 3. single layers: depths that are no multiple of the box (the networks' D is a multiple of 4), s2_lds at odd input extents -----
S1, S2 = 0, 1
LAYERS = [  # kind, cin, cout, (B, D, h, w), kernel, its output box (d, h, w)
    (S1, 16, 16, (1, 6, 12, 20), "k_conv3d_s1_lds", (2, 4, 16)),
    (S1, 16, 16, (2, 5, 12, 20), "k_conv3d_s1_lds", (2, 4, 16)),      # the partial box in depth, next to the other batch element
    (S1, 32, 32, (1, 3, 12, 20), "k_conv3d_s1_lds", (2, 8, 16)),      # two row tiles
    (S2, 8, 16, (1, 7, 18, 22), "k_conv3d_s2_lds", (2, 4, 16)),       # 4 x 9 x 11 outputs; the last input plane, row and column unread
    (S2, 8, 16, (2, 8, 12, 40), "k_conv3d_s2_lds", (2, 4, 16)),       # conv1 of the B = 2 cases above, alone
]


def _check_layer(lib, dev, kind, cin, cout, shape, kernel, box):
    """Reference and draw of test_conv3d_small_layers._run."""
    g = torch.Generator().manual_seed(cin * 131 + cout * 7 + kind)
    B, D, h, w = shape
    wt = (torch.randn((cout, cin, 3, 3, 3), generator=g) * 0.1)
    x = torch.randn((B, D, h, w, cin), generator=g)
    ref = F.conv3d(x.permute(0, 4, 1, 2, 3).double(), wt.double(), stride=2 if kind == S2 else 1, padding=1).permute(0, 2, 3, 4, 1)
    out_dims = ref.shape[1:4]
    assert any(n % b and n > b for n, b in zip(out_dims, box)), (shape, box)
    opt = Options(conv3d_lds_min_voxels=1)
    packed = lib.conv3d_layer_pack(wt.to(dev), cin, cout, kind)
    if dev == "cpu":        # the route export covers enerf_cost_reg only: what this entry launched is read off the trace
        with emu_trace(lib) as rows:
            out = lib.conv3d_layer(packed, cin, cout, kind, x, None, opt)
        launches = [(r[1], r[2]) for r in rows if r[0] == "launch"]
        assert len(launches) == 1 and kernel + "<" in launches[0][0], launches
        assert launches[0][1] == (B * int(np.prod([-(-n // b) for n, b in zip(out_dims, box)])), 1, 1), (launches, out_dims, box)
    else:
        out = lib.conv3d_layer(packed, cin, cout, kind, x.to(dev).contiguous(), None, opt)
        torch.cuda.synchronize()
    err = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
    print(kernel, cin, cout, shape, f"{err:.3e}")
    assert out.shape == ref.shape and err <= BOUND, (kind, cin, cout, shape, err)


@pytest.mark.parametrize("case", range(len(LAYERS)))
def test_ragged_layers_emulated(case):
    _check_layer(emu_lib(), "cpu", *LAYERS[case])


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(len(LAYERS)))
def test_ragged_layers_gpu(case):
    from enerf_amd.lib import get_lib
    _check_layer(get_lib(), "cuda:0", *LAYERS[case])


# ---- 4. the planar hand-off inside a frame: 96 x 160, level-0 volume 8 x 12 x 20 (1.5 x 1.25 boxes), level 1 8 x 48 x 80 ----------------
FRAME_OPTIONS = {"planar": dict(conv3d_lds_min_voxels=1),                                            # warp -> quad planes -> b4g
                 "channels_last": dict(conv3d_lds_min_voxels=1, conv3d_b4=3, conv3d_t2_variant=1)}   # b4 + t2_lds end to end
_FRAME = {}


def _frame_case(B):
    """-> (config, batch of CPU tensors, oracle outputs); computed once per B"""
    if B not in _FRAME:
        from enerf_amd.config import EnerfConfig
        from enerf_amd.synth import make_batch
        from golden_cases import load_weights
        from oracle import enerf_oracle as O
        cfg = EnerfConfig().with_cas(volume_planes=(8, 8), render_if=(True, True))
        batch = {k: torch.from_numpy(v) for k, v in make_batch(96, 160, 3, cfg, seed=11, B=B, textured=True).items()}
        with torch.no_grad():
            ref = O.forward(cfg, load_weights(), batch)
        assert int(96 * cfg.cas.volume_scale[0]) == 12 and int(160 * cfg.cas.volume_scale[0]) == 20
        _FRAME[B] = (cfg, batch, ref)
    return _FRAME[B]


def _check_frame(net, dev, B, variant, tol, psnr_db=None):
    from oracle import enerf_oracle as O
    cfg, batch, ref = _frame_case(B)
    net.options = Options(**FRAME_OPTIONS[variant])
    out = net({k: v.to(dev) for k, v in batch.items()})
    if dev != "cpu":
        torch.cuda.synchronize()
    assert sorted(out) == sorted(ref)
    for k in ref:
        a, r = out[k].cpu().double(), ref[k].double()
        err = float((a - r).abs().max() / max(float(r.abs().max()), 1e-12))
        print("frame", B, variant, k, f"{err:.3e}")
        assert a.shape == r.shape and err < tol, (variant, k, err)
    if psnr_db is not None:
        assert O.psnr(out["rgb_level1"].cpu(), ref["rgb_level1"]) > psnr_db


def _frame_net(cfg, lib=None):
    from enerf_amd.network import Network
    from golden_cases import load_weights
    net = Network(cfg, lib=lib).eval() if lib is not None else Network(cfg)
    net.load_state_dict(load_weights(), strict=False)
    return net


@pytest.mark.parametrize("variant", list(FRAME_OPTIONS))
def test_ragged_frame_emulated(variant):
    """5e-5 of max|ref|: the bound of test_batch2_ragged_rays_and_white_bkgd."""
    B = 2
    lib, opt = emu_lib(), Options(**FRAME_OPTIONS[variant])
    planar = int(variant == "planar")
    for shape in ((32, False, B, 8, 12, 20), (16, True, B, 8, 48, 80)):
        assert plan(*shape, opt)[1] == {"vol_planar": planar, "heads_planar": planar}, shape
    with emu_trace(lib) as rows:
        _check_frame(_frame_net(_frame_case(B)[0], lib), "cpu", B, variant, 5e-5)
    conv = [re.search(r"k_conv3d\w*", r[1]).group(0) for r in rows if r[0] == "launch" and "k_conv3d" in r[1] and "pack" not in r[1]]
    want = [kernel_of(r).split("<")[0] for shape in ((32, False, B, 8, 12, 20), (16, True, B, 8, 48, 80)) for r in plan(*shape, opt)[0]]
    assert conv == want, (variant, conv)
    assert conv.count("k_conv3d_s1_b4g") == (4 if planar else 0) and conv.count("k_conv3d_s1_b4") == (0 if planar else 4)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(FRAME_OPTIONS))
def test_ragged_frame_gpu(variant):
    """REL_TOL and the 70 dB of test_gpu_parity.py."""
    from test_gpu_parity import REL_TOL
    net = _frame_net(_frame_case(2)[0]).to("cuda:0").eval()
    _check_frame(net, "cuda:0", 2, variant, REL_TOL, psnr_db=70.0)
