"""The fused heads of a cost-regularisation network without their feature output (`enerf_cost_reg_prob`; in a frame: every cascade
level that is not rendered, whose 8-channel feature volume nobody reads).  With a null feature pointer the batched-4x4 heads kernels
(k_conv3d_s1_b4 / b4g / b4c) skip the feature MFMAs and stores and keep the depth head's FMA chain as it is, so

1. `prob` of `enerf_cost_reg_prob` EQUALS `prob` of `enerf_cost_reg` bit for bit — min net on 32 channels and full net on 16, at whole
   boxes (1, 8, 8, 16) and at boxes cut in h and w with two batch elements (2, 8, 24, 40), on each of the three kernels (b4c, which
   no plan takes for two boxes: whole boxes at (1, 8, 16, 32));
2. where the heads run on another kernel the entry is an error, not a wild store;
3. a 32 x 64, S = 3 frame with render_if (False, True) equals, output by output, the same frame with `heads_keep_feat = 1` (the
   feature volume computed and stored as before), and asks for exactly level 0's feature volume less workspace.

CPU: the kernel sources under the lane emulator (b4c through a one-CU plan).  GPU (`-m gpu`): the gfx950 build; b4c at the 784-box
shape of test_conv3d_ragged.py, which a 256-CU device routes there."""
import re

import pytest
import torch

from enerf_amd.lib import EnerfError, Options
from emu_lib import emu_cu_count, emu_lib, emu_trace
from test_conv3d_routes import _cost_reg_case, kernel_of, plan

NETS = {"min32": (32, False), "full16": (16, True)}
SHAPES = {"whole": (1, 8, 8, 16), "cut": (2, 8, 24, 40)}          # boxes of 4 x 8 x 16: 2 x 1 x 1 whole; 2 x 3 x 2.5 per batch element
# kernel of the heads: (options, CU count of the plan)
KERNELS = {"b4": (dict(conv3d_lds_min_voxels=1, conv3d_b4=3), 256),
           "b4g": (dict(conv3d_lds_min_voxels=1), 256),
           "b4c": (dict(conv3d_lds_min_voxels=1), 1)}               # few boxes: a whole round of four per CU only on one CU
# ... and even one CU takes b4g for the two boxes of (1, 8, 8, 16) (conv3d.hip route_b4: 4 slots against 3): b4c's whole-box case is
# 2 x 2 x 2 boxes
WHOLE_B4C = (1, 8, 16, 32)


def _dims(dims, kernel):
    return WHOLE_B4C if (dims, kernel) == ("whole", "b4c") else SHAPES[dims]


def _check_prob_only(lib, dev, shape, options, want_heads, cus=None):
    routes = plan(*shape, options, cus)[0] if cus is not None else None
    if routes is not None:
        assert routes[-1] == want_heads, (shape, routes)
    m, x, _, _ = _cost_reg_case(shape)
    m = m.to(dev)
    try:
        packed = lib.cost_reg_pack(m.raw(), dev)
        xd = x.to(dev).contiguous()
        feat, prob = lib.cost_reg(packed, shape[0], shape[1], xd, options=options)
        only = torch.full_like(prob, float("nan"))
        lib.cost_reg_prob(packed, shape[0], shape[1], xd, options=options, out=only)
        if dev != "cpu":
            torch.cuda.synchronize()
    finally:
        m.to("cpu")
    assert bool(feat.isfinite().all()) and bool(prob.isfinite().all())
    assert torch.equal(only, prob), (shape, want_heads, float((only - prob).abs().max()))


@pytest.mark.parametrize("kernel", list(KERNELS))
@pytest.mark.parametrize("dims", list(SHAPES))
@pytest.mark.parametrize("net", list(NETS))
def test_prob_only_equals_cost_reg_prob_emulated(net, dims, kernel):
    lib = emu_lib()
    opt, cus = KERNELS[kernel]
    shape = NETS[net] + _dims(dims, kernel)
    with emu_cu_count(lib, cus), emu_trace(lib) as rows:
        _check_prob_only(lib, "cpu", shape, Options(**opt), f"s1_{kernel}<8,4,true>", cus)
    conv = [re.search(r"k_conv3d\w*", r[1]).group(0) for r in rows if r[0] == "launch" and "k_conv3d" in r[1] and "pack" not in r[1]]
    n = len(conv) // 2                                                  # cost_reg, then cost_reg_prob: the same launches
    assert conv[:n] == conv[n:] == [kernel_of(r).split("<")[0] for r in plan(*shape, Options(**opt), cus)[0]], conv
    assert conv[-1] == f"k_conv3d_s1_{kernel}"


def test_prob_only_is_an_error_where_the_heads_run_on_another_kernel():
    """(1, 8, 8, 16) is below conv3d_lds_min_voxels: the global-load kernel; and the tap-packed / plain LDS kernels with b4 off."""
    lib = emu_lib()
    shape = NETS["min32"] + SHAPES["whole"]
    m, x, _, _ = _cost_reg_case(shape)
    packed = lib.cost_reg_pack(m.raw(), "cpu")
    for opt in (None, Options(conv3d_lds_min_voxels=1, conv3d_b4=1), Options(conv3d_lds_min_voxels=1, conv3d_b4=1, conv3d_pk8=1)):
        assert not plan(*shape, opt)[0][-1].startswith("s1_b4")
        with emu_trace(lib) as rows, pytest.raises(EnerfError, match="cannot skip the feature output"):
            lib.cost_reg_prob(packed, shape[0], shape[1], x, options=opt)
        assert not [r for r in rows if r[0] == "launch"]


def _device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["b4", "b4g"])
@pytest.mark.parametrize("dims", list(SHAPES))
@pytest.mark.parametrize("net", list(NETS))
def test_prob_only_equals_cost_reg_prob_gpu(net, dims, kernel):
    from enerf_amd.lib import get_lib
    _check_prob_only(get_lib(), "cuda:0", NETS[net] + SHAPES[dims], Options(**KERNELS[kernel][0]), f"s1_{kernel}<8,4,true>", _device_cus())


@pytest.mark.gpu
def test_prob_only_equals_cost_reg_prob_gpu_b4c():
    """7 x 7.5 x 13.5 boxes = 784: one round of four blocks per CU on 256 CUs, the last box row and column cut."""
    from enerf_amd.lib import get_lib
    shape, cus = (32, False, 1, 28, 60, 216), _device_cus()
    if plan(*shape, None, cus)[0][-1] != "s1_b4c<8,4,true>":
        pytest.skip(f"{cus} CUs route 784 boxes to {plan(*shape, None, cus)[0][-1]}: the slot-round rule takes b4c here only at 256 CUs")
    _check_prob_only(get_lib(), "cuda:0", shape, None, "s1_b4c<8,4,true>", cus)


# ---- 3. the frame ---------------------------------------------------------------------------------------------------------------
LDS = dict(conv3d_lds_min_voxels=1)                                  # level 0 is 8 x 4 x 8 voxels here: b4g only with the threshold down


def _frame_pair(fr, key):
    """-> ((outputs, trace, workspace bytes) without level 0's feature volume, the same with it)"""
    got = []
    for opt in (Options(**LDS), Options(heads_keep_feat=1, **LDS)):
        out, tr = fr.run(opt)
        got.append((out, tr, fr.net._frame_state(key)["need"]))
    return got


def _check_frame_pair(pair, cfg):
    from test_frame_driver import H, W, _launches, _same
    (out, tr, need), (ref, tr_ref, need_ref) = pair
    _same(out, ref)
    D, h, w = cfg.cas.volume_planes[0], int(H * cfg.cas.volume_scale[0]), int(W * cfg.cas.volume_scale[0])
    assert (D * h * w * 8) % 64 == 0                                   # (a workspace slot is rounded up to 64 floats)
    assert need_ref - need == D * h * w * 8 * 4, (need, need_ref)
    b4g = [tr[i][2] for i in _launches(tr, "k_conv3d_s1_b4g")]          # conv0 and the heads of both levels: the same launches
    assert len(b4g) == 4 and b4g == [tr_ref[i][2] for i in _launches(tr_ref, "k_conv3d_s1_b4g")]


@pytest.mark.parametrize("way", ["plain", "cached"])
def test_frame_without_level0_feature_volume_equals_frame_with_it_emulated(way):
    from test_frame_driver import Frame
    from test_source_cache import CFG_DEFAULT
    assert tuple(CFG_DEFAULT.cas.render_if) == (False, True)
    fr = Frame(CFG_DEFAULT, False, way)
    _check_frame_pair(_frame_pair(fr, 0 if way == "plain" else (0, "cached")), CFG_DEFAULT)


def test_rendered_levels_keep_their_feature_volume():
    """Both levels rendered: the option changes nothing, not even the workspace."""
    from test_frame_driver import Frame, _same
    from test_source_cache import CFG_BOTH
    (out, _, need), (ref, _, need_ref) = _frame_pair(Frame(CFG_BOTH, False, "plain"), 0)
    _same(out, ref)
    assert need == need_ref


@pytest.mark.gpu
def test_frame_without_level0_feature_volume_equals_frame_with_it_gpu():
    import __graft_entry__ as G
    from enerf_amd.synth import make_batch
    from test_frame_driver import H, W, S
    from test_source_cache import CFG_DEFAULT
    dev = torch.device("cuda:0")
    net = G._seeded_network(CFG_DEFAULT, dev)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in make_batch(H, W, S, CFG_DEFAULT, seed=3, textured=True).items()}
    outs, needs = [], []
    for opt in (Options(**LDS), Options(heads_keep_feat=1, **LDS)):
        net.options = opt
        with torch.no_grad():
            out = net(batch)
        torch.cuda.synchronize()
        outs.append({k: v.cpu() for k, v in out.items()})
        needs.append(net._frame_state(torch.cuda.current_stream(dev).cuda_stream)["need"])
    assert sorted(outs[0]) == sorted(outs[1])
    for k in outs[1]:
        assert torch.equal(outs[0][k], outs[1][k]), k
    D, h, w = CFG_DEFAULT.cas.volume_planes[0], int(H * CFG_DEFAULT.cas.volume_scale[0]), int(W * CFG_DEFAULT.cas.volume_scale[0])
    assert needs[1] - needs[0] == D * h * w * 8 * 4, needs
