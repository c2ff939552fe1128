"""Which kernel every 3-D convolution of the cost-regularisation networks runs (csrc/conv3d.hip conv3d_route, csrc/capi.hip
cost_reg_plan), read back as text through the emulator-only export ``emu_cost_reg_routes`` — no launch, milliseconds.

* The routes of both cascade levels of the three bench workloads, at their real shapes, 256 CUs and default options, are pinned to
  what the kernel traces of the commit BEFORE the route function show (``rocprofv3 --kernel-trace`` of ten frames each:
  profiles/frame_driver_refactor_kernels_parent.csv for dtu, profiles/conv3d_route_refactor_kernels_parent_{lego,zju}.csv); each
  layer's row was identified in the table by its grid.  The test also recounts the tables, so the pinned lists cannot drift from them.
* On a small two-level shape, under every option set the parity tests use, the routes the plan predicts are the kernels the emulator's
  launch trace then shows for the actual ``enerf_cost_reg`` call, in order: the plan is what gets launched."""
import collections
import csv
import ctypes as C
import os
import re

import pytest
import torch

from enerf_amd.lib import Options, throughput_options
from emu_lib import emu_cu_count, emu_lib, emu_trace

PROFILES = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles")


def plan(in_channels, full, B, D, h, w, options=None, cus=256):
    """-> ([route of every layer in launch order], {"vol_planar": 0|1, "heads_planar": 0|1})"""
    dll = emu_lib().dll
    dll.emu_cost_reg_routes.restype = C.c_longlong
    dll.emu_cost_reg_routes.argtypes = [C.c_int] * 6 + [C.c_void_p, C.c_int, C.c_char_p, C.c_longlong]
    opt = None if options is None else C.cast(C.pointer(options), C.c_void_p)
    buf = C.create_string_buffer(4096)
    n = dll.emu_cost_reg_routes(in_channels, int(full), B, D, h, w, opt, cus, buf, len(buf))
    assert 0 < n <= len(buf)
    lines = buf.raw[:n].decode().splitlines()
    return lines[:-2], {k: int(v) for k, v in (ln.split("=") for ln in lines[-2:])}


def kernel_of(route):
    """'s1_b4g<16,4,false>' -> 'k_conv3d_s1_b4g<16,4,false>', 'conv3d<32,1,0,1,3>' -> 'k_conv3d<32,1,0,1,3>'"""
    return "k_" + route if route.startswith("conv3d<") else "k_conv3d_" + route


# bench.py make_workload: image size and cascade of each workload.  Level i's cost volume is (volume_planes[i], H * volume_scale[i],
# W * volume_scale[i]) over the channels of the FeatureNet level it warps (32 at level 0, 16 at level 1); level 1 runs the full net.
def level_shapes(name):
    from enerf_amd.config import EnerfConfig
    cfg, H, W = {"dtu": (EnerfConfig.dtu_eval(), 512, 640), "lego": (EnerfConfig(), 800, 800),
                 "zju": (EnerfConfig().with_cas(volume_planes=(32, 8), render_if=(False, True)), 1024, 1024)}[name]
    cas = cfg.cas
    return [((32, 16)[i], i != 0, 1, cas.volume_planes[i], int(H * cas.volume_scale[i]), int(W * cas.volume_scale[i])) for i in range(2)]


# conv0 conv1 conv2 conv3 conv4 [conv5 conv6 conv7] conv9 conv11 heads
PINNED = {
    "dtu": [["s1_b4g<32,4,false>", "conv3d<8,1,1,1,1>", "s1_lds<16,1,2,4>", "conv3d<16,1,1,1,3>", "conv3d<32,1,0,1,3>",
             "conv3d<32,1,2,1,1>", "t2_all<16,8,1,4>", "s1_b4g<8,4,true>"],
            ["s1_b4g<16,4,false>", "s2_lds<8>", "s1_lds<16,1,2,4>", "conv3d<16,1,1,1,3>", "wl<32,0,2>", "wl<32,1,1>", "wl<64,0,1>",
             "conv3d<64,1,2,1,1>", "t2_all<32,16,1,4>", "t2_all<16,8,1,4>", "s1_b4g<8,4,true>"]],
    "lego": [["s1_b4g<32,4,false>", "s2_lds<8>", "s1_lds<16,1,2,4>", "conv3d<16,1,1,1,3>", "conv3d<32,1,0,1,3>", "t2_all<32,16,1,4>",
              "t2_all<16,8,1,4>", "s1_b4g<8,4,true>"],
             ["s1_b4c<16,4,false>", "s2_lds<8>", "s1_lds<16,1,4,8>", "conv3d<16,1,1,1,3>", "s1_lds<32,2,2,8>", "wl<32,1,1>",
              "wl<64,0,1>", "conv3d<64,1,2,1,1>", "t2_all<32,16,1,4>", "t2_all<16,8,1,4>", "s1_b4c<8,4,true>"]],
    # both levels' conv0 and heads on b4c: 1024 and 4096 boxes are whole rounds of four blocks per CU
    "zju": [["s1_b4c<32,4,false>", "s2_lds<8>", "s1_lds<16,1,2,4>", "conv3d<16,1,1,1,3>", "conv3d<32,1,0,1,3>", "t2_all<32,16,1,4>",
             "t2_all<16,8,1,4>", "s1_b4c<8,4,true>"],
            ["s1_b4c<16,4,false>", "s2_lds<8>", "s1_lds<16,1,4,8>", "conv3d<16,2,1,2,1>", "s1_lds<32,2,2,8>", "wl<32,1,2>",
             "wl<64,0,2>", "conv3d<64,2,2,2,1>", "t2_all<32,16,1,4>", "t2_all<16,8,1,4>", "s1_b4c<8,4,true>"]],
}
TABLES = {"dtu": "frame_driver_refactor_kernels_parent.csv", "lego": "conv3d_route_refactor_kernels_parent_lego.csv",
          "zju": "conv3d_route_refactor_kernels_parent_zju.csv"}
TABLE_FRAMES = 10


def traced_conv_kernels(name):
    """The templated k_conv3d* rows of the parent's kernel table (the pack kernels are no templates), per frame."""
    n = collections.Counter()
    with open(os.path.join(PROFILES, TABLES[name])) as f:
        for row in csv.DictReader(f):
            m = re.match(r"void enerf::(k_conv3d\w*<[^>]*>)\(", row["kernel"])
            if m:
                assert int(row["calls"]) % TABLE_FRAMES == 0, row
                n[m.group(1).replace(" ", "")] += int(row["calls"]) // TABLE_FRAMES
    return n


@pytest.mark.parametrize("name", list(PINNED))
def test_bench_workload_routes_are_the_parent_traces(name):
    levels = []
    for shape, want in zip(level_shapes(name), PINNED[name]):
        got, planar = plan(*shape)
        assert got == want, (name, shape, got)
        # conv0 and the heads on the asynchronously staged kernels, conv11 on the paired transposed one: both hand-offs planar
        assert planar == {"vol_planar": 1, "heads_planar": 1}, (name, shape, planar)
        levels += got
    assert collections.Counter(kernel_of(r) for r in levels) == traced_conv_kernels(name)


def test_slot_round_rule_at_its_edges():
    """b4c against b4g on 256 CUs (boxes come in eights here): 768 boxes are one round of three blocks per CU (3 < 4: b4g), 776 .. 1024
    one round of four against two of three (4 <= 6: b4c), 1032 two rounds of four against two of three (8 > 6: b4g)."""
    for w, want in ((16 * 96, "s1_b4g"), (16 * 97, "s1_b4c"), (16 * 128, "s1_b4c"), (16 * 129, "s1_b4g")):
        got, _ = plan(16, False, 1, 4, 64, w)                               # w / 16 boxes along x, 8 along y, one along z
        assert got[0] == want + "<16,4,false>" and got[-1] == want + "<8,4,true>", (w, got)


SMALL = [(32, False, 1, 8, 8, 16), (16, True, 1, 8, 16, 32)]           # two levels; conv3d_lds_min_voxels = 1 puts them on the LDS kernels
OPTION_SETS = {
    "default": None, "throughput": throughput_options(), "global_only": Options(conv3d_global_only=1), "pk8_off": Options(conv3d_pk8=1),
    "t2_round2": Options(conv3d_t2_variant=1), "t2_all": Options(conv3d_t2_variant=2), "small_rt2ct2": Options(conv3d_small_variant=2),
    "small_ct4": Options(conv3d_small_variant=3), "small_split3": Options(conv3d_small_variant=1), "b4_round2": Options(conv3d_b4=3),
    "lds": Options(conv3d_lds_min_voxels=1), "lds_round2": Options(conv3d_lds_min_voxels=1, conv3d_b4=3, conv3d_t2_variant=1),
    "lds_pk8_all": Options(conv3d_lds_min_voxels=1, conv3d_b4=1, conv3d_pk8=2), "lds_v2": Options(conv3d_lds_min_voxels=1, conv3d_b4=1, conv3d_pk8=1),
}


@pytest.mark.parametrize("cus", [256, 1])
@pytest.mark.parametrize("tag", list(OPTION_SETS))
def test_predicted_routes_are_what_cost_reg_launches(tag, cus):
    """... and what they compute is the float64 network (the bound of test_cost_reg_routes_gpu), so every route the option sets reach
    on the emulator — b4c through the one-CU count — is checked numerically here too."""
    lib, opt = emu_lib(), OPTION_SETS[tag]
    for shape in SMALL:
        want, _ = plan(*shape, opt, cus)
        assert "none" not in want
        with emu_cu_count(lib, cus), emu_trace(lib) as rows:
            _check_cost_reg(lib, "cpu", shape, opt, tag)
        got = [re.search(r"k_conv3d\w*", r[1]).group(0) for r in rows if r[0] == "launch" and "pack" not in r[1]]
        assert got == [kernel_of(r).split("<")[0] for r in want], (tag, cus, want, got)
    if tag == "lds":           # level 1 has 8 boxes.  One CU: two rounds of four against three of three (b4c); 256 CUs: 4 > 3 slots (b4g)
        assert want[0].startswith("s1_b4c" if cus == 1 else "s1_b4g")


# ---- every route that only enerf_cost_reg reaches (the b4 / pk8 images exist in the cost-reg nets' packed weights alone), and the
# LDS-staged ones at a few boxes, executed on the GPU against the float64 network --------------------------------------------------
LDS = dict(conv3d_lds_min_voxels=1)
FEW_BOXES = [(32, False, 1, 8, 16, 32), (16, True, 1, 8, 16, 32)]      # 2 x 2 x 2 boxes of 4 x 8 x 16 output voxels, both nets
GPU_CASES = {   # tag: (shapes, options, routes some layer must take at 256 CUs)
    "global": (FEW_BOXES, {}, ["conv3d<32,1,0,1,3>", "conv3d<8,1,1,1,1>", "conv3d<16,1,1,1,3>", "conv3d<16,1,2,1,1>", "conv3d<64,1,2,1,1>", "conv3d<8,1,0,1,1>"]),
    "lds": (FEW_BOXES, LDS, ["s1_b4g<32,4,false>", "s1_b4g<16,4,false>", "s1_b4g<8,4,true>", "s2_lds<8>", "s1_lds<16,1,2,4>",
                             "s1_lds<32,2,2,8>", "t2_all<32,16,1,4>", "t2_all<16,8,1,4>"]),
    "lds_round2": (FEW_BOXES, dict(LDS, conv3d_b4=3, conv3d_t2_variant=1), ["s1_b4<32,4,false>", "s1_b4<16,4,false>", "s1_b4<8,4,true>",
                                                                            "t2_lds<16>"]),
    "lds_pk8": (FEW_BOXES, dict(LDS, conv3d_b4=1, conv3d_pk8=2), ["s1_pk8<32,4>", "s1_pk8<16,4>", "s1_pk8<8,4>"]),
    "lds_v2": (FEW_BOXES, dict(LDS, conv3d_b4=1, conv3d_pk8=1), ["s1_lds<32,1,2,4>", "s1_lds<16,1,2,4>", "s1_lds<8,1,2,4>"]),
    # 7 x 8 x 14 = 784 boxes on 256 CUs: one round of four blocks per CU against two rounds of three
    "b4c": ([(8, False, 1, 28, 64, 224)], {}, ["s1_b4c<8,4,false>", "s1_b4c<8,4,true>"]),
}


@pytest.mark.parametrize("tag", list(GPU_CASES))
def test_gpu_cases_reach_their_routes(tag):
    shapes, opt, must = GPU_CASES[tag]
    taken = set()
    for shape in shapes:
        routes, _ = plan(*shape, Options(**opt))
        assert "none" not in routes
        taken |= set(routes)
    assert set(must) <= taken, (tag, sorted(set(must) - taken), sorted(taken))


_REF = {}


def _cost_reg_case(shape):
    """-> (CostRegParams, volume (B, D, h, w, C), float64 feat (B, D, h, w, 8), float64 prob (B, D, h, w)); computed once per shape"""
    if shape not in _REF:
        from enerf_amd.network import CostRegParams
        from oracle import enerf_oracle as O
        in_channels, full, B, D, h, w = shape
        torch.manual_seed(in_channels + int(full))
        m = CostRegParams(in_channels, full).eval()
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            for k, v in m.state_dict().items():
                if k.endswith("running_mean") or (v.dim() == 1 and k.endswith("bias")):
                    v.copy_(torch.randn(v.shape, generator=g) * 0.1)
                elif k.endswith("running_var") or (v.dim() == 1 and k.endswith("weight")):
                    v.copy_(torch.rand(v.shape, generator=g) + 0.5)
        x = torch.randn((B, D, h, w, in_channels), generator=g)
        with torch.no_grad():
            feat, prob = O.cost_reg({"m." + k: v.double() for k, v in m.state_dict().items()}, "m", x.permute(0, 4, 1, 2, 3).double())
        _REF[shape] = (m, x, feat.permute(0, 2, 3, 4, 1).contiguous(), prob)
    return _REF[shape]


def _check_cost_reg(lib, dev, shape, options, tag):
    m, x, ref_feat, ref_prob = _cost_reg_case(shape)
    m = m.to(dev)
    try:
        feat, prob = lib.cost_reg(lib.cost_reg_pack(m.raw(), dev), shape[0], shape[1], x.to(dev).contiguous(), options=options)
        if dev != "cpu":
            torch.cuda.synchronize()
    finally:
        m.to("cpu")
    for name, out, ref in (("feat", feat, ref_feat), ("prob", prob, ref_prob)):
        err = float((out.cpu().double() - ref).abs().max() / ref.abs().max())
        print(tag, shape, name, f"{err:.3e}")
        assert out.shape == ref.shape and err < 2e-5, (tag, shape, name, err)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(GPU_CASES))
def test_cost_reg_routes_gpu(tag):
    """The whole cost-reg network under the case's options against the same network in float64 (oracle.cost_reg on torch's conv3d /
    conv_transpose3d), with the single-layer bound of test_conv3d_small_layers.py: max error 2e-5 of the largest reference value."""
    from enerf_amd.lib import get_lib
    shapes, opt, _ = GPU_CASES[tag]
    for shape in shapes:
        _check_cost_reg(get_lib(), "cuda:0", shape, Options(**opt), tag)
